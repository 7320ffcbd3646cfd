#!/usr/bin/env python3
"""CCD finetune (text image super-resolution) on MI355X:

    python train_superres.py --config Dino/configs/CCD_vision_model_SR.yaml

The reference names the task and ships no script for it; this one follows train_segment.py.  The backbone and the MLA head come
from `model.pretrain_checkpoint` (entry `model.pretrain_key`: teacher | student; tensors it lacks or holds in another shape -
segmentation.cls.* - are logged and stay at their initialisation), `model.checkpoint` resumes a {net, optimizer, iteration} file.
AdamW (the fused optimiser) under a cosine schedule; every `training.show_iters` iterations the running loss and the PSNR of the
training batches (from the loss kernel's per-image squared errors) are logged; every `training.eval_iters` the test set is scored -
mean PSNR and SSIM of forward_sr, and of the bicubic baseline beside it - appended to log_all_evaluation.txt, and the best PSNR
keeps `best_psnr.pth`.
One rank, `data_aug: False`, no `multiscales`: anything else is refused (ccd_amd/superres.py: check_config).
"""
import argparse
import logging
import os
import time

import torch
import torch.utils.data

from Dino.modules import utils
from Dino.utils.utils import Config, Logger
from ccd_amd import superres as su
from ccd_amd.parallel import DataParallel


def make_loader(config, phase):
    """phase: 'train' | 'test' -> DataLoader of (lr fp32 [B, 3, 16, 64], hr fp32 [B, 3, 32, 128]), or None (test without data)."""
    train = phase == "train"
    section = getattr(config, f"dataset_{phase}") or {}
    bs = int(section.get("batch_size") or 64)
    if config.dataset_scheme == "synthetic":
        n = int(config.dataset_synthetic_samples or 32 * bs) if train else int(config.dataset_synthetic_test_samples or 2 * bs)
        ds = su.SyntheticPairSet(n, seed=int(config.seed or 0) + (0 if train else 7919))
        workers = 0
    else:
        roots = section.get("roots") or []
        if not roots:
            if train:
                raise ValueError("dataset.scheme superres_pair needs dataset.train.roots (TextZoom LMDBs)")
            return None
        from train import _lmdb_dirs
        parts = [su.PairDataset(p) for p in _lmdb_dirs(roots)]
        ds = parts[0] if len(parts) == 1 else torch.utils.data.ConcatDataset(parts)
        workers = int(config.dataset_num_workers or 0)
    return torch.utils.data.DataLoader(ds, batch_size=bs, shuffle=train, num_workers=workers, collate_fn=su.collate,
                                       pin_memory=bool(config.dataset_pin_memory), drop_last=train)


def report_line(res):
    return (f"PSNR: {res['psnr']:.3f} dB  SSIM: {res['ssim']:.4f}   bicubic PSNR: {res['bicubic_psnr']:.3f} dB  "
            f"bicubic SSIM: {res['bicubic_ssim']:.4f}  ({res['n_images']} images)")


def evaluate_round(model, loader, device, optimizer, iteration, out_dir, best):
    res = su.evaluate(model, loader, device)
    line = report_line(res)
    with open(os.path.join(out_dir, "log_all_evaluation.txt"), "a") as log:
        log.write("-" * 80 + "\n" + f"iteration: {iteration} \n" + line + "\n")
    logging.info(f"iteration: {iteration} eval {line}")
    psnr = res["psnr"]
    if psnr == psnr and psnr >= best:                    # (>=: a tie keeps the later checkpoint, as best_accuracy.pth does)
        torch.save({"net": model.state_dict(), "optimizer": optimizer.state_dict(), "iteration": iteration},
                   os.path.join(out_dir, "best_psnr.pth"))
        best = psnr
    return res, best


def main(config):
    world = int(os.environ.get("WORLD_SIZE", 1))
    key = su.check_config(config, world)
    torch.cuda.set_device(0)
    device = torch.device("cuda", 0)
    utils.fix_random_seeds(int(config.global_seed or config.seed or 0))
    model = DataParallel(su.build_model(config, device))     # `module.` key prefix, the layout of the other checkpoints
    if config.model_pretrain_checkpoint and os.path.isfile(config.model_pretrain_checkpoint):
        logging.info(f"Read pretrain vision model from {config.model_pretrain_checkpoint} ({key}).")
        su.load_pretrained(model, torch.load(config.model_pretrain_checkpoint, map_location="cpu", weights_only=False), key)
    if config.model_checkpoint and os.path.isfile(config.model_checkpoint):
        logging.info(f"Read vision model from {config.model_checkpoint}.")
        model.load_state_dict(torch.load(config.model_checkpoint, map_location="cpu", weights_only=False)["net"])
    model.module.ensure_arena()
    loader, test_loader = make_loader(config, "train"), make_loader(config, "test")
    if config.optimizer != "adamw":
        raise NotImplementedError("super-resolution finetuning uses adamw; only the fused AdamW is implemented")
    optimizer = su.make_optimizer(model, lr=config.lr, weight_decay=config.weight_decay, clip_grad=config.clip_grad)
    lr_schedule = utils.cosine_scheduler(config.lr, config.min_lr, config.training_epochs, len(loader), warmup_epochs=config.warmup_epochs)
    to_restore = {"iteration": 0}
    if config.model_checkpoint:
        utils.restart_from_checkpoint(config.model_checkpoint, run_variables=to_restore, optimizer=optimizer)
    iteration = int(to_restore["iteration"])
    out_dir = os.path.join(config.output_dir or "./saved_models/", config.global_name)
    os.makedirs(out_dir, exist_ok=True)
    total, it, t0 = int(config.training_epochs * len(loader)), iter(loader), time.time()
    running, mse, nrun, best, last = None, None, 0, float("-inf"), None
    while iteration < total:
        try:
            lr_images, hr_images = next(it)
        except StopIteration:
            it = iter(loader)
            lr_images, hr_images = next(it)
        loss = su.training_iteration(model, optimizer, lr_images.to(device, non_blocking=True), hr_images.to(device, non_blocking=True),
                                     lr_schedule[iteration])
        m = model.module.loss.last_mse.mean()
        running, mse = (loss, m) if running is None else (running + loss, mse + m)
        nrun += 1
        if iteration % config.training_show_iters == 0:
            psnr = -10.0 * torch.log10(mse / nrun)       # of the unclamped training output, [0, 1] images
            logging.info(f"iteration:{iteration}--> train loss:{(running / nrun).item():.6f} PSNR:{psnr.item():.3f} dB "
                         f"({(time.time() - t0):.0f} s elapsed)")
            if config.writer is not None:
                config.writer.add_scalar("metric/train_loss", (running / nrun).item(), iteration)
                config.writer.add_scalar("metric/lr", optimizer.param_groups[0]["lr"], iteration)
            running, mse, nrun = None, None, 0
        if test_loader is not None and (iteration % config.training_eval_iters == 0 or iteration == total - 1):
            last, best = evaluate_round(model, test_loader, device, optimizer, iteration, out_dir, best)
            if config.writer is not None:
                config.writer.add_scalar("metric/eval_psnr", last["psnr"], iteration)
        if iteration % config.training_save_iters == 0:
            torch.save({"net": model.state_dict(), "optimizer": optimizer.state_dict(), "iteration": iteration},
                       os.path.join(out_dir, f"{iteration}.pth"))
        iteration += 1
    torch.cuda.synchronize()
    return last


def _parse_arguments():
    parser = argparse.ArgumentParser()
    parser.add_argument("-c", "--config", type=str, required=True, help="path to config file")
    args, _ = parser.parse_known_args()
    return Config(args.config)


if __name__ == "__main__":
    from train import _ScalarLog
    config = _parse_arguments()
    Logger.init(config.global_workdir, config.global_name, config.global_phase)
    Logger.enable_file()
    logging.info(config)
    config.writer = _ScalarLog(f"./tensorboard/{config.global_name}")
    main(config)
