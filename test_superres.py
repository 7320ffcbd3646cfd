#!/usr/bin/env python3
"""Score a super-resolution checkpoint of train_superres.py on MI355X:

    python test_superres.py --config Dino/configs/CCD_vision_model_SR.yaml --checkpoint saved_models/superres_small/best_psnr.pth
                            [--images DIR]

Prints the mean PSNR and SSIM (Dino.metric.eval_superpixel: calculate_psnr, ssim) of forward_sr against the HR images, and of the
bicubic baseline beside them, for every root of `dataset.test.roots` - for the seeded test set under `dataset.scheme: synthetic`.
--images DIR writes the super-resolved images as 8-bit PNG files, one per image.
"""
import argparse
import os

import torch
import torch.utils.data

from Dino.utils.utils import Config
from ccd_amd import superres as su
from ccd_amd.parallel import DataParallel


def eval_sets(config):
    """[(name, DataLoader)]: one per test root, or the synthetic test set."""
    from train_superres import make_loader
    if config.dataset_scheme == "synthetic":
        return [("synthetic", make_loader(config, "test"))]
    from train import _lmdb_dirs
    section = config.dataset_test or {}
    out = []
    for root in _lmdb_dirs(section.get("roots") or []):
        out.append((root, torch.utils.data.DataLoader(su.PairDataset(root), batch_size=int(section.get("batch_size") or 64), shuffle=False,
                                                      num_workers=int(config.dataset_num_workers or 0), collate_fn=su.collate)))
    return out


def write_images(model, loader, device, out_dir):
    from PIL import Image
    os.makedirs(out_dir, exist_ok=True)
    k = 0
    for lr_images, _ in loader:
        sr = model.module.forward_sr(lr_images.to(device))
        for img in (sr * 255.0).round().to(torch.uint8).permute(0, 2, 3, 1).cpu().numpy():
            Image.fromarray(img, mode="RGB").save(os.path.join(out_dir, f"sr-{k + 1:09d}.png"))
            k += 1
    return k


def main(config, checkpoint, images_dir=None):
    su.check_config(config, int(os.environ.get("WORLD_SIZE", 1)))
    torch.cuda.set_device(0)
    device = torch.device("cuda", 0)
    model = DataParallel(su.build_model(config, device))
    model.load_state_dict(torch.load(checkpoint, map_location="cpu", weights_only=False)["net"])
    model.module.ensure_arena()
    model.eval()
    sets = eval_sets(config)
    if not sets:
        raise ValueError("nothing to score: dataset.test.roots is empty (and dataset.scheme is not synthetic)")
    results = []
    for name, loader in sets:
        res = su.evaluate(model, loader, device)
        results.append((name, res))
        print(f"{name}: {res['n_images']} images")
        print(f"  {'PSNR':>6}: {res['psnr']:.3f} dB   (bicubic: {res['bicubic_psnr']:.3f} dB)")
        print(f"  {'SSIM':>6}: {res['ssim']:.4f}      (bicubic: {res['bicubic_ssim']:.4f})")
        if images_dir:
            sub = os.path.join(images_dir, os.path.basename(os.path.normpath(name)))
            print(f"  wrote {write_images(model, loader, device, sub)} images to {sub}")
    return results


if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("-c", "--config", type=str, required=True, help="path to config file")
    parser.add_argument("--checkpoint", type=str, required=True, help="a {net, ...} file of train_superres.py")
    parser.add_argument("--images", type=str, default=None, help="directory for the super-resolved images (PNG)")
    args = parser.parse_args()
    main(Config(args.config), args.checkpoint, args.images)
