#!/usr/bin/env python3
"""Score a segmentation checkpoint of train_segment.py on MI355X:

    python test_segment.py --config Dino/configs/CCD_vision_model_SEG.yaml --checkpoint saved_models/segment_small/best_fore_iu.pth
                           [--masks DIR]

Prints the five Dino.metric.eval_IOU scores (pixel_accuracy, mean_accuracy, mean_IU, fore_IU, frequency_weighted_IU: the means over
the images, and the scores of the pooled confusion matrix) for every root of `dataset.test.roots` - for the seeded test set under
`dataset.scheme: synthetic`.  --masks DIR writes the predicted masks as 8-bit PNG files (0 / 255), one per image.
"""
import argparse
import os

import torch
import torch.utils.data

from Dino.utils.utils import Config
from ccd_amd import ops, segment as sg
from ccd_amd.parallel import DataParallel


def eval_sets(config):
    """[(name, DataLoader)]: one per test root, or the synthetic test set."""
    from train_segment import make_loader
    if config.dataset_scheme == "synthetic":
        return [("synthetic", make_loader(config, "test"))]
    from train import _lmdb_dirs
    section = config.dataset_test or {}
    out = []
    for root in _lmdb_dirs(section.get("roots") or []):
        ds = sg.MaskPairDataset(root, config.dataset_mask_path, img_h=int(config.dataset_image_height or 32),
                                img_w=int(config.dataset_image_width or 128), is_training=False)
        out.append((root, torch.utils.data.DataLoader(ds, batch_size=int(section.get("batch_size") or 64), shuffle=False,
                                                      num_workers=int(config.dataset_num_workers or 0), collate_fn=sg.collate)))
    return out


def write_masks(model, loader, device, out_dir):
    from PIL import Image
    os.makedirs(out_dir, exist_ok=True)
    k = 0
    for images, _ in loader:
        mask, _ = model.module.forward_mask(images.to(device))
        for m in (mask * 255).cpu().numpy():
            Image.fromarray(m, mode="L").save(os.path.join(out_dir, f"mask-{k + 1:09d}.png"))
            k += 1
    return k


def main(config, checkpoint, masks_dir=None):
    sg.check_config(config, int(os.environ.get("WORLD_SIZE", 1)))
    torch.cuda.set_device(0)
    device = torch.device("cuda", 0)
    model = DataParallel(sg.build_model(config, device))
    model.load_state_dict(torch.load(checkpoint, map_location="cpu", weights_only=False)["net"])
    model.module.ensure_arena()
    model.eval()
    sets = eval_sets(config)
    if not sets:
        raise ValueError("nothing to score: dataset.test.roots is empty (and dataset.scheme is not synthetic)")
    results = []
    for name, loader in sets:
        scores = sg.evaluate(model, loader, device).compute()
        results.append((name, scores))
        print(f"{name}: {scores['n_images']} images")
        for s in ops.SEG_SCORES:
            print(f"  {s:>22}: {scores[s]:.4f}   (pooled: {scores['dataset_' + s]:.4f})")
        if masks_dir:
            sub = os.path.join(masks_dir, os.path.basename(os.path.normpath(name)))
            print(f"  wrote {write_masks(model, loader, device, sub)} masks to {sub}")
    return results


if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("-c", "--config", type=str, required=True, help="path to config file")
    parser.add_argument("--checkpoint", type=str, required=True, help="a {net, ...} file of train_segment.py")
    parser.add_argument("--masks", type=str, default=None, help="directory for the predicted masks (PNG)")
    args = parser.parse_args()
    main(Config(args.config), args.checkpoint, args.masks)
