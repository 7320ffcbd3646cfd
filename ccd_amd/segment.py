"""Text segmentation finetuning on the MI355X-native modules: what train_segment.py, test_segment.py, tools/seg_finetune_bench.py
and the tests share - the configuration checks, the model and its optimiser, loading the backbone and the segmentation head of a
pretraining checkpoint, the datasets, one training iteration and one evaluation pass."""
from __future__ import annotations

import logging

import numpy as np
import torch

from .dataset.datasetsupervised_kmeans import MEAN, STD, ImageDatasetSelfSupervisedKmeans, resize_bilinear
from .finetune import make_optimizer          # noqa: F401  (AdamW over the arena, the model's unused parameters left alone)
from .model.dino_vision import DINO_Segment

SCHEMES = ("supervised_mask", "synthetic")
MASK_THRESHOLD = 128                          # a mask pixel of the LMDB pair is text from this grey level on


class SegmentConfig:
    """The attributes DINO_Segment reads from a Config (Dino/configs/CCD_vision_model_SEG.yaml)."""

    def __init__(self, arch="vit_small", patch_size=4, drop_path_rate=0.1, class_weight=(1.0, 1.0), ignore_index=255, dice_weight=0.0,
                 edge_weight=0.0, edge_radius=0):
        self.arch, self.patch_size, self.drop_path_rate = arch, patch_size, drop_path_rate
        self.seg_loss_class_weight, self.seg_loss_ignore_index = class_weight, ignore_index
        self.seg_loss_dice_weight, self.seg_loss_edge_weight, self.seg_loss_edge_radius = dice_weight, edge_weight, edge_radius


def check_config(config, world=1):
    """What this task deliberately does not do is refused here, with a message that says so."""
    if int(world) > 1:
        raise NotImplementedError(f"segmentation finetuning runs on one rank, got a world of {world}: the SyncBatchNorm exchange of the "
                                  "supervised path (the head's batch statistics across ranks) is not part of this task yet")
    if getattr(config, "dataset_data_aug", None):
        raise NotImplementedError("dataset.data_aug: True is not supported by segmentation finetuning: image and mask would have to be "
                                  "warped by one theta, which is follow-up work - set data_aug: False")
    if getattr(config, "dataset_multiscales", None):
        raise NotImplementedError("dataset.multiscales: True is not supported by segmentation finetuning (32 x 128 inputs only)")
    scheme = getattr(config, "dataset_scheme", None)
    if scheme not in SCHEMES:
        raise NotImplementedError(f"dataset.scheme {scheme!r}: segmentation finetuning reads `supervised_mask` image / mask LMDB pairs "
                                  "(or `synthetic` seeded batches)")
    key = getattr(config, "model_pretrain_key", None) or "teacher"
    if key not in ("teacher", "student"):
        raise ValueError(f"model.pretrain_key must be 'teacher' or 'student', got {key!r}")
    return key


def build_model(config=None, device="cuda"):
    """DINO_Segment on `device` with its arena attached, in train mode."""
    model = DINO_Segment(config or SegmentConfig()).to(device)
    model.ensure_arena()
    model.train()
    return model


def load_pretrained(model, checkpoint, key="teacher"):
    """The backbone and segmentation-head entries of checkpoint[key] (a pretraining checkpoint: {student, teacher, ...} with
    `module.`-prefixed keys) -> the model (wrapped or not).  The teacher of a pretraining run has no segmentation head: its backbone
    is taken, the head comes from the student entry when the checkpoint has one.  -> the names that stayed at their initialisation."""
    dd = model.state_dict()
    wrapped = all(n.startswith("module.") for n in dd)
    sources = [checkpoint[key]] + ([checkpoint["student"]] if key != "student" and "student" in checkpoint else [])
    picked, missing = {}, []
    for name, value in dd.items():
        bare = name[len("module."):] if wrapped else name
        for src in sources:
            hit = src.get("module." + bare, src.get(bare))
            if hit is not None and (src is sources[0] or bare.startswith("segmentation.")):
                picked[name] = hit
                break
        else:
            picked[name] = value
            missing.append(name)
    model.load_state_dict(picked)
    logging.info(f"not in the pretraining checkpoint (kept at init): {len(missing)} tensors")
    return missing


# ------------------------------------------------------------------------------------------------ data
def normalise(image_u8):
    """uint8 [H, W, 3] -> fp32 [3, H, W], the pretraining pipeline's mean / std."""
    x = image_u8.astype(np.float32) / 255.0
    return torch.from_numpy(((x - np.array(MEAN, np.float32)) / np.array(STD, np.float32)).transpose(2, 0, 1).copy())


class MaskPairDataset(ImageDatasetSelfSupervisedKmeans):
    """(image fp32 [3, 32, 128], mask uint8 [32, 128] in {0, 1}) from an image LMDB and its mask LMDB - the records of the pretraining
    pair reader, without augmentation; a mask pixel is text from grey level 128 on (after the bilinear resize)."""

    def __init__(self, path, mask_path, img_h=32, img_w=128, is_training=True, data_portion=1.0):
        if not mask_path:
            raise ValueError("supervised_mask needs dataset.mask_path: the masks are the supervision")
        super().__init__(path=path, is_training=is_training, img_h=img_h, img_w=img_w, data_aug=False, data_portion=data_portion,
                         mask=True, mask_path=mask_path)

    def __getitem__(self, idx):
        if self.use_portion:
            idx = int(self.optional_ind[idx])
        datum = self.get(idx)
        if datum is None:
            return None
        image, mask, _ = datum
        mask = resize_bilinear(mask.astype(np.float32), self.img_h, self.img_w) >= MASK_THRESHOLD
        return normalise(resize_bilinear(image, self.img_h, self.img_w)), torch.from_numpy(mask.astype(np.uint8))


class SyntheticMaskSet(torch.utils.data.Dataset):
    """Seeded (image fp32 [3, 32, 128], mask uint8 [32, 128]) for smoke runs: a few bright rectangles or strokes on noise, the mask
    marking them - a task a head can learn in a handful of iterations."""

    def __init__(self, length, seed=0, img_h=32, img_w=128):
        self.length, self.seed, self.h, self.w = int(length), int(seed), int(img_h), int(img_w)

    def __len__(self):
        return self.length

    def __getitem__(self, i):
        rng = np.random.RandomState((self.seed * 1_000_003 + i) % (2 ** 31))
        mask = np.zeros((self.h, self.w), np.uint8)
        for _ in range(rng.randint(2, 6)):
            y, x = rng.randint(2, self.h - 8), rng.randint(2, self.w - 14)
            if rng.rand() < 0.5:                                       # a rectangle
                mask[y:y + rng.randint(4, 12), x:x + rng.randint(4, 12)] = 1
            else:                                                      # a stroke, two pixels wide
                n = rng.randint(6, 20)
                yy = np.clip(y + np.cumsum(rng.randint(-1, 2, n)), 0, self.h - 2)
                xx = np.clip(x + np.arange(n), 0, self.w - 2)
                mask[yy, xx] = mask[yy + 1, xx] = 1
        image = 0.3 * rng.standard_normal((3, self.h, self.w)).astype(np.float32) + 1.5 * mask[None].astype(np.float32) - 0.5
        return torch.from_numpy(image), torch.from_numpy(mask)


def collate(batch):
    batch = [b for b in batch if b is not None]
    return torch.stack([b[0] for b in batch]), torch.stack([b[1] for b in batch])


# ------------------------------------------------------------------------------------------------ steps
def training_iteration(model, optimizer, images, masks, lr):
    """images fp32 [B, 3, 32, 128], masks uint8 [B, 32, 128] -> the loss (a device scalar); nothing is read back."""
    for g in optimizer.param_groups:
        g["lr"] = float(lr)
    loss = model(images, masks, return_loss=True)
    optimizer.zero_grad()
    loss.backward()
    optimizer.step()
    return loss.detach()


def fore_iou(confusion):
    """Foreground IoU of a [gt, pred] confusion matrix (device tensor in, device scalar out): TP / (TP + FP + FN), eval_IOU's 1e-6."""
    c = confusion.double()
    return c[1, 1] / (c[1, 1] + c[0, 1] + c[1, 0] + 1e-6)


@torch.no_grad()
def evaluate(model, loader, device):
    """One SegMeter pass: the eval-mode logits of every batch go to SegMeter.update_logits -> the meter (its five means read back
    once, by the caller)."""
    from .metric.eval_IOU import SegMeter
    mod = model.module if hasattr(model, "module") else model
    meter = SegMeter()
    for images, masks in loader:
        meter.update_logits(mod.forward_test(images.to(device, non_blocking=True)), masks.to(device, non_blocking=True))
    return meter
