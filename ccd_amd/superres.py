"""Text image super-resolution finetuning on the MI355X-native modules: what train_superres.py, test_superres.py,
tools/superres_bench.py and the tests share - the configuration checks, the model and its optimiser, loading the backbone and the
MLA head of a pretraining checkpoint, the datasets, one training iteration and one evaluation pass.  The task is TextZoom's:
lr fp32 [N, 3, 16, 64] -> sr fp32 [N, 3, 32, 128], both in [0, 1]; no other size is taken."""
from __future__ import annotations

import io
import logging
import os

import numpy as np
import torch

from .dataset import lmdb_file
from .dataset.datasetsupervised_kmeans import resize_bilinear
from .finetune import make_optimizer          # noqa: F401  (AdamW over the arena, the model's unused parameters left alone)
from .model.dino_vision import DINO_SuperRes
from .ops import SR_HR_SIZE, SR_LR_SIZE

SCHEMES = ("superres_pair", "synthetic")


class SuperResConfig:
    """The attributes DINO_SuperRes reads from a Config (Dino/configs/CCD_vision_model_SR.yaml)."""

    def __init__(self, arch="vit_small", patch_size=4, drop_path_rate=0.1, gp_weight=1e-4, ssim_weight=0.0):
        self.arch, self.patch_size, self.drop_path_rate = arch, patch_size, drop_path_rate
        self.sr_loss_gp_weight, self.sr_loss_ssim_weight = gp_weight, ssim_weight


def check_config(config, world=1):
    """What this task deliberately does not do is refused here, with a message that says so."""
    if int(world) > 1:
        raise NotImplementedError(f"super-resolution finetuning runs on one rank, got a world of {world}: the SyncBatchNorm exchange of "
                                  "the supervised path (the head's batch statistics across ranks) is not part of this task yet")
    if getattr(config, "dataset_data_aug", None):
        raise NotImplementedError("dataset.data_aug: True is not supported by super-resolution finetuning: the LR / HR pair would have to "
                                  "be warped by one theta at two scales, which is follow-up work - set data_aug: False")
    if getattr(config, "dataset_multiscales", None):
        raise NotImplementedError("dataset.multiscales: True is not supported by super-resolution finetuning (16 x 64 -> 32 x 128 only)")
    scheme = getattr(config, "dataset_scheme", None)
    if scheme not in SCHEMES:
        raise NotImplementedError(f"dataset.scheme {scheme!r}: super-resolution finetuning reads `superres_pair` LMDBs of HR / LR image "
                                  "pairs (or `synthetic` seeded batches)")
    key = getattr(config, "model_pretrain_key", None) or "teacher"
    if key not in ("teacher", "student"):
        raise ValueError(f"model.pretrain_key must be 'teacher' or 'student', got {key!r}")
    return key


def build_model(config=None, device="cuda"):
    """DINO_SuperRes on `device` with its arena attached, in train mode."""
    model = DINO_SuperRes(config or SuperResConfig()).to(device)
    model.ensure_arena()
    model.train()
    return model


def load_pretrained(model, checkpoint, key="teacher"):
    """segment.load_pretrained's rule - the backbone of checkpoint[key], the head of the student entry - except that a tensor whose
    shape differs from the model's (segmentation.cls.*: two classes in pretraining, three channels here) is not taken.  -> the names
    that stayed at their initialisation."""
    dd = model.state_dict()
    wrapped = all(n.startswith("module.") for n in dd)
    sources = [checkpoint[key]] + ([checkpoint["student"]] if key != "student" and "student" in checkpoint else [])
    picked, missing = {}, []
    for name, value in dd.items():
        bare = name[len("module."):] if wrapped else name
        for src in sources:
            hit = src.get("module." + bare, src.get(bare))
            if hit is not None and tuple(hit.shape) == tuple(value.shape) and (src is sources[0] or bare.startswith("segmentation.")):
                picked[name] = hit
                break
        else:
            picked[name] = value
            missing.append(name)
    model.load_state_dict(picked)
    logging.info(f"not in the pretraining checkpoint (kept at init): {len(missing)} tensors: {missing[:4]}{' ...' if len(missing) > 4 else ''}")
    return missing


# ------------------------------------------------------------------------------------------------ data
def to_unit(image_u8):
    """uint8 [H, W, 3] -> fp32 [3, H, W] in [0, 1]."""
    return torch.from_numpy((image_u8.astype(np.float32) / 255.0).transpose(2, 0, 1).copy())


class PairDataset(torch.utils.data.Dataset):
    """(lr fp32 [3, 16, 64], hr fp32 [3, 32, 128], label str) from a TextZoom LMDB: keys image_hr-%09d, image_lr-%09d, label-%09d
    and num-samples; both images are resized (bilinear) to the two fixed sizes."""

    def __init__(self, path):
        self.path = os.fspath(path)
        if not os.path.isdir(self.path):
            raise AssertionError(f"{path} is not a valid directory.")
        self._env = None
        with lmdb_file.LmdbReader(self.path) as env:
            n = env.get(b"num-samples")
            if n is None:
                raise lmdb_file.LmdbError(f"{self.path}: no 'num-samples' record")
            self.length = int(n)

    def __len__(self):
        return self.length

    def __getstate__(self):                  # the reader is opened once per DataLoader worker (an mmap does not survive pickling)
        state = dict(self.__dict__)
        state["_env"] = None
        return state

    def __getitem__(self, idx):
        from PIL import Image
        if self._env is None:
            self._env = lmdb_file.LmdbReader(self.path)
        try:
            pair = []
            for kind, (h, w) in (("lr", SR_LR_SIZE), ("hr", SR_HR_SIZE)):
                buf = self._env.get(f"image_{kind}-{idx + 1:09d}".encode())
                pair.append(to_unit(resize_bilinear(np.asarray(Image.open(io.BytesIO(buf)).convert("RGB")), h, w)))
            label = self._env.get(f"label-{idx + 1:09d}".encode())
        except Exception:
            return None
        return pair[0], pair[1], (label or b"").decode("utf-8", "replace")


class SyntheticPairSet(torch.utils.data.Dataset):
    """Seeded (lr, hr, "") for smoke runs: HR is a few dark strokes and rectangles on a bright, slightly graded background; LR is the
    2 x 2 mean of a lightly blurred HR plus noise - detail that bicubic interpolation does not bring back and a head can learn to."""

    def __init__(self, length, seed=0, noise=0.01):
        self.length, self.seed, self.noise = int(length), int(seed), float(noise)

    def __len__(self):
        return self.length

    def __getitem__(self, i):
        rng = np.random.RandomState((self.seed * 1_000_003 + i) % (2 ** 31))
        H, W = SR_HR_SIZE
        ink = np.zeros((H, W), np.float32)
        for _ in range(rng.randint(3, 8)):
            y, x = rng.randint(2, H - 10), rng.randint(2, W - 22)
            if rng.rand() < 0.3:                                       # a bar
                ink[y:y + rng.randint(2, 9), x:x + rng.randint(2, 5)] = 1.0
            else:                                                      # a stroke, two pixels wide
                n = rng.randint(8, 20)
                yy = np.clip(y + np.cumsum(rng.randint(-1, 2, n)), 0, H - 2)
                xx = np.clip(x + np.arange(n), 0, W - 2)
                ink[yy, xx] = ink[yy + 1, xx] = 1.0
        paper = rng.uniform(0.6, 0.95, 3).astype(np.float32)[:, None, None] + \
            np.linspace(0.0, rng.uniform(-0.1, 0.1), W, dtype=np.float32)[None, None, :]
        colour = rng.uniform(0.0, 0.3, 3).astype(np.float32)[:, None, None]
        hr = np.clip(paper * (1.0 - ink[None]) + colour * ink[None], 0.0, 1.0).astype(np.float32)
        pad = np.pad(hr, ((0, 0), (1, 1), (1, 1)), mode="edge")
        k = np.array([0.25, 0.5, 0.25], np.float32)                    # the light blur, separable
        blur = sum(k[a] * pad[:, a:a + H, :] for a in range(3))
        blur = sum(k[a] * blur[:, :, a:a + W] for a in range(3))
        lr = blur.reshape(3, H // 2, 2, W // 2, 2).mean(axis=(2, 4)) + self.noise * rng.standard_normal((3, H // 2, W // 2)).astype(np.float32)
        return torch.from_numpy(np.clip(lr, 0.0, 1.0).astype(np.float32)), torch.from_numpy(hr), ""


def collate(batch):
    batch = [b for b in batch if b is not None]
    return torch.stack([b[0] for b in batch]), torch.stack([b[1] for b in batch])


# ------------------------------------------------------------------------------------------------ steps
def training_iteration(model, optimizer, lr_images, hr_images, lr):
    """lr_images fp32 [B, 3, 16, 64], hr_images fp32 [B, 3, 32, 128] -> the loss (a device scalar); nothing is read back."""
    for g in optimizer.param_groups:
        g["lr"] = float(lr)
    loss = model(lr_images, hr_images, return_loss=True)
    optimizer.zero_grad()
    loss.backward()
    optimizer.step()
    return loss.detach()


@torch.no_grad()
def evaluate(model, loader, device):
    """-> {psnr, ssim, bicubic_psnr, bicubic_ssim, n_images}: the means over the batches (weighted by their size) of calculate_psnr and
    ssim of forward_sr against hr, and the same two numbers for clamp(base, 0, 1) - the bicubic baseline beside the model."""
    from .metric.eval_superpixel import calculate_psnr, ssim
    mod = model.module if hasattr(model, "module") else model
    sums, n = np.zeros(4), 0
    for lr_images, hr_images in loader:
        lr_images, hr_images = lr_images.to(device, non_blocking=True), hr_images.to(device, non_blocking=True)
        sr = mod.forward_sr(lr_images)
        base = mod.upsample(lr_images)[0].clamp_(0.0, 1.0)
        b = lr_images.shape[0]
        sums += b * np.array([float(calculate_psnr(sr, hr_images)), float(ssim(sr, hr_images)),
                              float(calculate_psnr(base, hr_images)), float(ssim(base, hr_images))])
        n += b
    m = sums / max(n, 1)
    return {"psnr": m[0], "ssim": m[1], "bicubic_psnr": m[2], "bicubic_ssim": m[3], "n_images": n}
