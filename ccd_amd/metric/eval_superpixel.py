"""The super-resolution metrics of the reference (Dino/metric/eval_superpixel.py), on the GPU: `calculate_psnr`, `gaussian`,
`create_window`, `ssim`, `SSIM`, `TRI_SSIM` (also importable as `Dino.metric.eval_superpixel`).

    calculate_psnr(img1, img2)                          -> 0-dim fp32 tensor, or float('inf') when the mse is 0
    ssim(img1, img2, window_size=11, size_average=True) -> 0-dim mean, or per-image means [N] when size_average=False
    SSIM(window_size=11, size_average=True)(img1, img2)         the same on img[:, :3] (an nn.Module; usable as a loss)
    TRI_SSIM(window_size=11, size_average=True)(img1, img2, img3)   three images, all channels
    gaussian(window_size, sigma), create_window(window_size, channel)   the host-side windows, bit-equal to the reference's

Each SSIM is one fused HIP launch (moments by two separable passes through LDS, map and per-tile sums in registers) plus a tiny
fixed-order reduction; the backward is one more fused launch, so autograd runs through every metric.  Nothing synchronises with the
host except `calculate_psnr`, which makes the reference's one `mse == 0` test.

Differences from the reference:
  * GPU only: CPU tensors raise RuntimeError.  Only fp32 inputs (TypeError otherwise) of one shape [N, C, H, W] (ValueError
    otherwise); window_size must be odd, 1..15 (ValueError otherwise; the reference also accepts even sizes).
  * The window is applied as two separable 1-D passes, g_i (g_j x), instead of one 2-D correlation with the rounded outer product
    g_i g_j: the moments differ from the reference's by fp32 rounding (about 1e-7 on the SSIM of [0, 1] images).
  * Sums run in fp64 in a fixed order: the PSNR's mse (the reference: fp32 mean) and the SSIM means.  Results are bitwise repeatable
    and an image's SSIM does not depend on the other images of the batch.
  * The gradients are once-differentiable (no double backward).
  * `SSIM` / `TRI_SSIM` keep no `window` / `channel` attributes (the reference caches its 2-D window there); like the
    reference's, their state_dict() is empty.
  * An empty batch gives nan for a mean and an empty [0] tensor for per-image means, as in the reference; planes with H, W or C == 0
    raise ValueError.
"""
from __future__ import annotations

from math import exp

import torch
import torch.nn as nn

from .. import _lib, ops

_SIGMA = 1.5
_taps_cache: dict = {}


def gaussian(window_size, sigma):
    """1-D Gaussian of window_size taps centred on window_size // 2, normalised to sum 1 (fp32, on the host)."""
    c = window_size // 2
    w = torch.tensor([exp(-float((i - c) * (i - c)) / (2.0 * sigma * sigma)) for i in range(window_size)], dtype=torch.float32)
    return w / w.sum()


def create_window(window_size, channel):
    """The 2-D window [channel, 1, window_size, window_size]: the outer product of gaussian(window_size, 1.5) with itself."""
    g = gaussian(window_size, _SIGMA)
    return torch.outer(g, g).expand(channel, 1, window_size, window_size).contiguous()


def _taps(window_size):
    t = _taps_cache.get(window_size)
    if t is None:
        t = _taps_cache[window_size] = tuple(gaussian(window_size, _SIGMA).tolist())
    return t


def _check(imgs, what, window_size=None):
    """Shape / dtype / device contract; returns the inputs with contiguous rows (views that have them are kept as they are)."""
    if not all(isinstance(x, torch.Tensor) for x in imgs):
        raise TypeError(f"{what}: expects torch tensors")
    shape = tuple(imgs[0].shape)
    if len(shape) != 4:
        raise ValueError(f"{what}: expects [N, C, H, W] images, got {list(shape)}")
    if any(tuple(x.shape) != shape for x in imgs):
        raise ValueError(f"{what}: the images differ in shape: {[list(x.shape) for x in imgs]}")
    if min(shape[1:]) < 1:
        raise ValueError(f"{what}: empty planes {list(shape)}")
    if any(x.dtype != torch.float32 for x in imgs):
        raise TypeError(f"{what}: only float32 images are supported, got {[str(x.dtype) for x in imgs]}")
    if window_size is not None and not (isinstance(window_size, int) and window_size % 2 == 1
                                        and 1 <= window_size <= ops.SSIM_MAX_WINDOW):
        raise ValueError(f"{what}: window_size must be an odd integer from 1 to {ops.SSIM_MAX_WINDOW}, got {window_size!r}")
    if _lib._stream_override is None:            # (bound to the host executor in kernel tests)
        if any(x.device.type != "cuda" for x in imgs):
            raise RuntimeError(f"{what} runs on an AMD GPU only (move the images with .cuda() first); there is no CPU path")
        if any(x.device != imgs[0].device for x in imgs):
            raise ValueError(f"{what}: the images are on different devices")
    out = []
    for x in imgs:
        W = x.shape[3]
        rows_ok = (x.stride(3) == 1 or W == 1) and (x.stride(2) == W or x.shape[2] == 1)
        out.append(x if rows_ok else x.contiguous())
    return out


def _ssim(imgs, window_size, size_average, what):
    imgs = _check(imgs, what, window_size)
    return ops.SsimFn.apply(window_size, _taps(window_size), bool(size_average), *imgs)


def calculate_psnr(img1, img2):
    """PSNR in dB of [0, 1] images over their first three channels: 20 log10(255 / sqrt(mse)) with mse the mean of
    (255 img1 - 255 img2)^2 over the whole batch; float('inf') when mse == 0."""
    a, b = _check([img1, img2], "calculate_psnr")
    psnr, mse = ops.PsnrFn.apply(a, b)
    if mse.item() == 0:
        return float("inf")
    return psnr


def ssim(img1, img2, window_size=11, size_average=True):
    """SSIM over all channels of img1, img2 [N, C, H, W] with a Gaussian window (sigma 1.5, zero padding)."""
    return _ssim([img1, img2], window_size, size_average, "ssim")


class SSIM(nn.Module):
    """SSIM of the first three channels (an RGB + mask batch is read in place); no parameters or buffers."""

    def __init__(self, window_size=11, size_average=True):
        super().__init__()
        self.window_size = window_size
        self.size_average = size_average

    def forward(self, img1, img2):
        if not (isinstance(img1, torch.Tensor) and isinstance(img2, torch.Tensor)) or img1.dim() != 4 or img2.dim() != 4:
            _check([img1, img2], "SSIM")                 # raises the contract's error
        return _ssim([img1[:, :3], img2[:, :3]], self.window_size, self.size_average, "SSIM")


class TRI_SSIM(nn.Module):
    """The three-image SSIM variant over all channels: (mu1 mu2 + mu2 mu3 + mu3 mu1 + C1)(s12 + s23 + s31 + C2) /
    ((mu1^2 + mu2^2 + mu3^2 + C1)(s1^2 + s2^2 + s3^2 + C2)); no parameters or buffers."""

    def __init__(self, window_size=11, size_average=True):
        super().__init__()
        self.window_size = window_size
        self.size_average = size_average

    def forward(self, img1, img2, img3):
        return _ssim([img1, img2, img3], self.window_size, self.size_average, "TRI_SSIM")
