"""Loss of the text super-resolution finetuning task on the fused HIP kernels (kernels/sr.h: ccd_sr_loss_fwd / _bwd): TSRN's
pixel loss plus its gradient-profile term.  Per channel plane x with zero padding

    g(x) = sqrt((0.5 (x[y, x+1] - x[y, x-1]))^2 + (0.5 (x[y-1, x] - x[y+1, x]))^2 + 1e-6)
    mse_n = mean (sr - hr)^2,   gp_n = mean |g(sr) - g(hr)|   over the 3 H W elements of image n
    L = mean_n (mse_n + gp_weight gp_n)  [ + ssim_weight (1 - SSIM(sr, hr)) ]

gp_weight 1e-4 is TSRN's published weight for [0, 1] images (untuned here).  sign(0) = 0 in the gradient: an image with sr == hr
gets a zero gradient.  The optional SSIM term is composed here from the fused SSIM module of Dino.metric.eval_superpixel."""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import ops


class SRLossFn(torch.autograd.Function):
    """loss, parts, per_image = SRLossFn.apply(sr fp32 [N, 3, H, W], hr, gp_weight).  The gradient goes to sr only."""

    @staticmethod
    def forward(ctx, sr, hr, gp_weight):
        loss, parts, per_image = ops.sr_loss_fwd(sr, hr, gp_weight)
        if ctx.needs_input_grad[0]:
            ctx.saved = (sr, hr, gp_weight)
        ctx.mark_non_differentiable(parts, per_image)
        return loss, parts, per_image

    @staticmethod
    def backward(ctx, d_loss, _dparts, _dper):
        sr, hr, gp_weight = ctx.saved
        ctx.saved = None
        return ops.sr_loss_bwd(sr, hr, gp_weight, 1.0, d_loss), None, None


class SRLoss(nn.Module):
    """SRLoss(gp_weight=1e-4, ssim_weight=0.0)(sr fp32 [N, 3, H, W], hr) -> scalar.  `last_parts` (fp64 [3]: L of the fused part,
    mean mse_n, mean gp_n) and `last_mse` (fp64 [N], per image) are device tensors of the last call: nothing is read back."""

    def __init__(self, gp_weight=1e-4, ssim_weight=0.0):
        super().__init__()
        self.gp_weight, self.ssim_weight = ops.sr_weight("gp_weight", gp_weight), ops.sr_weight("ssim_weight", ssim_weight)
        self.last_parts = self.last_mse = None
        self.ssim = None
        if self.ssim_weight > 0:
            from ..metric.eval_superpixel import SSIM
            self.ssim = SSIM()

    def forward(self, sr, hr):
        hr = hr.to(sr.device)
        loss, self.last_parts, per_image = SRLossFn.apply(sr, hr, self.gp_weight)
        self.last_mse = per_image[:, 0]
        if self.ssim is not None and sr.shape[0] > 0:
            loss = loss + self.ssim_weight * (1.0 - self.ssim(sr[:, :3], hr[:, :3]))
        return loss

    def extra_repr(self):
        return f"gp_weight={self.gp_weight}, ssim_weight={self.ssim_weight}"
