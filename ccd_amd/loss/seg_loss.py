"""Supervised text-segmentation loss of the finetuning task on the fused HIP kernels (kernels/seg_sup_loss.h:
ccd_seg_sup_loss_fwd / _bwd).  Text masks are thin strokes on a large background, so the pixel mean of the pretraining loss is not
enough: the classes are weighted, a Dice term scores the region and the band around glyph boundaries counts more (the trimap idea
of TexRNet).  With y = gt, p = sigmoid(z1 - z0), l = -log softmax(z)[y] and edge(q) = a scored pixel of the other class lies within
the (2 edge_radius + 1)^2 square around the scored pixel q:

    w = class_weight[y] (1 + edge_weight edge),   Omega = sum w,   CE = sum w l / Omega
    Dice_n = 1 - (2 sum p y + 1) / (sum p + sum y + 1) per image,   Dice = their mean over the images with a scored pixel
    L = CE + dice_weight Dice

With edge_weight = 0 and dice_weight = 0 this is F.cross_entropy(weight=class_weight, ignore_index=ignore_index) - except that a
batch without a scored pixel gives 0 with a zero gradient where torch gives NaN."""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import ops


class SegSupLossFn(torch.autograd.Function):
    """loss, parts, confusion = SegSupLossFn.apply(logits fp32 [N, 2, H, W], gt uint8 [N, H, W], params); params: ops.seg_sup_params'
    tuple.  The gradient goes to the logits only."""

    @staticmethod
    def forward(ctx, logits, gt, params):
        w0, w1, ignore, dice_weight, edge_weight, radius = params
        need = ctx.needs_input_grad[0]
        out = ops.seg_sup_loss(logits, gt, (w0, w1), ignore, dice_weight, edge_weight, radius, need_code=need)
        loss, parts, confusion = out
        if need:
            ctx.saved = (logits, out.code, out.ws, params)
        ctx.mark_non_differentiable(parts, confusion)
        return loss, parts, confusion

    @staticmethod
    def backward(ctx, d_loss, _dparts, _dconfusion):
        logits, code, ws, (w0, w1, _, dice_weight, edge_weight, _) = ctx.saved
        ctx.saved = None
        return ops.seg_sup_loss_bwd(logits, code, ws, (w0, w1), dice_weight, edge_weight, 1.0, d_loss), None, None


class SegSupLoss(nn.Module):
    """SegSupLoss(...)(logits fp32 [N, 2, H, W], gt uint8 [N, H, W]) -> scalar.  gt: 0 background, 1 text, ignore_index (2..255) and
    any other value are not scored.  `last_parts` (fp64 [4]: L, CE, Dice, Omega) and `last_confusion` (int64 [2, 2], [gt, pred] over
    the scored pixels of the batch, a tie predicting class 0) are device tensors of the last call: nothing is read back."""

    def __init__(self, class_weight=(1.0, 1.0), ignore_index=255, dice_weight=0.0, edge_weight=0.0, edge_radius=0):
        super().__init__()
        self.params = ops.seg_sup_params(class_weight, ignore_index, dice_weight, edge_weight, edge_radius)
        self.class_weight, self.ignore_index = self.params[:2], self.params[2]
        self.dice_weight, self.edge_weight, self.edge_radius = self.params[3:]
        self.last_parts = self.last_confusion = None

    def forward(self, logits, gt):
        if gt.dtype == torch.bool:
            gt = gt.view(torch.uint8)
        loss, self.last_parts, self.last_confusion = SegSupLossFn.apply(logits, gt.to(logits.device), self.params)
        return loss

    def extra_repr(self):
        return (f"class_weight={self.class_weight}, ignore_index={self.ignore_index}, dice_weight={self.dice_weight}, "
                f"edge_weight={self.edge_weight}, edge_radius={self.edge_radius}")
