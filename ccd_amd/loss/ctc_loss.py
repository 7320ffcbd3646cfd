"""CTC loss of the CTC recognition head on the fused HIP kernels (kernels/ctc.h: ccd_ctc_loss_fwd / _bwd): the semantics of
torch.nn.CTCLoss(blank=0, reduction='mean', zero_infinity=True) applied to log_softmax(logits) - the log-softmax is inside the kernel."""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import finetune_engine as fe
from .. import ops

F32 = torch.float32


class CTCLossFn(torch.autograd.Function):
    """loss, infeasible = CTCLossFn.apply(logits fp32 [B, T, C] (row stride >= C), targets int64 [B, Lmax] zero-padded)."""

    @staticmethod
    def forward(ctx, logits, targets):
        B, T, C = logits.shape
        assert logits.dtype == F32 and logits.stride(2) == 1 and logits.stride(0) == T * logits.stride(1)
        lg2 = logits.as_strided((B * T, C), (logits.stride(1), 1))
        nll, acc, ws = ops.ctc_loss_fwd(lg2, C, targets, T)
        if ctx.needs_input_grad[0]:
            ctx.saved = (logits, lg2, targets, ws)
        ctx.mark_non_differentiable(acc)
        return acc[0] / acc[1], acc

    @staticmethod
    def backward(ctx, d_loss, _dacc):
        logits, lg2, targets, ws = ctx.saved
        ctx.saved = None
        B, T, C = logits.shape
        padded = lg2.stride(0) == fe.CLS_PAD
        d = ops.ctc_loss_bwd(lg2, C, targets, T, ws, d_loss.reshape(1).to(F32).contiguous(), fe.CLS_PAD if padded else None)
        from ..decoder.ctc_decoder import HEAD_LOGITS
        if padded and logits._base is not None and logits._base.data_ptr() in HEAD_LOGITS:     # CTCHeadFn's: hand the bf16 buffer over
            fe._PARKED_LOGIT_GRADS[logits._base.data_ptr()] = d
            return torch.zeros((), dtype=F32, device=d.device).expand(logits.shape), None
        return d[:, :C].float().view(B, T, C), None


class CTCLoss(nn.Module):
    """CTCLoss()(logits [B, T, C], {'padded_targets': int64 [B, Lmax]}) -> scalar.  A sample whose label cannot be aligned to T frames
    (or holds a class outside [1, C)) contributes 0 and no gradient; `last_infeasible` counts them, on the device."""

    def __init__(self, blank=0, zero_infinity=True, **kwargs):
        super().__init__()
        if blank != 0 or not zero_infinity:
            raise NotImplementedError("HIP CTCLoss implements blank=0, zero_infinity=True, reduction='mean'")
        self.last_infeasible = None

    def forward(self, outputs, targets_dict, img_metas=None):
        targets = targets_dict['padded_targets'] if isinstance(targets_dict, dict) else targets_dict
        targets = targets.to(outputs.device).long().contiguous()
        if outputs.dtype != F32 or outputs.stride(-1) != 1 or outputs.stride(0) != outputs.shape[1] * outputs.stride(1):
            outputs = outputs.float().contiguous()
        loss, acc = CTCLossFn.apply(outputs, targets)
        self.last_infeasible = acc[2]
        return loss
