"""CTC recognition head (SVTR style): the 8 x 32 token grid of the backbone pooled over its height to 32 frames, one linear layer,
class 0 = blank.  Non-autoregressive: one encoder pass recognises a word.  The reference has no CTC head.

The nn.Module carries the parameters (`fc.weight [C, E]`, `fc.bias [C]`, held in the arena like every other module); the
computation is CTCHeadFn on the HIP kernels: ccd_ctc_pool_fwd / _bwd (kernels/ctc.h) around the classifier products, which are the
existing GEMMs exactly as NRTRDecoder's classifier uses them.  There is no PyTorch-eager fallback.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import finetune_engine as fe
from .. import ops
from ..modules.utils import trunc_normal_
from ..modules.vision_transformer import ArenaModule

BF16, F32 = torch.bfloat16, torch.float32
GRID_ROWS, GRID_COLS = 8, 32                  # the backbone's token grid for a 32 x 128 crop, patch 4: token = row * 32 + column


# data pointers of the padded logit buffers CTCHeadFn has handed out and whose backward has not run: only for these may CTCLossFn
# park its bf16 gradient instead of returning it
HEAD_LOGITS = set()


class CTCHeadFn(torch.autograd.Function):
    """logits = CTCHeadFn.apply(tokens bf16 [N, 256, E], module) -> fp32 [N, 32, C] view of a [N * 32, 128] buffer.  CTCLossFn parks
    its bf16, column-padded logit gradient for backward (finetune_engine._PARKED_LOGIT_GRADS, as TFLossFn does for DecoderFn)."""

    @staticmethod
    def forward(ctx, tokens, module):
        N, C = tokens.shape[0], module.num_classes
        module.refresh_packed()
        frames = ops.ctc_pool_fwd(tokens.contiguous(), GRID_ROWS, GRID_COLS)
        logits = ops.gemm_nt(frames, module.cls, epilogue=ops.EPI_F32, bias=module.cls_bias)           # [N * 32, 128] fp32
        if ctx.needs_input_grad[0]:
            ctx.module, ctx.frames, ctx.key = module, frames, logits.data_ptr()
            fe._PARKED_LOGIT_GRADS.pop(ctx.key, None)
            HEAD_LOGITS.add(ctx.key)
        return logits.view(N, GRID_COLS, fe.CLS_PAD)[:, :, :C]

    @staticmethod
    def backward(ctx, d_logits):
        module, frames = ctx.module, ctx.frames
        ctx.frames = None
        arena, pre, C, E = module.arena, module.arena_prefix, module.num_classes, module.in_features
        HEAD_LOGITS.discard(ctx.key)
        d_pad = fe._PARKED_LOGIT_GRADS.pop(ctx.key, None)
        if d_pad is None or any(st != 0 for st in d_logits.stride()):
            extra = torch.zeros((frames.shape[0], fe.CLS_PAD), dtype=BF16, device=frames.device)
            extra[:, :C] = d_logits.reshape(-1, C).to(BF16)
            d_pad = extra if d_pad is None else d_pad + extra
        dw = torch.empty((fe.CLS_PAD, E), dtype=F32, device=frames.device)
        ops.gemm_tn(d_pad, frames, dw, accumulate=False)
        ops.permute4(dw, (E, 1), (C, E), arena.g(pre + "fc.weight"), accumulate=True)
        db = torch.zeros(fe.CLS_PAD, dtype=F32, device=frames.device)
        ops.colsum_bf16(d_pad, db)
        arena.g(pre + "fc.bias").add_(db[:C])
        d_frames = ops.gemm_nt(d_pad, module.cls_t)                                                    # [N * 32, E] bf16
        if module.grad_ready_hook is not None:
            module.grad_ready_hook(pre)
        return ops.ctc_pool_bwd(d_frames, GRID_ROWS, GRID_COLS), None


class CTCDecoder(ArenaModule):
    def __init__(self, in_features, num_classes, **kwargs):
        super().__init__()
        if in_features % 64 or not 2 <= num_classes <= fe.CLS_PAD:
            raise NotImplementedError("HIP CTCDecoder: in_features a multiple of 64, 2..128 classes")
        self.in_features, self.num_classes = int(in_features), int(num_classes)
        self.fc = nn.Linear(in_features, num_classes)
        trunc_normal_(self.fc.weight, std=.02)
        nn.init.zeros_(self.fc.bias)
        self.cls = self.cls_t = self.cls_bias = None

    def refresh_packed(self):
        """The classifier zero-padded to 128 rows as bf16 GEMM operands (and its transpose), from the fp32 master weights."""
        arena, pre, C, E = self.ensure_arena(), self.arena_prefix, self.num_classes, self.in_features
        if self.cls is None or self.cls.device != arena.device:
            self.cls = torch.zeros((fe.CLS_PAD, E), dtype=BF16, device=arena.device)
            self.cls_t = torch.zeros((E, fe.CLS_PAD), dtype=BF16, device=arena.device)
            self.cls_bias = torch.zeros(fe.CLS_PAD, dtype=F32, device=arena.device)
        w = arena.w(pre + "fc.weight")
        ops.permute4(w, (E, 1), (C, E), self.cls, dst_strides=(E, 1))
        ops.permute4(w, (1, E), (E, C), self.cls_t, dst_strides=(fe.CLS_PAD, 1))
        self.cls_bias[:C].copy_(arena.w(pre + "fc.bias"))

    # ---------------------------------------------------------------------------------- surface (as NRTRDecoder's)
    def forward_train(self, tokens):
        """tokens [N, 256, E] -> logits fp32 [N, 32, C]."""
        return CTCHeadFn.apply(tokens.to(BF16), self)

    @torch.no_grad()
    def forward_test(self, tokens):
        """-> softmax probabilities fp32 [N, 32, C]."""
        return CTCHeadFn.apply(tokens.to(BF16), self).softmax(dim=-1)

    def forward(self, tokens, train_mode=True):
        return self.forward_train(tokens) if train_mode else self.forward_test(tokens)
