"""Parallel attention recognition head: the reference's `Attention` (Dino/modules/attention.py:5-30, selected by
`model_vision_attention: 'attention'`) followed by `BaseVision.cls` (Dino/modules/model_vision.py:31-39).  A learned reading-order query
per character position, an additive (tanh) score against each of the 256 backbone tokens, a softmax over the tokens, the weighted sum of
the tokens, one classifier for all positions: the 2-D token grid read in ONE pass, no sequential decoding.

    Q0 = b0[:, None] + W0 F          P = X Wv^T + bv          a = softmax_s(tanh(P + Q0) We^T + be)          logits = (a X) Wc^T + bc

The nn.Module carries the parameters under the reference's names (`attention.f0_embedding.weight [T, E]`, `attention.w0.{weight [256, T],
bias}`, `attention.wv.{weight, bias}`, `attention.we.{weight [T, E], bias}`, `cls.{weight, bias}`; a state dict of the reference's
`Attention` loads into `.attention`), held in the arena like every other module.  The computation is ParallelAttnFn on the HIP kernels:
the existing GEMMs for P, the classifier and their gradients, ccd_posattn_fwd / _bwd / _fold (kernels/posattn.h) for everything between.
Q0 and its three small gradients (dW0 = dQ0 F^T, db0 = rowsum dQ0, dF = W0^T dQ0: [256, E] against [T, E] and [256, T], once per step,
image-independent) are torch ops on the arena tensors.  There is no PyTorch-eager fallback.

The output has the NRTR decoder's shape, fp32 [N, T, C], and TFLoss takes it unchanged: position t predicts target t + 1 and the last
position has no target, so row T - 1 of We and be[T - 1] get an exactly zero gradient from the loss.  (Row T - 1 of F and column T - 1 of
W0 do not: Q0 sums over the positions and is shared by all of them.)
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import finetune_engine as fe
from .. import ops
from ..modules.vision_transformer import ArenaModule, _holder

BF16, F32 = torch.bfloat16, torch.float32
GRID_ROWS, GRID_COLS = 8, 32                  # the backbone's token grid for a 32 x 128 crop, patch 4: token = row * 32 + column
TOKENS, ROWS = ops.POSATTN_TOKENS, ops.POSATTN_MAX_T      # 256 tokens; a sample's positions are padded to 32 rows


class ParallelAttnFn(torch.autograd.Function):
    """logits, attn = ParallelAttnFn.apply(tokens bf16 [N, 256, E], module) -> fp32 [N, T, C] view of a [N * 32, 128] buffer (rows T..31 of
    a sample: the classifier's bias, never read) and the attention maps fp32 [N, T, 256].  TFLossFn parks its bf16, row- and
    column-padded logit gradient for backward (finetune_engine._PARKED_LOGIT_GRADS, as it does for DecoderFn)."""

    @staticmethod
    def forward(ctx, tokens, module):
        N, E, T, C = tokens.shape[0], module.in_features, module.max_seq_len, module.num_classes
        module.refresh_packed()
        arena, pre = module.arena, module.arena_prefix
        x2 = tokens.contiguous().view(N * TOKENS, E)
        P = ops.gemm_nt(x2, module.wv, bias=arena.w(pre + "attention.wv.bias"))                        # [N * 256, E] bf16
        attn, G = ops.posattn_fwd(P, x2, module.q0, module.we, arena.w(pre + "attention.we.bias"), T)
        logits = ops.gemm_nt(G, module.cls_w, epilogue=ops.EPI_F32, bias=module.cls_bias)              # [N * 32, 128] fp32
        if ctx.needs_input_grad[0]:
            ctx.module, ctx.saved, ctx.key = module, (x2, P, attn, G), logits.data_ptr()
            fe._PARKED_LOGIT_GRADS.pop(ctx.key, None)
        ctx.mark_non_differentiable(attn)
        return logits.view(N, ROWS, fe.CLS_PAD)[:, :T, :C], attn

    @staticmethod
    def backward(ctx, d_logits, _d_attn):
        module = ctx.module
        x2, P, attn, G = ctx.saved
        ctx.saved = None
        arena, pre, E, T, C = module.arena, module.arena_prefix, module.in_features, module.max_seq_len, module.num_classes
        N, dev = attn.shape[0], x2.device
        d_pad = fe._PARKED_LOGIT_GRADS.pop(ctx.key, None)
        if d_pad is None or any(st != 0 for st in d_logits.stride()):
            extra = torch.zeros((N * ROWS, fe.CLS_PAD), dtype=BF16, device=dev)
            extra.view(N, ROWS, fe.CLS_PAD)[:, :T, :C] = d_logits.to(BF16)
            d_pad = extra if d_pad is None else d_pad + extra
        dw = torch.empty((fe.CLS_PAD, E), dtype=F32, device=dev)
        ops.gemm_tn(d_pad, G, dw, accumulate=False)
        ops.permute4(dw, (E, 1), (C, E), arena.g(pre + "cls.weight"), accumulate=True)
        db = torch.zeros(fe.CLS_PAD, dtype=F32, device=dev)
        ops.colsum_bf16(d_pad, db)
        arena.g(pre + "cls.bias").add_(db[:C])
        dG = ops.gemm_nt(d_pad, module.cls_t)                                                          # [N * 32, E] bf16
        # dX1 | dP side by side: the token gradient dX1 + dP Wv is then ONE product against [I | Wv^T]
        both = torch.empty((N * TOKENS, 2 * E), dtype=BF16, device=dev)
        dX1, dP, dQ0, dWe, dbe = ops.posattn_bwd(dG, x2, P, module.q0, module.we, attn, out=(both[:, :E], both[:, E:]))
        arena.g(pre + "attention.we.weight").add_(dWe[:T])
        arena.g(pre + "attention.we.bias").add_(dbe[:T])
        F, W0 = arena.w(pre + "attention.f0_embedding.weight"), arena.w(pre + "attention.w0.weight")
        arena.g(pre + "attention.w0.weight").addmm_(dQ0, F.t())                                        # (image-independent, [256, T])
        arena.g(pre + "attention.w0.bias").add_(dQ0.sum(dim=1))
        arena.g(pre + "attention.f0_embedding.weight").addmm_(W0.t(), dQ0)
        dwv = torch.empty((E, E), dtype=F32, device=dev)
        ops.gemm_tn(dP, x2, dwv, accumulate=False)
        arena.g(pre + "attention.wv.weight").add_(dwv)
        arena.g(pre + "attention.wv.bias").add_(dQ0.sum(dim=0))                                        # dbv = sum_{n, s} dP = colsum dQ0: fixed order
        d_tokens = ops.gemm_nt(both, module.wv_cat)                                                    # [N * 256, E] bf16
        if module.grad_ready_hook is not None:
            module.grad_ready_hook(pre)
        return d_tokens.view(N, TOKENS, E), None


class ParallelAttnDecoder(ArenaModule):
    last_attn = None                           # the attention maps of the last forward, fp32 [N, T, 8, 32]

    def __init__(self, in_features, num_classes, max_seq_len=25, **kwargs):
        super().__init__()
        if in_features % 64 or in_features > 768 or not 2 <= num_classes <= fe.CLS_PAD or not 1 <= max_seq_len <= ROWS:
            raise NotImplementedError("HIP ParallelAttnDecoder: in_features a multiple of 64 up to 768, 2..128 classes, max_seq_len 1..32")
        self.in_features, self.num_classes, self.max_seq_len = int(in_features), int(num_classes), int(max_seq_len)
        E, T = self.in_features, self.max_seq_len
        # construction order == reference order (torch's default initialisations draw from the RNG stream in this order)
        self.attention = _holder(f0_embedding=nn.Embedding(T, E), w0=nn.Linear(T, TOKENS), wv=nn.Linear(E, E), we=nn.Linear(E, T))
        self.cls = nn.Linear(E, num_classes)
        self.wv = self.wv_cat = self.we = self.q0 = self.cls_w = self.cls_t = self.cls_bias = None

    def refresh_packed(self):
        """The bf16 GEMM / kernel operands from the fp32 master weights: Wv, [I | Wv^T], We zero-padded to 32 rows, Q0 = b0 + W0 F, the
        classifier zero-padded to 128 rows (and its transpose)."""
        arena, pre, C, E, T = self.ensure_arena(), self.arena_prefix, self.num_classes, self.in_features, self.max_seq_len
        if self.cls_w is None or self.cls_w.device != arena.device:
            z = lambda *shape, dt=BF16: torch.zeros(shape, dtype=dt, device=arena.device)
            self.cls_w, self.cls_t, self.cls_bias = z(fe.CLS_PAD, E), z(E, fe.CLS_PAD), z(fe.CLS_PAD, dt=F32)
            self.wv, self.wv_cat, self.we = z(E, E), z(E, 2 * E), z(ROWS, E)
            self.wv_cat[:, :E] = torch.eye(E, dtype=BF16, device=arena.device)
        w = arena.w(pre + "cls.weight")
        ops.permute4(w, (E, 1), (C, E), self.cls_w, dst_strides=(E, 1))
        ops.permute4(w, (1, E), (E, C), self.cls_t, dst_strides=(fe.CLS_PAD, 1))
        self.cls_bias[:C].copy_(arena.w(pre + "cls.bias"))
        wv = arena.w(pre + "attention.wv.weight")
        ops.permute4(wv, (E, 1), (E, E), self.wv, dst_strides=(E, 1))
        ops.permute4(wv, (1, E), (E, E), self.wv_cat[:, E:], dst_strides=(2 * E, 1))
        ops.permute4(arena.w(pre + "attention.we.weight"), (E, 1), (T, E), self.we, dst_strides=(E, 1))
        self.q0 = torch.addmm(arena.w(pre + "attention.w0.bias")[:, None], arena.w(pre + "attention.w0.weight"),
                              arena.w(pre + "attention.f0_embedding.weight")).to(BF16)

    # ---------------------------------------------------------------------------------- surface (as NRTRDecoder's)
    def forward_train(self, tokens):
        """tokens [N, 256, E] -> (logits fp32 [N, T, C], attn fp32 [N, T, 8, 32])."""
        logits, attn = ParallelAttnFn.apply(tokens.to(BF16), self)
        self.last_attn = attn.view(attn.shape[0], self.max_seq_len, GRID_ROWS, GRID_COLS)
        return logits, self.last_attn

    @torch.no_grad()
    def forward_test(self, tokens):
        """-> softmax probabilities fp32 [N, T, C]."""
        return self.forward_train(tokens)[0].softmax(dim=-1)

    def forward(self, tokens, train_mode=True):
        return self.forward_train(tokens) if train_mode else self.forward_test(tokens)
