"""Thin tensor-level wrappers over the C ABI (include/ccd_hip.h).  Every function enqueues HIP kernels on the
current stream; nothing here computes on the host."""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from . import _lib

EPI_BF16, EPI_GELU, EPI_RESID, EPI_F32, EPI_ATOMIC, EPI_DGELU = range(6)
BF16, F32 = torch.bfloat16, torch.float32
_EPI_NAMES = ("bf16", "gelu", "resid", "f32", "atomic", "dgelu")


class KernelTimer:
    """Optional per-launch timing with HIP events on the launching stream (bench.py's roofline leg).  Events are
    only read after the timed region has been synchronised, so recording them never stalls the stream."""

    def __init__(self, only=None):
        self.records = []          # (key, flops, algorithmic bytes, start_event, end_event)
        self.only = only           # optional set of keys: every other launch runs without events

    def span(self, key, flops, nbytes=0.0):
        if self.only is not None and key not in self.only:
            return None
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self.records.append((key, flops, nbytes, e0, e1))
        return e0, e1

    def summary(self):
        out = {}
        for key, flops, nbytes, e0, e1 in self.records:
            d = out.setdefault(key, {"launches": 0, "ms": 0.0, "flops": 0.0, "bytes": 0.0})
            d["launches"] += 1
            d["ms"] += e0.elapsed_time(e1)
            d["flops"] += flops
            d["bytes"] += nbytes
        return out


TIMER = None     # set to a KernelTimer to time every GEMM / attention / LayerNorm / loss launch


class _Span:
    """with _Span(key, flops, algorithmic bytes): the launches inside are bracketed by HIP events when a KernelTimer is attached."""

    def __init__(self, key, flops, nbytes, when=True):
        self.ev = TIMER.span(key, flops, nbytes) if TIMER is not None and when else None

    def __enter__(self):
        if self.ev:
            self.ev[0].record()

    def __exit__(self, *a):
        if self.ev:
            self.ev[1].record()


def policy_set(key, value):
    """Kernel-selection policy of the library (include/ccd_hip.h: ccd_policy_set), e.g. policy_set('gemm_256_min_m', 1)."""
    _lib.check(_lib.get().ccd_policy_set(key.encode(), int(value)), f"policy_set({key})")


def policy_get(key):
    v = ctypes.c_int(0)
    _lib.check(_lib.get().ccd_policy_get(key.encode(), ctypes.byref(v)), f"policy_get({key})")
    return v.value


class policy:
    """with ops.policy(gemm_256_min_m=1, gemm_row384=2): ...   (restores the previous values on exit)"""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.saved = {k: policy_get(k) for k in self.kw}
        for k, v in self.kw.items():
            policy_set(k, v)
        return self

    def __exit__(self, *a):
        for k, v in self.saved.items():
            policy_set(k, v)


def _call(name, *args):
    """The one launch path: entry point `name` of the library on the current stream.  The argument types come from the header
    (_lib.bind): a tensor goes in as it is and is checked against the parameter's element type."""
    try:
        code = getattr(_lib.get(), name)(*args, _lib.stream())
    except ctypes.ArgumentError as e:
        raise _lib.argument_error(name, e) from None
    _lib.check(code, name)


def upload(t, device):
    """A host tensor on `device` without a host synchronisation: through pinned memory and asynchronously to a GPU, a plain `.to` to
    the CPU (no copy)."""
    return t.pin_memory().to(device, non_blocking=True) if torch.device(device).type == "cuda" else t.to(device)


class _OncePerDevice:
    """A handle built on the host whose device copy is made once per device: `_upload(device)` says what the copy is, `on(device)`
    returns it."""

    _copies = None

    def on(self, device):
        if self._copies is None:
            self._copies = {}
        key = str(device)
        if key not in self._copies:
            self._copies[key] = self._upload(device)
        return self._copies[key]


def _ld(t):
    """(tensor, leading stride) of an optional 2-D operand: (None, 0) when it is absent."""
    return (None, 0) if t is None else (t, t.stride(0))


def _chk(t, dtype, name):
    """For what the header cannot say: the element type behind a void*, or a pointer inside a job structure."""
    if t is None:
        return
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if t.stride(-1) != 1:
        raise ValueError(f"{name}: innermost dimension must be contiguous")


def gemm_nt(a, b, *, epilogue=EPI_BF16, out=None, out2=None, bias=None, resid=None, rowscale=None,
            rows_per_sample=1, aux=None, alpha=1.0, m_fastest=None, d_rows=None, rows_mul=1, colsum=None,
            store_u=True):
    """out[M,N] = a[M,K] @ b[N,K]^T with a fused epilogue (see include/ccd_hip.h)."""
    M, K = a.shape
    N = b.shape[0]
    assert b.shape[1] == K
    odt = F32 if epilogue in (EPI_RESID, EPI_F32, EPI_ATOMIC) else BF16
    if out is None and (store_u or epilogue != EPI_GELU):
        out = torch.empty((M, N), dtype=odt, device=a.device)
    _chk(out, odt, "out")
    if epilogue == EPI_GELU and out2 is None:
        out2 = torch.empty((M, N), dtype=BF16, device=a.device)
    if m_fastest is None:
        m_fastest = 1 if N > M else 0
    # algorithmic bytes: each operand read once, each output written once (bf16 = 2 B, fp32 = 4 B)
    nbytes = 2.0 * (M * K + N * K) + M * N * {EPI_BF16: 2, EPI_GELU: 2 + (2 if store_u else 0), EPI_RESID: 8, EPI_F32: 4,
                                               EPI_ATOMIC: 8, EPI_DGELU: 4}[epilogue]
    with _Span("gemm_nt_" + _EPI_NAMES[epilogue], 2.0 * M * N * K, nbytes, when=d_rows is None):
        _call("ccd_gemm_nt", a, a.stride(0), b, b.stride(0), M, N, K, epilogue, out, N if out is None else out.stride(0), *_ld(out2), bias,
              *_ld(resid), rowscale, rows_per_sample, *_ld(aux), float(alpha), int(m_fastest), d_rows, int(rows_mul), colsum)
    return (out, out2) if epilogue == EPI_GELU else out      # (EPI_DGELU: out2, when given, receives gelu(aux))


def gemm_nt_resid_ln(a, b, *, bias, resid, rowscale, rows_per_sample, gamma, beta, eps, out=None):
    """out (fp32) = resid + (a @ b^T + bias) * rowscale[row // rows_per_sample];  y = LayerNorm(out) * gamma + beta.
    -> (out, y bf16, mean, rstd): the residual product with the following LayerNorm folded into its epilogue."""
    M, K = a.shape
    N = b.shape[0]
    assert b.shape[1] == K and N <= 512
    if out is None:
        out = torch.empty((M, N), dtype=F32, device=a.device)
    y = torch.empty((M, N), dtype=BF16, device=a.device)
    mean = torch.empty(M, dtype=F32, device=a.device)
    rstd = torch.empty(M, dtype=F32, device=a.device)
    with _Span("gemm_nt_resid", 2.0 * M * N * K, 2.0 * (M * K + N * K) + 10.0 * M * N):
        _call("ccd_gemm_nt_resid_ln", a, a.stride(0), b, b.stride(0), M, N, K, out, out.stride(0), bias, resid, resid.stride(0), rowscale,
              int(rows_per_sample), gamma, beta, float(eps), y, y.stride(0), mean, rstd)
    return out, y, mean, rstd


def lnbwd_tap_supported(g, N):
    """ccd_gemm_nt_lnbwd_tap_g16 takes the bf16 gradient stream at N = 384 (the ViT-Small path)."""
    return g.dtype == BF16 and N == 384 and policy_get("rowgemm") != 0


def gemm_nt_lnbwd(a, b, x, mean, rstd, gamma, g, dgamma, dbeta, accumulate=True, gb=None, rowscale=None, rows_per_sample=1,
                  dbias=None, tap=None):
    """dy = a @ b^T is the gradient of a LayerNorm output: g (+)= LN'(dy) with dgamma / dbeta (+ the bf16 tail of ln_bwd) in
    the epilogue of the product - dy never reaches HBM (ccd_gemm_nt + ccd_ln_bwd in one launch; N <= 384 or N = 512).
    tap = (d_tap bf16 [M, N], tap_gamma, tap_dgamma, tap_dbeta): a second LayerNorm of the same rows (a segmentation tap: same
    statistics, other gamma) whose backward pass joins the epilogue (lnbwd_tap_supported)."""
    g16 = g.dtype == BF16           # (round 6) the residual-gradient stream in bf16: ccd_gemm_nt_lnbwd_g16
    M, K = a.shape
    N = b.shape[0]
    assert b.shape[1] == K and tuple(x.shape) == (M, N) and tuple(g.shape) == (M, N) and N <= 512
    gbytes = 2.0 if g16 else 4.0
    common = (a, a.stride(0), b, b.stride(0), M, N, K, x, x.stride(0), mean, rstd, gamma, g, g.stride(0), 1 if accumulate else 0,
              dgamma, dbeta, *_ld(gb), rowscale, int(rows_per_sample), dbias)
    with _Span("gemm_nt_lnbwd", 2.0 * M * N * K, 2.0 * (M * K + N * K) + M * N * (4.0 + (2 * gbytes if accumulate else gbytes))
               + (2.0 * M * N if gb is not None else 0.0)):
        if tap is not None:
            d_tap, tap_gamma, tap_dgamma, tap_dbeta = tap
            assert g16 and tuple(d_tap.shape) == (M, N)
            _call("ccd_gemm_nt_lnbwd_tap_g16", *common, d_tap, d_tap.stride(0), tap_gamma, tap_dgamma, tap_dbeta)
        else:
            _call("ccd_gemm_nt_lnbwd_g16" if g16 else "ccd_gemm_nt_lnbwd", *common)
    return g


def mlp_bwd_fused_supported(g, E, H):
    """ccd_mlp_bwd_fused takes the bf16 gradient stream at E in {256, 384} with H a multiple of 128."""
    return g.dtype == BF16 and E in (256, 384) and H % 128 == 0


def mlp_bwd_fused(gb, w2t, w1t, u, *, db1, x, mean, rstd, gamma, g, dgamma, dbeta, gb_out, rowscale=None, rows_per_sample=1,
                  dbias=None, accumulate=True):
    """The data-gradient chain of the MLP branch in one launch (include/ccd_hip.h: ccd_mlp_bwd_fused):
    du = (gb @ w2t^T) * gelu'(u), dy2 = du @ w1t^T, then LayerNorm-2's backward of dy2 as in gemm_nt_lnbwd (bf16 stream g).
    w2t = fc2.weight^T [H, E], w1t = fc1.weight^T [E, H].  -> du bf16 [M, H]; db1 += colsum(du)."""
    M, E = gb.shape
    H = w2t.shape[0]
    assert tuple(w2t.shape) == (H, E) and tuple(w1t.shape) == (E, H) and tuple(u.shape) == (M, H) and tuple(x.shape) == (M, E)
    assert gb_out is None or gb_out.data_ptr() != gb.data_ptr()
    du = torch.empty((M, H), dtype=BF16, device=gb.device)
    # algorithmic bytes: gb, u in; du out; x in; g in + out; gb_out out; the weights once
    nbytes = M * (2.0 * E + 4.0 * H + 4.0 * E + (4.0 if accumulate else 2.0) * E + (2.0 * E if gb_out is not None else 0.0)) + 4.0 * E * H
    with _Span("mlp_bwd_fused", 4.0 * M * E * H, nbytes):
        _call("ccd_mlp_bwd_fused", gb, gb.stride(0), w2t, w2t.stride(0), w1t, w1t.stride(0), u, u.stride(0), du, du.stride(0), db1, x,
              x.stride(0), mean, rstd, gamma, g, g.stride(0), 1 if accumulate else 0, dgamma, dbeta, *_ld(gb_out), rowscale,
              int(rows_per_sample), dbias, M, E, H)
    return du


def mlp_fused(y, w1, b1, w2, b2, *, resid, rowscale, rows_per_sample, gamma, beta, eps, store_u=False, store_gact=False, out=None):
    """out (fp32) = resid + (gelu(y @ w1^T + b1) @ w2^T + b2) * rowscale[row // rows_per_sample];
    y_next = LayerNorm(out) * gamma + beta  ->  (out, y_next bf16, mean, rstd, u bf16 | None[, gelu(u) bf16 with store_gact]).
    The hidden activation never reaches HBM; `u` (the bf16 pre-activation) is written only when store_u, gelu(u) only when
    store_gact (the weight-gradient product of the backward pass reads it)."""
    M, E = y.shape
    H = w1.shape[0]
    assert tuple(w1.shape) == (H, E) and tuple(w2.shape) == (E, H) and tuple(resid.shape) == (M, E)
    dev = y.device
    if out is None:
        out = torch.empty((M, E), dtype=F32, device=dev)
    yn = torch.empty((M, E), dtype=BF16, device=dev)
    mean = torch.empty(M, dtype=F32, device=dev)
    rstd = torch.empty(M, dtype=F32, device=dev)
    u = torch.empty((M, H), dtype=BF16, device=dev) if store_u else None
    gact = torch.empty((M, H), dtype=BF16, device=dev) if (store_u and store_gact) else None
    # algorithmic bytes: y read, resid read, out + y_next written (+ u, + gelu(u)), weights once
    nbytes = M * E * (2.0 + 4.0 + 4.0 + 2.0) + (2.0 * M * H if store_u else 0.0) + (2.0 * M * H if gact is not None else 0.0) + 4.0 * E * H
    with _Span("mlp_fused", 4.0 * M * E * H, nbytes):
        _call("ccd_mlp_fused", y, y.stride(0), w1, w1.stride(0), b1, w2, w2.stride(0), b2, resid, resid.stride(0), rowscale,
              int(rows_per_sample), out, out.stride(0), gamma, beta, float(eps), yn, yn.stride(0), mean, rstd, *_ld(u), *_ld(gact), M, E, H)
    return (out, yn, mean, rstd, u, gact) if store_gact else (out, yn, mean, rstd, u)


def proj_mlp_fused(a, wp, bp, *, resid, rowscale1, gamma2, beta2, w1, b1, w2, b2, rowscale2, rows_per_sample, gamma, beta, eps,
                   save=False, out=None, tap_gamma=None, tap_beta=None, store_gact=False):
    """The second half of a transformer block in one launch (include/ccd_hip.h: ccd_proj_mlp_fused):
        x_mid = resid + (a @ wp^T + bp) * rowscale1;   y2 = LayerNorm(x_mid) * gamma2 + beta2
        out   = x_mid + (gelu(y2 @ w1^T + b1) @ w2^T + b2) * rowscale2;   y_next = LayerNorm(out) * gamma + beta
    -> (out, y_next, mean, rstd, saved) with saved = (x_mid, y2, mean2, rstd2, u) when `save` (what the backward pass reads), else None:
    then x_mid and y2 never reach HBM.  With tap_gamma / tap_beta a sixth result: LayerNorm(out) * tap_gamma + tap_beta (bf16).
    store_gact (with save): saved gains a sixth member, gelu(u) bf16 [M, H] (ccd_proj_mlp_fused_gact: what ccd_mlp_bwd_fused's caller
    hands to the weight-gradient pair).  Raises RuntimeError('unsupported shape') where the kernel does not apply."""
    M, E = a.shape
    H = w1.shape[0]
    assert tuple(wp.shape) == (E, E) and tuple(w1.shape) == (H, E) and tuple(w2.shape) == (E, H) and tuple(resid.shape) == (M, E)
    dev = a.device
    if out is None:
        out = torch.empty((M, E), dtype=F32, device=dev)
    yn = torch.empty((M, E), dtype=BF16, device=dev)
    mean = torch.empty(M, dtype=F32, device=dev)
    rstd = torch.empty(M, dtype=F32, device=dev)
    xmid = y2 = mean2 = rstd2 = u = None
    if save:
        xmid = torch.empty((M, E), dtype=F32, device=dev)
        y2 = torch.empty((M, E), dtype=BF16, device=dev)
        mean2 = torch.empty(M, dtype=F32, device=dev)
        rstd2 = torch.empty(M, dtype=F32, device=dev)
        u = torch.empty((M, H), dtype=BF16, device=dev)
    gact = torch.empty((M, H), dtype=BF16, device=dev) if (save and store_gact) else None
    tap = torch.empty((M, E), dtype=BF16, device=dev) if tap_gamma is not None else None
    # algorithmic bytes: a and resid read, out + y_next written (+ x_mid, y2, u [, gelu(u)] when saved), the three weight matrices once
    nbytes = M * E * (2.0 + 4.0 + 4.0 + 2.0) + (M * E * 6.0 + 2.0 * M * H if save else 0.0) + 4.0 * E * H + 2.0 * E * E + \
        (2.0 * M * E if tap is not None else 0.0) + (2.0 * M * H if gact is not None else 0.0)
    head = (a, a.stride(0), wp, wp.stride(0), bp, resid, resid.stride(0), rowscale1, gamma2, beta2, *_ld(xmid), *_ld(y2), mean2, rstd2,
            w1, w1.stride(0), b1, w2, w2.stride(0), b2, rowscale2, int(rows_per_sample), out, out.stride(0), gamma, beta, float(eps),
            yn, yn.stride(0), mean, rstd, *_ld(u))
    tail = (tap_gamma, tap_beta, *_ld(tap), M, E, H)
    with _Span("proj_mlp_fused", 4.0 * M * E * H + 2.0 * M * E * E, nbytes):
        if gact is not None:
            _call("ccd_proj_mlp_fused_gact", *head, gact, gact.stride(0), *tail)
        else:
            _call("ccd_proj_mlp_fused", *head, *tail)
    kept = None if not save else ((xmid, y2, mean2, rstd2, u, gact) if gact is not None else (xmid, y2, mean2, rstd2, u))
    res = (out, yn, mean, rstd, kept)
    return res + (tap,) if tap is not None else res


def gemm_tn_colsum(a, b, out, colsum, *, splits=0):
    """out[P,Q] += a[Mc,P]^T @ b[Mc,Q] and colsum[P] += a.sum(0): the weight and the bias gradient of a Linear in one pass
    over dY (fp32 atomics)."""
    Mc, Pd = a.shape
    Q = b.shape[1]
    assert b.shape[0] == Mc and tuple(out.shape) == (Pd, Q) and colsum.numel() == Pd
    with _Span("gemm_tn_atomic", 2.0 * Mc * Pd * Q, 2.0 * Mc * (Pd + Q) + 4.0 * Pd * Q):
        _call("ccd_gemm_tn_colsum", a, a.stride(0), b, b.stride(0), Pd, Q, Mc, out, out.stride(0), colsum, int(splits))
    return out


_TN_WS = {}
_TN_WS_RETIRED = []      # outgrown workspaces stay allocated: a captured HIP graph (pretrain.GraphedTrainingStep) may still write to them


def tn_pair_workspace(device, P1, Q1, P2, Q2):
    """The split-K workspace ccd_gemm_tn_pair_ws wants for these shapes: ONE fp32 buffer per (device, stream), grown to the largest
    request - launches on one stream use it in order, another stream gets its own.  A buffer that is outgrown is never freed (a graph
    captured earlier keeps its pointer).  None where the grouped kernel does not apply."""
    n = int(_lib.get().ccd_gemm_tn_pair_ws_floats(int(P1), int(Q1), int(P2), int(Q2)))
    if n <= 0:
        return None
    key = (device, _lib.stream())
    ws = _TN_WS.get(key)
    if ws is None or ws.numel() < n:
        if ws is not None:
            _TN_WS_RETIRED.append(ws)
        ws = torch.empty(n, dtype=torch.float32, device=device)
        _TN_WS[key] = ws
    return ws


def gemm_tn_pair(a1, b1, out1, a2, b2, out2, *, workspace=True):
    """out1 += a1^T @ b1 and out2 += a2^T @ b2 (same number of contraction rows) in one launch where the shapes allow it
    (ccd_gemm_tn_pair_ws: per-slice partial tiles in a workspace + one reduction pass; workspace=False: ccd_gemm_tn_pair's fp32
    atomics); equal to two gemm_tn calls up to fp32 summation order."""
    Mc = a1.shape[0]
    assert b1.shape[0] == Mc and a2.shape[0] == Mc and b2.shape[0] == Mc
    assert tuple(out1.shape) == (a1.shape[1], b1.shape[1]) and tuple(out2.shape) == (a2.shape[1], b2.shape[1])
    flops = 2.0 * Mc * (a1.shape[1] * b1.shape[1] + a2.shape[1] * b2.shape[1])
    nbytes = 2.0 * Mc * (a1.shape[1] + b1.shape[1] + a2.shape[1] + b2.shape[1]) + 4.0 * (out1.numel() + out2.numel())
    with _Span("gemm_tn_atomic", flops, nbytes):
        ws = tn_pair_workspace(a1.device, a1.shape[1], b1.shape[1], a2.shape[1], b2.shape[1]) if workspace else None
        _call("ccd_gemm_tn_pair_ws", a1, a1.stride(0), b1, b1.stride(0), a1.shape[1], b1.shape[1], out1, out1.stride(0), a2, a2.stride(0),
              b2, b2.stride(0), a2.shape[1], b2.shape[1], out2, out2.stride(0), Mc, ws, ws.numel() if ws is not None else 0)


def gemm_tn(a, b, out, *, accumulate=True, alpha=1.0, splits=0, d_rows=None, rows_mul=1):
    """out[P,Q] (+)= a[Mc,P]^T @ b[Mc,Q]  (fp32 out; accumulate=True adds with fp32 atomics, split over Mc)."""
    Mc, Pd = a.shape
    Q = b.shape[1]
    assert b.shape[0] == Mc and tuple(out.shape) == (Pd, Q)
    with _Span("gemm_tn_" + ("atomic" if accumulate else "f32"), 2.0 * Mc * Pd * Q, 2.0 * Mc * (Pd + Q) + 4.0 * Pd * Q,
               when=d_rows is None):
        _call("ccd_gemm_tn", a, a.stride(0), b, b.stride(0), Pd, Q, Mc, EPI_ATOMIC if accumulate else EPI_F32, out, out.stride(0),
              float(alpha), int(splits) if accumulate else 1, d_rows, int(rows_mul))
    return out


def ln_fwd(x, gamma, beta, eps=1e-6):
    """x [rows,E] fp32 -> (y bf16, mean, rstd)."""
    rows, E = x.shape
    y = torch.empty((rows, E), dtype=BF16, device=x.device)
    mean = torch.empty(rows, dtype=F32, device=x.device)
    rstd = torch.empty(rows, dtype=F32, device=x.device)
    with _Span("layernorm_fwd", 8.0 * rows * E, 6.0 * rows * E):
        _call("ccd_ln_fwd", x, gamma, beta, y, mean, rstd, rows, E, float(eps))
    return y, mean, rstd


def ln_bwd(dy, x, mean, rstd, gamma, g, dgamma, dbeta, accumulate=True, gb=None, rowscale=None, rows_per_sample=1,
           dbias=None):
    """g (+)= LN'(dy); dgamma += , dbeta += (in place).  Optional fused tail: gb = bf16(g * rowscale), dbias += colsum(gb)."""
    g16 = g.dtype == BF16
    rows, E = x.shape
    gbytes = 2.0 if g16 else 4.0
    with _Span("layernorm_bwd", 16.0 * rows * E, rows * E * (6.0 + (2 * gbytes if accumulate else gbytes) + (2.0 if gb is not None else 0.0))):
        _call("ccd_ln_bwd_g16" if g16 else "ccd_ln_bwd", dy, x, mean, rstd, gamma, g, 1 if accumulate else 0, dgamma, dbeta, gb, rowscale,
              int(rows_per_sample), dbias, rows, E)
    return g


def attention_fwd(qkv, heads, scale):
    """qkv [views,256,3*E] bf16 -> (out [views,256,E] bf16, lse [views,heads,256] fp32)."""
    views, T, E3 = qkv.shape
    assert T == 256 and E3 == 3 * heads * 64 and qkv.is_contiguous()
    out = torch.empty((views, T, E3 // 3), dtype=BF16, device=qkv.device)
    lse = torch.empty((views, heads, T), dtype=F32, device=qkv.device)
    # per (view, head): S = Q K^T and O = P V, 2 * 256 * 256 * 64 flop each; q, k, v read and o written once
    with _Span("attention_fwd", views * heads * 4.0 * T * T * 64, views * heads * (4.0 * T * 64 * 2 + 4.0 * T)):
        _call("ccd_attention_fwd", qkv, out, lse, views, heads, float(scale))
    return out, lse


def attention_probs(qkv, heads, scale):
    """qkv [views,256,3*E] bf16 -> the attention probabilities softmax(q k^T * scale), fp32 [views,heads,256,256] (inspection:
    get_last_selfattention; the training path never materialises them)."""
    if qkv.dim() != 3 or qkv.shape[1] != 256 or qkv.shape[2] != 3 * 64 * heads or not qkv.is_contiguous():
        raise ValueError(f"attention_probs: qkv must be a contiguous [views, 256, 3 * 64 * heads] tensor, got {tuple(qkv.shape)} "
                         f"with heads={heads}")
    views, T = qkv.shape[0], qkv.shape[1]
    probs = torch.empty((views, heads, T, T), dtype=F32, device=qkv.device)
    # per (view, head): S = Q K^T, 2 * 256 * 256 * 64 flop; q and k read once, P written once
    with _Span("attention_probs", views * heads * 2.0 * T * T * 64, views * heads * (2.0 * T * 64 * 2 + 4.0 * T * T)):
        _call("ccd_attention_probs", qkv, probs, views, heads, float(scale))
    return probs


def attention_bwd(qkv, out, d_out, lse, heads, scale, d_bias=None, dout_colsum=None, dout_colsum_mat=None):
    """-> d_qkv bf16 [views,256,3E].  d_bias (fp32 [3E], optional): += the qkv-bias gradient (column sums of d_qkv) without a
    pass over d_qkv - q part inside the dQ kernel, k part identically 0, v part = colsum(d_out) = `dout_colsum` [E], or
    `dout_colsum` [E] @ `dout_colsum_mat` [E, E] when the caller knows d_out = gb @ mat (see include/ccd_hip.h)."""
    assert qkv.is_contiguous() and out.is_contiguous() and d_out.is_contiguous()
    views = qkv.shape[0]
    d_qkv = torch.empty_like(qkv)
    delta = torch.empty_like(lse)
    ws = None
    if d_bias is not None:
        assert d_bias.numel() == qkv.shape[2] and d_bias.is_contiguous() and dout_colsum is not None
        assert dout_colsum.numel() == qkv.shape[2] // 3 and dout_colsum.is_contiguous()
        ws = torch.empty(int(_lib.get().ccd_attention_bwd_ws_floats(views, heads)), dtype=F32, device=qkv.device)
    # five products (S, dP, dV, dK, dQ) of 2 * 256 * 256 * 64 flop per (view, head); q, k, v, o, dO read and dq, dk, dv written once
    with _Span("attention_bwd", views * heads * 10.0 * 256 * 256 * 64, views * heads * (8.0 * 256 * 64 * 2 + 8.0 * 256)):
        _call("ccd_attention_bwd", qkv, out, d_out, lse, delta, d_qkv, views, heads, float(scale), d_bias, ws, dout_colsum,
              *_ld(dout_colsum_mat))
    return d_qkv


U8, I32 = torch.uint8, torch.int32


# ------------------------------------------------------------------------------------------ patch embed & helpers
def patch_embed_fwd(img, w, bias, pos, out=None):
    views, E = img.shape[0], w.shape[0]
    assert img.dtype == F32 and img.is_contiguous() and tuple(img.shape[1:]) == (3, 32, 128)
    if out is None:
        out = torch.empty((views * 256, E), dtype=F32, device=img.device)
    _call("ccd_patch_embed_fwd", img, w, bias, pos, out, views, E)
    return out


def patch_embed_bwd(img, g, d_w, d_bias, d_pos):
    views, E = img.shape[0], g.shape[-1]
    assert img.dtype == F32 and img.is_contiguous() and g.dtype in (F32, BF16) and g.is_contiguous()
    ws_p = torch.empty((views * 256, 48), dtype=BF16, device=g.device)
    if g.dtype == BF16:
        _call("ccd_patch_embed_bwd_g16", img, g, d_w, d_bias, d_pos, ws_p, views, E)
        return
    ws_g = torch.empty((views * 256, E), dtype=BF16, device=g.device)
    _call("ccd_patch_embed_bwd", img, g, d_w, d_bias, d_pos, ws_g, ws_p, views, E)


def small_matmul(a, b, out, trans_a=False, accumulate=False):
    """out[M,N] (+)= op(a) @ b, fp32."""
    K, N = b.shape
    M = a.shape[1] if trans_a else a.shape[0]
    _call("ccd_small_matmul_f32", a, b, out, M, N, K, int(trans_a), int(accumulate))
    return out


def colsum_bf16(x, out, d_rows=None, rows_mul=1):
    rows, N = x.shape
    _call("ccd_colsum_bf16", x, x.stride(0), rows, N, d_rows, int(rows_mul), out)
    return out


def cast_bf16(src, dst):
    _call("ccd_cast_bf16", src, dst, src.numel())
    return dst


def scale_cast_rows(src, dst, rowscale=None, rows_per_sample=1):
    rows, E = src.shape
    _call("ccd_scale_cast_rows", src, dst, rowscale, int(rows_per_sample), rows, E)
    return dst


def mirror_bf16(descs_dev, ndesc, total_tiles):
    _call("ccd_mirror_bf16", descs_dev, ndesc, total_tiles)


# ------------------------------------------------------------------------------------------ character-region path
def ccl_label(mask):
    """mask [B,32,128] fp32 (nonzero = text) -> uint8 id map [B,32,128] (255 = background)."""
    assert mask.dtype == F32 and mask.is_contiguous() and tuple(mask.shape[1:]) == (32, 128)
    out = torch.empty(mask.shape, dtype=U8, device=mask.device)
    _call("ccd_ccl_label", mask, out, mask.shape[0])
    return out


def mask_to_idmap(mask):
    out = torch.empty(mask.shape, dtype=U8, device=mask.device)
    _call("ccd_mask_to_idmap", mask, out, mask.shape[0])
    return out


def seg_to_mask(seg_logits, images):
    out = torch.empty((images, 32, 128), dtype=F32, device=seg_logits.device)
    _call("ccd_seg_to_mask", seg_logits, out, images)
    return out


def kmeans2_mask(grays, device=None):
    """Text masks of word images (clusterpixels(im, 2), mask_create/generate_mask.py:13-29) for a list of uint8 [h, w] gray
    images of any sizes -> list of uint8 [h, w] 0/1 arrays (numpy).  One workgroup per image of the ragged batch."""
    import numpy as np
    if not grays:
        return []
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    arrs = [np.ascontiguousarray(np.asarray(g, dtype=np.uint8)) for g in grays]
    for a in arrs:
        assert a.ndim == 2 and a.size > 0, "kmeans2_mask expects non-empty [h, w] gray images"
    sizes = np.array([a.size for a in arrs], dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    hw = np.array([a.shape for a in arrs], dtype=np.int32).reshape(-1)
    flat = torch.from_numpy(np.concatenate([a.reshape(-1) for a in arrs])).to(dev)
    d_offs, d_hw = torch.from_numpy(offs).to(dev), torch.from_numpy(hw).to(dev)
    out = torch.empty_like(flat)
    _call("ccd_kmeans2_mask", flat, d_offs, d_hw, out, len(arrs))
    host = out.cpu().numpy()
    return [host[offs[i]:offs[i + 1]].reshape(arrs[i].shape) for i in range(len(arrs))]


def augment_views(img, params, theta, mean, std, overlay=None, warp_maps=None):
    """img uint8 [B,H,W,3] (resized samples), params fp32 [B,2,96], theta fp32 [B,3,3] -> image_tensors fp32 [B,3,3,H,W]:
    (plain, colour-augmented, colour-augmented + warped by theta), normalised - the dataset's batch contract
    (datasetsupervised_kmeans.py:48-87).  The neighbourhood members (JPEG, blurs, convolutions) run in a pre-pass that stages
    one uint8 image per (sample, view).  overlay: fp16 [layers, 2, H, W] (alpha, intensity) cloud layers that rows with a `weather`
    member refer to (ccd_amd/dataset/weather.py), blended at the end of the pre-pass.  warp_maps: fp32 [maps, 2, H, W] source
    positions of the piecewise-affine warps that view-2 rows with params[84] = m > 0 take instead of theta (map m - 1)."""
    import ctypes as C
    assert img.dtype == U8 and img.is_contiguous() and img.dim() == 4 and img.shape[3] == 3
    B, H, W, _ = img.shape
    assert tuple(params.shape) == (B, 2, 96) and tuple(theta.shape) == (B, 3, 3) and params.is_contiguous()
    out = torch.empty((B, 3, 3, H, W), dtype=F32, device=img.device)
    staged = torch.empty((B, 2, H, W, 3), dtype=U8, device=img.device)
    m3, s3 = (C.c_float * 3)(*[float(v) for v in mean]), (C.c_float * 3)(*[float(v) for v in std])
    layers = 0
    if overlay is not None:
        assert overlay.dtype == torch.float16 and overlay.is_contiguous() and tuple(overlay.shape[1:]) == (2, H, W)
        layers = overlay.shape[0]
    maps = 0
    if warp_maps is not None:
        assert warp_maps.dtype == F32 and warp_maps.is_contiguous() and tuple(warp_maps.shape[1:]) == (2, H, W)
        maps = warp_maps.shape[0]
    _call("ccd_augment_views", img, params, theta, out, staged, B, H, W, m3, s3, overlay, int(layers), warp_maps, int(maps))
    return out


def warp_idmap(src, theta):
    """src uint8 [B,32,128], theta fp32 [B,3,3] (or [B,2,3]) -> warped id map (view 2)."""
    assert src.dtype == U8 and src.is_contiguous() and theta.dtype == F32 and theta.is_contiguous()
    out = torch.empty_like(src)
    _call("ccd_warp_idmap", src, theta, theta.stride(0), out, src.shape[0])
    return out


def region_stats(idmap):
    views = idmap.shape[0]
    dev = idmap.device
    tok_plane = torch.empty((views, 256, 4), dtype=U8, device=dev)      # up to 4 (plane, coefficient) pairs per token
    tok_coef = torch.empty((views, 256, 4), dtype=F32, device=dev)
    present = torch.empty((views, 26), dtype=U8, device=dev)
    _call("ccd_region_stats", idmap, tok_plane, tok_coef, present, views)
    return tok_plane, tok_coef, present


def select_scan(present, batch):
    dev = present.device
    nsel = torch.empty(batch, dtype=I32, device=dev)
    offset = torch.empty(batch, dtype=I32, device=dev)
    total = torch.empty(1, dtype=I32, device=dev)
    new_index = torch.empty((batch, 26), dtype=U8, device=dev)
    _call("ccd_select_scan", present, batch, nsel, offset, total, new_index)
    return nsel, offset, total, new_index


def region_pool_fwd(feat, tok_plane, tok_coef, nsel, offset, total, rows, batch):
    E = feat.shape[-1]
    _call("ccd_region_pool_fwd", feat, tok_plane, tok_coef, nsel, offset, total, rows, batch, E)
    return rows


def region_pool_bwd(d_rows, tok_plane, tok_coef, nsel, offset, total, d_feat, batch):
    E = d_feat.shape[-1]
    _call("ccd_region_pool_bwd", d_rows, tok_plane, tok_coef, nsel, offset, total, d_feat, batch, E)
    return d_feat


def idmap_to_planes(idmap):
    out = torch.empty((idmap.shape[0], 26, 32, 128), dtype=F32, device=idmap.device)
    _call("ccd_idmap_to_planes", idmap, out, idmap.shape[0])
    return out


def planes_to_idmap(planes):
    planes = planes.contiguous().float()
    out = torch.empty((planes.shape[0], 32, 128), dtype=U8, device=planes.device)
    _call("ccd_planes_to_idmap", planes, out, planes.shape[0])
    return out


# ------------------------------------------------------------------------------------------ Dino/utils/DBSCAN.py clusterers
def dbscan_label(mask):
    """DBSCAN_cluster: mask [B,32,128] fp32 (foreground = x > 0.1f) -> uint8 id map [B,32,128] (255 = none)."""
    assert mask.dtype == F32 and mask.is_contiguous() and tuple(mask.shape[1:]) == (32, 128)
    out = torch.empty(mask.shape, dtype=U8, device=mask.device)
    _call("ccd_dbscan_label", mask, out, mask.shape[0])
    return out


def region_boxes(mask):
    """region_cluster: mask [B,32,128] fp32 (nonzero = foreground) -> (boxes int32 [B,26,4] as ymin, xmin, ymax, xmax with
    half-open stops, count int32 [B]); slots >= count are zero."""
    assert mask.dtype == F32 and mask.is_contiguous() and tuple(mask.shape[1:]) == (32, 128)
    boxes = torch.empty((mask.shape[0], 26, 4), dtype=I32, device=mask.device)
    count = torch.empty((mask.shape[0],), dtype=I32, device=mask.device)
    _call("ccd_region_boxes", mask, boxes, count, mask.shape[0])
    return boxes, count


def idmap_to_planes_u8(idmap):
    """uint8 id map [B,32,128], 16-byte aligned (the kernel reads 16 pixels per load) -> the reference's uint8 planes
    [B,26,32,128]."""
    assert idmap.dtype == U8 and idmap.is_contiguous() and tuple(idmap.shape[1:]) == (32, 128)
    assert idmap.data_ptr() % 16 == 0, "idmap_to_planes_u8: the id map must start on a 16-byte boundary (pass a fresh or cloned tensor)"
    out = torch.empty((idmap.shape[0], 26, 32, 128), dtype=U8, device=idmap.device)
    _call("ccd_idmap_to_planes_u8", idmap, out, idmap.shape[0])
    return out


def boxes_to_planes_u8(boxes, count):
    """region_boxes' (boxes [B,26,4], count [B]) int32 -> the reference's uint8 planes [B,26,32,128] (filled boxes)."""
    assert boxes.dtype == I32 and boxes.is_contiguous() and boxes.dim() == 3 and tuple(boxes.shape[1:]) == (26, 4)
    assert count.dtype == I32 and count.is_contiguous() and tuple(count.shape) == (boxes.shape[0],)
    out = torch.empty((boxes.shape[0], 26, 32, 128), dtype=U8, device=boxes.device)
    _call("ccd_boxes_to_planes_u8", boxes, count, out, boxes.shape[0])
    return out


# ------------------------------------------------------------------------------------------ Dino/metric/eval_superpixel.py metrics
F64 = torch.float64
SSIM_MAX_WINDOW = 15


def _plane_strides(x):
    """(N stride, C stride) of an fp32 [N, C, H, W] tensor whose rows are contiguous with stride W (what the kernels read)."""
    assert x.dtype == F32 and x.dim() == 4
    assert x.stride(3) == 1 or x.shape[3] == 1, "rows must be contiguous"
    assert x.stride(2) == x.shape[3] or x.shape[2] == 1, "rows must follow each other with stride W"
    return x.stride(0), x.stride(1)


def _ssim_inputs(imgs):
    """ctypes arguments (x, n stride, c stride) x 3 for 2 or 3 same-shape inputs; a missing third input is NULL."""
    assert len(imgs) in (2, 3) and all(tuple(x.shape) == tuple(imgs[0].shape) for x in imgs)
    args = []
    for i in range(3):
        if i < len(imgs):
            args += [imgs[i], *_plane_strides(imgs[i])]
        else:
            args += [None, 0, 0]
    return args


def _taps_arg(window, taps):
    assert window % 2 == 1 and 1 <= window <= SSIM_MAX_WINDOW and len(taps) == window
    return (ctypes.c_float * window)(*taps)


def ssim_fwd(imgs, window, taps, size_average):
    """SSIM (2 inputs) / TRI_SSIM (3 inputs) of fp32 [N, C, H, W] images -> (per-image mean fp32 [N], batch mean fp32 0-dim or None).
    taps: the window's 1-D Gaussian (host floats)."""
    N, C, H, W = imgs[0].shape
    dev = imgs[0].device
    per = torch.empty((N,), dtype=F32, device=dev)
    mean = torch.empty((), dtype=F32, device=dev) if size_average else None
    if N == 0:
        return per, (mean.fill_(float("nan")) if size_average else None)
    nws = _lib.get().ccd_ssim_ws_doubles(N, C, H, W)
    if nws < 0:
        raise ValueError(f"ssim: unsupported shape {[N, C, H, W]}")
    ws = torch.empty((nws,), dtype=F64, device=dev)
    t = _taps_arg(window, taps)
    _call("ccd_ssim_fwd", *_ssim_inputs(imgs), N, C, H, W, window, t, ws)
    _call("ccd_ssim_reduce", ws, N, C, H, W, per, mean)
    return per, mean


def ssim_bwd(imgs, window, taps, gscale, need):
    """Gradients of sum_n gscale[n] * (sum of image n's map) w.r.t. the inputs with need[i]: contiguous fp32 [N, C, H, W] or None."""
    N, C, H, W = imgs[0].shape
    assert gscale.dtype == F32 and gscale.is_contiguous() and tuple(gscale.shape) == (N,)
    dx = [torch.empty((N, C, H, W), dtype=F32, device=x.device) if need[i] else None for i, x in enumerate(imgs)]
    dx += [None] * (3 - len(dx))
    if N and any(d is not None for d in dx):
        t = _taps_arg(window, taps)
        _call("ccd_ssim_bwd", *_ssim_inputs(imgs), N, C, H, W, window, t, gscale, dx[0], dx[1], dx[2])
    return dx[:len(imgs)]


def psnr_fwd(a, b):
    """calculate_psnr's sums on channels 0..min(C, 3)-1 of fp32 [N, C, H, W] a, b -> (psnr fp32 0-dim, mse fp64 0-dim), on the device."""
    assert tuple(a.shape) == tuple(b.shape)
    N, C, H, W = a.shape
    ch = min(C, 3)
    psnr = torch.empty((), dtype=F32, device=a.device)
    mse = torch.empty((), dtype=F64, device=a.device)
    if N == 0:
        return psnr.fill_(float("nan")), mse.fill_(float("nan"))
    nws = _lib.get().ccd_psnr_ws_doubles(N, ch, H, W)
    if nws < 0:
        raise ValueError(f"calculate_psnr: unsupported shape {[N, C, H, W]}")
    ws = torch.empty((nws,), dtype=F64, device=a.device)
    _call("ccd_psnr_fwd", a, *_plane_strides(a), b, *_plane_strides(b), N, ch, H, W, ws, mse, psnr)
    return psnr, mse


# ------------------------------------------------------------------------------------------ Dino/metric/eval_IOU.py metrics
SEG_CLASSES = 32             # labels are integers in [0, 32) (ccd_hip.h: CCD_SEG_CLASSES)
SEG_CHUNK = 4096             # pixels of one image per workgroup (segmetric.h: SEG_CHUNK); larger images are split
SEG_WAVE_PIXELS = (256, 1024)    # pixels a wavefront loads per step: 4 per lane, 16 per lane for two aligned uint8 maps
SEG_SCORES = ("pixel_accuracy", "mean_accuracy", "mean_IU", "fore_IU", "frequency_weighted_IU")
SEG_DTYPES = {torch.uint8: 0, torch.int32: 1, torch.int64: 2, torch.float32: 3}      # ccd_hip.h: CCD_SEG_U8 ..


def _seg_map(x, name):
    """A label map [B, H, W] (or [B, pixels]) -> (tensor read in place, dtype code, image stride, pixels).  bool goes through a
    uint8 view; the pixels of an image must be contiguous (a copy is made otherwise), the image stride is free."""
    if x.dtype == torch.bool:
        x = x.view(torch.uint8)
    if x.dtype not in SEG_DTYPES:
        raise TypeError(f"{name}: label maps are uint8, bool, int32, int64 or float32, got {str(x.dtype)[6:]}")
    if x.dim() not in (2, 3):
        raise ValueError(f"{name}: expects [B, H, W] label maps, got {list(x.shape)}")
    pixels = x[0].numel() if x.shape[0] else math.prod(x.shape[1:])
    if x.shape[0] and not x[0].is_contiguous():
        x = x.contiguous()
    return x, SEG_DTYPES[x.dtype], (x.stride(0) if x.shape[0] > 1 else pixels), pixels


def _seg_outputs(images, dev):
    return (torch.empty((images, SEG_CLASSES, SEG_CLASSES), dtype=I32, device=dev), torch.empty((images,), dtype=I32, device=dev))


def seg_confusion(eval_segm, gt_segm):
    """Label maps [B, H, W] -> (cm int32 [B, 32, 32] with cm[i, g, e] = pixels of gt label g and eval label e, status int32 [B]:
    bit 0 = a label outside [0, 32) / not integral / NaN, not counted)."""
    e, ecode, estride, pixels = _seg_map(eval_segm, "seg_confusion(eval)")
    g, gcode, gstride, gpixels = _seg_map(gt_segm, "seg_confusion(gt)")
    if e.shape[0] != g.shape[0] or pixels != gpixels:
        raise ValueError(f"seg_confusion: the maps differ in shape: {list(eval_segm.shape)} and {list(gt_segm.shape)}")
    cm, status = _seg_outputs(e.shape[0], e.device)
    if e.shape[0]:
        _call("ccd_seg_confusion", e, ecode, estride, g, gcode, gstride, e.shape[0], pixels, cm, status)
    return cm, status


def seg_confusion_logits(logits, gt_segm):
    """The same with eval = argmax over the channels of fp32 logits [B, C, H, W] (2 <= C <= 32, first maximum), read in place:
    image and channel strides are free, the pixels of a channel contiguous."""
    if logits.dtype != F32:
        raise TypeError(f"seg_confusion_logits: logits must be float32, got {str(logits.dtype)[6:]}")
    if logits.dim() not in (3, 4) or not 2 <= logits.shape[1] <= SEG_CLASSES:
        raise ValueError(f"seg_confusion_logits: expects [B, C, H, W] logits with 2 <= C <= {SEG_CLASSES}, got {list(logits.shape)}")
    g, gcode, gstride, pixels = _seg_map(gt_segm, "seg_confusion_logits(gt)")
    B, C = logits.shape[:2]
    if B != g.shape[0] or math.prod(logits.shape[2:]) != pixels:
        raise ValueError(f"seg_confusion_logits: logits {list(logits.shape)} do not match the gt maps {list(gt_segm.shape)}")
    if B and not logits[0, 0].is_contiguous():
        logits = logits.contiguous()
    cm, status = _seg_outputs(B, logits.device)
    if B:
        _call("ccd_seg_confusion_logits", logits, logits.stride(0) if B > 1 else C * pixels, logits.stride(1), C, g, gcode, gstride, B,
              pixels, cm, status)
    return cm, status


def seg_scores(cm, status):
    """cm int32 [B, 32, 32], status int32 [B] (updated in place: bit 1 = fore_IU undefined) -> scores fp64 [B, 5] in the order of
    SEG_SCORES; NaN where undefined."""
    assert cm.dtype == I32 and cm.is_contiguous() and tuple(cm.shape[1:]) == (SEG_CLASSES, SEG_CLASSES)
    assert status.dtype == I32 and status.is_contiguous() and tuple(status.shape) == (cm.shape[0],)
    scores = torch.empty((cm.shape[0], len(SEG_SCORES)), dtype=F64, device=cm.device)
    if cm.shape[0]:
        _call("ccd_seg_scores", cm, status, cm.shape[0], scores)
    return scores


# ------------------------------------------------------------------------------------------ Dino/metric/eval_acc.py scores
TEXT_COLS = 128              # normalised prediction characters per sample (ccd_hip.h: CCD_TEXT_COLS): steps * norm_width <= 128
TEXT_RECORD = ("distance", "equal_chars", "gt_chars", "word_correct")          # the int32 columns of a per-sample record
TEXT_TOTALS = ("correct_char", "total_char", "correct_word", "words", "total_ed", "total_ned")     # int64 x 5, then fp64 bits


def _text_score(who, x, layout, inner, table_raw, table_norm, gt_codes, gt_len, extra=()):
    """What the text_score* wrappers share: the checks, the records and the call of ccd_<who>.  x: the decoder's output, laid out as
    `layout` says - scores whose last axis C is the rows a table needs at least, or decoded paths, where the entry point is told
    how many rows the tables have; inner: what the last axis holds where it must be contiguous; extra: the entry point's arguments
    between the tables and the truth."""
    if x.dim() != layout.count(",") + 1 or gt_codes.dim() != 2 or gt_codes.shape[0] != x.shape[0] or tuple(gt_len.shape) != (x.shape[0],):
        raise ValueError(f"{who}: expects {layout}, gt [B, L] and gt_len [B], got {list(x.shape)}, {list(gt_codes.shape)}, "
                         f"{list(gt_len.shape)}")
    if inner and x.shape[-1] > 1 and x.stride(-1) != 1:
        raise ValueError(f"{who}: the {inner} must be contiguous")
    decoded = x.dim() == 2
    rows = "classes" if decoded else f">= {x.shape[2]}"
    for name, t in (("table_raw", table_raw), ("table_norm", table_norm)):
        if t.dim() != 2 or not t.is_contiguous() or (t.shape[0] != table_raw.shape[0] if decoded else t.shape[0] < x.shape[2]):
            raise ValueError(f"{who}: {name} must be a contiguous [{rows}, width] table, got {list(t.shape)}")
    assert gt_len.is_contiguous()
    records = torch.empty((x.shape[0], len(TEXT_RECORD)), dtype=I32, device=x.device)
    if x.shape[0]:
        _call("ccd_" + who, x, *x.stride()[:-1], *x.shape, *((table_raw.shape[0],) if decoded else ()), table_raw,
              table_raw.shape[1], table_norm, table_norm.shape[1], *extra, gt_codes if gt_codes.shape[1] else None, gt_codes.stride(0),
              gt_codes.shape[1], gt_len, records)
    return records


def text_score(scores, table_raw, table_norm, end_idx, pad_idx, gt_codes, gt_len):
    """Decoder scores fp32 [B, T, C] (any sample / step stride, e.g. probs[:, :done]) against the ground truth as int32 code points
    [B, L] with lengths int32 [B] -> records int32 [B, 4] in the order of TEXT_RECORD.  table_raw / table_norm: int32 [C, width], the
    code points of every class and of its normalised form, rows padded with -1 (AttnConvertor.score_table)."""
    return _text_score("text_score", scores, "scores [B, T, C]", None, table_raw, table_norm, gt_codes, gt_len,
                       (int(end_idx), int(pad_idx)))      # (the decoder has no <PAD> output: the tables hold one row more than C)


def text_totals(device):
    """The accumulator of text_accumulate: int64 [6] zeros, in the order of TEXT_TOTALS (the last one holds an fp64)."""
    return torch.zeros(len(TEXT_TOTALS), dtype=I64, device=device)


def text_accumulate(records, totals):
    """totals (text_totals) += the sums over records [B, 4], in a fixed order; no host synchronisation."""
    assert records.dtype == I32 and records.is_contiguous() and records.dim() == 2 and records.shape[1] == len(TEXT_RECORD)
    assert totals.dtype == I64 and totals.is_contiguous() and tuple(totals.shape) == (len(TEXT_TOTALS),)
    if records.shape[0]:
        _call("ccd_text_accumulate", records, records.shape[0], totals[:5], totals[5:].view(F64))


def text_score_ctc(logits, table_raw, table_norm, gt_codes, gt_len):
    """text_score for the logits fp32 [B, T, C] of a CTC head (any sample / step stride): a frame counts where its arg-max class is
    not the blank (class 0) and differs from the frame before.  Tables as CTCConvertor.score_table gives them; records as text_score."""
    return _text_score("text_score_ctc", logits, "logits [B, T, C]", "classes of a frame", table_raw, table_norm, gt_codes, gt_len)


def text_score_paths(paths, table_raw, table_norm, gt_codes, gt_len):
    """text_score for classes that are already decoded: paths int32 [B, T] (any row stride, e.g. rank 0 of ctc_beam_search's
    paths[:, 0]), a sample's classes in front of its first negative entry.  Tables as CTCConvertor.score_table gives them; records as
    text_score."""
    return _text_score("text_score_paths", paths, "paths [B, T]", "steps of a path", table_raw, table_norm, gt_codes, gt_len)


# ------------------------------------------------------------------------------------------ CTC recognition head (kernels/ctc.h)
CTC_MAX_STEPS, CTC_MAX_CLASSES, CTC_MAX_LABELS, CTC_MAX_BEAM = 64, 128, 31, 16         # ccd_hip.h: CCD_CTC_MAX_*


def ctc_pool_fwd(tokens, rows=8, cols=32):
    """tokens bf16 [N, rows * cols, E] (token = row * cols + column) -> frames bf16 [N * cols, E]: the mean over the rows."""
    if tokens.dim() != 3 or tokens.shape[1] != rows * cols or not tokens.is_contiguous():
        raise ValueError(f"ctc_pool_fwd: expects contiguous tokens [N, {rows * cols}, E], got {list(tokens.shape)}")
    N, _, E = tokens.shape
    frames = torch.empty((N * cols, E), dtype=BF16, device=tokens.device)
    if N:
        _call("ccd_ctc_pool_fwd", tokens, frames, N, rows, cols, E)
    return frames


def ctc_pool_bwd(d_frames, rows=8, cols=32):
    """d_frames bf16 [N * cols, E] -> d_tokens bf16 [N, rows * cols, E] = d_frames / rows at every row."""
    if d_frames.dim() != 2 or d_frames.shape[0] % cols or not d_frames.is_contiguous():
        raise ValueError(f"ctc_pool_bwd: expects contiguous d_frames [N * {cols}, E], got {list(d_frames.shape)}")
    N, E = d_frames.shape[0] // cols, d_frames.shape[1]
    d_tokens = torch.empty((N, rows * cols, E), dtype=BF16, device=d_frames.device)
    if N:
        _call("ccd_ctc_pool_bwd", d_frames, d_tokens, N, rows, cols, E)
    return d_tokens


def _ctc_rows(logits, C, T, targets, name):
    if logits.dim() != 2 or logits.stride(1) != 1 or logits.shape[0] % T or not 1 <= C <= logits.shape[1]:
        raise ValueError(f"{name}: expects logits [B * {T}, >= {C}] with dense rows, got {list(logits.shape)}")
    B = logits.shape[0] // T
    if targets.dim() != 2 or targets.shape[0] != B or not targets.is_contiguous():
        raise ValueError(f"{name}: expects contiguous targets [{B}, Lmax], got {list(targets.shape)}")
    return B


def _ctc_ws_elements(B, T):
    return (_lib.get().ccd_ctc_loss_ws_bytes(B, T) + 7) // 8


def ctc_loss_fwd(logits, C, targets, T):
    """logits fp32 [B * T, ld] (C valid columns, class 0 = blank), targets int64 [B, Lmax] zero-padded
    -> (nll fp32 [B], acc fp32 [3] = {sum nll / max(L, 1) over the feasible samples, B, infeasible samples}, workspace for
    ctc_loss_bwd).  The loss of torch.nn.CTCLoss(reduction='mean', zero_infinity=True) is acc[0] / acc[1]."""
    B = _ctc_rows(logits, C, T, targets, "ctc_loss_fwd")
    nll = torch.empty(B, dtype=F32, device=logits.device)
    acc = torch.zeros(3, dtype=F32, device=logits.device)
    ws = torch.empty(_ctc_ws_elements(B, T), dtype=F64, device=logits.device)
    _call("ccd_ctc_loss_fwd", logits, logits.stride(0), B, T, C, targets if targets.shape[1] else None, targets.shape[1], nll, acc, ws)
    return nll, acc, ws


def ctc_loss_bwd(logits, C, targets, T, ws, upstream=None, ldd=None):
    """-> d_logits bf16 [B * T, ldd] (default ldd: C rounded up to 8): (softmax - class posterior) * upstream / (max(L, 1) * B), zero
    behind column C and for an infeasible sample.  upstream: fp32 device scalar [1] or None (= 1)."""
    B = _ctc_rows(logits, C, T, targets, "ctc_loss_bwd")
    ldd = (C + 7) // 8 * 8 if ldd is None else int(ldd)
    if ws.dtype != F64 or not ws.is_contiguous() or ws.numel() != _ctc_ws_elements(B, T):
        raise ValueError(f"ctc_loss_bwd: ws must be the workspace ctc_loss_fwd returned for B = {B}, T = {T}")
    assert upstream is None or upstream.numel() == 1
    d = torch.empty((B * T, ldd), dtype=BF16, device=logits.device)
    _call("ccd_ctc_loss_bwd", logits, logits.stride(0), B, T, C, targets if targets.shape[1] else None, targets.shape[1], ws, upstream,
          d, ldd)
    return d


def _frame_scores(who, scores, what="scores"):
    """The check every CTC decoder starts with: `what` fp32 [B, T, C] with contiguous classes (any sample / step stride) -> (B, T, C)."""
    if scores.dim() != 3 or (scores.shape[2] > 1 and scores.stride(2) != 1):
        raise ValueError(f"{who}: expects {what} [B, T, C] with contiguous classes, got {list(scores.shape)}, strides {scores.stride()}")
    return scores.shape


def _beam_width(who, beam_width, limit):
    W = int(beam_width)
    if not 1 <= W <= limit:
        raise ValueError(f"{who}: beam_width must lie in 1..{limit}, got {beam_width}")
    return W


def _beam_outputs(B, W, T, device):
    """(paths int32 [B, W, T], lengths int32 [B, W], hyp_scores fp32 [B, W]) for a beam decoder to fill."""
    return (torch.empty((B, W, T), dtype=I32, device=device), torch.empty((B, W), dtype=I32, device=device),
            torch.empty((B, W), dtype=F32, device=device))


def ctc_greedy(logits):
    """logits fp32 [B, T, C] (any sample / step stride) -> (path int32 [B, T] left-aligned, -1-padded; length int32 [B]; conf fp32
    [B, T]): arg-max class per frame (first maximum), repeats collapsed, blanks dropped; conf = the softmax probability of the first
    frame of each kept run."""
    B, T, C = _frame_scores("ctc_greedy", logits, "logits")
    path = torch.empty((B, T), dtype=I32, device=logits.device)
    length = torch.empty(B, dtype=I32, device=logits.device)
    conf = torch.empty((B, T), dtype=F32, device=logits.device)
    _call("ccd_ctc_greedy", logits, logits.stride(0), logits.stride(1), B, T, C, path, length, conf)
    return path, length, conf


def ctc_beam_search(scores, beam_width, normalized=False):
    """CTC prefix beam search (kernels/ctc_beam.h): scores fp32 [B, T, C] (any sample / step stride), logits or - normalized=True -
    probabilities, as CTCDecoder.forward_test returns them -> (paths int32 [B, W, T] by rank, -1-padded; lengths int32 [B, W], -1 for
    an unused slot; hyp_scores fp32 [B, W]: the log of the word's probability summed over the alignments the beam kept, -inf for an
    unused slot).  W = beam_width in 1..CTC_MAX_BEAM."""
    B, T, C = _frame_scores("ctc_beam_search", scores)
    W = _beam_width("ctc_beam_search", beam_width, CTC_MAX_BEAM)
    paths, lengths, hyp_scores = _beam_outputs(B, W, T, scores.device)
    _call("ccd_ctc_beam_search", scores, scores.stride(0), scores.stride(1), B, T, C, 1 if normalized else 0, W, paths, lengths, hyp_scores)
    return paths, lengths, hyp_scores


# ------------------------------------------------------------------------------------------ language-model fusion (kernels/ctc_beam.h)
CTC_LM_MAX_ORDER = 3                                      # ccd_hip.h: CCD_CTC_LM_MAX_ORDER


class CTCCharLM(_OncePerDevice):
    """A character n-gram table for ctc_beam_search_lm (build it with ctc_char_lm): `table` fp32 [C^(order-1), C] on the host; a device
    copy is uploaded once per device."""

    def __init__(self, table, order):
        self.table, self.order, self.classes = table, order, table.shape[1]

    def _upload(self, device):
        return upload(self.table, device)


def ctc_char_lm(table, order):
    """A language-model handle from a host fp32 tensor [C^(order-1), C] (CharNGram.table; order in 1..CTC_LM_MAX_ORDER), built once
    per model.  Row: the last order - 1 classes of a prefix, most recent last, 0 where the prefix is shorter; column c >= 1: the
    log-probability of character c behind that context, column 0: of the word ending there.  Values are finite or -inf; NaN is refused."""
    if not isinstance(table, torch.Tensor) or table.dtype != F32 or table.dim() != 2 or table.device.type != "cpu":
        got = f"{str(table.dtype)[6:]} {list(table.shape)} on {table.device.type}" if isinstance(table, torch.Tensor) else type(table).__name__
        raise ValueError(f"ctc_char_lm: expects a host float32 tensor [C^(order-1), C], got {got}")
    order = int(order)
    if not 1 <= order <= CTC_LM_MAX_ORDER:
        raise ValueError(f"ctc_char_lm: order must lie in 1..{CTC_LM_MAX_ORDER}, got {order}")
    C = table.shape[1]
    if not 2 <= C <= CTC_MAX_CLASSES or table.shape[0] != C ** (order - 1):
        raise ValueError(f"ctc_char_lm: an order-{order} table over C classes (2..{CTC_MAX_CLASSES}) has shape [C^{order - 1}, C], "
                         f"got {list(table.shape)}")
    if bool(torch.isnan(table).any()) or bool((table == float("inf")).any()):
        raise ValueError("ctc_char_lm: the table holds NaN or +inf (entries are log-probabilities: finite or -inf)")
    return CTCCharLM(table.contiguous(), order)


def ctc_beam_search_lm(scores, beam_width, lm, weight=1.0, bonus=0.0, eos=False, normalized=False):
    """CTC prefix beam search fused with a character n-gram language model (kernels/ctc_beam.h: ctc_beam_kernel<CTC_BEAM_LM>): scores and
    beam_width as ctc_beam_search, lm a ctc_char_lm handle -> (paths, lengths, hyp_scores) shaped as ctc_beam_search returns them.
    Every extension of a prefix by character c adds weight * lm[row, c] + bonus to the candidate (-inf where the table says so), so a
    hypothesis scores log p_ctc(word | kept alignments) + weight * sum lm + bonus * len(word); eos=True adds weight * lm[row, 0] behind
    the last frame and ranks the hypotheses again (a -inf one becomes an unused slot).  weight = 0, bonus = 0 and a finite table give
    ctc_beam_search's result bit for bit."""
    B, T, C = _frame_scores("ctc_beam_search_lm", scores)
    if not isinstance(lm, CTCCharLM):
        raise TypeError(f"ctc_beam_search_lm: lm must come from ctc_char_lm, got {type(lm).__name__}")
    if lm.classes != C:
        raise ValueError(f"ctc_beam_search_lm: the table was built for {lm.classes} classes, the scores have {C}")
    W = _beam_width("ctc_beam_search_lm", beam_width, CTC_MAX_BEAM)
    paths, lengths, hyp_scores = _beam_outputs(B, W, T, scores.device)
    _call("ccd_ctc_beam_search_lm", scores, scores.stride(0), scores.stride(1), B, T, C, 1 if normalized else 0, W, lm.on(scores.device),
          lm.order, float(weight), float(bonus), 1 if eos else 0, paths, lengths, hyp_scores)
    return paths, lengths, hyp_scores


# ------------------------------------------------------------------------------------------ lexicon decoding (kernels/ctc_lexicon.h)
CTC_LEXICON_MAX_NBEST = 16                                # ccd_hip.h: CCD_CTC_LEXICON_MAX_NBEST
CTC_LEXICON_CLASSES = (7, 15, CTC_MAX_LABELS)             # longest word of a length class: 16 / 32 / 64 lanes per word


class CTCLexicon(_OncePerDevice):
    """A word list for ctc_lexicon_score (build it with ctc_lexicon): `words` int64 [V, max_len] on the host, in the caller's order;
    a device copy in that order and up to three length-class slices (L <= 7, <= 15, <= 31), each (words int64 [n, class width],
    columns int32 [n]), are uploaded once per device."""

    def __init__(self, words):
        self.words = words
        self.lengths = (words != 0).to(I64).cumprod(dim=1).sum(dim=1) if words.shape[0] else torch.zeros(0, dtype=I64)

    def __len__(self):
        return self.words.shape[0]

    def _upload(self, device):
        """(words on `device`, [(slice words, columns)])"""
        slices, lo = [], -1
        for hi in CTC_LEXICON_CLASSES:
            cols = torch.nonzero((self.lengths > lo) & (self.lengths <= hi)).flatten()
            lo = hi
            if cols.numel():
                width = min(hi, self.words.shape[1])
                slices.append((upload(self.words[cols][:, :width].contiguous(), device), upload(cols.to(I32), device)))
        return upload(self.words, device), slices


def ctc_lexicon(words):
    """A lexicon handle from a host int64 [V, max_len] tensor of zero-padded classes (CTCConvertor.str2tensor's layout; max_len in
    1..CTC_MAX_LABELS), built once per lexicon.  An all-zero row is the empty word; a row's word ends at its first zero."""
    if not isinstance(words, torch.Tensor) or words.dtype != I64 or words.dim() != 2 or words.device.type != "cpu":
        got = f"{str(words.dtype)[6:]} {list(words.shape)} on {words.device.type}" if isinstance(words, torch.Tensor) else type(words).__name__
        raise ValueError(f"ctc_lexicon: expects a host int64 tensor [V, max_len], got {got}")
    if not 1 <= words.shape[1] <= CTC_MAX_LABELS:
        raise ValueError(f"ctc_lexicon: max_len must lie in 1..{CTC_MAX_LABELS}, got {words.shape[1]}")
    return CTCLexicon(words.contiguous())


def ctc_lexicon_score(scores, lexicon, normalized=False, subset=None):
    """log p(word | frames) of every word of a lexicon (kernels/ctc_lexicon.h): scores fp32 [B, T, C] (any sample / step stride), logits
    or - normalized=True - probabilities; lexicon: a ctc_lexicon handle -> fp32 [B, V], the CTC forward log-likelihood summed over
    all alignments, -inf for a word no alignment of finite probability spells (a class outside [1, C), more characters than frames, a
    masked class).  subset int32 [B, K]: sample b scores only the words subset[b, k] -> fp32 [B, K], -inf where an entry is negative
    (padding) or >= V."""
    B, T, C = _frame_scores("ctc_lexicon_score", scores)
    if not isinstance(lexicon, CTCLexicon):
        raise TypeError(f"ctc_lexicon_score: lexicon must come from ctc_lexicon, got {type(lexicon).__name__}")
    V = len(lexicon)
    words, slices = lexicon.on(scores.device)
    flag = 1 if normalized else 0
    if subset is not None:
        if subset.dim() != 2 or subset.shape[0] != B or not subset.is_contiguous():
            raise ValueError(f"ctc_lexicon_score: expects a contiguous subset [{B}, K], got {list(subset.shape)}")
        K = subset.shape[1]
        out = torch.full((B, K), float("-inf"), dtype=F32, device=scores.device)
        if V and K:
            _call("ccd_ctc_lexicon_score", scores, scores.stride(0), scores.stride(1), B, T, C, flag, words, V, words.shape[1], None, subset,
                  K, out, K)
        return out
    out = torch.empty((B, V), dtype=F32, device=scores.device)
    for part, columns in slices:                                 # every column belongs to exactly one length class
        _call("ccd_ctc_lexicon_score", scores, scores.stride(0), scores.stride(1), B, T, C, flag, part, part.shape[0], part.shape[1],
              columns, None, 0, out, V)
    return out


def ctc_lexicon_best(word_scores, nbest=1):
    """word_scores fp32 [B, V] (any row stride) -> (index int32 [B, nbest], score fp32 [B, nbest]): the best columns of every row by
    (score descending, column ascending); -inf is never selected, a slot left over holds index -1 and score -inf."""
    if word_scores.dim() != 2 or (word_scores.shape[1] > 1 and word_scores.stride(1) != 1):
        raise ValueError(f"ctc_lexicon_best: expects word_scores [B, V] with contiguous columns, got {list(word_scores.shape)}, strides "
                         f"{word_scores.stride()}")
    n = int(nbest)
    if not 1 <= n <= CTC_LEXICON_MAX_NBEST:
        raise ValueError(f"ctc_lexicon_best: nbest must lie in 1..{CTC_LEXICON_MAX_NBEST}, got {nbest}")
    B, V = word_scores.shape
    index = torch.empty((B, n), dtype=I32, device=word_scores.device)
    best = torch.empty((B, n), dtype=F32, device=word_scores.device)
    ld = word_scores.stride(0) if B > 1 else V                  # (the stride of a single row says nothing)
    _call("ccd_ctc_lexicon_best", word_scores if V else None, ld, B, V, n, index, best)
    return index, best


# ------------------------------------------------------------------------------------------ trie search over a lexicon (kernels/ctc_beam.h)
CTC_TRIE_NODE_WORDS = 8                                   # ccd_hip.h: int32 words per node of ccd_ctc_beam_search_trie's table


class CTCLexiconTrie(_OncePerDevice):
    """The prefix tree of a lexicon for ctc_beam_search_trie / ctc_lexicon_search (build it with ctc_lexicon_trie): `nodes` int32
    [n_nodes, 8] on the host (the layout: ctc_lexicon_trie), `lexicon` the CTCLexicon it was built from, `stats` = {'nodes', 'bytes',
    'terminals'}; a device copy is uploaded once per device."""

    def __init__(self, lexicon, nodes):
        self.lexicon, self.nodes, self.n_nodes = lexicon, nodes, nodes.shape[0]
        self.stats = {"nodes": self.n_nodes, "bytes": self.n_nodes * CTC_TRIE_NODE_WORDS * 4, "terminals": int((nodes[:, 5] >= 0).sum())}

    def _upload(self, device):
        return upload(self.nodes, device)


def _trie_nodes(words):
    """words int64 numpy [V, max_len], zero-padded -> int32 numpy [n_nodes, 8], breadth-first.  Vectorised: the distinct words are
    sorted once (a prefix sorts in front of its extensions, the padding being 0), so the nodes of a depth are the rows at which the
    first `depth` columns change, in breadth-first order already; one pass per depth."""
    V, L = words.shape
    ended = np.cumsum(words == 0, axis=1) > 0
    w = np.where(ended, 0, words)                                    # a word ends at its first zero
    inside = ((w >= 0) & (w < 128)).all(axis=1)                      # a class outside 1..127 has no mask bit: the word is unreachable
    rows = np.flatnonzero(inside)
    uniq, first_row = np.unique(w[rows], axis=0, return_index=True) if rows.size else (np.zeros((0, L), np.int64), np.zeros(0, np.int64))
    word_row = rows[first_row] if rows.size else first_row           # of duplicate rows the lowest (np.unique: the first occurrence)
    N = uniq.shape[0]
    length = (uniq != 0).sum(axis=1)
    differs = np.ones(N, dtype=np.int64) * 0                         # the first column in which a row differs from the row before it
    if N > 1:
        differs[1:] = np.argmax(uniq[1:] != uniq[:-1], axis=1)
    mask, first, word, parent, edge = [np.zeros((1, 4), np.uint32)], [np.zeros(1, np.int64)], [np.full(1, -1, np.int64)], \
        [np.full(1, -1, np.int64)], [np.zeros(1, np.int64)]
    if N and length[0] == 0:
        word[0][0] = word_row[0]                                     # the empty word: the root is terminal
    above = np.zeros(N, dtype=np.int64)                              # the node of every row's prefix one level up: the root
    base = 1
    for depth in range(1, L + 1):
        new = (length >= depth) & (differs < depth)
        count = int(new.sum())
        if not count:
            break
        node = base + np.cumsum(new) - 1                             # of the row's prefix of `depth` classes (where length >= depth)
        at = np.flatnonzero(new)
        p, c = above[at], uniq[at, depth - 1]
        m = np.zeros((count, 4), np.uint32)
        f = np.zeros(count, np.int64)
        wd = np.full(count, -1, np.int64)
        ends = np.flatnonzero(length == depth)                       # (such a row opens its node: it sorts in front of its extensions)
        wd[node[ends] - base] = word_row[ends]
        mask.append(m), first.append(f), word.append(wd), parent.append(p), edge.append(c)
        # the parents' side: their mask bits and first children (parents ascend along `at`: the first occurrence is the lowest class)
        level = len(mask) - 2
        start = base - mask[level].shape[0]
        np.bitwise_or.at(mask[level], (p - start, c >> 5), (np.uint32(1) << (c & 31).astype(np.uint32)))
        which, where = np.unique(p, return_index=True)
        first[level][which - start] = base + where
        above = np.where(length >= depth, node, 0)
        base += count
    nodes = np.zeros((base, CTC_TRIE_NODE_WORDS), dtype=np.int32)
    nodes[:, :4] = np.concatenate(mask).view(np.int32)
    nodes[:, 4], nodes[:, 5], nodes[:, 6], nodes[:, 7] = np.concatenate(first), np.concatenate(word), np.concatenate(parent), np.concatenate(edge)
    return nodes


def ctc_lexicon_trie(lexicon):
    """The prefix tree of a ctc_lexicon handle, built once per lexicon on the host -> CTCLexiconTrie.  nodes int32 [n_nodes, 8], 32
    bytes per node: words 0..3 the 128-bit child mask (bit c & 31 of word c >> 5 is set iff the node has a child by class c; bit 0
    never), 4 first_child (the node of the child with the lowest class), 5 word_id (the row of lexicon.words that ends here - of
    duplicate rows the lowest - or -1), 6 the parent (-1 for the root), 7 the class on the edge from the parent (0 for the root).
    Breadth-first: the root is node 0, the children of a node are contiguous in ascending class order, so the child by class c is
    first_child + popcount(mask bits below c).  An all-zero row makes the root terminal; an empty lexicon is the root alone.  A word
    with a class outside 1..127 is left out: no scores have such a class."""
    if not isinstance(lexicon, CTCLexicon):
        raise TypeError(f"ctc_lexicon_trie: lexicon must come from ctc_lexicon, got {type(lexicon).__name__}")
    return CTCLexiconTrie(lexicon, torch.from_numpy(_trie_nodes(lexicon.words.numpy())))


def ctc_beam_search_trie(scores, beam_width, trie, normalized=False):
    """CTC prefix beam search along the prefix tree of a lexicon (kernels/ctc_beam.h: ctc_beam_kernel<CTC_BEAM_TRIE>): scores and
    beam_width as ctc_beam_search, trie a ctc_lexicon_trie handle -> (paths, lengths, hyp_scores) shaped as ctc_beam_search returns
    them, and word_ids int32 [B, W]: the row of the lexicon every hypothesis is, -1 for an unused slot.  A prefix grows only along an
    edge of the trie and is a hypothesis only where a word ends; prefixes that end no word compete for the beam's slots during the
    search, so a narrow beam may end with no word at all.  hyp_scores is a lower bound of ctc_lexicon_score's number for that word: the
    sum over the alignments the beam kept.  The cost does not depend on the size of the lexicon."""
    B, T, C = _frame_scores("ctc_beam_search_trie", scores)
    if not isinstance(trie, CTCLexiconTrie):
        raise TypeError(f"ctc_beam_search_trie: trie must come from ctc_lexicon_trie, got {type(trie).__name__}")
    W = _beam_width("ctc_beam_search_trie", beam_width, CTC_MAX_BEAM)
    paths, lengths, hyp_scores = _beam_outputs(B, W, T, scores.device)
    word_ids = torch.empty((B, W), dtype=I32, device=scores.device)
    _call("ccd_ctc_beam_search_trie", scores, scores.stride(0), scores.stride(1), B, T, C, 1 if normalized else 0, W, trie.on(scores.device),
          trie.n_nodes, paths, lengths, hyp_scores, word_ids)
    return paths, lengths, hyp_scores, word_ids


def ctc_lexicon_search(scores, trie, beam_width, nbest=1, normalized=False):
    """The two-stage closed-vocabulary decoder, on the device with no host synchronisation: ctc_beam_search_trie proposes up to
    beam_width words per sample, ctc_lexicon_score(subset=) scores those exactly and ctc_lexicon_best picks
    -> (word_ids int32 [B, nbest], log_probs fp32 [B, nbest]), best first; an empty slot is (-1, -inf).  The log-probabilities are the
    exact ones - the numbers ctc_lexicon_score gives those words - and the proposals are sorted by word id before they are scored, so a
    tie in the exact score falls to the lower word id, as on the exhaustive path.  The answer is the exhaustive path's whenever its
    best word is among the beam's proposals."""
    W, n = int(beam_width), int(nbest)
    if not 1 <= n <= max(W, 1):
        raise ValueError(f"ctc_lexicon_search: nbest must lie in 1..beam_width = {beam_width}, got {nbest}")
    _, _, _, ids = ctc_beam_search_trie(scores, W, trie, normalized=normalized)
    if not ids.shape[0]:                                                 # no sample: nothing to score
        return ids[:, :n], torch.empty((0, n), dtype=F32, device=scores.device)
    last = torch.iinfo(I32).max
    ids = torch.where(ids < 0, last, ids).sort(dim=1).values             # ascending, the empty slots last
    ids = torch.where(ids == last, -1, ids).contiguous()                 # ... as the negative padding of a subset
    index, best = ctc_lexicon_best(ctc_lexicon_score(scores, trie.lexicon, normalized=normalized, subset=ids), n)
    picked = ids.gather(1, index.clamp(min=0).long())
    return torch.where(index >= 0, picked, -1).to(I32), best


# ------------------------------------------------------------------------------------------ forced alignment (kernels/ctc_align.h)
def ctc_align(scores, targets, normalized=False, rows=None):
    """The best single alignment of every target (kernels/ctc_align.h): scores fp32 [B, T, C] (any sample / step stride), logits or -
    normalized=True - probabilities; targets int64 [N, Lmax] zero-padded (CTCConvertor.str2tensor's layout, Lmax in 1..CTC_MAX_LABELS);
    rows int32 [N]: target n is aligned against sample rows[n] (None: N == B, target n against sample n)
    -> (frame_char int32 [N, T]: the character index emitted at every frame, -1 for a blank frame; spans int32 [N, Lmax, 2]: first and
    last frame of every character, -1 behind the word; char_logp fp32 [N, Lmax]: the summed frame log-probability of every character;
    score fp32 [N]: the log-probability of the alignment).  An infeasible row (a class outside [1, C), more characters than frames, no
    alignment of finite probability, a rows entry outside [0, B)) has score -inf and padding everywhere else."""
    B, T, C = _frame_scores("ctc_align", scores)
    if targets.dim() != 2 or not targets.is_contiguous():
        raise ValueError(f"ctc_align: expects contiguous targets [N, Lmax], got {list(targets.shape)}")
    N, Lmax = targets.shape
    if not 1 <= Lmax <= CTC_MAX_LABELS:
        raise ValueError(f"ctc_align: Lmax must lie in 1..{CTC_MAX_LABELS}, got {Lmax}")
    if rows is None:
        if N != B:
            raise ValueError(f"ctc_align: without rows there is one target per sample, got {N} targets for {B} samples")
    elif rows.dim() != 1 or rows.shape[0] != N or not rows.is_contiguous():
        raise ValueError(f"ctc_align: expects contiguous rows [{N}], got {list(rows.shape)}")
    frame_char = torch.empty((N, T), dtype=I32, device=scores.device)
    spans = torch.empty((N, Lmax, 2), dtype=I32, device=scores.device)
    char_logp = torch.empty((N, Lmax), dtype=F32, device=scores.device)
    score = torch.empty(N, dtype=F32, device=scores.device)
    _call("ccd_ctc_align", scores if B else None, scores.stride(0), scores.stride(1), B, T, C, 1 if normalized else 0, targets, N, Lmax, rows,
          frame_char, spans, char_logp, score)
    return frame_char, spans, char_logp, score


def ctc_paths_to_targets(paths):
    """The -1-padded int32 paths [..., T] that ctc_greedy, ctc_beam_search(_lm) and a lexicon gather return -> zero-padded int64 targets
    [..., min(T, CTC_MAX_LABELS)] for ctc_align (a longer word is cut: it has no alignment anyway).  Tensor operations on the device,
    no synchronisation."""
    if paths.dim() < 1 or paths.dtype != I32:
        raise ValueError(f"ctc_paths_to_targets: expects int32 paths [..., T], got {str(paths.dtype)[6:]} {list(paths.shape)}")
    return paths[..., :CTC_MAX_LABELS].clamp(min=0).to(I64).contiguous()


# ------------------------------------------------------------------------------------------ NRTR beam search (kernels/nrtr_beam.h)
NRTR_MAX_BEAM = 16                                        # ccd_hip.h: CCD_NRTR_MAX_BEAM
NRTR_UNUSED, NRTR_LIVE, NRTR_FINISHED = 0, 1, 2           # ccd_hip.h: CCD_NRTR_UNUSED ..


def nrtr_beam_state(B, beam_width, seq_len, start_idx, pad_idx, device):
    """The state in front of step 0 -> (seq int64 [B * W, seq_len] = start, padding, ...; score fp64 [B, W] = 0, -inf, ...; state int32
    [B, W] = live, unused, ...; parent int32 [B, W])."""
    W = _beam_width("nrtr_beam_state", beam_width, NRTR_MAX_BEAM)
    seq = torch.full((B * W, seq_len), pad_idx, dtype=I64, device=device)
    seq[:, 0] = start_idx
    score = torch.full((B, W), float("-inf"), dtype=F64, device=device)
    score[:, 0] = 0.0
    state = torch.zeros((B, W), dtype=I32, device=device)
    state[:, 0] = NRTR_LIVE
    return seq, score, state, torch.full((B, W), -1, dtype=I32, device=device)


def _nrtr_beam_step(who, logits, C, step, end_idx, pad_idx, seq, score, state, parent, final, node=None, trie=None, class_offset=1,
                    joint=None, weight=0.0):
    """The body of nrtr_beam_step (trie None, joint None), nrtr_beam_step_trie and nrtr_beam_step_joint: the checks under the caller's
    name `who`, the outputs of the final step, the launch."""
    if score.dim() != 2 or not 1 <= score.shape[1] <= NRTR_MAX_BEAM:
        raise ValueError(f"{who}: score must be [B, W] with W in 1..{NRTR_MAX_BEAM}, got {list(score.shape)}")
    B, W = score.shape
    slots = [("score", score, F64), ("state", state, I32), ("parent", parent, I32)] + ([("node", node, I32)] if trie is not None else [])
    for name, t, dtype in slots + [("seq", seq, I64), ("logits", logits, F32)]:
        if t.dtype != dtype:
            raise ValueError(f"{who}: {name} must be {dtype}, got {t.dtype}")
    for name, t, _ in slots:
        if tuple(t.shape) != (B, W) or not t.is_contiguous():
            raise ValueError(f"{who}: {name} must be contiguous [{B}, {W}], got {list(t.shape)}")
    if seq.dim() != 2 or seq.shape[0] != B * W or not seq.is_contiguous():
        raise ValueError(f"{who}: seq must be contiguous [{B * W}, seq_len], got {list(seq.shape)}")
    if logits.dim() != 2 or logits.shape[0] != B * W or logits.stride(1) != 1 or not 1 <= int(C) <= logits.shape[1]:
        raise ValueError(f"{who}: expects logits [{B * W}, >= {C}] with dense rows, got {list(logits.shape)}")
    seq_len = seq.shape[1]
    if not 0 <= int(step) <= seq_len - 2:
        raise ValueError(f"{who}: step must lie in 0..seq_len - 2 = {seq_len - 2}, got {step}")
    if not 0 <= int(end_idx) < int(C) or not 0 <= int(pad_idx) < 65536:
        raise ValueError(f"{who}: end_idx must lie in [0, {C}) and pad_idx in [0, 65536), got {end_idx}, {pad_idx}")
    if trie is not None and (isinstance(class_offset, bool) or class_offset not in (0, 1)):
        raise ValueError(f"{who}: class_offset must be 0 or 1, got {class_offset!r}")
    out = _beam_outputs(B, W, seq_len - 1, seq.device) if final else (None, None, None)
    args = (logits, logits.stride(0), B, W, int(C), int(step), int(end_idx), int(pad_idx), seq, seq_len, score, state, parent, *out)
    if joint is not None:
        out += (torch.empty((B, W), dtype=F32, device=seq.device) if final else None,)
        _call("ccd_nrtr_beam_step_joint", *args, joint.log_probs, joint.Tc, joint.Cc, int(class_offset), weight, joint.prefix, joint.att,
              out[3])
    elif trie is None:
        _call("ccd_nrtr_beam_step", *args)
    else:
        out += (torch.empty((B, W), dtype=I32, device=seq.device) if final else None,)
        _call("ccd_nrtr_beam_step_trie", *args, trie.on(seq.device), trie.n_nodes, int(class_offset), node, out[3])
    return out if final else None


def nrtr_beam_step(logits, C, step, end_idx, pad_idx, seq, score, state, parent, final=False):
    """One decoding position of the beam over the NRTR decoder, in place: logits fp32 [B * W, ld >= C] (row b * W + r = slot r of sample
    b), seq int64 [B * W, seq_len], score fp64 [B, W], state int32 [B, W], parent int32 [B, W] (written) - the layout of ccd_hip.h.
    Writes seq[:, step + 1].  final=True also returns (paths int32 [B, W, seq_len - 1] by rank, -1-padded; lengths int32 [B, W], -1
    for an unused slot; hyp_scores fp32 [B, W], -inf for an unused slot) of the new state, as ctc_beam_search returns them."""
    return _nrtr_beam_step("nrtr_beam_step", logits, C, step, end_idx, pad_idx, seq, score, state, parent, final)


def nrtr_beam_trie_state(B, beam_width, device):
    """The trie node of every slot in front of step 0 -> node int32 [B, W], all zeros: the root of the lexicon's prefix tree."""
    return torch.zeros((B, _beam_width("nrtr_beam_trie_state", beam_width, NRTR_MAX_BEAM)), dtype=I32, device=device)


def nrtr_beam_step_trie(logits, C, step, end_idx, pad_idx, seq, score, state, parent, node, trie, class_offset=1, final=False):
    """nrtr_beam_step along the prefix tree of a lexicon (kernels/nrtr_beam.h: nrtr_beam_step_kernel<true>), in place: node int32 [B, W]
    (nrtr_beam_trie_state) is the trie node of every slot, trie a ctc_lexicon_trie handle whose mask bit for class c is c + class_offset
    (1: the lexicon's rows are class + 1, AttnConvertor.set_lexicon's layout; 0: the classes themselves).  A live slot extends only
    along an edge of its node and ends only where a word ends; the scores are nrtr_beam_step's, so a finished slot holds the exact
    log-probability of its word with the <EOS>.  final=True returns (paths, lengths, hyp_scores) as nrtr_beam_step does and word_ids
    int32 [B, W]: the lexicon row of every finished slot, -1 for a slot that is unused or still live."""
    if not isinstance(trie, CTCLexiconTrie):                         # (None included: it would select the plain step)
        raise TypeError(f"nrtr_beam_step_trie: trie must come from ctc_lexicon_trie, got {type(trie).__name__}")
    return _nrtr_beam_step("nrtr_beam_step_trie", logits, C, step, end_idx, pad_idx, seq, score, state, parent, final, node, trie, class_offset)


NRTR_JOINT_MAX_STEPS = 64                                 # ccd_hip.h: CCD_NRTR_JOINT_MAX_STEPS


class NRTRJointState:
    """The CTC side of a joint CTC / attention beam (nrtr_joint_state): log_probs fp64 [B, Tc, Cc], the workspace every step reads;
    prefix fp64 [B, W, 2, Tc], the prefix state of every slot; att fp64 [B, W], its attention score."""

    def __init__(self, log_probs, prefix, att):
        self.log_probs, self.prefix, self.att = log_probs, prefix, att
        self.B, self.W, _, self.Tc = prefix.shape
        self.Cc = log_probs.shape[2]


def nrtr_joint_state(frames, beam_width, normalized=False):
    """The CTC side of joint CTC / attention decoding in front of step 0 (kernels/nrtr_joint.h: ccd_nrtr_joint_begin): frames fp32
    [B, Tc, Cc] of an auxiliary CTC head (any sample / step stride; blank = class 0), logits or - normalized=True - probabilities ->
    an NRTRJointState handle: the fp64 frame log-probabilities, the root prefix state in every one of the W slots, and att = 0,
    -inf, .. as nrtr_beam_state's score.  Tc in 1..64, Cc in 1..128."""
    B, Tc, Cc = _frame_scores("nrtr_joint_state", frames, "frames")
    W = _beam_width("nrtr_joint_state", beam_width, NRTR_MAX_BEAM)
    if frames.dtype != F32:
        raise ValueError(f"nrtr_joint_state: frames must be {F32}, got {frames.dtype}")
    if not 1 <= Tc <= NRTR_JOINT_MAX_STEPS or not 1 <= Cc <= NRTR_MAX_CLASSES:
        raise ValueError(f"nrtr_joint_state: expects frames [B, 1..{NRTR_JOINT_MAX_STEPS}, 1..{NRTR_MAX_CLASSES}], got {list(frames.shape)}")
    dev = frames.device
    log_probs = torch.empty((B, Tc, Cc), dtype=F64, device=dev)
    prefix = torch.empty((B, W, 2, Tc), dtype=F64, device=dev)
    att = torch.full((B, W), float("-inf"), dtype=F64, device=dev)
    att[:, 0] = 0.0
    _call("ccd_nrtr_joint_begin", frames, frames.stride(0), frames.stride(1), B, Tc, Cc, 1 if normalized else 0, W, log_probs, prefix)
    return NRTRJointState(log_probs, prefix, att)


def nrtr_beam_step_joint(logits, C, step, end_idx, pad_idx, seq, score, state, parent, joint, weight, class_offset=1, final=False):
    """nrtr_beam_step with every candidate rescored by the CTC prefix probability of an auxiliary CTC head (kernels/nrtr_joint.h), in
    place: joint is nrtr_joint_state's handle (its prefix states and attention scores are updated like score and state), weight w in
    [0, 1], decoder class c is CTC class c + class_offset (1: the CTC head's classes are the decoder's + 1 behind the blank).  score
    holds S = (1 - w) attention + w CTC; at weight 0 the step is nrtr_beam_step's, bit for bit.  final=True returns (paths, lengths,
    hyp_scores, att_scores): nrtr_beam_step's three with the joint scores, and att_scores fp32 [B, W], the attention scores alone."""
    who = "nrtr_beam_step_joint"
    if not isinstance(joint, NRTRJointState):
        raise TypeError(f"{who}: joint must come from nrtr_joint_state, got {type(joint).__name__}")
    if isinstance(weight, bool) or not isinstance(weight, (int, float)) or not 0.0 <= float(weight) <= 1.0:      # (a NaN fails both)
        raise ValueError(f"{who}: weight must lie in [0, 1], got {weight!r}")
    if isinstance(class_offset, bool) or class_offset not in (0, 1):
        raise ValueError(f"{who}: class_offset must be 0 or 1, got {class_offset!r}")
    if tuple(score.shape) != (joint.B, joint.W) or joint.att.device != score.device:
        raise ValueError(f"{who}: joint was made for [{joint.B}, {joint.W}] slots on {joint.att.device}, score is {list(score.shape)} on "
                         f"{score.device}")
    return _nrtr_beam_step(who, logits, C, step, end_idx, pad_idx, seq, score, state, parent, final, joint=joint, weight=float(weight),
                           class_offset=class_offset)


def nrtr_beam_reorder(cache, parent, positions, step):
    """The decode loop's cache bf16 [L, B * W * positions, 3 D] (q | k | v of position t of slot r of sample b in row (b * W + r) *
    positions + t), in place: for every position <= step, the K and V columns of slot r become those of slot parent[r] (int32 [B, W];
    -1 or r: nothing moves).  The Q columns of those positions are unspecified afterwards; the positions behind `step` stay."""
    if parent.dim() != 2 or parent.dtype != I32 or not parent.is_contiguous() or not 1 <= parent.shape[1] <= NRTR_MAX_BEAM:
        raise ValueError(f"nrtr_beam_reorder: parent must be contiguous int32 [B, W] with W in 1..{NRTR_MAX_BEAM}, got "
                         f"{parent.dtype} {list(parent.shape)}")
    B, W = parent.shape
    if cache.dtype != BF16 or cache.dim() != 3 or not cache.is_contiguous() or cache.shape[1] != B * W * int(positions) or \
            cache.shape[2] % 24:
        raise ValueError(f"nrtr_beam_reorder: cache must be contiguous bfloat16 [L, {B * W} * {positions}, 3 D] with D a multiple of 8, got "
                         f"{cache.dtype} {list(cache.shape)}")
    if not 0 <= int(step) < int(positions):
        raise ValueError(f"nrtr_beam_reorder: step must lie in 0..positions - 1 = {int(positions) - 1}, got {step}")
    _call("ccd_nrtr_beam_reorder", cache, parent, cache.shape[0], B, W, int(positions), cache.shape[2] // 3, int(step))


# ------------------------------------------------------------------------------------------ scoring given words (kernels/nrtr_score.h)
XATTN_ROWS_MAX_TQ = 32                                    # queries of a word row (decoder_xattn.h: XA_TQ)
NRTR_MAX_CLASSES, NRTR_MAX_POSITIONS = 128, 128           # nrtr_beam.h: NRTR_MAX_C, NRTR_MAX_LEN


class CsrRows(_OncePerDevice):
    """Which sample owns which word row, in CSR form: the rows of sample b are ptr[b] .. ptr[b + 1] - 1.  Built and checked on the host
    (csr_rows below) - the counts are host knowledge, the word lists - and uploaded once per device."""

    def __init__(self, ptr):
        self.ptr = ptr                                    # numpy int32 [B + 1]
        self.B, self.R = len(ptr) - 1, int(ptr[-1])
        self.max_rows = int(np.diff(ptr).max()) if len(ptr) > 1 else 0

    def _upload(self, device):
        return upload(torch.from_numpy(self.ptr), device)


def csr_rows(ptr):
    """ptr: B + 1 host integers (a list, a numpy array, a CPU tensor), non-decreasing from 0 -> a CsrRows handle.  A sample may own no
    rows.  A device tensor is refused: checking it would wait for the device."""
    if isinstance(ptr, CsrRows):
        return ptr
    if isinstance(ptr, torch.Tensor):
        if ptr.device.type != "cpu":
            raise TypeError("csr_rows: expects host integers (the table is checked on the host), got a tensor on " + str(ptr.device))
        if ptr.dtype not in (I32, I64):
            raise TypeError(f"csr_rows: expects an integer table, got {ptr.dtype}")
        ptr = ptr.numpy()
    a = np.asarray(ptr)
    if a.ndim != 1 or a.size < 1 or a.dtype.kind not in "iu":
        raise TypeError(f"csr_rows: expects B + 1 integers, got {a.dtype} {list(a.shape)}")
    a = a.astype(np.int64)
    if a[0] != 0 or (np.diff(a) < 0).any() or a[-1] > 0x7fffffff:
        raise ValueError("csr_rows: row_ptr must start at 0 and never decrease (CSR: sample b owns the rows ptr[b] .. ptr[b + 1] - 1), got "
                         f"{a[:8].tolist()}{' ..' if a.size > 8 else ''}")
    return CsrRows(np.ascontiguousarray(a.astype(np.int32)))


def xattn_rows_chunk(R, H):
    """The rows of one sample that a workgroup of xattn_rows_fwd takes (ccd_hip.h: ccd_xattn_rows_chunk): max(1, ceil(R * H / (4 *
    compute units))).  It sizes the grid; results do not depend on it."""
    ch = _lib.get().ccd_xattn_rows_chunk(int(R), int(H))
    if ch < 1:
        _lib.check(ch, "ccd_xattn_rows_chunk")
    return ch


def xattn_rows_fwd(q, k, v, row_ptr, H, Tq, scale, want_moments=False):
    """The encoder-decoder attention of R word rows against the keys / values of the sample that owns each row (kernels/nrtr_score.h):
    q bf16 [R * Tq, >= 64 H], k, v bf16 [B * 256, >= 64 H] 2-D views (head h at column 64 h; any row stride that is a multiple of 8),
    row_ptr a CsrRows handle or B + 1 host integers (ops.csr_rows) -> (out bf16 [R * Tq, 64 H], moments fp32 [R, H, Tq, 4] or None).  `out` is
    bit-equal to dec_attn_fwd on k / v gathered per row; moments = sum p x, sum p y, sum p x^2, sum p y^2 of every attention map over
    the 8 x 32 token grid (x = key & 31, y = key >> 5).  Inference only."""
    rp = csr_rows(row_ptr)
    H, Tq = int(H), int(Tq)
    if not 1 <= Tq <= XATTN_ROWS_MAX_TQ:
        raise ValueError(f"xattn_rows_fwd: Tq must lie in 1..{XATTN_ROWS_MAX_TQ}, got {Tq}")
    if H < 1:
        raise ValueError(f"xattn_rows_fwd: H must be positive, got {H}")
    for name, t in (("q", q), ("k", k), ("v", v)):
        if t.dtype != BF16:
            raise TypeError(f"xattn_rows_fwd: {name} must be bfloat16, got {t.dtype}")
        if t.dim() != 2 or t.shape[1] < 64 * H or (t.shape[0] > 0 and t.stride(1) != 1) or (t.shape[0] > 1 and t.stride(0) % 8):
            raise ValueError(f"xattn_rows_fwd: {name} must be a 2-D view of >= {64 * H} dense columns whose row stride is a multiple of 8, "
                             f"got {list(t.shape)}, strides {t.stride()}")
    if q.shape[0] != rp.R * Tq:
        raise ValueError(f"xattn_rows_fwd: row_ptr ends at {rp.R} rows of {Tq} queries, q has {q.shape[0]} rows")
    if k.shape[0] != rp.B * 256 or v.shape[0] != rp.B * 256:
        raise ValueError(f"xattn_rows_fwd: row_ptr names {rp.B} samples of 256 keys, k / v have {k.shape[0]} / {v.shape[0]} rows")
    out = torch.empty((rp.R * Tq, 64 * H), dtype=BF16, device=q.device)
    moments = torch.empty((rp.R, H, Tq, 4), dtype=F32, device=q.device) if want_moments else None
    if rp.R and rp.B:
        ld = [t.stride(0) if t.shape[0] > 1 else t.shape[1] for t in (q, k, v)]
        _call("ccd_xattn_rows_fwd", q, ld[0], k, ld[1], v, ld[2], rp.on(q.device), out, 64 * H, moments, rp.R, rp.B, H, Tq, rp.max_rows,
              float(scale))
    return out, moments


def nrtr_word_score(logits, C, seq, end_idx, pad_idx, moments=None, H=None):
    """log-probabilities and positions of every character of R given words (kernels/nrtr_score.h; tests/nrtr_score_np.py is the
    specification): logits fp32 [R * T, ld >= C] of the teacher-forced decoder, seq int64 [R, T] = <BOS> c1 .. cn <EOS> <PAD> .. ->
    (char_logp fp32 [R, T - 1], score fp32 [R], length int32 [R], char_pos fp32 [R, T - 1, 4] or None).  char_logp[r, t] is the fp64
    log-softmax over the classes [0, C) at position t taken at seq[r, t + 1], for t = 0 .. n (entry n: the <EOS>), 0 behind it; score
    their fp64 sum = log p(word <EOS> | image); length = n.  A row without an <EOS> behind position 0, or with a character outside [0, C)
    or equal to pad_idx, is infeasible: score -inf, length -1, zeros.  moments fp32 [R, H, T, 4] (xattn_rows_fwd, the last layer's) gives
    char_pos = mean_x, mean_y, std_x, std_y of the head-averaged attention of every character, in token units."""
    if seq.dtype != I64:
        raise TypeError(f"nrtr_word_score: seq must be int64, got {seq.dtype}")
    if seq.dim() != 2 or not seq.is_contiguous():
        raise ValueError(f"nrtr_word_score: seq must be contiguous [R, T], got {list(seq.shape)}, strides {seq.stride()}")
    if logits.dtype != F32:
        raise TypeError(f"nrtr_word_score: logits must be float32, got {logits.dtype}")
    R, T = seq.shape
    C = int(C)
    if not 2 <= T <= NRTR_MAX_POSITIONS or not 1 <= C <= NRTR_MAX_CLASSES:
        raise ValueError(f"nrtr_word_score: expects 2..{NRTR_MAX_POSITIONS} positions and 1..{NRTR_MAX_CLASSES} classes, got T = {T}, C = {C}")
    if logits.dim() != 2 or logits.shape[0] != R * T or logits.shape[1] < C or (R and logits.stride(1) != 1):
        raise ValueError(f"nrtr_word_score: expects logits [{R * T}, >= {C}] with dense rows, got {list(logits.shape)}")
    if not 0 <= int(end_idx) < C:
        raise ValueError(f"nrtr_word_score: end_idx must lie in [0, {C}), got {end_idx}")
    dev = logits.device
    char_pos = None
    if moments is not None:
        if H is None or int(H) < 1:
            raise ValueError(f"nrtr_word_score: moments need the number of heads H >= 1, got {H!r}")
        if moments.dtype != F32:
            raise TypeError(f"nrtr_word_score: moments must be float32, got {moments.dtype}")
        if tuple(moments.shape) != (R, int(H), T, 4) or not moments.is_contiguous():
            raise ValueError(f"nrtr_word_score: moments must be contiguous [{R}, {int(H)}, {T}, 4], got {list(moments.shape)}")
        char_pos = torch.empty((R, T - 1, 4), dtype=F32, device=dev)
    char_logp = torch.empty((R, T - 1), dtype=F32, device=dev)
    score = torch.empty(R, dtype=F32, device=dev)
    length = torch.empty(R, dtype=I32, device=dev)
    if R:
        ld = logits.stride(0) if logits.shape[0] > 1 else logits.shape[1]
        _call("ccd_nrtr_word_score", logits, ld, C, seq, R, T, int(end_idx), int(pad_idx), moments, int(H) if moments is not None else 0,
              char_logp, score, length, char_pos)
    return char_logp, score, length, char_pos


# ------------------------------------------------------------------------------------------ two-pass decoding (kernels/nrtr_twopass.h)
NRTR_TWOPASS_MAX_PATH = 128                               # nrtr_twopass.h: NTP_MAX_PATH


def _twopass_proposals(who, paths, lengths):
    """The check both two-pass kernels start with: paths int32 [B, W, Tp] with dense entries (any sample / slot stride), lengths
    contiguous int32 [B, W] on the same device, W in 1..NRTR_MAX_BEAM, Tp in 1..NRTR_TWOPASS_MAX_PATH -> (B, W, Tp, sample stride, slot
    stride)."""
    for name, t in (("paths", paths), ("lengths", lengths)):
        if not isinstance(t, torch.Tensor) or t.dtype != I32:
            raise TypeError(f"{who}: {name} must be an int32 tensor, got {t.dtype if isinstance(t, torch.Tensor) else type(t).__name__}")
    if paths.dim() != 3 or (paths.shape[2] > 1 and paths.stride(2) != 1):
        raise ValueError(f"{who}: expects paths [B, W, Tp] with dense entries, got {list(paths.shape)}, strides {paths.stride()}")
    B, W, Tp = paths.shape
    if not 1 <= W <= NRTR_MAX_BEAM or not 1 <= Tp <= NRTR_TWOPASS_MAX_PATH:
        raise ValueError(f"{who}: expects paths [B, 1..{NRTR_MAX_BEAM}, 1..{NRTR_TWOPASS_MAX_PATH}], got {list(paths.shape)}")
    if tuple(lengths.shape) != (B, W) or not lengths.is_contiguous() or lengths.device != paths.device:
        raise ValueError(f"{who}: expects contiguous lengths [{B}, {W}] on {paths.device}, got {list(lengths.shape)} on {lengths.device}")
    return B, W, Tp, paths.stride(0) if B > 1 else W * Tp, paths.stride(1) if W > 1 else Tp


def _class_offset(who, class_offset):
    if isinstance(class_offset, bool) or class_offset not in (0, 1):
        raise ValueError(f"{who}: class_offset must be 0 or 1, got {class_offset!r}")
    return int(class_offset)


def nrtr_twopass_rows(paths, lengths, classes, start_idx, end_idx, pad_idx, seq_len, max_labels=None, class_offset=1, want_seq=True):
    """The words a CTC decoder proposes -> the rows of the NRTR decoder's teacher-forced pass and the CTC scorer's word table, in one
    launch (kernels/nrtr_twopass.h: ccd_nrtr_twopass_rows; tests/nrtr_twopass_np.py is the specification): paths int32 [B, W, Tp],
    -1-padded CTC classes, lengths int32 [B, W] (-1: an unused slot), as ctc_beam_search(_lm / _trie) returns them -> (seq int64 [B * W,
    seq_len] = <BOS> d1 .. dn <EOS> <PAD>.. with d = c - class_offset, AttnConvertor.words2rows' layout; targets int64 [B * W,
    max_labels] = c1 .. cn 0.., ctc_paths_to_targets' layout; subset int32 [B, W] = b * W + k, or -1).  A slot is INELIGIBLE - <BOS>
    <PAD>.., zeros, -1 - when it is unused, longer than min(Tp, seq_len - 2, max_labels), or holds a class with c < 1, d outside [0,
    classes), d == end_idx or d == pad_idx: seq holds no token but start_idx, end_idx, pad_idx and classes in [0, classes).  max_labels
    defaults to min(Tp, CTC_MAX_LABELS).  want_seq=False: the CTC side alone (seq is None; end_idx / pad_idx may be -1: no such class)."""
    who = "nrtr_twopass_rows"
    B, W, Tp, s0, s1 = _twopass_proposals(who, paths, lengths)
    off = _class_offset(who, class_offset)
    classes, seq_len = int(classes), int(seq_len)
    Lmax = min(Tp, CTC_MAX_LABELS) if max_labels is None else int(max_labels)
    if not 1 <= classes <= NRTR_MAX_CLASSES or not 2 <= seq_len <= NRTR_MAX_POSITIONS or not 1 <= Lmax <= CTC_MAX_LABELS:
        raise ValueError(f"{who}: expects classes in 1..{NRTR_MAX_CLASSES}, seq_len in 2..{NRTR_MAX_POSITIONS} and max_labels in "
                         f"1..{CTC_MAX_LABELS}, got {classes}, {seq_len}, {Lmax}")
    lowest = 0 if want_seq else -1
    for name, v in (("start_idx", start_idx), ("end_idx", end_idx), ("pad_idx", pad_idx)):
        if not lowest <= int(v) < 65536:
            raise ValueError(f"{who}: {name} must lie in [{lowest}, 65536), got {v}")
    dev = paths.device
    seq = torch.empty((B * W, seq_len), dtype=I64, device=dev) if want_seq else None
    targets = torch.empty((B * W, Lmax), dtype=I64, device=dev)
    subset = torch.empty((B, W), dtype=I32, device=dev)
    _call("ccd_nrtr_twopass_rows", paths if B else None, s0, s1, lengths if B else None, B, W, Tp, off, classes, int(start_idx),
          int(end_idx), int(pad_idx), seq if B else None, seq_len, targets if B else None, Lmax, subset if B else None)
    return seq, targets, subset


def nrtr_twopass_select(att, ctc, paths, lengths, subset, weight, max_seq_len, class_offset=1):
    """Combine, rank, gather (kernels/nrtr_twopass.h: ccd_nrtr_twopass_select): att fp32 [B * W] (nrtr_word_score's score of
    nrtr_twopass_rows' seq), ctc fp32 [B, W] (ctc_score_paths), the proposals and nrtr_twopass_rows' subset -> (paths int32 [B, W,
    max_seq_len] in decoder classes, -1-padded; lengths int32 [B, W]; scores, att_scores, ctc_scores fp32 [B, W]; source int32 [B, W]),
    best first.  A slot is eligible iff subset >= 0, its length lies in 0..min(Tp, max_seq_len) and both scores are finite; S = (1 -
    weight) att + weight ctc in fp64, a term whose weight is exactly 0 left out; ranks go by (S descending, slot ascending); a rank
    left over holds (-1.., -1, -inf, -inf, -inf, -1)."""
    who = "nrtr_twopass_select"
    B, W, Tp, s0, s1 = _twopass_proposals(who, paths, lengths)
    off = _class_offset(who, class_offset)
    if isinstance(weight, bool) or not isinstance(weight, (int, float)) or not 0.0 <= float(weight) <= 1.0:      # (a NaN fails both)
        raise ValueError(f"{who}: weight must lie in [0, 1], got {weight!r}")
    T = int(max_seq_len)
    if not 1 <= T <= NRTR_MAX_POSITIONS:
        raise ValueError(f"{who}: max_seq_len must lie in 1..{NRTR_MAX_POSITIONS}, got {max_seq_len}")
    dev = paths.device
    for name, t, dtype, shape in (("att", att, F32, (B * W,)), ("ctc", ctc, F32, (B, W)), ("subset", subset, I32, (B, W))):
        if not isinstance(t, torch.Tensor) or t.dtype != dtype:
            raise TypeError(f"{who}: {name} must be a {dtype} tensor, got {t.dtype if isinstance(t, torch.Tensor) else type(t).__name__}")
        if tuple(t.shape) != shape or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"{who}: expects contiguous {name} {list(shape)} on {dev}, got {list(t.shape)} on {t.device}")
    out_paths, out_lengths, scores = _beam_outputs(B, W, T, dev)
    att_scores, ctc_scores = torch.empty((B, W), dtype=F32, device=dev), torch.empty((B, W), dtype=F32, device=dev)
    source = torch.empty((B, W), dtype=I32, device=dev)
    if B:
        _call("ccd_nrtr_twopass_select", paths, s0, s1, lengths, B, W, Tp, off, att, ctc, subset, float(weight), T, out_paths, out_lengths,
              scores, att_scores, ctc_scores, source)
    return out_paths, out_lengths, scores, att_scores, ctc_scores, source


def ctc_score_paths(scores, paths, lengths, normalized=False, rows=None):
    """The exact log p(word | frames) of ANY decoder's hypotheses: scores fp32 [B, T, C] (any sample / step stride), logits or -
    normalized=True - probabilities; paths int32 [B, W, Tp] -1-padded CTC classes and lengths int32 [B, W], as ctc_beam_search(_lm /
    _trie) returns them -> fp32 [B, W], the CTC forward log-likelihood summed over ALL alignments (a beam's own score sums only the
    alignments the beam kept).  No new scoring kernel and no host copy: nrtr_twopass_rows writes the device word table and `subset`
    that ctc_lexicon_score's kernel takes (V = B * W words, sample b scoring its own W).  -inf for an unused slot, a class outside [1,
    C), a word no alignment spells, and a path longer than CTC_MAX_LABELS = 31 characters - the lexicon scorer's own limit on a word.
    rows: (targets, subset) of an nrtr_twopass_rows call on the same proposals, to save the launch (slots ineligible there are -inf)."""
    B, T, C = _frame_scores("ctc_score_paths", scores)
    Bp, W, Tp, _, _ = _twopass_proposals("ctc_score_paths", paths, lengths)
    if Bp != B or paths.device != scores.device:
        raise ValueError(f"ctc_score_paths: scores are {list(scores.shape)} on {scores.device}, paths {list(paths.shape)} on {paths.device}")
    if rows is None:
        _, targets, subset = nrtr_twopass_rows(paths, lengths, NRTR_MAX_CLASSES, -1, -1, -1, NRTR_MAX_POSITIONS, want_seq=False)
    else:
        targets, subset = rows
        if targets.dtype != I64 or targets.dim() != 2 or targets.shape[0] != B * W or not 1 <= targets.shape[1] <= CTC_MAX_LABELS or \
                not targets.is_contiguous() or subset.dtype != I32 or tuple(subset.shape) != (B, W) or not subset.is_contiguous():
            raise ValueError(f"ctc_score_paths: rows must be nrtr_twopass_rows' (targets int64 [{B * W}, 1..{CTC_MAX_LABELS}], subset int32 "
                             f"[{B}, {W}]), got {list(targets.shape)} and {list(subset.shape)}")
    out = torch.full((B, W), float("-inf"), dtype=F32, device=scores.device)
    if B:
        _call("ccd_ctc_lexicon_score", scores, scores.stride(0), scores.stride(1), B, T, C, 1 if normalized else 0, targets, B * W,
              targets.shape[1], None, subset, W, out, W)
    return out


class SsimFn(torch.autograd.Function):
    """apply(window, taps, size_average, img1, img2[, img3]) -> mean (0-dim) or per-image means [N]; backward on the kernels."""

    @staticmethod
    def forward(ctx, window, taps, size_average, *imgs):
        per, mean = ssim_fwd(imgs, window, taps, size_average)
        ctx.save_for_backward(*imgs)
        ctx.window, ctx.taps, ctx.size_average = window, taps, size_average
        return mean if size_average else per

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        imgs = ctx.saved_tensors
        N, C, H, W = imgs[0].shape
        if ctx.size_average:
            gscale = (grad.float() / float(N * C * H * W)).expand(N).contiguous()
        else:
            gscale = (grad.float() / float(C * H * W)).contiguous()
        dx = ssim_bwd(imgs, ctx.window, ctx.taps, gscale, ctx.needs_input_grad[3:])
        return (None, None, None, *dx)


class PsnrFn(torch.autograd.Function):
    """apply(a, b) -> (psnr 0-dim fp32, mse 0-dim fp64, not differentiable).  d psnr / d a = -(20 / ln 10) 255^2 (a - b) / (mse count)
    on the first min(C, 3) channels, zero on the others; d / d b = its negative (elementwise, not a hot path)."""

    @staticmethod
    def forward(ctx, a, b):
        psnr, mse = psnr_fwd(a, b)
        ctx.mark_non_differentiable(mse)
        ctx.save_for_backward(a, b, mse)
        return psnr, mse

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad, _grad_mse):
        a, b, mse = ctx.saved_tensors
        N, C, H, W = a.shape
        ch = min(C, 3)
        k = grad.double() * (-(20.0 / math.log(10.0)) * 255.0 ** 2) / (mse * float(N * ch * H * W))
        d = torch.zeros(a.shape, dtype=F32, device=a.device)
        d[:, :ch] = (k * (a[:, :ch].double() - b[:, :ch].double())).float()
        da = d if ctx.needs_input_grad[0] else None
        db = -d if ctx.needs_input_grad[1] else None
        return da, db


# ------------------------------------------------------------------------------------------ DINO head pieces
def l2norm_fwd(x, y, inv, d_rows=None, rows_mul=1):
    _call("ccd_l2norm_fwd", x, y, inv, x.shape[0], d_rows, rows_mul, x.shape[1])


def l2norm_bwd(x, inv, dy, dx, d_rows=None, rows_mul=1):
    _call("ccd_l2norm_bwd", x, inv, dy, dx, x.shape[0], d_rows, rows_mul, x.shape[1])


def weightnorm_fwd(v, g, w, w_t, inv):
    K, D = v.shape
    _call("ccd_weightnorm_fwd", v, g, w, w_t, inv, K, D)


def weightnorm_bwd(v, g, inv, dw, dv, dg):
    K, D = v.shape
    _call("ccd_weightnorm_bwd", v, g, inv, dw, dv, dg, K, D)


# ------------------------------------------------------------------------------------------ losses
def dino_loss_fwd(s_logits, t_logits, center, d_m, student_temp, teacher_temp, stats, loss_out):
    max_rows, K = s_logits.shape
    # (the kernels read the device-side row count M <= max_rows / 2; bytes are the worst case the launch is sized for)
    with _Span("dino_loss_fwd", 12.0 * max_rows * K, 8.0 * max_rows * K):
        _call("ccd_dino_loss_fwd", s_logits, t_logits, center, K, d_m, max_rows, float(student_temp), float(teacher_temp), stats, loss_out)


def dino_loss_bwd(s_logits, t_logits, center, d_m, student_temp, teacher_temp, stats, grad_scale, d_logits,
                  d_grad_scale=None):
    max_rows, K = s_logits.shape
    with _Span("dino_loss_bwd", 12.0 * max_rows * K, 10.0 * max_rows * K):
        _call("ccd_dino_loss_bwd", s_logits, t_logits, center, K, d_m, max_rows, float(student_temp), float(teacher_temp), stats,
              float(grad_scale), d_grad_scale, d_logits)


def head_loss_supported(K, D, max_rows):
    """True where ccd_head_loss_fwd / _bwd take the shape (D == 256, K % 512 == 0): the logits need not be materialised."""
    return D == 256 and K % 512 == 0 and max_rows > 0 and _lib.get().ccd_head_loss_ws_floats(int(max_rows), int(K)) > 0


_HEAD_LOSS_WS = {}


def _head_loss_ws(device, n):
    """One workspace per (device, stream) for the per-split partials of ccd_head_loss_fwd (grown, never shrunk)."""
    key = (device.index if device.type == "cuda" else -1, torch.cuda.current_stream(device).cuda_stream if device.type == "cuda" else 0)
    ws = _HEAD_LOSS_WS.get(key)
    if ws is None or ws.numel() < n:
        ws = _HEAD_LOSS_WS[key] = torch.empty(int(n), dtype=F32, device=device)
    return ws


def head_loss_fwd(zs, zt, ws, wt, center, d_m, student_temp, teacher_temp, stats, loss_out):
    """loss_out += DINO distillation loss of logits zs @ ws^T (student) against zt @ wt^T (teacher, centred) - the logits stay in
    registers (include/ccd_hip.h: ccd_head_loss_fwd).  stats [max_rows, 4] is what head_loss_bwd reads."""
    max_rows, D = zs.shape
    K = ws.shape[0]
    assert zt.shape == zs.shape and wt.shape == ws.shape and ws.shape[1] == D and stats.shape == (max_rows, 4)
    part = _head_loss_ws(zs.device, _lib.get().ccd_head_loss_ws_floats(max_rows, K))
    with _Span("head_loss_fwd", 0.0, 4.0 * K * D):          # (the live row count 2M is device-side: no flop figure)
        _call("ccd_head_loss_fwd", zs, zs.stride(0), zt, zt.stride(0), ws, ws.stride(0), wt, wt.stride(0), center, K, D, d_m, max_rows,
              float(student_temp), float(teacher_temp), part, stats, loss_out)


def head_loss_bwd(zs, zt, ws, wt, center, d_m, student_temp, teacher_temp, stats, grad_scale, d_logits, d_grad_scale=None):
    """d_logits (bf16 [max_rows, K], rows < 2M written) = d loss / d (zs @ ws^T), the products recomputed (ccd_head_loss_bwd)."""
    max_rows, D = zs.shape
    K = ws.shape[0]
    assert d_logits.shape == (max_rows, K)
    with _Span("head_loss_bwd", 0.0, 4.0 * K * D):
        _call("ccd_head_loss_bwd", zs, zs.stride(0), zt, zt.stride(0), ws, ws.stride(0), wt, wt.stride(0), center, K, D, d_m, max_rows,
              float(student_temp), float(teacher_temp), stats, float(grad_scale), d_grad_scale, d_logits, d_logits.stride(0))


def colsum_f32(x, out, d_rows=None, rows_mul=1):
    max_rows, K = x.shape
    _call("ccd_colsum_f32", x, K, d_rows, rows_mul, max_rows, out)


def matvec_bf16(w, v, out):
    """out[k] += w[k, :] . v   (w [K, D] bf16, v / out fp32; D % 256 == 0)."""
    K, D = w.shape
    assert v.numel() == D and out.numel() == K
    _call("ccd_matvec_bf16", w, w.stride(0), v, K, D, out)
    return out


def center_ema(center, batch_sum, d_m, world, momentum):
    _call("ccd_center_ema", center, batch_sum, center.numel(), d_m, int(world), float(momentum))


SINKHORN_STRIP = 1024        # columns per workgroup of the Sinkhorn column pass (sinkhorn.h: SK_STRIP)
SINKHORN_ROW_CHUNK = 128     # rows per workgroup of that pass (SK_ROW_CHUNK); the chunks' partial sums are folded in ascending order


def _sinkhorn_log_beta(logits, d_total, temp, n_iterations, rows_mul, c):
    """The Sinkhorn-Knopp iteration of Dino_loss.py:157-184 in the log domain (include/ccd_hip.h: ccd_sinkhorn_*): n_iterations
    column passes and n_iterations - 1 row passes over `logits`.  -> log beta [K], gauged to mean 0; `c` [K] (or None) receives
    -temp * log beta.
    In a process group the column state is all-reduced (MAX of the shifts, SUM of the re-based sums), as the reference all-reduces
    its prototype sums; ranks may hold different numbers of rows.  Nothing here reads a value back from the device."""
    import torch.distributed as dist
    if int(n_iterations) < 1:
        raise ValueError("sinkhorn: n_iterations must be at least 1")
    if logits.dim() != 2 or logits.dtype != F32 or not logits.is_contiguous():
        raise ValueError("sinkhorn: logits must be a dense [rows, K] fp32 matrix")
    max_rows, K = logits.shape
    dev, temp = logits.device, float(temp)
    ws = torch.empty(int(_lib.get().ccd_sinkhorn_ws_floats(max_rows, K)), dtype=F32, device=dev)
    col_m, col_s = torch.empty(K, dtype=F32, device=dev), torch.empty(K, dtype=F32, device=dev)
    log_beta, log_alpha = torch.empty(K, dtype=F32, device=dev), torch.empty(max_rows, dtype=F32, device=dev)
    shared = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
    passes = 2 * int(n_iterations) - 1
    with _Span("sinkhorn_potentials", 0.0, 4.0 * passes * max_rows * K):
        for it in range(int(n_iterations)):
            _call("ccd_sinkhorn_colpass", logits, K, d_total, int(rows_mul), max_rows, temp, log_alpha if it else None, ws, col_m, col_s)
            if shared:
                shift = col_m.clone()
                dist.all_reduce(shift, op=dist.ReduceOp.MAX)
                _call("ccd_sinkhorn_rescale", col_m, col_s, shift, K)
                dist.all_reduce(col_s)
            last = it == int(n_iterations) - 1
            _call("ccd_sinkhorn_finish", col_m, col_s, K, temp, log_beta, c if last else None)
            if not last:
                _call("ccd_sinkhorn_rowpass", logits, K, d_total, int(rows_mul), max_rows, temp, log_beta, log_alpha)
    return log_beta


def sinkhorn_potentials(logits, d_total, temp, n_iterations=3, rows_mul=2, out=None):
    """c [K] fp32 with softmax((logits - c) / temp) == DINOLoss.sinkhorn_knopp_teacher(logits, temp, n_iterations) of the reference on
    the first rows_mul * d_total[0] rows (d_total: int32 device scalar), mean(c) == 0: what the loss kernels take in place of the
    centre.  `logits`: [max_rows, K] fp32, or an engine.LazyLogits (materialised once by its tensor())."""
    from .engine import logits_tensor
    logits = logits_tensor(logits)
    if out is None:
        out = torch.empty(logits.shape[1], dtype=F32, device=logits.device)
    if out.dtype != F32 or out.numel() != logits.shape[1] or not out.is_contiguous():
        raise ValueError("sinkhorn_potentials: out must be a dense fp32 tensor of K elements")
    _sinkhorn_log_beta(logits, d_total, temp, n_iterations, rows_mul, out.view(-1))
    return out


def sinkhorn_assign(logits, d_total, temp, n_iterations=3, rows_mul=2):
    """The assignment itself, [max_rows, K] fp32 (rows past rows_mul * d_total[0] are zero): sinkhorn_potentials + one row softmax."""
    from .engine import logits_tensor
    logits = logits_tensor(logits)
    log_beta = _sinkhorn_log_beta(logits, d_total, temp, n_iterations, rows_mul, None)
    q = torch.zeros_like(logits)
    _call("ccd_sinkhorn_assign", logits, logits.shape[1], d_total, int(rows_mul), logits.shape[0], float(temp), log_beta, q)
    return q


def seg_loss(logits, mask_a, idmap_b, grad_scale, loss_out, d_logits=None):
    half = mask_a.shape[0]
    assert logits.shape[0] == 2 * half and logits.is_contiguous()
    _call("ccd_seg_loss", logits, mask_a, idmap_b, half, float(grad_scale), loss_out, d_logits)


# ------------------------------------------------------------------------------------------ supervised segmentation loss
SEG_SUP_MAX_PIXELS = 8192    # H * W of one image: its gt plane is staged in LDS (ccd_hip.h: CCD_SEG_SUP_MAX_PIXELS)
SEG_SUP_MAX_RADIUS = 4       # edge_radius (ccd_hip.h: CCD_SEG_SUP_MAX_RADIUS)
SEG_SUP_PARTS = ("loss", "ce", "dice", "omega")
SEG_SUP_WS_ROW, SEG_SUP_WS_TAIL = 11, 3      # fp64 partial sums per image; behind them Omega, N_v, the invalid gt pixels


def seg_sup_params(class_weight=(1.0, 1.0), ignore_index=255, dice_weight=0.0, edge_weight=0.0, edge_radius=0):
    """The five parameters of the supervised segmentation loss, checked -> (weight_bg, weight_text, ignore_index, dice_weight,
    edge_weight, edge_radius).  ValueError names the parameter that is refused."""
    def number(v):
        return isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v)
    cw = tuple(class_weight) if isinstance(class_weight, (tuple, list)) else None
    if cw is None or len(cw) != 2 or not all(number(v) and v >= 0 for v in cw):
        raise ValueError(f"seg_sup_loss: class_weight must be two finite numbers >= 0 (background, text), got {class_weight!r}")
    if isinstance(ignore_index, bool) or not isinstance(ignore_index, int) or not 2 <= ignore_index <= 255:
        raise ValueError(f"seg_sup_loss: ignore_index must be an integer in 2..255 (0 and 1 are the classes of a uint8 map), got {ignore_index!r}")
    for name, v in (("dice_weight", dice_weight), ("edge_weight", edge_weight)):
        if not number(v) or v < 0:
            raise ValueError(f"seg_sup_loss: {name} must be a finite number >= 0, got {v!r}")
    if isinstance(edge_radius, bool) or not isinstance(edge_radius, int) or not 0 <= edge_radius <= SEG_SUP_MAX_RADIUS:
        raise ValueError(f"seg_sup_loss: edge_radius must be an integer in 0..{SEG_SUP_MAX_RADIUS}, got {edge_radius!r}")
    return float(cw[0]), float(cw[1]), ignore_index, float(dice_weight), float(edge_weight), edge_radius


def _seg_sup_logits(logits, who):
    """fp32 logits [N, 2, H, W] as the kernels read them -> (tensor, image stride, channel stride): the planes stay in place when they
    are contiguous and 16-byte aligned with strides that are multiples of four elements (a channel slice of a wider buffer), a
    dense copy is made otherwise."""
    if logits.dtype != F32:
        raise TypeError(f"{who}: logits must be float32, got {str(logits.dtype)[6:]}")
    if logits.dim() != 4 or logits.shape[1] != 2 or logits.shape[0] < 1:
        raise ValueError(f"{who}: expects logits [N >= 1, 2, H, W], got {list(logits.shape)}")
    N, _, H, W = logits.shape
    if W % 4 != 0 or H * W > SEG_SUP_MAX_PIXELS or H < 1 or W < 4:
        raise ValueError(f"{who}: the kernels take W % 4 == 0 and H * W <= {SEG_SUP_MAX_PIXELS}, got {H} x {W}")
    sn, sc = (logits.stride(0) if N > 1 else 2 * H * W), logits.stride(1)
    if not logits[0, 0].is_contiguous() or logits.data_ptr() % 16 or sn % 4 or sc % 4 or sn < 0 or sc < 0:
        logits = logits.contiguous()
        sn, sc = 2 * H * W, H * W
    return logits, sn, sc


class SegSupLossResult(tuple):
    """(loss fp32 0-dim, parts fp64 [4] = L, CE, Dice, Omega, confusion int64 [2, 2] = [gt, pred]) with the buffers the backward
    pass reads as attributes: ws (fp64), code (uint8 [N, H, W] or None)."""
    ws = code = None


def seg_sup_loss(logits, gt, class_weight=(1.0, 1.0), ignore_index=255, dice_weight=0.0, edge_weight=0.0, edge_radius=0, need_code=True):
    """The fused supervised segmentation loss (kernels/seg_sup_loss.h), forward: fp32 logits [N, 2, H, W] (a channel slice is read
    in place) and a uint8 gt [N, H, W] (0 background, 1 text, ignore_index and every other value not scored) -> SegSupLossResult.
    L = CE + dice_weight * Dice with CE the class- and edge-weighted cross entropy over Omega = sum w and Dice the mean soft Dice
    loss of the images with a scored pixel; a batch without one gives L = 0 (not torch's NaN).  Three device tensors, no
    synchronisation."""
    p = seg_sup_params(class_weight, ignore_index, dice_weight, edge_weight, edge_radius)
    logits, sn, sc = _seg_sup_logits(logits, "seg_sup_loss")
    N, _, H, W = logits.shape
    if gt.dtype != torch.uint8:
        raise TypeError(f"seg_sup_loss: gt must be uint8, got {str(gt.dtype)[6:]}")
    if tuple(gt.shape) != (N, H, W) or gt.device != logits.device:
        raise ValueError(f"seg_sup_loss: gt must be [N, H, W] = {[N, H, W]} on {logits.device}, got {list(gt.shape)} on {gt.device}")
    if not gt[0].is_contiguous() or (N > 1 and gt.stride(0) < 0):
        gt = gt.contiguous()
    dev = logits.device
    ws = torch.empty((N * SEG_SUP_WS_ROW + SEG_SUP_WS_TAIL,), dtype=F64, device=dev)
    code = torch.empty((N, H, W), dtype=torch.uint8, device=dev) if need_code else None
    loss, parts = torch.empty((1,), dtype=F32, device=dev), torch.empty((4,), dtype=F64, device=dev)
    confusion = torch.empty((2, 2), dtype=torch.int64, device=dev)
    _call("ccd_seg_sup_loss_fwd", logits, sn, sc, 2, gt, gt.stride(0) if N > 1 else H * W, N, H, W, p[2], p[0], p[1], p[3], p[4], p[5],
          ws, code, loss, parts, confusion)
    out = SegSupLossResult((loss.view(()), parts, confusion))
    out.ws, out.code = ws, code
    return out


def seg_sup_loss_bwd(logits, code, ws, class_weight=(1.0, 1.0), dice_weight=0.0, edge_weight=0.0, grad_scale=1.0, d_grad=None):
    """The backward pass of seg_sup_loss on the same logits with the code and ws it left: d_logits fp32 [N, 2, H, W] (dense), scaled
    by grad_scale and, when given, by the device scalar d_grad (fp32, one element)."""
    w0, w1, _, dice_weight, edge_weight, _ = seg_sup_params(class_weight, 255, dice_weight, edge_weight, 0)
    logits, sn, sc = _seg_sup_logits(logits, "seg_sup_loss_bwd")
    N, _, H, W = logits.shape
    assert code is not None and code.dtype == torch.uint8 and tuple(code.shape) == (N, H, W) and code.is_contiguous()
    assert ws.dtype == F64 and ws.is_contiguous() and ws.numel() == N * SEG_SUP_WS_ROW + SEG_SUP_WS_TAIL
    if d_grad is not None:
        d_grad = d_grad.reshape(1).to(F32)
    d_logits = torch.empty((N, 2, H, W), dtype=F32, device=logits.device)
    _call("ccd_seg_sup_loss_bwd", logits, sn, sc, 2, code, N, H, W, w0, w1, dice_weight, edge_weight, ws, float(grad_scale), d_grad, d_logits)
    return d_logits


# ------------------------------------------------------------------------------------------ text super-resolution (kernels/sr.h)
SR_LR_SIZE, SR_HR_SIZE = (16, 64), (32, 128)     # TextZoom's sizes, the only ones the task takes
SR_MAX_H, SR_MAX_W = 32, 128                     # one plane of the loss in LDS (ccd_hip.h: CCD_SR_MAX_H / CCD_SR_MAX_W)
SR_MAX_LR_PIXELS = 2048                          # one LR plane of the upsample kernel (ccd_hip.h: CCD_SR_MAX_LR_PIXELS)
SR_PARTS = ("loss", "mse", "gp")
SR_WS_IMAGE = 6                                  # fp64 partial sums per image: (squared error, gradient-map error) x 3 planes


def sr_weight(name, v):
    """A weight of the super-resolution loss, checked -> float.  ValueError names the parameter that is refused."""
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0:
        raise ValueError(f"sr_loss: {name} must be a finite number >= 0, got {v!r}")
    return float(v)


def sr_upsample(lr, mean, std):
    """fp32 lr [N, 3, h, w] -> (base, xin) fp32 [N, 3, 2h, 2w]: base = F.interpolate(lr, scale_factor=2, mode="bicubic",
    align_corners=False) (not clamped), xin = (base - mean[c]) / std[c], in one launch."""
    if lr.dtype != F32:
        raise TypeError(f"sr_upsample: lr must be float32, got {str(lr.dtype)[6:]}")
    if lr.dim() != 4 or lr.shape[1] != 3:
        raise ValueError(f"sr_upsample: expects lr [N, 3, h, w], got {list(lr.shape)}")
    N, _, h, w = lr.shape
    if w % 2 != 0 or h < 1 or w < 2 or h * w > SR_MAX_LR_PIXELS:
        raise ValueError(f"sr_upsample: the kernel takes an even w and h * w <= {SR_MAX_LR_PIXELS}, got {h} x {w}")
    mean, std = [float(v) for v in mean], [float(v) for v in std]
    if len(mean) != 3 or len(std) != 3 or not all(math.isfinite(v) for v in mean) or not all(math.isfinite(v) and v > 0 for v in std):
        raise ValueError(f"sr_upsample: mean / std must be three finite numbers each, std > 0, got {mean!r} / {std!r}")
    lr = lr.contiguous()
    base = torch.empty((N, 3, 2 * h, 2 * w), dtype=F32, device=lr.device)
    xin = torch.empty_like(base)
    _call("ccd_sr_upsample", lr, N, h, w, *mean, *std, base, xin)
    return base, xin


def _sr_pair(sr, hr, who):
    for name, t in (("sr", sr), ("hr", hr)):
        if t.dtype != F32:
            raise TypeError(f"{who}: {name} must be float32, got {str(t.dtype)[6:]}")
    if sr.dim() != 4 or sr.shape[1] != 3:
        raise ValueError(f"{who}: expects sr [N, 3, H, W], got {list(sr.shape)}")
    if tuple(hr.shape) != tuple(sr.shape) or hr.device != sr.device:
        raise ValueError(f"{who}: hr must be {list(sr.shape)} on {sr.device}, got {list(hr.shape)} on {hr.device}")
    N, _, H, W = sr.shape
    if W % 4 != 0 or not 1 <= H <= SR_MAX_H or not 4 <= W <= SR_MAX_W:
        raise ValueError(f"{who}: the kernels take H <= {SR_MAX_H}, W <= {SR_MAX_W} and W % 4 == 0, got {H} x {W}")
    for name, t in (("sr", sr), ("hr", hr)):
        if not t.is_contiguous():
            raise ValueError(f"{who}: {name} must be contiguous (the planes are staged with 16-byte loads), got strides {t.stride()}")
    return N, H, W


class SRLossResult(tuple):
    """(loss fp32 0-dim, parts fp64 [3] = L, mean mse_n, mean gp_n, per_image fp64 [N, 2] = mse_n, gp_n); ws: the per-plane sums."""
    ws = None


def sr_loss_fwd(sr, hr, gp_weight=1e-4):
    """The fused super-resolution loss (kernels/sr.h), forward: fp32 sr, hr [N, 3, H, W] -> SRLossResult.  L = mean_n (mse_n +
    gp_weight gp_n), gp the mean absolute difference of TSRN's gradient maps.  N = 0 gives 0.  Device tensors, no synchronisation."""
    gp_weight = sr_weight("gp_weight", gp_weight)
    N, H, W = _sr_pair(sr, hr, "sr_loss_fwd")
    dev = sr.device
    ws = torch.empty((N * SR_WS_IMAGE,), dtype=F64, device=dev)
    per_image = torch.empty((N, 2), dtype=F64, device=dev)
    loss, parts = torch.empty((1,), dtype=F32, device=dev), torch.empty((3,), dtype=F64, device=dev)
    _call("ccd_sr_loss_fwd", sr, hr, N, H, W, gp_weight, ws, per_image, loss, parts)
    out = SRLossResult((loss.view(()), parts, per_image))
    out.ws = ws
    return out


def sr_loss_bwd(sr, hr, gp_weight=1e-4, grad_scale=1.0, d_grad=None):
    """The backward pass of sr_loss_fwd on the same sr, hr: d_sr fp32 [N, 3, H, W], scaled by grad_scale and, when given, by the
    device scalar d_grad (fp32, one element)."""
    gp_weight = sr_weight("gp_weight", gp_weight)
    N, H, W = _sr_pair(sr, hr, "sr_loss_bwd")
    if d_grad is not None:
        d_grad = d_grad.reshape(1).to(F32)
    d_sr = torch.empty_like(sr)
    _call("ccd_sr_loss_bwd", sr, hr, N, H, W, gp_weight, float(grad_scale), d_grad, d_sr)
    return d_sr


# ------------------------------------------------------------------------------------------ optimiser
def seg_sumsq(grad, chunk_seg, chunk_begin, chunk_len, norm2):
    _call("ccd_seg_sumsq", grad, chunk_seg, chunk_begin, chunk_len, chunk_seg.numel(), norm2)


def adamw(param, grad, exp_avg, exp_avg_sq, mirror, chunk_seg, chunk_begin, chunk_len, hyper, norm2, clip,
          beta1=0.9, beta2=0.999, eps=1e-8):
    _call("ccd_adamw", param, grad, exp_avg, exp_avg_sq, mirror, chunk_seg, chunk_begin, chunk_len, chunk_seg.numel(), hyper, norm2,
          float(clip), float(beta1), float(beta2), float(eps))


def seg_moments(grad, param, chunk_seg, chunk_begin, chunk_len, moments):
    """moments [segments, 3] fp32 += per-tensor {sum g^2, sum p^2, sum g p} (zeroed by the caller)."""
    assert moments.dtype == torch.float32 and moments.is_contiguous() and moments.shape[-1] == 3
    _call("ccd_seg_moments", grad, param, chunk_seg, chunk_begin, chunk_len, chunk_seg.numel(), moments)


def sgd_momentum(param, grad, buf, mirror, chunk_seg, chunk_begin, chunk_len, hyper, norm2, clip, momentum=0.9):
    """hyper [segments, 4] fp32 on the device: lr, weight decay, (unused), active."""
    _call("ccd_sgd_momentum", param, grad, buf, mirror, chunk_seg, chunk_begin, chunk_len, chunk_seg.numel(), hyper, norm2, float(clip),
          float(momentum))


def lars(param, grad, mu, mirror, chunk_seg, chunk_begin, chunk_len, hyper, moments, clip, momentum=0.9, eta=0.001):
    """hyper [segments, 4] fp32 on the device: lr, weight decay, adapt (ndim != 1), active; moments: seg_moments' table."""
    assert moments.shape[-1] == 3 and moments.is_contiguous()
    _call("ccd_lars", param, grad, mu, mirror, chunk_seg, chunk_begin, chunk_len, chunk_seg.numel(), hyper, moments, float(clip),
          float(momentum), float(eta))


def clip_scale(grad, chunk_seg, chunk_begin, chunk_len, norm2, clip):
    _call("ccd_clip_scale", grad, chunk_seg, chunk_begin, chunk_len, chunk_seg.numel(), norm2, float(clip))


def ema(teacher, student, mirror, m, d_m=None):
    """teacher = m teacher + (1 - m) student (+ bf16 mirror); d_m (fp32 [2] on the device: {m, 1 - m}) overrides m at run time."""
    _call("ccd_ema", teacher, student, mirror, teacher.numel(), float(m), float(1.0 - m), d_m)


# ------------------------------------------------------------------------------------------ segmentation head
class ConvDesc(ctypes.Structure):
    """ccd_conv_desc of include/ccd_hip.h (host-side, passed by pointer)."""
    _fields_ = [("g_h_log2", ctypes.c_int), ("g_w_log2", ctypes.c_int), ("s_h", ctypes.c_int), ("s_w", ctypes.c_int),
                ("s_mul", ctypes.c_int), ("cin", ctypes.c_int), ("ntaps", ctypes.c_int),
                ("dy", ctypes.c_byte * 16), ("dx", ctypes.c_byte * 16),
                ("c_map", ctypes.c_int), ("c_py", ctypes.c_int), ("c_px", ctypes.c_int)]


def conv_desc(grid_hw, src_hw, cin, taps, s_mul=1, parity=None):
    """grid_hw: output-row grid (powers of two); taps: [(dy, dx)]; parity (py, px) turns on the 2x scatter."""
    gh, gw = grid_hw
    assert gh & (gh - 1) == 0 and gw & (gw - 1) == 0 and 1 <= len(taps) <= 16
    d = ConvDesc()
    d.g_h_log2, d.g_w_log2 = gh.bit_length() - 1, gw.bit_length() - 1
    d.s_h, d.s_w, d.s_mul, d.cin, d.ntaps = src_hw[0], src_hw[1], s_mul, cin, len(taps)
    for i, (a, b) in enumerate(taps):
        d.dy[i], d.dx[i] = a, b
    if parity is not None:
        d.c_map, d.c_py, d.c_px = 1, parity[0], parity[1]
    return d


def conv_gemm(src, desc, w, rows, out, *, bias=None, colsum=None, colsumsq=None):
    """out[rows -> c_map, N] (bf16) = gather(src)[rows, ntaps*cin] @ w[N, ntaps*cin]^T (+ bias); stats += column sums."""
    N = w.shape[0]
    assert w.shape[1] == desc.ntaps * desc.cin and src.dim() == 2 and out.dim() == 2 and out.shape[1] >= N
    with _Span("conv_gemm", 2.0 * rows * N * w.shape[1], 2.0 * (src.numel() + w.numel() + rows * N)):
        _call("ccd_conv_gemm", src, src.stride(0), desc, w, w.stride(0), rows, N, out, out.stride(0), bias, colsum, colsumsq)
    return out


def conv_wgrad(a, src, desc, out):
    """out[P, ntaps*cin] (fp32) += a[rows, P]^T @ gather(src)[rows, ntaps*cin] (implicit patch matrix)."""
    rows, Pd = a.shape
    assert tuple(out.shape) == (Pd, desc.ntaps * desc.cin)
    with _Span("conv_wgrad", 2.0 * rows * Pd * out.shape[1], 2.0 * (a.numel() + src.numel()) + 4.0 * out.numel()):
        _call("ccd_conv_wgrad", a, a.stride(0), Pd, src, src.stride(0), desc, rows, out, out.stride(0))
    return out


def im2col(src, desc, rows, out=None):
    if out is None:
        out = torch.empty((rows, desc.ntaps * desc.cin), dtype=BF16, device=src.device)
    assert out.is_contiguous() and out.numel() == rows * desc.ntaps * desc.cin
    _call("ccd_im2col", src, src.stride(0), desc, rows, out)
    return out


def bn_finalize(stats, count, eps, momentum, mean_rstd, running_mean, running_var):
    C = running_mean.numel()
    assert stats.numel() == 2 * C and mean_rstd.numel() == 2 * C
    _call("ccd_bn_finalize", stats, float(count), float(eps), float(momentum), mean_rstd, running_mean, running_var, C)


def bn_relu_fwd(x, mean_rstd, gamma, beta, out):
    rows, C = x.shape
    _call("ccd_bn_relu_fwd", x, x.stride(0), mean_rstd, gamma, beta, out, out.stride(0), rows, C)
    return out


def bn_relu_bwd_reduce(dy, x, mean_rstd, gamma, beta, red):
    rows, C = x.shape
    _call("ccd_bn_relu_bwd_reduce", dy, dy.stride(0), x, x.stride(0), mean_rstd, gamma, beta, red, rows, C)


def bn_relu_bwd_apply(dy, x, mean_rstd, gamma, beta, red, count, red_local, dgamma, dbeta, dx):
    rows, C = x.shape
    _call("ccd_bn_relu_bwd_apply", dy, dy.stride(0), x, x.stride(0), mean_rstd, gamma, beta, red, float(count), red_local, dgamma, dbeta,
          dx, dx.stride(0), rows, C)
    return dx


def cls_gather_fwd(zT, bias, images, H, W):
    """zT fp32 [>=18, pixels] (row co*9+tap) -> fp32 logits [images, 2, H, W]."""
    assert zT.shape[0] >= 18 and zT.shape[1] == images * H * W
    logits = torch.empty((images, 2, H, W), dtype=F32, device=zT.device)
    _call("ccd_cls_gather_fwd", zT, zT.stride(0), bias, logits, images, H, W)
    return logits


def cls_grad_cols(dlogits, images, H, W):
    """fp32 dlogits [images, 2, H, W] -> bf16 g [pixels, 64] (column co*9+tap = shifted gradient plane)."""
    assert dlogits.is_contiguous() and tuple(dlogits.shape) == (images, 2, H, W)
    g = torch.empty((images * H * W, 64), dtype=BF16, device=dlogits.device)
    _call("ccd_cls_grad_cols", dlogits, g, images, H, W)
    return g


def img_gather_fwd(zT, bias, base, images, H, W):
    """zT fp32 [>=27, pixels] (row co*9+tap), base fp32 [images, 3, H, W] -> fp32 sr [images, 3, H, W] = base + bias + the tap sums."""
    assert zT.shape[0] >= 27 and zT.shape[1] == images * H * W and bias.numel() == 3
    assert base.dtype == F32 and base.is_contiguous() and tuple(base.shape) == (images, 3, H, W) and base.device == zT.device
    sr = torch.empty((images, 3, H, W), dtype=F32, device=zT.device)
    _call("ccd_img_gather_fwd", zT, zT.stride(0), bias, base, sr, images, H, W)
    return sr


def img_grad_cols(d_sr, images, H, W):
    """fp32 d_sr [images, 3, H, W] -> bf16 g [pixels, 64] (column co*9+tap < 27 = shifted gradient plane, the rest zero)."""
    assert d_sr.is_contiguous() and tuple(d_sr.shape) == (images, 3, H, W)
    g = torch.empty((images * H * W, 64), dtype=BF16, device=d_sr.device)
    _call("ccd_img_grad_cols", d_sr, g, images, H, W)
    return g


def cls_tail_supported(y, H, W):
    """The fused BatchNorm + ReLU + classifier kernels exist for the reference's head shape only (kernels/cls_tail.h)."""
    return y.shape[1] == 128 and (H, W) == (32, 128) and y.stride(0) % 8 == 0


def cls_tail_fwd(y, mean_rstd, gamma, beta, w, bias, images, H, W):
    """logits fp32 [images, 2, H, W] = Conv2d(C, 2, 3, padding=1)(relu(bn(y))); y bf16 [images*H*W, C] BEFORE its BatchNorm."""
    C = y.shape[1]
    assert y.shape[0] == images * H * W and y.stride(1) == 1 and w.is_contiguous() and tuple(w.shape) == (2, C, 3, 3)
    logits = torch.empty((images, 2, H, W), dtype=F32, device=y.device)
    _call("ccd_cls_tail_fwd", y, y.stride(0), mean_rstd, gamma, beta, w, bias, logits, images, H, W, C)
    return logits


def cls_tail_bwd_reduce(dlogits, y, mean_rstd, gamma, beta, w, red, db_cls, images, H, W):
    """red [2C] += BatchNorm's two backward sums of d(relu(bn(y))) under the classifier; db_cls [2] += sum dlogits."""
    C = y.shape[1]
    assert dlogits.is_contiguous() and tuple(dlogits.shape) == (images, 2, H, W) and y.shape[0] == images * H * W
    assert w.is_contiguous() and red.numel() == 2 * C and red.is_contiguous() and db_cls.is_contiguous()
    _call("ccd_cls_tail_bwd_reduce", dlogits, y, y.stride(0), mean_rstd, gamma, beta, w, red, db_cls, images, H, W, C)
    return red


def cls_tail_bwd_apply(dlogits, y, mean_rstd, gamma, beta, w, red, count, red_local, dgamma, dbeta, dw_cls, dbias_t, dy,
                       images, H, W):
    """dy bf16 [images*H*W, C] = gradient w.r.t. y; dgamma / dbeta / dw_cls [2, C, 3, 3] / dbias_t [C] accumulate (fp32)."""
    C = y.shape[1]
    assert dlogits.is_contiguous() and y.shape[0] == images * H * W and dy.shape == y.shape and dy.stride(1) == 1
    assert dw_cls.is_contiguous() and tuple(dw_cls.shape) == (2, C, 3, 3) and dbias_t.is_contiguous() and dbias_t.numel() == C
    assert dgamma.is_contiguous() and dbeta.is_contiguous() and red.is_contiguous() and red_local.is_contiguous()
    _call("ccd_cls_tail_bwd_apply", dlogits, y, y.stride(0), mean_rstd, gamma, beta, w, red, float(count), red_local, dgamma, dbeta, dw_cls,
          dbias_t, dy, dy.stride(0), images, H, W, C)
    return dy


def permute4(src, strides, dims, dst, accumulate=False, dst_strides=None):
    """dst[idx . dst_strides] (bf16 cast, or fp32 += when accumulate) <- src.flatten()[idx . strides]; dst_strides
    default to contiguous over `dims`."""
    _chk(dst, F32 if accumulate else BF16, "dst")
    n = list(dims) + [1] * (4 - len(dims))
    s = list(strides) + [0] * (4 - len(strides))
    if dst_strides is None:
        d = [n[1] * n[2] * n[3], n[2] * n[3], n[3], 1]
        assert dst.is_contiguous() and dst.numel() == n[0] * n[1] * n[2] * n[3]
    else:
        d = list(dst_strides) + [0] * (4 - len(dst_strides))
    arr_l, arr_i = ctypes.c_long * 4, ctypes.c_int * 4
    _call("ccd_permute4", src, arr_l(*s), arr_l(*d), arr_i(*n), dst, 1 if accumulate else 0)
    return dst


class _PermuteJob(ctypes.Structure):
    _fields_ = [("src", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("src_strides", ctypes.c_long * 4),
                ("dst_strides", ctypes.c_long * 4), ("dims", ctypes.c_int * 4)]


PERMUTE_MULTI_MAX = 24


def permute4_multi(jobs, accumulate=False):
    """jobs: [(src, strides, dims, dst[, dst_strides])] - ops.permute4's arguments, up to 24 of them in ONE launch."""
    for lo in range(0, len(jobs), PERMUTE_MULTI_MAX):
        part = jobs[lo:lo + PERMUTE_MULTI_MAX]
        arr = (_PermuteJob * len(part))()
        for k, job in enumerate(part):
            src, strides, dims, dst = job[:4]
            dst_strides = job[4] if len(job) > 4 else None
            _chk(src, F32, "src"); _chk(dst, F32 if accumulate else BF16, "dst")
            n = list(dims) + [1] * (4 - len(dims))
            s_ = list(strides) + [0] * (4 - len(strides))
            if dst_strides is None:
                d = [n[1] * n[2] * n[3], n[2] * n[3], n[3], 1]
                assert dst.is_contiguous() and dst.numel() == n[0] * n[1] * n[2] * n[3]
            else:
                d = list(dst_strides) + [0] * (4 - len(dst_strides))
            arr[k].src, arr[k].dst = src.data_ptr(), dst.data_ptr()
            arr[k].src_strides[:], arr[k].dst_strides[:], arr[k].dims[:] = s_, d, n
        _call("ccd_permute4_multi", arr, len(part), 1 if accumulate else 0)


class _BnFinalizeJob(ctypes.Structure):
    _fields_ = [("stats", ctypes.c_void_p), ("mean_rstd", ctypes.c_void_p), ("running_mean", ctypes.c_void_p),
                ("running_var", ctypes.c_void_p), ("batches", ctypes.c_void_p), ("count", ctypes.c_float), ("eps", ctypes.c_float),
                ("momentum", ctypes.c_float), ("C", ctypes.c_int)]


def bn_finalize_multi(jobs):
    """jobs: [(stats, count, eps, momentum, mean_rstd, running_mean, running_var, num_batches_tracked or None)], at most 4: the
    BatchNorm layers of one level in one launch (mean / rstd, running statistics, batch counter)."""
    assert 1 <= len(jobs) <= 4
    arr = (_BnFinalizeJob * len(jobs))()
    for k, (stats, count, eps, momentum, mean_rstd, rm, rv, nb) in enumerate(jobs):
        C = rm.numel()
        assert stats.numel() == 2 * C and mean_rstd.numel() == 2 * C and (nb is None or nb.dtype == torch.int64)
        arr[k].stats, arr[k].mean_rstd, arr[k].running_mean, arr[k].running_var = (t.data_ptr() for t in (stats, mean_rstd, rm, rv))
        arr[k].batches = nb.data_ptr() if nb is not None else None
        arr[k].count, arr[k].eps, arr[k].momentum, arr[k].C = float(count), float(eps), float(momentum), C
    _call("ccd_bn_finalize_multi", arr, len(jobs))


# ------------------------------------------------------------------------------------------------ finetune path
I64 = torch.int64


def dropout(src, p, seed, *, resid=None, out=None, out_dtype=None):
    """out = (resid if given) + Dropout_p(src) with the counter-based mask of `seed` (ccd_hip.h: ccd_dropout)."""
    assert src.is_contiguous() and src.dtype in (F32, BF16)
    if out is None:
        out = torch.empty(src.shape, dtype=out_dtype or src.dtype, device=src.device)
    assert out.is_contiguous() and out.shape == src.shape and out.dtype in (F32, BF16)
    _call("ccd_dropout", src, int(src.dtype == BF16), resid, out, int(out.dtype == BF16), src.numel(), int(seed) & 0xFFFFFFFFFFFFFFFF,
          float(p))
    return out


def droppath_scales(keep, samples, seed, d_seed=None):
    """keep fp32 [depth] (device) -> fp32 [depth, 2, samples]: per-(block, branch, sample) DropPath scale (0 or 1/keep).
    d_seed (int64 [1] on the device, optional) is added to `seed` when the kernel runs (HIP-graph replays)."""
    out = torch.empty((keep.shape[0], 2, samples), dtype=F32, device=keep.device)
    _call("ccd_droppath_scales", keep, out, 2 * samples, keep.shape[0], int(seed) & 0xFFFFFFFFFFFFFFFF, d_seed)
    return out


def dec_embed_fwd(tokens, emb, pos, p=0.0, seed=0):
    """tokens int64 [B,T] -> x fp32 [B*T, D] = dropout(emb[tokens] + pos[:T])."""
    assert tokens.dtype == I64 and tokens.is_contiguous()
    B, T = tokens.shape
    D = emb.shape[1]
    x = torch.empty((B * T, D), dtype=F32, device=emb.device)
    _call("ccd_dec_embed_fwd", tokens, emb, pos, x, B * T, T, D, emb.shape[0], int(seed) & 0xFFFFFFFFFFFFFFFF, float(p))
    return x


def dec_embed_bwd(tokens, dx, demb, padding_idx, p=0.0, seed=0):
    _call("ccd_dec_embed_bwd", tokens, dx, demb, tokens.numel(), dx.shape[1], demb.shape[0], int(padding_idx),
          int(seed) & 0xFFFFFFFFFFFFFFFF, float(p))


def dec_attn_fwd(q, k, v, B, H, Tq, Tk, scale, *, tokens=None, key_len=None, pad_idx=-1, causal=False, p=0.0, seed=0,
                 want_probs=False):
    """q [B*Tq, >=64H] / k, v [B*Tk, >=64H] bf16 2-D views (row stride = .stride(0)) -> (out bf16 [B*Tq, 64H], lse, probs)."""
    for t_ in (q, k, v):
        assert t_.dtype == BF16 and t_.dim() == 2 and t_.stride(1) == 1
    out = torch.empty((B * Tq, 64 * H), dtype=BF16, device=q.device)
    lse = torch.empty((B, H, Tq), dtype=F32, device=q.device)
    probs = torch.empty((B, H, Tq, Tk), dtype=F32, device=q.device) if want_probs else None
    _call("ccd_dec_attn_fwd", q, q.stride(0), k, k.stride(0), v, v.stride(0), out, out.stride(0), lse, probs, tokens, key_len, int(pad_idx),
          int(causal), B, H, Tq, Tk, float(scale), int(seed) & 0xFFFFFFFFFFFFFFFF, float(p))
    return out, lse, probs


def dec_attn_bwd(q, k, v, out, d_out, lse, dq, dk, dv, B, H, Tq, Tk, scale, *, tokens=None, key_len=None, pad_idx=-1,
                 causal=False, p=0.0, seed=0):
    """dq / dk / dv: preallocated bf16 2-D views the gradients are written into (all rows, head columns only)."""
    for t_ in (q, k, v, dq, dk, dv):
        assert t_.dtype == BF16 and t_.dim() == 2 and t_.stride(1) == 1
    assert out.stride(0) == d_out.stride(0)
    _call("ccd_dec_attn_bwd", q, q.stride(0), k, k.stride(0), v, v.stride(0), out, d_out, out.stride(0), lse, tokens, key_len, int(pad_idx),
          int(causal), B, H, Tq, Tk, float(scale), int(seed) & 0xFFFFFFFFFFFFFFFF, float(p), dq, dq.stride(0), dk, dk.stride(0), dv,
          dv.stride(0))


def tf_loss_fwd(logits, C, targets, pad_idx):
    """logits fp32 [B*T, ld>=C], targets int64 [B,T] -> (row_lse [B*T], acc [2] = (sum of NLL, counted rows))."""
    assert targets.dtype == I64 and targets.is_contiguous()
    B, T = targets.shape
    row_lse = torch.empty(B * T, dtype=F32, device=logits.device)
    acc = torch.empty(2, dtype=F32, device=logits.device)
    _call("ccd_tf_loss_fwd", logits, logits.stride(0), int(C), targets, B * T, T, int(pad_idx), row_lse, acc)
    return row_lse, acc


def tf_loss_bwd(logits, C, targets, pad_idx, row_lse, acc, upstream, ldd):
    """upstream: fp32 device scalar (the gradient arriving at the loss) or None for 1."""
    B, T = targets.shape
    d = torch.empty((B * T, ldd), dtype=BF16, device=logits.device)
    _call("ccd_tf_loss_bwd", logits, logits.stride(0), int(C), targets, B * T, T, int(pad_idx), row_lse, acc, upstream, d, ldd)
    return d


def greedy_step(logits, C, probs, step, seq):
    """probs fp32 [B, steps, C], seq int64 [B, seq_len]: writes probs[:, step] and seq[:, step+1]."""
    assert seq.dtype == I64 and seq.is_contiguous() and probs.is_contiguous()
    B = seq.shape[0]
    _call("ccd_greedy_step", logits, logits.stride(0), int(C), B, probs, probs.shape[1], int(step), seq, seq.shape[1])


# ------------------------------------------------------------------------------------------ parallel attention head (kernels/posattn.h)
POSATTN_TOKENS, POSATTN_MAX_T = 256, 32                   # posattn.h: PA_TOK, PA_TQ


def _posattn_views(fn, E, **views):
    for name, t in views.items():
        if t.dtype != BF16:
            raise TypeError(f"{fn}: {name} must be bfloat16, got {t.dtype}")
        if t.dim() != 2 or t.shape[1] != E or (t.shape[0] > 0 and t.stride(1) != 1):
            raise ValueError(f"{fn}: {name} must be a 2-D view of {E} dense columns, got {list(t.shape)}, strides {t.stride()}")


def _posattn_ld(t):
    return t.stride(0) if t.shape[0] > 1 else t.shape[1]


def posattn_fwd(P, X, Q0, We, be, T):
    """The parallel attention head's scores, softmax and glimpses in one launch (kernels/posattn.h; tests/parallel_attn_np.py is the
    specification): P = X Wv^T + bv and X bf16 [N * 256, E] 2-D views (any row stride that is a multiple of 8, 16-byte aligned rows), Q0
    bf16 [256, E], We bf16 [32, E] with rows T.. zero, be fp32 [T] -> (attn fp32 [N, T, 256], G bf16 [N * 32, E]).  attn[n, t] = softmax
    over the 256 tokens of be[t] + tanh(P_n + Q0) We[t]; G[n * 32 + t] = attn[n, t] X_n, rows T..31 of every image zero.  tanh(P + Q0) is
    never stored.  E a multiple of 64 up to 768, 1 <= T <= 32; two runs give the same bits."""
    E, T = int(Q0.shape[-1]), int(T)
    _posattn_views("posattn_fwd", E, P=P, X=X, Q0=Q0, We=We)
    if P.shape[0] != X.shape[0]:
        raise ValueError(f"posattn_fwd: P has {P.shape[0]} rows, X {X.shape[0]}")
    rows = P.shape[0]
    N = rows // POSATTN_TOKENS
    tokens = POSATTN_TOKENS if rows == N * POSATTN_TOKENS else rows      # (not whole images: the library refuses the shape)
    if tuple(Q0.shape) != (POSATTN_TOKENS, E) or tuple(We.shape) != (POSATTN_MAX_T, E) or not Q0.is_contiguous() or not We.is_contiguous():
        raise ValueError(f"posattn_fwd: Q0 must be a dense [256, {E}] and We a dense [32, {E}], got {list(Q0.shape)} and {list(We.shape)}")
    if be.dtype != F32 or be.numel() < T:
        raise ValueError(f"posattn_fwd: be must hold {T} fp32 values, got {be.dtype} {list(be.shape)}")
    attn = torch.empty((N, max(T, 0), POSATTN_TOKENS), dtype=F32, device=P.device)
    G = torch.empty((N * POSATTN_MAX_T, E), dtype=BF16, device=P.device)
    _call("ccd_posattn_fwd", P, _posattn_ld(P), X, _posattn_ld(X), Q0, We, be, attn, G, E, N, tokens, E, T)
    return attn, G


def posattn_bwd(dG, X, P, Q0, We, attn, out=None):
    """Backward of posattn_fwd given dG bf16 [N * 32, E] (rows T.. of an image are not read): -> (dX1 bf16 [N * 256, E] = attn^T dG, dP bf16
    [N * 256, E] = dM (1 - tanh(P + Q0)^2), dQ0 fp32 [256, E] = sum_n dP_n, dWe fp32 [32, E], dbe fp32 [32]).  The gradient of X through
    P (dP Wv), dWv and dbv are the caller's GEMMs on dP.  `out` = (dX1, dP) 2-D views to write into (row strides multiples of 8).  The
    sums over the images are folded by a finishing launch in a fixed order (ccd_posattn_fold): no atomics, two runs give the same bits."""
    E = int(Q0.shape[-1])
    N, T = int(attn.shape[0]), int(attn.shape[1])
    dX1, dP = out if out is not None else (torch.empty((N * POSATTN_TOKENS, E), dtype=BF16, device=X.device) for _ in range(2))
    _posattn_views("posattn_bwd", E, dG=dG, X=X, P=P, Q0=Q0, We=We, dX1=dX1, dP=dP)
    if attn.dtype != F32 or attn.dim() != 3 or attn.shape[2] != POSATTN_TOKENS or not attn.is_contiguous():
        raise ValueError(f"posattn_bwd: attn must be a dense fp32 [N, T, 256], got {attn.dtype} {list(attn.shape)}")
    for name, t, rows in (("dG", dG, N * POSATTN_MAX_T), ("X", X, N * POSATTN_TOKENS), ("P", P, N * POSATTN_TOKENS),
                          ("dX1", dX1, N * POSATTN_TOKENS), ("dP", dP, N * POSATTN_TOKENS), ("Q0", Q0, POSATTN_TOKENS), ("We", We, POSATTN_MAX_T)):
        if t.shape[0] != rows:
            raise ValueError(f"posattn_bwd: {name} must have {rows} rows for {N} images, got {t.shape[0]}")
    if not Q0.is_contiguous() or not We.is_contiguous():
        raise ValueError("posattn_bwd: Q0 and We must be dense")
    dWe_part = torch.empty((N, POSATTN_MAX_T, E), dtype=F32, device=X.device)
    dbe_part = torch.empty((N, POSATTN_MAX_T), dtype=F32, device=X.device)
    dQ0 = torch.empty((POSATTN_TOKENS, E), dtype=F32, device=X.device)
    dWe = torch.empty((POSATTN_MAX_T, E), dtype=F32, device=X.device)
    dbe = torch.empty(POSATTN_MAX_T, dtype=F32, device=X.device)
    _call("ccd_posattn_bwd", dG, _posattn_ld(dG), X, _posattn_ld(X), P, _posattn_ld(P), Q0, We, attn, dX1, _posattn_ld(dX1), dP,
          _posattn_ld(dP), dWe_part, dbe_part, N, POSATTN_TOKENS, E, T)
    _call("ccd_posattn_fold", dP, _posattn_ld(dP), dWe_part, dbe_part, dQ0, dWe, dbe, N, E)
    return dX1, dP, dQ0, dWe, dbe
