"""The checks of the parallel attention head (kernels/posattn.h: ccd_posattn_fwd / _bwd / _fold; ccd_amd/decoder/parallel_attn_decoder.py)
that run on either backend: the CPU SIMT executor (tests/test_parallel_attn_sim.py) and the MI355X (tests/test_parallel_attn_gpu.py).
`device` is where the tensors live.  tests/parallel_attn_np.py is the specification.

Gates (those of check_dec_attn in tests/kernel_checks.py, for the same reason - bf16 operands, fp32 accumulation):
  * probabilities a: rtol 2e-3, atol 1e-5;   G: rtol 1e-2, atol 1e-2;   every gradient: rtol 2e-2, atol 2e-2 * max |reference|.
The kernels take P, X, Q0, We as bf16 and the specification is evaluated in fp64 on exactly those bf16 values, so the gates measure the
kernels' arithmetic alone.  Except in the one case at the default scale, We is scaled until the maps are peaked (median peak probability
above 0.1, asserted on the reference): nearly uniform maps would hide a broken softmax or a wrong token order."""
import numpy as np
import pytest
import torch

import parallel_attn_np as S

BF16, F32 = torch.bfloat16, torch.float32
PEAKED = 5.0                                   # We ~ N(0, (PEAKED / sqrt(E))^2): score std ~ 3 over the tokens, see kernel_case


def close(got, want, rtol, atol, what):
    got, want = got.detach().double().cpu().numpy(), np.asarray(want, np.float64)
    assert got.shape == want.shape, f"{what}: shape {got.shape} vs {want.shape}"
    err = np.abs(got - want)
    bad = ~(err <= atol + rtol * np.abs(want))
    print(f"{what}: max err {err.max() if err.size else 0:.4g} (want max {np.abs(want).max() if want.size else 0:.4g})")
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.size} off, max err {err.max():.4g} (want max {np.abs(want).max():.4g})"


def grad_close(got, want, what):
    close(got, want, 2e-2, 2e-2 * float(np.abs(want).max()) + 1e-12, what)


_CASES = {}


def kernel_case(N, E, T, we_scale, seed=5):
    """Operands (bf16 on the host) and the fp64 reference, computed once per shape.  P and X live in wider buffers (row strides larger
    than E).  we_scale None = the default initialisation's scale of nn.Linear(E, T): U(-1 / sqrt(E), 1 / sqrt(E))."""
    key = (N, E, T, we_scale, seed)
    if key in _CASES:
        return _CASES[key]
    g = torch.Generator().manual_seed(seed)
    pbuf = torch.randn(N * 256, E + 24, generator=g).to(BF16)
    xbuf = torch.randn(N * 256, 2 * E + 8, generator=g).to(BF16)
    Q0 = (0.5 * torch.randn(256, E, generator=g)).to(BF16)
    We = torch.zeros(32, E, dtype=BF16)
    if we_scale is None:
        We[:T] = ((torch.rand(T, E, generator=g) * 2 - 1) / E ** 0.5).to(BF16)
    else:
        We[:T] = (torch.randn(T, E, generator=g) * we_scale / E ** 0.5).to(BF16)
    be = torch.randn(T, generator=g)
    dG = torch.zeros(N * 32, E + 8, dtype=BF16)
    dG.view(N, 32, E + 8)[:, :T, :E] = torch.randn(N, T, E, generator=g).to(BF16)
    dG.view(N, 32, E + 8)[:, T:] = 7.0                                 # rows T.. of dG must not be read
    f64 = lambda t: t.double().numpy()
    P, X = pbuf[:, 8:8 + E], xbuf[:, E:2 * E]
    a, G = S.core_forward(f64(P).reshape(N, 256, E), f64(X).reshape(N, 256, E), f64(Q0), f64(We[:T]), f64(be))
    grads = S.core_backward(f64(dG.view(N, 32, E + 8)[:, :T, :E]), f64(X).reshape(N, 256, E), f64(P).reshape(N, 256, E), f64(Q0),
                            f64(We[:T]), a)
    peak = float(np.median(a.max(axis=2))) if N else 0.0
    absda = np.abs(f64(dG.view(N, 32, E + 8)[:, :T, :E])) @ np.abs(f64(X).reshape(N, 256, E)).transpose(0, 2, 1)      # [N, T, 256]
    dbe_bound = (2 * E + 512 + 256 * N) * 2.0 ** -24 * (a * (absda + (a * absda).sum(axis=2, keepdims=True))).sum(axis=(0, 2))
    if we_scale is not None and N:
        assert peak > 0.1, f"the inputs do not give peaked maps: median peak probability {peak:.3f}"
    _CASES[key] = dict(pbuf=pbuf, xbuf=xbuf, Q0=Q0, We=We, be=be, dG=dG, a=a, G=G, grads=grads, peak=peak, dbe_bound=dbe_bound)
    return _CASES[key]


def _run(device, c, N, E, T):
    from ccd_amd import ops
    P, X = c["pbuf"].to(device)[:, 8:8 + E], c["xbuf"].to(device)[:, E:2 * E]
    Q0, We, be, dG = c["Q0"].to(device), c["We"].to(device), c["be"].to(device), c["dG"].to(device)[:, :E]
    attn, G = ops.posattn_fwd(P, X, Q0, We, be, T)
    dxb = torch.zeros(N * 256, E + 8, dtype=BF16, device=device)
    dpb = torch.zeros(N * 256, E + 16, dtype=BF16, device=device)
    out = ops.posattn_bwd(dG, X, P, Q0, We, attn, out=(dxb[:, :E], dpb[:, :E]))
    return attn, G, out, dxb, dpb


def check_kernels(device, N, E, T, we_scale=PEAKED):
    c = kernel_case(N, E, T, we_scale)
    attn, G, (dX1, dP, dQ0, dWe, dbe), dxb, dpb = _run(device, c, N, E, T)
    assert tuple(attn.shape) == (N, T, 256) and attn.dtype == F32                # exactly T rows per image
    assert tuple(G.shape) == (N * 32, E) and G.dtype == BF16
    close(attn, c["a"], 2e-3, 1e-5, "posattn/a")
    Gv = G.view(N, 32, E)
    close(Gv[:, :T], c["G"], 1e-2, 1e-2, "posattn/G")
    assert (Gv[:, T:] == 0).all(), "rows T..31 of G must be exactly zero"
    r = c["grads"]
    grad_close(dX1.view(N, 256, E), r["dX1"], "posattn/dX1")
    grad_close(dP.view(N, 256, E), r["dP"], "posattn/dP")
    grad_close(dQ0, r["dQ0"], "posattn/dQ0")
    grad_close(dWe[:T], r["dWe"], "posattn/dWe")
    # dbe is exactly zero in exact arithmetic (every softmax row's gradient sums to zero), so "2e-2 * max |reference|" is no gate.
    # The kernel sums fp32 dA = a (da - delta): with u = 2^-24, |da| carries E u absda (absda = sum_e |dG| |X|), delta another
    # 256 u sum_s a absda, and the sum over the 256 N terms 256 N u of their magnitudes: bound = (2 E + 512 + 256 N) u sum a (absda + <a, absda>)
    assert (np.abs(dbe[:T].double().cpu().numpy()) <= c["dbe_bound"]).all(), (dbe[:T], c["dbe_bound"])
    assert (dWe[T:] == 0).all() and (dbe[T:] == 0).all()
    assert (dxb[:, E:] == 0).all() and (dpb[:, E:] == 0).all(), "nothing outside the [:, :E] views may be written"
    return c["peak"]


def check_default_scale(device, N=1, E=64, T=25):
    peak = check_kernels(device, N, E, T, we_scale=None)
    assert peak < 0.05                                                 # the nearly uniform maps of the default initialisation


def check_saturation(device, N=1, E=64, T=25):
    """One-hot maps and tanh = +-1 in fp32: everything stays finite, every map sums to 1, dP is 0 where M^2 rounds to 1."""
    from ccd_amd import ops
    g = torch.Generator().manual_seed(9)
    P = (torch.randn(N * 256, E, generator=g) * 40).to(BF16)
    P[P.abs() < 12] = 12.0                                             # |P + Q0| >= 11: 1 - tanh^2 < 2^-24
    X = torch.randn(N * 256, E, generator=g).to(BF16)
    Q0 = torch.randn(256, E, generator=g).clamp(-1, 1).to(BF16)
    We = torch.zeros(32, E, dtype=BF16)
    We[:T] = (torch.randn(T, E, generator=g) * 600).to(BF16)          # score gaps of hundreds between tokens
    be = torch.zeros(T)
    dG = torch.zeros(N * 32, E, dtype=BF16)
    dG.view(N, 32, E)[:, :T] = torch.randn(N, T, E, generator=g).to(BF16)
    dev = lambda t: t.to(device)
    a, _ = S.core_forward(P.double().view(N, 256, E), X.double().view(N, 256, E), Q0.double(), We[:T].double(), be.double())
    assert a.max(axis=2).min() > 0.999, "the inputs do not give one-hot maps"
    attn, G = ops.posattn_fwd(dev(P), dev(X), dev(Q0), dev(We), dev(be), T)
    dX1, dP, dQ0, dWe, dbe = ops.posattn_bwd(dev(dG), dev(X), dev(P), dev(Q0), dev(We), attn)
    for name, t in dict(attn=attn, G=G, dX1=dX1, dP=dP, dQ0=dQ0, dWe=dWe, dbe=dbe).items():
        assert torch.isfinite(t.float()).all(), name
    assert float((attn.double().sum(-1) - 1).abs().max()) <= 1e-5
    assert float(attn.max(-1).values.min()) > 0.999, "the maps should be one-hot"
    M = torch.tanh(P.float() + Q0.float().repeat(N, 1))
    assert (M * M == 1).all()
    assert (dP[(M * M == 1).to(device)] == 0).all()
    close(attn, a, 2e-3, 1e-5, "saturated/a")


def check_repeatable(device, N=3, E=192, T=25):
    c = kernel_case(N, E, T, PEAKED)
    one = _run(device, c, N, E, T)
    two = _run(device, c, N, E, T)
    flat = lambda r: [r[0], r[1], *r[2]]
    for x, y in zip(flat(one), flat(two)):
        assert torch.equal(x.view(torch.int16 if x.dtype == BF16 else torch.int32), y.view(torch.int16 if y.dtype == BF16 else torch.int32))


def check_abi(device):
    """CCD_ESHAPE (-2) before any launch for every unsupported shape, N = 0 succeeds.  None of these launches anything."""
    from ccd_amd import _lib, ops
    lib, st = _lib.get(), _lib.stream()
    E, T, N = 64, 25, 1
    z = lambda *s, dt=BF16: torch.zeros(*s, dtype=dt, device=device)
    P, X, Q0, We, be = z(N * 256, E), z(N * 256, E), z(256, E), z(32, E), z(T, dt=F32)
    attn, G, dG = z(N, 32, 256, dt=F32), z(N * 32, E), z(N * 32, E)
    dX1, dP, dWp, dbp = z(N * 256, E), z(N * 256, E), z(N, 32, E, dt=F32), z(N, 32, dt=F32)
    wide = z(N * 256, E + 8)

    def fwd(view=P, ld=E, tokens=256, E=E, T=T, N=N):
        return lib.ccd_posattn_fwd(view, ld, X, 64, Q0, We, be, attn, G, 64, N, tokens, E, T, st)

    def bwd(view=dP, ld=E, tokens=256, E=E, T=T, N=N):
        return lib.ccd_posattn_bwd(dG, 64, X, 64, P, 64, Q0, We, attn, dX1, 64, view, ld, dWp, dbp, N, tokens, E, T, st)

    for f in (fwd, bwd):                                               # (the varied view: P of the forward, dP of the backward)
        assert f() == 0                                                # the base line itself is valid
        assert f(E=96) == -2 and f(E=0) == -2 and f(E=832) == -2       # E % 64, E <= 768
        assert f(T=0) == -2 and f(T=33) == -2
        assert f(tokens=255) == -2 and f(tokens=128) == -2
        assert f(view=wide[:, 4:4 + E], ld=E + 8) == -2                # rows 8 bytes off a 16-byte boundary
        assert f(ld=E + 4) == -2 and f(ld=E - 8) == -2                 # stride not a multiple of 8 / below E
        assert f(N=0) == 0
    assert lib.ccd_posattn_fwd(None, E, None, E, None, None, None, None, None, E, 0, 256, E, T, st) == 0
    assert lib.ccd_posattn_bwd(None, E, None, E, None, E, None, None, None, None, E, None, E, None, None, 0, 256, E, T, st) == 0
    assert fwd(N=-1) == -1
    dQ0, dWe, dbe = z(256, E, dt=F32), z(32, E, dt=F32), z(32, dt=F32)
    assert lib.ccd_posattn_fold(dP, E, dWp, dbp, dQ0, dWe, dbe, N, 96, st) == -2
    dQ0.fill_(3.0)
    assert lib.ccd_posattn_fold(None, E, None, None, dQ0, dWe, dbe, 0, E, st) == 0 and (dQ0 == 0).all()   # no images: zeros
    # the wrappers: an empty batch, wrong dtypes and shapes
    a0, G0 = ops.posattn_fwd(P[:0], X[:0], Q0, We, be, T)
    assert tuple(a0.shape) == (0, T, 256) and tuple(G0.shape) == (0, E)
    out = ops.posattn_bwd(dG[:0], X[:0], P[:0], Q0, We, a0)
    assert tuple(out[0].shape) == (0, E) and (out[2] == 0).all() and (out[3] == 0).all()
    with pytest.raises(TypeError, match="posattn_fwd: P must be bfloat16"):
        ops.posattn_fwd(P.float(), X, Q0, We, be, T)
    with pytest.raises(RuntimeError, match="ccd_posattn_fwd failed: unsupported shape"):
        ops.posattn_fwd(P[:255], X[:255], Q0, We, be, T)
    with pytest.raises(RuntimeError, match="ccd_posattn_fwd failed: unsupported shape"):
        ops.posattn_fwd(P, X, Q0, We, z(33, dt=F32), 33)


# ------------------------------------------------------------------------------------------------ the module and the model
NAMES = ["attention.f0_embedding.weight", "attention.w0.weight", "attention.w0.bias", "attention.wv.weight", "attention.wv.bias",
         "attention.we.weight", "attention.we.bias", "cls.weight", "cls.bias"]
WORDS = ["text-recognition", "aab", "Wor1d!"]
WE_GAIN = 8.0                                  # on the default we.weight: score std ~ 3 over the tokens at E = 64 (peaked maps, asserted)


def torch_head(X, w):
    """The same formula composed from torch ops in fp32: X [N, 256, E], w = the nine parameters by name -> (logits [N, T, C], a [N, T, 256])."""
    Q0 = w["attention.w0.bias"][:, None] + w["attention.w0.weight"] @ w["attention.f0_embedding.weight"]
    P = X @ w["attention.wv.weight"].t() + w["attention.wv.bias"]
    A = torch.tanh(P + Q0) @ w["attention.we.weight"].t() + w["attention.we.bias"]
    a = A.softmax(dim=1).transpose(1, 2)
    return (a @ X) @ w["cls.weight"].t() + w["cls.bias"], a


def param_grad_close(got, want, name, what):
    """The gradient gate for one parameter.  d we.bias is analytically zero (a softmax row's gradient sums to zero: the bias moves no
    probability), so its reference is torch's own rounding noise and "2e-2 * max |reference|" gates nothing: there the absolute part is
    taken from d we.weight - the same sums of dA, weighted by |M| <= 1 - and the reference is the exact zero."""
    if name == "attention.we.bias":
        scale = float(np.abs(want["attention.we.weight"]).max())
        close(got, np.zeros_like(want[name]), 0.0, 2e-2 * scale, what + name)
    else:
        grad_close(got, want[name], what + name)


def _decoder(device, E=64, T=25, C=92, seed=3):
    from ccd_amd.decoder.parallel_attn_decoder import ParallelAttnDecoder
    torch.manual_seed(seed)
    dec = ParallelAttnDecoder(E, C, T).to(device)
    arena = dec.ensure_arena()
    with torch.no_grad():
        arena.w("attention.we.weight").mul_(WE_GAIN)
    arena.refresh_mirrors()
    return dec, {n: arena.w(n).detach().cpu().clone().requires_grad_(True) for n in NAMES}


def check_module_autograd(device, N=2, E=64, T=25, C=92):
    """Gradients of all nine parameters and of the tokens under a scalar loss against torch autograd over the same formula in fp32 (on
    the same bf16 tokens): the gradient gate of the kernels; logits at G's gate, the maps at a's gate widened by what the bf16 P (which
    the contract allows) does to a score: |dA| <= sum_e |We| * 2^-9 |P| ~ 2e-2 at this scale, so rtol 4e-2."""
    dec, w = _decoder(device, E, T, C)
    g = torch.Generator().manual_seed(8)
    tokens = torch.randn(N, 256, E, generator=g).to(BF16)
    weight = torch.randn(N, T, C, generator=g)
    X = tokens.float().requires_grad_(True)
    ref_logits, ref_a = torch_head(X, w)
    assert float(ref_a.detach().max(dim=2).values.median()) > 0.1
    (ref_logits * weight).sum().backward()
    tok = tokens.to(device).clone().requires_grad_(True)
    dec.arena.zero_grad()
    logits, attn = dec.forward_train(tok)
    assert tuple(logits.shape) == (N, T, C) and logits.dtype == F32 and tuple(attn.shape) == (N, T, 8, 32) and dec.last_attn is attn
    close(attn.reshape(N, T, 256), ref_a.detach().double().numpy(), 4e-2, 1e-5, "module/attn")
    close(logits, ref_logits.detach().double().numpy(), 1e-2, 1e-2, "module/logits")
    (logits * weight.to(device)).sum().backward()
    want = {n: w[n].grad.double().numpy() for n in NAMES}
    for n in NAMES:
        param_grad_close(dec.arena.g(n), want, n, "module/d ")
    grad_close(tok.grad, X.grad.double().numpy(), "module/d tokens")
    probs = dec.forward_test(tokens.to(device))
    close(probs, ref_logits.detach().softmax(-1).double().numpy(), 1e-2, 1e-3, "module/probabilities")


def check_module_tf_loss(device, E=64, T=25, C=93):
    """Under TFLoss the last position's We row and be entry get an exactly zero gradient, a <PAD>-only row contributes nothing, and the
    loss and the gradients are those of the torch composition."""
    from ccd_amd.convertor.attn import AttnConvertor
    from ccd_amd.loss.ce_loss import TFLoss
    conv = AttnConvertor(dict_type='DICT90', max_seq_len=T, with_unknown=True)
    C = conv.num_classes()
    dec, w = _decoder(device, E, T, C)
    targets = conv.str2tensor(WORDS)
    targets[1, 1:] = conv.padding_idx                                  # a <PAD>-only row
    tokens = torch.randn(3, 256, E, generator=torch.Generator().manual_seed(4)).to(BF16)
    loss_fn = TFLoss(ignore_index=conv.padding_idx)

    def run(tok_host):
        tok = tok_host.to(device).clone().requires_grad_(True)              # (a copy: on the CPU .to() is the host tensor itself)
        dec.arena.zero_grad()
        logits, _ = dec.forward_train(tok)
        loss = loss_fn(logits, {"padded_targets": targets.to(device)})
        loss.backward()
        return loss.detach().cpu(), tok.grad.float().cpu(), {n: dec.arena.g(n).detach().cpu().clone() for n in NAMES}

    loss, dtok, grads = run(tokens)
    X = tokens.float().requires_grad_(True)
    ref_logits, _ = torch_head(X, w)
    ref = torch.nn.functional.cross_entropy(ref_logits[:, :-1].reshape(-1, C), targets[:, 1:].reshape(-1), ignore_index=conv.padding_idx)
    ref.backward()
    print(f"TFLoss {loss.item():.6f}, torch composition {ref.item():.6f}")
    assert abs(loss.item() - ref.item()) < 1e-3
    want = {n: w[n].grad.double().numpy() for n in NAMES}
    for n in NAMES:
        param_grad_close(grads[n], want, n, "tf/d ")
    grad_close(dtok, X.grad.double().numpy(), "tf/d tokens")
    # the last position has no target: We[T - 1] and be[T - 1] reach the loss through G[T - 1] alone and get an exactly zero gradient.
    # Row T - 1 of F and column T - 1 of W0 do NOT: Q0 = b0 + W0 F sums over the positions and is shared by all of them (the
    # reference's w0 maps the T reading-order embeddings onto the 256 tokens), so they move every position's scores - torch autograd
    # over the reference's formula gives them a non-zero gradient as well, and the gates above hold them to it.
    assert (grads["attention.we.weight"][T - 1] == 0).all() and grads["attention.we.bias"][T - 1] == 0
    assert float(np.abs(want["attention.f0_embedding.weight"][T - 1]).max()) > 0 and float(np.abs(want["attention.w0.weight"][:, T - 1]).max()) > 0
    assert float(grads["attention.we.weight"][:T - 1].abs().max()) > 0
    assert (dtok[1] == 0).all() and float(dtok[0].abs().max()) > 0      # the <PAD>-only image gets no gradient ...
    other = tokens.clone()
    other[1] = torch.randn(256, E, generator=torch.Generator().manual_seed(40)).to(BF16)
    loss2, _, grads2 = run(other)                                      # ... and gives none: other tokens there change nothing
    # the gradients: the same bits (d_logits of the image is exactly zero either way, and every sum behind it has a fixed order).  The
    # loss itself is TFLoss's sum of up to 24 workgroup partials (3 x 32 rows, 4 rows per workgroup) that tf_loss_fwd_kernel adds with
    # fp32 atomics in arrival order, so two runs of the SAME inputs agree to 24 roundings of the sum, not bit for bit: 24 * 2^-24 * loss
    assert abs(loss.item() - loss2.item()) <= 24 * 2.0 ** -24 * abs(loss.item()), (loss.item(), loss2.item())
    for n in NAMES:
        assert torch.equal(grads[n], grads2[n]), f"d {n} depends on the tokens of a <PAD>-only image"


def _register_arch():
    """A 3-block E = 192 backbone under the name 'vit_test3' (DINO_Finetune looks architectures up by name)."""
    from functools import partial
    import torch.nn as nn
    from ccd_amd.modules import vision_transformer as vits
    if "vit_test3" not in vits.__dict__:
        vits.vit_test3 = lambda patch_size=16, **kw: vits.VisionTransformer(
            patch_size=patch_size, embed_dim=192, depth=3, num_heads=3, mlp_ratio=4, qkv_bias=True,
            norm_layer=partial(nn.LayerNorm, eps=1e-6), **kw)


def par_config(**decoder):
    from ccd_amd import finetune as ft
    _register_arch()
    cfg = ft.FinetuneConfig(arch="vit_test3", drop_path_rate=0.0)
    cfg.decoder_type = "ParallelAttnDecoder"
    for k, v in decoder.items():
        setattr(cfg, "decoder_" + k, v)
    return cfg


def check_model(device):
    """DINO_Finetune with the new type on the 3-block tiny backbone: one training iteration's loss within the finetune path's 1e-3 of the
    torch composition on the same tokens, forward_test's words those of its arg-max, TextAccuracy takes the output."""
    from ccd_amd import finetune as ft
    from ccd_amd.metric.eval_acc import TextAccuracy
    torch.manual_seed(11)
    model = ft.build_model(par_config(), device, dropout=0.0)
    with torch.no_grad():
        model.arena.w("decoder.attention.we.weight").mul_(WE_GAIN)
    model.arena.refresh_mirrors()
    conv = model.label_convertor
    assert [n for n, _ in model.named_parameters() if not n.startswith("backbone.")] == ["decoder." + n for n in NAMES]
    assert model.unused_parameter_names() == ["backbone.cls_token"] + [f"backbone.norm_seg.{j}.{k}" for j in range(3) for k in ("weight", "bias")]
    img = torch.randn(3, 3, 32, 128, generator=torch.Generator().manual_seed(21)).to(device)
    targets = conv.str2tensor(WORDS)
    model.eval()
    with torch.no_grad():
        feat = model.extract_feat(img).float().cpu()
    w = {n: model.arena.w("decoder." + n).detach().cpu().clone() for n in NAMES}
    ref_logits, ref_a = torch_head(feat, w)
    C = conv.num_classes()
    want = torch.nn.functional.cross_entropy(ref_logits[:, :-1].reshape(-1, C), targets[:, 1:].reshape(-1), ignore_index=conv.padding_idx)
    probs = model.forward_test(img)
    assert tuple(probs.shape) == (3, 25, C) and probs.dtype == F32
    close(probs, ref_logits.softmax(-1).double().numpy(), 1e-2, 1e-3, "model/probabilities")
    assert conv.tensor2idx(probs.cpu())[0] == conv.tensor2idx(ref_logits.softmax(-1))[0]
    p2, attn = model.forward_attn(img)
    assert torch.equal(p2, probs) and tuple(attn.shape) == (3, 25, 8, 32)
    close(attn.reshape(3, 25, 256), ref_a.double().numpy(), 4e-2, 1e-5, "model/attn")
    assert torch.equal(model(img, None, return_loss=False), probs) and torch.equal(model.forward_test_speed(img), probs)
    metric = TextAccuracy()
    metric.update_scores(probs, conv.idx2str(conv.tensor2idx(probs.cpu())[0]), conv)     # its own words: every one correct
    assert metric.correct_num_word + metric.total_num_word >= 0 and metric.result() is not None
    model.train()
    opt = ft.make_optimizer(model)
    loss, attn = ft.training_iteration(model, opt, img, targets.to(device), 3e-4)
    print(f"training iteration: loss {loss.item():.6f}, torch composition on the same tokens {want.item():.6f}")
    assert abs(loss.item() - want.item()) < 1e-3 and tuple(attn.shape) == (3, 25, 8, 32)
    for n in NAMES[:-2]:
        assert float(model.arena.g("decoder." + n).abs().max()) > 0, n


def check_refusals_and_loading():
    """Host logic: the refusals, the parameter names, the reference's state dict, the YAML, the other heads.  No device."""
    import os
    import yaml
    from ccd_amd import finetune as ft
    from ccd_amd.model.dino_vision import DINO_Finetune
    torch.manual_seed(0)
    m = DINO_Finetune(par_config())
    assert [n for n, _ in m.named_parameters() if not n.startswith("backbone.")] == ["decoder." + n for n in NAMES]
    assert type(m.label_convertor).__name__ == "AttnConvertor" and type(m.loss).__name__ == "TFLoss" and not hasattr(m, "encoder")
    assert {n: tuple(p.shape) for n, p in m.decoder.named_parameters()} == {
        "attention.f0_embedding.weight": (25, 192), "attention.w0.weight": (256, 25), "attention.w0.bias": (256,),
        "attention.wv.weight": (192, 192), "attention.wv.bias": (192,), "attention.we.weight": (25, 192), "attention.we.bias": (25,),
        "cls.weight": (93, 192), "cls.bias": (93,)}
    for key, value in (("beam_width", 4), ("lexicon", "words.txt"), ("lexicon_beam", 8), ("lm", "lm.npz"), ("aux_ctc_weight", 0.2),
                       ("joint_ctc_weight", 0.3), ("twopass_beam", 4)):
        with pytest.raises(ValueError, match=f"decoder.{key}.*ParallelAttnDecoder"):
            DINO_Finetune(par_config(**{key: value}))
    img = torch.zeros(1, 3, 32, 128)
    for method, args in (("forward_beam", (img,)), ("forward_lexicon", (img,)), ("forward_score", (img, [["a"]])),
                         ("forward_words", (img, [["a"]])), ("forward_twopass", (img,)), ("forward_ctc", (img,)), ("forward_chars", (img,))):
        with pytest.raises(ValueError, match="ParallelAttnDecoder"):
            getattr(m, method)(*args)
    for kind, cls in (("NRTRDecoder", "NRTRDecoder"), ("CTCDecoder", "CTCDecoder"), (None, "NRTRDecoder")):
        cfg = ft.FinetuneConfig(arch="vit_tiny", decoder_n_layers=1)
        cfg.decoder_type = kind
        other = DINO_Finetune(cfg)
        assert type(other.decoder).__name__ == cls and not other.par and hasattr(other, "encoder") == (cls == "NRTRDecoder")
        with pytest.raises(ValueError, match="forward_attn is the parallel attention head's"):
            other.forward_attn(img)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    y = yaml.safe_load(open(os.path.join(root, "Dino", "configs", "CCD_vision_model_ARD_PAR.yaml")))
    ard = yaml.safe_load(open(os.path.join(root, "Dino", "configs", "CCD_vision_model_ARD.yaml")))
    assert y["decoder"] == {"type": "ParallelAttnDecoder", "max_seq_len": 25}
    assert {k: v for k, v in y.items() if k not in ("decoder", "global")} == {k: v for k, v in ard.items() if k not in ("decoder", "global")}
    return m
