"""LayerNorm statistics on ill-conditioned rows, at every site that computes them: the stand-alone kernel (layernorm.h) and the four
fused epilogues (mlp_fused.h live rows and dead_rows, rowgemm.h, gemm_row384.h).  Used by test_ln_conditioning_sim.py (CPU SIMT
executor) and test_ln_conditioning_gpu.py (-m gpu).

The rows mix five families inside one call, so neighbouring rows of one wave / tile have different statistics:
  (a) randn + c, c in {0, +-30, +-300, +-3000}         cancellation in  s2 / E - mean^2
  (b) randn with one channel set to 1000 (channel 0, E/2, E-1)    a one-pass formula shifted by the row's first element
  (c) every channel 7.25                               var == 0 exactly
  (d) randn * 1e-3 and randn * 1e-3 + 0.2              eps placement: rstd ~ 707 with eps inside the root, ~1000 without it, ~302 with 1e-5
  (e) randn * 3 + 0.5                                  the baseline
For the fused sites the rows are the `resid` operand and the product branch is present but small (rms <= 1e-4); the reference is
the fp64 LayerNorm of the kernel's OWN fp32 output rows, so the products' rounding plays no part (kernel_checks.py covers them).

Gates (ISSUE: derived, not fitted): a two-pass fp32 sum over E <= 512 terms has relative error of a few 2^-24 log2(E) ~ 5e-7; the
rstd gate 1e-5 leaves 20x on that and is 5x - 35x below the one-pass error at |mean| / std = 30 (condition number 1 + 30^2 = 901
times 2^-24 = 5e-5).  one_pass_f32 / two_pass_f32 below are the two formulas in plain torch: the tests show that the gate
separates them on these very rows."""
import torch

from ccd_amd import ops

BF = torch.bfloat16
EPS = 1e-6
RSTD_RTOL = 1e-5
MEAN_RTOL, MEAN_ATOL = 1e-5, 1e-6
Y_RTOL, Y_ATOL = 1e-2, 1e-2

# row i of a call is of kind KINDS[(i + start) % 14]: every family within any 14 consecutive rows
KINDS = ["a+0", "a+30", "b/first", "a-30", "c", "a+300", "d+0", "a-300", "b/mid", "d+0.2", "a+3000", "e", "a-3000", "b/last"]
ONE_PASS_MUST_FAIL = ("a+30", "a-30", "a+300", "a-300", "a+3000", "a-3000", "d+0.2")
BACKWARD_KINDS = [k for k in KINDS if k[0] in "ab"]


def make_rows(M, E, seed, start=0, kinds=KINDS):
    """-> (x fp32 [M, E], the kind of every row)."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn((M, E), generator=g)
    x = torch.empty((M, E))
    labels = []
    for i in range(M):
        k = kinds[(i + start) % len(kinds)]
        labels.append(k)
        if k[0] == "a":
            x[i] = z[i] + float(k[1:])
        elif k[0] == "b":
            x[i] = z[i]
            x[i, {"first": 0, "mid": E // 2, "last": E - 1}[k[2:]]] = 1000.0
        elif k == "c":
            x[i] = 7.25
        elif k[0] == "d":
            x[i] = z[i] * 1e-3 + float(k[1:])
        else:
            x[i] = z[i] * 3 + 0.5
    return x, labels


def ref_stats(rows):
    """fp64 statistics of fp32 rows -> (mean, rstd), eps inside the root."""
    r = rows.detach().cpu().double()
    mean = r.mean(1)
    var = (r - mean[:, None]).pow(2).mean(1)
    return mean, (var + EPS).rsqrt()


def ref_ln(rows, gamma, beta):
    r = rows.detach().cpu().double()
    mean, rstd = ref_stats(rows)
    return (r - mean[:, None]) * rstd[:, None] * gamma.double() + beta.double()


def one_pass_f32(x, pivot_first=False):
    """var = s2 / E - mean^2 from fp32 sums, clamped at 0 (what the fused sites computed); pivot_first: both sums taken of
    x - x[:, 0] (the textbook shifted one-pass formula with the first element as the shift)."""
    x = x.float()
    E = x.shape[1]
    sh = x[:, :1] if pivot_first else torch.zeros_like(x[:, :1])
    d = x - sh
    m = d.sum(1) / E
    var = ((d * d).sum(1) / E - m * m).clamp_min(0)
    return m + sh[:, 0], 1.0 / torch.sqrt(var + EPS)


def two_pass_f32(x):
    x = x.float()
    E = x.shape[1]
    m = x.sum(1) / E
    d = x - m[:, None]
    return m, 1.0 / torch.sqrt((d * d).sum(1) / E + EPS)


def rstd_errors(rstd, rows, labels):
    """-> {kind: max relative error of rstd against the fp64 statistics of `rows`}."""
    want = ref_stats(rows)[1]
    rel = ((rstd.detach().cpu().double() - want).abs() / want)
    rel = torch.where(torch.isfinite(rel), rel, torch.full_like(rel, float("inf")))
    out = {}
    for i, k in enumerate(labels):
        out[k] = max(out.get(k, 0.0), float(rel[i]))
    return out


def mean_errors(mean, rows, labels):
    """-> {kind: max of |mean - fp64 mean| / (atol + rtol |fp64 mean|)}: <= 1 passes."""
    want = ref_stats(rows)[0]
    q = (mean.detach().cpu().double() - want).abs() / (MEAN_ATOL + MEAN_RTOL * want.abs())
    q = torch.where(torch.isfinite(q), q, torch.full_like(q, float("inf")))
    out = {}
    for i, k in enumerate(labels):
        out[k] = max(out.get(k, 0.0), float(q[i]))
    return out


def check_stats(mean, rstd, rows, labels, what):
    """The mean and rstd gates against the fp64 statistics of the kernel's own rows; failures are listed per family."""
    assert tuple(mean.shape) == (rows.shape[0],) and tuple(rstd.shape) == (rows.shape[0],), what
    me, re = mean_errors(mean, rows, labels), rstd_errors(rstd, rows, labels)
    print(f"{what}: max rstd rel err {max(re.values()):.3g}, max mean err / tol {max(me.values()):.3g}")
    bad_r = {k: f"{v:.3g}" for k, v in re.items() if not v <= RSTD_RTOL}
    bad_m = {k: f"{v:.3g}" for k, v in me.items() if not v <= 1.0}
    assert not bad_r and not bad_m, f"{what}: rstd relative error over {RSTD_RTOL:g} in {bad_r}; mean error / tolerance over 1 in {bad_m}"


def check_y(y, rows, gamma, beta, what):
    want = ref_ln(rows, gamma, beta)
    got = y.detach().float().cpu().double()
    assert got.shape == want.shape, what
    err = (got - want).abs()
    bad = ~(err <= Y_ATOL + Y_RTOL * want.abs())
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.numel()} off, max err {float(err.max()):.4g} in rows {sorted(set(bad.nonzero()[:, 0].tolist()))[:8]}"


def same_bits(a, b, what):
    assert torch.equal(a.cpu().view(torch.int32), b.cpu().view(torch.int32)), f"{what}: two calls on the same operands differ"


def _affine(E, g):
    return torch.randn(E, generator=g).abs() + 0.5, torch.randn(E, generator=g) * 0.3


def _dropped_has(labels, scale_rows, kinds):
    dropped = {labels[i] for i in range(len(labels)) if scale_rows[i] == 0}
    assert set(kinds) <= dropped, f"the dropped samples must hold rows of {kinds}, have {sorted(dropped)}"


def _small(branch, what):
    rms = float(branch.double().pow(2).mean().sqrt())
    assert 0 < rms <= 1e-4, f"{what}: the product branch must be present but small, rms {rms:.3g}"


# ------------------------------------------------------------------------------------------------ forward sites
def check_ln_fwd(dev, rows, E, seed=70, start=0):
    g = torch.Generator().manual_seed(seed)
    x, labels = make_rows(rows, E, seed + 1, start)
    gamma, beta = _affine(E, g)
    y, mean, rstd = ops.ln_fwd(x.to(dev), gamma.to(dev), beta.to(dev), EPS)
    tag = f"ln_fwd {rows}x{E}"
    check_stats(mean, rstd, x, labels, tag)
    check_y(y, x, gamma, beta, tag + "/y")
    _, mean_b, rstd_b = ops.ln_fwd(x.to(dev), gamma.to(dev), beta.to(dev), EPS)
    same_bits(mean, mean_b, tag + "/mean")
    same_bits(rstd, rstd_b, tag + "/rstd")


def check_gemm_resid_ln(dev, M, N, K, seed=71, rps=16):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn((M, K), generator=g).to(BF)
    b = (torch.randn((N, K), generator=g) * (4e-5 / K ** 0.5)).to(BF)
    bias = torch.randn(N, generator=g) * 2e-5
    resid, labels = make_rows(M, N, seed + 1)
    rowscale = (torch.rand((M + rps - 1) // rps, generator=g) > 0.3).float() * 1.25
    rowscale[0] = 0.0                              # rows 0 .. rps-1: every family through a dropped sample
    rowscale[-1] = 1.25                            # the ragged last tile is live
    sc = rowscale.repeat_interleave(rps)[:M]
    _dropped_has(labels, sc, KINDS)
    _small((a.float() @ b.float().t() + bias) * 1.25, "gemm_resid_ln")
    gamma, beta = _affine(N, g)
    call = lambda: ops.gemm_nt_resid_ln(a.to(dev), b.to(dev), bias=bias.to(dev), resid=resid.to(dev), rowscale=rowscale.to(dev),
                                        rows_per_sample=rps, gamma=gamma.to(dev), beta=beta.to(dev), eps=EPS)
    out, y, mean, rstd = call()
    tag = f"gemm_resid_ln {M}x{N}x{K}"
    out = out.cpu()
    assert torch.equal(out[sc == 0], resid[sc == 0]), tag + ": dropped sample: the stream must pass through unchanged"
    assert float((out - resid).abs().max()) <= 1e-3, tag + "/out"
    check_stats(mean, rstd, out, labels, tag)
    check_y(y, out, gamma, beta, tag + "/y")
    _, _, mean_b, rstd_b = call()
    same_bits(mean, mean_b, tag + "/mean")
    same_bits(rstd, rstd_b, tag + "/rstd")


def _mlp_weights(E, H, g):
    w1 = (torch.randn((H, E), generator=g) * 0.08).to(BF)
    w2 = (torch.randn((E, H), generator=g) * (2e-5 / H ** 0.5)).to(BF)
    return w1, torch.randn(H, generator=g) * 0.5, w2, torch.randn(E, generator=g) * 2e-5


def _mlp_branch(y, w1, b1, w2, b2):
    u = (y.float() @ w1.float().t() + b1).to(BF)
    return torch.nn.functional.gelu(u.float()).to(BF).float() @ w2.float().t() + b2


def check_mlp_fused(dev, M, E, H, rps, seed=72):
    """rps a multiple of 128: sample 1 is dropped as a whole (whole tiles: the dead_rows path); else per-row scales with samples 0
    and 1 dropped."""
    g = torch.Generator().manual_seed(seed)
    y = torch.randn((M, E), generator=g).to(BF)
    w1, b1, w2, b2 = _mlp_weights(E, H, g)
    resid, labels = make_rows(M, E, seed + 1)
    rowscale = (torch.rand((M + rps - 1) // rps, generator=g) > 0.3).float() * 1.25
    rowscale[-1] = 1.25
    if rps % 128 == 0:
        rowscale[0], rowscale[1] = 1.25, 0.0
    else:
        rowscale[0] = rowscale[1] = 0.0
    sc = rowscale.repeat_interleave(rps)[:M]
    _dropped_has(labels, sc, KINDS)
    _small(_mlp_branch(y, w1, b1, w2, b2) * 1.25, "mlp_fused")
    gamma, beta = _affine(E, g)
    call = lambda: ops.mlp_fused(y.to(dev), w1.to(dev), b1.to(dev), w2.to(dev), b2.to(dev), resid=resid.to(dev), rowscale=rowscale.to(dev),
                                 rows_per_sample=rps, gamma=gamma.to(dev), beta=beta.to(dev), eps=EPS, store_u=True)
    out, yn, mean, rstd, _ = call()
    tag = f"mlp_fused {M}x{E}x{H} rps={rps}"
    out = out.cpu()
    assert torch.equal(out[sc == 0], resid[sc == 0]), tag + ": dropped sample: the stream must pass through unchanged"
    assert float((out - resid).abs().max()) <= 1e-3, tag + "/out"
    check_stats(mean, rstd, out, labels, tag)
    check_y(yn, out, gamma, beta, tag + "/y")
    _, _, mean_b, rstd_b, _ = call()
    same_bits(mean, mean_b, tag + "/mean")
    same_bits(rstd, rstd_b, tag + "/rstd")


def check_proj_mlp_fused(dev, M, E, H, rps, save, seed=73):
    """save: every combination of dropped branches (samples 0 .. 4), x_mid / y2 / mean2 / rstd2 checked against the kernel's own
    x_mid, and the tap output; without the saved tensors only the projection branch may be dropped."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn((M, E), generator=g).to(BF)
    wp = (torch.randn((E, E), generator=g) * (4e-5 / E ** 0.5)).to(BF)
    bp = torch.randn(E, generator=g) * 2e-5
    w1, b1, w2, b2 = _mlp_weights(E, H, g)
    w2 = (w2.float() * 0.25).to(BF)                # (y2 of an outlier row reaches ~20: a hidden row of larger rms)
    resid, labels = make_rows(M, E, seed + 1)
    ns = (M + rps - 1) // rps
    rs1, rs2 = torch.full((ns,), 1.25), torch.full((ns,), 1.25)
    for i, (s1, s2) in enumerate([(1.25, 1.25), (0.0, 1.25), (1.25, 0.0), (0.0, 0.0), (1.25, 1.25)][:ns]):
        rs1[i], rs2[i] = s1, (s2 if save else 1.25)
    ga2, be2 = _affine(E, g)
    ga, be = _affine(E, g)
    gat, bet = _affine(E, g)
    sc1, sc2 = rs1.repeat_interleave(rps)[:M], rs2.repeat_interleave(rps)[:M]
    _dropped_has(labels, sc1, KINDS)
    _small((a.float() @ wp.float().t() + bp) * 1.25, "proj_mlp_fused/proj")
    call = lambda: ops.proj_mlp_fused(a.to(dev), wp.to(dev), bp.to(dev), resid=resid.to(dev), rowscale1=rs1.to(dev), gamma2=ga2.to(dev),
                                      beta2=be2.to(dev), w1=w1.to(dev), b1=b1.to(dev), w2=w2.to(dev), b2=b2.to(dev),
                                      rowscale2=rs2.to(dev) if save else None, rows_per_sample=rps, gamma=ga.to(dev), beta=be.to(dev),
                                      eps=EPS, save=save, tap_gamma=gat.to(dev), tap_beta=bet.to(dev))
    out, yn, mean, rstd, saved, tap = call()
    tag = f"proj_mlp_fused {M}x{E}x{H} save={save}"
    out = out.cpu()
    if save:
        xmid, y2, mean2, rstd2, _ = saved
        xmid = xmid.cpu()
        _dropped_has(labels, sc2, KINDS)
        assert torch.equal(xmid[sc1 == 0], resid[sc1 == 0]), tag + ": dropped projection branch: x_mid must equal the stream"
        assert torch.equal(out[sc2 == 0], xmid[sc2 == 0]), tag + ": dropped MLP branch: x_out must equal x_mid"
        both = (sc1 == 0) & (sc2 == 0)
        assert both.any() and torch.equal(out[both], resid[both]), tag + ": both branches dropped: the stream must pass through unchanged"
        assert float((xmid - resid).abs().max()) <= 1e-3, tag + "/x_mid"
        check_stats(mean2, rstd2, xmid, labels, tag + "/2")
        check_y(y2, xmid, ga2, be2, tag + "/y2")
        _small(_mlp_branch(y2.cpu(), w1, b1, w2, b2) * 1.25, "proj_mlp_fused/mlp")      # (of the y2 just checked)
    else:
        assert saved is None
    check_stats(mean, rstd, out, labels, tag)
    check_y(yn, out, ga, be, tag + "/y")
    check_y(tap, out, gat, bet, tag + "/tap")
    # (the second product accumulates ON x_mid / sc2: a row at 3000 moves by its own rounding, a few ulp = 1e-3)
    assert float((out - resid).abs().max()) <= 4e-3, tag + "/out"
    res_b = call()
    same_bits(mean, res_b[2], tag + "/mean")
    same_bits(rstd, res_b[3], tag + "/rstd")
    if save:
        same_bits(saved[2], res_b[4][2], tag + "/mean2")
        same_bits(saved[3], res_b[4][3], tag + "/rstd2")


# ------------------------------------------------------------------------------------------------ backward sites
def _rounded_stats(x):
    mean, rstd = ref_stats(x)
    return mean.float(), rstd.float()


def check_ln_bwd(dev, rows=37, E=192, seed=74):
    """ops.ln_bwd on rows of families (a) and (b), statistics handed in (fp64, rounded to fp32), against fp64 autograd; the
    tolerances are check_layernorm's."""
    from kernel_checks import close
    g = torch.Generator().manual_seed(seed)
    x, _ = make_rows(rows, E, seed + 1, kinds=BACKWARD_KINDS)
    gamma = 1 + 0.1 * torch.randn(E, generator=g)
    mean, rstd = _rounded_stats(x)
    dy = torch.randn((rows, E), generator=g).to(BF)
    xr = x.double().requires_grad_(True); gr = gamma.double().requires_grad_(True); br = torch.zeros(E, dtype=torch.float64, requires_grad=True)
    torch.nn.functional.layer_norm(xr, (E,), gr, br, EPS).backward(dy.double())
    g0 = torch.randn((rows, E), generator=g)
    for acc in (True, False):
        gbuf = g0.clone().to(dev)
        dgam = torch.zeros(E).to(dev); dbet = torch.zeros(E).to(dev)
        ops.ln_bwd(dy.to(dev), x.to(dev), mean.to(dev), rstd.to(dev), gamma.to(dev), gbuf, dgam, dbet, accumulate=acc)
        close(gbuf, xr.grad + (g0 if acc else 0), 1e-3, 1e-4, f"ln_bwd/dx acc={acc}")
        close(dgam, gr.grad, 1e-3, 1e-3, "ln_bwd/dgamma")
        close(dbet, br.grad, 1e-3, 1e-3, "ln_bwd/dbeta")


def check_gemm_lnbwd(dev, M=300, N=384, K=384, seed=75, g16=False):
    """ops.gemm_nt_lnbwd (fp32 or bf16 gradient stream) on rows of families (a) and (b), statistics handed in, against fp64
    autograd; the tolerances are kernel_checks.check_gemm_lnbwd's."""
    from kernel_checks import close
    g = torch.Generator().manual_seed(seed)
    a = torch.randn((M, K), generator=g).to(BF); b = (torch.randn((N, K), generator=g) * 0.2).to(BF)
    x, _ = make_rows(M, N, seed + 1, kinds=BACKWARD_KINDS)
    gamma = 1 + 0.1 * torch.randn(N, generator=g)
    mean, rstd = _rounded_stats(x)
    g0 = torch.randn((M, N), generator=g)
    if g16:
        g0 = g0.to(BF).float()
    dy = a.double() @ b.double().t()
    xr = x.double().requires_grad_(True); gr = gamma.double().requires_grad_(True); br = torch.zeros(N, dtype=torch.float64, requires_grad=True)
    torch.nn.functional.layer_norm(xr, (N,), gr, br, EPS).backward(dy)
    scale_dy = float(dy.pow(2).mean().sqrt())
    for acc in (True, False):
        gbuf = (g0.to(BF) if g16 else g0.clone()).to(dev)
        dgam = torch.full((N,), 0.5).to(dev); dbet = torch.full((N,), -0.25).to(dev)
        ops.gemm_nt_lnbwd(a.to(dev), b.to(dev), x.to(dev), mean.to(dev), rstd.to(dev), gamma.to(dev), gbuf, dgam, dbet, accumulate=acc)
        tag = f"lnbwd g16={g16} acc={acc}"
        close(gbuf, xr.grad + (g0 if acc else 0), 1e-2 if g16 else 2e-3, 2e-3 * scale_dy, tag + "/g")
        close(dgam, gr.grad + 0.5, 2e-3, 2e-3 * scale_dy * M ** 0.5, tag + "/dgamma")
        close(dbet, br.grad - 0.25, 2e-3, 2e-3 * scale_dy * M ** 0.5, tag + "/dbeta")


# ------------------------------------------------------------------------------------------------ no kernel: the gate on these rows
def formula_errors(E, seed=76, rows=140):
    """-> {formula: {kind: max relative error of rstd}} of the fp32 formulas on 10 rows of every kind."""
    x, labels = make_rows(rows, E, seed)
    return {"one_pass": rstd_errors(one_pass_f32(x)[1], x, labels),
            "one_pass_pivot_first": rstd_errors(one_pass_f32(x, pivot_first=True)[1], x, labels),
            "two_pass": rstd_errors(two_pass_f32(x)[1], x, labels)}
