"""LayerNorm statistics on ill-conditioned rows under the CPU SIMT executor (tests/hipsim): every site that computes them, at the
smallest shapes the suite uses for that site, and - with no kernel at all - the proof that the gates of ln_conditioning_checks.py
separate the one-pass formula from the two-pass one on these very rows."""
import pytest

from backends import Backend
import ln_conditioning_checks as lc


@pytest.fixture(scope="module")
def sim():
    with Backend("sim") as b:
        yield b


@pytest.fixture(autouse=True)
def one_cu(monkeypatch):
    """Kernel tests run on a 1-CU chip: persistent kernels then walk several work items per workgroup."""
    monkeypatch.setenv("CCD_SIM_CUS", "1")


@pytest.mark.parametrize("rows,E,start", [(37, 192, 0), (9, 384, 5), (33, 512, 0)])
def test_ln_fwd_conditioning_sim(sim, rows, E, start):
    lc.check_ln_fwd(sim.device, rows, E, start=start)


@pytest.mark.parametrize("M,N,K", [(300, 384, 128), (140, 192, 64)])
def test_gemm_resid_ln_row384_conditioning_sim(sim, M, N, K):
    lc.check_gemm_resid_ln(sim.device, M, N, K)                    # gemm_row384.h


@pytest.mark.parametrize("M,N,K,force", [(130, 512, 128, False), (200, 128, 256, True), (300, 384, 192, True)])
def test_gemm_resid_ln_rowgemm_conditioning_sim(sim, M, N, K, force):
    from ccd_amd import ops
    if force:
        with ops.policy(rowgemm=2):                                # rowgemm.h forced (the default only at N = 512)
            lc.check_gemm_resid_ln(sim.device, M, N, K)
    else:
        lc.check_gemm_resid_ln(sim.device, M, N, K)


@pytest.mark.parametrize("M,E,H,rps", [(300, 128, 256, 128), (200, 384, 128, 8), (130, 512, 128, 8)])
def test_mlp_fused_conditioning_sim(sim, M, E, H, rps):
    """rps = 128 with sample 1 dropped: its tile takes the dead_rows path; rps = 8: per-row scales in the live epilogue."""
    lc.check_mlp_fused(sim.device, M, E, H, rps)


@pytest.mark.parametrize("M,E,H,save", [(128 * 5 + 40, 128, 256, True), (300, 384, 128, False)])
def test_proj_mlp_fused_conditioning_sim(sim, M, E, H, save):
    lc.check_proj_mlp_fused(sim.device, M, E, H, 128, save)


def test_ln_bwd_conditioning_sim(sim):
    lc.check_ln_bwd(sim.device, 37, 192)


@pytest.mark.parametrize("g16", [False, True])
def test_gemm_lnbwd_conditioning_sim(sim, g16):
    lc.check_gemm_lnbwd(sim.device, 300, 384, 384, g16=g16)


# ---------------------------------------------------------------------------- no kernel: the gate separates the formulas
@pytest.mark.parametrize("E", [128, 192, 384, 512])
def test_gate_separates_one_pass_from_two_pass(E):
    """fp32 var = s2 / E - mean^2 must MISS the rstd gate on the offset rows from |c| = 30 on (condition number 1 + c^2 >= 901,
    times 2^-24: 5e-5) and on the small-variance rows at 0.2 (1 + 0.04 / 1e-6 = 4e4 on a variance that eps only halves); the fp32
    two-pass formula must pass every family.  Keeps the inputs honest if someone later softens them."""
    errs = lc.formula_errors(E)
    print(E, {f: {k: f"{v:.2g}" for k, v in e.items()} for f, e in errs.items()})
    for kind in lc.ONE_PASS_MUST_FAIL:
        assert errs["one_pass"][kind] > lc.RSTD_RTOL, f"one-pass passes on {kind}: {errs['one_pass'][kind]:.3g}"
    for kind in lc.KINDS:
        assert errs["two_pass"][kind] <= lc.RSTD_RTOL, f"two-pass fails on {kind}: {errs['two_pass'][kind]:.3g}"


@pytest.mark.parametrize("E", [384, 512])
def test_gate_catches_a_shift_by_the_first_element(E):
    """What the outlier rows are for.  The UNSHIFTED one-pass formula is well conditioned on them (|mean| / std = 1 / sqrt(E): it
    measures 5e-8 .. 1.3e-7 there, printed by the test above), so they add nothing against it.  They are there for the obvious
    cheap repair, the one-pass formula shifted by the row's first element: that one is well conditioned on every offset row (the
    shift removes c) - and on a row whose FIRST channel is the outlier its two sums are 1e6 each and cancel to 1e6 (E - 1) / E^2
    = 2600 (E = 384) or 1950 (E = 512): relative error 1e6 * 2^-24 / 2600 = 2.3e-5 and up.  (At E <= 192 what is left is 5000 and
    more and the error is at the gate, not over it: those widths are not asserted.)"""
    errs = lc.formula_errors(E)["one_pass_pivot_first"]
    for kind in ("a+30", "a-300", "a+3000"):
        assert errs[kind] <= lc.RSTD_RTOL, f"shifted one-pass fails on {kind}: {errs[kind]:.3g}"
    assert errs["b/first"] > lc.RSTD_RTOL, f"shifted one-pass passes on b/first: {errs['b/first']:.3g}"
