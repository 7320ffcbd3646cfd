"""LayerNorm statistics on ill-conditioned rows on a real MI355X (run with -m gpu): the shapes of test_ln_conditioning_sim.py, and one
more per fused entry point at which a workgroup walks several row tiles."""
import pytest
import torch

from backends import Backend
import ln_conditioning_checks as lc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    with Backend("hip") as b:
        yield b


@pytest.mark.parametrize("rows,E,start", [(37, 192, 0), (9, 384, 5), (33, 512, 0)])
def test_ln_fwd_conditioning(hip, rows, E, start):
    lc.check_ln_fwd(hip.device, rows, E, start=start)


@pytest.mark.parametrize("M,N,K", [(300, 384, 128), (140, 192, 64), (4096 + 72, 384, 384)])
def test_gemm_resid_ln_row384_conditioning(hip, M, N, K):
    lc.check_gemm_resid_ln(hip.device, M, N, K)                    # gemm_row384.h


@pytest.mark.parametrize("M,N,K,force", [(130, 512, 128, False), (200, 128, 256, True), (300, 384, 192, True), (4096 + 72, 384, 384, True)])
def test_gemm_resid_ln_rowgemm_conditioning(hip, M, N, K, force):
    from ccd_amd import ops
    if force:
        with ops.policy(rowgemm=2):                                # rowgemm.h forced (the default only at N = 512)
            lc.check_gemm_resid_ln(hip.device, M, N, K)
    else:
        lc.check_gemm_resid_ln(hip.device, M, N, K)


@pytest.mark.parametrize("M,E,H,rps", [(300, 128, 256, 128), (200, 384, 128, 8), (130, 512, 128, 8), (4096 + 72, 384, 1536, 256)])
def test_mlp_fused_conditioning(hip, M, E, H, rps):
    """rps a multiple of 128 with sample 1 dropped: its tiles take the dead_rows path; rps = 8: per-row scales in the live epilogue."""
    lc.check_mlp_fused(hip.device, M, E, H, rps)


@pytest.mark.parametrize("M,E,H,rps,save", [(128 * 5 + 40, 128, 256, 128, True), (300, 384, 128, 128, False),
                                            (4096 + 72, 384, 1536, 256, True)])
def test_proj_mlp_fused_conditioning(hip, M, E, H, rps, save):
    lc.check_proj_mlp_fused(hip.device, M, E, H, rps, save)


def test_ln_bwd_conditioning(hip):
    lc.check_ln_bwd(hip.device, 37, 192)


@pytest.mark.parametrize("g16", [False, True])
def test_gemm_lnbwd_conditioning(hip, g16):
    lc.check_gemm_lnbwd(hip.device, 300, 384, 384, g16=g16)
