"""The Sinkhorn-Knopp teacher assignment on a real MI355X, through libccd_hip.so (run with -m gpu): what tests/test_sinkhorn_sim.py
checks under the executor, at the same gates (sinkhorn_checks), plus a [96, 65536] case, a run that may not synchronise with the
host, and the training step replayed as a HIP graph with the key on."""
import pytest
import torch

from backends import Backend
import sinkhorn_checks as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    with Backend("hip") as b:
        yield b


def test_fixtures(hip, golden_dir):
    sc.check_fixtures(hip.device, golden_dir)


@pytest.mark.parametrize("n", [1, 3])
def test_column_tails(hip, n):
    for K in (1, 255, 256, 257, 1023, 1024, 1025, 4100):
        sc.check_shape(hip.device, rows=5, K=K, temp=0.04 if K % 2 else 0.07, n=n)


@pytest.mark.parametrize("n", [1, 3])
def test_row_tails(hip, n):
    for rows in (1, 2, 63, 64, 65, 127, 128, 129):
        sc.check_shape(hip.device, rows=rows, K=36, temp=0.04, n=n)
        sc.check_shape(hip.device, rows=rows, K=37, temp=0.07, n=n)


@pytest.mark.parametrize("n", [1, 3])
def test_device_row_count_and_misaligned_base(hip, n):
    sc.check_shape(hip.device, rows=34, K=260, n=n, dead_rows=36, rows_mul=2)
    sc.check_shape(hip.device, rows=130, K=50, n=n, dead_rows=126, rows_mul=2, temp=0.07)
    sc.check_shape(hip.device, rows=128, K=8, n=n, dead_rows=128, rows_mul=1)
    sc.check_shape(hip.device, rows=9, K=256, n=n, base_offset=1)
    sc.check_shape(hip.device, rows=130, K=1028, n=n, base_offset=3, temp=0.07)


def test_full_width(hip):
    sc.check_shape(hip.device, rows=96, K=65536, temp=0.04, n=3)


def test_large_logits(hip):
    sc.check_large_logits(hip.device)


def test_repeatable(hip):
    sc.check_repeatable(hip.device)
    sc.check_repeatable(hip.device, rows=700, K=8192)


def test_abi_contract(hip):
    sc.check_abi_contract(hip.device)


def test_no_host_sync(hip):
    from ccd_amd import ops
    from ccd_amd.loss.Dino_loss import DINOLoss
    import sinkhorn_np as R
    t_np = R.cosine_logits(140, 2048, 3)
    t = torch.from_numpy(t_np).to(hip.device)
    d_rows = torch.tensor([70], dtype=torch.int32, device=hip.device)
    loss = DINOLoss(2048, 2, 0.04, 0.04, 0, 40).to(hip.device)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")            # torch raises on a synchronising call
    try:
        c = ops.sinkhorn_potentials(t, d_rows, 0.04, 3, rows_mul=2)
        q = loss.sinkhorn_knopp_teacher(t, 0.04)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    sc.assert_within_gate(q.cpu().numpy(), c.cpu().numpy(), t_np, 0.04, 3, R.format_rtol(t_np, 0.04), "[140, 2048] without a host sync")


def test_loss_matches_numpy(hip):
    sc.check_loss_matches_numpy(hip.device, batch=8)


def test_fused_matches_unfused(hip):
    sc.check_fused_matches_unfused(hip.device)


def test_default_is_unchanged(hip):
    sc.check_default_is_unchanged(hip.device)


def test_graphed_step(hip):
    sc.check_graphed_step(hip.device)
