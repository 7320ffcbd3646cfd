"""The Sinkhorn-Knopp kernels (ccd_amd/csrc/kernels/sinkhorn.h) under the CPU SIMT executor (tests/hipsim): the reference's recorded
cases, the tails of a strip of columns and of a chunk of rows, device-side row counts with NaN behind them, misaligned matrices,
logits at which fp32 exp overflows, bit repeatability, the ABI's error codes, and DINOLoss with the key on.  Gates: sinkhorn_checks."""
import pytest

from backends import Backend
import sinkhorn_checks as sc


@pytest.fixture(scope="module")
def sim():
    with Backend("sim") as b:
        yield b


def test_fixtures_sim(sim, golden_dir):
    sc.check_fixtures(sim.device, golden_dir)


def test_strip_and_chunk_constants_sim(sim):
    from ccd_amd import ops
    assert (ops.SINKHORN_STRIP, ops.SINKHORN_ROW_CHUNK) == (1024, 128)         # what the tails below are placed around


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("K", [1, 255, 256, 257, 1023, 1024, 1025, 4100])
def test_column_tails_sim(sim, K, n):
    sc.check_shape(sim.device, rows=5, K=K, temp=0.04 if K % 2 else 0.07, n=n)


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("rows", [1, 2, 63, 64, 65, 127, 128, 129])
def test_row_tails_sim(sim, rows, n):
    sc.check_shape(sim.device, rows=rows, K=36, temp=0.04, n=n)           # 16-byte loads
    sc.check_shape(sim.device, rows=rows, K=37, temp=0.07, n=n)           # one element at a time


@pytest.mark.parametrize("n", [1, 3])
def test_device_row_count_sim(sim, n):
    sc.check_shape(sim.device, rows=34, K=260, n=n, dead_rows=36, rows_mul=2)
    sc.check_shape(sim.device, rows=130, K=50, n=n, dead_rows=126, rows_mul=2, temp=0.07)      # the second chunk is partly live
    sc.check_shape(sim.device, rows=128, K=8, n=n, dead_rows=128, rows_mul=1)                  # ... and not at all


@pytest.mark.parametrize("n", [1, 3])
def test_misaligned_base_sim(sim, n):
    sc.check_shape(sim.device, rows=9, K=256, n=n, base_offset=1)
    sc.check_shape(sim.device, rows=130, K=1028, n=n, base_offset=3, temp=0.07)


def test_large_logits_sim(sim):
    sc.check_large_logits(sim.device)


def test_repeatable_sim(sim):
    sc.check_repeatable(sim.device)


def test_abi_contract_sim(sim):
    sc.check_abi_contract(sim.device)


def test_loss_matches_numpy_sim(sim):
    sc.check_loss_matches_numpy(sim.device)


def test_fused_matches_unfused_sim(sim):
    sc.check_fused_matches_unfused(sim.device)


def test_default_is_unchanged_sim(sim):
    sc.check_default_is_unchanged(sim.device)
