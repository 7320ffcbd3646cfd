"""Dino.utils.DBSCAN kernels under the CPU SIMT executor (tests/hipsim): the product's kernel sources + C ABI compiled for the
host, against the reference's recorded outputs and the numpy restatement."""
import numpy as np
import pytest
import torch

from backends import Backend
import cluster_checks as cc
import cluster_np


@pytest.fixture(scope="module")
def sim():
    with Backend("sim") as b:
        yield b


def test_cluster_fixtures_sim(sim, golden_dir):
    cc.check_fixtures(sim.device, golden_dir)


def test_cluster_random_sim(sim):
    cc.check_random(sim.device, cluster_np.random_masks(6, seed=17))


def test_cluster_ops_sim(sim):
    cc.check_ops_layers(sim.device, cluster_np.random_masks(4, seed=23))


def test_cluster_public_classes_sim(sim, golden_dir):
    from ccd_amd.utils.DBSCAN import DBSCAN_cluster, label_cluster, region_cluster
    names, masks, want, ties = cluster_np.load_cases(golden_dir)
    i = names.index("text_like_0")
    for k, cls in (("dbscan", DBSCAN_cluster), ("label", label_cluster), ("region", region_cluster)):
        # numpy [H, W] in -> numpy uint8 [26, H, W] out (the reference contract)
        got = cls()(masks[i])
        assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == (26, 32, 128)
        np.testing.assert_array_equal(got, want[k][i])
        # torch [H, W] in -> torch uint8 [26, H, W]; integer, bool and float64 masks
        np.testing.assert_array_equal(cls()(torch.from_numpy(masks[i])).numpy(), want[k][i])
        np.testing.assert_array_equal(cls()(masks[i].astype(bool)), want[k][i])
        np.testing.assert_array_equal(cls()(torch.from_numpy(masks[i].astype(np.int64))).numpy(), want[k][i])
        np.testing.assert_array_equal(cls()(masks[i].astype(np.float64)), want[k][i])
        # an empty batch is a no-op
        assert tuple(cls()(torch.zeros(0, 32, 128)).shape) == (0, 26, 32, 128)
    # a tiny float64 value is nonzero for label / region (tested in its own dtype, not after rounding to fp32)
    m = np.zeros((32, 128)); m[4:20, 10:30] = 1e-60
    assert label_cluster()(m).any() and region_cluster()(m).any() and not DBSCAN_cluster()(m).any()
    with pytest.raises(ValueError, match="32, 128"):
        region_cluster()(torch.zeros(2, 32, 64))


def test_idmap_to_planes_u8_alignment_is_asserted(sim):
    from ccd_amd import ops
    buf = torch.full((2 * 32 * 128 + 16,), 255, dtype=torch.uint8)
    with pytest.raises(AssertionError, match="16-byte"):
        ops.idmap_to_planes_u8(buf[1:1 + 32 * 128].view(1, 32, 128))
    assert not ops.idmap_to_planes_u8(buf[16:16 + 32 * 128].view(1, 32, 128)).any()
