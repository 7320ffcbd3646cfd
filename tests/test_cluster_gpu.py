"""Dino.utils.DBSCAN on a real MI355X, through libccd_hip.so (run with -m gpu): the reference's recorded outputs, the numpy
restatement on random and text-like masks, batched == per-image, the numpy contract and label_cluster == the pretraining path."""
import numpy as np
import pytest
import torch

from backends import Backend
import cluster_checks as cc
import cluster_np
from ccd_amd.synthetic import make_text_like_batch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    with Backend("hip") as b:
        yield b


def _masks_256():
    _, text, _ = make_text_like_batch(64, seed=5)
    return np.concatenate([cluster_np.random_masks(192, seed=29), text.numpy().astype(np.float32)])


def test_cluster_fixtures(hip, golden_dir):
    cc.check_fixtures(hip.device, golden_dir)


def test_cluster_random_and_text_like(hip):
    cc.check_random(hip.device, _masks_256())


def test_cluster_ops_layers(hip):
    cc.check_ops_layers(hip.device, _masks_256()[::8].copy())


def test_cluster_batched_equals_per_image(hip):
    masks = _masks_256()
    assert masks.shape == (256, 32, 128)
    batched = cc.batched_planes(hip.device, masks)
    t = torch.from_numpy(masks).to(hip.device)
    for k, cls in cc.CLASSES.items():
        f = cls()
        per_image = torch.stack([f(t[i]) for i in range(t.shape[0])]).cpu().numpy()
        np.testing.assert_array_equal(per_image, batched[k], err_msg=k)


def test_cluster_numpy_contract(hip, golden_dir):
    from ccd_amd.utils.DBSCAN import DBSCAN_cluster, label_cluster, region_cluster
    names, masks, want, ties = cluster_np.load_cases(golden_dir)
    for k, cls in (("dbscan", DBSCAN_cluster), ("label", label_cluster), ("region", region_cluster)):
        for name in ("text_like_1", "border_two_clusters", "specks_use_slots", "threshold_edges"):
            i = names.index(name)
            got = cls()(masks[i])
            assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == (26, 32, 128)
            np.testing.assert_array_equal(got, want[k][i], err_msg=f"{k}/{name}")
            np.testing.assert_array_equal(cls()(masks[i].astype(np.float64)), want[k][i], err_msg=f"{k}/{name}/f64")
            np.testing.assert_array_equal(cls()(torch.from_numpy(masks[i] != 0).cuda()).cpu().numpy(),
                                          cluster_np.CLUSTERERS[k](masks[i] != 0), err_msg=f"{k}/{name}/bool")


def test_label_cluster_is_the_pretraining_path(hip, golden_dir):
    from ccd_amd import ops
    from Dino.model.dino_vision import label
    _, masks, _ = make_text_like_batch(32, seed=8, device=hip.device)
    masks = masks.float().contiguous()
    want = ops.idmap_to_planes(ops.ccl_label(masks)).to(torch.uint8)
    torch.testing.assert_close(label(masks), want, rtol=0, atol=0)


def test_cluster_rejects_other_shapes(hip):
    from ccd_amd.utils.DBSCAN import DBSCAN_cluster, label_cluster, region_cluster
    for cls in (DBSCAN_cluster, label_cluster, region_cluster):
        with pytest.raises(ValueError, match="32, 128"):
            cls()(torch.zeros(32, 64, device=hip.device))
        with pytest.raises(ValueError, match="32, 128"):
            cls()(np.zeros((32, 64), np.float32))
