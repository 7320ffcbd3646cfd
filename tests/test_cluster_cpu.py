"""Dino.utils.DBSCAN without a GPU: the numpy restatement of the three clusterers against the reference's recorded outputs
(tests/golden/cluster_cases.npz) and against scikit-learn's DBSCAN, and the reference's import paths."""
import numpy as np
import pytest

import cluster_np


def test_restatement_matches_reference_fixtures(golden_dir):
    names, masks, planes, ties = cluster_np.load_cases(golden_dir)
    assert len(names) >= 30
    checked = 0
    for k, f in cluster_np.CLUSTERERS.items():
        for i, name in enumerate(names):
            if ties[k][i]:
                continue
            np.testing.assert_array_equal(f(masks[i]), planes[k][i], err_msg=f"{k}/{name}")
            checked += 1
    assert checked >= 3 * len(names) - 8


def test_fixture_covers_the_edge_cases(golden_dir):
    names, masks, planes, ties = cluster_np.load_cases(golden_dir)
    case = dict(zip(names, range(len(names))))
    # nonzero mask with no pixel > 0.1: zero DBSCAN planes, label / region still see the pixels
    i = case["below_threshold"]
    assert masks[i].any() and not planes["dbscan"][i].any() and planes["label"][i].any() and planes["region"][i].any()
    assert not planes["dbscan"][case["lines_1px"]].any()
    # more than 26 qualifying clusters: DBSCAN keeps the 26 leftmost, label_cluster the first 26 found
    i = case["many_staggered"]
    assert planes["dbscan"][i].any(axis=(1, 2)).all() and not np.array_equal(planes["dbscan"][i], planes["label"][i])
    # specks use up region slots
    assert planes["region"][case["specks_use_slots"]].any(axis=(1, 2)).sum() == 6
    # overlapping region planes
    assert (planes["region"][case["overlapping_boxes"]].sum(axis=0) > 1).any()
    assert not ties["region"].any() and ties["dbscan"][case["mean_col_tie"]]


def test_region_fixture_pins_the_tie_order(golden_dir):
    """Equal xmin + xmax between boxes that both make a plane, and a tie across the 26-slot cut: the opposite tie order gives
    different planes there, so a kernel that broke ties the other way would fail the fixture."""
    names, masks, planes, ties = cluster_np.load_cases(golden_dir)
    for name in ("region_key_tie", "region_tie_cut"):
        i = names.index(name)
        assert not ties["region"][i]
        want = planes["region"][i]
        np.testing.assert_array_equal(cluster_np.region_planes(masks[i]), want)
        flipped = cluster_np.box_planes(cluster_np.region_boxes(masks[i], reverse_ties=True))
        assert not np.array_equal(flipped, want), name
    assert planes["region"][names.index("region_key_tie")].any(axis=(1, 2)).sum() == 6


def test_dbscan_restatement_matches_sklearn():
    sklearn_cluster = pytest.importorskip("sklearn.cluster")
    masks = cluster_np.random_masks(99, seed=3)
    for m in masks:
        ys, xs = np.nonzero(m > 0.1)
        want = np.full(m.shape, -1)
        if ys.size:
            want[ys, xs] = sklearn_cluster.DBSCAN(eps=1.5, min_samples=4).fit_predict(np.stack([ys, xs], 1))
        np.testing.assert_array_equal(cluster_np.dbscan_assign(m), want)


def test_reference_import_paths():
    import Dino.utils.DBSCAN as D
    from Dino.model.dino_vision import dbscan, label
    from ccd_amd.utils import DBSCAN as mine
    assert D is mine
    assert isinstance(dbscan, D.DBSCAN_cluster) and isinstance(label, D.label_cluster)
    assert isinstance(D.region_cluster(), D.region_cluster) and isinstance(D.DBSCAN_cluster(eps=3.0, min_samples=9), D.DBSCAN_cluster)


def test_shape_is_checked_before_any_device_work():
    from ccd_amd.utils.DBSCAN import DBSCAN_cluster, label_cluster, region_cluster
    for cls in (DBSCAN_cluster, label_cluster, region_cluster):
        with pytest.raises(ValueError, match="32, 128"):
            cls()(np.zeros((32, 64), np.float32))
