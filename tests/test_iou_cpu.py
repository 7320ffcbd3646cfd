"""Dino.metric.eval_IOU without a GPU: the numpy restatement (tests/iou_np.py) against the reference's recorded outputs
(tests/golden/iou_cases.npz), the host helpers, the public names, the import paths, SegMeter's arithmetic and the error contract."""
import inspect

import numpy as np
import pytest
import torch

import iou_np as R


def test_restatement_matches_reference_fixtures(golden_dir):
    names, cases, _ = R.load_cases(golden_dir)
    assert len(names) == 11
    for name in names:
        c = cases[name]
        cm = R.confusion(c["eval"], c["gt"])
        # counts: the class lists and the per-class gt areas the reference's helpers gave
        t, n = cm.sum(1), cm.sum(0)
        np.testing.assert_array_equal(np.flatnonzero(t), c["gt_classes"], err_msg=name)
        np.testing.assert_array_equal(np.flatnonzero(n), c["eval_classes"], err_msg=name)
        np.testing.assert_array_equal(np.flatnonzero((t > 0) | (n > 0)), c["union_classes"], err_msg=name)
        np.testing.assert_array_equal(t[t > 0], c["masks_sum"], err_msg=name)
        assert cm.sum() == c["eval"].size
        got = R.scores_of(cm)
        assert np.isnan(got).tolist() == np.isnan(c["scores"]).tolist(), name
        assert bool(c["fore_raised"]) == bool(np.isnan(c["scores"][3])), name
        np.testing.assert_allclose(np.nan_to_num(got), np.nan_to_num(c["scores"]), rtol=0, atol=1e-13, err_msg=name)


def test_fixture_covers_the_issue_cases(golden_dir):
    names, cases, _ = R.load_cases(golden_dir)
    shapes = {tuple(cases[n]["eval"].shape) for n in names}
    assert {(32, 128), (1, 1), (5, 7), (33, 130)} <= shapes
    assert bool(cases["zeros_zeros"]["fore_raised"]) and cases["zeros_zeros"]["scores"][[0, 1, 2, 4]].tolist() == [1.0] * 4
    assert cases["ones_zeros"]["scores"].tolist() == [0.0] * 5
    three = cases["three_disjoint"]
    assert three["eval_classes"].tolist() == [0, 1] and three["gt_classes"].tolist() == [0, 2]
    assert len(cases["classes27"]["union_classes"]) == 27
    assert cases["labels_0_31"]["union_classes"].tolist() == [0, 31]
    single = cases["single_pixel"]
    assert int(single["eval"].sum()) == 1 and int(single["gt"].sum()) == 1
    flipped = (cases["binary_flip10"]["eval"] != cases["binary_flip10"]["gt"]).mean()
    assert 0.07 < flipped < 0.13


def test_helpers_match_recorded_class_lists(golden_dir):
    from ccd_amd.metric import eval_IOU as M
    names, cases, _ = R.load_cases(golden_dir)
    z = np.load(golden_dir + "/iou_cases.npz")
    for name in names:
        c = cases[name]
        ev, gt = c["eval"], c["gt"]
        cl, n_cl = M.extract_classes(gt)
        np.testing.assert_array_equal(cl, c["gt_classes"])
        assert n_cl == len(c["gt_classes"])
        np.testing.assert_array_equal(M.extract_classes(ev)[0], c["eval_classes"])
        ucl, n_ucl = M.union_classes(ev, gt)
        np.testing.assert_array_equal(ucl, c["union_classes"])
        assert n_ucl == len(ucl)
        masks = M.extract_masks(gt, cl, n_cl)
        assert masks.dtype == np.float64 and masks.shape == (n_cl,) + gt.shape
        np.testing.assert_array_equal(masks.sum(axis=(1, 2)), c["masks_sum"])
        em, gm = M.extract_both_masks(ev, gt, ucl, n_ucl)
        assert em.shape == gm.shape == (n_ucl,) + gt.shape and em.sum() == gm.sum() == gt.size
        assert M.segm_size(gt) == gt.shape and M.get_pixel_area(gt) == gt.size
        M.check_size(ev, gt)
    with pytest.raises(M.EvalSegErr) as e:
        M.check_size(np.zeros((2, 3)), np.zeros((2, 4)))
    assert str(e.value) == str(z["diffdim_message"]) and e.value.value == "DiffDim: Different dimensions of matrices!"
    with pytest.raises(IndexError):
        M.segm_size(np.zeros(3))


def test_public_names_and_signatures_match_the_reference(golden_dir):
    from ccd_amd.metric import eval_IOU as M
    _, _, api = R.load_cases(golden_dir)
    assert len(api) == 13
    for entry in api:
        name, params = entry[:-1].split("(")
        obj = getattr(M, name)
        assert ", ".join(inspect.signature(obj).parameters) == params, entry
    assert issubclass(M.EvalSegErr, Exception)


def test_import_paths():
    import Dino.metric.eval_IOU as D
    from ccd_amd.metric import eval_IOU as mine
    from Dino.metric.eval_IOU import fore_IU, frequency_weighted_IU, mean_accuracy, mean_IU, pixel_accuracy  # noqa: F401
    from Dino.metric.eval_IOU import SegMeter, confusion, seg_logits_scores, segmentation_scores  # noqa: F401
    import Dino.metric
    assert D is mine and Dino.metric.eval_IOU is mine
    from ccd_amd import ops
    assert ops.SEG_CLASSES == 32 and ops.SEG_CHUNK == 4096 and mine.SegScores._fields == ops.SEG_SCORES + ("status",)


def _hand_made():
    """Confusion matrices with known scores: (cm int64 [3, 32, 32], status)."""
    cm = np.zeros((3, 32, 32), dtype=np.int64)
    cm[0, 0, 0], cm[0, 0, 1], cm[0, 1, 0], cm[0, 1, 1] = 50, 10, 5, 35          # binary
    cm[1, 0, 0] = 100                                                         # one class: fore_IU undefined
    cm[2, 0, 0], cm[2, 2, 0], cm[2, 0, 1], cm[2, 31, 31] = 40, 30, 20, 10       # class 1 in eval only, class 2 in gt only
    return cm


def test_host_scores_of_a_matrix_match_the_restatement():
    from ccd_amd.metric.eval_IOU import _scores_of_matrix
    for cm in _hand_made():
        got = np.array(_scores_of_matrix(cm.tolist()))
        want = R.scores_of(cm)
        assert np.isnan(got).tolist() == np.isnan(want).tolist()
        np.testing.assert_allclose(np.nan_to_num(got), np.nan_to_num(want), rtol=0, atol=1e-13)
    binary = _scores_of_matrix(_hand_made()[0].tolist())
    assert binary[0] == 0.85 and binary[3] == 35 / (40 + 45 - 35 + 1e-6)
    assert all(np.isnan(_scores_of_matrix(np.zeros((32, 32), dtype=np.int64).tolist())))


def test_segmeter_arithmetic():
    from ccd_amd.metric.eval_IOU import SegMeter
    cm = _hand_made()
    scores = np.stack([R.scores_of(c) for c in cm])
    status = np.array([0, 2, 0], dtype=np.int32)
    meter = SegMeter()
    empty = meter.compute()
    assert empty["n_images"] == 0 and np.isnan(empty["mean_IU"]) and np.isnan(empty["dataset_fore_IU"])
    # two updates: images 0..1, then image 2 and an invalid image (status bit 0: NaN scores, its counts are not pooled)
    meter._add(torch.from_numpy(cm[:2]).int(), torch.from_numpy(scores[:2]), torch.from_numpy(status[:2]))
    bad_cm = np.zeros((1, 32, 32), dtype=np.int64)
    bad_cm[0, 3, 3] = 77
    meter._add(torch.from_numpy(np.concatenate([cm[2:], bad_cm])).int(),
               torch.from_numpy(np.concatenate([scores[2:], np.full((1, 5), np.nan)])), torch.tensor([0, 1], dtype=torch.int32))
    out = meter.compute()
    assert out["n_images"] == 4 and out["n_fore_defined"] == 2
    for k, name in enumerate(R.NAMES):
        col = scores[:, k]
        assert abs(out[name] - np.nanmean(col)) < 1e-14, name
    pooled = R.scores_of(cm.sum(0))
    for k, name in enumerate(R.NAMES):
        assert abs(out["dataset_" + name] - pooled[k]) < 1e-13, name
    meter.reset()
    assert meter.compute()["n_images"] == 0 and meter.sums is None


def test_contract_errors_before_any_device_work():
    from ccd_amd import _lib
    from ccd_amd.metric import eval_IOU as M
    assert _lib._stream_override is None
    a = torch.zeros(2, 8, 16, dtype=torch.uint8)
    fns = (M.pixel_accuracy, M.mean_accuracy, M.mean_IU, M.fore_IU, M.frequency_weighted_IU, M.confusion, M.segmentation_scores,
           M.SegMeter().update)
    for f in fns:
        with pytest.raises(M.EvalSegErr):
            f(a, torch.zeros(2, 8, 17, dtype=torch.uint8))
        with pytest.raises(M.EvalSegErr):
            f(a, a[0])
        with pytest.raises(TypeError):
            f(a.double(), a.double())
        with pytest.raises(TypeError):
            f(a.half(), a)
        with pytest.raises(TypeError):
            f(a, a.numpy())
        with pytest.raises(RuntimeError, match="GPU"):
            f(a, a)
        with pytest.raises(RuntimeError, match="GPU"):
            f(a.bool(), a.float())
    with pytest.raises(M.EvalSegErr):
        M.pixel_accuracy(np.zeros((4, 5), np.uint8), np.zeros((5, 4), np.uint8))
    with pytest.raises(ValueError):
        M.pixel_accuracy(np.full((4, 5), 0.5), np.zeros((4, 5)))
    with pytest.raises(TypeError):
        M.confusion(a.numpy(), a.numpy())
    logits = torch.zeros(2, 2, 8, 16)
    for f in (M.seg_logits_scores, M.SegMeter().update_logits):
        with pytest.raises(TypeError):
            f(logits.double(), a)
        with pytest.raises(ValueError):
            f(logits[0], a)
        with pytest.raises(M.EvalSegErr):
            f(logits, a[:, :7])
        with pytest.raises(RuntimeError, match="GPU"):
            f(logits, a)
        with pytest.raises(RuntimeError, match="GPU"):
            f(logits, a.float()[:, None])
