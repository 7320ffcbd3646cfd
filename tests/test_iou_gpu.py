"""Dino.metric.eval_IOU on a real MI355X, through libccd_hip.so (run with -m gpu): the reference's recorded outputs, the numpy
restatement on the pipeline's shapes, the multi-workgroup path, the logits path, repeatability, batch invariance, the numpy-in
contract and the absence of host synchronisation.

Gates.  The counts are integers: any difference from np.bincount is a bug.  Each score is a sum of at most 32 fp64 quotients of
exactly represented integers (t d <= A^2 < 2^53 for A <= 2^26 pixels) followed by at most one division, so its error is bounded by
about 34 ulp, roughly 4e-15, on values in [0, 1]; 1e-13 absolute leaves a 25x margin for the difference in summation order
against numpy and nothing for a wrong count."""
import functools

import numpy as np
import pytest
import torch

from backends import Backend
import iou_np as R

pytestmark = pytest.mark.gpu

TOL = 1e-13


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    with Backend("hip") as b:
        yield b


def _check(scores, cm, ev, gt, label):
    """SegScores + cm of the module against the restatement of the uint8 [B, ...] maps ev, gt; returns the restatement's scores."""
    want_cm, want = R.batch(ev, gt)
    assert cm.dtype == torch.int32 and cm.is_cuda
    np.testing.assert_array_equal(cm.cpu().numpy(), want_cm, err_msg=label)
    got = torch.stack(list(scores[:5]), 1)
    assert got.dtype == torch.float64 and got.is_cuda and tuple(got.shape) == (len(ev), 5)
    got = got.cpu().numpy()
    assert np.isnan(got).tolist() == np.isnan(want).tolist(), label
    np.testing.assert_allclose(np.nan_to_num(got), np.nan_to_num(want), rtol=0, atol=TOL, err_msg=label)
    np.testing.assert_array_equal(scores.status.cpu().numpy(), 2 * np.isnan(want[:, 3]).astype(np.int32), err_msg=label)
    return want


def test_iou_fixtures(hip, golden_dir):
    from ccd_amd.metric.eval_IOU import confusion, segmentation_scores
    names, cases, _ = R.load_cases(golden_dir)
    for name in names:
        c = cases[name]
        ev, gt = torch.from_numpy(c["eval"]).to(hip.device), torch.from_numpy(c["gt"]).to(hip.device)
        s = segmentation_scores(ev, gt)
        _check(s, confusion(ev, gt), c["eval"][None], c["gt"][None], name)
        got = np.array([float(v[0]) for v in s[:5]])
        assert np.isnan(got).tolist() == np.isnan(c["scores"]).tolist(), name
        np.testing.assert_allclose(np.nan_to_num(got), np.nan_to_num(c["scores"]), rtol=0, atol=TOL, err_msg=name)
        assert bool(s.status[0].item() & 2) == bool(c["fore_raised"]), name


@functools.lru_cache(maxsize=None)
def _maps(kind):
    """(eval, gt) uint8 maps on the host, made once."""
    if kind == "binary":
        return R.random_maps((64, 32, 128), 2, 21)
    if kind == "classes27":
        return R.random_maps((8, 32, 128), 27, 22, flip=0.2)
    if kind == "odd":
        return R.random_maps((3, 97, 203), 5, 23)
    if kind == "large":
        return R.text_like((1, 512, 512), 24)
    raise KeyError(kind)


@pytest.mark.parametrize("kind,dtype", [("binary", torch.float32), ("classes27", torch.uint8), ("odd", torch.int64),
                                        ("large", torch.uint8), ("large", torch.float32)])
def test_scores_against_restatement(hip, kind, dtype):
    from ccd_amd.metric.eval_IOU import confusion, segmentation_scores
    ev, gt = _maps(kind)
    e, g = torch.from_numpy(ev).to(hip.device).to(dtype), torch.from_numpy(gt).to(hip.device).to(dtype)
    _check(segmentation_scores(e, g), confusion(e, g), ev, gt, f"{kind} {dtype}")


def test_logits_against_argmax(hip):
    from ccd_amd import ops
    from ccd_amd.metric.eval_IOU import seg_logits_scores
    g = torch.Generator().manual_seed(31)
    logits = torch.randn(32, 2, 32, 128, generator=g)
    logits[3, :, 5, 7] = 0.5                                                  # a tie: class 0
    _, gt = R.text_like((16, 32, 128), 32)
    pred = logits[:16].argmax(1).numpy().astype(np.uint8)
    assert pred[3, 5, 7] == 0
    dev_logits, masks = logits.to(hip.device), torch.from_numpy(gt).to(hip.device).float()
    view = dev_logits[:16]                                                    # the student's half of a 2B batch, read in place
    s = seg_logits_scores(view, masks)
    cm, _ = ops.seg_confusion_logits(view, masks)
    _check(s, cm, pred, gt, "logits [:16]")
    # 5 classes through a channel view of 6
    six = torch.randn(4, 6, 16, 40, generator=g)
    six[:, 5] = 50.0
    _, gt5 = R.random_maps((4, 16, 40), 5, 33)
    d6 = six.to(hip.device)
    s = seg_logits_scores(d6[:, :5], torch.from_numpy(gt5).to(hip.device))
    cm, _ = ops.seg_confusion_logits(d6[:, :5], torch.from_numpy(gt5).to(hip.device))
    _check(s, cm, six[:, :5].argmax(1).numpy().astype(np.uint8), gt5, "logits [:, :5]")


def test_repeatable_and_batch_invariant(hip):
    from ccd_amd import ops
    for kind, dtype in (("binary", torch.float32), ("large", torch.uint8), ("odd", torch.int64)):
        ev, gt = _maps(kind)
        e, g = torch.from_numpy(ev).to(hip.device).to(dtype), torch.from_numpy(gt).to(hip.device).to(dtype)
        cm1, st1 = ops.seg_confusion(e, g)
        sc1 = ops.seg_scores(cm1, st1)
        cm2, st2 = ops.seg_confusion(e, g)
        sc2 = ops.seg_scores(cm2, st2)
        assert torch.equal(cm1, cm2) and torch.equal(st1, st2) and torch.equal(sc1.view(torch.int64), sc2.view(torch.int64)), kind
        for i in range(0, len(ev), 7):
            cmi, sti = ops.seg_confusion(e[i:i + 1], g[i:i + 1])
            sci = ops.seg_scores(cmi, sti)
            assert torch.equal(cm1[i:i + 1], cmi) and torch.equal(sc1[i:i + 1].view(torch.int64), sci.view(torch.int64)), (kind, i)


def test_strided_and_invalid_inputs(hip):
    from ccd_amd.metric import eval_IOU as M
    ev, gt = R.random_maps((4, 3, 32, 128), 3, 41)
    e4, g4 = torch.from_numpy(ev).to(hip.device).float(), torch.from_numpy(gt).to(hip.device)
    _check(M.segmentation_scores(e4[:, 1], g4[:, 2]), M.confusion(e4[:, 1], g4[:, 2]), ev[:, 1], gt[:, 2], "x[:, 1] views")
    off = torch.zeros(4 * 4096 + 1, device=hip.device)[1:].view(4, 32, 128)        # a base 4 bytes off 16-byte alignment
    off.copy_(e4[:, 0])
    _check(M.segmentation_scores(off, g4[:, 0]), M.confusion(off, g4[:, 0]), ev[:, 0], gt[:, 0], "misaligned")
    bad = e4[:, 0].clone()
    bad[1, 3, 3], bad[2, 0, 0], bad[3, 31, 127] = 32.0, 0.5, float("nan")
    s = M.segmentation_scores(bad, g4[:, 0])
    assert s.status.tolist()[1:] == [1, 1, 1] and s.status[0].item() & 1 == 0
    assert torch.isnan(torch.stack(list(s[:5]), 1)[1:]).all() and not torch.isnan(s.mean_IU[0])
    assert M.confusion(bad, g4[:, 0]).sum((1, 2)).tolist() == [4096, 4095, 4095, 4095]
    one = torch.zeros(32, 128, device=hip.device)
    assert torch.isnan(M.fore_IU(one, one)) and M.fore_IU(one, one).shape == () and M.pixel_accuracy(one, one).item() == 1.0
    assert M.mean_IU(one.bool(), one.bool()).item() == 1.0


def test_numpy_contract(hip, golden_dir):
    from Dino.metric import eval_IOU as M
    _, cases, _ = R.load_cases(golden_dir)
    c = cases["classes27"]
    fns = (M.pixel_accuracy, M.mean_accuracy, M.mean_IU, M.fore_IU, M.frequency_weighted_IU)
    for k, f in enumerate(fns):
        v = f(c["eval"], c["gt"])
        assert isinstance(v, float) and abs(v - c["scores"][k]) <= TOL
        assert abs(f(c["eval"].astype(np.int16), c["gt"].astype(np.float64)) - c["scores"][k]) <= TOL
    zeros = cases["zeros_zeros"]
    assert M.pixel_accuracy(zeros["eval"], zeros["gt"]) == 1.0
    with pytest.raises(IndexError):
        M.fore_IU(zeros["eval"], zeros["gt"])
    with pytest.raises(M.EvalSegErr):
        M.mean_IU(c["eval"], c["gt"][:, :100])
    for bad in (np.full((32, 128), 32, np.uint8), np.full((32, 128), -1, np.int32), np.full((32, 128), 0.5, np.float32),
                np.full((32, 128), np.nan, np.float32), np.full((32, 128), 0.5, np.float64)):
        with pytest.raises(ValueError):
            M.mean_IU(bad, c["gt"])


def test_no_host_sync_and_meter(hip):
    from ccd_amd.metric.eval_IOU import SegMeter, seg_logits_scores, segmentation_scores
    ev, gt = _maps("binary")
    gt = gt.copy()
    ev = ev.copy()
    ev[5], gt[5] = 0, 0                                                       # fore_IU undefined for one image
    e, g = torch.from_numpy(ev).to(hip.device).float(), torch.from_numpy(gt).to(hip.device).float()
    logits = torch.stack([1.0 - e[32:], e[32:]], 1).contiguous()
    meter = SegMeter()
    meter.update(e[:1], g[:1])                                                # (allocates the meter's state)
    meter.reset()
    torch.cuda.synchronize()
    # scores and accumulation without one host synchronisation (torch raises on a synchronising call)
    torch.cuda.set_sync_debug_mode("error")
    try:
        s = segmentation_scores(e, g)
        sl = seg_logits_scores(logits, g[32:])
        meter.update(e[:32], g[:32])
        meter.update_logits(logits, g[32:])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    cms, want = R.batch(ev, gt)
    assert torch.equal(torch.stack(list(sl[:5]), 1).view(torch.int64), torch.stack(list(s[:5]), 1)[32:].view(torch.int64))
    out = meter.compute()
    assert out["n_images"] == 64 and out["n_fore_defined"] == 63
    pooled = R.scores_of(cms.sum(0))
    for k, name in enumerate(R.NAMES):
        assert abs(out[name] - np.nanmean(want[:, k])) <= TOL, name
        assert abs(out["dataset_" + name] - pooled[k]) <= TOL, name
