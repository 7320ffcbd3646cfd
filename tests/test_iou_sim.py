"""Dino.metric.eval_IOU kernels under the CPU SIMT executor (tests/hipsim): the confusion counts against np.bincount (exactly) and
the five scores against the numpy restatement (1e-13: at most 32 fp64 quotients per sum, see tests/test_iou_gpu.py), on every
fixture case, every dtype pair, the tails of a wavefront's load and of a workgroup's chunk, split images, strided and misaligned
views, the logits path, the status bits and the ABI's error codes."""
import numpy as np
import pytest
import torch

from backends import Backend
import iou_np as R

TOL = 1e-13
DTYPES = (torch.uint8, torch.int32, torch.int64, torch.float32)


@pytest.fixture(scope="module")
def sim():
    with Backend("sim") as b:
        yield b


def _check(cm, scores, status, ev, gt, label=""):
    """cm / scores / status of the module against the restatement of the uint8 [B, ...] maps ev, gt."""
    want_cm, want = R.batch(ev, gt)
    assert cm.dtype == torch.int32 and tuple(cm.shape) == (len(ev), 32, 32)
    np.testing.assert_array_equal(cm.numpy(), want_cm, err_msg=label)
    got = scores.numpy() if isinstance(scores, torch.Tensor) else np.stack([s.numpy() for s in scores[:5]], axis=1)
    assert got.dtype == np.float64
    assert np.isnan(got).tolist() == np.isnan(want).tolist(), label
    np.testing.assert_allclose(np.nan_to_num(got), np.nan_to_num(want), rtol=0, atol=TOL, err_msg=label)
    np.testing.assert_array_equal(status.numpy(), 2 * np.isnan(want[:, 3]).astype(np.int32), err_msg=label)


def _run(ev_t, gt_t):
    from ccd_amd import ops
    cm, status = ops.seg_confusion(ev_t, gt_t)
    return cm, ops.seg_scores(cm, status), status


def test_fixtures_sim(sim, golden_dir):
    from ccd_amd.metric.eval_IOU import confusion, segmentation_scores
    names, cases, _ = R.load_cases(golden_dir)
    for name in names:
        c = cases[name]
        ev, gt = torch.from_numpy(c["eval"]), torch.from_numpy(c["gt"])
        s = segmentation_scores(ev, gt)
        _check(confusion(ev, gt), s, s.status, c["eval"][None], c["gt"][None], name)
        got = np.array([float(v[0]) for v in s[:5]])
        assert np.isnan(got).tolist() == np.isnan(c["scores"]).tolist(), name
        np.testing.assert_allclose(np.nan_to_num(got), np.nan_to_num(c["scores"]), rtol=0, atol=TOL, err_msg=name)
        assert bool(s.status[0] & 2) == bool(c["fore_raised"])


@pytest.mark.parametrize("edt", DTYPES)
@pytest.mark.parametrize("gdt", DTYPES)
def test_every_dtype_pair_sim(sim, edt, gdt):
    ev, gt = R.random_maps((2, 9, 30), 27, 11)
    _check(*_run(torch.from_numpy(ev).to(edt), torch.from_numpy(gt).to(gdt)), ev, gt, f"{edt} {gdt}")


def test_bool_maps_sim(sim):
    from ccd_amd.metric.eval_IOU import segmentation_scores
    ev, gt = R.text_like((2, 8, 40), 3)
    s = segmentation_scores(torch.from_numpy(ev).bool(), torch.from_numpy(gt).bool())
    _, want = R.batch(ev, gt)
    np.testing.assert_allclose(np.stack([v.numpy() for v in s[:5]], 1), want, rtol=0, atol=TOL)


def test_load_width_and_chunk_tails_sim(sim):
    """H W one less than, equal to and one more than the pixels a wavefront loads per step (4 per lane; 16 per lane for two aligned
    uint8 maps) and than the chunk of one workgroup; binary fp32 maps as the pipeline has them, and uint8 maps."""
    from ccd_amd import ops
    sizes = sorted({w + d for w in ops.SEG_WAVE_PIXELS + (ops.SEG_CHUNK,) for d in (-1, 0, 1)})
    assert sizes == [255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097]
    for n in sizes:
        ev, gt = R.random_maps((1, 1, n), 2, n)
        _check(*_run(torch.from_numpy(ev).float(), torch.from_numpy(gt).float()), ev, gt, f"fp32 {n}")
        _check(*_run(torch.from_numpy(ev), torch.from_numpy(gt)), ev, gt, f"uint8 {n}")


def test_image_split_over_workgroups_sim(sim):
    from ccd_amd import ops
    n = 2 * ops.SEG_CHUNK + 517                         # 3 workgroups per image, the last one partly filled
    ev, gt = R.random_maps((2, 1, n), 3, 5)
    _check(*_run(torch.from_numpy(ev), torch.from_numpy(gt).float()), ev, gt)
    ev, gt = R.random_maps((1, 1, n), 27, 6)            # more distinct keys per step than a wave combines: the LDS-atomic tail
    _check(*_run(torch.from_numpy(ev).long(), torch.from_numpy(gt).int()), ev, gt)


def test_strided_and_misaligned_views_sim(sim):
    ev, gt = R.random_maps((3, 3, 10, 24), 4, 9)
    e4, g4 = torch.from_numpy(ev).float(), torch.from_numpy(gt)
    # x[:, 1] of a [B, 3, H, W] tensor is read in place (image stride 3 H W)
    view_e, view_g = e4[:, 1], g4[:, 1]
    assert not view_e.is_contiguous()
    _check(*_run(view_e, view_g), ev[:, 1], gt[:, 1], "strided")
    # base pointers off 16-byte alignment: element offsets 1 (fp32: 4 bytes) and 3 (uint8)
    flat_e = torch.zeros(3 * 240 + 1, dtype=torch.float32)
    flat_g = torch.zeros(3 * 240 + 3, dtype=torch.uint8)
    off_e, off_g = flat_e[1:].view(3, 10, 24), flat_g[3:].view(3, 10, 24)
    off_e.copy_(e4[:, 0])
    off_g.copy_(g4[:, 0])
    assert off_e.data_ptr() % 16 != 0 and off_g.data_ptr() % 4 != 0
    _check(*_run(off_e, off_g), ev[:, 0], gt[:, 0], "misaligned")
    # an image stride that is no multiple of 4 elements: rows of a [B, 241] buffer
    buf = torch.zeros(3, 241, dtype=torch.float32)
    buf[:, :240] = e4[:, 2].reshape(3, 240)
    _check(*_run(buf[:, :240].unflatten(1, (10, 24)), g4[:, 2]), ev[:, 2], gt[:, 2], "odd stride")


def test_batch_invariance_and_repeatability_sim(sim):
    ev, gt = R.text_like((3, 16, 70), 8)
    e, g = torch.from_numpy(ev).float(), torch.from_numpy(gt).float()
    cm, scores, status = _run(e, g)
    cm2, scores2, status2 = _run(e, g)
    assert torch.equal(cm, cm2) and torch.equal(status, status2) and scores.numpy().tobytes() == scores2.numpy().tobytes()
    for i in range(3):
        cmi, si, sti = _run(e[i:i + 1], g[i:i + 1])
        assert torch.equal(cm[i:i + 1], cmi) and torch.equal(status[i:i + 1], sti)
        assert scores[i:i + 1].numpy().tobytes() == si.numpy().tobytes()
    _check(cm, scores, status, ev, gt)


def _logits_check(logits, gt, label):
    from ccd_amd.metric.eval_IOU import seg_logits_scores
    from ccd_amd import ops
    pred = logits.argmax(1).numpy().astype(np.uint8)
    cm, status = ops.seg_confusion_logits(logits, torch.from_numpy(gt))
    s = seg_logits_scores(logits, torch.from_numpy(gt).float())
    _check(cm, s, s.status, pred, gt, label)
    assert torch.equal(status & 1, torch.zeros_like(status))


def test_logits_path_sim(sim):
    g = torch.Generator().manual_seed(4)
    logits = torch.randn(2, 2, 6, 10, generator=g)
    _logits_check(logits, R.random_maps((2, 6, 10), 2, 1)[1], "[2, 2, 6, 10]")
    # an exact tie: the first index wins, as in torch.argmax
    logits = torch.randn(1, 5, 9, 13, generator=g)
    logits[0, 3, 4, 6] = logits[0, 1, 4, 6] = logits[0].max() + 1.0
    logits[0, :, 0, 0] = 0.25
    assert logits[0, :, 4, 6].argmax() == 1 and logits[0, :, 0, 0].argmax() == 0
    _logits_check(logits, R.random_maps((1, 9, 13), 5, 2)[1], "[1, 5, 9, 13]")
    # a [:, :2] channel view of a 3-channel tensor, read in place
    three = torch.randn(3, 3, 8, 12, generator=g)
    three[:, 2] = 100.0                                                    # would win every pixel if it were read
    assert not three[:, :2].is_contiguous()
    _logits_check(three[:, :2], R.random_maps((3, 8, 12), 2, 3)[1], "[:, :2]")
    # two classes: logit1 > logit0 (a tie is class 0), the rule of ops.seg_to_mask
    two = torch.zeros(1, 2, 4, 8)
    two[0, 1, 0, :4] = 1e-3
    from ccd_amd import ops
    cm, _ = ops.seg_confusion_logits(two, torch.zeros(1, 4, 8, dtype=torch.uint8))
    assert cm[0, 0, 1] == 4 and cm[0, 0, 0] == 28


def test_status_bits_sim(sim):
    from ccd_amd import ops
    from ccd_amd.metric import eval_IOU as M
    base = torch.zeros(6, 4, 9)
    base[:, 1:3, 2:7] = 1.0
    ev = base.clone()
    ev[1, 0, 0], ev[2, 3, 8], ev[3, 1, 1], ev[4, 2, 2] = 32.0, -1.0, 0.5, float("nan")
    cm, status = ops.seg_confusion(ev, base)
    assert status.tolist() == [0, 1, 1, 1, 1, 0]
    assert cm.sum((1, 2)).tolist() == [36, 35, 35, 35, 35, 36]                # the offending pixels are not counted
    scores = ops.seg_scores(cm, status)
    assert torch.isnan(scores[1:5]).all() and not torch.isnan(scores[[0, 5]]).any() and status.tolist() == [0, 1, 1, 1, 1, 0]
    # the same in gt, in integer maps, and in logits
    cm, status = ops.seg_confusion(base, ev)
    assert status.tolist() == [0, 1, 1, 1, 1, 0]
    for dt, bad in ((torch.int32, -1), (torch.int64, 32), (torch.int64, 1 << 40), (torch.uint8, 200)):
        m = torch.zeros(2, 3, 5, dtype=dt)
        m[1, 2, 4] = bad
        assert ops.seg_confusion(m, torch.zeros(2, 3, 5, dtype=torch.uint8))[1].tolist() == [0, 1]
    logits = torch.randn(2, 2, 3, 5)
    logits[1, 1, 0, 0] = float("nan")
    s = M.seg_logits_scores(logits, torch.zeros(2, 3, 5, dtype=torch.uint8))
    assert s.status[0] & 1 == 0 and s.status[1] == 1 and torch.isnan(s.mean_IU[1]) and not torch.isnan(s.mean_IU[0])
    # the numpy path raises what the contract says
    one = np.zeros((4, 9), dtype=np.uint8)
    assert isinstance(M.pixel_accuracy(one, one), float) and M.pixel_accuracy(one, one) == 1.0
    with pytest.raises(IndexError):
        M.fore_IU(one, one)
    with pytest.raises(ValueError):
        M.mean_IU(ev[1].numpy(), base[1].numpy())
    with pytest.raises(ValueError):
        M.mean_IU(np.full((4, 9), 40, dtype=np.int16), one)
    with pytest.raises(M.EvalSegErr):
        M.mean_IU(one, one[:, :8])
    # the tensor path gives NaN where the numpy path raises
    assert torch.isnan(M.fore_IU(torch.from_numpy(one), torch.from_numpy(one)))
    assert M.fore_IU(base, base).shape == (6,) and M.fore_IU(base[0], base[0]).shape == ()


def test_meter_sim(sim):
    from ccd_amd.metric.eval_IOU import SegMeter
    ev, gt = R.text_like((5, 8, 40), 12)
    gt[4] = 0
    ev[4] = 0                                                                # fore_IU undefined for the last image
    meter = SegMeter()
    meter.update(torch.from_numpy(ev[:2]), torch.from_numpy(gt[:2]).float())
    logits = torch.stack([1.0 - torch.from_numpy(ev[2:]).float(), torch.from_numpy(ev[2:]).float()], 1)
    meter.update_logits(logits, torch.from_numpy(gt[2:]))
    out = meter.compute()
    cms, want = R.batch(ev, gt)
    assert out["n_images"] == 5 and out["n_fore_defined"] == 4
    pooled = R.scores_of(cms.sum(0))
    for k, name in enumerate(R.NAMES):
        assert abs(out[name] - np.nanmean(want[:, k])) < TOL and abs(out["dataset_" + name] - pooled[k]) < TOL, name


def test_abi_contract_sim(sim):
    from ccd_amd import _lib, ops
    lib = _lib.get()
    assert lib.ccd_abi_version() >= 17
    x = torch.zeros(2, 64, dtype=torch.uint8)
    cm = torch.full((2, 32, 32), 7, dtype=torch.int32)
    status = torch.full((2,), 7, dtype=torch.int32)
    scores = torch.zeros(2, 5, dtype=torch.float64)
    p = _lib.ptr
    ok = (p(x), 0, 64, p(x), 0, 64, 2, 64, p(cm), p(status), 0)
    assert lib.ccd_seg_confusion(*ok) == 0 and cm[:, 0, 0].tolist() == [64, 64] and cm.sum() == 128 and status.tolist() == [0, 0]
    for i in (0, 3, 8, 9):                                # a missing pointer
        bad = list(ok)
        bad[i] = None
        assert lib.ccd_seg_confusion(*bad) == -1, i
    for i, v in ((1, 4), (4, -1), (7, 0), (7, 1 << 31)):     # an unknown dtype code, pixels < 1, pixels >= 2^31
        bad = list(ok)
        bad[i] = v
        assert lib.ccd_seg_confusion(*bad) == -2, (i, v)
    assert lib.ccd_seg_confusion(None, 0, 0, None, 0, 0, 0, 64, None, None, 0) == 0          # an empty batch: a no-op
    lg = torch.zeros(2, 2, 64)
    okl = (p(lg), 128, 64, 2, p(x), 0, 64, 2, 64, p(cm), p(status), 0)
    assert lib.ccd_seg_confusion_logits(*okl) == 0 and cm[:, 0, 0].tolist() == [64, 64]
    for i in (0, 4, 9, 10):
        bad = list(okl)
        bad[i] = None
        assert lib.ccd_seg_confusion_logits(*bad) == -1, i
    for i, v in ((3, 1), (3, 33), (5, 9), (8, 0), (8, 1 << 31)):
        bad = list(okl)
        bad[i] = v
        assert lib.ccd_seg_confusion_logits(*bad) == -2, (i, v)
    assert lib.ccd_seg_confusion_logits(None, 0, 0, 2, None, 0, 0, 0, 64, None, None, 0) == 0
    assert lib.ccd_seg_scores(p(cm), p(status), 2, p(scores), 0) == 0 and status.tolist() == [2, 2]
    for i in (0, 1, 3):
        bad = [p(cm), p(status), 2, p(scores), 0]
        bad[i] = None
        assert lib.ccd_seg_scores(*bad) == -1
    assert lib.ccd_seg_scores(None, None, 0, None, 0) == 0
    # the wrappers: an empty batch gives empty results without a launch
    cm0, st0 = ops.seg_confusion(x[:0].view(0, 8, 8), x[:0].view(0, 8, 8))
    assert tuple(cm0.shape) == (0, 32, 32) and tuple(ops.seg_scores(cm0, st0).shape) == (0, 5)
