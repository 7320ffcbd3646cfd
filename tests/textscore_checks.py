"""The checks of the recognition-scoring kernels (kernels/textscore.h) that run on either backend: the CPU SIMT executor
(tests/test_textscore_sim.py) and the MI355X (tests/test_textscore_gpu.py).  `device` is where the tensors live.

Gates.  A record is four integers: any difference from TextAccuracy.update on the decoded strings is a bug.  Of the totals only
`ned` is a floating-point sum; its terms distance / max(len, 1) are correctly rounded fp64 quotients on both sides, so only the
order of the n-term sum differs: rel n * 2^-52 (textscore_np.check_result)."""
import numpy as np
import pytest
import torch

import textscore_np as R


def _score(conv, scores, gts, device):
    """ops.text_score on scores (a tensor on the device, or a numpy array) -> records as numpy."""
    from ccd_amd import ops
    from ccd_amd.metric.eval_acc import encode_truth
    if not isinstance(scores, torch.Tensor):
        scores = torch.from_numpy(scores).to(device)
    raw, norm = (torch.from_numpy(t).to(device) for t in conv.score_table())
    codes, lens = (torch.from_numpy(a).to(device) for a in encode_truth(gts))
    rec = ops.text_score(scores, raw, norm, conv.end_idx, conv.padding_idx, codes, lens)
    assert rec.dtype == torch.int32 and rec.device == scores.device and tuple(rec.shape) == (len(gts), 4)
    return rec.cpu().numpy()


def check_fixture(device, golden_dir):
    """The 18 pairs behind eval_acc.npz, scored in three batches of six, against the reference's recorded values."""
    from ccd_amd.metric.eval_acc import TextAccuracy
    conv, scores, gts, values = R.fixture_case(golden_dir)
    dev_scores = torch.from_numpy(scores).to(device)
    metric = TextAccuracy()
    for i in (0, 6, 12):
        metric.update_scores(dev_scores[i:i + 6], gts[i:i + 6], conv)
    got = metric.result()
    R.check_result(got, dict(values, time=got["time"]), 18)
    assert type(got["words"]) is float and got["time"] == 0.0
    np.testing.assert_array_equal(_score(conv, dev_scores, gts, device), R.host_records(scores, conv, gts)[0])


def check_adversarial(device, B, T):
    from ccd_amd.metric.eval_acc import TextAccuracy
    conv, scores, gts = R.adversarial_case(B, T)
    want, _ = R.host_records(scores, conv, gts)
    got = _score(conv, scores, gts, device)
    bad = np.flatnonzero((got != want).any(1))
    assert bad.size == 0, [(int(i), gts[i], got[i].tolist(), want[i].tolist()) for i in bad[:5]]
    metric = TextAccuracy()
    half = (B + 1) // 2                                            # two uneven batches into one accumulator
    dev_scores = torch.from_numpy(scores).to(device)
    for a, b in ((0, half), (half, B)):
        if b > a:
            metric.update_scores(dev_scores[a:b], gts[a:b], conv)
    res = metric.result()
    R.check_result(res, dict(R.host_result(conv, [(scores, gts)]), time=res["time"]), B)


def check_named_edges(device):
    """The hand-made samples one by one, with the values they must give."""
    from ccd_amd.convertor.attn import AttnConvertor
    conv = AttnConvertor(max_seq_len=25)
    cls = lambda s: conv.str2idx([s])[0]
    ukn, pad = conv.unknown_idx, conv.padding_idx
    cases = [([], "", [0, 0, 0, 1]),                                           # <EOS> at step 0, empty ground truth
             (cls("!!--"), ".. ..", [0, 0, 5, 1]),                             # both normalise to nothing
             (cls("Hello-World"), "hello world!", [0, 8, 12, 1]),              # 'ello' and 'orld' match position-wise
             (cls("ab") + [pad] + cls("c"), "abc", [0, 3, 3, 1]),              # <PAD> skipped
             ([ukn] * 25, "ukn" * 25, [0, 0, 75, 1]),                          # 75 normalised columns, no <EOS>
             ([ukn] * 25, "", [75, 0, 0, 0]),
             (cls("ki"), "Kİ", [0, 0, 2, 1]),                        # both fold to 'ki'
             (cls("k^i"), "K^İ", [3, 0, 3, 0]),                      # '^' is no DICT90 character: 'kukni' against 'k^i'
             (cls("abc"), "a\U0001F600c一", [2, 2, 4, 0])]
    rows = R.rows_of(conv, [c[0] for c in cases], 25)
    gts = [c[1] for c in cases]
    scores = R.make_scores(rows, conv.num_classes(), 3)
    np.testing.assert_array_equal(R.host_records(scores, conv, gts)[0], [c[2] for c in cases])
    np.testing.assert_array_equal(_score(conv, scores, gts, device), [c[2] for c in cases])
    # an exact tie between two classes of a step: the lower index wins
    tie = torch.from_numpy(scores[:1].copy())
    tie[0, 0, :] = -5.0
    tie[0, 0, [7, 3]] = 0.0                                                    # step 0: classes 3 and 7 tie -> '3'
    tie[0, 1, conv.end_idx] = 1.0
    assert _score(conv, tie.to(device), ["3"], device).tolist() == [[0, 1, 1, 1]]


def check_strided_views(device):
    """probs[:, :done] of a longer buffer and every second sample of a batch are read in place."""
    conv, scores, gts = R.adversarial_case(67, 25)
    want, _ = R.host_records(scores, conv, gts)
    buf = torch.full((67, 40, 93), 9.0)                                        # (steps behind `done` would win every arg-max)
    buf[:, :25] = torch.from_numpy(scores)
    buf = buf.to(device)
    view = buf[:, :25]
    assert not view.is_contiguous()
    np.testing.assert_array_equal(_score(conv, view, gts, device), want)
    every_other = view[::2]
    assert every_other.stride(0) == 2 * 40 * 93
    np.testing.assert_array_equal(_score(conv, every_other, gts[::2], device), want[::2])
    # the ground truth as rows of a wider buffer
    from ccd_amd import ops
    from ccd_amd.metric.eval_acc import encode_truth
    codes, lens = encode_truth(gts)
    wide = torch.full((67, codes.shape[1] + 3), 97, dtype=torch.int32)
    wide[:, :codes.shape[1]] = torch.from_numpy(codes)
    raw, norm = (torch.from_numpy(t).to(device) for t in conv.score_table())
    rec = ops.text_score(view, raw, norm, conv.end_idx, conv.padding_idx, wide.to(device)[:, :codes.shape[1]], torch.from_numpy(lens).to(device))
    np.testing.assert_array_equal(rec.cpu().numpy(), want)


def check_repeatable(device):
    from ccd_amd.metric.eval_acc import TextAccuracy
    conv, scores, gts = R.adversarial_case(67, 40)
    dev_scores = torch.from_numpy(scores).to(device)
    totals = []
    for _ in range(2):
        m = TextAccuracy()
        recs = [m.update_scores(dev_scores[a:b], gts[a:b], conv) for a, b in ((0, 30), (30, 67))]
        totals.append((m._totals.cpu().numpy().tobytes(), torch.cat(recs).cpu().numpy().tobytes()))
    assert totals[0] == totals[1]
    # the accumulator adds to what it holds, and mixes with the host path in one result()
    m = TextAccuracy()
    m.update_scores(dev_scores[:30], gts[:30], conv)
    idx, _ = conv.tensor2idx(torch.from_numpy(scores[30:]))
    m.update(gts[30:], conv.idx2str(idx))
    res = m.result()
    R.check_result(res, dict(R.host_result(conv, [(scores, gts)]), time=res["time"]), 67)
    assert m.result() == res                                                   # reading the totals does not consume them


def check_abi_contract(device):
    from ccd_amd import _lib, ops
    from ccd_amd.metric.eval_acc import TextAccuracy, encode_truth
    lib = _lib.get()
    assert lib.ccd_abi_version() >= 18
    conv, scores, gts = R.adversarial_case(5, 25)
    s = torch.from_numpy(scores).to(device)
    raw, norm = (torch.from_numpy(t).to(device) for t in conv.score_table())
    codes, lens = (torch.from_numpy(a).to(device) for a in encode_truth(gts))
    rec = torch.full((5, 4), -7, dtype=torch.int32, device=device)
    st = _lib.stream()
    ok = [s, 25 * 93, 93, 5, 25, 93, raw, 5, norm, 3, conv.end_idx, conv.padding_idx, codes, codes.shape[1], codes.shape[1], lens, rec, st]
    assert lib.ccd_text_score(*ok) == 0
    np.testing.assert_array_equal(rec.cpu().numpy(), R.host_records(scores, conv, gts)[0])
    for i in (0, 6, 8, 12, 15, 16):                                            # a missing pointer
        bad = list(ok)
        bad[i] = None
        assert lib.ccd_text_score(*bad) == -1, i
    for i, v in ((1, -1), (2, -1), (3, -1), (13, -1), (14, -1)):               # a negative stride, batch or size
        bad = list(ok)
        bad[i] = v
        assert lib.ccd_text_score(*bad) == -1, (i, v)
    # steps * norm_width > 128 (43 x 3; 129 x 1), widths outside 1..64, no steps, no classes, end_idx outside the classes
    for i, v in ((4, 43), (4, 0), (5, 0), (7, 0), (7, 65), (9, 0), (9, 65), (10, -1), (10, 93)):
        bad = list(ok)
        bad[i] = v
        assert lib.ccd_text_score(*bad) == -2, (i, v)
    assert lib.ccd_text_score(*(ok[:4] + [129] + ok[5:9] + [1] + ok[10:])) == -2
    # a decoder without a <PAD> output (NRTRDecoder: num_classes - 1 scores): pad_idx lies behind the classes, the tables keep their row
    rows92 = R.rows_of(conv, [[1, 2], [], [3], [4, 5, 6], [7]], 25)
    rows92[rows92 == conv.padding_idx] = conv.end_idx
    scores92 = R.make_scores(rows92, 92, 1)
    no_pad = [torch.from_numpy(scores92).to(device), 25 * 92, 92, 5, 25, 92] + ok[6:]
    assert lib.ccd_text_score(*no_pad) == 0
    np.testing.assert_array_equal(rec.cpu().numpy(), R.host_records(scores92, conv, gts)[0])
    np.testing.assert_array_equal(_score(conv, scores92, gts, device), rec.cpu().numpy())           # (the wrapper takes the longer tables)
    assert lib.ccd_text_score(None, 0, 0, 0, 25, 93, None, 5, None, 3, 91, 92, None, 0, 0, None, None, st) == 0      # an empty batch
    empty = list(ok)
    empty[12], empty[14] = None, 0                                             # gt_cols == 0: no ground-truth pointer needed
    assert lib.ccd_text_score(*empty) == 0 and rec[:, 2].tolist() == [0] * 5
    totals = ops.text_totals(device)
    ned = totals[5:].view(torch.float64)
    assert lib.ccd_text_accumulate(rec, 5, totals[:5], ned, st) == 0 and totals[3].item() == 5
    for i in (0, 2, 3):
        bad = [rec, 5, totals[:5], ned, st]
        bad[i] = None
        assert lib.ccd_text_accumulate(*bad) == -1, i
    assert lib.ccd_text_accumulate(rec, -1, totals[:5], ned, st) == -1
    assert lib.ccd_text_accumulate(None, 0, None, None, st) == 0 and totals[3].item() == 5
    # the wrappers: an empty batch gives an empty result without a launch; what the static check refuses raises
    assert tuple(ops.text_score(s[:0], raw, norm, conv.end_idx, conv.padding_idx, codes[:0], lens[:0]).shape) == (0, 4)
    with pytest.raises(RuntimeError, match="ccd_text_score failed: unsupported shape"):
        ops.text_score(torch.zeros(1, 43, 93, device=device), raw, norm, conv.end_idx, conv.padding_idx, codes[:1], lens[:1])
    with pytest.raises(TypeError, match=r"^ccd_text_score: gt expects int32, got int64$"):
        ops.text_score(s, raw, norm, conv.end_idx, conv.padding_idx, codes.long(), lens)
    with pytest.raises(NotImplementedError):
        TextAccuracy(case_sensitive=True).update_scores(s, gts, conv)
    from ccd_amd.convertor.attn import AttnConvertor
    with pytest.raises(ValueError, match="score on the host"):
        TextAccuracy().update_scores(torch.zeros(1, 64, 93, device=device), ["a"], AttnConvertor(max_seq_len=64))
