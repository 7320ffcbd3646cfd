"""Recognition scoring (ccd_amd/metric/eval_acc.py) restated in numpy, and the cases the kernel tests share.

    normalise_codes(codes)              the per-code-point normalisation rule of kernels/textscore.h, vectorised
    restate(scores, convertor, gts)     arg-max decoding + scoring -> records int [B, 4] (distance, equal raw characters, raw gt
                                        length, word correct), from the class tables alone - no strings
    host_records(scores, conv, gts)     the same four numbers from the host path: tensor2idx + idx2str + TextAccuracy.update
    make_scores(classes, C, seed)       class sequences -> fp32 [B, T, C] scores whose arg-max they are, by a wide margin
    fixture_case / adversarial_case     the inputs of tests/test_textscore_{sim,gpu}.py
"""
import functools
import os

import numpy as np
import torch

RECORD = ("distance", "equal_chars", "gt_chars", "word_correct")
GT_LENGTHS = (0, 1, 63, 64, 65, 127, 128, 129, 200)
MARGIN = 1.0                 # least gap between the winner of a step and the runner-up that make_scores guarantees (it gives ~6.7)


def normalise_codes(codes):
    """int array of code points -> the normalised code points, -1 where the metric drops the character."""
    c = np.asarray(codes, dtype=np.int64)
    upper = (c >= ord("A")) & (c <= ord("Z"))
    out = np.where(upper, c + 32, c)
    out = np.where(c == 0x212A, ord("k"), out)
    out = np.where(c == 0x0130, ord("i"), out)
    keep = (((out >= ord("a")) & (out <= ord("z"))) | ((out >= ord("0")) & (out <= ord("9"))) | (out == ord("^"))
            | ((out >= 0x4E00) & (out <= 0x9FA5)))
    return np.where(keep, out, -1)


def codes_of(s):
    return np.frombuffer(s.encode("utf-32-le", "surrogatepass"), dtype="<u4").astype(np.int64)


def distance(a, b):
    """Levenshtein distance of two int arrays, one row of the table at a time (D[i][j] = j + min_{k <= j} (t[k] - k))."""
    j = np.arange(len(a) + 1)
    row = j.copy()
    for i, ch in enumerate(b, start=1):
        t = np.concatenate([[i], np.minimum(row[1:] + 1, row[:-1] + (a != ch))])
        row = j + np.minimum.accumulate(t - j)
    return int(row[-1])


def decode(scores, end_idx, pad_idx):
    """fp32 [B, T, C] -> per sample the kept classes: first maximum per step, cut at the first end class, padding skipped."""
    cls = np.asarray(scores).argmax(-1)                   # (numpy: the first maximum)
    out = []
    for row in cls:
        ends = np.flatnonzero(row == end_idx)
        row = row[:ends[0]] if ends.size else row
        out.append(row[row != pad_idx])
    return out


def restate(scores, convertor, gts):
    raw_t, norm_t = convertor.score_table()
    rec = np.zeros((len(gts), 4), dtype=np.int64)
    for i, (cls, gt) in enumerate(zip(decode(scores, convertor.end_idx, convertor.padding_idx), gts)):
        raw = raw_t[cls].ravel()
        raw = raw[raw >= 0]
        norm = norm_t[cls].ravel()
        norm = norm[norm >= 0]
        g = codes_of(gt)
        gn = normalise_codes(g)
        gn = gn[gn >= 0]
        n = min(len(raw), len(g))
        d = distance(norm, gn)
        rec[i] = d, int((raw[:n] == g[:n]).sum()), len(g), int(d == 0)
    return rec


def host_records(scores, convertor, gts):
    """What TextAccuracy.update adds for each sample, decoded by tensor2idx + idx2str (the host path of compute())."""
    from ccd_amd.metric.eval_acc import TextAccuracy
    idx, _ = convertor.tensor2idx(torch.as_tensor(np.ascontiguousarray(scores)))
    preds = convertor.idx2str(idx)
    rec = np.zeros((len(gts), 4), dtype=np.int64)
    for i, (gt, pt) in enumerate(zip(gts, preds)):
        m = TextAccuracy()
        m.update([gt], [pt])
        rec[i] = m.total_ed, m.correct_num_char, m.total_num_char, m.correct_num_word
    return rec, preds


def host_result(convertor, batches):
    """result() of one TextAccuracy over (scores, gts) batches on the host path."""
    from ccd_amd.metric.eval_acc import TextAccuracy
    m = TextAccuracy()
    for scores, gts in batches:
        idx, _ = convertor.tensor2idx(torch.as_tensor(np.ascontiguousarray(scores)))
        m.update(list(gts), convertor.idx2str(idx))
    return m.result()


def make_scores(classes, C, seed):
    """classes int [B, T] -> fp32 [B, T, C]: log 0.9 for the class of a step, log(0.1 / (C - 1)) plus noise of at most 0.01 for
    the others.  The margin is asserted: with it the first maximum of the scores (the kernel) and the maximum of their softmax
    (tensor2idx) are the same class."""
    classes = np.asarray(classes)
    rs = np.random.RandomState(seed)
    s = (np.log(0.1 / (C - 1)) + rs.uniform(-0.01, 0.01, size=classes.shape + (C,))).astype(np.float32)
    np.put_along_axis(s, classes[..., None], np.float32(np.log(0.9)), axis=-1)
    top = np.sort(s, axis=-1)
    assert (top[..., -1] - top[..., -2]).min() > MARGIN
    assert (s.argmax(-1) == classes).all()
    return s


def rows_of(convertor, seqs, T, rs=None):
    """class lists -> int [B, T] rows.  A list shorter than T is followed by the end class, then by padding - or, with rs, by
    random classes (a second end class among them): whatever follows the first end class must not count."""
    out = np.full((len(seqs), T), convertor.padding_idx, dtype=np.int64)
    for row, seq in zip(out, seqs):
        seq = list(seq)[:T]
        row[:len(seq)] = seq
        if len(seq) < T:
            row[len(seq)] = convertor.end_idx
            if rs is not None and len(seq) + 1 < T:
                row[len(seq) + 1:] = rs.randint(0, convertor.num_classes(), size=T - len(seq) - 1)
    return out


def fixture_case(golden_dir):
    """The 18 prediction / ground-truth pairs behind tests/golden/eval_acc.npz: (convertor, scores [18, 25, 93], gts, names -> values)."""
    from ccd_amd.convertor.attn import AttnConvertor
    g = np.load(os.path.join(golden_dir, "eval_acc.npz"))
    conv = AttnConvertor(dict_type="DICT90", with_unknown=True, max_seq_len=25)
    preds = [str(s) for s in g["pred"]]
    classes = rows_of(conv, conv.str2idx(preds), 25)
    scores = make_scores(classes, conv.num_classes(), 7)
    assert conv.idx2str(conv.tensor2idx(torch.from_numpy(scores))[0]) == preds
    return conv, scores, [str(s) for s in g["gt"]], dict(zip([str(n) for n in g["names"]], g["values"].tolist()))


SPECIAL = "^一龥丁KİΣ!-. \U0001F600é"       # '^', CJK (both ends of the kept range), U+212A, U+0130, Σ, punctuation, astral


@functools.lru_cache(maxsize=None)
def adversarial_case(B, T):
    """(convertor, scores fp32 [B, T, 93], ground truths): the first samples are the hand-made edge cases, random ones follow."""
    from ccd_amd.convertor.attn import AttnConvertor
    conv = AttnConvertor(dict_type="DICT90", with_unknown=True, max_seq_len=T)
    rs = np.random.RandomState(1000 * B + T)
    ukn, pad, end = conv.unknown_idx, conv.padding_idx, conv.end_idx
    cls = lambda s: conv.str2idx([s])[0]
    alphabet = list("abcXYZ019!-.~ ") + list(SPECIAL)
    word = lambda n: "".join(rs.choice(alphabet, size=n))
    seqs, gts = [], []

    def add(seq, gt):
        seqs.append(list(seq))
        gts.append(gt)

    # <UKN> classes: the normalised prediction ('ukn' each) crosses 64 columns; no <EOS> at all; a 200-character ground truth
    add([ukn] * T, "ukn" * 22 + word(200 - 66))
    add([], "")                                               # <EOS> at step 0 against the empty string
    add(cls("ab") + [pad, pad] + cls("Cd") + [pad] + cls("e"), "abCde")          # <PAD> in the middle
    add(cls("!!--"), ".. ..")                                 # both normalise to the empty string: distance 0, a correct word
    add(cls("Hello-World"), "hello world!")                   # case-only and punctuation-only differences
    add(cls("k^i"), "K^İ" + "一龥" + "\U0001F600")
    add([ukn, ukn] + cls("a"), "<UKN>uKnK")             # the raw text of <UKN> position by position
    add(cls("abc"), "")                                       # an empty ground truth: distance = the prediction's length
    add([], "abc")
    for n in GT_LENGTHS:                                      # every ground-truth length around the 64-lane chunks
        gt = word(n)
        keep = [c for c in cls(gt) if rs.rand() > 0.15][:T]
        add(keep, gt)
        add([ukn if rs.rand() < 0.5 else int(rs.randint(0, 90)) for _ in range(T)], gt)
    while len(seqs) < B:
        gt = word(int(rs.choice(GT_LENGTHS + (5, 9, 17, 30))))
        body = [c if rs.rand() > 0.1 else int(rs.randint(0, 91)) for c in cls(gt)]
        if rs.rand() < 0.3:
            body.insert(int(rs.randint(0, len(body) + 1)), pad)
        add(body[:int(rs.randint(0, T + 1))], gt)
    order = list(range(len(seqs))) if B >= len(seqs) else list(rs.permutation(len(seqs))[:B])
    if B < len(seqs):
        order[0] = 0                                          # the <UKN> sample is in every batch
    classes = rows_of(conv, [seqs[i] for i in order], T, rs)
    return conv, make_scores(classes, conv.num_classes(), B + T), [gts[i] for i in order]


def check_result(got, want, n):
    """result() dictionaries: integer-valued entries exactly, quotients at rel 1e-15, ned at rel n * 2^-52 (only the order of the
    fp64 sum of n terms differs from the host)."""
    assert list(got) == list(want) == ["ccr", "cwr", "ted", "ned", "ted/w", "words", "time"]
    for k in ("ted", "words"):
        assert got[k] == want[k], (k, got[k], want[k])
    for k in ("ccr", "cwr", "ted/w"):
        assert abs(got[k] - want[k]) <= 1e-15 * abs(want[k]), (k, got[k], want[k])
    assert abs(got["ned"] - want["ned"]) <= n * 2.0 ** -52 * abs(want["ned"]), (got["ned"], want["ned"])
