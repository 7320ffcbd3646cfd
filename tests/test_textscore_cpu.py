"""Host side of the device scoring path of TextAccuracy (no kernel runs): the normalisation rule the kernel applies per code point
against Python's `_KEEP.sub('', s.lower())` for every code point and for random strings, `encode_truth`, `score_table`, and the
numpy restatement of decode + scoring (tests/textscore_np.py) against tensor2idx + idx2str + update."""
import sys

import numpy as np
import pytest

import textscore_np as R


def test_normalisation_rule_matches_python_for_every_code_point():
    from ccd_amd.metric.eval_acc import _KEEP, normalise
    points = np.arange(sys.maxunicode + 1)
    points = points[(points < 0xD800) | (points > 0xDFFF)]                    # the 1 112 064 scalar values
    assert points.size == 1_112_064
    got = R.normalise_codes(points)
    sub, mismatches = _KEEP.sub, 0
    for p, g in zip(points.tolist(), got.tolist()):
        want = sub("", chr(p).lower())
        mismatches += want != ("" if g < 0 else chr(g))
    assert mismatches == 0
    assert normalise("Hello, World-1^") == "helloworld1^"


def test_normalisation_rule_matches_python_on_random_strings():
    """The rule is applied per code point while str.lower() sees the whole string (final sigma, I WITH DOT ABOVE -> two code
    points): 200 000 random strings over an alphabet that has those, of which every kept character must come out the same."""
    from ccd_amd.metric.eval_acc import normalise
    rs = np.random.RandomState(5)
    alphabet = np.array([ord(c) for c in "abzAKZ09^ .-_ΣσςİKıIi̇一龥丁鿿㐀ÀßǅŉΐᾈΩ"] + [0x1F600, 0x10400, 0x1E900])
    lens = rs.randint(0, 12, size=200_000)
    flat = alphabet[rs.randint(0, alphabet.size, size=int(lens.sum()))]
    norm = R.normalise_codes(flat)
    text = flat.astype("<u4").tobytes().decode("utf-32-le")
    stops = np.cumsum(lens)
    mismatches = 0
    for a, b in zip((stops - lens).tolist(), stops.tolist()):
        kept = norm[a:b]
        mismatches += normalise(text[a:b]) != kept[kept >= 0].astype("<u4").tobytes().decode("utf-32-le")
    assert mismatches == 0


def test_encode_truth():
    from ccd_amd.metric.eval_acc import encode_truth
    words = ["", "a", "Hello", R.SPECIAL, "x" * 200, "龥\U0001F600", ""]
    codes, lens = encode_truth(words)
    assert codes.dtype == np.int32 and lens.dtype == np.int32 and codes.shape == (7, 200)
    assert lens.tolist() == [len(w) for w in words]
    for row, n, w in zip(codes, lens, words):
        assert row[:n].tolist() == [ord(c) for c in w] and not row[n:].any()
    codes, lens = encode_truth(["", ""])
    assert codes.shape == (2, 1) and lens.tolist() == [0, 0]
    codes, lens = encode_truth([])
    assert codes.shape == (0, 1) and lens.shape == (0,)
    assert encode_truth(("ab", "c"))[0].tolist() == [[97, 98], [99, 0]]            # what a collated batch hands over: a tuple


def test_score_table_against_idx2char():
    from ccd_amd.convertor.attn import AttnConvertor
    from ccd_amd.metric.eval_acc import normalise
    conv = AttnConvertor(dict_type="DICT90", with_unknown=True, max_seq_len=40)
    raw, norm = conv.score_table()
    assert raw.dtype == norm.dtype == np.int32 and raw.shape == (93, 5) and norm.shape == (93, 3)
    assert conv.score_table()[0] is raw                                            # built once
    text = lambda row: "".join(chr(c) for c in row if c >= 0)
    for c, s in enumerate(conv.idx2char):
        want = "" if c in (conv.end_idx, conv.padding_idx) else s
        assert text(raw[c]) == want and text(norm[c]) == normalise(want), c
        assert (raw[c][len(want):] == -1).all() and (norm[c][len(normalise(want)):] == -1).all()
    assert text(raw[conv.unknown_idx]) == "<UKN>" and text(norm[conv.unknown_idx]) == "ukn"
    # without <UKN> every class is one character wide; a separate start class is written as idx2str writes it
    raw, norm = AttnConvertor(dict_type="DICT36", with_unknown=False, max_seq_len=128).score_table()
    assert raw.shape == (38, 1) and norm.shape == (38, 1)
    two = AttnConvertor(dict_type="DICT36", with_unknown=False, start_end_same=False, max_seq_len=20)
    raw, norm = two.score_table()
    assert text(raw[two.start_idx]) == "<BOS/EOS>" and text(norm[two.start_idx]) == "boseos" and text(raw[two.end_idx]) == ""


def test_score_table_is_none_when_the_prediction_cannot_fit():
    from ccd_amd.convertor.attn import AttnConvertor
    from ccd_amd import ops
    assert AttnConvertor(max_seq_len=64, with_unknown=True).score_table() is None           # 64 steps x 'ukn' = 192 > 128
    assert AttnConvertor(max_seq_len=42, with_unknown=True).score_table() is not None       # 126
    assert AttnConvertor(max_seq_len=43, with_unknown=True).score_table() is None           # 129
    assert AttnConvertor(max_seq_len=128, with_unknown=False).score_table() is not None
    assert AttnConvertor(max_seq_len=129, with_unknown=False).score_table() is None
    assert ops.TEXT_COLS == 128


@pytest.mark.parametrize("B,T", [(1, 25), (5, 40), (67, 25), (67, 40)])
def test_restatement_agrees_with_the_host_path(B, T):
    conv, scores, gts = R.adversarial_case(B, T)
    want, preds = R.host_records(scores, conv, gts)
    np.testing.assert_array_equal(R.restate(scores, conv, gts), want)
    assert preds[0] == "<UKN>" * T and want[0].tolist()[2:] == [200, 0]


def test_restatement_on_the_fixture(golden_dir):
    conv, scores, gts, values = R.fixture_case(golden_dir)
    rec = R.restate(scores, conv, gts)
    np.testing.assert_array_equal(rec, R.host_records(scores, conv, gts)[0])
    assert rec[:, 0].sum() == values["ted"] and len(rec) == values["words"]
    assert rec[:, 3].sum() / 18 == values["cwr"] and rec[:, 1].sum() / rec[:, 2].sum() == values["ccr"]
    got = R.host_result(conv, [(scores[i:i + 6], gts[i:i + 6]) for i in (0, 6, 12)])
    for k in ("ccr", "cwr", "ted", "ned", "ted/w", "words"):
        assert got[k] == pytest.approx(values[k], rel=1e-12), k
