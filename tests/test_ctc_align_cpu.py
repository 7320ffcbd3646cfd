"""The alignment oracle (tests/ctc_align_np.py) proves itself against brute force over EVERY frame path that collapses to the word, and
the seeded inputs of the executor / GPU tests meet the margin condition.  The host half of CTCConvertor.tensor2chars.  No GPU, no
kernel."""
import itertools

import numpy as np
import pytest

import ctc_align_checks as K
import ctc_align_np as A
import ctc_beam_np as R
import ctc_lexicon_np as L


def _words(C, longest=3):
    return [w for n in range(longest + 1) for w in itertools.product(range(1, C), repeat=n)]


@pytest.mark.parametrize("normalized", (False, True))
def test_oracle_equals_brute_force(normalized):
    """All words of length 0..3 over C <= 3 at T <= 5: the score is the brute-force maximum, the path one of the maximisers."""
    seen = 0
    for T in range(1, 6):
        for C in (2, 3):
            x = R.small_case(T, C, seed=10 * T + C)
            x = R.softmax32(x) if normalized else x
            for w in _words(C):
                best, paths = A.brute_force(x, w, normalized)
                got = A.align(x, w, normalized)
                if got is None:
                    assert best == -np.inf and not A.feasible(w, T, C), (T, C, w)
                    continue
                assert abs(got.score - best) <= 1e-12 and A.path_of(got.frame_char, w) in paths, (T, C, w)
                assert A.valid(got.frame_char.tolist(), w) and abs(A.path_score(x, got.frame_char, w, normalized) - got.score) <= 1e-12
                assert abs(got.char_logp.sum() + sum(R.log_probs(x, normalized)[t, 0] for t in np.flatnonzero(got.frame_char < 0)) - best) <= 1e-12
                assert (len(paths) == 1) or got.margin == 0.0
                seen += 1
    assert seen >= 50


def test_exact_ties_follow_the_tie_rule():
    """Uniform frames (every path of a word ties) and frames with a few exact ties: of the maximisers the oracle returns the one the tie
    rule names - read from the last frame to the first, the largest state sequence.  `ab` at T = 5 is a b _ _ _."""
    got = A.align(np.zeros((5, 3), dtype=np.float32), (1, 2))
    assert got.frame_char.tolist() == [0, 1, -1, -1, -1] and got.spans.tolist() == [[0, 0], [1, 1]] and got.margin == 0.0
    assert got.score == pytest.approx(5 * np.log(1.0 / 3.0), abs=1e-12)
    rng = np.random.default_rng(3)
    seen = 0
    for T in range(1, 6):
        for C in (2, 3):
            for kind in ("uniform", "masked", "masked"):
                # every live class of a frame has the same lp, so all paths of finite probability add the same numbers in the same
                # order and tie exactly; masks (at least one class stays) take some of them away
                live = np.ones((T, C), dtype=bool) if kind == "uniform" else rng.random((T, C)) < 0.7
                live[np.arange(T), rng.integers(0, C, T)] = True
                for normalized in (False, True):
                    data = np.where(live, np.float32(0.5), np.float32(0.0)) if normalized else np.where(live, np.float32(0.0), -np.inf)
                    for w in _words(C):
                        best, paths = A.brute_force(data.astype(np.float32), w, normalized)
                        got = A.align(data.astype(np.float32), w, normalized)
                        assert (got is None) == (not paths), (T, C, kind, normalized, w)
                        if got is None:
                            continue
                        assert got.score == best and A.path_of(got.frame_char, w) == A.stay_first(paths), (T, C, kind, normalized, w)
                        assert len(paths) == 1 or got.margin == 0.0
                        seen += len(paths) > 1
    assert seen >= 50


def test_infeasible_rows_and_masks():
    x = R.small_case(4, 3, seed=3)
    assert A.align(x, (3,)) is None and A.align(x, (0, 1)) is None and A.align(x, (1, 1, 1)) is None and A.align(x, (-1,)) is None
    assert A.align(x, (1, 1)) is not None and A.align(x, (1, 2, 1, 2)).frame_char.tolist() == [0, 1, 2, 3]
    x[:, 2] = -np.inf
    assert A.align(x, (2,)) is None and A.align(x, (1,)) is not None
    x[1, :] = -np.inf
    assert A.align(x, ()) is None
    p = np.array([[0.5, 0.5, 0.0], [0.25, 0.0, 0.75]], dtype=np.float32)
    got = A.align(p, (1,), normalized=True)
    assert got.frame_char.tolist() == [0, -1] and got.score == pytest.approx(np.log(0.5) + np.log(0.25)) and got.margin == np.inf
    empty = A.align(R.small_case(6, 4, seed=1), ())
    assert empty.frame_char.tolist() == [-1] * 6 and empty.score == pytest.approx(R.log_probs(R.small_case(6, 4, seed=1), False)[:, 0].sum())


def test_score_is_below_the_sum_over_alignments():
    x = R.small_case(6, 3, seed=8)
    for w in _words(3):
        got = A.align(x, w)
        total = L.score(x, [w])[0]
        assert (got is None) == (total == -np.inf) and (got is None or got.score <= total + 1e-12)


def test_the_seeded_rows_meet_the_margin_condition():
    """The inputs of the executor and GPU tests: every feasible row has a margin >= 1e-6, so exact integers are required of all of them."""
    groups, want = K.seeded_oracle(0, 24)
    margins = [a.margin for row in want for a in row if a is not None]
    lengths = {len(w) for _, words, _ in groups for w in words}
    print(f"{len(margins)} feasible rows of {9 * len(groups)}, smallest margin {min(margins):.3e}")
    assert min(margins) >= A.SEEDED_MARGIN and 0 in lengths and max(lengths) >= 28
    assert max(x.shape[1] for x, _, _ in groups) >= 60 and max(x.shape[2] for x, _, _ in groups) >= 120
    assert K.seeded_oracle(0, 6)[0][0][1] == groups[0][1]                      # the executor's groups are the first of these


def test_chars_of_is_the_host_view():
    """CTCConvertor.chars_of on a hand-made record: the geometry of both kinds of box and the confidence."""
    from ccd_amd.convertor.ctc import CTCConvertor
    conv = CTCConvertor()
    a, b = conv.char2idx["a"], conv.char2idx["b"]
    Lmax, T = 3, 8
    rec = np.array([[a, b, 0, 1, 2, 5, 5, -1, -1, np.log(0.25), np.log(0.5), 0.0, -3.0, 0],
                    [a, 0, 0, -1, -1, -1, -1, -1, -1, 0, 0, 0, -np.inf, -1]], dtype=np.float32)
    got = conv.chars_of(rec, 1, T, Lmax, image_width=128, boxes="emission")
    assert got == [[("ab", -3.0, [("a", 16.0, 48.0, 1, 2, pytest.approx(0.5)), ("b", 80.0, 96.0, 5, 5, pytest.approx(0.5))])]]
    cells = conv.chars_of(rec, 1, T, Lmax, image_width=128, boxes="cells")[0][0][2]
    assert [(c[1], c[2]) for c in cells] == [(0.0, 64.0), (64.0, 128.0)] and [c[3:5] for c in cells] == [(1, 2), (5, 5)]
    from ccd_amd.convertor.attn import AttnConvertor
    with pytest.raises(NotImplementedError, match="CTC head only"):
        AttnConvertor().tensor2chars(None)
