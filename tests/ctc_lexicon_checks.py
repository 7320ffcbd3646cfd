"""The checks of lexicon-constrained CTC decoding (kernels/ctc_lexicon.h: ccd_ctc_lexicon_score, ccd_ctc_lexicon_best) that run on either
backend: the CPU SIMT executor (tests/test_ctc_lexicon_sim.py) and the MI355X (tests/test_ctc_lexicon_gpu.py).  `device` is where the
tensors live.

Oracle: tests/ctc_lexicon_np.py, the specification in fp64 numpy, itself checked against tests/ctc_np.ctc_reference, torch's fp64
F.ctc_loss and brute force in tests/test_ctc_lexicon_cpu.py.  Gates (the project's existing ones):
  * |score - oracle| <= 2^-23 |oracle| + 1e-9: the one rounding to fp32 (ctc_beam_checks.one_rounding); -inf exactly where the oracle says;
  * against another kernel's fp32 number (the -nll of ccd_ctc_loss_fwd, a beam score): <= 2^-22 max(1, |v|), two roundings;
  * the order of ccd_ctc_lexicon_best equals the oracle's stable order - on inputs where the oracle's smallest gap between the
    scores of two different words of a sample is >= 1e-9 (asserted per sample; a word listed twice is the tie case and is excluded);
  * two runs give identical bits."""
import functools

import numpy as np
import pytest
import torch

import ctc_beam_checks as BK
import ctc_beam_np as R
import ctc_lexicon_np as L

LD = 128
SEEDS = (100, 101, 102)
one_rounding = BK.one_rounding


def two_roundings(v):
    return 2.0 ** -22 * max(1.0, abs(v))


def frames_view(device, x):
    """x fp32 [B, T, C] -> the [B, T, C] view of a [B * T, 128] buffer with NaN behind column C, the view CTCHeadFn hands out."""
    x = torch.as_tensor(np.asarray(x, dtype=np.float32))
    B, T, C = x.shape
    buf = torch.full((B * T, LD), float("nan"))
    buf[:, :C] = x.reshape(B * T, C)
    return buf.to(device).view(B, T, LD)[:, :, :C]


def run_score(device, x, words, normalized=False, subset=None, max_len=None):
    """-> fp32 [B, V] (or [B, K]) as numpy, through ops.ctc_lexicon / ops.ctc_lexicon_score."""
    from ccd_amd import ops
    lexicon = ops.ctc_lexicon(torch.from_numpy(L.to_tensor(words, max_len)))
    if subset is not None:
        subset = torch.as_tensor(subset, dtype=torch.int32).to(device)
    out = ops.ctc_lexicon_score(frames_view(device, x), lexicon, normalized=normalized, subset=subset)
    assert out.dtype == torch.float32 and tuple(out.shape) == (x.shape[0], len(words) if subset is None else subset.shape[1])
    return out.cpu().numpy()


def run_raw(device, x, table, normalized=False):
    """One launch of ccd_ctc_lexicon_score on the unsplit int64 table [V, max_len]: the lanes per word follow max_len alone."""
    from ccd_amd import _lib
    view = frames_view(device, x)
    B, T, C = view.shape
    words = torch.from_numpy(table).to(device)
    out = torch.full((B, table.shape[0]), 77.0, device=device)
    assert _lib.get().ccd_ctc_lexicon_score(view, view.stride(0), view.stride(1), B, T, C, 1 if normalized else 0, words, table.shape[0],
                                            table.shape[1], None, None, 0, out, table.shape[0], _lib.stream()) == 0
    return out.cpu().numpy()


def run_best(device, scores, nbest):
    from ccd_amd import ops
    index, best = ops.ctc_lexicon_best(torch.as_tensor(scores).to(device), nbest)
    assert index.dtype == torch.int32 and best.dtype == torch.float32 and tuple(index.shape) == tuple(best.shape) == (len(scores), nbest)
    return index.cpu().numpy(), best.cpu().numpy()


def compare_scores(got, want, where):
    """One sample: fp32 [V] against the oracle's fp64 [V]."""
    assert not np.isnan(got).any(), where
    for v, (g, w) in enumerate(zip(got, want)):
        if w == -np.inf:
            assert g == -np.inf, (where, v, g)
        else:
            assert abs(float(g) - w) <= one_rounding(w), (where, v, float(g), w)


def compare_best(index, best, scores32, want, nbest, where):
    """One sample: the kernel's slots against the oracle's stable order `want` = [(column, fp64 score)]; the scores are the fp32 row's."""
    for r in range(nbest):
        if r < len(want):
            assert index[r] == want[r][0], (where, r, index.tolist(), want)
            assert best[r].tobytes() == scores32[want[r][0]].tobytes(), (where, r)
        else:
            assert index[r] == -1 and best[r] == -np.inf, (where, r, index.tolist())


@functools.lru_cache(maxsize=None)
def batch_oracle(seed, normalized):
    """(words, fp64 scores [9, 70]) of the oracle batch; the gap condition and the two -inf words hold for every sample."""
    x = BK.peaked(seed, normalized)
    words = L.batch_lexicon(seed)
    exact = np.stack([L.score(x[b], words, normalized) for b in range(x.shape[0])])
    for b in range(x.shape[0]):
        assert L.min_gap(exact[b], words) >= L.MIN_GAP, (seed, normalized, b)
        assert int(np.isneginf(exact[b]).sum()) == 2, (seed, normalized, b)
    return words, exact


# ------------------------------------------------------------------------------------------------ 1. against brute force
def check_exhaustive(device):
    """The lexicon is every word brute force finds (in dictionary order): its scores, their sum and its order."""
    for T, C in R.EXHAUSTIVE:
        for normalized in (False, True):
            x = R.small_case(T, C, seed=10 * T + C)
            x = R.softmax32(x) if normalized else x
            exact = R.brute_force(x, normalized)
            words = sorted(w for w, _ in exact)
            want = dict(exact)
            assert L.min_gap(np.array([want[w] for w in words]), words) >= L.MIN_GAP
            got = run_score(device, x[None], words, normalized)[0]
            compare_scores(got, np.array([want[w] for w in words]), (T, C, normalized))
            assert abs(float(np.exp(got.astype(np.float64)).sum()) - 1.0) <= 16 * 2.0 ** -23
            index, best = run_best(device, got[None], 16)
            compare_best(index[0], best[0], got, [(words.index(w), s) for w, s in exact], 16, (T, C, normalized))


# ------------------------------------------------------------------------------------------------ 2. against the oracle
def check_oracle_batch(device, seeds=SEEDS):
    """B = 9, T = 32, C = 92, V = 70 (one partial strip, all three length classes), logits and the fp32 softmax."""
    differ = 0
    for seed in seeds:
        for normalized in (False, True):
            x = BK.peaked(seed, normalized)
            words, exact = batch_oracle(seed, normalized)
            got = run_score(device, x, words, normalized)
            for b in range(x.shape[0]):
                compare_scores(got[b], exact[b], (seed, normalized, b))
            for nbest in (1, 4, 16):
                index, best = run_best(device, got, nbest)
                for b in range(x.shape[0]):
                    compare_best(index[b], best[b], got[b], L.best(exact[b], nbest), nbest, (seed, normalized, nbest, b))
            if seed == seeds[0]:
                assert run_score(device, x, words, normalized).tobytes() == got.tobytes()
                again = run_best(device, got, 16)
                assert all(a.tobytes() == c.tobytes() for a, c in zip(again, run_best(device, got, 16)))
            if not normalized:
                import ctc_np as G
                greedy = G.greedy(x)
                differ += sum(tuple(greedy[0][b, :greedy[1][b]].tolist()) != tuple(words[L.best(exact[b], 1)[0][0]])
                              for b in range(x.shape[0]))
    print(f"the lexicon's best word differs from the greedy word on {differ} of {9 * len(seeds)} samples")


# ------------------------------------------------------------------------------------------------ 3. the length-class seams
SEAM_WORDS = [(3, 3, 4, 5, 5, 6, 7), (3, 3, 4, 5, 5, 6, 7, 7), (9, 9, 1, 2, 2, 3, 4, 4, 5, 6, 7, 7, 8, 9, 9),
              (9, 9, 1, 2, 2, 3, 4, 4, 5, 6, 7, 7, 8, 9, 9, 9), (), (17,), (11, 11)]       # lengths 7, 8, 15, 16: 15 / 17 / 31 / 33 states


def check_seams(device):
    """A word's score is the same bits whichever segment width (16 / 32 / 64 lanes per word) it is scored in; seven words per
    launch: full and partial waves at 4 and 2 words per wave."""
    for normalized in (False, True):
        x = BK.peaked(100, normalized)[:2]
        seen = {}
        for max_len in (7, 8, 15, 16, 31):
            pool = [w for w in SEAM_WORDS if len(w) <= max_len]
            words = [pool[k % len(pool)] for k in range(7)]
            words[0] = max(pool, key=len)                                     # the longest word that fits is always there
            got = run_raw(device, x, L.to_tensor(words, max_len), normalized)
            for b in range(2):
                exact = L.score(x[b], words, normalized)
                compare_scores(got[b], exact, ("seam", normalized, max_len, b))
                for k, w in enumerate(words):
                    assert seen.setdefault((b, w), got[b, k].tobytes()) == got[b, k].tobytes(), (normalized, max_len, b, w)
        assert len({w for _, w in seen}) == len(SEAM_WORDS)


# ------------------------------------------------------------------------------------------------ 4. the limits
def check_limits(device):
    """T = 64, C = 128 with label 127 and L = 31 (63 states); T = 1; C = 2."""
    long_words = [(127,) * 31, tuple(127 if i & 1 else 1 for i in range(31)), (127,), (126, 127, 127), (), (127,) * 33]
    for normalized in (False, True):
        x = BK.peaked(103, normalized, 5, 64, 128)[:2]
        got = run_score(device, x, long_words[:5], normalized)
        for b in range(2):
            exact = L.score(x[b], long_words[:5], normalized)
            assert np.isfinite(exact).all()
            compare_scores(got[b], exact, ("long", normalized, b))
        one = R.small_case(1, 92, seed=5)
        one = R.softmax32(one) if normalized else one
        words = [(), (40,), (40, 41)]
        exact = L.score(one, words, normalized)
        assert np.isfinite(exact[:2]).all() and exact[2] == -np.inf
        compare_scores(run_score(device, one[None], words, normalized)[0], exact, ("T=1", normalized))
        two = R.small_case(6, 2, seed=62)
        two = R.softmax32(two) if normalized else two
        words = [(), (1,), (1, 1), (1, 1, 1), (1, 1, 1, 1), (2,)]
        exact = L.score(two, words, normalized)
        assert np.isfinite(exact[:4]).all() and np.isneginf(exact[4:]).all()
        compare_scores(run_score(device, two[None], words, normalized)[0], exact, ("C=2", normalized))


# ------------------------------------------------------------------------------------------------ 5. masks
def check_masks(device):
    """An all -inf frame gives every word of that sample -inf and no best word; a masked class gives -inf for the words that hold
    it; the other samples are untouched; no NaN anywhere."""
    words = [(), (1,), (2,), (3,), (1, 2), (3, 1), (2, 2), (1, 3, 2), (2, 1, 2)]
    y = np.stack([R.small_case(5, 4, seed=6), R.small_case(5, 4, seed=7), R.small_case(5, 4, seed=8)])
    y[1, 2, :] = -np.inf
    y[2, :, 3] = -np.inf
    y[2, 0, 1] = -np.inf
    for normalized in (False, True):
        data = R.softmax32(y) if normalized else y
        if normalized:
            data[1, 2, :] = 0.0
        got = run_score(device, data, words, normalized)
        assert not np.isnan(got).any()
        exact = np.stack([L.score(data[b], words, normalized) for b in range(3)])
        for b in range(3):
            compare_scores(got[b], exact[b], ("masked", normalized, b))
        assert np.isneginf(got[1]).all() and np.isfinite(got[0]).all()
        assert [np.isneginf(v) for v in got[2]] == [3 in w for w in words]
        index, best = run_best(device, got, 4)
        assert (index[1] == -1).all() and np.isneginf(best[1]).all()
        for b in (0, 2):
            assert L.min_gap(exact[b], words) >= L.MIN_GAP
            compare_best(index[b], best[b], got[b], L.best(exact[b], 4), 4, ("masked", normalized, b))


# ------------------------------------------------------------------------------------------------ 6. subset
def check_subset(device):
    """[B, 5] entries out of order, repeated, -1 and >= V: the gathered columns of the full result, bit for bit; -inf at the padding."""
    x = BK.peaked(100, True)
    words, _ = batch_oracle(100, True)
    V = len(words)
    full = run_score(device, x, words, True)
    rng = np.random.default_rng(6)
    subset = rng.integers(0, V, (x.shape[0], 5)).astype(np.int32)
    subset[0] = [69, 3, 3, 0, 64]
    subset[1] = [-1, 5, V, 68, -7]
    subset[2] = [V + 5, -1, -1, 2 ** 31 - 1, 1]
    got = run_score(device, x, words, True, subset=subset)
    for b in range(x.shape[0]):
        for k in range(5):
            v = int(subset[b, k])
            if 0 <= v < V:
                assert got[b, k].tobytes() == full[b, v].tobytes(), (b, k, v)
            else:
                assert got[b, k] == -np.inf, (b, k, v)
    assert np.isfinite(got).sum() >= 5 * x.shape[0] - 12


# ------------------------------------------------------------------------------------------------ 7. ties
def check_ties(device):
    """One word at columns 3 and 40: identical bits, column 3 first."""
    x = BK.peaked(100, False)
    words = list(L.batch_lexicon(100))
    top = tuple(R.beam_search(x[0], 4)[0][0][0])                              # the beam's best word of sample 0: it leads the lexicon
    assert top not in words
    words[3] = words[40] = top
    got = run_score(device, x, words)
    assert all(got[b, 3].tobytes() == got[b, 40].tobytes() for b in range(x.shape[0]))
    exact = L.score(x[0], words)
    assert L.min_gap(exact, words) >= L.MIN_GAP and L.best(exact, 2) == [(3, exact[3]), (40, exact[40])]
    for nbest in (1, 2):
        index, best = run_best(device, got, nbest)
        assert index[0].tolist() == [3, 40][:nbest] and all(v.tobytes() == got[0, 3].tobytes() for v in best[0])
    index, _ = run_best(device, got, 16)
    for row in index.tolist():
        assert (3 in row or 40 not in row) and (40 not in row or row.index(3) + 1 == row.index(40)), row


# ------------------------------------------------------------------------------------------------ 8. against the other kernels
def check_against_loss(device, seeds=SEEDS):
    """score == -nll of ccd_ctc_loss_fwd on replicated rows for every (sample, feasible word) of the oracle batch (two roundings)."""
    worst = 0.0
    for seed in seeds:
        x = BK.peaked(seed, False)
        words, exact = batch_oracle(seed, False)
        got = run_score(device, x, words)
        keep = [[k for k in range(len(words)) if exact[b, k] > -np.inf] for b in range(x.shape[0])]
        pairs, nll = BK._nll_of(device, x, [[words[k] for k in row] for row in keep])
        assert len(pairs) == 68 * x.shape[0]
        at = iter(nll)
        for b, row in enumerate(keep):
            for k in row:
                v = next(at)
                assert abs(float(got[b, k]) + v) <= two_roundings(v), (seed, b, k, float(got[b, k]), -v)
                worst = max(worst, abs(float(got[b, k]) + v) / two_roundings(v))
    print(f"largest |score + nll| in units of the gate: {worst:.3f}")


def check_against_beam(device):
    """The words ops.ctc_beam_search(x, 16) returns, used as the lexicon: beam score <= lexicon score + tol; equality where nothing
    was pruned (R.EXHAUSTIVE)."""
    cases = [(BK.peaked(100, False), False, False), (BK.peaked(101, True), True, False)] + \
            [(R.small_case(T, C, seed=10 * T + C)[None], False, True) for T, C in R.EXHAUSTIVE]
    for x, normalized, exact in cases:
        paths, lengths, scores = BK.run_beam(device, x, 16, normalized)
        found = {(b, tuple(paths[b, r, :lengths[b, r]].tolist())): float(scores[b, r]) for b in range(x.shape[0]) for r in range(16)
                 if 0 <= lengths[b, r] <= 31}
        words = sorted({w for _, w in found})
        got = run_score(device, x, words, normalized)
        slack = 0.0
        for (b, w), s in found.items():
            v = float(got[b, words.index(w)])
            assert s <= v + two_roundings(v), (b, w, s, v)
            if exact:
                assert abs(s - v) <= two_roundings(v), (b, w, s, v)
            slack = max(slack, v - s)
        print(f"T = {x.shape[1]}, {len(words)} words: largest log p(word) - beam score {slack:.3e}")


def check_property(device, B, V, n_pairs):
    """V random words of length 0..31 over a small and a full alphabet (several strips, all three classes) under B samples: random
    pairs against ccd_ctc_loss_fwd (two roundings), the infeasible pairs -inf, two runs bit-identical."""
    from ccd_amd import ops
    rng = np.random.default_rng(7)
    T, C = 32, 92
    x = R.peaked_batch(200, B, T, C)
    words = []
    for v in range(V):
        n = int(rng.integers(0, 32))
        words.append(tuple(int(c) for c in rng.integers(1, 5 if v % 3 == 0 else C + 3 * (v % 50 == 1), n)))
    ok = np.array([L.feasible(w, T, C) for w in words])
    assert V // 2 <= ok.sum() <= V - 5 and {len(w) for w in words} == set(range(32))       # (a condition on the generator)
    got = run_score(device, x, words)
    assert got.shape == (B, V) and run_score(device, x, words).tobytes() == got.tobytes()
    assert np.isneginf(got[:, ~ok]).all() and np.isfinite(got[:, ok]).all()
    feasible = np.flatnonzero(ok)
    pick = [(int(rng.integers(0, B)), int(feasible[rng.integers(0, feasible.size)])) for _ in range(n_pairs)]
    buf = torch.full((n_pairs * T, LD), float("nan"))
    targets = torch.zeros(n_pairs, 31, dtype=torch.long)
    for n, (b, v) in enumerate(pick):
        buf[n * T:(n + 1) * T, :C] = torch.from_numpy(x[b])
        targets[n, :len(words[v])] = torch.tensor(words[v], dtype=torch.long)
    nll, acc, _ = ops.ctc_loss_fwd(buf.to(device), C, targets.to(device), T)
    assert int(acc[2]) == 0
    for (b, v), value in zip(pick, nll.cpu().numpy().astype(np.float64)):
        assert abs(float(got[b, v]) + value) <= two_roundings(value), (b, v, float(got[b, v]), -value)


# ------------------------------------------------------------------------------------------------ 9. the ABI's contract
def check_abi_contract(device):
    from ccd_amd import _lib, ops
    lib = _lib.get()
    assert lib.ccd_abi_version() >= 23 and ops.CTC_LEXICON_MAX_NBEST == 16
    st = _lib.stream()
    B, T, C, V, M = 3, 8, 12, 5, 4
    x = torch.randn(B, T, C, generator=torch.Generator().manual_seed(1)).to(device)
    table = torch.from_numpy(L.to_tensor([(1, 2), (3,), (), (4, 4, 5, 6), (11, 1)], M)).to(device)
    columns = torch.arange(V, dtype=torch.int32).to(device)
    subset = torch.zeros(B, 2, dtype=torch.int32).to(device)
    out = torch.full((B, V), 77.0, device=device)
    ok = [x, T * C, C, B, T, C, 0, table, V, M, None, None, 0, out, V, st]

    def untouched():
        return bool((out == 77.0).all())

    for i in (0, 7, 13):                                                       # a missing pointer
        bad = list(ok)
        bad[i] = None
        assert lib.ccd_ctc_lexicon_score(*bad) == -1 and untouched(), i
    for i in (1, 2, 3, 8, 9, 12, 14):                                          # a negative size or stride
        bad = list(ok)
        bad[i] = -1
        assert lib.ccd_ctc_lexicon_score(*bad) == -1 and untouched(), i
    for i, v in ((4, 0), (4, 65), (5, 1), (5, 129), (9, 0), (9, 32), (6, 2), (6, -1), (14, V - 1)):     # steps, classes, max_len, normalized, ld_out
        bad = list(ok)
        bad[i] = v
        assert lib.ccd_ctc_lexicon_score(*bad) == -2 and untouched(), (i, v)
    bad = list(ok)
    bad[10], bad[11], bad[12] = columns, subset, 2                             # columns with subset
    assert lib.ccd_ctc_lexicon_score(*bad) == -1 and untouched()
    bad = list(ok)
    bad[11], bad[12], bad[14] = subset, 2, 1                                   # ld_out below the subset's columns
    assert lib.ccd_ctc_lexicon_score(*bad) == -2 and untouched()
    assert lib.ccd_ctc_lexicon_score(None, 0, 0, 0, T, C, 0, None, V, M, None, None, 0, None, V, st) == 0 and untouched()     # batch 0
    assert lib.ccd_ctc_lexicon_score(x, T * C, C, B, T, C, 0, None, 0, M, None, None, 0, None, 0, st) == 0 and untouched()    # no words
    assert lib.ccd_ctc_lexicon_score(*ok) == 0 and not untouched()
    want = out.clone()
    swapped = torch.full((B, V), 77.0, device=device)
    with_columns = list(ok)
    with_columns[10], with_columns[13] = torch.tensor([4, 3, 2, 1, 0], dtype=torch.int32).to(device), swapped
    assert lib.ccd_ctc_lexicon_score(*with_columns) == 0 and torch.equal(swapped, want.flip(1))
    for normalized in (0, 1):                                                  # the limits themselves are inside
        big = torch.rand(1, 64, 128).to(device)
        words = torch.full((2, 31), 127, dtype=torch.long).to(device)
        res = torch.zeros(1, 2, device=device)
        assert lib.ccd_ctc_lexicon_score(big, 64 * 128, 128, 1, 64, 128, normalized, words, 2, 31, None, None, 0, res, 2, st) == 0
        assert bool(torch.isfinite(res).all())
    # ccd_ctc_lexicon_best
    index = torch.full((B, 2), 77, dtype=torch.int32, device=device)
    best = torch.full((B, 2), 77.0, device=device)
    ok = [want, V, B, V, 2, index, best, st]

    def untouched2():
        return bool((index == 77).all() and (best == 77.0).all())

    for i in (0, 5, 6):
        bad = list(ok)
        bad[i] = None
        assert lib.ccd_ctc_lexicon_best(*bad) == -1 and untouched2(), i
    for i in (1, 2, 3):
        bad = list(ok)
        bad[i] = -1
        assert lib.ccd_ctc_lexicon_best(*bad) == -1 and untouched2(), i
    for i, v in ((4, 0), (4, 17), (1, V - 1)):
        bad = list(ok)
        bad[i] = v
        assert lib.ccd_ctc_lexicon_best(*bad) == -2 and untouched2(), (i, v)
    assert lib.ccd_ctc_lexicon_best(None, V, 0, V, 2, None, None, st) == 0 and untouched2()                  # batch 0: a no-op
    assert lib.ccd_ctc_lexicon_best(*ok) == 0 and int(index.min()) >= 0 and int(index.max()) < V
    # the wrappers
    lexicon = ops.ctc_lexicon(table.cpu())
    with pytest.raises(ValueError, match="ctc_lexicon: expects a host int64 tensor"):
        ops.ctc_lexicon(table.cpu().int())
    with pytest.raises(ValueError, match="ctc_lexicon: max_len must lie in 1..31"):
        ops.ctc_lexicon(torch.zeros(2, 32, dtype=torch.long))
    with pytest.raises(TypeError, match="lexicon must come from ctc_lexicon"):
        ops.ctc_lexicon_score(x, table)
    with pytest.raises(ValueError, match="contiguous classes"):
        ops.ctc_lexicon_score(x.transpose(1, 2), lexicon)
    with pytest.raises(TypeError, match=r"^ccd_ctc_lexicon_score: scores expects float32, got float64$"):
        ops.ctc_lexicon_score(x.double(), lexicon)
    with pytest.raises(TypeError, match=r"^ccd_ctc_lexicon_score: subset expects int32, got int64$"):
        ops.ctc_lexicon_score(x, lexicon, subset=torch.zeros(B, 2, dtype=torch.long, device=device))
    with pytest.raises(ValueError, match=r"expects a contiguous subset \[3, K\]"):
        ops.ctc_lexicon_score(x, lexicon, subset=torch.zeros(B + 1, 2, dtype=torch.int32, device=device))
    with pytest.raises(RuntimeError, match="ccd_ctc_lexicon_score failed: unsupported shape"):
        ops.ctc_lexicon_score(torch.zeros(1, 65, 12, device=device), lexicon)
    with pytest.raises(ValueError, match="nbest must lie in 1..16"):
        ops.ctc_lexicon_best(want, 17)
    with pytest.raises(ValueError, match="contiguous columns"):
        ops.ctc_lexicon_best(want.t(), 1)
    assert torch.equal(ops.ctc_lexicon_score(x, lexicon), want)
    assert tuple(ops.ctc_lexicon_score(torch.zeros(0, 8, 12, device=device), lexicon).shape) == (0, V)
    empty = ops.ctc_lexicon(torch.zeros(0, 3, dtype=torch.long))
    assert tuple(ops.ctc_lexicon_score(x, empty).shape) == (B, 0)
    index, best = ops.ctc_lexicon_best(ops.ctc_lexicon_score(x, empty), 2)
    assert bool((index == -1).all()) and bool(torch.isneginf(best).all())


# ------------------------------------------------------------------------------------------------ 10. the Python surface
def lexicon_strings(conv, seed):
    """The oracle batch's lexicon as strings of the convertor's alphabet (the words with a class outside 1..90 left out)."""
    return conv.idx2str([list(w) for w in L.batch_lexicon(seed) if all(1 <= c <= 90 for c in w)])


def oracle_words(conv, probs):
    """The exact scores fp64 [B, V] of the convertor's lexicon under fp32 probabilities [B, T, C]; every sample meets the condition."""
    table = conv.lexicon.words.numpy()
    words = [tuple(row[:n].tolist()) for row, n in zip(table, conv.lexicon.lengths.tolist())]
    exact = np.stack([L.score(probs[b], words, normalized=True) for b in range(probs.shape[0])])
    for b in range(probs.shape[0]):
        assert L.min_gap(exact[b], words) >= L.MIN_GAP, b
    return words, exact


def check_convertor(device, tmp_path):
    from ccd_amd.convertor.attn import AttnConvertor
    from ccd_amd.convertor.ctc import CTCConvertor
    # set_lexicon from a list and from a file: counts, lower, <UKN>
    conv = CTCConvertor(lower=True)
    stats = conv.set_lexicon(["Hello", "hello", "wor ld", "x" * 32, "", "café", "cafè", "y" * 31])
    assert stats == {"read": 8, "kept": 5, "too_long": 1, "duplicates": 2} and conv.lexicon_stats is stats
    assert conv.lexicon_words == ["Hello", "wor ld", "", "café", "y" * 31]
    assert conv.lexicon.words[0, :6].tolist() == conv.str2idx(["hello"])[0] + [0]
    assert conv.lexicon.words[3, :5].tolist() == conv.str2idx(["caf"])[0] + [conv.unknown_idx, 0]
    assert tuple(conv.lexicon.words.shape) == (5, 31) and conv.lexicon.lengths.tolist() == [5, 6, 0, 4, 31]
    path = tmp_path / "lexicon.txt"
    path.write_text("Hello\n\nhello\r\nWorld\n" + "x" * 32 + "\n\n", encoding="utf-8")
    cased = CTCConvertor(lexicon=str(path))
    assert cased.lexicon_stats == {"read": 4, "kept": 3, "too_long": 1, "duplicates": 0} and cased.lexicon_words == ["Hello", "hello", "World"]
    cased.set_lexicon(None)
    assert cased.lexicon is None and cased.lexicon_stats is None
    with pytest.raises(KeyError):
        CTCConvertor(with_unknown=False, lexicon=["café"])
    with pytest.raises(ValueError, match="lexicon.*beam_width|beam_width.*lexicon"):
        CTCConvertor(beam_width=4, lexicon=["a"])
    with pytest.raises(NotImplementedError, match="CTC head only"):
        AttnConvertor(lexicon=["a"])
    with pytest.raises(ValueError, match="has no lexicon"):
        CTCConvertor().tensor2lexicon(torch.zeros(1, 4, 92, device=device))
    # tensor2lexicon: the oracle's three best
    probs = BK.peaked(100, True)
    conv = CTCConvertor(lexicon=lexicon_strings(CTCConvertor(), 100))
    assert conv.lexicon_stats["kept"] == len(conv.lexicon_words) >= 50
    words, exact = oracle_words(conv, probs)
    dev = torch.from_numpy(probs).to(device)
    indexes, log_probs, ids = conv.tensor2lexicon(dev, nbest=3)
    assert tuple(log_probs.shape) == tuple(ids.shape) == (9, 3) and log_probs.dtype == torch.float32 and log_probs.device.type == "cpu"
    for b in range(9):
        want = L.best(exact[b], 3)
        assert ids[b].tolist() == [k for k, _ in want] and indexes[b] == [list(words[k]) for k, _ in want], b
        assert conv.idx2str(indexes[b]) == [conv.lexicon_words[k] for k, _ in want]
        for r in range(3):
            assert abs(float(log_probs[b, r]) - want[r][1]) <= one_rounding(want[r][1])
    subset = torch.tensor([[5, -1, 2, 7]] * 9, dtype=torch.int32).to(device)
    indexes, log_probs, ids = conv.tensor2lexicon(dev, nbest=4, subset=subset)
    for b in range(9):
        want = sorted([5, 2, 7], key=lambda k: -exact[b, k])
        assert ids[b].tolist() == want + [-1] and indexes[b] == [list(words[k]) for k in want] and np.isneginf(float(log_probs[b, 3]))
    with pytest.raises(ValueError, match="nbest must lie in 1..16"):
        conv.tensor2lexicon(dev, nbest=17)
    assert conv.tensor2idx(dev) == CTCConvertor().tensor2idx(dev)


# ------------------------------------------------------------------------------------------------ 11. TextAccuracy
def oracle_strings(conv, probs):
    """The best lexicon word of every sample as the oracle scores the fp32 probabilities (numpy [B, T, C])."""
    _, exact = oracle_words(conv, probs)
    return [conv.lexicon_words[L.best(exact[b], 1)[0][0]] for b in range(probs.shape[0])]


def check_update_scores(device):
    """TextAccuracy.update_scores with a lexicon convertor: the totals of the host update() on the oracle's best lexicon strings;
    without a lexicon the records of today's greedy path, bit for bit."""
    import ctc_checks as K
    from ccd_amd import ops
    from ccd_amd.convertor.ctc import CTCConvertor
    from ccd_amd.metric.eval_acc import TextAccuracy, encode_truth
    probs = BK.peaked(101, True)
    conv = CTCConvertor(lexicon=lexicon_strings(CTCConvertor(), 101))
    strings = oracle_strings(conv, probs)
    gts = [s if b % 2 else s[:-1] + "Q" for b, s in enumerate(strings)]       # half of them right
    host = TextAccuracy()
    host.update(gts, strings)
    want = host.result()
    dev = TextAccuracy()
    dev.update_scores(torch.from_numpy(probs).to(device), gts, conv)
    got = dev.result()
    for k in ("ccr", "cwr", "ted", "ted/w", "words"):
        assert got[k] == want[k], (k, got[k], want[k])
    assert abs(got["ned"] - want["ned"]) <= 9 * 2.0 ** -52 * max(1.0, want["ned"]) and 0 < want["cwr"] < 1
    x = K.greedy_case().to(device)
    raw, norm = (torch.from_numpy(t).to(device) for t in conv.score_table())
    codes, lens = (torch.from_numpy(a).to(device) for a in encode_truth(K.GREEDY_TRUTH))
    plain = TextAccuracy().update_scores(x, list(K.GREEDY_TRUTH), CTCConvertor())
    assert torch.equal(plain, ops.text_score_ctc(x, raw, norm, codes, lens))
