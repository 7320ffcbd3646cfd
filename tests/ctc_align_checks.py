"""The checks of CTC forced alignment (kernels/ctc_align.h: ccd_ctc_align) that run on either backend: the CPU SIMT executor
(tests/test_ctc_align_sim.py) and the MI355X (tests/test_ctc_align_gpu.py).  `device` is where the tensors live.

Oracle: tests/ctc_align_np.py, the specification in fp64 numpy, itself checked against brute force over every frame path in
tests/test_ctc_align_cpu.py.  Gates:
  * frame_char and spans equal the oracle's exactly - on rows whose margin (the smallest gap between winner and runner-up over the
    decisions on the best path, the final one included) is >= 1e-9; below it a valid alignment of the word whose summed lp equals the
    oracle's score is required instead.  Every seeded row is asserted to have a margin >= 1e-6: the excluded share is zero;
  * |score - oracle| and |char_logp - oracle| <= 2^-22 max(1, |v|), the tolerance tests/ctc_lexicon_checks.py uses for fp32 scores;
  * an infeasible row: score -inf, frame_char and spans -1, char_logp 0 - exactly;
  * two runs give identical bits."""
import functools

import numpy as np
import pytest
import torch

import ctc_align_np as A
import ctc_beam_np as R
import ctc_lexicon_checks as LK

LD = 128
frames_view = LK.frames_view


def tol(v):
    return 2.0 ** -22 * max(1.0, abs(v))


def to_targets(words, max_len=None):
    max_len = max(1, max(map(len, words), default=1)) if max_len is None else max_len
    t = np.zeros((len(words), max_len), dtype=np.int64)
    for row, w in zip(t, words):
        row[:len(w)] = w
    return t


def run_align(device, x, words, normalized=False, rows=None, max_len=None):
    """x fp32 [B, T, C], words a list of tuples -> (frame_char [N, T], spans [N, Lmax, 2], char_logp [N, Lmax], score [N]) as numpy,
    through ops.ctc_align; the scores are read in place from a [B * T, 128] buffer with NaN behind column C."""
    from ccd_amd import ops
    view = frames_view(device, x)
    targets = torch.from_numpy(to_targets(words, max_len)).to(device)
    if rows is not None:
        rows = torch.as_tensor(rows, dtype=torch.int32).to(device)
    out = ops.ctc_align(view, targets, normalized=normalized, rows=rows)
    N, Lmax, T = targets.shape[0], targets.shape[1], view.shape[1]
    assert [o.dtype for o in out] == [torch.int32, torch.int32, torch.float32, torch.float32]
    assert [tuple(o.shape) for o in out] == [(N, T), (N, Lmax, 2), (N, Lmax), (N,)]
    return tuple(o.cpu().numpy() for o in out)


def compare_row(got, want, x, word, normalized, where):
    """One row: got = (frame_char [T], spans [Lmax, 2], char_logp [Lmax], score) against the oracle's Alignment (None: infeasible)."""
    fc, sp, cl, sc = got
    assert not np.isnan(cl).any() and not np.isnan(sc), where
    if want is None:
        assert sc == -np.inf and (fc == -1).all() and (sp == -1).all() and (cl == 0).all(), (where, float(sc), fc.tolist())
        return
    L = len(word)
    assert abs(float(sc) - want.score) <= tol(want.score), (where, float(sc), want.score)
    assert (sp[L:] == -1).all() and (cl[L:] == 0).all(), where
    if want.margin >= A.MIN_MARGIN:
        assert fc.tolist() == want.frame_char.tolist(), (where, fc.tolist(), want.frame_char.tolist())
        assert sp[:L].tolist() == want.spans.tolist(), (where, sp[:L].tolist(), want.spans.tolist())
        for j in range(L):
            assert abs(float(cl[j]) - want.char_logp[j]) <= tol(want.char_logp[j]), (where, j, float(cl[j]), want.char_logp[j])
    else:                                                                      # a near-tie: any alignment of that score
        assert A.valid(fc.tolist(), word), (where, fc.tolist())
        assert abs(A.path_score(x, fc.tolist(), word, normalized) - want.score) <= tol(want.score), where


# ------------------------------------------------------------------------------------------------ 1. seeded rows against the oracle
def seeded_groups(seed, n_groups, B=9):
    """n_groups batches (x fp32 [B, T, C], words, normalized): T in 1..64, C in 2..128, logits N(0, 1) * {1, 3, 8} rounded to fp32 (the
    fp32 softmax of them for normalized), word lengths 0..31 (mostly cut to what T can hold), a class == C now and then."""
    rng = np.random.default_rng(seed)
    groups = []
    for g in range(n_groups):
        T = int(rng.integers(1, 65))
        C = int(rng.integers(2, 129))
        x = np.stack([(rng.normal(0.0, 1.0, (T, C)) * (1.0, 3.0, 8.0)[int(rng.integers(0, 3))]).astype(np.float32) for _ in range(B)])
        words = []
        for _ in range(B):
            L = int(rng.integers(0, 32))
            if rng.random() < 0.8:
                L = min(L, T)
            words.append(tuple(int(c) for c in rng.integers(1, C + (1 if rng.random() < 0.05 else 0), L)))
        normalized = bool(g & 1)
        groups.append((R.softmax32(x) if normalized else x, words, normalized))
    return groups


@functools.lru_cache(maxsize=None)
def seeded_oracle(seed, n_groups):
    """(groups, the oracle's Alignment of every row) computed once per process; every feasible row meets the margin condition."""
    groups = seeded_groups(seed, n_groups)
    want = [[A.align(x[b], words[b], normalized) for b in range(x.shape[0])] for x, words, normalized in groups]
    margins = [a.margin for row in want for a in row if a is not None]
    assert len(margins) >= 5 * n_groups and min(margins) >= A.SEEDED_MARGIN, (len(margins), min(margins))
    return groups, want


def check_seeded(device, n_groups, seed=0):
    groups, want = seeded_oracle(seed, n_groups)
    seen = [0, 0]
    for g, ((x, words, normalized), exact) in enumerate(zip(groups, want)):
        got = run_align(device, x, words, normalized, max_len=31 if g % 3 == 0 else None)
        for b in range(x.shape[0]):
            compare_row(tuple(o[b] for o in got), exact[b], x[b], words[b], normalized, ("seeded", g, b))
            seen[exact[b] is None] += 1
        if g < 2:
            again = run_align(device, x, words, normalized, max_len=31 if g % 3 == 0 else None)
            assert all(a.tobytes() == c.tobytes() for a, c in zip(got, again)), g
    print(f"{seen[0]} feasible and {seen[1]} infeasible rows")
    assert seen[1] >= 1


# ------------------------------------------------------------------------------------------------ 2. seams and limits
def _both(x):
    return ((x, False), (R.softmax32(x), True))


def check_limits(device):
    """T = 64 with L = 31; C = 128 with labels >= 64; T = 1; L = 0; adjacent repeats at exactly L + repeats = T and at T - 1; a label
    == classes and a negative label."""
    rng = np.random.default_rng(11)
    big = rng.normal(0.0, 3.0, (5, 64, 128)).astype(np.float32)
    words = [tuple(int(c) for c in rng.integers(64, 128, 31)), (127,) * 31, tuple(127 if i & 1 else 64 for i in range(31)), (), (100, 5, 64)]
    for x, normalized in _both(big):
        got = run_align(device, x, words, normalized)
        for b, w in enumerate(words):
            exact = A.align(x[b], w, normalized)
            assert exact is not None and exact.margin >= A.SEEDED_MARGIN
            compare_row(tuple(o[b] for o in got), exact, x[b], w, normalized, ("big", normalized, b))
    for x, normalized in _both(rng.normal(0.0, 2.0, (3, 1, 92)).astype(np.float32)):           # T = 1
        words = [(), (40,), (40, 41)]
        got = run_align(device, x, words, normalized)
        exact = [A.align(x[b], w, normalized) for b, w in enumerate(words)]
        assert exact[0] is not None and exact[1] is not None and exact[2] is None
        assert exact[1].frame_char.tolist() == [0] and exact[0].frame_char.tolist() == [-1]
        for b, w in enumerate(words):
            compare_row(tuple(o[b] for o in got), exact[b], x[b], w, normalized, ("T=1", normalized, b))
    # L + repeats == T is the tightest fit (one alignment); one frame fewer has none
    tight = (7, 7, 3, 3, 3, 9)                                                 # L = 6, 3 repeats
    for T, fits in ((9, True), (8, False), (10, True)):
        for x, normalized in _both(rng.normal(0.0, 2.0, (2, T, 12)).astype(np.float32)):
            words = [tight, (1, 2)]
            got = run_align(device, x, words, normalized)
            exact = [A.align(x[b], w, normalized) for b, w in enumerate(words)]
            assert (exact[0] is not None) == fits and exact[1] is not None
            if T == 9:
                assert exact[0].frame_char.tolist() == [0, -1, 1, 2, -1, 3, -1, 4, 5]
            for b, w in enumerate(words):
                compare_row(tuple(o[b] for o in got), exact[b], x[b], w, normalized, ("tight", T, normalized, b))
    # labels outside [1, classes): infeasible, never an index; the neighbours are untouched
    x = rng.normal(0.0, 2.0, (4, 8, 12)).astype(np.float32)
    words = [(3, 12, 4), (3, 4), (5, -2), (11,)]
    got = run_align(device, x, words)
    for b, w in enumerate(words):
        exact = A.align(x[b], w)
        assert (exact is None) == (b in (0, 2))
        compare_row(tuple(o[b] for o in got), exact, x[b], w, False, ("label", b))
    huge = to_targets(words)
    huge[0, 1], huge[2, 1] = 2 ** 40, -2 ** 40
    from ccd_amd import ops
    out = ops.ctc_align(frames_view(device, x), torch.from_numpy(huge).to(device))
    assert np.isneginf(out[3].cpu().numpy()).tolist() == [True, False, True, False]


def check_masks(device):
    """-inf / zero-probability entries: a masked column forces a detour, a masked frame or class leaves no finite alignment; no NaN."""
    base = np.stack([R.small_case(6, 4, seed=s) for s in (21, 22, 23, 24)])
    base[0, :, 1] = -20.0
    base[0, 2, 1] = base[0, 3, 1] = 40.0                                       # class 1 would sit on frames 2, 3 ...
    base[1] = base[0]
    base[1, 2, 1] = base[1, 3, 1] = -np.inf                                    # ... but is masked there: a detour
    base[2, 4, :] = -np.inf                                                    # a frame without any class
    base[3, :, 2] = -np.inf                                                    # class 2 never
    words = [(1,), (1,), (1,), (1, 2)]
    for normalized in (False, True):
        x = R.softmax32(base) if normalized else base.copy()
        if normalized:
            x[2, 4, :] = 0.0
        got = run_align(device, x, words, normalized)
        exact = [A.align(x[b], w, normalized) for b, w in enumerate(words)]
        assert exact[0] is not None and exact[1] is not None and exact[2] is None and exact[3] is None
        assert exact[0].spans.tolist() == [[2, 3]] and not set(exact[1].frame_char[2:4].tolist()) & {0}
        for b, w in enumerate(words):
            assert exact[b] is None or exact[b].margin >= A.SEEDED_MARGIN
            compare_row(tuple(o[b] for o in got), exact[b], x[b], w, normalized, ("mask", normalized, b))
        blank_only = run_align(device, x[3:], [()], normalized)
        compare_row(tuple(o[0] for o in blank_only), A.align(x[3], (), normalized), x[3], (), normalized, ("mask", normalized, "empty"))


def check_uniform(device):
    """Uniform frames: every alignment ties, the tie rule alone decides.  `ab` over five frames is a b _ _ _."""
    for normalized in (False, True):
        for T, C, word in ((5, 3, (1, 2)), (5, 3, ()), (7, 4, (2, 2, 3)), (64, 128, (127,) * 31), (8, 5, (1, 2, 3, 4, 1, 2))):
            x = np.full((1, T, C), 0.25 if normalized else 0.0, dtype=np.float32)
            exact = A.align(x[0], word, normalized)
            assert exact.margin == 0.0 or not word
            got = run_align(device, x, [word], normalized)
            assert got[0][0].tolist() == exact.frame_char.tolist(), (T, C, word, got[0][0].tolist())
            assert got[1][0, :len(word)].tolist() == exact.spans.tolist()
            assert abs(float(got[3][0]) - exact.score) <= tol(exact.score)
            if word == (1, 2):
                assert got[0][0].tolist() == [0, 1, -1, -1, -1]


# ------------------------------------------------------------------------------------------------ 3. rows
def check_rows(device):
    """8 targets per sample through `rows`: the bits of aligning them against replicated scores; a bad entry is infeasible and disturbs
    nothing."""
    rng = np.random.default_rng(5)
    B, T, C, K = 3, 20, 30, 8
    for normalized in (False, True):
        x = rng.normal(0.0, 3.0, (B, T, C)).astype(np.float32)
        x = R.softmax32(x) if normalized else x
        words = [tuple(int(c) for c in rng.integers(1, C, int(rng.integers(0, 12)))) for _ in range(B * K)]
        rows = np.repeat(np.arange(B), K).astype(np.int32)
        got = run_align(device, x, words, normalized, rows=rows, max_len=12)
        want = run_align(device, np.repeat(x, K, axis=0), words, normalized, max_len=12)
        assert all(a.tobytes() == c.tobytes() for a, c in zip(got, want)) and np.isfinite(got[3]).all()
        rows[[1, 10, 23]] = [-1, B, 2 ** 31 - 1]
        rows[5] = 2                                                            # out of order: any sample
        bad = run_align(device, x, words, normalized, rows=rows, max_len=12)
        for n in range(B * K):
            if n in (1, 10, 23):
                compare_row(tuple(o[n] for o in bad), None, None, words[n], normalized, ("rows", n))
            elif n == 5:
                compare_row(tuple(o[n] for o in bad), A.align(x[2], words[n], normalized), x[2], words[n], normalized, ("rows", n))
            else:
                assert all(o[n].tobytes() == w[n].tobytes() for o, w in zip(bad, got)), n


# ------------------------------------------------------------------------------------------------ 4. against the other kernels
def check_against_loss(device, n_groups, seed=0):
    """max <= sum: score <= -nll of ccd_ctc_loss_fwd for the same row, up to the tolerance (logits: the loss takes nothing else)."""
    from ccd_amd import ops
    groups, want = seeded_oracle(seed, n_groups)
    n, closest = 0, np.inf
    for (x, words, normalized), exact in zip(groups, want):
        if normalized:
            continue
        B, T, C = x.shape
        buf = torch.full((B * T, LD), float("nan"))
        buf[:, :C] = torch.from_numpy(x.reshape(B * T, C))
        targets = torch.from_numpy(to_targets(words, 31)).to(device)
        nll, acc, _ = ops.ctc_loss_fwd(buf.to(device), C, targets, T)
        nll = nll.cpu().numpy().astype(np.float64)
        score = run_align(device, x, words, False, max_len=31)[3]
        assert int(acc[2]) == sum(a is None for a in exact)
        for b in range(B):
            if exact[b] is not None:
                assert float(score[b]) <= -nll[b] + tol(nll[b]), (b, float(score[b]), -nll[b])
                closest = min(closest, -nll[b] - float(score[b]))
                n += 1
    print(f"{n} rows; smallest log p(word) - score {closest:.3e}")
    assert n >= 2 * n_groups


def check_single_alignment_bits(device):
    """A word with exactly one alignment (L + adjacent repeats == T): the sum over alignments IS the best alignment, added in the same
    frame order, so ccd_ctc_lexicon_score and ccd_ctc_align return the same bits - if the two kernels form the same lp."""
    from ccd_amd import ops
    rng = np.random.default_rng(17)
    cases = [(9, 12, (7, 7, 3, 3, 3, 9)), (20, 92, tuple(int(c) for c in 1 + (np.arange(20) * 37) % 91)), (1, 5, (4,)),
             (61, 128, (127,) * 31), (31, 128, tuple(127 - (i & 1) for i in range(31)))]
    for T, C, word in cases:
        assert len(word) + sum(a == b for a, b in zip(word, word[1:])) == T
        for scale in (1.0, 8.0):
            for x, normalized in _both((rng.normal(0.0, 1.0, (5, T, C)) * scale).astype(np.float32)):
                view = frames_view(device, x)
                lexicon = ops.ctc_lexicon(torch.from_numpy(to_targets([word])))
                summed = ops.ctc_lexicon_score(view, lexicon, normalized=normalized)[:, 0].cpu().numpy()
                best = run_align(device, x, [word] * 5, normalized)[3]
                assert np.isfinite(best).all() and best.tobytes() == summed.tobytes(), (T, C, normalized, best.tolist(), summed.tolist())


def check_against_greedy(device, n_groups, seed=0):
    """The word ccd_ctc_greedy returns, aligned: the per-frame arg-max path - a character exactly where the arg-max is not the blank,
    score = the sum of the per-frame maxima of lp.  Rows whose greedy word has more than 31 characters are cut and left out."""
    from ccd_amd import ops
    groups, _ = seeded_oracle(seed, n_groups)
    n = 0
    for x, _, normalized in groups:
        view = frames_view(device, x)
        path, length, _ = ops.ctc_greedy(view)
        targets = ops.ctc_paths_to_targets(path)
        assert targets.dtype == torch.int64 and tuple(targets.shape) == (x.shape[0], min(x.shape[1], 31))
        fc, _, _, score = (o.cpu().numpy() for o in ops.ctc_align(view, targets, normalized=normalized))
        for b in range(x.shape[0]):
            if int(length[b]) > 31:
                continue
            lp = R.log_probs(x[b], normalized)
            top = np.sort(lp, axis=1)
            assert (top[:, -1] - top[:, -2]).min() >= A.SEEDED_MARGIN if x.shape[2] > 1 else True
            best = lp.argmax(axis=1)
            assert ((fc[b] >= 0) == (best != 0)).all(), (b, fc[b].tolist(), best.tolist())
            total = 0.0
            for t in range(lp.shape[0]):
                total += lp[t, best[t]]
            assert abs(float(score[b]) - total) <= tol(total), (b, float(score[b]), total)
            n += 1
    print(f"{n} greedy words aligned")
    assert n >= 3 * n_groups


# ------------------------------------------------------------------------------------------------ 5. the ABI's contract
def check_abi_contract(device):
    from ccd_amd import _lib, ops
    lib = _lib.get()
    assert lib.ccd_abi_version() >= 25
    st = _lib.stream()
    B, T, C, M = 3, 8, 12, 4
    x = torch.randn(B, T, C, generator=torch.Generator().manual_seed(1)).to(device)
    targets = torch.from_numpy(to_targets([(1, 2), (3,), (4, 4, 5, 6)], M)).to(device)
    rows = torch.tensor([2, 0, 1], dtype=torch.int32).to(device)
    fc = torch.full((B, T), 77, dtype=torch.int32, device=device)
    sp = torch.full((B, M, 2), 77, dtype=torch.int32, device=device)
    cl = torch.full((B, M), 77.0, device=device)
    sc = torch.full((B,), 77.0, device=device)
    ok = [x, T * C, C, B, T, C, 0, targets, B, M, None, fc, sp, cl, sc, st]

    def untouched():
        return bool((fc == 77).all() and (sp == 77).all() and (cl == 77.0).all() and (sc == 77.0).all())

    for i in (0, 7, 11, 12, 13, 14):                                           # a missing pointer
        bad = list(ok)
        bad[i] = None
        assert lib.ccd_ctc_align(*bad) == -1 and untouched(), i
    for i in (1, 2, 3, 8, 9):                                                  # a negative size or stride
        bad = list(ok)
        bad[i] = -1
        assert lib.ccd_ctc_align(*bad) == -1 and untouched(), i
    bad = list(ok)
    bad[8] = B - 1                                                             # no rows: one target per sample
    assert lib.ccd_ctc_align(*bad) == -1 and untouched()
    for i, v in ((4, 0), (4, 65), (4, -1), (5, 0), (5, 129), (9, 0), (9, 32), (6, 2), (6, -1)):      # steps, classes, max_len, normalized
        bad = list(ok)
        bad[i] = v
        assert lib.ccd_ctc_align(*bad) == -2 and untouched(), (i, v)
    assert lib.ccd_ctc_align(x, T * C, C, B, T, C, 0, None, 0, M, None, None, None, None, None, st) == 0 and untouched()      # n_rows 0
    assert lib.ccd_ctc_align(*ok) == 0 and not untouched()
    assert bool(torch.isfinite(sc).all()) and int(fc.min()) >= -1 and int(fc.max()) <= 3
    with_rows = list(ok)
    with_rows[10] = rows
    first = sc.clone()
    assert lib.ccd_ctc_align(*with_rows) == 0 and not torch.equal(sc, first)
    for normalized in (0, 1):                                                  # the limits themselves are inside
        big = torch.rand(1, 64, 128).to(device) + 0.01
        words = torch.full((1, 31), 127, dtype=torch.long).to(device)
        out = [torch.zeros(1, 64, dtype=torch.int32, device=device), torch.zeros(1, 31, 2, dtype=torch.int32, device=device),
               torch.zeros(1, 31, device=device), torch.zeros(1, device=device)]
        assert lib.ccd_ctc_align(big, 64 * 128, 128, 1, 64, 128, normalized, words, 1, 31, None, *out, st) == 0
        assert bool(torch.isfinite(out[3]).all()) and 60 <= int(out[1].max()) <= 63       # (31 + 30 repeats of 64 frames)
    one = torch.rand(2, 4, 1).to(device)                                       # classes = 1: nothing but the blank
    out = ops.ctc_align(one, torch.tensor([[0], [1]]).to(device), normalized=True)
    assert out[3].cpu().tolist() == [0.0, -np.inf] and bool((out[0] == -1).all())
    # the wrappers
    with pytest.raises(ValueError, match="contiguous classes"):
        ops.ctc_align(x.transpose(1, 2), targets)
    with pytest.raises(TypeError, match=r"^ccd_ctc_align: scores expects float32, got float64$"):
        ops.ctc_align(x.double(), targets)
    with pytest.raises(TypeError, match=r"^ccd_ctc_align: targets expects int64, got int32$"):
        ops.ctc_align(x, targets.int())
    with pytest.raises(TypeError, match=r"^ccd_ctc_align: rows expects int32, got int64$"):
        ops.ctc_align(x, targets, rows=rows.long())
    with pytest.raises(ValueError, match="one target per sample"):
        ops.ctc_align(x, targets[:2])
    with pytest.raises(ValueError, match=r"contiguous rows \[3\]"):
        ops.ctc_align(x, targets, rows=rows[:2])
    with pytest.raises(ValueError, match="Lmax must lie in 1..31"):
        ops.ctc_align(x, torch.zeros(B, 32, dtype=torch.long, device=device))
    with pytest.raises(RuntimeError, match="ccd_ctc_align failed: unsupported shape"):
        ops.ctc_align(torch.zeros(1, 65, 12, device=device), targets[:1])
    assert torch.equal(ops.ctc_align(x, targets, rows=rows)[3], sc)
    empty = ops.ctc_align(x, targets[:0], rows=rows[:0])
    assert [tuple(o.shape) for o in empty] == [(0, T), (0, M, 2), (0, M), (0,)]
    paths = torch.tensor([[3, 4, -1, -1], [-1, -1, -1, -1]], dtype=torch.int32).to(device)
    assert ops.ctc_paths_to_targets(paths).cpu().tolist() == [[3, 4, 0, 0], [0, 0, 0, 0]]
    assert tuple(ops.ctc_paths_to_targets(torch.full((2, 3, 40), -1, dtype=torch.int32).to(device)).shape) == (2, 3, 31)
    with pytest.raises(ValueError, match="expects int32 paths"):
        ops.ctc_paths_to_targets(paths.long())


# ------------------------------------------------------------------------------------------------ 6. the Python surface
def _words_of(conv, res):
    """The strings of the targets of a tensor2align result (None where the row holds no word)."""
    targets, rows = res["targets"].cpu().numpy(), res["rows"].cpu().numpy()
    return [None if r < 0 else conv.idx2str([[int(c) for c in row[:int(np.argmin(row != 0)) if (row == 0).any() else len(row)]]])[0]
            for row, r in zip(targets, rows)]


def check_result(res, probs, normalized=True):
    """Every row of a tensor2align result against the oracle on the host copy of the scores."""
    out = {k: v.cpu().numpy() for k, v in res.items()}
    n = 0
    for i, r in enumerate(out["rows"]):
        row = out["targets"][i]
        word = tuple(int(c) for c in row[:int(np.argmin(row != 0)) if (row == 0).any() else len(row)])
        exact = None if r < 0 else A.align(probs[r], word, normalized)
        assert exact is None or exact.margin >= A.MIN_MARGIN
        compare_row((out["frame_char"][i], out["spans"][i], out["char_logp"][i], out["score"][i]), exact,
                    None if r < 0 else probs[r], word, normalized, ("result", i))
        n += exact is not None
    return n


def check_convertor(device):
    import ctc_beam_checks as BK
    from ccd_amd.convertor.attn import AttnConvertor
    from ccd_amd.convertor.char_lm import CharNGram
    from ccd_amd.convertor.ctc import CTCConvertor
    probs = BK.peaked(100, True)
    dev = torch.from_numpy(probs).to(device)
    N, T = probs.shape[:2]
    plain = CTCConvertor()
    # greedy: the word tensor2idx decodes
    res = plain.tensor2align(dev)
    assert set(res) == {"targets", "frame_char", "spans", "char_logp", "score", "rows"} and res["rows"].cpu().tolist() == list(range(N))
    assert _words_of(plain, res) == plain.idx2str(plain.tensor2idx(dev)[0])
    assert check_result(res, probs) == N
    # beam of 4, the three best: tensor2nbest's words by rank
    beam = CTCConvertor(beam_width=4)
    res = beam.tensor2align(dev, nbest=3)
    want = [beam.idx2str(w) for w in beam.tensor2nbest(dev, nbest=3)[0]]
    assert all(len(w) == 3 for w in want) and _words_of(beam, res) == [s for w in want for s in w]
    assert res["rows"].cpu().tolist() == [i for i in range(N) for _ in range(3)] and check_result(res, probs) == 3 * N
    # lexicon, the two best
    lex = CTCConvertor(lexicon=LK.lexicon_strings(CTCConvertor(), 100))
    res = lex.tensor2align(dev, nbest=2)
    want = [lex.idx2str(w) for w in lex.tensor2lexicon(dev, nbest=2)[0]]
    assert all(len(w) == 2 for w in want) and _words_of(lex, res) == [s for w in want for s in w] and check_result(res, probs) == 2 * N
    # language model
    lm = CTCConvertor(beam_width=4, lm=CharNGram.from_words(plain, ["hello", "world", "help", "hold", "word"], order=2), lm_weight=0.5)
    res = lm.tensor2align(dev, nbest=2)
    want = [lm.idx2str(w) for w in lm.tensor2nbest(dev, nbest=2)[0]]
    got = _words_of(lm, res)
    assert [[s for s in got[2 * i:2 * i + 2] if s is not None] for i in range(N)] == want and check_result(res, probs) == sum(map(len, want))
    # given transcriptions
    words = ["hello", "", "Q", "a" * 40, "world", "x", "zz", "CTC", "1234"]
    res = plain.tensor2align(dev, words=words)
    assert tuple(res["targets"].shape) == (N, 25) and _words_of(plain, res) == [w[:25] for w in words] and check_result(res, probs) >= N - 1
    logits = BK.peaked(100, False)
    res = plain.tensor2align(torch.from_numpy(logits).to(device), words=words, normalized=False)
    assert check_result(res, logits, normalized=False) >= N - 1
    with pytest.raises(ValueError, match="one string per sample"):
        plain.tensor2align(dev, words=words[:3])
    with pytest.raises(ValueError, match="nbest must lie in 1..beam_width = 4"):
        beam.tensor2align(dev, nbest=5)
    with pytest.raises(ValueError, match="one word per sample"):
        plain.tensor2align(dev, nbest=2)
    # tensor2chars
    for conv, nbest in ((plain, 1), (beam, 3), (lex, 2)):
        for boxes in ("emission", "cells"):
            chars = conv.tensor2chars(dev, nbest=nbest, image_width=128, boxes=boxes)
            res = {k: v.cpu().numpy() for k, v in conv.tensor2align(dev, nbest=nbest).items()}
            assert len(chars) == N and all(len(c) == nbest for c in chars)
            for i, entries in enumerate(chars):
                for r, (word, log_prob, cs) in enumerate(entries):
                    n = i * nbest + r
                    assert word == _words_of(conv, {k: torch.from_numpy(v[n:n + 1]) for k, v in res.items()})[0]
                    assert log_prob == float(res["score"][n]) and "".join(c[0] for c in cs) == word
                    edge = 0.0
                    for j, (_, x0, x1, first, last, conf) in enumerate(cs):
                        assert 0.0 <= x0 < x1 <= 128.0 and edge <= x0 and 0.0 < conf <= 1.0
                        assert [first, last] == res["spans"][n, j].tolist()
                        if boxes == "emission":
                            assert x0 == first * 128.0 / T and x1 == (last + 1) * 128.0 / T
                            assert abs(conf - np.exp(float(res["char_logp"][n, j]) / (last - first + 1))) <= 1e-12
                        else:
                            assert x0 == edge and x0 <= first * 128.0 / T and x1 >= (last + 1) * 128.0 / T
                        edge = x1
                    assert boxes == "emission" or not cs or edge == 128.0      # the cells tile the width
    assert plain.tensor2chars(dev, words=words)[3] == [] and plain.tensor2chars(dev, words=words)[1] == [("", pytest.approx(
        float(np.log(probs[1, :, 0].astype(np.float64)).sum()), abs=1e-3), [])]
    with pytest.raises(ValueError, match="boxes must be"):
        plain.tensor2chars(dev, boxes="ink")
    attn = AttnConvertor()
    for method in (attn.tensor2align, attn.tensor2chars):
        with pytest.raises(NotImplementedError, match="CTC head only"):
            method(dev)
