"""The checks of CTC prefix beam search fused with a character n-gram language model (kernels/ctc_beam.h: ctc_beam_kernel<true>,
ccd_ctc_beam_search_lm) that run on either backend: the CPU SIMT executor (tests/test_ctc_beam_lm_sim.py) and the MI355X
(tests/test_ctc_beam_lm_gpu.py).  `device` is where the tensors live.

Oracle: tests/ctc_beam_lm_np.py, the specification in fp64 numpy, itself checked against brute force in tests/test_ctc_beam_lm_cpu.py.
Gates, those of tests/ctc_beam_checks.py:
  * paths, lengths and the slot order equal the oracle's - on inputs where the oracle's own smallest gap between neighbouring
    candidate scores (the eos re-rank included) is >= 1e-9, asserted for every sample;
  * |score - oracle| <= 2^-23 |oracle| + 1e-9: the one rounding to fp32;
  * weight 0, bonus 0 and a finite table: the three outputs of ops.ctc_beam_search, byte for byte;
  * two runs give identical bits."""
import functools

import numpy as np
import pytest
import torch

import ctc_beam_checks as B
import ctc_beam_lm_np as L
import ctc_beam_np as R

LD = 128
SEEDS = B.SEEDS                       # the peaked batches of the plain beam's checks
WIDTHS = B.WIDTHS
ORDERS = (2, 3)
TABLE_SEEDS = (42, 43)
WEIGHT, BONUS = 0.5, 0.8              # of the oracle comparisons
LONG_SEED = 103                       # T = 64, C = 128: the gap condition holds (asserted in oracle())


def run_lm(device, x, W, table, order, weight=1.0, bonus=0.0, eos=False, normalized=False):
    """x fp32 [B, T, C], table fp32 numpy [C^(order-1), C] -> (paths [B, W, T], lengths [B, W], scores [B, W]) as numpy; the scores
    are read in place from a [B * T, 128] buffer with NaN behind column C, as ctc_beam_checks.run_beam hands them over."""
    from ccd_amd import ops
    x = torch.as_tensor(x)
    n, T, C = x.shape
    buf = torch.full((n * T, LD), float("nan"))
    buf[:, :C] = x.reshape(n * T, C)
    view = buf.to(device).view(n, T, LD)[:, :, :C]
    lm = table if isinstance(table, ops.CTCCharLM) else ops.ctc_char_lm(torch.from_numpy(np.ascontiguousarray(table)), order)
    paths, lengths, scores = ops.ctc_beam_search_lm(view, W, lm, weight, bonus, eos, normalized=normalized)
    assert paths.dtype == torch.int32 and lengths.dtype == torch.int32 and scores.dtype == torch.float32
    assert tuple(paths.shape) == (n, W, T) and tuple(lengths.shape) == (n, W) and tuple(scores.shape) == (n, W)
    return paths.cpu().numpy(), lengths.cpu().numpy(), scores.cpu().numpy()


@functools.lru_cache(maxsize=None)
def table_of(seed, C, order):
    return L.synthetic_table(seed, C, order)


@functools.lru_cache(maxsize=None)
def oracle(seed, W, normalized, order, table_seed, n=9, T=32, C=92):
    """The oracle's hypotheses of every sample of a peaked batch at WEIGHT, BONUS and eos on, computed once per process; the gap
    condition holds for each."""
    x = B.peaked(seed, normalized, n, T, C)
    table = table_of(table_seed, C, order)
    out = []
    for b in range(n):
        hyps, gap = L.beam_search_lm(x[b], W, table, order, WEIGHT, BONUS, True, normalized)
        assert gap >= R.MIN_GAP, (seed, W, normalized, order, table_seed, b, gap)
        out.append(hyps)
    return out


# ------------------------------------------------------------------------------------------------ against brute force
def exact_words(x, normalized, table, order, weight, bonus, eos):
    """Every word with its exact fused score, brute force + word_term, by (score descending, word); -inf words left out."""
    words = [(w, s + L.word_term(w, table, order, weight, bonus, eos)) for w, s in R.brute_force(x, normalized)]
    return sorted([e for e in words if e[1] > -np.inf], key=lambda e: (-e[1], e[0]))


def check_exhaustive(device):
    """Every word fits the beam: the hypotheses are all the words the table allows, in the order of their exact fused scores - with a
    finite table and with the column of the last class at -inf."""
    for T, C in R.EXHAUSTIVE:
        for normalized in (False, True):
            x = R.small_case(T, C, seed=10 * T + C)
            x = R.softmax32(x) if normalized else x
            for order in (1, 2, 3):
                for table in (L.synthetic_table(40 + order, C, order), L.masked_table(40 + order, C, order, (C - 1,))):
                    for eos in (False, True):
                        exact = exact_words(x, normalized, table, order, 0.7, 0.35, eos)
                        assert len(exact) >= 1 and L.beam_search_lm(x, 16, table, order, 0.7, 0.35, eos, normalized)[1] >= R.MIN_GAP
                        paths, lengths, scores = run_lm(device, x[None], 16, table, order, 0.7, 0.35, eos, normalized)
                        B.compare((paths[0], lengths[0], scores[0]), exact, 16, T, (T, C, normalized, order, eos))
                        if np.isneginf(table).any():
                            assert not (paths[0] == C - 1).any()


# ------------------------------------------------------------------------------------------------ against the oracle
def check_oracle(device, seeds=SEEDS):
    """B = 9 (a partial last workgroup), T = 32, C = 92, W in {1, 4, 16}, logits and the fp32 softmax, orders 2 and 3, two tables."""
    for seed in seeds:
        for normalized in (False, True):
            x = B.peaked(seed, normalized)
            for order in ORDERS:
                for table_seed in TABLE_SEEDS:
                    from ccd_amd import ops
                    lm = ops.ctc_char_lm(torch.from_numpy(table_of(table_seed, 92, order)), order)
                    for W in WIDTHS:
                        want = oracle(seed, W, normalized, order, table_seed)
                        got = run_lm(device, x, W, lm, order, WEIGHT, BONUS, True, normalized)
                        for b in range(x.shape[0]):
                            B.compare(tuple(a[b] for a in got), want[b], W, 32, (seed, normalized, order, table_seed, W, b))
                        if W == 16 and seed == seeds[0] and table_seed == TABLE_SEEDS[0]:
                            again = run_lm(device, x, W, lm, order, WEIGHT, BONUS, True, normalized)
                            assert all(a.tobytes() == c.tobytes() for a, c in zip(got, again))


def check_oracle_long(device):
    """T = 64 with C = 128 at order 3, the limits of the ABI (a table of 8.4 MB, full LDS rows), at W = 16 on one batch of 5."""
    for normalized in (False, True):
        x = B.peaked(LONG_SEED, normalized, 5, 64, 128)
        want = oracle(LONG_SEED, 16, normalized, 3, TABLE_SEEDS[0], 5, 64, 128)
        got = run_lm(device, x, 16, table_of(TABLE_SEEDS[0], 128, 3), 3, WEIGHT, BONUS, True, normalized)
        for b in range(5):
            B.compare(tuple(a[b] for a in got), want[b], 16, 64, ("long", normalized, b))


# ------------------------------------------------------------------------------------------------ weight 0
def check_weight_zero(device):
    """Weight 0, bonus 0 and a finite table: ops.ctc_beam_search's three outputs, byte for byte, with and without eos."""
    for normalized in (False, True):
        x = B.peaked(100, normalized)
        for W in (16, 1):
            plain = B.run_beam(device, x, W, normalized)
            for order in (1, 2, 3):
                for eos in (False, True):
                    got = run_lm(device, x, W, table_of(42, 92, order), order, 0.0, 0.0, eos, normalized)
                    assert all(a.tobytes() == c.tobytes() for a, c in zip(got, plain)), (normalized, W, order, eos)


# ------------------------------------------------------------------------------------------------ merges
def merge_case():
    """The frames of ctc_beam_checks.tie_case - the bit-identical columns of classes 2 and 4 - with a table that tells the twins
    apart; at W = 8 words are merged whose absorbed extension carries a g far from 0."""
    table = L.synthetic_table(44, 6, 2)
    table[:, 4] -= np.float32(2.0)
    return B.tie_case(), table


def check_merge(device):
    x, table = merge_case()
    for W in (4, 8, 16):
        want, gap = L.beam_search_lm(x, W, table, 2, 1.0, 0.25)
        wrong, _ = L.beam_search_lm(x, W, table, 2, 1.0, 0.25, merge_lm=False)
        assert gap >= R.MIN_GAP
        # the case shows the mistake: without g in the merged mass a word or a score is off by far more than the tolerance
        assert [w for w, _ in wrong] != [w for w, _ in want] or \
            max(abs(a[1] - c[1]) for a, c in zip(want, wrong)) > 1e3 * max(B.one_rounding(a[1]) for a in want), W
        paths, lengths, scores = run_lm(device, x[None], W, table, 2, 1.0, 0.25)
        B.compare((paths[0], lengths[0], scores[0]), want, W, 6, ("merge", W))
    words = [w for w, _ in L.beam_search_lm(x, 16, table, 2, 1.0, 0.25)[0]]
    plain = [w for w, _ in R.beam_search(x, 16, ties=True)[0]]
    assert words != plain                                                    # the table separates the twins


# ------------------------------------------------------------------------------------------------ the end of the word
def eos_case():
    """T = 5, C = 4 at order 2: the end column makes the context of the plain best word the least likely to end a word."""
    x = R.small_case(5, 4, seed=6)
    first = R.beam_search(x, 16)[0][0][0]
    table = L.synthetic_table(45, 4, 2)
    table[:, 0] = np.float32(-0.5)
    table[L.row_of(first, 2, 4), 0] = np.float32(-9.0)
    return x, table, first


def check_eos(device):
    x, table, first = eos_case()
    off, gap0 = L.beam_search_lm(x, 16, table, 2, 1.0, 0.0, False)
    on, gap1 = L.beam_search_lm(x, 16, table, 2, 1.0, 0.0, True)
    assert min(gap0, gap1) >= R.MIN_GAP and off[0][0] != on[0][0] and len(on) == len(off)      # the re-rank changes rank 0
    for eos, want in ((False, off), (True, on)):
        paths, lengths, scores = run_lm(device, x[None], 16, table, 2, 1.0, 0.0, eos)
        B.compare((paths[0], lengths[0], scores[0]), want, 16, 5, ("eos", eos))
    # a -inf end column: the words behind that context are no hypotheses, their slots move to the end and are unused
    masked = table.copy()
    masked[L.row_of(on[0][0], 2, 4), 0] = -np.inf
    want, gap = L.beam_search_lm(x, 16, masked, 2, 1.0, 0.0, True)
    gone = [w for w, _ in on if L.row_of(w, 2, 4) == L.row_of(on[0][0], 2, 4)]
    assert gap >= R.MIN_GAP and gone and len(want) == len(on) - len(gone) and not set(gone) & {w for w, _ in want}
    paths, lengths, scores = run_lm(device, x[None], 16, masked, 2, 1.0, 0.0, True)
    B.compare((paths[0], lengths[0], scores[0]), want, 16, 5, "eos -inf")
    assert (lengths[0, len(want):] == -1).all() and np.isneginf(scores[0, len(want):]).all() and (paths[0, len(want):] == -1).all()
    # with W = 2 the emptied slot is inside the beam: the -inf term did not steer the pruning
    want2, gap2 = L.beam_search_lm(x, 2, masked, 2, 1.0, 0.0, True)
    assert gap2 >= R.MIN_GAP
    paths, lengths, scores = run_lm(device, x[None], 2, masked, 2, 1.0, 0.0, True)
    B.compare((paths[0], lengths[0], scores[0]), want2, 2, 5, "eos -inf, W = 2")


# ------------------------------------------------------------------------------------------------ a character set
def check_charset(device):
    """A hard mask: weight 0, bonus 0 and -inf in the columns of two classes alone - the two the plain beam decodes most often.
    Neither appears in any path; every other score is a plain CTC score of the kept alignments."""
    x = B.peaked(100, False)
    plain = B.run_beam(device, x, 4)[0]
    counts = np.bincount(plain[plain > 0].ravel(), minlength=92)
    banned = tuple(int(c) for c in np.argsort(-counts, kind="stable")[:2])
    assert counts[list(banned)].min() >= 1
    for order in (1, 2):
        table = np.zeros((92 ** (order - 1), 92), dtype=np.float32)
        table[:, list(banned)] = -np.inf
        paths, lengths, scores = run_lm(device, x, 4, table, order, 0.0, 0.0, False)
        assert not np.isin(paths, banned).any() and (lengths[:, 0] >= 0).all() and np.isfinite(scores[:, 0]).all()
        for b in (0, 8):
            want, gap = L.beam_search_lm(x[b], 4, table, order, 0.0, 0.0, False)
            assert gap >= R.MIN_GAP
            B.compare((paths[b], lengths[b], scores[b]), want, 4, 32, ("charset", order, b))


# ------------------------------------------------------------------------------------------------ the ABI's contract
def check_abi_contract(device):
    from ccd_amd import _lib, ops
    lib = _lib.get()
    assert lib.ccd_abi_version() >= 24
    st = _lib.stream()
    n, T, C, W = 3, 8, 12, 4
    x = torch.randn(n, T, C, generator=torch.Generator().manual_seed(1)).to(device)
    table = torch.from_numpy(L.synthetic_table(46, C, 2)).to(device)
    paths = torch.full((n, W, T), 77, dtype=torch.int32, device=device)
    lengths = torch.full((n, W), 77, dtype=torch.int32, device=device)
    scores = torch.full((n, W), 77.0, device=device)
    ok = [x, T * C, C, n, T, C, 0, W, table, 2, 1.0, 0.0, 1, paths, lengths, scores, st]

    def untouched():
        return bool((paths == 77).all() and (lengths == 77).all() and (scores == 77.0).all())

    for i in (0, 8, 13, 14, 15):                                               # a missing pointer, lm included
        bad = list(ok)
        bad[i] = None
        assert lib.ccd_ctc_beam_search_lm(*bad) == -1 and untouched(), i
    for i, v in ((1, -1), (2, -1), (3, -1)):                                   # a negative stride or batch
        bad = list(ok)
        bad[i] = v
        assert lib.ccd_ctc_beam_search_lm(*bad) == -1 and untouched(), (i, v)
    for i, v in ((7, 0), (7, 17), (4, 0), (4, 65), (5, 1), (5, 129), (6, 2), (6, -1),      # what ccd_ctc_beam_search refuses
                 (9, 0), (9, 4), (12, 2), (12, -1),                                        # order, eos
                 (10, float("inf")), (10, float("nan")), (11, float("-inf")), (11, float("nan"))):     # weight, bonus
        bad = list(ok)
        bad[i] = v
        assert lib.ccd_ctc_beam_search_lm(*bad) == -2 and untouched(), (i, v)
    assert lib.ccd_ctc_beam_search_lm(None, 0, 0, 0, T, C, 0, W, None, 2, 1.0, 0.0, 1, None, None, None, st) == 0 and untouched()
    assert lib.ccd_ctc_beam_search_lm(*ok) == 0 and not untouched()
    # the wrappers
    lm = ops.ctc_char_lm(table.cpu(), 2)
    with pytest.raises(ValueError, match="built for 12 classes, the scores have 13"):
        ops.ctc_beam_search_lm(torch.zeros(1, 8, 13, device=device), 4, lm)
    with pytest.raises(ValueError, match="beam_width must lie in 1..16"):
        ops.ctc_beam_search_lm(x, 17, lm)
    with pytest.raises(ValueError, match="contiguous classes"):
        ops.ctc_beam_search_lm(x.transpose(1, 2), 4, lm)
    with pytest.raises(TypeError, match="lm must come from ctc_char_lm"):
        ops.ctc_beam_search_lm(x, 4, table)
    with pytest.raises(RuntimeError, match="ccd_ctc_beam_search_lm failed: unsupported shape"):
        ops.ctc_beam_search_lm(x, 4, lm, weight=float("inf"))
    with pytest.raises(ValueError, match="NaN"):
        ops.ctc_char_lm(torch.full((12, 12), float("nan")), 2)
    with pytest.raises(ValueError, match=r"has shape \[C\^2, C\]"):
        ops.ctc_char_lm(table.cpu(), 3)
    with pytest.raises(ValueError, match="order must lie in 1..3"):
        ops.ctc_char_lm(table.cpu(), 4)
    assert tuple(ops.ctc_beam_search_lm(torch.zeros(0, 8, 12, device=device), 4, lm)[0].shape) == (0, 4, 8)


# ------------------------------------------------------------------------------------------------ the Python surface
LM_WORDS = ["the", "clear", "Street", "street", "Hello", "World", "hello", "2024", "open", "Open", "a", "I"]


def _lm_convertor(W):
    from ccd_amd.convertor.char_lm import CharNGram
    from ccd_amd.convertor.ctc import CTCConvertor
    conv = CTCConvertor(beam_width=W)
    conv.set_lm(CharNGram.from_words(conv, LM_WORDS, order=2), weight=0.6, bonus=0.4)
    assert conv.lm_order == 2 and conv.lm_eos and conv.lm_stats == {"order": 2, "classes": 92, "rows": 92, "bytes": 92 * 92 * 4}
    return conv


def oracle_hyps(conv, probs, W):
    """The hypotheses of every sample as the oracle decodes the fp32 probabilities (numpy [B, T, C]) with the convertor's language
    model; no sample may miss the condition."""
    out = []
    table = conv.lm_model.table.numpy()
    for b in range(probs.shape[0]):
        hyps, gap = L.beam_search_lm(probs[b], W, table, conv.lm_order, conv.lm_weight, conv.lm_bonus, conv.lm_eos, normalized=True)
        assert gap >= R.MIN_GAP, (b, gap)
        out.append(hyps)
    return out


def oracle_strings(conv, probs, W):
    return conv.idx2str([list(h[0][0]) for h in oracle_hyps(conv, probs, W)])


def check_convertor(device):
    """tensor2nbest with a language model: the oracle's three best words and their fused scores; tensor2idx stays the greedy rule."""
    from ccd_amd.convertor.ctc import CTCConvertor
    probs = B.peaked(100, True)
    conv = _lm_convertor(4)
    want = oracle_hyps(conv, probs, 4)
    dev = torch.from_numpy(probs).to(device)
    indexes, log_probs = conv.tensor2nbest(dev, nbest=3)
    assert tuple(log_probs.shape) == (9, 3) and log_probs.dtype == torch.float32 and log_probs.device.type == "cpu"
    for b in range(9):
        assert indexes[b] == [list(w) for w, _ in want[b][:3]], b
        for r in range(3):
            assert abs(float(log_probs[b, r]) - want[b][r][1]) <= B.one_rounding(want[b][r][1])
    plain = CTCConvertor(beam_width=4).tensor2nbest(dev, nbest=3)
    assert not torch.equal(plain[1], log_probs)                                # the fused scores, not the plain ones
    assert conv.tensor2idx(dev) == CTCConvertor().tensor2idx(dev)
    conv.set_lm(None)
    again = conv.tensor2nbest(dev, nbest=3)
    assert again[0] == plain[0] and torch.equal(again[1], plain[1])            # absent: today's behaviour


def check_update_scores(device):
    """TextAccuracy.update_scores with a language-model convertor: the totals of the host update() on the oracle's strings."""
    from ccd_amd.metric.eval_acc import TextAccuracy
    probs = B.peaked(101, True)
    conv = _lm_convertor(4)
    strings = oracle_strings(conv, probs, 4)
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
