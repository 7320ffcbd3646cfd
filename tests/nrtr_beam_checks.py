"""The checks of beam search over the NRTR decoder (kernels/nrtr_beam.h: ccd_nrtr_beam_step, ccd_nrtr_beam_reorder) that run on either
backend: the CPU SIMT executor (tests/test_nrtr_beam_sim.py) and the MI355X (tests/test_nrtr_beam_gpu.py).  `device` is where the
tensors live.

Oracle: tests/nrtr_beam_np.py, the specification in fp64 numpy, itself checked against the arg-max chain and brute force in
tests/test_nrtr_beam_cpu.py.  The logits of a step come from a random Markov table - table[sample, step, previous token] is a row of
C fp32 values, gathered with torch - so the kernel's own permutation of the sequences decides what it is fed next.
Gates:
  * paths, lengths and the parents of every step equal the oracle's - on samples where the oracle's smallest gap between
    neighbouring candidates is >= 1e-9 (fp64 rounding is seven orders below it); at most 2 % of the samples may miss that;
  * |score - oracle| <= 1e-6 |oracle| (the one rounding to fp32 is 6e-8);
  * the cache permutation is compared bit for bit."""
import functools

import numpy as np
import pytest
import torch

import nrtr_beam_np as R

LD_PAD = 5                                                       # the logits rows are C + 5 wide, NaN behind column C


def drive(device, tab, W):
    """tab fp32 [B, T, C + 1, C] -> (paths [B, W, T], lengths [B, W], scores [B, W], parents [B, T, W]) as numpy: T calls of
    ops.nrtr_beam_step; start = end = C - 1, padding = C.  Rows of slots that are not live hold NaN: the kernel must not read them."""
    from ccd_amd import ops
    B, T, _, C = tab.shape
    end, pad = C - 1, C
    seq, score, state, parent = ops.nrtr_beam_state(B, W, T + 1, end, pad, device)
    table = torch.from_numpy(tab).to(device)
    sample = torch.arange(B, device=device).repeat_interleave(W)
    buf = torch.full((B * W, C + LD_PAD), float("nan"), device=device)
    parents, out = [], None
    for s in range(T):
        rows = table[sample, s, seq[:, s]]
        rows[state.view(-1) != ops.NRTR_LIVE] = float("nan")
        buf[:, :C] = rows
        out = ops.nrtr_beam_step(buf, C, s, end, pad, seq, score, state, parent, final=s == T - 1)
        assert (out is None) == (s < T - 1)
        parents.append(parent.cpu().numpy().copy())
    paths, lengths, scores = out
    assert paths.dtype == torch.int32 and lengths.dtype == torch.int32 and scores.dtype == torch.float32
    assert tuple(paths.shape) == (B, W, T) and tuple(lengths.shape) == (B, W) and tuple(scores.shape) == (B, W)
    # the state agrees with what was returned: sequences hold the start token, the path, then end / padding
    assert (seq[:, 0] == end).all() and (scores.double() - score).abs().nan_to_num(0.0).max() <= 1e-4
    return paths.cpu().numpy(), lengths.cpu().numpy(), scores.cpu().numpy(), np.stack(parents, axis=1)


@functools.lru_cache(maxsize=None)
def case_tables(seed, B, T, C, mode="flat"):
    return R.tables(seed, B, T, C, mode)


@functools.lru_cache(maxsize=None)
def oracle(seed, B, W, C, T, mode="flat", ties=False):
    """The oracle's result of every sample, computed once per process."""
    tab = case_tables(seed, B, T, C, mode)
    return [R.beam_search(tab[b], W, C - 1, C - 1, C, ties) for b in range(B)]


def compare(got, want, where):
    """One sample: got = (paths [W, T], lengths [W], scores [W], parents [T, W]) against the oracle's tuple."""
    paths, lengths, scores, parents = got
    w_paths, w_lengths, w_scores, w_parents, _ = want
    np.testing.assert_array_equal(parents, w_parents, err_msg=str(where))
    np.testing.assert_array_equal(lengths, w_lengths, err_msg=str(where))
    np.testing.assert_array_equal(paths, w_paths, err_msg=str(where))
    for r in range(len(lengths)):
        if w_lengths[r] < 0:
            assert scores[r] == -np.inf, (where, r)
        else:
            assert abs(float(scores[r]) - w_scores[r]) <= 1e-6 * abs(w_scores[r]), (where, r, float(scores[r]), w_scores[r])


def dropped_fraction(cases, seed):
    """The share of samples whose oracle gap misses MIN_GAP, over all cases."""
    gaps = [want[4] for case in cases for want in oracle(seed, *case)]
    return sum(g < R.MIN_GAP for g in gaps) / len(gaps)


def _run_cases(device, cases, seed):
    compared = 0
    for case in cases:
        B, W, C, T = case[:4]
        mode = case[4] if len(case) > 4 else "flat"
        want = oracle(seed, B, W, C, T, mode)
        got = drive(device, case_tables(seed, B, T, C, mode), W)
        for b in range(B):
            if want[b][4] >= R.MIN_GAP:
                compare(tuple(a[b] for a in got), want[b], (case, b))
                compared += 1
    return compared


SEED = 7


def check_oracle(device):
    """B in {1, 5}, W in {1, 2, 3, 8, 16}, C in {3, 64, 65, 92, 128}, T in {4, 25}: the 64-lane boundary, a row stride, W > C."""
    total = sum(c[0] for c in R.CASES)
    assert _run_cases(device, R.CASES, SEED) >= 0.98 * total
    # W > C leaves unused slots behind in the first steps: C = 3, W = 16 holds 3 hypotheses after step 0, 7 after step 1
    paths, lengths, scores, parents = drive(device, case_tables(SEED, 1, 1, 3), 16)
    assert (lengths[0, :3] >= 0).all() and (lengths[0, 3:] == -1).all() and np.isneginf(scores[0, 3:]).all() and (paths[0, 3:] == -1).all()
    assert (parents[0, 0, :3] == 0).all() and (parents[0, 0, 3:] == -1).all()


def check_end_heavy(device):
    """Peaked rows whose peak is now and then the end class (nrtr_beam_np.markov_table, "end"): finished slots carry through many steps and compete with live ones."""
    total = sum(c[0] for c in R.END_HEAVY)
    assert _run_cases(device, R.END_HEAVY, SEED) >= 0.98 * total
    for B, W, C, T, mode in R.END_HEAVY[:2]:
        lengths = np.stack([w[1] for w in oracle(SEED, B, W, C, T, mode)])
        assert (lengths == T).any() and ((lengths >= 0) & (lengths < T - 8)).any(), (W, C)      # both kinds, finished long before the end


def check_width_one_is_greedy(device):
    tab = case_tables(SEED, 5, 25, 92, "end")
    paths, lengths, scores, _ = drive(device, tab, 1)
    for b in range(5):
        word, score = R.greedy(tab[b], 91, 91)
        assert paths[b, 0, :lengths[b, 0]].tolist() == word and abs(float(scores[b, 0]) - score) <= 1e-6 * abs(score)


def check_exhaustive(device):
    """A beam at least as wide as the number of hypotheses returns every one of them, in the order of the exact scores."""
    for C, T in ((3, 2), (2, 4)):
        tab = case_tables(SEED + 1, 1, T, C)
        exact = R.brute_force(tab[0], C - 1, C - 1)
        assert len(exact) <= 16
        paths, lengths, scores, _ = drive(device, tab, 16)
        for r, (word, score, finished) in enumerate(exact):
            assert paths[0, r, :lengths[0, r]].tolist() == list(word) and (lengths[0, r] < T) == finished, (C, T, r)
            assert abs(float(scores[0, r]) - score) <= 1e-6 * abs(score)
        assert (lengths[0, len(exact):] == -1).all()
        assert abs(float(np.exp(scores[0, :len(exact)].astype(np.float64)).sum()) - 1.0) <= 1e-5


# ------------------------------------------------------------------------------------------------ ties
def tie_table():
    """T = 6, C = 6 (end = 5): classes 0 and 1 are twins - equal logits in every row, and the same row behind either - and lead at
    step 1.  Every hypothesis with one of them has a twin with the same score bits; from step 2 on two slots hold equal scores and
    identical logit rows."""
    tab = R.markov_table(21, 6, 6)
    tab[1, :, 0] += 5.0
    tab[:5, :, 5] -= 6.0                                         # (no word ends early: the best ones all pass step 1)
    tab[:, :, 1] = tab[:, :, 0]
    tab[:, 1, :] = tab[:, 0, :]
    return tab[None]


def check_ties(device):
    tab = tie_table()
    for W in (1, 2, 3, 4, 8, 16):
        want = R.beam_search(tab[0], W, 5, 5, 6, ties=True)
        assert want[4] >= R.MIN_GAP
        got = drive(device, tab, W)
        compare(tuple(a[0] for a in got), want, ("ties", W))
        paths, lengths, scores, _ = (a[0] for a in got)
        words = [tuple(paths[r, :lengths[r]].tolist()) for r in range(W) if lengths[r] >= 0]
        check_tied_order(words, scores)


def check_tied_order(words, scores):
    """Words that differ only in 0 <-> 1 are tied bit for bit; the lower flat index won wherever they first differ, so they come in
    lexicographic order.  The best word holds a twin class and spells it 0."""
    plain = lambda w: tuple(0 if c == 1 else c for c in w)                                     # noqa: E731
    assert 0 in words[0] and 1 not in words[0], words[0]
    pairs = 0
    for r in range(len(words)):
        for q in range(r + 1, len(words)):
            if plain(words[r]) == plain(words[q]):
                assert np.asarray(scores[r]).tobytes() == np.asarray(scores[q]).tobytes() and words[r] < words[q], (words[r], words[q])
                pairs += 1
    assert len(words) < 2 or (plain(words[1]) == plain(words[0]) and pairs >= 1)


# ------------------------------------------------------------------------------------------------ the cache permutation
def _parents(kind, B, W, gen):
    ident = torch.arange(W, dtype=torch.int32).repeat(B, 1)
    if kind == "identity":
        return ident
    if kind == "swap":
        p = ident.clone()
        p[:, 0], p[:, 1] = 1, 0
        return p
    if kind == "cycle3":
        p = ident.clone()
        p[:, 0], p[:, 1], p[:, 2] = 1, 2, 0
        return p
    if kind == "zero":
        return torch.zeros_like(ident)
    if kind == "permutation":
        return torch.stack([torch.randperm(W, generator=gen) for _ in range(B)]).int()
    if kind == "mapping":                                                                      # shared parents and unused slots (-1)
        return torch.randint(-1, W, (B, W), generator=gen).int()
    raise KeyError(kind)


def check_reorder(device):
    """L = 2, B = 3, T' = 26, D = 128: the K and V columns of positions <= s are the parents', the rest of K and V and every Q column
    behind s are untouched, bit for bit; in place, whatever cycles or shared parents the permutation has."""
    from ccd_amd import ops
    L, B, Tp, D = 2, 3, 26, 128
    gen = torch.Generator().manual_seed(3)
    for W in (1, 3, 16):
        base = torch.randn(L, B * W * Tp, 3 * D, generator=gen).to(torch.bfloat16)
        kinds = ["identity", "zero", "permutation", "mapping"] + (["swap", "cycle3"] if W >= 3 else [])
        for kind in kinds:
            parent = _parents(kind, B, W, gen)
            for s in (0, 7, 25):
                want = base.clone().view(L, B, W, Tp, 3 * D)
                src = base.view(L, B, W, Tp, 3 * D)
                for b in range(B):
                    for r in range(W):
                        p = int(parent[b, r])
                        if p >= 0:
                            want[:, b, r, :s + 1, D:] = src[:, b, p, :s + 1, D:]
                cache = base.clone().to(device)
                ops.nrtr_beam_reorder(cache, parent.to(device), Tp, s)
                got = cache.cpu().view(L, B, W, Tp, 3 * D)
                assert torch.equal(got[..., D:].view(torch.int16), want[..., D:].view(torch.int16)), (W, kind, s)
                assert torch.equal(got[..., s + 1:, :D].view(torch.int16), want[..., s + 1:, :D].view(torch.int16)), (W, kind, s)


# ------------------------------------------------------------------------------------------------ arguments
def check_arguments(device):
    from ccd_amd import _lib, ops
    assert _lib.get().ccd_abi_version() >= 22 and ops.NRTR_MAX_BEAM == 16
    B, W, C, T = 2, 4, 12, 5
    seq, score, state, parent = ops.nrtr_beam_state(B, W, T + 1, C - 1, C, device)
    logits = torch.randn(B * W, C + 3, generator=torch.Generator().manual_seed(1)).to(device)
    ok = dict(logits=logits, C=C, step=0, end_idx=C - 1, pad_idx=C, seq=seq, score=score, state=state, parent=parent)

    def bad(**kw):
        before = [t.clone() for t in (seq, score, state, parent)]
        with pytest.raises(ValueError):
            ops.nrtr_beam_step(**{**ok, **kw})
        assert all(torch.equal(a, b) for a, b in zip((seq, score, state, parent), before))

    for width in (0, 17):
        with pytest.raises(ValueError, match="beam_width must lie in 1..16"):
            ops.nrtr_beam_state(B, width, T + 1, C - 1, C, device)
    bad(score=torch.zeros(B, 17, dtype=torch.float64, device=device))                           # width 17
    bad(score=torch.zeros(B, 0, dtype=torch.float64, device=device))                            # width 0
    bad(score=score.float())                                                                    # wrong dtypes
    bad(state=state.long())
    bad(parent=parent.long())
    bad(seq=seq.int())
    bad(logits=logits.double())
    bad(state=state[:1])                                                                        # wrong shapes
    bad(parent=parent.view(-1))
    bad(seq=seq[:-1])
    bad(seq=seq.view(B, W, T + 1))
    bad(logits=logits[:-1])
    bad(logits=logits[:, :C - 1])
    bad(logits=logits.t().contiguous().t())
    bad(step=T)                                                                                 # seq[:, step + 1] does not exist
    bad(step=-1)
    bad(end_idx=C)
    bad(pad_idx=-1)
    cache = torch.zeros(2, B * W * (T + 1), 3 * 64, dtype=torch.bfloat16, device=device)
    for kw in (dict(parent=parent.long()), dict(parent=parent.view(-1)), dict(parent=torch.zeros(B, 17, dtype=torch.int32, device=device)),
               dict(cache=cache.float()), dict(cache=cache[:, :-1]), dict(cache=cache.view(-1, 3 * 64)), dict(cache=cache[:, :, :100]),
               dict(step=T + 1), dict(step=-1), dict(positions=T)):
        with pytest.raises(ValueError, match="nrtr_beam_reorder"):
            ops.nrtr_beam_reorder(**{**dict(cache=cache, parent=parent, positions=T + 1, step=0), **kw})
    # the entry points themselves refuse what the wrappers let through, and launch nothing
    lib, st = _lib.get(), _lib.stream()
    args = [logits, C + 3, B, W, C, 0, C - 1, C, seq, T + 1, score, state, parent, None, None, None, st]
    for i, v, code in ((0, None, -1), (8, None, -1), (12, None, -1), (1, -1, -1), (5, -1, -1), (3, 0, -2), (3, 17, -2), (4, 129, -2),
                       (1, C - 1, -2), (9, 129, -2), (5, T, -2), (6, C, -2), (7, 65536, -2)):
        call = list(args)
        call[i] = v
        assert lib.ccd_nrtr_beam_step(*call) == code, (i, v)
    call = list(args)
    call[13] = torch.zeros(B, W, T, dtype=torch.int32, device=device)                           # paths without lengths and scores
    assert lib.ccd_nrtr_beam_step(*call) == -1
    assert int(state.sum()) == B and int(parent.min()) == -1 and int(parent.max()) == -1        # nothing ran
    assert lib.ccd_nrtr_beam_step(None, C, 0, W, C, 0, C - 1, C, None, T + 1, None, None, None, None, None, None, st) == 0
    for i, v, code in ((0, None, -1), (1, None, -1), (7, -1, -1), (4, 0, -2), (4, 17, -2), (6, 12, -2), (7, T + 1, -2)):
        call = [cache, parent, 2, B, W, T + 1, 64, 0, st]
        call[i] = v
        assert lib.ccd_nrtr_beam_reorder(*call) == code, (i, v)
    assert lib.ccd_nrtr_beam_reorder(None, None, 2, 0, W, T + 1, 64, 0, st) == 0
    ops.nrtr_beam_step(**ok)
    assert int(parent.min()) == 0 and int(parent.max()) == 0 and int((state == ops.NRTR_UNUSED).sum()) == 0


# ------------------------------------------------------------------------------------------------ the convertor
def check_convertor(device):
    """paths2nbest: index lists by rank, unused slots dropped, log-probabilities on the host; path_score_table + text_score_paths give
    the records of the host's update() on the strings (class 0, '0', included: the reason for the shifted rows)."""
    from ccd_amd import ops
    from ccd_amd.convertor.attn import AttnConvertor
    from ccd_amd.metric.eval_acc import TextAccuracy
    conv = AttnConvertor(dict_type="DICT90", max_seq_len=25, with_unknown=True, beam_width=4)
    assert conv.beam_width == 4 and AttnConvertor().beam_width == 0
    for width in (-1, 17):
        with pytest.raises(ValueError, match="beam_width must lie in 0..16"):
            AttnConvertor(beam_width=width)
    words = ["0a0", "Hello", "", "x" * 25, "a<UKN>b"]
    rows = [[0, 10, 0], conv.str2idx(["Hello"])[0], [], [33] * 25, [10, 90, 11]]
    paths = torch.full((5, 4, 25), -1, dtype=torch.int32)
    lengths = torch.full((5, 4), -1, dtype=torch.int32)
    scores = torch.full((5, 4), float("-inf"))
    for b, row in enumerate(rows):
        for r in range(2 if b else 4):
            cut = row[:len(row) - r] if r else row
            paths[b, r, :len(cut)] = torch.tensor(cut, dtype=torch.int32)
            lengths[b, r], scores[b, r] = len(cut), -1.0 - r
    indexes, log_probs = conv.paths2nbest(paths.to(device), lengths.to(device), scores.to(device), nbest=3)
    assert tuple(log_probs.shape) == (5, 3) and log_probs.device.type == "cpu" and log_probs.dtype == torch.float32
    assert [len(w) for w in indexes] == [3, 2, 2, 2, 2] and [w[0] for w in indexes] == rows and np.isneginf(float(log_probs[1, 2]))
    assert conv.idx2str([w[0] for w in indexes]) == words
    with pytest.raises(ValueError, match="nbest must lie in"):
        conv.paths2nbest(paths, lengths, scores, nbest=5)
    truth = ["0a0", "hello", "q", "x" * 24 + "y", "a?b"]
    metric = TextAccuracy()
    rec = metric.update_paths(paths.to(device)[:, 0], truth, conv).cpu().numpy()
    for b in range(5):
        one = TextAccuracy()
        one.update([truth[b]], [words[b]])
        assert rec[b].tolist() == [int(one.total_ed), int(one.correct_num_char), len(truth[b]), int(one.correct_num_word)], (b, rec[b])
    host = TextAccuracy()
    host.update(truth, words)
    got, want = metric.result(), host.result()
    assert all(got[k] == want[k] for k in ("ccr", "cwr", "ted", "words")) and abs(got["ned"] - want["ned"]) < 1e-12
    # compute() on the host path (a model that is not on a GPU): idx2str of rank 0 of paths2nbest, scored by update()

    class Stub(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.weight = torch.nn.Parameter(torch.zeros(1))
            self.label_convertor = conv
            self.widths = []

        def forward_beam(self, img, beam_width=None):
            self.widths.append(beam_width)
            return paths, lengths, scores

    stub = Stub()
    res = TextAccuracy().compute(stub, [(torch.zeros(5, 3, 32, 128), (truth,))])
    assert stub.widths == [4] and all(res[k] == want[k] for k in ("ccr", "cwr", "ted", "words")) and abs(res["ned"] - want["ned"]) < 1e-12
