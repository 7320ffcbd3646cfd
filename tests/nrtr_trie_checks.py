"""The checks of beam search over the NRTR decoder along a lexicon's prefix tree (kernels/nrtr_beam.h: nrtr_beam_step_kernel<true>,
ccd_nrtr_beam_step_trie) that run on either backend: the CPU SIMT executor (tests/test_nrtr_trie_sim.py) and the MI355X
(tests/test_nrtr_trie_gpu.py).  `device` is where the tensors live.

Oracle: tests/nrtr_trie_np.py, the specification in fp64 numpy, itself checked against brute force over the lexicon in
tests/test_nrtr_trie_cpu.py.  As in tests/nrtr_beam_checks.py the logits of a step come from a random Markov table gathered with
torch, so the kernel's own permutation of the sequences decides what it is fed next.  The lexicon of a case is the union of the
lexicons nrtr_trie_np.lexicon generates for its samples (about 300 words each), as rows class + 1, and its trie is the one
ops.ctc_lexicon_trie builds.
Gates:
  * the parents of every step, paths, lengths, word ids and the final nodes equal the oracle's - on samples where the oracle's
    smallest gap between neighbouring candidates is >= 1e-9; at most 2 % of the samples may miss that;
  * |score - oracle| <= 1e-6 |oracle| (the one rounding to fp32 is 6e-8);
  * every returned word id >= 0 names the lexicon row that equals its path."""
import functools

import numpy as np
import pytest
import torch

import nrtr_beam_checks as K
import nrtr_beam_np as R
import nrtr_trie_np as S

LD_PAD = K.LD_PAD
SEED = 11
CASES = [(5, 1, 92, 25), (5, 4, 92, 25), (5, 8, 92, 25), (5, 16, 92, 25), (5, 16, 65, 25), (5, 8, 64, 4), (5, 3, 128, 25),
         (5, 2, 127, 25), (1, 16, 3, 4)]                       # (B, W, C, T); each with the tables "flat" and "end"
MODES = ("flat", "end")


def handle_of(words, class_offset=1):
    """A list of class sequences -> the ops.ctc_lexicon_trie handle of the rows class + class_offset."""
    from ccd_amd import ops
    return ops.ctc_lexicon_trie(ops.ctc_lexicon(torch.from_numpy(S.rows_of(words, class_offset))))


def drive(device, tab, W, trie, end=None, pad=None, class_offset=1):
    """tab fp32 [B, T, C + 1, C] -> (paths [B, W, T], lengths [B, W], scores [B, W], word_ids [B, W], node [B, W], parents [B, T, W])
    as numpy: T calls of ops.nrtr_beam_step_trie; start = end (default C - 1), padding C.  Rows of slots that are not live hold NaN,
    and the logits have a row stride: the kernel must not read either."""
    from ccd_amd import ops
    B, T, _, C = tab.shape
    end, pad = C - 1 if end is None else end, C if pad is None else pad
    seq, score, state, parent = ops.nrtr_beam_state(B, W, T + 1, end, pad, device)
    node = ops.nrtr_beam_trie_state(B, W, device)
    assert node.dtype == torch.int32 and tuple(node.shape) == (B, W) and int(node.abs().sum()) == 0
    table = torch.from_numpy(tab).to(device)
    sample = torch.arange(B, device=device).repeat_interleave(W)
    buf = torch.full((B * W, C + LD_PAD), float("nan"), device=device)
    parents, out = [], None
    for s in range(T):
        rows = table[sample, s, seq[:, s]]
        rows[state.view(-1) != ops.NRTR_LIVE] = float("nan")
        buf[:, :C] = rows
        out = ops.nrtr_beam_step_trie(buf, C, s, end, pad, seq, score, state, parent, node, trie, class_offset=class_offset,
                                      final=s == T - 1)
        assert (out is None) == (s < T - 1)
        parents.append(parent.cpu().numpy().copy())
    paths, lengths, scores, ids = out
    assert paths.dtype == lengths.dtype == ids.dtype == torch.int32 and scores.dtype == torch.float32
    assert tuple(paths.shape) == (B, W, T) and tuple(lengths.shape) == tuple(scores.shape) == tuple(ids.shape) == (B, W)
    assert (seq[:, 0] == end).all() and (scores.double() - score).abs().nan_to_num(0.0).max() <= 1e-4
    return (paths.cpu().numpy(), lengths.cpu().numpy(), scores.cpu().numpy(), ids.cpu().numpy(), node.cpu().numpy(),
            np.stack(parents, axis=1))


@functools.lru_cache(maxsize=None)
def case_lexicon(seed, B, T, C, mode):
    """(the tables, the sorted union of the samples' lexicons, its trie handle), built once per process."""
    tab = K.case_tables(seed, B, T, C, mode)
    words = sorted(set().union(*[S.lexicon(seed * 977 + b, tab[b]) for b in range(B)]))
    return tab, words, handle_of(words)


@functools.lru_cache(maxsize=None)
def oracle(seed, B, W, C, T, mode):
    """The oracle's result of every sample, computed once per process."""
    tab, _, trie = case_lexicon(seed, B, T, C, mode)
    nodes = trie.nodes.numpy()
    return [S.beam_search_trie(tab[b], W, C - 1, C - 1, C, nodes) for b in range(B)]


def compare(got, want, words, where):
    """One sample: got = (paths [W, T], lengths [W], scores [W], word_ids [W], node [W], parents [T, W]) against the oracle's tuple."""
    paths, lengths, scores, ids, node, parents = got
    w_paths, w_lengths, w_scores, w_ids, w_node, w_parents, _ = want
    np.testing.assert_array_equal(parents, w_parents, err_msg=str(where))
    np.testing.assert_array_equal(lengths, w_lengths, err_msg=str(where))
    np.testing.assert_array_equal(paths, w_paths, err_msg=str(where))
    np.testing.assert_array_equal(ids, w_ids, err_msg=str(where))
    np.testing.assert_array_equal(node, w_node, err_msg=str(where))
    for r in range(len(lengths)):
        if w_lengths[r] < 0:
            assert scores[r] == -np.inf and ids[r] == -1, (where, r)
        else:
            assert abs(float(scores[r]) - w_scores[r]) <= 1e-6 * abs(w_scores[r]), (where, r, float(scores[r]), w_scores[r])
        if ids[r] >= 0:                                                        # the id names the row that equals the path
            assert tuple(paths[r, :lengths[r]].tolist()) == tuple(words[ids[r]]), (where, r)


def all_cases():
    return [case + (mode,) for case in CASES for mode in MODES]


def dropped_fraction(seed=SEED):
    """The share of samples whose oracle gap misses MIN_GAP, over all cases."""
    gaps = [want[6] for case in all_cases() for want in oracle(seed, *case)]
    return sum(g < S.MIN_GAP for g in gaps) / len(gaps)


# ------------------------------------------------------------------------------------------------ 1. against the oracle
def check_oracle(device):
    """W in {1, 2, 3, 4, 8, 16}, C in {3, 64, 65, 92, 127, 128} (the 64-lane boundary, bit 127 of the mask), T in {4, 25}, both kinds of
    table: finished slots beside live ones, unused slots where the lexicon offers fewer candidates than the beam is wide."""
    total = compared = live_at_end = words_found = 0
    for B, W, C, T, mode in all_cases():
        tab, words, trie = case_lexicon(SEED, B, T, C, mode)
        want = oracle(SEED, B, W, C, T, mode)
        got = drive(device, tab, W, trie)
        for b in range(B):
            total += 1
            if want[b][6] >= S.MIN_GAP:
                compare(tuple(a[b] for a in got), want[b], words, ((B, W, C, T, mode), b))
                compared += 1
            live_at_end += int(((want[b][1] == T) & (want[b][3] == -1)).sum())
            words_found += int((want[b][3] >= 0).sum())
    assert compared >= 0.98 * total, (compared, total)
    assert live_at_end > 0 and words_found > 0                                 # both kinds of slot occur behind the last step


# ------------------------------------------------------------------------------------------------ 2. a beam as wide as the lexicon
def small_lexicon(seed, table):
    """12 words of at most T - 1 classes - half of them along likely paths - plus prefixes of some, 16 words at the most, and one of
    them replaced by a word of T + 1 classes, whose <EOS> never fits."""
    rng = np.random.default_rng(seed)
    T, _, C = table.shape
    words = set()
    while len(words) < 11:
        length = int(rng.integers(1, T))
        words.add(S.likely_word(rng, table, length, C - 1, C - 1) if len(words) % 2 else
                  tuple(int(c) for c in rng.integers(0, C - 1, length)))
    for w in sorted(words):
        if len(w) > 1 and rng.random() < 0.3 and len(words) < 15:
            words.add(w[:int(rng.integers(1, len(w)))])
    words.add(S.likely_word(rng, table, T + 1, C - 1, C - 1, pick=1))
    return sorted(words)


def check_wide_beam(device):
    """A lexicon of at most 16 words at W = 16: live prefixes and finished words never outnumber the words, so no slot is ever dropped
    and the beam returns EVERY word of at most T - 1 classes, ranked by its exact score, with that score."""
    C, T = 92, 25
    for seed in range(5):
        tab = K.case_tables(SEED + 1 + seed, 1, T, C, "end")
        words = small_lexicon(seed, tab[0])
        assert 12 <= len(words) <= 16
        exact = S.exact_words(tab[0], words, C - 1, C - 1)
        assert len(exact) == len(words) - 1                                    # all but the word that is too long
        paths, lengths, scores, ids, _, _ = drive(device, tab, 16, handle_of(words))
        ranks = [r for r in range(16) if ids[0, r] >= 0]                       # (the live prefix of the long word sits among them, by its
        assert ids[0, ranks].tolist() == [k for k, _ in exact], (seed, ids[0].tolist(), exact)     # score; it is no word: -1)
        for r, (k, score) in zip(ranks, exact):
            assert tuple(paths[0, r, :lengths[0, r]].tolist()) == tuple(words[k]), (seed, r)
            assert abs(float(scores[0, r]) - score) <= 1e-6 * abs(score), (seed, r, float(scores[0, r]), score)
        rest = [r for r in range(16) if ids[0, r] < 0]                         # what is left: that live prefix, at T classes, and unused slots
        assert sum(lengths[0, r] == T for r in rest) == 1 and all(lengths[0, r] in (T, -1) for r in rest)


# ------------------------------------------------------------------------------------------------ 3. W = 1
def greedy_trie(table, nodes, start_idx, end_idx, class_offset=1):
    """The constrained arg-max chain (first maximum among the allowed classes) -> (word, score, word id; -1 if it never ends)."""
    T, _, C = table.shape
    smp = S.TrieSample(1, start_idx, nodes, class_offset)
    prev, node, word, score = start_idx, 0, [], 0.0
    for s in range(T):
        lp = np.where(smp.allowed(node, C, end_idx), S.log_softmax64(table[s, prev]), -np.inf)
        c = int(np.argmax(lp))
        if lp[c] == -np.inf:
            return None, -np.inf, -1
        score += lp[c]
        if c == end_idx:
            return word, score, int(nodes[node, 5])
        word.append(c)
        node = S.N.child(nodes, node, c + class_offset)
        prev = c
    return word, score, -1


def check_width_one(device):
    tab, words, trie = case_lexicon(SEED, 5, 25, 92, "end")
    paths, lengths, scores, ids, _, _ = drive(device, tab, 1, trie)
    for b in range(5):
        word, score, k = greedy_trie(tab[b], trie.nodes.numpy(), 91, 91)
        assert paths[b, 0, :lengths[b, 0]].tolist() == word and ids[b, 0] == k, (b, word, k)
        assert abs(float(scores[b, 0]) - score) <= 1e-6 * abs(score)


# ------------------------------------------------------------------------------------------------ 4. -inf logits
def check_masked_sample(device):
    """-inf on every class the root allows leaves sample 1 without a candidate at step 0: all its slots are unused from then on."""
    tab, words, trie = case_lexicon(SEED, 5, 25, 92, "flat")
    tab = tab.copy()
    first = sorted({w[0] for w in words})
    tab[1, 0, 91, first] = -np.inf
    nodes = trie.nodes.numpy()
    got = drive(device, tab, 8, trie)
    paths, lengths, scores, ids, node, parents = got
    assert (ids[1] == -1).all() and (lengths[1] == -1).all() and np.isneginf(scores[1]).all() and (paths[1] == -1).all()
    assert (node[1] == 0).all() and (parents[1] == -1).all()
    for b in (0, 2, 3, 4):                                                     # the neighbours are untouched
        want = S.beam_search_trie(tab[b], 8, 91, 91, 92, nodes)
        assert want[6] >= S.MIN_GAP
        compare(tuple(a[b] for a in got), want, words, ("masked", b))


# ------------------------------------------------------------------------------------------------ 5. the boundaries of the mask
def check_boundary_classes(device):
    """C = 128 with the end class 5, so that class 127 is a character: classes 31, 63 and 126 test bits 32, 64 and 127, class 127 has
    no bit - a word with it is left out of the trie and never proposed, whatever its logit.  Their neighbours 30, 32, 62, 64 and 125
    are in no word: a kernel that tested the bit beside the right one would follow them."""
    C, T, end = 128, 6, 5
    tab = K.case_tables(SEED + 9, 2, T, C, "flat").copy()
    for c in (30, 31, 32, 62, 63, 64, 125, 126, 127):                          # all of them likely
        tab[:, :, :, c] += np.float32(4.0)
    words = [(31,), (63,), (126,), (31, 63), (63, 126), (126, 31, 63), (127,), (126, 127), (31, 127, 63), (7,), (7, 126), (0,), (0, 31)]
    trie = handle_of(words)
    nodes = trie.nodes.numpy()
    assert (nodes == S.trie_of(words)).all() and not (nodes[:, 5] == 6).any() and not (nodes[:, 5] == 7).any() and not (nodes[:, 5] == 8).any()
    got = drive(device, tab, 16, trie, end=end, pad=C)
    for b in range(2):
        want = S.beam_search_trie(tab[b], 16, end, end, C, nodes)
        assert want[6] >= S.MIN_GAP
        compare(tuple(a[b] for a in got), want, words, ("boundary", b))
        exact = S.exact_words(tab[b], [w for w in words if 127 not in w], end, end)
        kept = [k for k, w in enumerate(words) if 127 not in w]
        assert got[3][b, :len(exact)].tolist() == [kept[k] for k, _ in exact]  # every reachable word, by its exact score
        assert not np.isin(got[3][b], (6, 7, 8)).any() and not (got[0][b] == 127).any()


# ------------------------------------------------------------------------------------------------ 6. arguments
def check_arguments(device):
    from ccd_amd import _lib, ops
    lib = _lib.get()
    assert lib.ccd_abi_version() >= 27
    B, W, C, T = 2, 4, 12, 5
    seq, score, state, parent = ops.nrtr_beam_state(B, W, T + 1, C - 1, C, device)
    node = ops.nrtr_beam_trie_state(B, W, device)
    trie = handle_of([(3,), (3, 4), (7, 7)])
    logits = torch.randn(B * W, C + 3, generator=torch.Generator().manual_seed(1)).to(device)
    ok = dict(logits=logits, C=C, step=0, end_idx=C - 1, pad_idx=C, seq=seq, score=score, state=state, parent=parent, node=node, trie=trie)
    tensors = (seq, score, state, parent, node)

    def bad(error=ValueError, **kw):
        before = [t.clone() for t in tensors]
        with pytest.raises(error):
            ops.nrtr_beam_step_trie(**{**ok, **kw})
        assert all(torch.equal(a, b) for a, b in zip(tensors, before))

    for width in (0, 17):
        with pytest.raises(ValueError, match="beam_width must lie in 1..16"):
            ops.nrtr_beam_trie_state(B, width, device)
    bad(node=node.long())                                                      # a wrong dtype or shape of node
    bad(node=node[:1])
    bad(node=node.view(-1))
    bad(node=node.t().contiguous().t())
    bad(TypeError, trie=trie.nodes)                                            # a foreign trie
    bad(TypeError, trie=trie.lexicon)
    bad(class_offset=2)
    bad(class_offset=-1)
    bad(score=score.float())                                                   # what nrtr_beam_step refuses
    bad(state=state.long())
    bad(seq=seq[:-1])
    bad(logits=logits[:, :C - 1])
    bad(step=T)
    bad(end_idx=C)
    # the entry point itself refuses what the wrapper lets through, and launches nothing
    st, nodes = _lib.stream(), trie.on(device)
    args = [logits, C + 3, B, W, C, 0, C - 1, C, seq, T + 1, score, state, parent, None, None, None, nodes, trie.n_nodes, 1, node, None, st]
    for i, v, code in ((0, None, -1), (8, None, -1), (12, None, -1), (16, None, -1), (19, None, -1), (1, -1, -1), (5, -1, -1),
                       (3, 0, -2), (3, 17, -2), (4, 129, -2), (9, 129, -2), (5, T, -2), (6, C, -2), (7, 65536, -2),
                       (17, 0, -2), (17, -3, -2), (18, 2, -2), (18, -1, -2)):
        call = list(args)
        call[i] = v
        assert lib.ccd_nrtr_beam_step_trie(*call) == code, (i, v)
    call = list(args)
    call[20] = torch.zeros(B, W, dtype=torch.int32, device=device)            # word_ids without paths
    assert lib.ccd_nrtr_beam_step_trie(*call) == -1
    call = list(args)                                                          # paths, lengths and scores without word_ids
    call[13], call[14], call[15] = (torch.zeros(B, W, T, dtype=torch.int32, device=device), torch.zeros(B, W, dtype=torch.int32, device=device),
                                    torch.zeros(B, W, device=device))
    assert lib.ccd_nrtr_beam_step_trie(*call) == -1
    assert int(state.sum()) == B and int(parent.min()) == -1 and int(parent.max()) == -1 and int(node.abs().sum()) == 0      # nothing ran
    assert lib.ccd_nrtr_beam_step_trie(None, C, 0, W, C, 0, C - 1, C, None, T + 1, None, None, None, None, None, None, None, 1, 1, None,
                                       None, st) == 0
    ops.nrtr_beam_step_trie(**ok)                                              # the root allows classes 3 and 7: two live slots
    assert parent.cpu().tolist() == [[0, 0, -1, -1]] * B and state.cpu().tolist() == [[1, 1, 0, 0]] * B
    assert sorted(seq.view(B, W, T + 1)[0, :2, 1].cpu().tolist()) == [3, 7] and int(node.min()) == 0 and int(node.max()) == 2
    # class_offset 0: the rows are the classes themselves
    node.zero_()
    seq2, score2, state2, parent2 = ops.nrtr_beam_state(B, W, T + 1, C - 1, C, device)
    ops.nrtr_beam_step_trie(logits, C, 0, C - 1, C, seq2, score2, state2, parent2, node, trie, class_offset=0)
    assert sorted(seq2.view(B, W, T + 1)[0, :2, 1].cpu().tolist()) == [4, 8]
    # a node outside the table is clamped into it: the call returns and the state stays well-formed
    node.fill_(2 ** 30)
    ops.nrtr_beam_step_trie(logits, C, 1, C - 1, C, seq2, score2, state2, parent2, node, trie, class_offset=0)
    assert int(node.min()) >= 0 and int(node.max()) < trie.n_nodes
