"""The checks of CTC prefix beam search along a lexicon's prefix tree (kernels/ctc_beam.h: ctc_beam_kernel<CTC_BEAM_TRIE>,
ccd_ctc_beam_search_trie) and of the two-stage decoder ops.ctc_lexicon_search that run on either backend: the CPU SIMT executor
(tests/test_ctc_trie_sim.py) and the MI355X (tests/test_ctc_trie_gpu.py).  `device` is where the tensors live.

Oracle: tests/ctc_trie_np.py, the specification in fp64 numpy, itself checked against brute force in tests/test_ctc_trie_cpu.py.
Gates, those of tests/ctc_beam_checks.py:
  * paths, lengths, word ids and the slot order equal the oracle's - on inputs where the oracle's own smallest gap between neighbouring
    candidate scores (the final re-rank included) is >= 1e-9, asserted for every sample;
  * |score - oracle| <= 2^-23 |oracle| + 1e-9: the one rounding to fp32;
  * two runs give identical bits;
  * recall at W = 16: the searched best word is the exhaustive scorer's on the same device, for every sample, with the bits of its score
    (a condition the numpy oracle meets on these inputs: tests/test_ctc_trie_cpu.py)."""
import functools
import itertools

import numpy as np
import pytest
import torch

import ctc_beam_checks as B
import ctc_beam_np as R
import ctc_lexicon_checks as LK
import ctc_lexicon_np as X
import ctc_trie_np as N

SEEDS = B.SEEDS
WIDTHS = B.WIDTHS
LONG_SEED = 103                       # T = 64, C = 128: the gap condition holds (asserted in oracle())


def trie_of(words, max_len=None):
    """A list of class sequences -> the ops.ctc_lexicon_trie handle of its lexicon."""
    from ccd_amd import ops
    return ops.ctc_lexicon_trie(ops.ctc_lexicon(torch.from_numpy(X.to_tensor(words, max_len))))


def run_trie(device, x, W, trie, normalized=False):
    """x fp32 [B, T, C], trie: a handle or a word list -> (paths [B, W, T], lengths [B, W], scores [B, W], word_ids [B, W]) as numpy;
    the scores are read in place from the strided view ctc_lexicon_checks.frames_view hands over."""
    from ccd_amd import ops
    view = LK.frames_view(device, x)
    n, T, _ = view.shape
    trie = trie if isinstance(trie, ops.CTCLexiconTrie) else trie_of(trie)
    paths, lengths, scores, ids = ops.ctc_beam_search_trie(view, W, trie, normalized=normalized)
    assert paths.dtype == lengths.dtype == ids.dtype == torch.int32 and scores.dtype == torch.float32
    assert tuple(paths.shape) == (n, W, T) and tuple(lengths.shape) == tuple(scores.shape) == tuple(ids.shape) == (n, W)
    return paths.cpu().numpy(), lengths.cpu().numpy(), scores.cpu().numpy(), ids.cpu().numpy()


def compare(got, want, W, T, where):
    """One sample: got = (paths [W, T], lengths [W], scores [W], word_ids [W]) against want = [(word, score, word id)] by rank."""
    B.compare(got[:3], [(w, s) for w, s, _ in want], W, T, where)
    assert got[3].tolist() == [k for _, _, k in want] + [-1] * (W - len(want)), (where, got[3].tolist(), want)


@functools.lru_cache(maxsize=None)
def lexicon(seed, normalized, n=9, T=32, C=92):
    """(x, words, the trie handle) of tests/ctc_trie_np.batch_lexicon, built once per process."""
    x, words = N.batch_lexicon(seed, normalized, n, T, C)
    return x, words, trie_of(words)


@functools.lru_cache(maxsize=None)
def oracle(seed, W, normalized, n=9, T=32, C=92):
    """The oracle's hypotheses of every sample of a batch_lexicon case, computed once per process; the gap condition holds for each."""
    x, _, trie = lexicon(seed, normalized, n, T, C)
    nodes = trie.nodes.numpy()
    out = []
    for b in range(n):
        hyps, gap = N.beam_search_trie(x[b], W, nodes, normalized)
        assert gap >= R.MIN_GAP, (seed, W, normalized, b, gap)
        out.append(hyps)
    return out


# ------------------------------------------------------------------------------------------------ 1. against brute force
def exhaustive_lexicons(T, C, exact):
    """The four lexicons of an exhaustive shape: all of brute force's words, every second one, all but the one-character words, and the
    empty word with EVERY word of T // 2 + 1 classes (some of them have no alignment)."""
    words = sorted(w for w, _ in exact)
    long_words = [tuple(w) for w in itertools.product(range(1, C), repeat=T // 2 + 1)]
    return [words, words[::2], [w for w in words if len(w) != 1], [()] + long_words]


def exact_hypotheses(x, normalized, words):
    """The lexicon's feasible words with their exact scores and ids, by (score descending, id)."""
    lp = R.log_probs(x, normalized)
    scored = [(tuple(w), X.word_score(lp, w), k) for k, w in enumerate(words)]
    return sorted([e for e in scored if e[1] > -np.inf], key=lambda e: (-e[1], e[2]))


def check_exhaustive(device):
    """Every prefix of the trie fits the beam: the hypotheses are exactly the lexicon's feasible words with their exact scores, in
    order; every other slot is empty."""
    for T, C in R.EXHAUSTIVE:
        for normalized in (False, True):
            x = R.small_case(T, C, seed=10 * T + C)
            x = R.softmax32(x) if normalized else x
            for which, words in enumerate(exhaustive_lexicons(T, C, R.brute_force(x, normalized))):
                want = exact_hypotheses(x, normalized, words)
                assert len(want) >= 1 and N.beam_search_trie(x, 16, N.build_trie(words), normalized)[1] >= R.MIN_GAP
                got = run_trie(device, x[None], 16, words, normalized)
                compare(tuple(a[0] for a in got), want, 16, T, (T, C, normalized, which))


# ------------------------------------------------------------------------------------------------ 2. against the oracle
def check_oracle(device, seeds=SEEDS):
    """B = 9 (a partial last workgroup), T = 32, C = 92, about 12 000 nodes, W in {1, 4, 16}, logits and the fp32 softmax - the many
    empty slots of W = 1 included."""
    empty = 0
    for seed in seeds:
        for normalized in (False, True):
            x, _, trie = lexicon(seed, normalized)
            for W in WIDTHS:
                want = oracle(seed, W, normalized)
                got = run_trie(device, x, W, trie, normalized)
                for b in range(x.shape[0]):
                    compare(tuple(a[b] for a in got), want[b], W, 32, (seed, normalized, W, b))
                if W == 16:
                    again = run_trie(device, x, W, trie, normalized)
                    assert all(a.tobytes() == c.tobytes() for a, c in zip(got, again))
            empty += sum(not h for h in oracle(seed, 1, normalized))
    print(f"W = 1 ends with no word on {empty} of {18 * len(seeds)} samples")


def check_oracle_long(device):
    """T = 64 with C = 128, the limits of the ABI, at W = 16 on one batch of 5: the plain beam's words exceed 31 classes and are not in
    the lexicon, so this is oracle equality only."""
    for normalized in (False, True):
        x, _, trie = lexicon(LONG_SEED, normalized, 5, 64, 128)
        want = oracle(LONG_SEED, 16, normalized, 5, 64, 128)
        got = run_trie(device, x, 16, trie, normalized)
        for b in range(5):
            compare(tuple(a[b] for a in got), want[b], 16, 64, ("long", normalized, b))


# ------------------------------------------------------------------------------------------------ 4. recall
def check_recall(device, seeds=SEEDS):
    """W = 16: the best word of ops.ctc_lexicon_search is the one ctc_lexicon_best(ctc_lexicon_score(all words)) picks on the same
    device, for all 9 samples, and its log-probability is ctc_lexicon_score(subset=)'s for that word, bit for bit."""
    from ccd_amd import ops
    for seed in seeds:
        for normalized in (False, True):
            x, words, trie = lexicon(seed, normalized)
            view = LK.frames_view(device, x)
            ids, log_probs = ops.ctc_lexicon_search(view, trie, 16, nbest=1, normalized=normalized)
            assert ids.dtype == torch.int32 and log_probs.dtype == torch.float32 and tuple(ids.shape) == tuple(log_probs.shape) == (9, 1)
            index, best = ops.ctc_lexicon_best(ops.ctc_lexicon_score(view, trie.lexicon, normalized=normalized), 1)
            assert ids.cpu().tolist() == index.cpu().tolist(), (seed, normalized, ids.cpu().tolist(), index.cpu().tolist())
            alone = ops.ctc_lexicon_score(view, trie.lexicon, normalized=normalized, subset=ids.contiguous())
            assert log_probs.cpu().numpy().tobytes() == alone.cpu().numpy().tobytes(), (seed, normalized)
            assert bool(torch.isfinite(log_probs).all()) and int(ids.min()) >= 0 and int(ids.max()) < len(words)
    # the n-best list: exact scores descending, a tie to the lower id, (-1, -inf) where the beam proposed fewer words
    x, words, trie = lexicon(seeds[0], False)
    view = LK.frames_view(device, x)
    ids, log_probs = (t.cpu().numpy() for t in ops.ctc_lexicon_search(view, trie, 4, nbest=4))
    proposed = run_trie(device, x, 4, trie)[3]
    full = ops.ctc_lexicon_score(view, trie.lexicon).cpu().numpy()
    for b in range(9):
        want = sorted((int(k) for k in proposed[b] if k >= 0), key=lambda k: (-full[b, k], k))
        assert ids[b].tolist() == want + [-1] * (4 - len(want)), (b, ids[b].tolist(), want)
        assert log_probs[b, :len(want)].tobytes() == full[b, want].tobytes() and np.isneginf(log_probs[b, len(want):]).all(), b
    assert (proposed < 0).any()


# ------------------------------------------------------------------------------------------------ 6. a merge inside the trie
def merge_case():
    """T = 4, C = 3 with mass on 1, blank, 1, 1 and the lexicon {(1,), (1, 1)}: the extension of (1,) by 1 spells the live prefix
    (1, 1) and is merged into it."""
    x = R.small_case(4, 3, seed=31)
    for t, c in enumerate((1, 0, 1, 1)):
        x[t, c] += np.float32(3.0)
    return x, [(1,), (1, 1)]


def check_merge(device):
    x, words = merge_case()
    nodes = N.build_trie(words)
    exact = dict(R.brute_force(x))
    for W in (2, 3, 16):
        want, gap = N.beam_search_trie(x, W, nodes)
        assert gap >= R.MIN_GAP
        if W >= 3:                                                             # (), (1,), (1, 1): nothing is pruned, the oracle is exact
            assert [w for w, _, _ in want] == sorted(words, key=lambda w: -exact[w])
            assert all(abs(s - exact[w]) <= 1e-12 for w, s, _ in want)
        got = run_trie(device, x[None], W, words)
        compare(tuple(a[0] for a in got), want, W, 4, ("merge", W))


# ------------------------------------------------------------------------------------------------ 7. a full lexicon is no constraint
def check_full_lexicon(device):
    """Every word of at most 2 classes over C = 4 at T = 2: paths, lengths and score bytes are ops.ctc_beam_search's."""
    words = [()] + [(a,) for a in range(1, 4)] + [(a, c) for a in range(1, 4) for c in range(1, 4)]
    x = np.stack([R.small_case(2, 4, seed=s) for s in (71, 72, 73)])
    for normalized in (False, True):
        data = R.softmax32(x) if normalized else x
        for W in (1, 4, 16):
            plain = B.run_beam(device, data, W, normalized)
            got = run_trie(device, data, W, words, normalized)
            assert all(a.tobytes() == c.tobytes() for a, c in zip(got[:3], plain)), (normalized, W)
            for b in range(3):
                for r in range(W):
                    word = tuple(got[0][b, r, :max(got[1][b, r], 0)].tolist())
                    assert got[3][b, r] == (words.index(word) if got[1][b, r] >= 0 else -1), (b, r)


# ------------------------------------------------------------------------------------------------ 8. the ABI's contract
def check_abi_contract(device):
    from ccd_amd import _lib, ops
    lib = _lib.get()
    assert lib.ccd_abi_version() >= 26
    st = _lib.stream()
    n, T, C, W = 3, 8, 12, 4
    x = torch.randn(n, T, C, generator=torch.Generator().manual_seed(1)).to(device)
    words = [(3,), (3, 11), (3, 95, 4), (95,), (3,), (7, 7)]                   # classes >= C = 12 on two paths, a duplicate row
    trie = trie_of(words)
    nodes = trie.on(device)
    paths = torch.full((n, W, T), 77, dtype=torch.int32, device=device)
    lengths = torch.full((n, W), 77, dtype=torch.int32, device=device)
    scores = torch.full((n, W), 77.0, device=device)
    ids = torch.full((n, W), 77, dtype=torch.int32, device=device)
    ok = [x, T * C, C, n, T, C, 0, W, nodes, trie.n_nodes, paths, lengths, scores, ids, st]

    def untouched():
        return bool((paths == 77).all() and (lengths == 77).all() and (scores == 77.0).all() and (ids == 77).all())

    for i in (0, 8, 10, 11, 12, 13):                                           # a missing pointer, nodes and word_ids included
        bad = list(ok)
        bad[i] = None
        assert lib.ccd_ctc_beam_search_trie(*bad) == -1 and untouched(), i
    for i, v in ((1, -1), (2, -1), (3, -1)):                                   # a negative stride or batch
        bad = list(ok)
        bad[i] = v
        assert lib.ccd_ctc_beam_search_trie(*bad) == -1 and untouched(), (i, v)
    for i, v in ((7, 0), (7, 17), (4, 0), (4, 65), (5, 1), (5, 129), (6, 2), (6, -1),      # what ccd_ctc_beam_search refuses
                 (9, 0), (9, -3)):                                                         # n_nodes
        bad = list(ok)
        bad[i] = v
        assert lib.ccd_ctc_beam_search_trie(*bad) == -2 and untouched(), (i, v)
    assert lib.ccd_ctc_beam_search_trie(None, 0, 0, 0, T, C, 0, W, None, 1, None, None, None, None, st) == 0 and untouched()
    assert lib.ccd_ctc_beam_search_trie(*ok) == 0 and not untouched()
    # a mask bit of a class >= C is unreachable, of duplicate rows the lowest is reported: the oracle's words
    got = tuple(t.cpu().numpy() for t in (paths, lengths, scores, ids))
    for b in range(n):
        want, gap = N.beam_search_trie(x[b].cpu().numpy(), W, trie.nodes.numpy())
        assert gap >= R.MIN_GAP and {k for _, _, k in want} <= {0, 1, 5}
        compare(tuple(a[b] for a in got), want, W, T, ("abi", b))
    assert not np.isin(got[3], (2, 3, 4)).any() and (got[3] >= 0).any() and not (got[0] >= C).any()
    # the empty lexicon: the root alone, no word
    empty = run_trie(device, x.cpu().numpy(), W, [])
    assert (empty[0] == -1).all() and (empty[1] == -1).all() and np.isneginf(empty[2]).all() and (empty[3] == -1).all()
    only = run_trie(device, x.cpu().numpy(), W, [()])                          # the empty word: the root is terminal
    assert (only[1][:, 0] == 0).all() and (only[3][:, 0] == 0).all() and (only[1][:, 1:] == -1).all()
    # the wrappers
    with pytest.raises(ValueError, match="beam_width must lie in 1..16"):
        ops.ctc_beam_search_trie(x, 17, trie)
    with pytest.raises(ValueError, match="contiguous classes"):
        ops.ctc_beam_search_trie(x.transpose(1, 2), 4, trie)
    with pytest.raises(TypeError, match="trie must come from ctc_lexicon_trie"):
        ops.ctc_beam_search_trie(x, 4, trie.lexicon)
    with pytest.raises(TypeError, match="lexicon must come from ctc_lexicon"):
        ops.ctc_lexicon_trie(trie.nodes)
    with pytest.raises(TypeError, match=r"^ccd_ctc_beam_search_trie: scores expects float32, got float64$"):
        ops.ctc_beam_search_trie(x.double(), 4, trie)
    with pytest.raises(RuntimeError, match="ccd_ctc_beam_search_trie failed: unsupported shape"):
        ops.ctc_beam_search_trie(torch.zeros(1, 65, 12, device=device), 4, trie)
    with pytest.raises(ValueError, match=r"nbest must lie in 1..beam_width = 4"):
        ops.ctc_lexicon_search(x, trie, 4, nbest=5)
    assert tuple(ops.ctc_beam_search_trie(torch.zeros(0, 8, 12, device=device), 4, trie)[3].shape) == (0, 4)
    assert tuple(ops.ctc_lexicon_search(torch.zeros(0, 8, 12, device=device), trie, 4, nbest=2)[0].shape) == (0, 2)
    assert trie.stats == {"nodes": trie.n_nodes, "bytes": 32 * trie.n_nodes, "terminals": 5} and trie.on(device) is nodes


def check_malformed_table(device):
    """A table whose first_child words point anywhere: every derived node id is clamped into the table, the call returns and the
    outputs are well-formed (which words come out is not specified)."""
    from ccd_amd import ops
    x, words, trie = lexicon(100, False)
    for value in (2 ** 30, -5, trie.n_nodes):
        nodes = trie.nodes.clone()
        nodes[:, 4] = value
        bad = ops.CTCLexiconTrie(trie.lexicon, nodes)
        paths, lengths, scores, ids = run_trie(device, x, 16, bad)
        assert (lengths >= -1).all() and (lengths <= 32).all() and (ids >= -1).all() and (ids < len(words)).all()
        assert (paths >= -1).all() and (paths < 92).all() and not np.isnan(scores).any()


# ------------------------------------------------------------------------------------------------ 9. the Python surface
def lexicon_strings(conv, words):
    """The words as strings that encode back to the same classes: class 91, <UKN>, is written as a character outside the alphabet."""
    assert conv.unknown_idx == 91
    strings = ["".join("é" if c == 91 else conv.idx2char[c] for c in w) for w in words]
    assert conv.str2idx(strings) == [list(w) for w in words]
    return strings


@functools.lru_cache(maxsize=None)
def convertors(seed):
    """(probabilities, words, a convertor with lexicon_beam 16, one with the exhaustive path) over batch_lexicon(seed, softmax)."""
    from ccd_amd.convertor.ctc import CTCConvertor
    x, words = N.batch_lexicon(seed, True)
    strings = lexicon_strings(CTCConvertor(), words)
    searched, full = CTCConvertor(lexicon=strings, lexicon_beam=16), CTCConvertor(lexicon=strings)
    assert searched.lexicon_stats["kept"] == full.lexicon_stats["kept"] == len(words)
    return x, words, searched, full


def check_convertor(device):
    """tensor2lexicon with lexicon_beam = 16: the exhaustive path's words and the bits of their log-probabilities; the refusals."""
    from ccd_amd.convertor.attn import AttnConvertor
    from ccd_amd.convertor.ctc import CTCConvertor
    probs, words, searched, full = convertors(100)
    assert searched.lexicon_beam == 16 and searched.lexicon_trie is not None and full.lexicon_beam == 0
    assert searched.lexicon_stats["nodes"] == searched.lexicon_trie.n_nodes == N.build_trie(words).shape[0]
    assert "nodes" not in full.lexicon_stats
    dev = torch.from_numpy(probs).to(device)
    want = full.tensor2lexicon(dev, nbest=1)
    got = searched.tensor2lexicon(dev, nbest=1)
    assert got[0] == want[0] and torch.equal(got[2], want[2]) and got[1].numpy().tobytes() == want[1].numpy().tobytes()
    assert got[2].dtype == torch.int64 and got[1].device.type == "cpu" and tuple(got[1].shape) == (9, 1)
    late = CTCConvertor(lexicon=lexicon_strings(CTCConvertor(), words))        # the argument overrides, the trie is built on demand
    assert late.lexicon_trie is None
    again = late.tensor2lexicon(dev, nbest=1, beam=16)
    assert again[0] == want[0] and torch.equal(again[2], want[2]) and late.lexicon_trie is not None and late.lexicon_beam == 0
    exhaustive = searched.tensor2lexicon(dev, nbest=3, beam=0)
    assert exhaustive[0] == full.tensor2lexicon(dev, nbest=3)[0]
    three = searched.tensor2lexicon(dev, nbest=3)                              # exact scores, descending; every word a lexicon row
    assert all(three[1][b, r] >= three[1][b, r + 1] for b in range(9) for r in range(2))
    assert all(three[0][b][r] == list(words[int(three[2][b, r])]) for b in range(9) for r in range(len(three[0][b])))
    subset = torch.tensor([[5, -1, 2, 7]] * 9, dtype=torch.int32).to(device)
    with pytest.raises(ValueError, match="a subset and a beam exclude each other"):
        searched.tensor2lexicon(dev, nbest=1, subset=subset)
    assert searched.tensor2lexicon(dev, nbest=1, subset=subset, beam=0)[0] == full.tensor2lexicon(dev, nbest=1, subset=subset)[0]
    with pytest.raises(ValueError, match="nbest must lie in 1..beam = 16"):
        searched.tensor2lexicon(dev, nbest=17)
    with pytest.raises(ValueError, match="lexicon_beam must lie in 0..16"):
        CTCConvertor(lexicon=["a"], lexicon_beam=17)
    with pytest.raises(ValueError, match="lexicon_beam = 4 needs a lexicon"):
        CTCConvertor(lexicon_beam=4)
    with pytest.raises(ValueError, match="lexicon.*beam_width|beam_width.*lexicon"):
        CTCConvertor(beam_width=4, lexicon=["a"], lexicon_beam=4)
    with pytest.raises(NotImplementedError, match="CTC head only"):
        AttnConvertor(lexicon_beam=4)
    conv = CTCConvertor()
    stats = conv.set_lexicon(["ab", "abc", "b"], beam=8)
    assert stats == {"read": 3, "kept": 3, "too_long": 0, "duplicates": 0, "nodes": 5} and conv.lexicon_beam == 8
    assert conv.set_lexicon(["ab", "abc", "b"], beam=0) == {"read": 3, "kept": 3, "too_long": 0, "duplicates": 0} and conv.lexicon_trie is None
    conv.set_lexicon(["ab"], beam=8)
    conv.set_lexicon(None)
    assert conv.lexicon is None and conv.lexicon_trie is None and conv.lexicon_beam == 0
    assert searched.tensor2idx(dev) == CTCConvertor().tensor2idx(dev)


def check_align(device):
    """tensor2align with lexicon_beam: the targets are the rows of the searched words, rank by rank."""
    probs, words, searched, full = convertors(100)
    dev = torch.from_numpy(probs).to(device)
    _, _, ids = searched.tensor2lexicon(dev, nbest=2)
    res = searched.tensor2align(dev, nbest=2)
    table = searched.lexicon.words
    for b in range(9):
        for r in range(2):
            row = b * 2 + r
            if ids[b, r] >= 0:
                assert int(res["rows"][row]) == b and torch.equal(res["targets"][row].cpu(), table[int(ids[b, r])]), (b, r)
                assert bool(torch.isfinite(res["score"][row]))
            else:
                assert int(res["rows"][row]) == -1
    assert torch.equal(res["targets"][0::2].cpu(), full.tensor2align(dev, nbest=1)["targets"].cpu())      # (recall at W = 16)
    from ccd_amd.convertor.ctc import CTCConvertor
    with pytest.raises(ValueError, match="nbest must lie in 1..lexicon_beam = 4"):
        CTCConvertor(lexicon=["ab", "b"], lexicon_beam=4).tensor2align(dev, nbest=5)


def host_strings(conv, dev):
    """What the host path decodes: tensor2lexicon -> idx2str, the empty string where the search found no word."""
    return conv.idx2str([w[0] if w else [] for w in conv.tensor2lexicon(dev, nbest=1)[0]])


def check_update_scores(device, sync_debug=False):
    """TextAccuracy.update_scores with lexicon_beam scores what the host path (tensor2lexicon -> idx2str) decodes; on the GPU the
    device path runs under torch.cuda.set_sync_debug_mode("error")."""
    from ccd_amd.metric.eval_acc import TextAccuracy
    probs, _, searched, full = convertors(101)
    dev = torch.from_numpy(probs).to(device)
    strings = host_strings(searched, dev)
    assert strings == host_strings(full, dev) and all(strings)                 # (recall at W = 16)
    gts = [s if b % 2 else s[:-1] + "Q" for b, s in enumerate(strings)]       # half of them right
    host = TextAccuracy()
    host.update(gts, strings)
    want = host.result()
    metric = TextAccuracy()
    if sync_debug:
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
    try:
        metric.update_scores(dev, gts, searched)
    finally:
        if sync_debug:
            torch.cuda.set_sync_debug_mode("default")
    got = metric.result()
    for k in ("ccr", "cwr", "ted", "ted/w", "words"):
        assert got[k] == want[k], (k, got[k], want[k])
    assert abs(got["ned"] - want["ned"]) <= 9 * 2.0 ** -52 * max(1.0, want["ned"]) and 0 < want["cwr"] < 1
