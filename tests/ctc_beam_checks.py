"""The checks of CTC prefix beam search (kernels/ctc_beam.h, ccd_ctc_beam_search) and of ccd_text_score_paths that run on either backend:
the CPU SIMT executor (tests/test_ctc_beam_sim.py) and the MI355X (tests/test_ctc_beam_gpu.py).  `device` is where the tensors live.

Oracle: tests/ctc_beam_np.py, the specification in fp64 numpy, itself checked against brute force in tests/test_ctc_beam_cpu.py.
Gates:
  * paths, lengths and the slot order equal the oracle's - on inputs where the oracle's own smallest gap between neighbouring
    candidate scores is >= 1e-9 (asserted for every sample: a condition on the inputs, fp64 rounding is nine orders below it);
  * |score - oracle| <= 2^-23 |oracle| + 1e-9: the one rounding to fp32;
  * score <= -nll + 2^-22 max(1, |nll|) for the nll ccd_ctc_loss_fwd gives the hypothesis as a target (two fp32 roundings), with
    equality where every word fits the beam;
  * two runs give identical bits."""
import functools

import numpy as np
import pytest
import torch

import ctc_beam_np as R

LD = 128
SEEDS = (100, 101, 102)
WIDTHS = (1, 4, 16)


def one_rounding(exact):
    return 2.0 ** -23 * abs(exact) + 1e-9


def run_beam(device, x, W, normalized=False):
    """x fp32 [B, T, C] -> (paths [B, W, T], lengths [B, W], scores [B, W]) as numpy; the scores are read in place from a [B * T, 128]
    buffer with NaN behind column C, the view CTCHeadFn hands out."""
    from ccd_amd import ops
    x = torch.as_tensor(x)
    B, T, C = x.shape
    buf = torch.full((B * T, LD), float("nan"))
    buf[:, :C] = x.reshape(B * T, C)
    view = buf.to(device).view(B, T, LD)[:, :, :C]
    paths, lengths, scores = ops.ctc_beam_search(view, W, normalized=normalized)
    assert paths.dtype == torch.int32 and lengths.dtype == torch.int32 and scores.dtype == torch.float32
    assert tuple(paths.shape) == (B, W, T) and tuple(lengths.shape) == (B, W) and tuple(scores.shape) == (B, W)
    return paths.cpu().numpy(), lengths.cpu().numpy(), scores.cpu().numpy()


def compare(got, want, W, T, where):
    """One sample: got = (paths [W, T], lengths [W], scores [W]) against want = [(word, score)] by rank."""
    paths, lengths, scores = got
    for r in range(W):
        if r < len(want):
            word, exact = want[r]
            assert lengths[r] == len(word) and paths[r, :len(word)].tolist() == list(word), (where, r, paths[r].tolist(), word)
            assert (paths[r, len(word):] == -1).all(), (where, r)
            assert abs(float(scores[r]) - exact) <= one_rounding(exact), (where, r, float(scores[r]), exact)
        else:
            assert lengths[r] == -1 and scores[r] == -np.inf and (paths[r] == -1).all(), (where, r)


@functools.lru_cache(maxsize=None)
def peaked(seed, normalized, B=9, T=32, C=92):
    x = R.peaked_batch(seed, B, T, C)
    return R.softmax32(x) if normalized else x


@functools.lru_cache(maxsize=None)
def oracle(seed, W, normalized, B=9, T=32, C=92):
    """The oracle's hypotheses of every sample of a peaked batch, computed once per process; the gap condition holds for each."""
    x = peaked(seed, normalized, B, T, C)
    out = []
    for b in range(B):
        hyps, gap = R.beam_search(x[b], W, normalized)
        assert gap >= R.MIN_GAP, (seed, W, normalized, b, gap)
        out.append(hyps)
    return out


# ------------------------------------------------------------------------------------------------ against brute force
def check_exhaustive(device):
    """Every word fits the beam: the hypotheses are all the words, in the order of their exact probabilities."""
    for T, C in R.EXHAUSTIVE:
        for normalized in (False, True):
            x = R.small_case(T, C, seed=10 * T + C)
            x = R.softmax32(x) if normalized else x
            exact = R.brute_force(x, normalized)
            assert R.beam_search(x, 16, normalized)[1] >= R.MIN_GAP
            paths, lengths, scores = run_beam(device, x[None], 16, normalized)
            compare((paths[0], lengths[0], scores[0]), exact, 16, T, (T, C, normalized))
            assert abs(float(np.exp(scores[0].astype(np.float64)).sum()) - 1.0) <= 16 * 2.0 ** -23


# ------------------------------------------------------------------------------------------------ against the oracle
def check_oracle(device, seeds=SEEDS):
    """B = 9 (a partial last workgroup), T = 32, C = 92, W in {1, 4, 16}, logits and the fp32 softmax; then T = 64, C = 128."""
    differ = 0
    for seed in seeds:
        for normalized in (False, True):
            x = peaked(seed, normalized)
            for W in WIDTHS:
                want = oracle(seed, W, normalized)
                got = run_beam(device, x, W, normalized)
                for b in range(x.shape[0]):
                    compare(tuple(a[b] for a in got), want[b], W, 32, (seed, normalized, W, b))
                if W == 16 and seed == seeds[0]:
                    again = run_beam(device, x, W, normalized)
                    assert all(a.tobytes() == c.tobytes() for a, c in zip(got, again))
            differ += sum(oracle(seed, 16, normalized)[b][0][0] != oracle(seed, 1, normalized)[b][0][0] for b in range(x.shape[0]))
    print(f"best word at W = 16 differs from W = 1 on {differ} samples")


def check_oracle_long(device):
    """T = 64 with C = 128, the limits of the ABI, at W = 16 on one batch of 5."""
    for normalized in (False, True):
        x = peaked(103, normalized, 5, 64, 128)
        want = oracle(103, 16, normalized, 5, 64, 128)
        got = run_beam(device, x, 16, normalized)
        for b in range(5):
            compare(tuple(a[b] for a in got), want[b], 16, 64, ("long", normalized, b))


# ------------------------------------------------------------------------------------------------ ties, empty slots, masks
def tie_case():
    """T = 6, C = 6; the columns of classes 2 and 4 are bit-identical and lead at frame 1: every word with one of them has a twin of
    the same score bits, and the best word holds one."""
    x = R.small_case(6, 6, seed=21)
    x[1, 2] += 5.0
    x[:, 4] = x[:, 2]
    return x


def _twin(word):
    return tuple({2: 4, 4: 2}.get(c, c) for c in word)


def check_ties(device):
    x = tie_case()
    for W in (1, 2, 3, 4, 8, 16):
        want, gap = R.beam_search(x, W, ties=True)
        assert gap >= R.MIN_GAP
        paths, lengths, scores = run_beam(device, x[None], W)
        compare((paths[0], lengths[0], scores[0]), want, W, 6, ("ties", W))
        words = [tuple(paths[0, r, :lengths[0, r]].tolist()) for r in range(W) if lengths[0, r] >= 0]
        assert words[0] < _twin(words[0]), words[0]                           # the lower class first, where the twins first differ
        for r, w in enumerate(words):
            if _twin(w) != w and _twin(w) in words:
                q = words.index(_twin(w))
                assert scores[0, r].tobytes() == scores[0, q].tobytes() and (r < q) == (w < _twin(w)), (W, w, r, q)
        if W >= 2:
            assert words[1] == _twin(words[0]), words[:2]


def check_fewer_than_beam(device):
    # T = 1, C = 3: "", 1, 2 and thirteen empty slots
    x = R.small_case(1, 3, seed=5)
    paths, lengths, scores = run_beam(device, x[None], 16)
    want = R.brute_force(x)
    assert len(want) == 3
    compare((paths[0], lengths[0], scores[0]), want, 16, 1, "T=1")
    assert (lengths[0, 3:] == -1).all() and np.isneginf(scores[0, 3:]).all() and (paths[0, 3:] == -1).all()
    # an all -inf frame empties the beam of that sample alone; a masked class never appears
    y = np.stack([R.small_case(5, 4, seed=6), R.small_case(5, 4, seed=7), R.small_case(5, 4, seed=8)])
    y[1, 2, :] = -np.inf
    y[2, :, 3] = -np.inf
    y[2, 0, 1] = -np.inf
    for normalized in (False, True):
        data = R.softmax32(y) if normalized else y
        if normalized:
            data[1, 2, :] = 0.0
        paths, lengths, scores = run_beam(device, data, 16, normalized)
        assert (lengths[1] == -1).all() and np.isneginf(scores[1]).all() and (paths[1] == -1).all()
        for b in (0, 2):
            want, gap = R.beam_search(data[b], 16, normalized)
            assert gap >= R.MIN_GAP and not np.isnan(scores[b]).any()
            compare((paths[b], lengths[b], scores[b]), want, 16, 5, ("masked", normalized, b))
        assert not (paths[2] == 3).any() and (lengths[2] >= 0).sum() > 4


# ------------------------------------------------------------------------------------------------ against the loss kernel
def _nll_of(device, x, words):
    """-log p(word | x) by ccd_ctc_loss_fwd for every (sample, word): x [B, T, C] logits, words[b] = list of tuples."""
    from ccd_amd import ops
    B, T, C = x.shape
    pairs = [(b, w) for b in range(B) for w in words[b]]
    buf = torch.full((len(pairs) * T, LD), float("nan"))
    targets = torch.zeros(len(pairs), 31, dtype=torch.long)
    for n, (b, w) in enumerate(pairs):
        buf[n * T:(n + 1) * T, :C] = torch.from_numpy(x[b])
        targets[n, :len(w)] = torch.tensor(w, dtype=torch.long)
    nll, acc, _ = ops.ctc_loss_fwd(buf.to(device), C, targets.to(device), T)
    assert int(acc[2]) == 0
    return pairs, nll.cpu().numpy().astype(np.float64)


def check_lower_bound(device):
    """exp(score) is a lower bound of the word's CTC probability, and the probability itself where nothing was pruned."""
    for x, W, exact in [(peaked(100, False), 16, False), (peaked(101, False), 4, False)] + \
                       [(R.small_case(T, C, seed=10 * T + C)[None], 16, True) for T, C in R.EXHAUSTIVE]:
        paths, lengths, scores = run_beam(device, x, W)
        words = [[tuple(paths[b, r, :lengths[b, r]].tolist()) for r in range(W) if 0 <= lengths[b, r] <= 31] for b in range(x.shape[0])]
        score_of = {(b, tuple(paths[b, r, :lengths[b, r]].tolist())): float(scores[b, r]) for b in range(x.shape[0]) for r in range(W)
                    if lengths[b, r] >= 0}
        pairs, nll = _nll_of(device, x, words)
        assert len(pairs) >= x.shape[0]
        slack = 0.0
        for (b, w), v in zip(pairs, nll):
            tol = 2.0 ** -22 * max(1.0, abs(v))
            s = score_of[(b, w)]
            assert s <= -v + tol, (b, w, s, -v)
            if exact:
                assert abs(s + v) <= tol, (b, w, s, -v)
            slack = max(slack, -v - s)
        print(f"W = {W}, T = {x.shape[1]}: largest log p(word) - score {slack:.3e}")


# ------------------------------------------------------------------------------------------------ text_score_paths
def check_score_paths(device):
    """Records of ops.text_score_paths: those of text_score_ctc on one-hot scores that spell the same paths, and those of the host
    TextAccuracy.update on the strings (<UKN>, repeated characters, an empty word, 32 characters)."""
    import ctc_checks as K
    import ctc_np as G
    from ccd_amd import ops
    from ccd_amd.convertor.ctc import CTCConvertor
    from ccd_amd.metric.eval_acc import TextAccuracy, encode_truth
    conv = CTCConvertor()
    x = K.greedy_case()
    gts = list(K.GREEDY_TRUTH)
    path, length, _ = G.greedy(x.numpy())
    path[8] = -1
    path[8, :3] = [5, 5, 91]                                                   # repeated characters next to each other, then <UKN>
    length[8] = 3
    words = [path[b, :length[b]].tolist() for b in range(9)]
    assert any(91 in w for w in words) and [] in words and max(map(len, words)) == 32
    onehot = torch.full((9, 42, 92), -4.0)                                     # 42 frames x 3 normalised characters fit the kernel
    for b, w in enumerate(words):
        frames = []
        for c in w:                                                            # a blank between equal neighbours, blanks behind the word
            frames += [0, c] if frames and frames[-1] == c else [c]
        for t, c in enumerate(frames + [0] * (42 - len(frames))):
            onehot[b, t, c] = 9.0
    raw, norm = (torch.from_numpy(t).to(device) for t in conv.score_table())
    codes, lens = (torch.from_numpy(a).to(device) for a in encode_truth(gts))
    rec = ops.text_score_paths(torch.from_numpy(path).to(device), raw, norm, codes, lens).cpu().numpy()
    idx, _ = conv.tensor2idx(onehot)
    assert idx == words
    np.testing.assert_array_equal(rec, ops.text_score_ctc(onehot.to(device), raw, norm, codes, lens).cpu().numpy())
    for b in range(9):
        one = TextAccuracy()
        one.update([gts[b]], conv.idx2str([words[b]]))
        assert rec[b].tolist() == [int(one.total_ed), int(one.correct_num_char), len(gts[b]), int(one.correct_num_word)], (b, rec[b])
    # rank 0 of a [B, W, T] result is read in place; classes outside [1, C) count nothing and are never an index
    wide = torch.full((9, 4, 32), 7, dtype=torch.int32)
    wide[:, 0] = torch.from_numpy(path)
    np.testing.assert_array_equal(ops.text_score_paths(wide.to(device)[:, 0], raw, norm, codes, lens).cpu().numpy(), rec)
    odd, plain = torch.from_numpy(path).clone(), torch.from_numpy(path).clone()
    odd[1] = 9
    odd[1, :6] = torch.tensor([5, 0, 92, 2 ** 30, 6, -7], dtype=torch.int32)
    plain[1] = -1
    plain[1, :2] = torch.tensor([5, 6], dtype=torch.int32)
    np.testing.assert_array_equal(ops.text_score_paths(odd.to(device), raw, norm, codes, lens).cpu().numpy(),
                                  ops.text_score_paths(plain.to(device), raw, norm, codes, lens).cpu().numpy())
    with pytest.raises(ValueError, match="text_score_paths: expects paths"):
        ops.text_score_paths(torch.from_numpy(path).to(device)[None], raw, norm, codes, lens)
    with pytest.raises(TypeError, match=r"^ccd_text_score_paths: paths expects int32, got int64$"):
        ops.text_score_paths(torch.from_numpy(path).long().to(device), raw, norm, codes, lens)


# ------------------------------------------------------------------------------------------------ the ABI's contract
def check_abi_contract(device):
    from ccd_amd import _lib, ops
    from ccd_amd.convertor.ctc import CTCConvertor
    from ccd_amd.metric.eval_acc import encode_truth
    lib = _lib.get()
    assert lib.ccd_abi_version() >= 21
    st = _lib.stream()
    B, T, C, W = 3, 8, 12, 4
    x = torch.randn(B, T, C, generator=torch.Generator().manual_seed(1)).to(device)
    paths = torch.full((B, W, T), 77, dtype=torch.int32, device=device)
    lengths = torch.full((B, W), 77, dtype=torch.int32, device=device)
    scores = torch.full((B, W), 77.0, device=device)
    ok = [x, T * C, C, B, T, C, 0, W, paths, lengths, scores, st]

    def untouched():
        return bool((paths == 77).all() and (lengths == 77).all() and (scores == 77.0).all())

    for i in (0, 8, 9, 10):                                                    # a missing pointer
        bad = list(ok)
        bad[i] = None
        assert lib.ccd_ctc_beam_search(*bad) == -1 and untouched(), i
    for i, v in ((1, -1), (2, -1), (3, -1)):                                   # a negative stride or batch
        bad = list(ok)
        bad[i] = v
        assert lib.ccd_ctc_beam_search(*bad) == -1 and untouched(), (i, v)
    for i, v in ((7, 0), (7, 17), (4, 0), (4, 65), (5, 1), (5, 129), (6, 2), (6, -1)):     # beam, steps, classes, normalized
        bad = list(ok)
        bad[i] = v
        assert lib.ccd_ctc_beam_search(*bad) == -2 and untouched(), (i, v)
    assert lib.ccd_ctc_beam_search(None, 0, 0, 0, T, C, 0, W, None, None, None, st) == 0 and untouched()      # batch 0: a no-op
    assert lib.ccd_ctc_beam_search(*ok) == 0 and not untouched()
    for normalized in (0, 1):                                                  # the limits themselves are inside
        big = torch.rand(1, 64, 128).to(device)
        out = [torch.zeros(1, 16, 64, dtype=torch.int32, device=device), torch.zeros(1, 16, dtype=torch.int32, device=device),
               torch.zeros(1, 16, device=device)]
        assert lib.ccd_ctc_beam_search(big, 64 * 128, 128, 1, 64, 128, normalized, 16, *out, st) == 0
        assert int(out[1].min()) >= 0 and bool(torch.isfinite(out[2]).all())
    # text_score_paths: the error codes of ccd_text_score
    conv = CTCConvertor()
    raw, norm = (torch.from_numpy(t).to(device) for t in conv.score_table())
    codes, lens = (torch.from_numpy(a).to(device) for a in encode_truth(["ab", "c", ""]))
    p = torch.full((B, 32), -1, dtype=torch.int32, device=device)
    rec = torch.full((B, 4), 77, dtype=torch.int32, device=device)
    ok = [p, 32, B, 32, 92, raw, raw.shape[1], norm, norm.shape[1], codes, codes.shape[1], codes.shape[1], lens, rec, st]
    for i in (0, 5, 7, 9, 12, 13):
        bad = list(ok)
        bad[i] = None
        assert lib.ccd_text_score_paths(*bad) == -1 and bool((rec == 77).all()), i
    for i, v in ((1, -1), (2, -1), (10, -1), (3, 43), (3, 0), (4, 0), (6, 65), (8, 0)):
        bad = list(ok)
        bad[i] = v
        assert lib.ccd_text_score_paths(*bad) == (-1 if v == -1 else -2) and bool((rec == 77).all()), (i, v)
    assert lib.ccd_text_score_paths(None, 0, 0, 32, 92, None, 1, None, 1, None, 0, 0, None, None, st) == 0
    assert lib.ccd_text_score_paths(*ok) == 0 and rec.cpu().tolist() == [[2, 0, 2, 0], [1, 0, 1, 0], [0, 0, 0, 1]]
    # the wrappers
    with pytest.raises(ValueError, match="beam_width must lie in 1..16"):
        ops.ctc_beam_search(x, 17)
    with pytest.raises(ValueError, match="contiguous classes"):
        ops.ctc_beam_search(x.transpose(1, 2), 4)
    with pytest.raises(TypeError, match=r"^ccd_ctc_beam_search: scores expects float32, got float64$"):
        ops.ctc_beam_search(x.double(), 4)
    with pytest.raises(RuntimeError, match="ccd_ctc_beam_search failed: unsupported shape"):
        ops.ctc_beam_search(torch.zeros(1, 65, 12, device=device), 4)
    assert tuple(ops.ctc_beam_search(torch.zeros(0, 8, 12, device=device), 4)[0].shape) == (0, 4, 8)


# ------------------------------------------------------------------------------------------------ the Python surface
def check_convertor(device):
    """tensor2nbest: the oracle's three best words and their log-probabilities; tensor2idx stays the greedy rule."""
    from ccd_amd.convertor.ctc import CTCConvertor
    probs = peaked(100, True)
    want = oracle(100, 4, True)
    conv = CTCConvertor(beam_width=4)
    dev = torch.from_numpy(probs).to(device)
    indexes, log_probs = conv.tensor2nbest(dev, nbest=3)
    assert tuple(log_probs.shape) == (9, 3) and log_probs.dtype == torch.float32 and log_probs.device.type == "cpu"
    for b in range(9):
        assert indexes[b] == [list(w) for w, _ in want[b][:3]], b
        for r in range(3):
            assert abs(float(log_probs[b, r]) - want[b][r][1]) <= one_rounding(want[b][r][1])
    wide, _ = CTCConvertor().tensor2nbest(dev, beam_width=16, nbest=1)
    assert [w[0] for w in wide] == [list(h[0][0]) for h in oracle(100, 16, True)]
    one, lp = conv.tensor2nbest(torch.from_numpy(R.softmax32(R.small_case(1, 3, seed=5)[None])).to(device), nbest=4)
    assert len(one[0]) == 3 and np.isneginf(float(lp[0, 3]))                    # an empty slot: no word, -inf
    assert conv.tensor2idx(dev) == CTCConvertor().tensor2idx(dev)
    with pytest.raises(ValueError, match="beam_width >= 1"):
        CTCConvertor().tensor2nbest(dev)
    with pytest.raises(ValueError, match="nbest must lie in"):
        conv.tensor2nbest(dev, nbest=5)
    with pytest.raises(ValueError, match="beam_width must lie in 0..16"):
        CTCConvertor(beam_width=17)


def oracle_strings(conv, probs, W):
    """The best word of every sample as the oracle decodes the fp32 probabilities (numpy [B, T, C]); no sample may miss the condition."""
    out = []
    for b in range(probs.shape[0]):
        hyps, gap = R.beam_search(probs[b], W, normalized=True)
        assert gap >= R.MIN_GAP, (b, gap)
        out.append(list(hyps[0][0]))
    return conv.idx2str(out)


def check_update_scores(device):
    """TextAccuracy.update_scores with a beam convertor: the totals of the host update() on the oracle's strings; beam_width = 0 gives
    the records of today's greedy path, bit for bit."""
    import ctc_checks as K
    from ccd_amd import ops
    from ccd_amd.convertor.ctc import CTCConvertor
    from ccd_amd.metric.eval_acc import TextAccuracy, encode_truth
    probs = peaked(101, True)
    conv = CTCConvertor(beam_width=4)
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
    x = K.greedy_case().to(device)
    raw, norm = (torch.from_numpy(t).to(device) for t in conv.score_table())
    codes, lens = (torch.from_numpy(a).to(device) for a in encode_truth(K.GREEDY_TRUTH))
    plain = TextAccuracy().update_scores(x, list(K.GREEDY_TRUTH), CTCConvertor(beam_width=0))
    assert torch.equal(plain, ops.text_score_ctc(x, raw, norm, codes, lens))
