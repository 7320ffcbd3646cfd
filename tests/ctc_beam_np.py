"""The fp64 oracle of CTC prefix beam search (kernels/ctc_beam.h, ccd_ctc_beam_search) in plain numpy, and its inputs:
    log_probs(x, normalized)          fp32 frames [T, C] -> fp64 log-probabilities, -inf where a class is masked
    beam_search(x, W, normalized)     the specification -> (hypotheses [(word, score)] by rank, smallest score gap)
    brute_force(x, normalized)        every one of the C^T alignments, summed per collapsed word -> [(word, score)] by score
    peaked_batch(seed)                the moderately peaked [9, 32, 92] inputs of the tests

The specification.  A beam entry is a prefix of classes 1..C-1 with pb / pnb, the log mass of its alignments that end in the blank / in
a non-blank; entries are ordered by rank; the start is the empty prefix with pb = 0, pnb = -inf.  Per frame, with
tot_i = logaddexp(pb_i, pnb_i):
    stay (i, 0):     the same prefix, pb' = tot_i + lp[0], pnb' = pnb_i + lp[last_i] (-inf for the empty prefix);
    extend (i, c):   prefix_i + c, pb' = -inf, pnb' = (pb_i if c == last_i else tot_i) + lp[c], c = 1..C-1;
    merge:           an extend candidate that spells the prefix of a live entry j is log-added into the pnb' of j's stay candidate and
                     disappears (prefixes are unique: j absorbs at most one, and no two extend candidates coincide);
    select:          the W best candidates of finite score logaddexp(pb', pnb') by (score descending, k = rank * C + class ascending).
The gap returned is the smallest one of any frame's selection (beam_np.select; callers assert >= MIN_GAP)."""
import itertools

import numpy as np

from beam_np import MIN_GAP, log_softmax64, select      # noqa: F401  (MIN_GAP: for the callers)

NEG = -np.inf


def _lae(a, b):
    m = max(a, b)
    if m == NEG:
        return NEG
    return m + np.log1p(np.exp(min(a, b) - m))


def log_probs(x, normalized):
    """x fp32 [T, C]: logits (normalized False: beam_np.log_softmax64 of every frame) or probabilities (True: log p - log sum p,
    computed in fp64 from the fp32 values, the sum over the classes in ascending order; a zero probability gives -inf)."""
    x = np.asarray(x, dtype=np.float32)
    if not normalized:
        return np.stack([log_softmax64(frame) for frame in x])
    x64 = x.astype(np.float64)
    out = np.full(x.shape, NEG)
    for t in range(x.shape[0]):
        live = x[t] > 0
        total = np.cumsum(np.where(live, x64[t], 0.0))[-1]                     # ascending class order
        if live.any():
            out[t, live] = np.log(x64[t, live]) - np.log(total)
    return out


def beam_search(x, W, normalized=False, ties=False):
    """x fp32 [T, C] -> ([(word tuple, score)] by rank, at most W of them; the smallest gap, inf when no frame had two candidates)."""
    lp = log_probs(x, normalized)
    T, C = lp.shape
    entries = [((), 0.0, NEG)]
    gap = np.inf
    for t in range(T):
        row = lp[t]
        n = len(entries)
        where = {e[0]: j for j, e in enumerate(entries)}
        tot = [_lae(pb, pnb) for _, pb, pnb in entries]
        stay_pb = [tot[i] + row[0] for i in range(n)]
        stay_pnb = [entries[i][2] + row[entries[i][0][-1]] if entries[i][0] else NEG for i in range(n)]
        score = np.full((n, C), NEG)
        for i, (p, pb, pnb) in enumerate(entries):
            base = np.full(C, tot[i])
            if p:
                base[p[-1]] = pb
            score[i, 1:] = base[1:] + row[1:]
        for j, (p, _, _) in enumerate(entries):                                # merges: j absorbs (i, last_j) where prefix_i = prefix_j[:-1]
            i = where.get(p[:-1]) if p else None
            if i is not None:
                stay_pnb[j] = _lae(stay_pnb[j], score[i, p[-1]])
                score[i, p[-1]] = NEG
        for i in range(n):
            score[i, 0] = _lae(stay_pb[i], stay_pnb[i])
        best, near = select(score, W, ties)
        gap = min(gap, near)
        nxt = []
        for k in best:
            i, c = divmod(int(k), C)
            p = entries[i][0]
            nxt.append((p, stay_pb[i], stay_pnb[i]) if c == 0 else (p + (c,), NEG, float(score[i, c])))
        entries = nxt
    return [(p, _lae(pb, pnb)) for p, pb, pnb in entries], gap


def collapse(alignment):
    word, before = [], 0
    for c in alignment:
        if c != 0 and c != before:
            word.append(c)
        before = c
    return tuple(word)


def brute_force(x, normalized=False):
    """x fp32 [T, C], C^T small -> [(word, log of the summed probability of its alignments)] by (score descending, word)."""
    lp = log_probs(x, normalized)
    T, C = lp.shape
    mass = {}
    for a in itertools.product(range(C), repeat=T):
        mass.setdefault(collapse(a), []).append(sum(lp[t, c] for t, c in enumerate(a)))
    words = []
    for w, v in mass.items():
        v = np.array(v)
        m = v.max()
        if m > NEG:
            words.append((w, float(m + np.log(np.exp(v - m).sum()))))
    return sorted(words, key=lambda e: (-e[1], e[0]))


def peaked_batch(seed, B=9, T=32, C=92):
    """normal(0, 1) fp32 [B, T, C]; per (b, t) in order uniform(2, 8) is added to a random class with probability 0.6 and to the blank
    otherwise: a recogniser's moderately peaked frames.  Seeds 100..102 give gaps >= 1.8e-6 at W in {1, 4, 16}, logits or their fp32
    softmax (tests/test_ctc_beam_cpu.py asserts the condition, >= 1e-9, for every sample)."""
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 1.0, (B, T, C)).astype(np.float32)
    for b in range(B):
        for t in range(T):
            c = int(rng.integers(0, C))
            x[b, t, c if rng.random() < 0.6 else 0] += np.float32(rng.uniform(2.0, 8.0))
    return x


def softmax32(x):
    """The fp32 softmax a CTC head hands out (CTCDecoder.forward_test), computed by torch on the CPU."""
    import torch
    return torch.from_numpy(np.asarray(x, dtype=np.float32)).softmax(-1).numpy()


def small_case(T, C, seed):
    return (np.random.default_rng(seed).normal(0.0, 1.5, (T, C))).astype(np.float32)


EXHAUSTIVE = ((3, 3), (4, 2), (6, 2))          # (T, C): 9, 3 and 4 words, every one fits a beam of 16
