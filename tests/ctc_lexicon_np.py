"""The fp64 specification of lexicon-constrained CTC decoding (kernels/ctc_lexicon.h: ccd_ctc_lexicon_score, ccd_ctc_lexicon_best) in
plain numpy, and its inputs:
    word_score(lp, word)                  the CTC forward log-likelihood of one word under frame log-probabilities lp [T, C]
    score(x, words, normalized)           fp32 frames [T, C] + a list of words -> fp64 [V]
    best(scores, nbest)                   a score row -> [(column, score)] by (score descending, column ascending), -inf never chosen
    min_gap(scores, words)                the smallest difference between the scores of two different words of a row
    batch_lexicon(seed)                   the 70-word lexicon of the oracle-batch check

The specification.  Frame log-probabilities are those of ctc_beam_np.log_probs: a lexicon score and a beam score of the same word are
comparable numbers.  A word w of classes 1..C-1 with L labels has the states l' = (blank, w_1, blank, ..., w_L, blank), S = 2 L + 1;
    alpha_0(s) = lp[0, l'_s] for s < 2, -inf otherwise;
    alpha_t(s) = lse3(alpha_{t-1}(s), alpha_{t-1}(s - 1), alpha_{t-1}(s - 2) if s is odd, s >= 3 and l'_s != l'_{s-2}) + lp[t, l'_s];
    score = lse3(alpha_{T-1}(S - 1), alpha_{T-1}(S - 2) if S >= 2, -inf),
with lse3(a, b, c) = log(exp(a - m) + exp(b - m) + exp(c - m)) + m, m the largest of the three (0 where all are -inf: -inf stays -inf,
never NaN) - the grouping of kernels/ctc.h.  The score is -inf for a label outside [1, C), for L + adjacent equal labels > T, and where
every alignment meets a masked class.  L = 0 is the empty word: the sum of the blanks."""
import numpy as np

import ctc_beam_np as R

NEG = -np.inf
MIN_GAP = R.MIN_GAP


def lse3(a, b, c):
    m = max(a, b, c)
    if m == NEG:
        m = 0.0
    with np.errstate(divide="ignore"):
        return float(np.log(np.exp(a - m) + np.exp(b - m) + np.exp(c - m)) + m)


def feasible(word, T, C):
    word = list(word)
    if any(c < 1 or c >= C for c in word):
        return False
    return len(word) + sum(1 for a, b in zip(word, word[1:]) if a == b) <= T


def word_score(lp, word):
    """lp fp64 [T, C] (finite or -inf), word: a sequence of classes -> the log of the summed probability of its alignments."""
    T, C = lp.shape
    word = [int(c) for c in word]
    if not feasible(word, T, C):
        return NEG
    ext = [0]
    for c in word:
        ext += [c, 0]
    ext = np.array(ext)
    S = ext.size
    skip = np.array([s % 2 == 1 and s >= 3 and ext[s] != ext[s - 2] for s in range(S)])
    a = np.where(np.arange(S) < 2, lp[0, ext], NEG)
    with np.errstate(divide="ignore"):
        for t in range(1, T):                                                 # lse3 on every state at once
            a1 = np.concatenate(([NEG], a[:-1]))
            a2 = np.where(skip, np.concatenate(([NEG, NEG], a[:-2]))[:S], NEG)
            m = np.maximum(np.maximum(a, a1), a2)
            m = np.where(m == NEG, 0.0, m)
            a = np.log(np.exp(a - m) + np.exp(a1 - m) + np.exp(a2 - m)) + m + lp[t, ext]
    return lse3(a[S - 1], a[S - 2] if S >= 2 else NEG, NEG)


def score(x, words, normalized=False):
    """x fp32 [T, C], words: a list of class sequences -> fp64 [V]."""
    lp = R.log_probs(x, normalized)
    return np.array([word_score(lp, w) for w in words], dtype=np.float64).reshape(len(words))


def best(scores, nbest):
    """One row -> [(column, score)], at most nbest of them: score descending, column ascending among equals, -inf never."""
    scores = np.asarray(scores, dtype=np.float64)
    order = np.argsort(-scores, kind="stable")
    return [(int(k), float(scores[k])) for k in order[:nbest] if scores[k] > NEG]


def min_gap(scores, words):
    """The smallest |difference| between the finite scores of two DIFFERENT words of a row (a word listed twice is the tie case)."""
    first = {}
    for k, w in enumerate(words):
        first.setdefault(tuple(w), k)
    v = np.sort(np.array([scores[k] for k in first.values() if scores[k] > NEG]))
    return float(np.diff(v).min()) if v.size >= 2 else np.inf


def to_tensor(words, max_len=None):
    """A list of class sequences -> int64 [V, max_len] zero-padded (numpy); max_len defaults to the longest word, at least 1."""
    width = max(1, max(map(len, words), default=1)) if max_len is None else max_len
    out = np.zeros((len(words), width), dtype=np.int64)
    for row, w in zip(out, words):
        row[:len(w)] = list(w)
    return out


FIXED_WORDS = [(), (17,), (11, 11), (5,) * 17, tuple(1 + (i & 1) for i in range(31)), (3, 95, 4)]


def batch_lexicon(seed, B=9, T=32, C=92):
    """The lexicon of the oracle-batch check, V = 70, for R.peaked_batch(seed): per sample the ranks 1 and 2 (not rank 0) of the beam
    of width 4 over the logits and the rank-0 word with one class replaced; random words of length 1..19 up to 64 words; then
    FIXED_WORDS: the empty word, a repeat, (5,) * 17 (33 frames: infeasible at T = 32), 63 states, a class outside [1, C)."""
    rng = np.random.default_rng(1000 + seed)
    x = R.peaked_batch(seed, B, T, C)
    words = []
    for b in range(B):
        hyps, _ = R.beam_search(x[b], 4)
        words += [tuple(hyps[1][0]), tuple(hyps[2][0])]
        top = list(hyps[0][0])
        if top:
            at = int(rng.integers(0, len(top)))
            top[at] = 1 + (top[at] % 91)
        words.append(tuple(top))
    while len(words) < 64:
        words.append(tuple(int(c) for c in rng.integers(1, C, int(rng.integers(1, 20)))))
    return words[:64] + FIXED_WORDS
