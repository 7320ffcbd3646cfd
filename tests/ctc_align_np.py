"""The fp64 oracle of CTC forced alignment (kernels/ctc_align.h, ccd_ctc_align) in plain numpy, and its inputs:
    align(x, word, normalized)        the specification -> Alignment(score, frame_char, spans, char_logp, margin), None when infeasible
    brute_force(x, word, normalized)  every frame path that collapses to the word -> (best score, [the paths that reach it])
    path_of(frame_char, word)         frame_char -> the class of every frame (0 = blank)
    valid(frame_char, word)           is frame_char an alignment of the word at all
    stay_first(paths)                 of paths of equal score, the one the tie rule names

The specification.  lp = ctc_beam_np.log_probs (the beam's and the lexicon's: fp64 over the fp32 row, the sum over the classes in ascending
order, a zero probability or a -inf logit masks a class).  Over the extended sequence l' = (blank, l_1, blank, ..., l_L, blank), S = 2 L + 1:
    v_0(s) = lp[0, l'_s] for s < 2, -inf behind
    v_t(s) = max(v_{t-1}(s), v_{t-1}(s - 1), v_{t-1}(s - 2) where l'_s is a label that differs from l'_{s-2}) + lp[t, l'_s]
Tie rule: the candidates are taken in the order s, s - 1, s - 2 and a later one replaces the current one only if it is STRICTLY greater; the
path ends in state S - 1 unless v(S - 2) is strictly greater.  score = v at the end state (the sum of lp along the path in frame order);
char_logp[j] = the sum of lp over the frames of character j in ascending frame order.  Infeasible (None): a label outside [1, C),
L + adjacent equal labels > T, no alignment of finite probability.

The margin of a row is the smallest gap between the winner and the runner-up over the decisions ON THE BEST PATH, the final one included
(inf where a decision had one finite candidate): where it is large, a kernel whose fp64 numbers differ in the last bits must still return
the same integers."""
import collections
import itertools

import numpy as np

from ctc_beam_np import collapse, log_probs

NEG = -np.inf
MIN_MARGIN = 1e-9            # exact integers are required where the margin is at least this
SEEDED_MARGIN = 1e-6         # ... and every seeded row is asserted to have at least this

Alignment = collections.namedtuple("Alignment", "score frame_char spans char_logp margin")


def feasible(word, T, C):
    word = tuple(word)
    repeats = sum(1 for a, b in zip(word, word[1:]) if a == b)
    return all(1 <= c < C for c in word) and len(word) + repeats <= T


def align(x, word, normalized=False):
    """x fp32 [T, C], word a tuple of classes -> Alignment or None."""
    x = np.asarray(x, dtype=np.float32)
    T, C = x.shape
    word = tuple(int(c) for c in word)
    if not feasible(word, T, C):
        return None
    lp = log_probs(x, normalized)
    L = len(word)
    S = 2 * L + 1
    ext = [0] * S
    ext[1::2] = word
    skip = [s >= 3 and (s & 1) == 1 and ext[s] != ext[s - 2] for s in range(S)]
    v = np.full(S, NEG)
    v[:min(2, S)] = [lp[0, ext[s]] for s in range(min(2, S))]
    back = np.zeros((T, S), dtype=np.int64)
    gaps = np.full((T, S), np.inf)
    for t in range(1, T):
        new = np.full(S, NEG)
        for s in range(S):
            cand = [v[s]]
            if s >= 1:
                cand.append(v[s - 1])
            if skip[s]:
                cand.append(v[s - 2])
            best, k = cand[0], 0
            for i in range(1, len(cand)):
                if cand[i] > best:
                    best, k = cand[i], i
            back[t, s] = k
            rest = [c for i, c in enumerate(cand) if i != k]
            if rest and best > NEG and max(rest) > NEG:
                gaps[t, s] = best - max(rest)
            new[s] = best + lp[t, ext[s]]
        v = new
    end, margin = S - 1, np.inf
    if S >= 2:
        if v[S - 2] > v[S - 1]:
            end = S - 2
        hi, lo = max(v[S - 1], v[S - 2]), min(v[S - 1], v[S - 2])
        if lo > NEG:
            margin = hi - lo
    score = v[end]
    if not score > NEG:
        return None
    states = np.zeros(T, dtype=np.int64)
    s = end
    for t in range(T - 1, -1, -1):
        states[t] = s
        margin = min(margin, gaps[t, s])
        s -= back[t, s]
    frame_char = np.where(states & 1, states >> 1, -1).astype(np.int32)
    spans = np.full((L, 2), -1, dtype=np.int32)
    char_logp = np.zeros(L)
    for t in range(T):                                                         # ascending frame order
        j = frame_char[t]
        if j >= 0:
            if spans[j, 0] < 0:
                spans[j, 0] = t
            spans[j, 1] = t
            char_logp[j] += lp[t, word[j]]
    return Alignment(float(score), frame_char, spans, char_logp, float(margin))


def path_of(frame_char, word):
    return tuple(0 if j < 0 else word[j] for j in frame_char)


def valid(frame_char, word):
    """frame_char is an alignment of the word: the characters 0..L-1 in order, each on a contiguous run, equal neighbours apart."""
    word = tuple(word)
    kept = [j for t, j in enumerate(frame_char) if j >= 0 and (t == 0 or frame_char[t - 1] != j)]
    return kept == list(range(len(word))) and all(-1 <= j < len(word) for j in frame_char) and collapse(path_of(frame_char, word)) == word


def path_score(x, frame_char, word, normalized=False):
    lp = log_probs(x, normalized)
    total = 0.0
    for t, c in enumerate(path_of(frame_char, word)):
        total += lp[t, c]
    return total


def brute_force(x, word, normalized=False):
    """Every one of the C^T frame paths that collapses to the word -> (the best summed lp, the paths that reach it exactly); (-inf, [])
    where none has finite probability."""
    lp = log_probs(x, normalized)
    T, C = lp.shape
    word = tuple(word)
    best, paths = NEG, []
    for a in itertools.product(range(C), repeat=T):
        if collapse(a) != word:
            continue
        total = 0.0
        for t, c in enumerate(a):
            total += lp[t, c]
        if total > best:
            best, paths = total, [a]
        elif total == best and total > NEG:
            paths.append(a)
    return best, paths


def stay_first(paths):
    """Of paths of equal score, the one the tie rule names.  At every frame, walking from the last one down, the rule prefers to have
    stayed in the state over having come from s - 1, and that over s - 2; at the end it prefers the trailing blank.  In terms of the state
    sequence: the lexicographically LARGEST sequence of states read from the last frame to the first."""
    def states(a):
        out, runs = [], 0
        for t, c in enumerate(a):
            runs += c != 0 and (t == 0 or a[t - 1] != c)                       # a run of a character begins
            out.append(2 * runs - 1 if c else 2 * runs)
        return out
    return max(paths, key=lambda a: states(a)[::-1])

