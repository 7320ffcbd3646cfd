"""The fp64 specification of joint CTC / attention decoding (kernels/nrtr_joint.h: ccd_nrtr_joint_begin, ccd_nrtr_beam_step_joint) in
plain numpy, and its inputs.

The rules ("Joint CTC / attention decoding"):
  * decoder side as tests/nrtr_beam_np.py: C classes, end_idx, pad_idx, W slots per sample, each live, finished or unused; the
    attention score A of a slot is the fp64 sum of log_softmax64(logits)[token] over its steps;
  * CTC side: frames [Tc, Cc] per sample, lp = log_softmax64 per frame (or log of the row, `normalized`), blank = class 0; decoder
    class c != end_idx is CTC class k = c + class_offset;
  * every live slot carries the prefix state rn[Tc], rb[Tc]: the log-probability that the frames 0..t spell exactly the slot's prefix
    and end in a non-blank / in a blank.  Root: rn = -inf, rb[t] = lp[0, 0] + .. + lp[t, 0] in ascending order;
  * extension of prefix g (last CTC class `last`) by k:
        n[0] = lp[0, k] if g is empty else -inf;  b[0] = -inf
        phi[t] = rb[t - 1] if k == last else logaddexp(rn[t - 1], rb[t - 1])
        n[t] = logaddexp(n[t - 1], phi[t]) + lp[t, k];  b[t] = logaddexp(n[t - 1], b[t - 1]) + lp[t, 0]
        psi(g.k) = logsumexp(n[0], phi[1] + lp[1, k], .., phi[Tc - 1] + lp[Tc - 1, k])   the CTC output STARTS with g.k
    full(g) = logaddexp(rn[Tc - 1], rb[Tc - 1])                                          the CTC output IS g;
  * candidates of a live slot r, weight w in [0, 1]: (r, c), c != end_idx: S = (1 - w) (A_r + la[c]) + w psi(g_r.k); (r, end_idx): S =
    (1 - w) (A_r + la[end_idx]) + w full(g_r).  A candidate exists iff its attention part is finite and (w == 0 or its CTC part >
    -inf); a class with c + class_offset >= Cc has no CTC class.  At w == 0 the CTC term is dropped, not multiplied.  A finished slot
    gives (r, end_idx) with S and A unchanged;
  * selection, ties, tokens, parents and states are nrtr_beam_np's, applied to S; a selected extension takes (n, b) as its prefix
    state, a finished or carried slot keeps its parent's.

`gap` is nrtr_beam_np's: the smallest distance between neighbouring candidates of which one was kept."""
import itertools

import numpy as np

from beam_np import MIN_GAP, log_softmax64, select      # noqa: F401  (MIN_GAP: for the callers)
from nrtr_beam_np import FINISHED, LIVE, UNUSED

NEG = -np.inf


def lae(a, b):
    """log(exp(a) + exp(b)); -inf when both are."""
    m, lo = (a, b) if a > b else (b, a)
    return m if m == NEG else m + np.log1p(np.exp(lo - m))


def lse(xs):
    """log sum exp over a list, the maximum taken out, the sum in list order; -inf of nothing but -inf."""
    xs = np.asarray(xs, dtype=np.float64)
    m = xs.max()
    if m == NEG:
        return NEG
    return m + np.log(np.cumsum(np.exp(xs - m))[-1])


def frame_log_probs(frames, normalized=False):
    """frames fp32 [Tc, Cc] -> lp fp64 [Tc, Cc]."""
    if not normalized:
        return np.stack([log_softmax64(row) for row in frames])
    p = np.asarray(frames, dtype=np.float32).astype(np.float64)
    with np.errstate(divide="ignore"):
        num = np.where(p > 0, np.log(np.where(p > 0, p, 1.0)), NEG)
        total = np.array([np.cumsum(np.where(row > 0, row, 0.0))[-1] for row in p])
        return np.where(p > 0, num - np.log(total)[:, None], NEG)


def root_state(lp):
    """-> (rn, rb) of the empty prefix."""
    return np.full(lp.shape[0], NEG), np.cumsum(lp[:, 0])


def extend(lp, rn, rb, last, k, empty):
    """The prefix g (state rn, rb; last CTC class `last`; `empty`: g has no character) extended by CTC class k -> (n, b, psi)."""
    Tc = lp.shape[0]
    n, b = np.full(Tc, NEG), np.full(Tc, NEG)
    n[0] = lp[0, k] if empty else NEG
    terms = [n[0]]
    for t in range(1, Tc):
        phi = rb[t - 1] if k == last else lae(rn[t - 1], rb[t - 1])
        n[t] = lae(n[t - 1], phi) + lp[t, k]
        b[t] = lae(n[t - 1], b[t - 1]) + lp[t, 0]
        terms.append(phi + lp[t, k])
    return n, b, lse(terms)


def psi_all(lp, rn, rb, last, ks, empty):
    """psi(g.k) of `extend` for all the CTC classes ks at once (the same terms in the same order, as numpy vectors)."""
    Tc = lp.shape[0]
    phi = np.full((Tc, len(ks)), NEG)
    phi[0] = 0.0 if empty else NEG                                             # n[0] = lp[0, k] for the empty prefix
    for t in range(1, Tc):
        phi[t] = np.where(ks == last, rb[t - 1], lae(rn[t - 1], rb[t - 1]))
    terms = phi + lp[:, ks]
    m = terms.max(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = m + np.log(np.cumsum(np.exp(terms - m), axis=0)[-1])
    return np.where(m == NEG, NEG, out)


def full(rn, rb):
    return lae(rn[-1], rb[-1])


def prefix_scores(lp, word):
    """A word of CTC classes -> (psi(word), full(word)) by the recursion from the root; psi of the empty word is 0 (every output
    starts with it)."""
    rn, rb = root_state(lp)
    psi, last = 0.0, -1
    for i, k in enumerate(word):
        rn, rb, psi = extend(lp, rn, rb, last, k, i == 0)
        last = k
    return psi, full(rn, rb)


def enumerate_alignments(lp):
    """Every alignment of the Tc frames -> {collapsed word: log-probability}, by brute force."""
    Tc, Cc = lp.shape
    out = {}
    for ali in itertools.product(range(Cc), repeat=Tc):
        word, prev = [], 0
        for k in ali:
            if k != 0 and k != prev:
                word.append(k)
            prev = k
        p = float(sum(lp[t, k] for t, k in enumerate(ali)))
        word = tuple(word)
        out[word] = lae(out[word], p) if word in out else p
    return out


class JointSample:
    """The W slots of one sample."""

    def __init__(self, W, start_idx, lp, weight, class_offset=1):
        self.W, self.lp, self.w, self.off = W, lp, float(weight), class_offset
        self.seqs = [[start_idx] for _ in range(W)]
        self.score = np.full(W, NEG)
        self.score[0] = 0.0
        self.att = self.score.copy()
        self.state = [LIVE] + [UNUSED] * (W - 1)
        self.pre = [root_state(lp) for _ in range(W)]

    def step(self, logits, end_idx, pad_idx, ties=False):
        """logits [W, C] fp32 (rows of slots that are not live are not read) -> (parent [W], gap)."""
        W, C, w, lp = self.W, logits.shape[1], self.w, self.lp
        Cc = lp.shape[1]
        cand = np.full((W, C), NEG)
        attc = np.full((W, C), NEG)
        for r in range(W):
            if self.state[r] == LIVE:
                attc[r] = self.att[r] + log_softmax64(logits[r])
                if w == 0:
                    cand[r] = attc[r]
                    continue
                rn, rb = self.pre[r]
                empty = len(self.seqs[r]) == 1
                ctc = np.full(C, NEG)
                ks = np.array([c + self.off for c in range(C) if c != end_idx and c + self.off < Cc], dtype=np.int64)
                ctc[ks - self.off] = psi_all(lp, rn, rb, -1 if empty else self.seqs[r][-1] + self.off, ks, empty)
                ctc[end_idx] = full(rn, rb)
                ok = (attc[r] > NEG) & (ctc > NEG)
                with np.errstate(invalid="ignore"):
                    cand[r] = np.where(ok, (1 - w) * attc[r] + w * ctc, NEG)
            elif self.state[r] == FINISHED:
                cand[r, end_idx] = self.score[r]
                attc[r, end_idx] = self.att[r]
        best, gap = select(cand, W, ties)
        dead = (np.full(lp.shape[0], NEG), np.full(lp.shape[0], NEG))
        seqs, score, att, state, parent, pre = [], np.full(W, NEG), np.full(W, NEG), [UNUSED] * W, [-1] * W, []
        for n in range(W):
            if n < len(best):
                r, c = divmod(int(best[n]), C)
                done = self.state[r] == FINISHED
                seqs.append(self.seqs[r] + [pad_idx if done else c])
                score[n], att[n], parent[n] = cand[r, c], attc[r, c], r
                state[n] = FINISHED if done or c == end_idx else LIVE
                if state[n] == FINISHED:
                    pre.append(self.pre[r])
                elif c + self.off < Cc:
                    rn, rb = self.pre[r]
                    empty = len(self.seqs[r]) == 1
                    pre.append(extend(lp, rn, rb, -1 if empty else self.seqs[r][-1] + self.off, c + self.off, empty)[:2])
                else:
                    pre.append(dead)
            else:
                seqs.append(self.seqs[n] + [pad_idx])
                pre.append(dead)
        self.seqs, self.score, self.att, self.state, self.pre = seqs, score, att, state, pre
        return parent, gap

    def outputs(self, end_idx, T):
        """-> (paths [W, T] -1-padded, lengths [W], scores [W] fp64, att_scores [W] fp64)."""
        paths, lengths = np.full((self.W, T), -1, dtype=np.int32), np.full(self.W, -1, dtype=np.int32)
        for r in range(self.W):
            if self.state[r] == UNUSED:
                continue
            body = self.seqs[r][1:]
            n = body.index(end_idx) if end_idx in body else len(body)
            paths[r, :n] = body[:n]
            lengths[r] = n
        return paths, lengths, self.score.copy(), self.att.copy()


def beam_search(table, frames, W, start_idx, end_idx, pad_idx, weight, class_offset=1, normalized=False, ties=False):
    """One sample.  table fp32 [T, C + 1, C] as nrtr_beam_np.beam_search's, frames fp32 [Tc, Cc] -> (paths, lengths, scores,
    att_scores, parents [T, W], gap, prefix states [W, 2, Tc])."""
    T = table.shape[0]
    smp = JointSample(W, start_idx, frame_log_probs(frames, normalized), weight, class_offset)
    parents, gap = [], np.inf
    for s in range(T):
        logits = np.stack([table[s, smp.seqs[r][-1]] for r in range(W)])
        parent, g = smp.step(logits, end_idx, pad_idx, ties)
        parents.append(parent)
        gap = min(gap, g)
    return smp.outputs(end_idx, T) + (np.asarray(parents, dtype=np.int32), gap, np.asarray(smp.pre))


def brute_force(table, frames, start_idx, end_idx, weight, class_offset=1):
    """Every hypothesis of one sample with its exact joint score - a finished word: (1 - w) A + w full(word); one that ran to T
    classes: (1 - w) A + w psi(word) - by score descending -> [(word, S, A, finished)]."""
    import nrtr_beam_np as R
    lp = frame_log_probs(frames)
    out = []
    for word, a, finished in R.brute_force(table, start_idx, end_idx):
        ks = [c + class_offset for c in word]
        if any(k >= lp.shape[1] for k in ks):
            continue
        psi, fl = prefix_scores(lp, ks)
        t = fl if finished else psi
        if t > NEG and a > NEG:
            out.append((word, (1 - weight) * a + weight * t, a, finished))
    out.sort(key=lambda t: -t[1])
    return out


def frames_of(seed, B, Tc, Cc, pad=3):
    """fp32 [B, Tc, Cc + pad]: 2 * standard_normal with 5 added to the blank logit, NaN behind column Cc (a padded row stride)."""
    rng = np.random.RandomState(seed)
    f = np.full((B, Tc, Cc + pad), np.nan, dtype=np.float32)
    f[:, :, :Cc] = (2.0 * rng.standard_normal((B, Tc, Cc))).astype(np.float32)
    f[:, :, 0] += np.float32(5.0)
    return f


# the kernel-level cases (B, W, C, T, mode, Tc, w, normalized); Cc = C.  Every Tc meets W = 16 and C = 128 once.
CASES = [
    (5, 8, 92, 25, "end", 32, 0.3, False),
    (5, 16, 65, 25, "end", 32, 0.7, False),
    (5, 16, 65, 25, "end", 1, 0.3, False),
    (5, 3, 128, 25, "end", 32, 0.7, False),
    (5, 3, 128, 25, "end", 1, 0.3, False),
    (5, 3, 128, 25, "end", 33, 0.3, True),
    (5, 3, 128, 25, "end", 64, 0.7, False),
    (5, 16, 64, 25, "flat", 33, 0.7, False),
    (5, 16, 64, 25, "flat", 64, 0.3, False),
    (5, 2, 3, 4, "flat", 32, 0.3, False),
    (5, 16, 3, 6, "flat", 32, 0.7, False),
    (5, 16, 3, 6, "flat", 33, 0.3, True),
    (1, 1, 92, 25, "end", 32, 0.7, False),
]
