"""The fp64 specification of beam search over the NRTR attention decoder (kernels/nrtr_beam.h, ccd_nrtr_beam_step) in plain numpy,
and its inputs.

The rules ("Beam search over the NRTR decoder"):
  * C decoder outputs, end_idx < C, padding_idx; T steps; W slots per sample, ordered by rank;
  * a slot: a token sequence that starts with start_idx, an fp64 score = the sum of log_softmax(logits)[token] over its steps, and a
    state - live, finished or unused.  Before step 0: slot 0 live with score 0, the others unused with score -inf;
  * candidates at a step: a live slot r gives (r, c) for every class c with score[r] + log_softmax(logits[r])[c], the log-softmax in
    fp64 over the fp32 row (the sum over the classes in ascending order); a finished slot gives (r, end_idx) alone, score unchanged,
    still finished, padding_idx written; an unused slot gives none.  A candidate of score -inf (a -inf logit) is no candidate;
  * the new slots are the W best by (score descending, r * C + c ascending); fewer candidates leave unused slots; class end_idx
    finishes a hypothesis and the end_idx token is written;
  * after T steps: paths = the classes in front of the first end_idx, lengths (T if never finished, -1 unused), scores (-inf unused).

`gap` is the oracle's own smallest distance between two neighbouring candidates of which at least one was kept (kept against
dropped decides the set, kept against kept the ranks; beam_np.select): a case is only compared where it is >= MIN_GAP."""
import itertools

import numpy as np

from beam_np import MIN_GAP, log_softmax64, select      # noqa: F401  (MIN_GAP: for the callers)

UNUSED, LIVE, FINISHED = 0, 1, 2


class Sample:
    """The W slots of one sample."""

    def __init__(self, W, start_idx):
        self.W = W
        self.seqs = [[start_idx] for _ in range(W)]
        self.score = np.full(W, -np.inf)
        self.score[0] = 0.0
        self.state = [LIVE] + [UNUSED] * (W - 1)

    def step(self, logits, end_idx, pad_idx, ties=False):
        """logits [W, C] fp32 (rows of slots that are not live are not read) -> (parent [W], gap)."""
        W, C = self.W, logits.shape[1]
        cand = np.full((W, C), -np.inf)                          # candidate (r, c) at k = r * C + c
        for r in range(W):
            if self.state[r] == LIVE:
                cand[r] = self.score[r] + log_softmax64(logits[r])
            elif self.state[r] == FINISHED:
                cand[r, end_idx] = self.score[r]
        best, gap = select(cand, W, ties)
        seqs, score, state, parent = [], np.full(W, -np.inf), [UNUSED] * W, [-1] * W
        for n in range(W):
            if n < len(best):
                r, c = divmod(int(best[n]), C)
                done = self.state[r] == FINISHED
                seqs.append(self.seqs[r] + [pad_idx if done else c])
                score[n], parent[n] = cand[r, c], r
                state[n] = FINISHED if done or c == end_idx else LIVE
            else:
                seqs.append(self.seqs[n] + [pad_idx])            # an unused slot keeps its row and takes the padding token
        self.seqs, self.score, self.state = seqs, score, state
        return parent, gap

    def outputs(self, end_idx, T):
        """-> (paths [W, T] -1-padded, lengths [W], scores [W] fp64)."""
        paths, lengths = np.full((self.W, T), -1, dtype=np.int32), np.full(self.W, -1, dtype=np.int32)
        for r in range(self.W):
            if self.state[r] == UNUSED:
                continue
            body = self.seqs[r][1:]
            n = body.index(end_idx) if end_idx in body else len(body)
            paths[r, :n] = body[:n]
            lengths[r] = n
        return paths, lengths, self.score.copy()


def beam_search(table, W, start_idx, end_idx, pad_idx, ties=False):
    """One sample.  table fp32 [T, C + 1, C]: the logits of a slot at step s are table[s, its last token] (a Markov model; row C is
    the padding token's, never read).  -> (paths, lengths, scores, parents [T, W], gap)."""
    T = table.shape[0]
    smp = Sample(W, start_idx)
    parents, gap = [], np.inf
    for s in range(T):
        logits = np.stack([table[s, smp.seqs[r][-1]] for r in range(W)])
        parent, g = smp.step(logits, end_idx, pad_idx, ties)
        parents.append(parent)
        gap = min(gap, g)
    return smp.outputs(end_idx, T) + (np.asarray(parents, dtype=np.int32), gap)


def greedy(table, start_idx, end_idx):
    """The arg-max chain (first maximum) of one sample -> (word in front of the first end_idx, score with the end term)."""
    T = table.shape[0]
    prev, word, score = start_idx, [], 0.0
    for s in range(T):
        row = table[s, prev]
        c = int(np.argmax(row))
        score += log_softmax64(row)[c]
        if c == end_idx:
            return word, score
        word.append(c)
        prev = c
    return word, score


def brute_force(table, start_idx, end_idx):
    """Every hypothesis of one sample - a word shorter than T closed by end_idx, or T classes without one - with its exact score,
    by (score descending, order of first difference ascending) -> [(word, score, finished)]."""
    T, _, C = table.shape
    out = []

    def walk(s, prev, word, score):
        if s == T:
            out.append((tuple(word), score, False))
            return
        lp = log_softmax64(table[s, prev])
        for c in range(C):
            if c == end_idx:
                out.append((tuple(word), score + lp[c], True))
            else:
                walk(s + 1, c, word + [c], score + lp[c])

    walk(0, start_idx, [], 0.0)
    out.sort(key=lambda t: -t[1])
    return out


def markov_table(seed, T, C, mode="flat", scale=2.0):
    """fp32 [T, C + 1, C].  "flat": normal logits - without a length penalty every hypothesis of a beam finishes within a few steps.
    "end": every row also has a peak of 6 on one class, the end class C - 1 in 6 % of the rows and 1 added to every end logit, so
    that words end anywhere between the first and the last step and finished slots sit next to live ones for many steps."""
    rng = np.random.RandomState(seed)
    t = (rng.standard_normal((T, C + 1, C)) * scale).astype(np.float32)
    if mode == "end":
        peak = np.where(rng.random_sample((T, C + 1)) < 0.06, C - 1, rng.randint(0, C, (T, C + 1)))
        np.put_along_axis(t, peak[..., None], np.take_along_axis(t, peak[..., None], 2) + np.float32(6.0), 2)
        t[:, :, C - 1] += np.float32(1.0)
    else:
        assert mode == "flat"
    return t


def tables(seed, B, T, C, mode="flat"):
    return np.stack([markov_table(seed * 131 + b, T, C, mode) for b in range(B)])


# the kernel-level cases: every (W, C) pair once, B and T alternating so that each value meets each width and class count
WIDTHS, CLASSES = (1, 2, 3, 8, 16), (3, 64, 65, 92, 128)
_BT = ((1, 4), (5, 25), (5, 4), (1, 25))
CASES = [(B, W, C, T) for n, (W, C) in enumerate(itertools.product(WIDTHS, CLASSES)) for B, T in (_BT[n % 4],)]
END_HEAVY = [(5, 8, 92, 25, "end"), (5, 16, 65, 25, "end"), (5, 3, 128, 25, "end")]          # (B, W, C, T, mode)
