"""The fp64 oracle of CTC prefix beam search fused with a character n-gram language model (kernels/ctc_beam.h: ctc_beam_kernel<true>,
ccd_ctc_beam_search_lm) in plain numpy, and its inputs:
    beam_search_lm(x, W, table, order, weight, bonus, eos, normalized)   the specification -> (hypotheses [(word, score)] by rank, gap)
    row_of(prefix, order, C)          the table row a prefix addresses
    word_term(word, table, ...)       what the language model adds to a whole word: Lambda(word), plus the end term with eos
    synthetic_table(seed, C, order)   a normalised random table, fp32 [C^(order-1), C]
    masked_table(seed, C, order, classes)   the same with the columns of `classes` at -inf in every row

The specification.  The table is lm fp32 [C^(order-1), C], row-major, order in 1..3.  The row of a prefix p is built from its last
order - 1 classes, the most recent last, a missing position being 0 (the blank's number: "start of word"): row 0 at order 1, p[-1] at
order 2, p[-2] * C + p[-1] at order 3.  Column c >= 1 is the log-probability of character c behind that context, column 0 that of the
word ending there (read only with eos).  Values are finite or -inf; rows need not be normalised.
The term of extending a prefix by c:
    g = -inf where lm[row, c] == -inf, else float64(weight) * float64(lm[row, c]) + float64(bonus)     (the product, then the sum)
with weight and bonus fp32.  Per frame everything is as ctc_beam_np.beam_search states it but for one thing: an extend candidate (i, c)
has pnb' = ((pb_i if c == last_i else tot_i) + lp[c]) + g(i, c), and that same number is what a merge log-adds into entry j's stay
candidate.  Stay candidates, the selection key and the tie rule are unchanged: pb and pnb of a prefix both carry Lambda(prefix), the sum
of g over its characters.
eos, behind the last frame: the score of every entry gets float64(weight) * float64(lm[row, 0]) (no bonus), -inf where the table says
-inf; the entries are ranked again by (score descending, previous rank ascending) - a `select` over the scores -, and a -inf entry is
no hypothesis any more.  The term never steers the pruning.  Without eos the order is the last selection's."""
import numpy as np

import ctc_beam_np as R
from beam_np import select

NEG = -np.inf


def row_of(prefix, order, C):
    if order == 1:
        return 0
    last = prefix[-1] if len(prefix) >= 1 else 0
    if order == 2:
        return last
    return (prefix[-2] if len(prefix) >= 2 else 0) * C + last


def _term(value, weight, bonus):
    """g of one table entry: fp64 product of the fp32 weight and the fp32 entry, then the fp32 bonus added in fp64."""
    if value == NEG:
        return NEG
    return np.float64(np.float32(weight)) * np.float64(value) + np.float64(np.float32(bonus))


def _terms(values, weight, bonus):
    """_term of every entry of a table row at once (the same fp64 operations, element by element)."""
    v = np.asarray(values, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        g = np.float64(np.float32(weight)) * v.astype(np.float64) + np.float64(np.float32(bonus))
    return np.where(v == NEG, NEG, g)


def word_term(word, table, order, weight, bonus, eos):
    """Lambda(word) = sum of g over the word's characters, plus weight * lm[row(word), 0] with eos - what the fused score of a word
    holds on top of log p_ctc(word)."""
    C = table.shape[1]
    total = 0.0
    for n, c in enumerate(word):
        total += _term(table[row_of(word[:n], order, C), c], weight, bonus)
    if eos:
        total += _term(table[row_of(word, order, C), 0], weight, 0.0)
    return float(total)


def beam_search_lm(x, W, table, order, weight=1.0, bonus=0.0, eos=False, normalized=False, ties=False, merge_lm=True):
    """x fp32 [T, C], table fp32 [C^(order-1), C] -> ([(word tuple, score)] by rank, at most W of them; the smallest gap of any
    selection, the eos re-rank included; inf when no selection had two candidates).  merge_lm=False is NOT the specification: it is
    the mistake of leaving g out of what a merge log-adds, for the test that shows its case would catch that."""
    lp = R.log_probs(x, normalized)
    T, C = lp.shape
    table = np.asarray(table, dtype=np.float32)
    assert order in (1, 2, 3) and table.shape == (C ** (order - 1), C) and not np.isnan(table).any()
    entries = [((), 0.0, NEG)]
    gap = np.inf
    for t in range(T):
        row = lp[t]
        n = len(entries)
        where = {e[0]: j for j, e in enumerate(entries)}
        tot = [R._lae(pb, pnb) for _, pb, pnb in entries]
        stay_pb = [tot[i] + row[0] for i in range(n)]
        stay_pnb = [entries[i][2] + row[entries[i][0][-1]] if entries[i][0] else NEG for i in range(n)]
        score = np.full((n, C), NEG)
        for i, (p, pb, pnb) in enumerate(entries):
            base = np.full(C, tot[i])
            if p:
                base[p[-1]] = pb
            lm_row = table[row_of(p, order, C)]
            g = _terms(lm_row, weight, bonus)
            score[i, 1:] = (base[1:] + row[1:]) + g[1:]
        for j, (p, _, _) in enumerate(entries):                                # merges: j absorbs (i, last_j) where prefix_i = prefix_j[:-1]
            i = where.get(p[:-1]) if p else None
            if i is not None:
                absorbed = score[i, p[-1]]
                if not merge_lm:                                               # (the mistake: the CTC part alone)
                    absorbed = (entries[i][1] if entries[i][0] and entries[i][0][-1] == p[-1] else tot[i]) + row[p[-1]]
                stay_pnb[j] = R._lae(stay_pnb[j], absorbed)
                score[i, p[-1]] = NEG
        for i in range(n):
            score[i, 0] = R._lae(stay_pb[i], stay_pnb[i])
        best, near = select(score, W, ties)
        gap = min(gap, near)
        nxt = []
        for k in best:
            i, c = divmod(int(k), C)
            p = entries[i][0]
            nxt.append((p, stay_pb[i], stay_pnb[i]) if c == 0 else (p + (c,), NEG, float(score[i, c])))
        entries = nxt
    hyps = [(p, R._lae(pb, pnb)) for p, pb, pnb in entries]
    if eos:
        final = np.array([s + _term(table[row_of(p, order, C), 0], weight, 0.0) for p, s in hyps], dtype=np.float64)
        best, near = select(final, len(hyps), ties)
        gap = min(gap, near)
        hyps = [(hyps[int(k)][0], float(final[int(k)])) for k in best]
    return hyps, gap


def synthetic_table(seed, C, order):
    """default_rng(seed).normal(0, 1.5) of shape [C^(order-1), C], log-softmaxed per row in fp64, cast to fp32."""
    t = np.random.default_rng(seed).normal(0.0, 1.5, (C ** (order - 1), C))
    m = t.max(axis=1, keepdims=True)
    t = (t - m) - np.log(np.exp(t - m).sum(axis=1, keepdims=True))
    return t.astype(np.float32)


def masked_table(seed, C, order, classes):
    """synthetic_table with the columns of `classes` at -inf in every row: a character that may never follow, or - class 0 - a word
    that may never end."""
    t = synthetic_table(seed, C, order)
    t[:, list(classes)] = NEG
    return t


def row_masked_table(seed, C, order):
    """synthetic_table with one fixed character per row at -inf: character 1 + row % (C - 1) never follows the context of that row."""
    t = synthetic_table(seed, C, order)
    rows = np.arange(t.shape[0])
    t[rows, 1 + rows % (C - 1)] = NEG
    return t
