"""The fp64 oracle of CTC prefix beam search along the prefix tree of a lexicon (kernels/ctc_beam.h: ctc_beam_kernel<CTC_BEAM_TRIE>,
ccd_ctc_beam_search_trie) in plain numpy, a reference trie builder, and its inputs:
    build_trie(words)                         the node table int32 [n_nodes, 8], by a plain-Python dictionary builder
    child(nodes, node, c), allowed(nodes, node, C)   popcount addressing and the mask bits of a node
    beam_search_trie(x, W, nodes, normalized) the specification -> (hypotheses [(word, score, word_id)] by rank, gap)
    search(x, W, nodes, words, normalized)    the two-stage decoder: the proposals, scored exactly -> [(word_id, exact score)] by rank
    batch_lexicon(seed, normalized)           the peaked batch and its lexicon of about 1 500 words

The node table.  32 bytes per node: words 0..3 the 128-bit child mask (bit c & 31 of word c >> 5 is set iff the node has a child by
class c; bit 0 never), word 4 first_child (the node of the child with the lowest class; 0 for a leaf), word 5 word_id (the row of the
word list that ends here, of duplicate rows the lowest, or -1), word 6 the parent (-1 for the root), word 7 the class on the edge from
the parent (0 for the root).  Breadth-first: the root is node 0, the children of a node are contiguous in ascending class order, so the
child by class c is first_child + popcount(mask bits below c).  A row ends at its first zero; an all-zero row makes the root terminal; an
empty list is the root alone; a word with a class outside 1..127 is left out (no scores have such a class).

The specification.  Everything is as ctc_beam_np.beam_search states it, with these additions:
    every beam entry carries a node; the empty prefix carries node 0;
    an extend candidate (i, c) exists iff bit c of mask[node_i] is set, otherwise it is -inf: never selected, never merged; the bits of
    classes >= C are never looked at;
    the score of an allowed extension is the plain beam's, (pb_i if c == last_i else tot_i) + lp[c], with no added term;
    a selected extension carries child(node_i, c), a stay keeps the node; merges work as in the plain beam (the node is a function of
    the prefix: an absorbed candidate and its absorber agree on it);
    behind the last frame the score of an entry is logaddexp(pb, pnb) if word_id[node] >= 0, else -inf; the entries are ranked again by
    (score descending, previous rank ascending) - a `select` over the scores, whose gap counts -, and a -inf entry is no hypothesis.
Prefixes that end no word compete for the beam's slots during the search: with W = 1 most samples end with no word at all."""
import numpy as np

import ctc_beam_np as R
import ctc_lexicon_np as X
from beam_np import select

NEG = -np.inf
NODE_WORDS = 8


def _cut(word):
    """The classes of a row in front of its first zero."""
    out = []
    for c in word:
        if int(c) == 0:
            break
        out.append(int(c))
    return tuple(out)


def build_trie(words):
    """A list of class sequences (or zero-padded rows) -> int32 [n_nodes, 8]: dictionaries first, then numbered breadth-first."""
    kids, word_id = [{}], [-1]
    for row, w in enumerate(words):
        w = _cut(w)
        if any(c < 1 or c > 127 for c in w):
            continue
        node = 0
        for c in w:
            if c not in kids[node]:
                kids[node][c] = len(kids)
                kids.append({})
                word_id.append(-1)
            node = kids[node][c]
        if word_id[node] < 0:
            word_id[node] = row
    order, parent, edge = [0], [-1], [0]
    for at in range(len(kids)):                                                # `order` grows while it is walked: breadth-first
        if at >= len(order):
            break
        for c in sorted(kids[order[at]]):
            order.append(kids[order[at]][c])
            parent.append(at)
            edge.append(c)
    number = {old: new for new, old in enumerate(order)}
    nodes = np.zeros((len(order), NODE_WORDS), dtype=np.int64)
    for new, old in enumerate(order):
        for c in kids[old]:
            nodes[new, c >> 5] |= 1 << (c & 31)
        nodes[new, 4] = min((number[k] for k in kids[old].values()), default=0)
        nodes[new, 5], nodes[new, 6], nodes[new, 7] = word_id[old], parent[new], edge[new]
    nodes[:, :4] = np.where(nodes[:, :4] >= 2 ** 31, nodes[:, :4] - 2 ** 32, nodes[:, :4])     # the bit patterns as int32
    return nodes.astype(np.int32)


def mask_of(nodes, node):
    """The 128-bit child mask of a node as a Python int."""
    return sum((int(nodes[node, k]) & 0xFFFFFFFF) << (32 * k) for k in range(4))


def allowed(nodes, node, C):
    """bool [C]: the node has a child by class c (bits of classes >= C are not looked at)."""
    m = mask_of(nodes, node)
    return np.array([(m >> c) & 1 == 1 for c in range(C)])


def child(nodes, node, c):
    m = mask_of(nodes, node)
    assert (m >> c) & 1
    return int(nodes[node, 4]) + bin(m & ((1 << c) - 1)).count("1")


def node_of(nodes, word):
    """The node a word's classes lead to, or None where the trie has no such path."""
    node = 0
    for c in word:
        if not (mask_of(nodes, node) >> c) & 1:
            return None
        node = child(nodes, node, c)
    return node


def beam_search_trie(x, W, nodes, normalized=False, ties=False):
    """x fp32 [T, C], nodes int32 [n_nodes, 8] -> ([(word tuple, score, word id)] by rank, at most W of them; the smallest gap of any
    selection, the final re-rank included; inf when no selection had two candidates)."""
    lp = R.log_probs(x, normalized)
    T, C = lp.shape
    entries = [((), 0.0, NEG, 0)]
    gap = np.inf
    masks = {}                                                                 # allowed(node), looked up once per node
    for t in range(T):
        row = lp[t]
        n = len(entries)
        where = {e[0]: j for j, e in enumerate(entries)}
        tot = [R._lae(pb, pnb) for _, pb, pnb, _ in entries]
        stay_pb = [tot[i] + row[0] for i in range(n)]
        stay_pnb = [entries[i][2] + row[entries[i][0][-1]] if entries[i][0] else NEG for i in range(n)]
        score = np.full((n, C), NEG)
        for i, (p, pb, pnb, node) in enumerate(entries):
            base = np.full(C, tot[i])
            if p:
                base[p[-1]] = pb
            ok = masks[node] if node in masks else masks.setdefault(node, allowed(nodes, node, C))
            score[i, 1:] = np.where(ok[1:], base[1:] + row[1:], NEG)
        for j, (p, _, _, _) in enumerate(entries):                             # merges: j absorbs (i, last_j) where prefix_i = prefix_j[:-1]
            i = where.get(p[:-1]) if p else None
            if i is not None:
                assert allowed(nodes, entries[i][3], C)[p[-1]] and child(nodes, entries[i][3], p[-1]) == entries[j][3]
                stay_pnb[j] = R._lae(stay_pnb[j], score[i, p[-1]])
                score[i, p[-1]] = NEG
        for i in range(n):
            score[i, 0] = R._lae(stay_pb[i], stay_pnb[i])
        best, near = select(score, W, ties)
        gap = min(gap, near)
        nxt = []
        for k in best:
            i, c = divmod(int(k), C)
            p, node = entries[i][0], entries[i][3]
            nxt.append((p, stay_pb[i], stay_pnb[i], node) if c == 0 else (p + (c,), NEG, float(score[i, c]), child(nodes, node, c)))
        entries = nxt
    final = np.array([R._lae(pb, pnb) if nodes[node, 5] >= 0 else NEG for _, pb, pnb, node in entries], dtype=np.float64)
    best, near = select(final, len(entries), ties)
    gap = min(gap, near)
    return [(entries[int(k)][0], float(final[int(k)]), int(nodes[entries[int(k)][3], 5])) for k in best], gap


def search(x, W, nodes, words, normalized=False, nbest=1):
    """The two-stage decoder (ops.ctc_lexicon_search) on one sample: the words the trie beam proposes, each scored exactly
    (ctc_lexicon_np.word_score), the `nbest` best by (exact score descending, word id ascending) -> ([(word id, exact score)], gap of
    the beam)."""
    hyps, gap = beam_search_trie(x, W, nodes, normalized)
    lp = R.log_probs(x, normalized)
    ids = sorted(h[2] for h in hyps)
    exact = [(k, X.word_score(lp, words[k])) for k in ids]
    exact = sorted([e for e in exact if e[1] > NEG], key=lambda e: (-e[1], e[0]))
    return exact[:nbest], gap


def batch_lexicon(seed, normalized, n=9, T=32, C=92, extra=1500):
    """(x fp32 [n, T, C], the sorted word list): the peaked batch, every second hypothesis of the plain beam of width 16, forty
    neighbours of each sample's best plain word (a class dropped, replaced or inserted), and random words of 2..15 classes up to
    `extra` words."""
    x = R.peaked_batch(seed, n, T, C)
    x = R.softmax32(x) if normalized else x
    rng = np.random.default_rng(seed + 7)
    words = set()
    for b in range(n):
        hyps, _ = R.beam_search(x[b], 16, normalized)
        words |= {tuple(w) for r, (w, s) in enumerate(hyps) if r % 2 == 1 and 1 <= len(w) <= 31}
        g = hyps[0][0]
        for _ in range(40):                                                    # neighbours of the plain beam's best word
            w = list(g)
            k = int(rng.integers(0, 3))
            if k == 0 and len(w) > 1:
                del w[int(rng.integers(0, len(w)))]
            elif k == 1 and w:
                w[int(rng.integers(0, len(w)))] = int(rng.integers(1, C))
            else:
                w.insert(int(rng.integers(0, len(w) + 1)), int(rng.integers(1, C)))
            if 1 <= len(w) <= 31:
                words.add(tuple(w))
    while len(words) < extra:
        L = int(rng.integers(2, 16))
        words.add(tuple(int(c) for c in rng.integers(1, C, L)))
    return x, sorted(words)
