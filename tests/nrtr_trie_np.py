"""The fp64 specification of beam search over the NRTR decoder along a lexicon's prefix tree (kernels/nrtr_beam.h:
nrtr_beam_step_kernel<true>, ccd_nrtr_beam_step_trie) in plain numpy, and its inputs:
    TrieSample                                  nrtr_beam_np.Sample with a trie node per slot
    beam_search_trie(table, W, ..., nodes)      the specification on a Markov table -> paths, lengths, scores, word ids, nodes, parents, gap
    word_score(table, word, start, end)         the exact log p(word <EOS>) of a word under the table
    exact_words(table, words, start, end)       brute force over a lexicon: every word of at most T - 1 classes, best first
    lexicon(seed, table)                        the word list of one sample (classes of the decoder, not yet shifted)
    rows_of(words, offset), trie_of(words)      the zero-padded rows class + offset, and ctc_trie_np.build_trie of them

The rules.  Everything is as nrtr_beam_np states it, with these additions:
    every slot carries a node of the trie (the table of ctc_trie_np.build_trie); before step 0 every slot is at node 0, the root;
    class c of the decoder is bit c + class_offset of a node's 128-bit child mask - the lexicon's rows are class + 1 for an
    AttnConvertor, whose class 0 is the character '0', and the trie never sets bit 0;
    a live slot r at node n gives the candidate (r, c), c != end_idx, iff c + class_offset <= 127 and that bit of mask[n] is set, and
    (r, end_idx) iff word_id[n] >= 0.  Every other candidate is -inf: it is no candidate and is never selected;
    an allowed candidate scores score[r] + log_softmax(logits[r])[c], the log-softmax over ALL C classes: nothing is renormalised
    over the allowed ones, so the score of a finished slot is the exact log-probability of its word with the <EOS>;
    finished and unused slots behave as in the plain beam;
    a selected extension carries child(n, c + class_offset) (clamped into the table; a well-formed table never needs it), a selected
    end_idx and a carried finished slot keep their node, an unused slot's node is 0;
    after the last step word_ids[r] = word_id[node[r]] if slot r is finished, else -1: a slot that is still live - a prefix, or a
    word whose <EOS> did not fit - and an unused slot are no word.  Paths, lengths and scores are the plain beam's."""
import numpy as np

import ctc_trie_np as N
import nrtr_beam_np as R
from beam_np import MIN_GAP, log_softmax64, select      # noqa: F401  (MIN_GAP: for the callers)

UNUSED, LIVE, FINISHED = R.UNUSED, R.LIVE, R.FINISHED
MASK_BITS = 128


class TrieSample(R.Sample):
    """The W slots of one sample, each with its node."""

    def __init__(self, W, start_idx, nodes, class_offset=1):
        super().__init__(W, start_idx)
        self.nodes, self.offset = nodes, class_offset
        self.node = [0] * W
        self._allowed = {}

    def allowed(self, node, C, end_idx):
        """bool [C]: the candidates a live slot at `node` has."""
        key = (node, C, end_idx)
        if key not in self._allowed:
            bits = N.allowed(self.nodes, node, MASK_BITS)
            ok = np.array([c + self.offset < MASK_BITS and bool(bits[c + self.offset]) for c in range(C)])
            ok[end_idx] = self.nodes[node, 5] >= 0
            self._allowed[key] = ok
        return self._allowed[key]

    def step(self, logits, end_idx, pad_idx, ties=False):
        """logits [W, C] fp32 (rows of slots that are not live are not read) -> (parent [W], gap)."""
        W, C = self.W, logits.shape[1]
        cand = np.full((W, C), -np.inf)
        for r in range(W):
            if self.state[r] == LIVE:
                cand[r] = np.where(self.allowed(self.node[r], C, end_idx), self.score[r] + log_softmax64(logits[r]), -np.inf)
            elif self.state[r] == FINISHED:
                cand[r, end_idx] = self.score[r]
        best, gap = select(cand, W, ties)
        seqs, score, state, parent, node = [], np.full(W, -np.inf), [UNUSED] * W, [-1] * W, [0] * W
        for n in range(W):
            if n < len(best):
                r, c = divmod(int(best[n]), C)
                done = self.state[r] == FINISHED
                seqs.append(self.seqs[r] + [pad_idx if done else c])
                score[n], parent[n] = cand[r, c], r
                state[n] = FINISHED if done or c == end_idx else LIVE
                if state[n] == FINISHED:
                    node[n] = self.node[r]
                else:
                    node[n] = min(max(N.child(self.nodes, self.node[r], c + self.offset), 0), self.nodes.shape[0] - 1)
            else:
                seqs.append(self.seqs[n] + [pad_idx])
        self.seqs, self.score, self.state, self.node = seqs, score, state, node
        return parent, gap

    def word_ids(self):
        return np.array([int(self.nodes[self.node[r], 5]) if self.state[r] == FINISHED else -1 for r in range(self.W)], dtype=np.int32)


def beam_search_trie(table, W, start_idx, end_idx, pad_idx, nodes, class_offset=1, ties=False):
    """One sample.  table fp32 [T, C + 1, C] (nrtr_beam_np.beam_search) -> (paths [W, T], lengths [W], scores [W] fp64, word_ids [W],
    node [W], parents [T, W], gap)."""
    T = table.shape[0]
    smp = TrieSample(W, start_idx, nodes, class_offset)
    parents, gap = [], np.inf
    for s in range(T):
        logits = np.stack([table[s, smp.seqs[r][-1]] for r in range(W)])
        parent, g = smp.step(logits, end_idx, pad_idx, ties)
        parents.append(parent)
        gap = min(gap, g)
    return smp.outputs(end_idx, T) + (smp.word_ids(), np.asarray(smp.node, dtype=np.int32), np.asarray(parents, dtype=np.int32), gap)


def word_score(table, word, start_idx, end_idx):
    """log p(word <EOS>) under the Markov table: the sum of log_softmax(table[s, previous token])[token] over the word's classes and
    the end class behind them.  -inf for a word of more than T - 1 classes: its <EOS> has no step left."""
    T = table.shape[0]
    if len(word) > T - 1:
        return -np.inf
    prev, score = start_idx, 0.0
    for s, c in enumerate(list(word) + [end_idx]):
        score += log_softmax64(table[s, prev])[c]
        prev = c
    return float(score)


def exact_words(table, words, start_idx, end_idx):
    """Brute force over the lexicon -> [(word id, score)] of every distinct word of finite score, by (score descending, id ascending);
    of equal words the lowest row counts, as in the trie."""
    first = {}
    for k, w in enumerate(words):
        first.setdefault(tuple(w), k)
    scored = [(k, word_score(table, w, start_idx, end_idx)) for w, k in first.items()]
    return sorted([e for e in scored if e[1] > -np.inf], key=lambda e: (-e[1], e[0]))


def likely_word(rng, table, length, start_idx, end_idx, pick=4):
    """`length` classes along the table: at every step a random one of the `pick` best classes that are not the end class."""
    prev, word = start_idx, []
    T = table.shape[0]
    for s in range(length):
        row = table[min(s, T - 1), prev].astype(np.float64).copy()
        row[end_idx] = -np.inf
        best = np.argsort(-row, kind="stable")[:max(1, min(pick, row.size - 1))]
        prev = int(best[int(rng.integers(0, len(best)))])
        word.append(prev)
    return tuple(word)


def lexicon(seed, table, size=300):
    """The word list of one sample, classes of the decoder (the end class C - 1 never occurs): half the words follow likely paths of
    the table (a random pick among the 4 best non-end classes per step), half are uniformly random words of 1..T - 1 classes; 30 % of
    the words also contribute one of their own proper prefixes; one word of T + 1 classes follows the best non-end class of every
    step, so that a slot can be live at the last step at a node that ends no word.  C = 3: 6 words.  Sorted, distinct."""
    T, _, C = table.shape
    rng = np.random.default_rng(seed)
    end = C - 1
    size = 6 if C == 3 else size
    words = {likely_word(rng, table, T + 1, end, end, pick=1)}
    tries = 0
    while len(words) < size and tries < 50 * size:
        tries += 1
        length = int(rng.integers(1, T))
        if tries % 2:
            w = likely_word(rng, table, length, end, end)
        else:
            w = tuple(int(c) for c in rng.integers(0, C - 1, length))
        words.add(w)
        if len(w) > 1 and rng.random() < 0.3 and len(words) < size:
            words.add(w[:int(rng.integers(1, len(w)))])
    return sorted(words)


def rows_of(words, class_offset=1, max_len=None):
    """The zero-padded int64 rows class + class_offset of a word list (ops.ctc_lexicon's layout)."""
    width = max(1, max(map(len, words), default=1)) if max_len is None else max_len
    rows = np.zeros((len(words), width), dtype=np.int64)
    for row, w in zip(rows, words):
        row[:len(w)] = np.asarray(w, dtype=np.int64) + class_offset
    return rows


def trie_of(words, class_offset=1):
    """ctc_trie_np.build_trie of the shifted rows: the reference builder's table."""
    return N.build_trie(rows_of(words, class_offset))
