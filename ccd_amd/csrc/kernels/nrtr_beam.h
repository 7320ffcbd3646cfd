// nrtr_beam.h - beam search over the NRTR attention decoder (ccd_nrtr_beam_step, ccd_nrtr_beam_reorder):
//   nrtr_beam_step_kernel     one decoding position: the logits of the W hypotheses of a sample -> the W best successors, their
//                             parents, the permuted token sequences; at the caller's wish the n-best lists as ctc_beam_kernel writes them
//   nrtr_beam_reorder_kernel  the per-layer q|k|v cache of the incremental decoder, permuted by those parents
// The semantics are restated in numpy in tests/nrtr_beam_np.py, which is the specification:
//   a sample holds W slots by rank; a slot is live, finished or unused and carries a token sequence and an fp64 score, the sum of
//   log_softmax(logits)[token] over its steps.  Start: slot 0 live with score 0, the others unused with score -inf.
//   candidates at a step   live slot r: (r, c) for every class c, score[r] + log_softmax(logits[r])[c] (fp64 over the fp32 row);
//                          finished slot r: (r, end_idx) alone, score unchanged, stays finished, writes padding_idx;
//                          unused slot: none.  A candidate of score -inf (a -inf logit) is no candidate.
//   selection              the W best by (score descending, k = r * C + c ascending); fewer candidates leave unused slots behind;
//                          class end_idx finishes the hypothesis (the token is written).
//
// Step kernel: ONE WAVEFRONT PER SAMPLE, one wavefront per workgroup (the candidate table is 16 KB of LDS).  Lane l owns the classes l
// and l + 64 of every slot and the positions l and l + 64 of every sequence, in every role: it loads them, it scans them, it stores
// them - so whatever a lane writes to global memory it has read itself before, and the update is in place without a second buffer.
//   1. every old sequence (positions 0..step, as 16-bit tokens) and the old scores / states go to LDS;
//   2. per live slot: cand[r][c] = score[r] + log_softmax(logits[r])[c] (beam_wave.h; the slot's row of the table holds the terms
//      of the sum on the way).  Finished: cand[r][end_idx] = score[r].  Everything else -inf;
//   3. W rounds of the wave arg-max of beam_wave.h over the table; the owner of the winner overwrites it with -inf.  Lane r keeps
//      rank r;
//   4. the new rows: positions 0..step from the parent's row in LDS, position step + 1 the new token; score, state, parent by lane r.
// Every loop that shuffles has a wave-uniform trip count (W, the slots).  fp64 throughout (ctc_real).  Phases 1, 3 and 4 and the
// finished slot of phase 2 are nrtr_beam_stage / _select / _store / _carry below: one copy for this kernel, its trie instance and the
// joint kernel of nrtr_joint.h.
//
// Beam search over a lexicon's prefix tree (ccd_nrtr_beam_step_trie, nrtr_beam_step_kernel<true>; tests/nrtr_trie_np.py is the
// specification): the same kernel - `template <bool kTrie>`, whose `false` instance is the code above and nothing else - with a trie
// node per slot, node int32 [B, W], in and out like score and state (the caller starts every slot at the root, node 0).  The table is
// ctc_beam_kernel<CTC_BEAM_TRIE>'s (ccd_hip.h has the layout), its mask bit for decoder class c is bit c + class_offset: the lexicon
// rows of an AttnConvertor are class + 1, because its class 0 is a character and the trie never sets bit 0.
//   live slot r at node n  (r, c), c != end_idx, exists iff c + class_offset <= 127 and that bit of mask[n] is set; (r, end_idx) iff
//                          word_id[n] >= 0.  Everything else is -inf: no candidate.  An allowed candidate scores what the plain
//                          instance gives it - the log-softmax runs over ALL C classes, nothing is renormalised - so the score of
//                          a finished slot is the exact log p(word <EOS> | image), comparable across words: no second stage.
//   nodes                  a selected extension carries first_child[n] + popcount(mask[n] bits below c + class_offset), clamped to
//                          [0, n_nodes) as the CTC instance clamps; end_idx and a carried finished slot keep the node; unused: 0.
//   final                  word_ids int32 [B, W]: word_id[node] of a finished slot, -1 for a live or unused one.
// Where the table is read: in phase 1 lane r < W loads node[r] (clamped: whatever the caller left there addresses the table) and the
// six-word record of that node (ctc_trie_fetch: one 24-byte request per slot and step, next to the score and the state) and parks
// the mask as two 64-bit words, first_child, word_id and the node in LDS - 28 B per slot, 448 B beside the 20.2 KB above.  Phase 2
// reads the two mask words of slot r at a wave-uniform address (a broadcast) and writes -inf instead of the sum where the lane's bit
// is clear.  Behind phase 3 lane r derives its new node from the record of its winner's parent, which still stands (the selection
// overwrites candidates only); a slot that finishes takes the word id from there too, so the last step needs no second fetch.  The
// cost is a beam step's, whatever the size of the lexicon.
//
// Reorder kernel: pure data movement.  One thread owns the same 16-byte piece of the K | V columns of one (layer, sample, position)
// in all W rows: it loads the piece of row parent[r] for every r whose parent differs (compile-time register index r, the gather is
// in the address: nothing goes to scratch), waits for all loads, then stores row r.  Cycles (0 <-> 1) and shared parents are safe
// because no other thread touches these bytes; rows with parent[r] == r (or an unused slot, parent -1) move nothing.
#pragma once

#include "beam_wave.h"

namespace ccd {

constexpr int NRTR_MAX_BEAM = 16;
constexpr int NRTR_MAX_C = 128;
constexpr int NRTR_MAX_LEN = 128;                                  // positions of a sequence (max_seq_len + 1)
constexpr int NRTR_UNUSED = 0, NRTR_LIVE = 1, NRTR_FINISHED = 2;

struct NrtrBeamWave {
    ctc_real cand[NRTR_MAX_BEAM][NRTR_MAX_C];
    ctc_real score[NRTR_MAX_BEAM];
    int state[NRTR_MAX_BEAM];
    unsigned short tok[NRTR_MAX_BEAM][NRTR_MAX_LEN];
};

template <bool kTrie>
struct NrtrBeamTrieWave {};                                        // (nothing without a lexicon trie)
template <>
struct NrtrBeamTrieWave<true> {
    unsigned long long allow[NRTR_MAX_BEAM][2];                    // bit k & 63 of [r][k >> 6]: the node of slot r has a child by bit k
    int node[NRTR_MAX_BEAM], first[NRTR_MAX_BEAM], word[NRTR_MAX_BEAM];    // the node of slot r, its first child, the word that ends there
};

static_assert(sizeof(NrtrBeamWave) == 20672 && sizeof(NrtrBeamTrieWave<true>) == 448, "the LDS layout of the step kernels is fixed");

struct NrtrBeamTrie {                                              // the lexicon trie of a launch (unused without one)
    const int* nodes;                                              // int32 [n_nodes, 8]: ccd_ctc_beam_search_trie's table
    int n_nodes, class_offset;                                     // class c of the decoder is bit c + class_offset of a mask
    int* node;                                                     // int32 [B, W], in and out: the node of every slot
    int* word_ids;                                                 // int32 [B, W], written with the paths
};

// Bit k of the 128-bit mask (m0 the low half); a k above 127 has no bit.
__device__ __forceinline__ bool nrtr_trie_bit(unsigned long long m0, unsigned long long m1, int k) {
    return k <= 127 && (((k < 64 ? m0 >> k : m1 >> (k - 64)) & 1ull) != 0ull);
}

// ---- the parts every step kernel runs (the two instances below, nrtr_joint.h's nrtr_beam_step_joint_kernel): ALL 64 LANES CALL THEM,
// the `__shared__` table comes by reference.  They keep the contracts of the decoder in one place: the tie rule, "a lane only stores
// what it loaded", wave-uniform trip counts (W) around every shuffle and ballot, fp64 compared and never re-rounded (the operation
// order of a score is the caller's, under -ffp-contract=off), registers and LDS only - nothing here indexes a private array.  None
// of them fences on entry or exit: the fences between the phases stay in the kernels, next to the staging and the candidates a
// kernel adds of its own; the one fence inside, behind every round of the selection, orders the knock-out against the next scan.

// Phase 1: lane r < W parks score and state of slot r; every lane stages its positions (<= step) of the W token rows as 16-bit.
__device__ __forceinline__ void nrtr_beam_stage(NrtrBeamWave& s, const long long* seq, int seq_len, const ctc_real* score, const int* state,
                                                long row0, int W, int step) {
    const int lane = lane_id(), c0 = lane, c1 = lane + 64;
    ctc_real my_score = ctc_neg_inf();
    int my_state = NRTR_UNUSED;
    if (lane < W) {
        my_score = score[row0 + lane];
        my_state = state[row0 + lane];
    }
    if (lane < NRTR_MAX_BEAM) {
        s.score[lane] = my_score;
        s.state[lane] = my_state;
    }
    for (int r = 0; r < W; ++r) {
        const long long* const q = seq + (row0 + r) * seq_len;
        if (c0 <= step) s.tok[r][c0] = (unsigned short)q[c0];
        if (c1 <= step) s.tok[r][c1] = (unsigned short)q[c1];
    }
}

// Phase 2, a slot that is not live (state st, score sc): a finished one offers (r, end_idx) alone, an unused one nothing.
__device__ __forceinline__ void nrtr_beam_carry(ctc_real* cand, int st, ctc_real sc, int end_idx, int C) {
    const int c0 = lane_id(), c1 = c0 + 64;
    const bool carry = st == NRTR_FINISHED;
    if (c0 < C) cand[c0] = carry && c0 == end_idx ? sc : ctc_neg_inf();
    if (c1 < C) cand[c1] = carry && c1 == end_idx ? sc : ctc_neg_inf();
}

struct NrtrBeamPick {                                              // what lane r knows about the winner of rank r
    ctc_real score;                                                // -inf, unused, -1, 0, pad_idx: there was none
    int state, parent, c, tok;                                     // the winner is candidate (parent, c) of the table
};

// Phase 3: the W best of s.cand, one per round; lane r keeps rank r.  Only s.cand is overwritten (fenced after every round), so what
// a kernel parked per slot or per candidate beside it still stands afterwards: the mode-specific follow-ups read it out of
// (pick.parent, pick.c) behind the call.
__device__ __forceinline__ NrtrBeamPick nrtr_beam_select(NrtrBeamWave& s, int W, int C, int end_idx, int pad_idx) {
    const int lane = lane_id(), c0 = lane, c1 = lane + 64;
    const bool has0 = c0 < C, has1 = c1 < C;
    NrtrBeamPick pick = {ctc_neg_inf(), NRTR_UNUSED, -1, 0, pad_idx};
    for (int r = 0; r < W; ++r) {
        ctc_real best = ctc_neg_inf();
        int best_k = 0x7fffffff;
        for (int i = 0; i < W; ++i) {                                      // k ascends along the scan: `>` keeps the lowest k of equals
            if (has0) {
                const ctc_real v = s.cand[i][c0];
                if (v > best) {
                    best = v;
                    best_k = i * C + c0;
                }
            }
            if (has1) {
                const ctc_real v = s.cand[i][c1];
                if (v > best) {
                    best = v;
                    best_k = i * C + c1;
                }
            }
        }
        beam_wave_best(best, best_k);
        if (best > ctc_neg_inf()) {                                        // wave-uniform: every lane holds the same winner
            const int i = best_k / C, c = best_k - i * C;
            if (lane == (c & 63)) s.cand[i][c] = ctc_neg_inf();            // (only this lane ever reads the entry again)
            if (lane == r) {
                const bool was_finished = s.state[i] == NRTR_FINISHED;
                pick.score = best;
                pick.parent = i;
                pick.c = c;
                pick.state = was_finished || c == end_idx ? NRTR_FINISHED : NRTR_LIVE;
                pick.tok = was_finished ? pad_idx : c;
            }
        }
        wave_lds_fence();
    }
    return pick;
}

// Phase 4, in place: score, state, parent (and hyp_scores) of slot `lane` by lane < W, then the W rows - positions 0..step from the
// parent's row in LDS, position step + 1 the new token.  A lane stores the positions it loaded in nrtr_beam_stage and nothing else,
// which is what makes one buffer enough.  paths / lengths (all or none, with hyp_scores): the n-best lists.
__device__ __forceinline__ void nrtr_beam_store(const NrtrBeamWave& s, const NrtrBeamPick& pick, long long* seq, int seq_len, ctc_real* score,
                                                int* state, int* __restrict__ parent, int* __restrict__ paths, int* __restrict__ lengths,
                                                float* __restrict__ hyp_scores, long row0, int W, int step, int end_idx) {
    const int lane = lane_id(), c0 = lane, c1 = lane + 64;
    if (lane < W) {
        score[row0 + lane] = pick.score;
        state[row0 + lane] = pick.state;
        parent[row0 + lane] = pick.parent;
        if (hyp_scores) hyp_scores[row0 + lane] = pick.state == NRTR_UNUSED ? -__builtin_inff() : (float)pick.score;
    }
    const int T = seq_len - 1;
    for (int r = 0; r < W; ++r) {
        const int p = shfl(pick.parent, r), tk = shfl(pick.tok, r);        // wave-uniform
        long long* const q = seq + (row0 + r) * seq_len;
        int t0 = -1, t1 = -1;                                              // the new row's tokens at this lane's positions
        if (p >= 0) {
            if (c0 <= step) t0 = s.tok[p][c0];
            if (c1 <= step) t1 = s.tok[p][c1];
            if (c0 == step + 1) t0 = tk;
            if (c1 == step + 1) t1 = tk;
            if (p != r) {
                if (c0 <= step) q[c0] = t0;
                if (c1 <= step) q[c1] = t1;
            }
        }
        if (c0 == step + 1) q[c0] = tk;                                    // (an unused slot: padding_idx)
        if (c1 == step + 1) q[c1] = tk;
        if (paths) {                                                       // the classes in front of the first end_idx behind position 0
            const bool e0 = p >= 0 && c0 >= 1 && c0 <= step + 1 && t0 == end_idx, e1 = p >= 0 && c1 <= step + 1 && t1 == end_idx;
            const unsigned long long m0 = ballot(e0), m1 = ballot(e1);
            const int first = m0 ? __builtin_ctzll(m0) : (m1 ? 64 + __builtin_ctzll(m1) : step + 2);
            const int len = p >= 0 ? first - 1 : -1;
            int* const o = paths + (row0 + r) * T;
            if (c0 >= 1 && c0 <= T) o[c0 - 1] = c0 - 1 < len ? t0 : -1;
            if (c1 <= T) o[c1 - 1] = c1 - 1 < len ? t1 : -1;
            if (lane == 0) lengths[row0 + r] = len;
        }
    }
}

// grid = B, block = 64.  The launcher has checked 1 <= W <= 16, 1 <= C <= 128, 0 <= step, step + 2 <= seq_len <= 128, end_idx in
// [0, C), pad_idx in [0, 65536).  paths / lengths / hyp_scores: all three or none.  Every line the trie adds sits behind `if constexpr
// (kTrie)` (`trie` is not looked at without one; with one the launcher has checked n_nodes >= 1, class_offset in {0, 1}, and word_ids
// comes with the paths): the `false` instance is the four shared parts, its own live candidates and nothing else.
template <bool kTrie>
__global__ __launch_bounds__(64) void nrtr_beam_step_kernel(const float* __restrict__ logits, long ldl, int W, int C, int step, int end_idx,
                                                            int pad_idx, long long* seq, int seq_len, ctc_real* score, int* state,
                                                            int* __restrict__ parent, int* __restrict__ paths, int* __restrict__ lengths,
                                                            float* __restrict__ hyp_scores, NrtrBeamTrie trie) {
    __shared__ NrtrBeamWave s;
    __shared__ NrtrBeamTrieWave<kTrie> tr;
    const int lane = lane_id(), b = blockIdx.x;
    const int c0 = lane, c1 = lane + 64;
    const bool has0 = c0 < C, has1 = c1 < C;
    const long row0 = (long)b * W;
    const float ninf = -__builtin_inff();

    // ---- 1. the old state
    nrtr_beam_stage(s, seq, seq_len, score, state, row0, W, step);
    if constexpr (kTrie) {
        int rec[CTC_TRIE_RECORD] = {0, 0, 0, 0, 0, -1}, my_node = 0;       // (a slot behind W: no edge, no word)
        if (lane < W) {
            const int n = trie.node[row0 + lane];
            my_node = n < 0 ? 0 : (n >= trie.n_nodes ? trie.n_nodes - 1 : n);
            ctc_trie_fetch(trie.nodes, my_node, rec);
        }
        if (lane < NRTR_MAX_BEAM) {
            tr.allow[lane][0] = (unsigned long long)(unsigned)rec[0] | ((unsigned long long)(unsigned)rec[1] << 32);
            tr.allow[lane][1] = (unsigned long long)(unsigned)rec[2] | ((unsigned long long)(unsigned)rec[3] << 32);
            tr.first[lane] = rec[4];
            tr.word[lane] = rec[5];
            tr.node[lane] = my_node;
        }
    }
    wave_lds_fence();

    // ---- 2. the candidates
    for (int r = 0; r < W; ++r) {
        const int st = s.state[r];                                         // wave-uniform
        const ctc_real sc = s.score[r];
        if (st == NRTR_LIVE) {
            const float* const x = logits + (row0 + r) * ldl;
            const CtcReal2 lp = beam_wave_log_probs(has0 ? x[c0] : ninf, has1 ? x[c1] : ninf, has0, has1, false, s.cand[r], C);
            if constexpr (kTrie) {                                         // an extension the trie has no edge for, an end where no
                const unsigned long long m0 = tr.allow[r][0], m1 = tr.allow[r][1];             // word ends: no candidate
                const bool word = tr.word[r] >= 0;
                const bool ok0 = c0 == end_idx ? word : nrtr_trie_bit(m0, m1, c0 + trie.class_offset);
                const bool ok1 = c1 == end_idx ? word : nrtr_trie_bit(m0, m1, c1 + trie.class_offset);
                if (has0) s.cand[r][c0] = ok0 ? sc + lp.c0 : ctc_neg_inf();
                if (has1) s.cand[r][c1] = ok1 ? sc + lp.c1 : ctc_neg_inf();
            } else {
                if (has0) s.cand[r][c0] = sc + lp.c0;                      // (-inf stays -inf: a score is finite or -inf)
                if (has1) s.cand[r][c1] = sc + lp.c1;
            }
        } else {
            nrtr_beam_carry(s.cand[r], st, sc, end_idx, C);
        }
    }
    wave_lds_fence();

    // ---- 3. the W best, one per round; lane r keeps the slot of rank r
    const NrtrBeamPick pick = nrtr_beam_select(s, W, C, end_idx, pad_idx);

    // ---- 4. the new state, in place: a lane stores what it loaded in phase 1 (positions) or owns (slot `lane`)
    if constexpr (kTrie) {
        int new_node = 0, new_word = -1;                                   // the node of the new slot; its word, if it has finished
        if (pick.parent >= 0) {                                            // the parent's record, which phase 1 left standing
            const int i = pick.parent;
            if (pick.state == NRTR_FINISHED) {
                new_node = tr.node[i];
                new_word = tr.word[i];
            } else {
                const int child = ctc_trie_child(tr.first[i], tr.allow[i][0], tr.allow[i][1], pick.c + trie.class_offset);
                new_node = child < 0 ? 0 : (child >= trie.n_nodes ? trie.n_nodes - 1 : child);
            }
        }
        if (lane < W) {
            trie.node[row0 + lane] = new_node;
            if (paths) trie.word_ids[row0 + lane] = new_word;              // (a live or an unused slot is no word: -1)
        }
    }
    nrtr_beam_store(s, pick, seq, seq_len, score, state, parent, paths, lengths, hyp_scores, row0, W, step, end_idx);
}

// One thread per 16-byte piece of the K | V columns of (layer, sample, position <= step): total = L * B * (step + 1) * chunks threads,
// chunks = 2 D / 8.  cache bf16 [L, B * W * Tp, 3 D] (q | k | v per row, row = (b * W + r) * Tp + position), 16-byte aligned, D % 8 == 0.
__global__ __launch_bounds__(256) void nrtr_beam_reorder_kernel(bf16_t* cache, const int* __restrict__ parent, int L, int B, int W, int Tp,
                                                                int D, int step, long total) {
    const long id = (long)blockIdx.x * 256 + threadIdx.x;
    if (id >= total) return;
    const int chunks = D / 4;
    const int chunk = (int)(id % chunks);
    long rest = id / chunks;
    const int t = (int)(rest % (step + 1));
    rest /= step + 1;
    const int b = (int)(rest % B), l = (int)(rest / B);
    const long ld = 3L * D;
    bf16_t* const base = cache + (((long)l * B + b) * W * Tp + t) * ld + D + 8L * chunk;      // slot 0; slot r lies r * Tp rows further
    const int* const par = parent + (long)b * W;
    u32x4 v[NRTR_MAX_BEAM];
    bool move[NRTR_MAX_BEAM];
#pragma unroll
    for (int r = 0; r < NRTR_MAX_BEAM; ++r) {
        move[r] = false;
        if (r < W) {
            const int p = par[r];
            move[r] = p != r && (unsigned)p < (unsigned)W;
            if (move[r]) v[r] = *reinterpret_cast<const u32x4*>(base + (long)p * Tp * ld);
        }
    }
    glds_wait_all();                                                       // every load has landed before the first store leaves
#pragma unroll
    for (int r = 0; r < NRTR_MAX_BEAM; ++r)
        if (move[r]) *reinterpret_cast<u32x4*>(base + (long)r * Tp * ld) = v[r];
}

}  // namespace ccd
