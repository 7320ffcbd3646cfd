// ctc_beam.h - CTC prefix beam search for the CTC head (ccd_ctc_beam_search):
//   ctc_beam_kernel   frame scores fp32 [B, T, C] (logits or probabilities) -> the W most probable words with the log of their
//                     probability summed over alignments: paths int32 [B, W, T], lengths int32 [B, W], scores fp32 [B, W], by rank.
// Best-path decoding (ctc_greedy_kernel) picks the most probable alignment; this picks the most probable words.  The semantics
// are restated in numpy in tests/ctc_beam_np.py, which is the specification:
//   a beam entry is a prefix of classes 1..C-1 with pb / pnb, the log mass of its alignments ending in the blank / in a non-blank;
//   the start is the empty prefix, pb = 0, pnb = -inf.  Per frame, tot_i = logaddexp(pb_i, pnb_i):
//     stay (i, 0)    same prefix: pb' = tot_i + lp[0], pnb' = pnb_i + lp[last_i] (-inf for the empty prefix)
//     extend (i, c)  prefix_i + c: pb' = -inf, pnb' = (c == last_i ? pb_i : tot_i) + lp[c]
//     merge          an extend candidate that spells the prefix of a live entry j is log-added into the pnb' of j's stay candidate
//                    and disappears (prefixes are unique: j absorbs at most one, no two extend candidates coincide)
//     select         the W best candidates of finite score logaddexp(pb', pnb'), by (score descending, k = rank * C + class ascending).
//
// Lane mapping: ONE WAVEFRONT PER SAMPLE, as the loss kernels.  Lane l owns the classes l and l + 64 in every role: it loads their
// scores, keeps their log-probabilities in registers and scans the candidates (i, l) and (i, l + 64) of every entry i - at most
// 2 W = 32 candidates per lane, none of them stored: a candidate's score is one add of the entry's pb or tot (read from LDS at a
// wave-uniform address: a broadcast) and the lane's own lp, minus the candidates a 64-bit mask per (entry, half) marks as merged.
// The log-probabilities of a frame and the selection - W rounds of a wave arg-max, each lane folding the candidates it has not given
// away yet (a 32-bit mask in a register) - are the steps of beam_wave.h, shared with nrtr_beam_step_kernel.  The entries (pb, pnb,
// length, last class) and the prefixes - bytes, classes are < 128; two buffers of W x 64, swapped per frame - live in LDS: 4.1 KB per
// wave, 16.5 KB per workgroup.
// The merge test: the 16 x 16 pairs (i, j) four to a lane, prefiltered on len_j = len_i + 1 and on the last class of prefix_i; the
// survivors (a ballot mask, so the walk is wave-uniform) compare the len_i positions one per lane and a second ballot decides.
//
// Every loop that shuffles or ballots has a wave-uniform trip count (T, W, the live entries, the bits of a ballot mask); no lane
// of a live wave leaves before the last shuffle.  Arithmetic is fp64 (ctc_real) throughout; probabilities (normalized) go through the
// same ascending-order sum as logits.  What the software fp64 exp / log and the W-fold rescan cost on the device: tools/ctc_bench.py,
// case `beam`.
//
// Language-model fusion (ccd_ctc_beam_search_lm, ctc_beam_kernel<CTC_BEAM_LM>; tests/ctc_beam_lm_np.py is the specification): the same kernel -
// `template <int kMode>`, whose CTC_BEAM_PLAIN instance is the code above and nothing else - with one additive term per extension from a character
// n-gram table lm fp32 [C^(order-1), C]: the row of an entry is its last order - 1 classes (most recent last, 0 where the prefix is
// shorter), column c >= 1 the log-probability of character c behind that context, column 0 that of the word ending there.
//     g(i, c) = lm[row_i, c] == -inf ? -inf : (double)weight * (double)lm[row_i, c] + (double)bonus      (the product, then the sum)
//     extend (i, c)   pnb' = ((c == last_i ? pb_i : tot_i) + lp[c]) + g(i, c); a merge log-adds that same number
// so pb and pnb of a prefix both carry the sum of g over its characters.  Stay candidates, the key and the tie rule are unchanged.
// Where the table is read: when the entries of a frame are written, lane r derives the row of entry r from the last two prefix bytes
// in LDS; every lane then requests lm[row_i * C + c] for its two classes of every live entry - coalesced 4-byte loads of a table that
// stays in L2 - into registers, right behind the selection.  They are stored into a per-wave fp32 [16][128] LDS block behind the next
// frame's fp64 log-softmax, which hides them; the scan reads its own two columns back (dynamic entry index), and the one cross-lane
// read is the absorbed class of a merge, behind a wave_lds_fence.  g is formed where the candidate score is: one fp64 multiply and add.
// eos: behind the last frame lane r adds (double)weight * lm[row_r, 0] to entry r (-inf where the table says so), counts the entries
// that beat it by (score descending, previous rank ascending) and the results are written by that rank; a -inf entry is an unused slot.
// LDS: 8 KB + 64 B per wave on top of the 4.2 KB above: 50 176 B = 49 KB per workgroup (17 152 B without a language model) - under the
// 64 KB static limit, three workgroups per CU by LDS.  The 32 values in flight cost registers (176 VGPRs against 106: two waves per
// SIMD), which a kernel of one wave per sample does not miss.
//
// Trie search over a lexicon (ccd_ctc_beam_search_trie, ctc_beam_kernel<CTC_BEAM_TRIE>; tests/ctc_trie_np.py is the specification): the
// third instance.  The lexicon is a prefix tree, nodes int32 [n_nodes, 8] in breadth-first order (ccd_hip.h has the layout): every entry
// carries the node of its prefix (the empty prefix: node 0), an extend candidate (i, c) exists iff bit c of the 128-bit child mask of
// node_i is set - otherwise it is -inf: never selected, never merged - and scores exactly what the plain instance gives it.  Behind the
// last frame an entry whose node ends no word is -inf, the entries are ranked again as the eos re-rank does (the code is shared), and
// word_ids int32 [B, W] names the lexicon row of every hypothesis.  The cost is a beam's, whatever the size of the lexicon.
// Where the table is read: the record of entry i - the mask as two 64-bit words, first_child, word_id, the node id - lives in LDS, 28 B
// per entry, 448 B per wave.  The allowed test costs the scan nothing: `merged` of a frame starts as the complement of the mask instead
// of zero, so an extension without an edge is `gone` like one that was merged away (bit 0, the stay, is not looked at).  The lane
// that keeps the entry of rank r derives its node while the old entries still stand: the parent's node for a stay, first_child +
// popcount(mask bits below c) for an extension, clamped to [0, n_nodes) so that no table, however malformed, makes an address
// outside it.  It then requests the six words of that node's record into registers - one 24-byte load per entry and frame -
// and stores them into LDS behind the next frame's log-softmax, as the language model's values are.  Mask bits of classes >= C are
// never scanned (has0 / has1): such a word is unreachable, as it is -inf for ccd_ctc_lexicon_score.  The record of the last frame's
// entries stays in registers: lane r reads the word id of entry r from there.
// What it costs next to the plain instance and to scoring every word of the lexicon: tools/ctc_bench.py, case `trie`.
#pragma once

#include "beam_wave.h"

namespace ccd {

constexpr int CTC_MAX_BEAM = 16;

struct CtcBeamWave {
    ctc_real lp[CTC_MAX_C];                                      // this frame: first the terms of the sum, then the log-probabilities
    ctc_real pb[CTC_MAX_BEAM], pnb[CTC_MAX_BEAM], tot[CTC_MAX_BEAM];
    ctc_real stay_pb[CTC_MAX_BEAM], stay_pnb[CTC_MAX_BEAM], stay_score[CTC_MAX_BEAM];
    unsigned long long merged[CTC_MAX_BEAM][2];                  // bit c & 63 of [i][c >> 6]: extend candidate (i, c) was merged away
    int len[CTC_MAX_BEAM], last[CTC_MAX_BEAM], absorb[CTC_MAX_BEAM];     // last: 0 for the empty prefix; absorb: the entry whose
    unsigned char prefix[2][CTC_MAX_BEAM][CTC_MAX_T];            // extension this entry's stay candidate takes in, or -1
};

enum CtcBeamMode { CTC_BEAM_PLAIN = 0, CTC_BEAM_LM = 1, CTC_BEAM_TRIE = 2 };

template <bool kLm>
struct CtcBeamLmWave {};                                         // (nothing without a language model)
template <>
struct CtcBeamLmWave<true> {
    float v[CTC_MAX_BEAM][CTC_MAX_C];                            // lm[row_i, c] of the live entries, as the table holds it
    int row[CTC_MAX_BEAM];                                       // the table row of entry i
};

struct CtcBeamLm {                                               // the language model of a launch (unused without one)
    const float* table;                                          // fp32 [C^(order-1), C]
    int order, eos;
    double weight, bonus;
};

template <bool kTrie>
struct CtcBeamTrieWave {};                                       // (nothing without a lexicon trie)
template <>
struct CtcBeamTrieWave<true> {
    unsigned long long allow[CTC_MAX_BEAM][2];                   // bit c & 63 of [i][c >> 6]: the node of entry i has a child by class c
    int node[CTC_MAX_BEAM], first[CTC_MAX_BEAM], word[CTC_MAX_BEAM];     // the node of entry i, its first child, the word that ends there
};

struct CtcBeamTrie {                                             // the lexicon trie of a launch (unused without one)
    const int* nodes;                                            // int32 [n_nodes, 8]: mask[4], first_child, word_id, parent, class
    int n_nodes;
    int* word_ids;                                               // int32 [B, W]
};                                                               // (ctc_trie_fetch / ctc_trie_child: beam_wave.h)

// g of one table value: the fp64 product, then the fp64 sum; -inf stays -inf whatever the weight.
__device__ __forceinline__ ctc_real ctc_lm_term(float v, double weight, double bonus) {
    return v == -__builtin_inff() ? ctc_neg_inf() : weight * (double)v + bonus;
}

// All 64 lanes.  Requests lm[row_i, c] of the lane's two classes for every live entry into registers (consumed a frame later).
__device__ __forceinline__ void ctc_lm_fetch(const CtcBeamLmWave<true>& w, const float* __restrict__ table, int C, int n, int c0, int c1,
                                             bool has0, bool has1, float (&r)[2 * CTC_MAX_BEAM]) {
#pragma unroll
    for (int i = 0; i < CTC_MAX_BEAM; ++i) {
        r[2 * i] = r[2 * i + 1] = 0.f;
        if (i < n) {
            const float* const p = table + (long)w.row[i] * C;
            if (has0) r[2 * i] = p[c0];
            if (has1) r[2 * i + 1] = p[c1];
        }
    }
}

// grid = ceil(B / CTC_WAVES).  The launcher has checked 1 <= W <= CTC_MAX_BEAM, 1 <= T <= CTC_MAX_T, 2 <= C <= CTC_MAX_C and, with a
// language model (kLm; `lm` is not looked at without one), 1 <= order <= 3, eos in {0, 1}, weight and bonus finite; the table holds
// C^(order-1) rows of C.  Every line the model adds sits behind `if constexpr (kLm)`, every line the trie adds behind `if constexpr
// (kTrie)` (`trie` is not looked at without one; with one the launcher has checked n_nodes >= 1): the CTC_BEAM_PLAIN instance is the
// kernel as it was.
template <int kMode>
__global__ __launch_bounds__(CTC_THREADS) void ctc_beam_kernel(const float* __restrict__ scores, long sample_stride, long step_stride, int B,
                                                               int T, int C, int normalized, int W, int* __restrict__ paths,
                                                               int* __restrict__ lengths, float* __restrict__ hyp_scores, CtcBeamLm lm,
                                                               CtcBeamTrie trie) {
    constexpr bool kLm = kMode == CTC_BEAM_LM, kTrie = kMode == CTC_BEAM_TRIE;
    __shared__ CtcBeamWave waves[CTC_WAVES];
    __shared__ CtcBeamLmWave<kLm> tables[CTC_WAVES];
    __shared__ CtcBeamTrieWave<kTrie> tries[CTC_WAVES];
    const int lane = lane_id(), b = blockIdx.x * CTC_WAVES + wave_id();
    if (b >= B) return;                                                    // (whole waves; no workgroup barrier below)
    CtcBeamWave& s = waves[wave_id()];
    CtcBeamLmWave<kLm>& m = tables[wave_id()];
    CtcBeamTrieWave<kTrie>& tr = tries[wave_id()];
    const float* const x = scores + (long)b * sample_stride;
    const int c0 = lane, c1 = lane + 64;
    const bool has0 = c0 < C, has1 = c1 < C;

    if (lane < CTC_MAX_BEAM) {
        s.pb[lane] = lane == 0 ? (ctc_real)0 : ctc_neg_inf();
        s.pnb[lane] = ctc_neg_inf();
        s.len[lane] = lane == 0 ? 0 : -1;
        s.last[lane] = 0;
        if constexpr (kLm) m.row[lane] = 0;                                // the empty prefix: every position missing
    }
    wave_lds_fence();
    int n = 1, cur = 0;                                                    // live entries (wave-uniform), the prefix buffer that holds them
    float next0 = has0 ? x[c0] : 0.f, next1 = has1 ? x[c1] : 0.f;
    float lmv[2 * CTC_MAX_BEAM];                                           // kLm: the table values requested for the next frame's entries
    if constexpr (kLm) ctc_lm_fetch(m, lm.table, C, n, c0, c1, has0, has1, lmv);
    int rec[CTC_TRIE_RECORD] = {0, 0, 0, 0, 0, -1};                        // kTrie: the record requested for the next frame's entry `lane`
    int rec_node = 0;                                                      // and its node: the root
    if constexpr (kTrie)
        if (lane < CTC_MAX_BEAM) ctc_trie_fetch(trie.nodes, 0, rec);
    for (int t = 0; t < T; ++t) {
        const float v0 = next0, v1 = next1;
        if (t + 1 < T) {                                                   // the next frame is requested before this frame's arithmetic
            const float* const p = x + (long)(t + 1) * step_stride;
            next0 = has0 ? p[c0] : 0.f;
            next1 = has1 ? p[c1] : 0.f;
        }
        // ---- log-probabilities of the lane's two classes
        const CtcReal2 lp = beam_wave_log_probs(v0, v1, has0, has1, normalized, s.lp, C);
        const ctc_real lp0 = lp.c0, lp1 = lp.c1;
        if (has0) s.lp[c0] = lp0;
        if (has1) s.lp[c1] = lp1;
        if constexpr (kLm) {                                               // requested behind the last selection: a log-softmax ago
#pragma unroll
            for (int i = 0; i < CTC_MAX_BEAM; ++i)
                if (i < n) {
                    m.v[i][c0] = lmv[2 * i];
                    m.v[i][c1] = lmv[2 * i + 1];
                }
        }
        if constexpr (kTrie) {                                             // likewise
            if (lane < CTC_MAX_BEAM) {
                tr.allow[lane][0] = (unsigned long long)(unsigned)rec[0] | ((unsigned long long)(unsigned)rec[1] << 32);
                tr.allow[lane][1] = (unsigned long long)(unsigned)rec[2] | ((unsigned long long)(unsigned)rec[3] << 32);
                tr.first[lane] = rec[4];
                tr.word[lane] = rec[5];
                tr.node[lane] = rec_node;
            }
        }
        if (lane < n) {
            s.tot[lane] = ctc_lae(s.pb[lane], s.pnb[lane]);
            s.absorb[lane] = -1;
        }
        if constexpr (kTrie) {                                             // an extension the trie has no edge for is gone from the start
            if (lane < CTC_MAX_BEAM) {
                s.merged[lane][0] = ~((unsigned long long)(unsigned)rec[0] | ((unsigned long long)(unsigned)rec[1] << 32));
                s.merged[lane][1] = ~((unsigned long long)(unsigned)rec[2] | ((unsigned long long)(unsigned)rec[3] << 32));
            }
        } else {
            if (lane < 2 * CTC_MAX_BEAM) s.merged[lane >> 1][lane & 1] = 0ull;
        }
        wave_lds_fence();

        // ---- merges: extend candidate (i, last_j) spells live entry j where prefix_j = prefix_i + last_j
        for (int q = 0; q * 4 < n; ++q) {                                  // pair (i, j) = (p >> 4, p & 15), p = 64 q + lane: rows i < n
            const int p = q * 64 + lane, i = p >> 4, j = p & 15;
            bool maybe = i < n && j < n;
            if (maybe) {
                const int li = s.len[i];
                maybe = s.len[j] == li + 1 && (li == 0 || s.prefix[cur][j][li - 1] == s.last[i]);
            }
            unsigned long long pairs = ballot(maybe);
            while (pairs) {
                const int bit = __builtin_ctzll(pairs);
                pairs &= pairs - 1;
                const int pi = q * 4 + (bit >> 4), pj = bit & 15, li = s.len[pi];
                const bool differs = lane < li && s.prefix[cur][pi][lane] != s.prefix[cur][pj][lane];
                if (ballot(differs) == 0ull && lane == 0) {
                    const int lj = s.last[pj];
                    s.absorb[pj] = pi;
                    s.merged[pi][lj >> 6] |= 1ull << (lj & 63);
                }
            }
        }
        wave_lds_fence();

        // ---- the stay candidate of entry `lane`
        if (lane < n) {
            const int lj = s.last[lane], from = s.absorb[lane];
            const ctc_real lpl = s.lp[lj];
            ctc_real pnb = s.len[lane] > 0 ? s.pnb[lane] + lpl : ctc_neg_inf();
            if (from >= 0) {
                ctc_real ext = (s.last[from] == lj ? s.pb[from] : s.tot[from]) + lpl;
                if constexpr (kLm) ext = ext + ctc_lm_term(m.v[from][lj], lm.weight, lm.bonus);       // (another lane's column)
                pnb = ctc_lae(pnb, ext);
            }
            const ctc_real pb = s.tot[lane] + s.lp[0];
            s.stay_pb[lane] = pb;
            s.stay_pnb[lane] = pnb;
            s.stay_score[lane] = ctc_lae(pb, pnb);
        }
        wave_lds_fence();

        // ---- the W best candidates, one per round; lane r keeps the entry of rank r
        unsigned given = 0u;                                               // bit 2 i + h: this lane's candidate (i, lane + 64 h) is taken
        ctc_real new_pb = ctc_neg_inf(), new_pnb = ctc_neg_inf();
        int new_len = -1, new_last = 0, n_new = 0, new_node = 0;
        for (int r = 0; r < W; ++r) {
            ctc_real best = ctc_neg_inf();
            int best_k = 0x7fffffff;
            for (int i = 0; i < n; ++i) {                                  // k ascends along the scan: `>` keeps the lowest k of equals
                const ctc_real pbi = s.pb[i], toti = s.tot[i];
                const int lasti = s.last[i];
                if (has0 && !((given >> (2 * i)) & 1u)) {
                    const bool gone = (s.merged[i][0] >> lane) & 1ull;
                    ctc_real ext = (c0 == lasti ? pbi : toti) + lp0;
                    if constexpr (kLm) ext = ext + ctc_lm_term(m.v[i][c0], lm.weight, lm.bonus);
                    const ctc_real sc = c0 == 0 ? s.stay_score[i] : (gone ? ctc_neg_inf() : ext);
                    if (sc > best) {
                        best = sc;
                        best_k = i * C + c0;
                    }
                }
                if (has1 && !((given >> (2 * i + 1)) & 1u)) {
                    const bool gone = (s.merged[i][1] >> lane) & 1ull;
                    ctc_real ext = (c1 == lasti ? pbi : toti) + lp1;
                    if constexpr (kLm) ext = ext + ctc_lm_term(m.v[i][c1], lm.weight, lm.bonus);
                    const ctc_real sc = gone ? ctc_neg_inf() : ext;
                    if (sc > best) {
                        best = sc;
                        best_k = i * C + c1;
                    }
                }
            }
            beam_wave_best(best, best_k);
            if (best > ctc_neg_inf()) {                                    // wave-uniform: every lane holds the same winner
                const int i = best_k / C, c = best_k - i * C, li = s.len[i];
                if (lane == (c & 63)) given |= 1u << (2 * i + (c >> 6));
                if (lane < li) s.prefix[cur ^ 1][r][lane] = s.prefix[cur][i][lane];
                if (c > 0 && lane == li) s.prefix[cur ^ 1][r][li] = (unsigned char)c;      // (li <= t <= 63)
                if (lane == r) {
                    new_pb = c > 0 ? ctc_neg_inf() : s.stay_pb[i];
                    new_pnb = c > 0 ? best : s.stay_pnb[i];
                    new_len = li + (c > 0 ? 1 : 0);
                    new_last = c > 0 ? c : s.last[i];
                    if constexpr (kTrie) {                                 // the parent's record, while it stands
                        const int child = c > 0 ? ctc_trie_child(tr.first[i], tr.allow[i][0], tr.allow[i][1], c) : tr.node[i];
                        new_node = child < 0 ? 0 : (child >= trie.n_nodes ? trie.n_nodes - 1 : child);
                    }
                }
                ++n_new;
            }
        }
        wave_lds_fence();                                                  // every read of the old entries is done
        if (lane < CTC_MAX_BEAM) {
            s.pb[lane] = new_pb;
            s.pnb[lane] = new_pnb;
            s.len[lane] = new_len;
            s.last[lane] = new_last;
            if constexpr (kLm) {                                           // the row of the new entry from its last two prefix bytes
                const int p1 = new_len >= 1 ? (int)s.prefix[cur ^ 1][lane][new_len - 1] : 0;
                const int p2 = new_len >= 2 ? (int)s.prefix[cur ^ 1][lane][new_len - 2] : 0;
                m.row[lane] = lm.order == 1 ? 0 : (lm.order == 2 ? p1 : p2 * C + p1);
            }
        }
        n = uniform_i32(n_new);
        cur ^= 1;
        wave_lds_fence();
        if constexpr (kLm)
            if (t + 1 < T) ctc_lm_fetch(m, lm.table, C, n, c0, c1, has0, has1, lmv);
        if constexpr (kTrie) {                                             // (behind the last frame too: the word ids)
            rec_node = new_node;
            if (lane < CTC_MAX_BEAM) ctc_trie_fetch(trie.nodes, new_node, rec);
        }
    }

    if constexpr (kLm || kTrie) {
        if (kTrie || lm.eos) {                                             // (wave-uniform)
            // ---- the end of the word: lane r re-scores entry r and counts the entries that beat it; absorb[rank] = the entry
            ctc_real fs = ctc_neg_inf();
            if constexpr (kLm) {
                if (lane < n) {
                    const float v = lm.table[(long)m.row[lane] * C];
                    fs = v == -__builtin_inff() ? ctc_neg_inf() : ctc_lae(s.pb[lane], s.pnb[lane]) + lm.weight * (double)v;
                }
            } else {                                                       // a word only where the node ends one
                if (lane < n && rec[5] >= 0) fs = ctc_lae(s.pb[lane], s.pnb[lane]);
                if (lane < CTC_MAX_BEAM) tr.word[lane] = rec[5];
            }
            if (lane < CTC_MAX_BEAM) s.stay_score[lane] = fs;
            wave_lds_fence();
            if (lane < CTC_MAX_BEAM) {
                int rank = 0;
                for (int q = 0; q < CTC_MAX_BEAM; ++q) {
                    const ctc_real os = s.stay_score[q];
                    rank += (os > fs || (os == fs && q < lane)) ? 1 : 0;
                }
                s.absorb[rank] = lane;
            }
            wave_lds_fence();
            if (lane < W) {
                const int src = s.absorb[lane];
                const ctc_real sc = s.stay_score[src];
                lengths[(long)b * W + lane] = sc > ctc_neg_inf() ? s.len[src] : -1;
                hyp_scores[(long)b * W + lane] = (float)sc;
                if constexpr (kTrie) trie.word_ids[(long)b * W + lane] = sc > ctc_neg_inf() ? tr.word[src] : -1;
            }
            for (int r = 0; r < W; ++r) {
                const int src = s.absorb[r], len = s.stay_score[src] > ctc_neg_inf() ? s.len[src] : -1;
                if (lane < T) paths[((long)b * W + r) * T + lane] = lane < len ? (int)s.prefix[cur][src][lane] : -1;
            }
            return;
        }
    }
    // ---- the entries are in rank order: the selection of the last frame sorted them by logaddexp(pb, pnb)
    if (lane < W) {
        const int len = s.len[lane];
        lengths[(long)b * W + lane] = len;
        hyp_scores[(long)b * W + lane] = len >= 0 ? (float)ctc_lae(s.pb[lane], s.pnb[lane]) : -__builtin_inff();
    }
    for (int r = 0; r < W; ++r) {
        const int len = s.len[r];
        if (lane < T) paths[((long)b * W + r) * T + lane] = lane < len ? (int)s.prefix[cur][r][lane] : -1;
    }
}

}  // namespace ccd
