// ctc_lexicon.h - lexicon-constrained decoding for the CTC head (ccd_ctc_lexicon_score, ccd_ctc_lexicon_best):
//   ctc_lexicon_score_kernel   frame scores fp32 [B, T, C] (logits or probabilities) + a word list int64 [V, max_len] -> fp32 [B, V],
//                              log p(word | frames): the CTC forward log-likelihood of every word under every sample, exactly
//   ctc_lexicon_best_kernel    a score row per sample -> its `nbest` best columns by (score descending, column ascending)
// Greedy decoding and the beam return a word of their own choosing; these two answer the closed-vocabulary question - of THESE
// words, which is the most probable, and how probable is each.  The semantics are restated in numpy in tests/ctc_lexicon_np.py,
// which is the specification: the frame log-probabilities are those of the beam (beam_wave.h: fp64 over the fp32 row, the sum over the
// classes in ascending order), the recursion is the alpha recursion of ctc_loss_fwd_kernel with ctc_lse3's grouping, in fp64, rounded
// once to fp32.  A lexicon score and a beam score of the same word are therefore comparable numbers.
//
// Work split of the scoring kernel: a workgroup takes ONE SAMPLE and a STRIP of CTC_LEX_STRIP = 64 words; grid = (strips, B).
// Staging: the workgroup computes the sample's frame log-probabilities ONCE into LDS as fp64 [T][C] (dynamic LDS of T * C * 8 bytes,
// 64 KiB at the limits T = 64, C = 128, 23 KiB at T = 32, C = 92) - not the fp32 rows plus per-frame normalisers: the recursion then
// reads an emission with one LDS load and no subtraction.  Wave w takes the frames w, w + 4, ...; beam_wave_log_probs uses the frame's
// own row of the table as its scratch row.  The T x C softmax costs about as much as two words' recursions; a strip of 64 amortises it.
//
// Lane mapping of the recursion: lane = CTC state, as in ctc_loss_fwd_kernel, but PACKED: a word of max_len labels needs
// 2 max_len + 1 lanes, a segment is the smallest of 16 / 32 / 64 lanes that holds them (the template parameter SEG, chosen by the
// launcher from max_len alone - a row of `words` cannot hold more labels than max_len, so no device data is trusted), and a wave
// carries 64 / SEG = 4 / 2 / 1 words at once.  Words of 3 - 10 characters would otherwise idle 45 - 57 of the 64 lanes.  Within a
// segment lane i plays the parts it plays in ctc_target: lane i < max_len holds label i (the length is the first zero, found in the
// segment's bits of a ballot), then state i of (blank, l_1, blank, ..., l_L, blank).  Shuffles use computed lane indices inside the
// lane's own segment and are guarded by the lane's index WITHIN ITS SEGMENT.  Every loop that shuffles has a wave-uniform trip
// count (T; the groups of a strip): a segment without a word (the tail of a strip, a padding entry of `subset`) or with an
// infeasible word runs the recursion on blanks and writes -inf.
//
// The only global writes are the fp32 scores: no workspace.  No atomics: the same input gives the same bits.  What the software
// fp64 exp / log cost on the device: tools/ctc_bench.py, case `lexicon`.
#pragma once

#include "beam_wave.h"

namespace ccd {

constexpr int CTC_LEX_STRIP = 64;                                // words of a workgroup
constexpr int CTC_LEX_MAX_NBEST = 16;

// the segment's SEG bits of a ballot mask
template <int SEG>
__device__ __forceinline__ unsigned long long ctc_lex_seg_bits(unsigned long long mask, int base) {
    return SEG == 64 ? mask : (mask >> base) & ((1ull << (SEG & 63)) - 1ull);
}

// grid = (ceil(cols / CTC_LEX_STRIP), min(B, 65535)), dynamic LDS = T * C * sizeof(ctc_real).  cols = subset ? subset_cols : V.
// The launcher has checked 1 <= T <= CTC_MAX_T, 2 <= C <= CTC_MAX_C, 1 <= Lmax <= CTC_MAX_L and 2 Lmax + 1 <= SEG.
template <int SEG>
__global__ __launch_bounds__(CTC_THREADS) void ctc_lexicon_score_kernel(const float* __restrict__ scores, long sample_stride, long step_stride,
                                                                        int B, int T, int C, int normalized, const long* __restrict__ words,
                                                                        int V, int Lmax, const int* __restrict__ columns,
                                                                        const int* __restrict__ subset, int cols, float* __restrict__ out,
                                                                        long ld_out) {
    constexpr int PER_WAVE = 64 / SEG;
    ctc_real* const lp = reinterpret_cast<ctc_real*>(dynamic_smem());
    const int lane = lane_id(), wave = wave_id();
    const int i = lane & (SEG - 1), base = lane - i;                       // the lane's index within its segment, the segment's lane 0
    const int c0 = lane, c1 = lane + 64;
    const bool has0 = c0 < C, has1 = c1 < C;
    const int first = blockIdx.x * CTC_LEX_STRIP;
    const int n = cols - first < CTC_LEX_STRIP ? cols - first : CTC_LEX_STRIP;     // columns of this strip (>= 1)

    for (int b = blockIdx.y; b < B; b += gridDim.y) {                      // (one trip unless B > 65535)
        // ---- the sample's frame log-probabilities, wave w the frames w, w + 4, ...
        const float* const x = scores + (long)b * sample_stride;
        for (int t = wave; t < T; t += CTC_WAVES) {
            const float* const p = x + (long)t * step_stride;
            ctc_real* const row = lp + t * C;
            const CtcReal2 v = beam_wave_log_probs(has0 ? p[c0] : 0.f, has1 ? p[c1] : 0.f, has0, has1, normalized != 0, row, C);
            if (has0) row[c0] = v.c0;
            if (has1) row[c1] = v.c1;
        }
        __syncthreads();

        // ---- the strip: PER_WAVE words per wave and trip
        for (int g = wave * PER_WAVE; g < n; g += CTC_WAVES * PER_WAVE) {
            const int k = first + g + base / SEG;                          // the segment's column
            int v = -1;
            if (g + base / SEG < n) v = subset ? subset[(long)b * cols + k] : k;
            const bool present = v >= 0 && v < V;
            // the word on the lanes of its segment (ctc_target, segment-local)
            const long mine = present && i < Lmax ? words[(long)v * Lmax + i] : 0;
            const int L = __builtin_ctzll(ctc_lex_seg_bits<SEG>(ballot(mine == 0), base));     // (lanes >= Lmax hold 0, Lmax < SEG)
            const bool bad = i < L && (mine < 1 || mine >= C);
            const int lab = (i < L && !bad) ? (int)mine : 0;
            const int before = shfl(lab, i ? lane - 1 : lane);
            const int repeats = __builtin_popcountll(ctc_lex_seg_bits<SEG>(ballot(i >= 1 && i < L && lab == before), base));
            const unsigned long long bad_bits = ctc_lex_seg_bits<SEG>(ballot(bad), base);      // (every lane ballots: no short circuit)
            const bool feasible = present && bad_bits == 0ull && L + repeats <= T;
            const int S = 2 * L + 1;
            const int mine_s = shfl(lab, base + (i >> 1)), prev_s = shfl(lab, i >= 2 ? base + (i >> 1) - 1 : base);
            const bool live = i < S, odd = (i & 1) && live;
            const int label = odd ? mine_s : 0;
            const bool skip = odd && i >= 3 && mine_s != prev_s;

            // ---- alpha, frame by frame
            ctc_real a = i < 2 && live ? lp[label] : ctc_neg_inf();
            for (int t = 1; t < T; ++t) {
                const ctc_real e = lp[t * C + label];
                const ctc_real a1 = shfl(a, i ? lane - 1 : lane), a2 = shfl(a, i >= 2 ? lane - 2 : lane);
                const ctc_real s = ctc_lse3(a, i >= 1 ? a1 : ctc_neg_inf(), skip ? a2 : ctc_neg_inf()) + e;
                a = live ? s : ctc_neg_inf();
            }
            const ctc_real l1 = shfl(a, base + S - 1), l2 = shfl(a, base + (S >= 2 ? S - 2 : 0));
            const ctc_real ll = ctc_lse3(l1, S >= 2 ? l2 : ctc_neg_inf(), ctc_neg_inf());
            if (i == 0 && g + base / SEG < n) {
                const long col = columns ? (present ? (long)columns[v] : -1) : (long)k;
                if (col >= 0 && col < ld_out) out[(long)b * ld_out + col] = feasible ? (float)ll : -__builtin_inff();
            }
        }
        __syncthreads();                                                   // the table is rewritten for the next sample
    }
}

// grid = ceil(B / CTC_WAVES): one wavefront per sample.  Round r picks the best column behind the winner of round r - 1 in the order
// (score descending, column ascending): nothing is marked, a row of any width is read in place.  -inf (and NaN) is never picked; a
// slot left over has index -1 and score -inf.
__global__ __launch_bounds__(CTC_THREADS) void ctc_lexicon_best_kernel(const float* __restrict__ word_scores, long ld, int B, int cols, int nbest,
                                                                       int* __restrict__ index, float* __restrict__ best_out) {
    const int lane = lane_id(), b = blockIdx.x * CTC_WAVES + wave_id();
    if (b >= B) return;                                                    // (whole waves; no workgroup barrier below)
    const float* const row = word_scores + (long)b * ld;
    ctc_real last = __builtin_inf();                                       // the winner of the round before
    int last_k = -1;
    for (int r = 0; r < nbest; ++r) {
        ctc_real best = ctc_neg_inf();
        int best_k = 0x7fffffff;
        for (int k = lane; k < cols; k += 64) {                            // k ascends along the scan: `>` keeps the lowest k of equals
            const ctc_real s = (ctc_real)row[k];
            if ((s < last || (s == last && k > last_k)) && s > best) {
                best = s;
                best_k = k;
            }
        }
        beam_wave_best(best, best_k);
        const bool found = best > ctc_neg_inf();                           // wave-uniform: every lane holds the same winner
        if (lane == 0) {
            index[(long)b * nbest + r] = found ? best_k : -1;
            best_out[(long)b * nbest + r] = found ? (float)best : -__builtin_inff();
        }
        if (found) {
            last = best;
            last_k = best_k;
        } else {
            last = ctc_neg_inf();                                          // nothing is left: the later rounds find nothing either
            last_k = 0x7fffffff;
        }
    }
}

}  // namespace ccd
