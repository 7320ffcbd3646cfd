// nrtr_twopass.h - two-pass decoding (ccd_nrtr_twopass_rows, ccd_nrtr_twopass_select): the CTC beam PROPOSES W words per image, the
// NRTR decoder scores all of them in one teacher-forced pass, the two exact scores are combined and the list is ranked again
// ("attention rescoring").  The heavy stages exist (ccd_ctc_beam_search, ccd_ctc_lexicon_score, ccd_xattn_rows_fwd,
// ccd_nrtr_word_score); these two kernels are the device-side path between them.  tests/nrtr_twopass_np.py restates both in numpy
// and is the specification:
//   proposals  paths int32 [B, W, Tp], CTC classes (0 is the blank and never part of a word), -1-padded; lengths int32 [B, W], -1 for an
//              unused slot.  CTC class c is decoder class d = c - class_offset.
//   rows       slot k of image b is ELIGIBLE iff 0 <= n <= min(Tp, seq_len - 2, Lmax) for its length n and every one of its n classes
//              has c >= 1, 0 <= d < classes, d != end_idx, d != pad_idx.  It writes row b * W + k of
//                seq      int64 [B * W, seq_len]  <BOS> d1 .. dn <EOS> <PAD>..   (eligible)   <BOS> <PAD>..   (not)
//                targets  int64 [B * W, Lmax]     c1 .. cn 0..                   (eligible)   0..             (not)
//                subset   int32 [B, W]            b * W + k                      (eligible)   -1              (not)
//              The proposals are NOT trusted: a class is read only in front of a length that fits, and nothing but start_idx, end_idx,
//              pad_idx and classes in [0, classes) is ever written to seq - the rows index an embedding table.  seq may be null (the
//              CTC side alone: ops.ctc_score_paths); the rules stay.
//   select     slot k is eligible iff subset >= 0, its length lies in 0..min(Tp, max_seq_len) and both att and ctc are finite.
//              S = (1 - w) att + w ctc in fp64, a term whose weight is exactly 0 left out (w = 0: S = att; 0 * -inf never arises).
//              Rank by (S descending, slot ascending), beam_wave.h's comparison.  Rank r holds the word in decoder classes, -1-padded,
//              its length, (float)S, att, ctc and the slot; a rank left over holds (-1.., -1, -inf, -inf, -inf, -1).
// ONE WAVEFRONT PER IMAGE, four images to a workgroup (the waves share nothing: no LDS, no barrier, no atomics, no workspace).  Lane l
// owns the positions l and l + 64 of a row and, in the select kernel, slot l.  Shuffles and ballots stand in loops over W or outside
// loops; the early return of a wave without an image is wave-uniform.  Plain vector stores.
#pragma once

#include "beam_wave.h"
#include "nrtr_beam.h"

namespace ccd {

constexpr int NTP_WAVES = 4;                                       // images per workgroup
constexpr int NTP_MAX_PATH = 128;                                  // Tp: two characters per lane

struct NrtrTwopassPaths {
    const int* paths;                                              // int32: slot k of image b at paths + b * sample_stride + k * slot_stride
    long sample_stride, slot_stride;
    const int* lengths;                                            // int32 [B, W]
    int B, W, Tp, class_offset;
};

// Neither infinite nor NaN, by the exponent bits (lane-local).
__device__ __forceinline__ bool nrtr_twopass_finite(float x) {
    return (__builtin_bit_cast(unsigned, x) & 0x7f800000u) != 0x7f800000u;
}

// grid = ceil(B / 4), block = 256.  The launcher has checked 1 <= W <= 16, 1 <= Tp <= 128, 2 <= seq_len <= 128, 1 <= Lmax <= 31,
// 1 <= classes <= 128, class_offset in {0, 1}.
__global__ __launch_bounds__(64 * NTP_WAVES) void nrtr_twopass_rows_kernel(NrtrTwopassPaths p, int classes, int start_idx, int end_idx,
                                                                          int pad_idx, long long* __restrict__ seq, int seq_len,
                                                                          long long* __restrict__ targets, int Lmax,
                                                                          int* __restrict__ subset) {
    const int lane = lane_id();
    const int b = blockIdx.x * NTP_WAVES + (threadIdx.x >> 6);
    if (b >= p.B) return;                                                  // wave-uniform
    int longest = p.Tp < seq_len - 2 ? p.Tp : seq_len - 2;
    longest = Lmax < longest ? Lmax : longest;
    for (int k = 0; k < p.W; ++k) {                                        // wave-uniform trip count
        const long r = (long)b * p.W + k;
        const int n = p.lengths[r];
        const bool fits = n >= 0 && n <= longest;                          // wave-uniform
        const int* const path = p.paths + (long)b * p.sample_stride + (long)k * p.slot_stride;
        // position q of the row holds character q - 1: the lane reads the characters of its two positions (n <= 126: all are read)
        int d[2];
        bool bad = false;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int j = lane + 64 * i - 1;
            d[i] = -1;
            if (fits && j >= 0 && j < n) {
                const int c = path[j];
                d[i] = c - p.class_offset;
                bad = bad || c < 1 || d[i] < 0 || d[i] >= classes || d[i] == end_idx || d[i] == pad_idx;
            }
        }
        const bool eligible = fits && ballot(bad) == 0ull;                 // wave-uniform
        if (seq) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int q = lane + 64 * i;
                if (q >= seq_len) continue;
                int tok = q == 0 ? start_idx : pad_idx;
                if (eligible && q >= 1) tok = q <= n ? d[i] : (q == n + 1 ? end_idx : pad_idx);
                seq[r * seq_len + q] = tok;
            }
        }
        if (lane < Lmax) targets[r * Lmax + lane] = eligible && lane < n ? path[lane] : 0;
        if (lane == 0) subset[r] = eligible ? (int)r : -1;
    }
}

// grid = ceil(B / 4), block = 256.  The launcher has checked 1 <= W <= 16, 1 <= Tp <= 128, 1 <= T <= 128, 0 <= w <= 1, class_offset in
// {0, 1}.  att fp32 [B * W], ctc fp32 [B, W], subset int32 [B, W]; out_paths int32 [B, W, T], the others [B, W].
__global__ __launch_bounds__(64 * NTP_WAVES) void nrtr_twopass_select_kernel(NrtrTwopassPaths p, const float* __restrict__ att,
                                                                            const float* __restrict__ ctc,
                                                                            const int* __restrict__ subset, ctc_real w, int T,
                                                                            int* __restrict__ out_paths, int* __restrict__ out_lengths,
                                                                            float* __restrict__ scores, float* __restrict__ att_scores,
                                                                            float* __restrict__ ctc_scores, int* __restrict__ source) {
    const int lane = lane_id();
    const int b = blockIdx.x * NTP_WAVES + (threadIdx.x >> 6);
    if (b >= p.B) return;                                                  // wave-uniform
    const float ninf = -__builtin_inff();
    const int longest = p.Tp < T ? p.Tp : T;
    float a = ninf, c = ninf;
    int n = -1;
    ctc_real S = ctc_neg_inf();                                            // the lane's slot; -inf: not (or no longer) a candidate
    if (lane < p.W) {
        const long r = (long)b * p.W + lane;
        a = att[r];
        c = ctc[r];
        n = p.lengths[r];
        const bool finite = nrtr_twopass_finite(a) && nrtr_twopass_finite(c);
        if (subset[r] >= 0 && n >= 0 && n <= longest && finite)
            S = w == 0 ? (ctc_real)a : (w == 1 ? (ctc_real)c : (1 - w) * (ctc_real)a + w * (ctc_real)c);
    }
    // W rounds of the wave arg-max by (S descending, slot ascending); lane r keeps the winner of round r
    ctc_real win_S = ctc_neg_inf();
    float win_a = ninf, win_c = ninf;
    int win_k = -1, win_n = -1;
    for (int r = 0; r < p.W; ++r) {                                        // wave-uniform trip count
        ctc_real best = S;
        int best_k = lane;
        beam_wave_best(best, best_k);
        const float ba = shfl(a, best_k), bc = shfl(c, best_k);
        const int bn = shfl(n, best_k);
        if (best == ctc_neg_inf()) continue;                               // (wave-uniform) nothing left: the ranks from r on stay empty
        if (lane == best_k) S = ctc_neg_inf();
        if (lane == r) {
            win_S = best;
            win_a = ba;
            win_c = bc;
            win_k = best_k;
            win_n = bn;
        }
    }
    if (lane < p.W) {
        const long r = (long)b * p.W + lane;
        out_lengths[r] = win_n;
        scores[r] = (float)win_S;
        att_scores[r] = win_a;
        ctc_scores[r] = win_c;
        source[r] = win_k;
    }
    for (int r = 0; r < p.W; ++r) {                                        // wave-uniform trip count
        const int k = shfl(win_k, r), len = shfl(win_n, r);
        const int* const path = p.paths + (long)b * p.sample_stride + (long)(k < 0 ? 0 : k) * p.slot_stride;
        int* const dst = out_paths + ((long)b * p.W + r) * T;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int j = lane + 64 * i;
            if (j < T) dst[j] = k >= 0 && j < len ? path[j] - p.class_offset : -1;      // (len <= min(Tp, T): checked above)
        }
    }
}

}  // namespace ccd
