// ctc_align.h - CTC forced alignment for the CTC head (ccd_ctc_align):
//   ctc_align_kernel   frame scores fp32 [B, T, C] (logits or probabilities) + zero-padded targets int64 [N, Lmax] (+ rows int32 [N]:
//                      the sample of every target) -> the best single alignment of each target: frame_char int32 [N, T], spans int32
//                      [N, Lmax, 2], char_logp fp32 [N, Lmax], score fp32 [N].
// The loss sums a word over all its alignments; this is the max-plus twin of that recursion - WHERE the characters of a word sit and
// how sure the network is of each.  The semantics are restated in numpy in tests/ctc_align_np.py, which is the specification:
//   lp          the frame log-probabilities of the beam and the lexicon (beam_wave.h: fp64 over the fp32 row, the sum over the classes
//               in ascending order);
//   v_0(s)      lp[0, l'_s] for s < 2, -inf behind; v_t(s) = max(v_{t-1}(s), v_{t-1}(s - 1), v_{t-1}(s - 2) where the loss allows the
//               skip) + lp[t, l'_s] over l' = (blank, l_1, blank, ..., l_L, blank), in fp64;
//   tie rule    the candidates in the order s, s - 1, s - 2, a later one replaces the current one only where it is STRICTLY greater; the
//               path ends in state S - 1 unless v(S - 2) is strictly greater.  Uniform frames align `ab` over five frames as a b _ _ _.
//
// Lane mapping: ONE WAVEFRONT PER TARGET ROW, lane s = state s, as ctc_loss_fwd_kernel (ctc_target is that kernel's).  In the prologue
// the same lanes play another part, again as in that kernel: lane t < T folds frame t - its row maximum and the log of its sum over the
// classes in ascending order - and keeps the two numbers; the emission of state s at frame t is then (x[t, l'_s] - max_t) - lsum_t
// (log p - lsum_t for probabilities) with max_t and lsum_t shuffled from lane t.  These are the operations of beam_wave_log_probs on the
// same values in the same order, so lp has the beam's bits (tests/ctc_align_checks.py: a word with ONE alignment scores the bits of
// ccd_ctc_lexicon_score), but the code is not shared: beam_wave_log_probs spends the whole wave on one frame - every lane adds the same
// C numbers out of an LDS row, T times in a row - which suits a kernel that needs all C log-probabilities of the frame on the lanes and
// made this one, which needs S of them, slower than the loss (63 us against 48 us at 512 x 32 x 92).  The recursion itself holds no exp
// and no log for logits - two shuffles, two compares, one add per frame; for probabilities the emission costs its own log, off the
// dependent chain.
// Backpointers: which of the three candidates won is 2 bits per (state, frame); a lane keeps its own column - 64 frames x 2 bits - in
// two 64-bit registers, nothing is stored.  The backtrace walks the frames downwards with the state in a wave-uniform register: one
// shuffle per frame (the 2 bits of the lane the path is on), lane t keeps the state of frame t.
// Character sums: lane t forms lp[t, class of its state] again from its own frame's maximum and log-sum (the same operations: the same
// bits as the emission the recursion added), and lane j adds the frames of character j in ascending frame order (T rounds of two
// shuffles).  score is v at the end state: that very sum over all frames.
// No LDS, no workspace, no atomics: the same input gives the same bits.  Every loop that shuffles has a wave-uniform trip count (T); the
// exits before them (row beyond N, infeasible target) are wave-uniform.  The frame prologue (lane t walks frame t's C classes serially,
// rows 4 * step_stride bytes apart: uncoalesced, T of 64 lanes busy) is ctc_loss_fwd_kernel's and has its price.
// Measured (tools/ctc_bench.py, case `align`, profiles/ctc_align.json; 512 x 32 x 92): 0.040 ms on logits next to 0.048 ms of
// ctc_loss_fwd_kernel on the same rows, 0.028 ms on probabilities (no exp in the prologue).
#pragma once

#include "ctc.h"

namespace ccd {

// lp of one class of a frame from its fp32 score, the frame's maximum and the log of its sum: beam_wave_log_probs' operations.
__device__ __forceinline__ ctc_real ctc_align_lp(float xv, float mx, ctc_real lsum, int normalized) {
    if (normalized) return xv > 0.f ? ::log((ctc_real)xv) - lsum : ctc_neg_inf();
    return xv > -__builtin_inff() ? ((ctc_real)xv - (ctc_real)mx) - lsum : ctc_neg_inf();
}

// Padding of an infeasible row.  All 64 lanes.
__device__ __forceinline__ void ctc_align_pad(int lane, int T, int Lmax, int* __restrict__ fc, int* __restrict__ sp, float* __restrict__ cl,
                                              float* __restrict__ sc) {
    if (lane < T) fc[lane] = -1;
    if (lane < Lmax) {
        sp[2 * lane] = -1;
        sp[2 * lane + 1] = -1;
        cl[lane] = 0.f;
    }
    if (lane == 0) sc[0] = -__builtin_inff();
}

// grid = ceil(N / CTC_WAVES).  The launcher has checked 1 <= T <= CTC_MAX_T, 1 <= C <= CTC_MAX_C, 1 <= Lmax <= CTC_MAX_L.
__global__ __launch_bounds__(CTC_THREADS) void ctc_align_kernel(const float* __restrict__ scores, long sample_stride, long step_stride, int B,
                                                                int T, int C, int normalized, const long* __restrict__ targets, int N,
                                                                int Lmax, const int* __restrict__ rows, int* __restrict__ frame_char,
                                                                int* __restrict__ spans, float* __restrict__ char_logp,
                                                                float* __restrict__ score) {
    const int lane = lane_id(), n = blockIdx.x * CTC_WAVES + wave_id();
    if (n >= N) return;                                                    // (whole waves; no workgroup barrier below)
    int* const fc = frame_char + (long)n * T;
    int* const sp = spans + (long)n * Lmax * 2;
    float* const cl = char_logp + (long)n * Lmax;
    const CtcTarget tg = ctc_target(targets + (long)n * Lmax, Lmax, T, C);
    const int b = rows ? rows[n] : n;                                      // wave-uniform; never an index unless inside [0, B)
    if (!tg.feasible || b < 0 || b >= B) {
        ctc_align_pad(lane, T, Lmax, fc, sp, cl, score + n);
        return;
    }
    const float* const x = scores + (long)b * sample_stride;
    const bool live = lane < tg.S;
    const float ninf = -__builtin_inff();

    // ---- lane t: the maximum of frame t and the log of its sum over the classes, in ascending order
    float mx = 0.f;
    ctc_real lsum = 0;
    if (lane < T) {
        const float* const p = x + (long)lane * step_stride;
        ctc_real sum = 0;
        if (normalized) {
            for (int c = 0; c < C; ++c) sum += p[c] > 0.f ? (ctc_real)p[c] : 0;
        } else {
            mx = ninf;
            for (int c = 0; c < C; ++c) mx = p[c] > mx ? p[c] : mx;
            for (int c = 0; c < C; ++c) sum += p[c] > ninf ? ::exp((ctc_real)p[c] - (ctc_real)mx) : 0;
        }
        lsum = ::log(sum);
    }

    // ---- v and the backpointers, frame by frame (the next frame's score is requested before this frame's arithmetic)
    ctc_real v = ctc_neg_inf();
    unsigned long long bp_lo = 0ull, bp_hi = 0ull;                         // bits 2 t, 2 t + 1 of lo (t < 32) / hi: the winner at frame t
    float x_next = x[tg.label];
    for (int t = 0; t < T; ++t) {
        const float xv = x_next;
        if (t + 1 < T) x_next = x[(long)(t + 1) * step_stride + tg.label];
        const ctc_real e = ctc_align_lp(xv, shfl(mx, t), shfl(lsum, t), normalized);
        if (t == 0) {
            v = lane < 2 && live ? e : ctc_neg_inf();
        } else {
            const ctc_real v1 = shfl(v, lane ? lane - 1 : 0), v2 = shfl(v, lane >= 2 ? lane - 2 : 0);
            ctc_real best = v;
            unsigned long long k = 0ull;
            if (lane >= 1 && v1 > best) {
                best = v1;
                k = 1ull;
            }
            if (tg.skip && v2 > best) {
                best = v2;
                k = 2ull;
            }
            v = live ? best + e : ctc_neg_inf();
            if (t < 32) bp_lo |= k << (2 * t);
            else bp_hi |= k << (2 * (t - 32));
        }
    }
    const ctc_real end1 = shfl(v, tg.S - 1), end2 = shfl(v, tg.S >= 2 ? tg.S - 2 : 0);
    const bool early = tg.S >= 2 && end2 > end1;
    const ctc_real total = early ? end2 : end1;
    if (!(total > ctc_neg_inf())) {                                        // wave-uniform: a masked class on every alignment
        ctc_align_pad(lane, T, Lmax, fc, sp, cl, score + n);
        return;
    }

    // ---- the backtrace: lane t keeps the state of frame t
    int s = early ? tg.S - 2 : tg.S - 1, state = 0;
    for (int t = T - 1; t >= 0; --t) {
        if (lane == t) state = s;
        const int k = (int)((t < 32 ? bp_lo >> (2 * t) : bp_hi >> (2 * (t - 32))) & 3ull);
        s -= shfl(k, s);                                                   // (frame 0 holds no backpointer: k = 0)
    }

    // ---- lane t: the emission of its frame on the path, as the recursion added it
    const int cls = shfl(tg.label, state);
    ctc_real lp = 0;
    if (lane < T) {
        lp = ctc_align_lp(x[(long)lane * step_stride + cls], mx, lsum, normalized);
        fc[lane] = (state & 1) ? state >> 1 : -1;
    }
    // ---- lane j: the frames of character j, in ascending order
    int first = -1, last = -1;
    ctc_real sum = 0;
    for (int t = 0; t < T; ++t) {
        const int st = shfl(state, t);
        const ctc_real lpt = shfl(lp, t);
        if (st == 2 * lane + 1) {
            if (first < 0) first = t;
            last = t;
            sum += lpt;
        }
    }
    if (lane < Lmax) {                                                     // (lane >= L: no frame is in state 2 lane + 1 >= S)
        sp[2 * lane] = first;
        sp[2 * lane + 1] = last;
        cl[lane] = (float)sum;
    }
    if (lane == 0) score[n] = (float)total;
}

}  // namespace ccd
