// ctc.h - the CTC recognition head (SVTR style: pool the 8 x 32 token grid over its height, one linear layer, CTC):
//   ctc_pool_fwd_kernel / ctc_pool_bwd_kernel   tokens bf16 [N, rows * cols, E] <-> frames bf16 [N * cols, E] (mean over the rows)
//   ctc_loss_fwd_kernel    logits fp32 [B * T, ldl] + zero-padded targets -> nll [B], the forward variables into the workspace
//   ctc_loss_acc_kernel    per-sample results -> acc {sum nll / max(L, 1), B, infeasible samples}, one workgroup, a fixed order
//   ctc_loss_bwd_kernel    workspace -> d_logits bf16 [B * T, ldd]
//   ctc_greedy_kernel      logits -> best path (arg-max per frame, repeats collapsed, blanks dropped) with its confidences
// Semantics of the loss: torch.nn.CTCLoss(blank=0, reduction='mean', zero_infinity=True) on log_softmax(logits).
//
// Lane mapping of the loss kernels: ONE WAVEFRONT PER SAMPLE, lane s = state s of the extended label sequence
// l' = (blank, l_1, blank, l_2, ..., l_L, blank), S = 2 L + 1 <= 63 states (lane 63 idles).  alpha_t(s) needs alpha_{t-1} of
// the lanes s, s - 1 and (odd s whose label differs from the one before) s - 2: two shuffles per frame; beta_t(s) the lanes
// s, s + 1, s + 2.  In the prologue the same lanes play other parts: lane i < Lmax holds target i (the length is the first zero,
// found by a ballot), lane t < T folds frame t's log-sum-exp over the classes.  Every loop that shuffles has a wave-uniform
// trip count (T, L, or the bits of a ballot mask).
//
// Arithmetic: the recursion is in the log domain with torch's own grouping, log(exp(a1 - m) + exp(a2 - m) + exp(a3 - m)) + m + e
// with m = 0 where all three are -inf (so that -inf stays -inf instead of NaN).  It is carried in fp64 (ctc_real): the
// gradient is softmax - posterior, and where the two nearly cancel an fp32 alpha + beta (|alpha| ~ 150 at T = 32: one part in
// 10^5 after exp) is wrong in the digits bf16 keeps.  With `typedef float ctc_real` 6 of the 260 504 gradient elements of
// tests/ctc_checks.py are neither the fp64 gradient rounded to bf16 nor its neighbour (and nll carries exactly the 4.3e-4 of
// torch's fp32 CPU kernel, whose grouping this is); in fp64 none is, and nll is off by its own rounding to fp32.  The price:
// gfx950 has no fp64 exp or log instruction, so every ::exp / ::log below is a software sequence of fp64 FMAs where fp32 would
// be one v_exp_f32 / v_log_f32 - per sample and direction about 4 T S of them in the recursion and C T in the softmax - and the
// workspace is T * 65 + 2 doubles per sample.  What that costs on the device is not measured (tools/ctc_bench.py, case `loss`).
// The frame prologue (lane t walks frame t's C classes serially, rows 4 ldl bytes apart: uncoalesced, T of 64 lanes busy) is
// the simplest form, as in text_score_kernel; lanes over classes with wave_max / wave_sum per frame would coalesce.  Not measured.
//
// Class sums of the backward pass (the posterior of class c at frame t is the sum over the states that carry c) in a fixed
// order: the blanks (even lanes) by the xor tree of the wave, a repeated character at its first occurrence by walking the
// later occurrences in ascending state order (a ballot mask; nothing to walk for a word without repeated characters).
#pragma once

#include "common.h"

namespace ccd {

constexpr int CTC_THREADS = 256;
constexpr int CTC_WAVES = CTC_THREADS / 64;
constexpr int CTC_MAX_T = 64, CTC_MAX_C = 128, CTC_MAX_L = 31;
typedef double ctc_real;

// workspace of a sample, in ctc_real: alpha [T][64], lse [T], nll, state (L, or -1 - L when infeasible)
constexpr long ctc_ws_stride(int T) { return (long)T * 65 + 2; }

__device__ __forceinline__ ctc_real ctc_neg_inf() { return -(ctc_real)__builtin_inf(); }
// log(exp(a) + exp(b) + exp(c)), -inf when all three are
__device__ __forceinline__ ctc_real ctc_lse3(ctc_real a, ctc_real b, ctc_real c) {
    ctc_real m = a > b ? a : b;
    m = m > c ? m : c;
    if (m == ctc_neg_inf()) m = 0;
    return ::log(::exp(a - m) + ::exp(b - m) + ::exp(c - m)) + m;
}
__device__ __forceinline__ ctc_real ctc_wave_sum(ctc_real v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += shfl_xor(v, m);
    return v;
}

// The target of a sample on the lanes of its wave.
struct CtcTarget {
    int L, S;          // label length, states
    int label;         // lane s: l'_s (0 for the blanks, the idle lanes and a label outside [1, C))
    bool skip;         // lane s: the transition s - 2 -> s exists
    bool first;        // odd lane s: no earlier state carries this label
    bool feasible;     // every label inside [1, C) and L + adjacent repeats <= T
};
__device__ __forceinline__ CtcTarget ctc_target(const long* __restrict__ tg, int Lmax, int T, int C) {
    const int lane = lane_id();
    const long mine = lane < Lmax ? tg[lane] : 0;
    const int L = __builtin_ctzll(ballot(mine == 0));                      // (lanes >= Lmax hold 0: a bit is always set, L <= Lmax <= 31)
    const bool bad = lane < L && (mine < 1 || mine >= C);
    const int lab = (lane < L && !bad) ? (int)mine : 0;
    const int before = shfl(lab, lane ? lane - 1 : 0);
    const int repeats = __builtin_popcountll(ballot(lane >= 1 && lane < L && lab == before));
    CtcTarget r;
    r.L = L;
    r.S = 2 * L + 1;
    r.feasible = ballot(bad) == 0 && L + repeats <= T;
    const int mine_s = shfl(lab, lane >> 1), prev_s = shfl(lab, lane >= 2 ? (lane >> 1) - 1 : 0);
    const bool odd = (lane & 1) && lane < r.S;
    r.label = odd ? mine_s : 0;
    r.skip = odd && lane >= 3 && mine_s != prev_s;
    r.first = odd;
    for (int j = 0; j < L; ++j) {
        const int lj = shfl(lab, j);
        if (odd && j < (lane >> 1) && lj == r.label) r.first = false;
    }
    return r;
}

// grid = ceil(B / CTC_WAVES)
__global__ __launch_bounds__(CTC_THREADS) void ctc_loss_fwd_kernel(const float* __restrict__ logits, long ldl, int B, int T, int C,
                                                                   const long* __restrict__ targets, int Lmax, float* __restrict__ nll,
                                                                   ctc_real* __restrict__ ws) {
    const int lane = lane_id(), b = blockIdx.x * CTC_WAVES + wave_id();
    if (b >= B) return;                                                    // (whole waves; no workgroup barrier below)
    const CtcTarget tg = ctc_target(targets + (long)b * Lmax, Lmax, T, C);
    const float* const x = logits + (long)b * T * ldl;
    ctc_real* const w = ws + (long)b * ctc_ws_stride(T);
    ctc_real* const w_lse = w + (long)T * 64;
    if (!tg.feasible) {
        if (lane == 0) {
            nll[b] = 0.f;
            w_lse[T] = 0;
            w_lse[T + 1] = -1 - tg.L;
        }
        return;
    }
    // ---- lane t: log-sum-exp of frame t over the classes
    ctc_real lse = 0;
    if (lane < T) {
        const float* const p = x + (long)lane * ldl;
        float mx = p[0];
        for (int c = 1; c < C; ++c) mx = p[c] > mx ? p[c] : mx;
        ctc_real sum = 0;
        for (int c = 0; c < C; ++c) sum += ::exp((ctc_real)p[c] - (ctc_real)mx);
        lse = (ctc_real)mx + ::log(sum);
        w_lse[lane] = lse;
    }
    // ---- alpha, frame by frame (the next frame's emission is requested before this frame's arithmetic)
    const bool live = lane < tg.S;
    const ctc_real lse0 = shfl(lse, 0);                                    // (every lane takes part in a shuffle)
    ctc_real a = lane < 2 && live ? (ctc_real)x[tg.label] - lse0 : ctc_neg_inf();
    w[lane] = a;
    float e_next = T > 1 ? x[ldl + tg.label] : 0.f;
    for (int t = 1; t < T; ++t) {
        const ctc_real e = (ctc_real)e_next - shfl(lse, t);
        if (t + 1 < T) e_next = x[(long)(t + 1) * ldl + tg.label];
        const ctc_real a1 = shfl(a, lane ? lane - 1 : 0), a2 = shfl(a, lane >= 2 ? lane - 2 : 0);
        const ctc_real s = ctc_lse3(a, lane >= 1 ? a1 : ctc_neg_inf(), tg.skip ? a2 : ctc_neg_inf()) + e;
        a = live ? s : ctc_neg_inf();
        w[(long)t * 64 + lane] = a;
    }
    const ctc_real l1 = shfl(a, tg.S - 1), l2 = shfl(a, tg.S >= 2 ? tg.S - 2 : 0);
    const ctc_real ll = ctc_lse3(l1, tg.S >= 2 ? l2 : ctc_neg_inf(), ctc_neg_inf());
    if (lane == 0) {
        const bool ok = ll > ctc_neg_inf();                                // (a -inf logit on every alignment: torch's inf, zeroed)
        nll[b] = ok ? (float)-ll : 0.f;
        w_lse[T] = ok ? -ll : 0;
        w_lse[T + 1] = ok ? tg.L : -1 - tg.L;
    }
}

// One workgroup.  Thread t adds samples t, t + 256, ... in ascending order, the partial sums meet in a tree in LDS: no atomics,
// the same batch gives the same bits.
__global__ __launch_bounds__(CTC_THREADS) void ctc_loss_acc_kernel(const ctc_real* __restrict__ ws, int B, int T, float* __restrict__ acc) {
    __shared__ double sums[CTC_THREADS];
    __shared__ int bad[CTC_THREADS];
    const int t = threadIdx.x;
    double s = 0.0;
    int n = 0;
    for (int i = t; i < B; i += CTC_THREADS) {
        const ctc_real* const m = ws + (long)i * ctc_ws_stride(T) + (long)T * 65;
        const int state = (int)m[1];
        if (state >= 0) s += m[0] / (double)(state > 1 ? state : 1);
        else ++n;
    }
    sums[t] = s;
    bad[t] = n;
    __syncthreads();
    for (int h = CTC_THREADS / 2; h > 0; h >>= 1) {
        if (t < h) {
            sums[t] += sums[t + h];
            bad[t] += bad[t + h];
        }
        __syncthreads();
    }
    if (t == 0) {
        acc[0] = (float)sums[0];
        acc[1] = (float)B;
        acc[2] = (float)bad[0];
    }
}

// grid = ceil(B / CTC_WAVES).  d_logits[b, t, c] = (softmax - posterior of class c) * upstream / (max(L, 1) * B), zero for c >= C and
// for an infeasible sample.
__global__ __launch_bounds__(CTC_THREADS) void ctc_loss_bwd_kernel(const float* __restrict__ logits, long ldl, int B, int T, int C,
                                                                   const long* __restrict__ targets, int Lmax,
                                                                   const ctc_real* __restrict__ ws, const float* __restrict__ upstream,
                                                                   bf16_t* __restrict__ d_logits, long ldd) {
    const int lane = lane_id(), b = blockIdx.x * CTC_WAVES + wave_id();
    if (b >= B) return;
    const ctc_real* const w = ws + (long)b * ctc_ws_stride(T);
    const ctc_real* const w_lse = w + (long)T * 64;
    bf16_t* const d = d_logits + (long)b * T * ldd;
    if (w_lse[T + 1] < 0) {                                                // wave-uniform
        for (long i = lane; i < (long)T * ldd; i += 64) d[i] = 0;
        return;
    }
    const CtcTarget tg = ctc_target(targets + (long)b * Lmax, Lmax, T, C);
    const float* const x = logits + (long)b * T * ldl;
    const ctc_real nll = w_lse[T];
    const ctc_real scale = (ctc_real)(upstream ? upstream[0] : 1.f) / ((ctc_real)(tg.L > 1 ? tg.L : 1) * (ctc_real)B);
    const ctc_real lse = lane < T ? w_lse[lane] : 0;
    const bool live = lane < tg.S;
    // the transition s -> s + 2 exists where s + 2 -> s's own rule says so
    const bool skip2 = shfl(tg.skip ? 1 : 0, lane + 2 < 64 ? lane + 2 : 63) != 0 && lane + 2 < tg.S;
    // the state whose class sum a class reads: classes lane and lane + 64 (-1: no state carries it)
    int state_of[2] = {lane == 0 ? 0 : -1, -1};
    for (int j = 0; j < tg.L; ++j) {
        const int lj = shfl(tg.label, 2 * j + 1);
        if (state_of[0] < 0 && lj == lane) state_of[0] = 2 * j + 1;
        if (state_of[1] < 0 && lj == lane + 64) state_of[1] = 2 * j + 1;
    }
    const unsigned long long later = ballot(live && (lane & 1) && !tg.first);      // later occurrences of a repeated character

    ctc_real beta = ctc_neg_inf();
    float e_next = x[(long)(T - 1) * ldl + tg.label];
    for (int t = T - 1; t >= 0; --t) {
        const ctc_real lse_t = shfl(lse, t);
        const ctc_real e = (ctc_real)e_next - lse_t;
        if (t > 0) e_next = x[(long)(t - 1) * ldl + tg.label];
        if (t == T - 1) {
            beta = live && lane + 2 >= tg.S ? e : ctc_neg_inf();
        } else {
            const ctc_real b1 = shfl(beta, lane + 1 < 64 ? lane + 1 : 63), b2 = shfl(beta, lane + 2 < 64 ? lane + 2 : 63);
            const ctc_real s = ctc_lse3(beta, lane + 1 < tg.S ? b1 : ctc_neg_inf(), skip2 ? b2 : ctc_neg_inf()) + e;
            beta = live ? s : ctc_neg_inf();
        }
        // posterior of the state; alpha and beta both hold this frame's emission
        const ctc_real ab = w[(long)t * 64 + lane] + beta;
        ctc_real post = live && ab > ctc_neg_inf() ? ::exp(ab - e + nll) : 0;
        const ctc_real blanks = ctc_wave_sum((lane & 1) ? 0 : post);
        if (later) {
            unsigned long long walk = later;
            while (walk) {
                const int p = __builtin_ctzll(walk);
                walk &= walk - 1;
                const ctc_real v = shfl(post, p);
                const int lp = shfl(tg.label, p);
                if (tg.first && lp == tg.label) post += v;
            }
        }
        if (lane == 0) post = blanks;
        const float* const row = x + (long)t * ldl;
        bf16_t* const out = d + (long)t * ldd;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int c = lane + 64 * h;
            const ctc_real g = shfl(post, state_of[h] < 0 ? 0 : state_of[h]);
            if (c < C) out[c] = f2bf((float)((::exp((ctc_real)row[c] - lse_t) - (state_of[h] < 0 ? 0 : g)) * scale));
        }
        for (long c = C + lane; c < ldd; c += 64) out[c] = 0;
    }
}

// grid = ceil(B / CTC_WAVES): lane t takes frame t.  conf = softmax probability of the arg-max = 1 / sum exp(x - max).
__global__ __launch_bounds__(CTC_THREADS) void ctc_greedy_kernel(const float* __restrict__ logits, long sample_stride, long step_stride, int B,
                                                                 int T, int C, int* __restrict__ path, int* __restrict__ length,
                                                                 float* __restrict__ conf) {
    __shared__ int cls_lds[CTC_THREADS];
    __shared__ float prob_lds[CTC_THREADS];
    const int lane = lane_id(), b = blockIdx.x * CTC_WAVES + wave_id();
    if (b >= B) return;
    int* const run_cls = cls_lds + wave_id() * 64;
    float* const run_prob = prob_lds + wave_id() * 64;
    int cls = -1;
    float prob = 0.f;
    if (lane < T) {
        const float* const p = logits + (long)b * sample_stride + (long)lane * step_stride;
        float best = p[0];
        cls = 0;
        for (int c = 1; c < C; ++c)
            if (p[c] > best) {
                best = p[c];
                cls = c;
            }
        float sum = 0.f;
        for (int c = 0; c < C; ++c) sum += expf(p[c] - best);
        prob = 1.0f / sum;
    }
    const int before = shfl(cls, lane ? lane - 1 : 0);
    const bool keep = cls > 0 && (lane == 0 || cls != before);
    const unsigned long long kept = ballot(keep);
    const int n = __builtin_popcountll(kept), at = __builtin_popcountll(kept & ((1ull << lane) - 1ull));
    if (keep) {                                                            // left-align through LDS: every lane then stores its own slot
        run_cls[at] = cls;
        run_prob[at] = prob;
    }
    wave_lds_fence();
    if (lane < T) {
        path[(long)b * T + lane] = lane < n ? run_cls[lane] : -1;
        conf[(long)b * T + lane] = lane < n ? run_prob[lane] : 0.f;
    }
    if (lane == 0) length[b] = n;
}

// ---- frame pooling: one thread per 8 channels of a frame
__global__ __launch_bounds__(256) void ctc_pool_fwd_kernel(const bf16_t* __restrict__ tokens, bf16_t* __restrict__ frames, long chunks, int rows,
                                                           int cols, int E8) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < chunks; i += (long)gridDim.x * 256) {
        const long frame = i / E8;
        const int e8 = (int)(i - frame * E8);
        const long n = frame / cols;
        const int c = (int)(frame - n * cols);
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, v[8];
        for (int r = 0; r < rows; ++r) {
            const u32x4 w = *reinterpret_cast<const u32x4*>(tokens + ((n * rows + r) * cols + c) * (long)E8 * 8 + e8 * 8);
            unpack8(w, v);
#pragma unroll
            for (int k = 0; k < 8; ++k) acc[k] += v[k];
        }
        const float inv = 1.0f / (float)rows;
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[k] *= inv;
        *reinterpret_cast<u32x4*>(frames + i * 8) = pack8(acc);
    }
}
__global__ __launch_bounds__(256) void ctc_pool_bwd_kernel(const bf16_t* __restrict__ d_frames, bf16_t* __restrict__ d_tokens, long chunks, int rows,
                                                           int cols, int E8) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < chunks; i += (long)gridDim.x * 256) {
        const long frame = i / E8;
        const int e8 = (int)(i - frame * E8);
        const long n = frame / cols;
        const int c = (int)(frame - n * cols);
        float v[8];
        unpack8(*reinterpret_cast<const u32x4*>(d_frames + i * 8), v);
        const float inv = 1.0f / (float)rows;
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] *= inv;
        const u32x4 w = pack8(v);
        for (int r = 0; r < rows; ++r) *reinterpret_cast<u32x4*>(d_tokens + ((n * rows + r) * cols + c) * (long)E8 * 8 + e8 * 8) = w;
    }
}

}  // namespace ccd
