// beam_wave.h - the wave primitives the two beam-search step kernels share (ctc_beam.h: ctc_beam_kernel, nrtr_beam.h:
// nrtr_beam_step_kernel).  Both run ONE WAVEFRONT PER SAMPLE with lane l owning the classes l and l + 64 of a row of C <= 128 classes,
// and both take these steps, which are described here and nowhere else:
//   log-probs    of an fp32 row in fp64.  Logits: the row maximum by xor shuffles, exp(x - max) to an LDS row, the sum over the row,
//                then (x - max) - log(sum); probabilities (the CTC head's softmax output): p to the LDS row, log p - log(sum).  The
//                sum runs in ascending class order - every lane adds the same C LDS words - so it is the same number on every lane
//                and the same bits on every run.  log-sum-exp of nothing is -inf, never NaN: values are finite or -inf, and -inf
//                masks a class.  Both kinds of row share ONE copy of the sum loop: with a second copy inlined into
//                ctc_beam_kernel the compiler trades 10 VGPRs for an occupancy nobody uses, and the kernel runs 1 - 2.5 % slower.
//   selection    W rounds of a wave arg-max on the key (score descending, k = rank * C + class ascending): each lane folds its own
//                candidates (k ascends along its scan, `>` keeps the lowest k of equals), six xor-shuffle steps fold the lanes.
//   trie walk    the record of a node of a lexicon's prefix tree and the child by a mask bit (ctc_trie_fetch, ctc_trie_child: lane-local,
//                the exceptions to the rule below), for the trie instances of both kernels.
// EVERY FUNCTION BELOW IS CALLED BY ALL 64 LANES OF THE WAVE (they shuffle, or fence LDS that other lanes read): the caller's
// branch around a call must be wave-uniform.  No atomics: the same input gives the same bits.
// Arithmetic is fp64 (ctc_real): the selection compares scores whose neighbours lie 1e-5 nats apart at |score| ~ 100 .. 150, which
// is one fp32 ulp.  The operation order is part of the contract (-ffp-contract=off): tests/beam_np.py restates it in numpy.
#pragma once

#include "ctc.h"

namespace ccd {

struct CtcReal2 {
    ctc_real c0, c1;                                             // the values of a lane's two classes, lane and lane + 64
};

// log(exp(a) + exp(b)); -inf when both are.  (Lane-local; the one function here that any subset of the lanes may call.)
__device__ __forceinline__ ctc_real ctc_lae(ctc_real a, ctc_real b) {
    const ctc_real m = a > b ? a : b, lo = a > b ? b : a;
    if (m == ctc_neg_inf()) return m;
    return m + ::log1p(::exp(lo - m));
}

// All 64 lanes.  The lane's best candidate (score `best`, key `best_k`) -> the wave's winner by (score descending, k ascending),
// on every lane.
__device__ __forceinline__ void beam_wave_best(ctc_real& best, int& best_k) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const ctc_real os = shfl_xor(best, m);
        const int ok = shfl_xor(best_k, m);
        if (os > best || (os == best && ok < best_k)) {
            best = os;
            best_k = ok;
        }
    }
}

// All 64 lanes.  log(e[0] + e[1] + ... + e[C - 1]), added in that order, where the lane brings e[lane] and e[lane + 64] (those
// below C) and `row` is C words of LDS that belong to the wave.  Fenced on both sides: when this returns, the caller may overwrite
// the row.
__device__ __forceinline__ ctc_real beam_wave_log_sum(ctc_real* row, int C, ctc_real e0, ctc_real e1) {
    const int c0 = lane_id(), c1 = c0 + 64;
    if (c0 < C) row[c0] = e0;
    if (c1 < C) row[c1] = e1;
    wave_lds_fence();
    ctc_real sum = 0;
    for (int c = 0; c < C; ++c) sum += row[c];                   // ascending class order, the same on every lane
    const ctc_real lsum = ::log(sum);
    wave_lds_fence();
    return lsum;
}

// All 64 lanes.  The fp64 log-probabilities of an fp32 row of logits (x - max - log sum exp(x - max)) or, `normalized`, of
// probabilities (log p - log sum p): the lane holds the values v0 / v1 of the classes lane / lane + 64 (has0 / has1: the class
// exists; the value of an absent class is not looked at) and gets their log-probabilities, -inf where the class is absent or
// masked - a -inf logit, a probability <= 0.  A row of nothing but masked classes is -inf everywhere.  A NaN is outside the
// specification (the row maximum below skips it, the sum does not).  `row`: as beam_wave_log_sum.
__device__ __forceinline__ CtcReal2 beam_wave_log_probs(float v0, float v1, bool has0, bool has1, bool normalized, ctc_real* row, int C) {
    ctc_real num0, num1, e0, e1;
    bool live0, live1;
    if (normalized) {
        live0 = has0 && v0 > 0.f;
        live1 = has1 && v1 > 0.f;
        e0 = live0 ? (ctc_real)v0 : 0;
        e1 = live1 ? (ctc_real)v1 : 0;
        num0 = live0 ? ::log(e0) : 0;
        num1 = live1 ? ::log(e1) : 0;
    } else {
        const float ninf = -__builtin_inff();
        float mx = has0 ? v0 : ninf;
        mx = has1 && v1 > mx ? v1 : mx;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const float o = shfl_xor(mx, m);
            mx = o > mx ? o : mx;
        }
        live0 = has0 && v0 > ninf;
        live1 = has1 && v1 > ninf;
        num0 = live0 ? (ctc_real)v0 - (ctc_real)mx : 0;
        num1 = live1 ? (ctc_real)v1 - (ctc_real)mx : 0;
        e0 = live0 ? ::exp(num0) : 0;
        e1 = live1 ? ::exp(num1) : 0;
    }
    const ctc_real lsum = beam_wave_log_sum(row, C, e0, e1);
    return {live0 ? num0 - lsum : ctc_neg_inf(), live1 ? num1 - lsum : ctc_neg_inf()};
}

// ---- a lexicon's prefix tree (ccd_hip.h has the node layout), walked by ctc_beam_kernel<CTC_BEAM_TRIE> and nrtr_beam_step_kernel<true>
constexpr int CTC_TRIE_NODE_WORDS = 8, CTC_TRIE_RECORD = 6;      // words per node; those the kernel reads: the mask, first_child, word_id

// The lanes below CTC_MAX_BEAM.  Requests the record of `node` (in [0, n_nodes)) into registers (consumed a frame later).
__device__ __forceinline__ void ctc_trie_fetch(const int* __restrict__ nodes, int node, int (&r)[CTC_TRIE_RECORD]) {
    const int* const p = nodes + (long)node * CTC_TRIE_NODE_WORDS;
#pragma unroll
    for (int k = 0; k < CTC_TRIE_RECORD; ++k) r[k] = p[k];
}

// The child of a node by class c (1 <= c < 128, its mask bit set): the children are contiguous in ascending class order.
__device__ __forceinline__ int ctc_trie_child(int first, unsigned long long m0, unsigned long long m1, int c) {
    const int below = c < 64 ? __builtin_popcountll(m0 & ((1ull << c) - 1ull))
                             : __builtin_popcountll(m0) + __builtin_popcountll(m1 & ((1ull << (c - 64)) - 1ull));
    return first + below;
}

}  // namespace ccd
