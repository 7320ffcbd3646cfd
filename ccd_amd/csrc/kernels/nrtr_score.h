// nrtr_score.h - scoring GIVEN words with the NRTR attention decoder (ccd_xattn_rows_fwd, ccd_nrtr_word_score; inference only):
//   xattn_rows_fwd_kernel    the encoder-decoder attention of R word rows (Tq <= 32 queries each) against the keys and values of the
//                            sample that owns the row - row_ptr int32 [B + 1] in CSR form says which - so the 256 image tokens of a
//                            sample are never replicated per word; at the caller's wish the first and second moments of every
//                            attention map over the 8 x 32 token grid (the probabilities themselves are never written)
//   nrtr_word_score_kernel   the teacher-forced logits of those rows -> log p of every character, log p(word <EOS> | image), the
//                            word's length and where the decoder looked for every character
// The semantics of the second kernel are restated in numpy in tests/nrtr_score_np.py, which is the specification.
//
// xattn_rows_fwd_kernel.  The arithmetic of one row is xattn_fwd_kernel's (decoder_xattn.h), instruction for instruction: the same
// MFMA shapes in the same order, fast_exp2, the same max / sum merge order over the four waves, the same bf16 rounding of P, the same
// order of the merge sum - `out` is BIT-EQUAL to ccd_dec_attn_fwd on K / V gathered per row (no dropout, no mask, no lse).
// What differs is who reads K and V:
//   grid (B * H, NC), 4 waves.  Workgroup (b, h, c) takes the chunks c, c + NC, .. of sample b's rows, CH rows to a chunk (the rule:
//   xattn_rows_chunk below; any CH >= 1 and any NC >= 1 give the same bits, a row's result depends on nothing but the row).  It loads
//   its 64 keys per wave as MFMA fragments into registers ONCE and stages the V^T image into LDS ONCE (att_stage_transposed), then
//   walks its rows: Q of the row as fragments straight from global memory (the next row's are requested before this row's products
//   start), S^T = K.Q^T, the statistics of the four key slices merged through LDS, P.V, the four partial outputs summed through LDS.
//   A workgroup without rows - a sample that owns none, a chunk slot behind the sample's last row - leaves before it loads anything.
//   HBM bytes: 64 KB of K / V per (sample, head, chunk) + 8 KB of q / out per (row, head) at Tq = 32; the replicated path reads the
//   64 KB per (row, head).
// LDS map (dynamic, every region a multiple of 16 B):
//   [0, 32768)          V^T image [64 d][256 keys] bf16, written once, read by every row's P.V product
//   [32768, 67584)      merge buffer: per wave fp32 [32 q][64 d (+ 4 pad)] (XA_MERGE).  xattn_fwd_kernel overlays it on the V^T image;
//                       here the image has to survive the loop
//   [67584, 68608)      per-wave (max, sum) of the 32 queries
//   [68608, 70656)      per-wave moment partials fp32 [4 waves][32 q][4]
//   70 656 B -> 2 workgroups (8 waves) per CU of 160 KB.
// Barriers per row: three (max, sum, merge); each buffer is written in a phase two barriers away from the phase that read it.
// Moments, `moments` fp32 [R, H, Tq, 4] = sum_j p_j x_j, sum_j p_j y_j, sum_j p_j x_j^2, sum_j p_j y_j^2 over the 256 keys, x = j & 31,
// y = j >> 5, p the fp32 probabilities (what ccd_dec_attn_fwd writes as `probs`).  A lane holds 2 x 16 of them for ONE query: the keys
// 64 w + 32 t + row(r, hf), so x = row(r, hf) and y = 2 w + t is constant over a tile.  Fixed order, no atomics: per tile t the 16 terms
// p x, p x^2 and p in ascending r, the tile sums times y, y^2; t = 0 then 1; + the other half-wave (one shuffle); + the waves 0, 1, 2,
// 3 in that order.  Every term is non-negative and rounded at most once before it is added, and the longest chain of additions in
// front of a term is 16 + 1 + 1 + 3 = 21: |fp32 sum - exact| <= 23 * 2^-24 * exact (+ denormals), inside the 256 * 2^-24 a plain loop
// over 256 terms would be bounded by.
//
// nrtr_word_score_kernel.  ONE WAVEFRONT PER ROW, four rows to a workgroup, lane l owning the classes l and l + 64 (C <= 128) and the
// positions l and l + 64 (T <= 128), the conventions of nrtr_beam_step_kernel - whose log-softmax this is: beam_wave_log_probs of
// beam_wave.h, the same fp64 operations in the same order, so the score of a word is the number the beam gives the same path.
//   seq int64 [R, T]: <BOS> c1 .. cn <EOS> <PAD> ..  The first end_idx behind position 0 ends the word, n = its position - 1.
//   infeasible  no end_idx behind position 0 (a word of more than T - 2 characters), or one of c1 .. cn outside [0, C) or equal to
//               pad_idx: score -inf, length -1, zeros elsewhere.  Nothing is read through such a token.
//   feasible    char_logp[t] = log_softmax(logits[r * T + t, :C])[seq[t + 1]] for t = 0 .. n (entry n: the <EOS>), 0 behind it; score =
//               their fp64 sum in position order, rounded once; length = n.  A -inf logit at a target gives -inf there and in the score.
//   char_pos    (moments given) mean_x, mean_y, std_x, std_y of the head-averaged map of position t, in token units: the moments are
//               linear in p, so their mean over the heads (ascending h, fp64) is the moment of the averaged map; var = E x^2 - (E x)^2,
//               clamped at 0.  Zeros behind the <EOS> and on an infeasible row.
#pragma once

#include "beam_wave.h"
#include "decoder_xattn.h"

namespace ccd {

constexpr int XR_VT = XA_TK * XA_D * 2;                                // the V^T image
constexpr int XR_STATS = 2 * 4 * XA_TQ * 4;                            // per-wave (max, sum)
constexpr int XR_MOM = 4 * XA_TQ * 4 * 4;                              // per-wave moment partials
constexpr int XR_SMEM = XR_VT + XA_MERGE + XR_STATS + XR_MOM;
static_assert(XR_VT % 16 == 0 && XA_MERGE % 16 == 0 && XR_STATS % 16 == 0 && XR_MOM % 16 == 0, "16-byte LDS regions");
static_assert(2 * XR_SMEM <= 160 * 1024, "two workgroups per CU");

// The chunk rule: CH rows of one sample to a workgroup.  Long lists are cut until about four workgroups per CU exist (two are
// resident: 70 KB of LDS each) - B = 1 with 1000 words and 8 heads gives CH = 8 on 256 CUs, 1000 workgroups - and a chunk is never
// shorter than it has to be for that: every chunk re-reads the sample's 64 KB of K / V.  Results do not depend on CH.
inline int xattn_rows_chunk(long rows, int heads, int cus) {
    const long target = 4L * (cus > 0 ? cus : 1);
    const long ch = (rows * heads + target - 1) / target;
    return (int)(ch < 1 ? 1 : (ch > 0x7fffffffL ? 0x7fffffffL : ch));
}

struct XattnRowsParams {
    const bf16_t *q, *k, *v;
    const int* row_ptr;
    bf16_t* out;
    float* moments;
    long ldq, ldk, ldv, ldo;
    int R, H, Tq, CH;
    float scale;
};

__global__ __launch_bounds__(256, 2) void xattn_rows_fwd_kernel(XattnRowsParams p) {
    const int b = blockIdx.x / p.H, h = blockIdx.x % p.H;
    int r_lo = p.row_ptr[b], r_hi = p.row_ptr[b + 1];                  // (clamped: whatever the table holds, no row leaves [0, R))
    r_lo = r_lo < 0 ? 0 : r_lo;
    r_hi = r_hi > p.R ? p.R : r_hi;
    const long first = (long)r_lo + (long)blockIdx.y * p.CH;
    if (first >= r_hi) return;                                         // workgroup-uniform: no rows, nothing is loaded
    char* smem = dynamic_smem();
    char* vt_img = smem;
    float* mg_all = reinterpret_cast<float*>(smem + XR_VT);
    float* st_m = reinterpret_cast<float*>(smem + XR_VT + XA_MERGE);
    float* st_l = st_m + 4 * XA_TQ;
    float* st_mom = st_l + 4 * XA_TQ;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, hf = lane >> 5, lq = lane & 31;
    const int Tq = p.Tq;
    const bf16_t* k_base = p.k + (long)b * XA_TK * p.ldk + h * XA_D;
    const bf16_t* v_base = p.v + (long)b * XA_TK * p.ldv + h * XA_D;
    bf16x8 kf[2][4], qf[4], qn[4];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
            kf[t][kk] = *reinterpret_cast<const bf16x8*>(k_base + (long)(64 * w + 32 * t + lq) * p.ldk + 16 * kk + 8 * hf);
    const bf16_t* q_lane = p.q + (long)lq * p.ldq + h * XA_D + 8 * hf;  // this lane's query of row 0
    const long q_row = (long)Tq * p.ldq;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
        qn[kk] = lq < Tq ? *reinterpret_cast<const bf16x8*>(q_lane + first * q_row + 16 * kk) : xa_zero_frag();
    att_stage_transposed(v_base, p.ldv, vt_img);                       // (complete behind the first barrier of the first row)
    const float c2 = p.scale * 1.4426950408889634f;
    const long chunk_step = (long)gridDim.y * p.CH;
    for (long c0 = first; c0 < r_hi; c0 += chunk_step) {
        const long c1 = c0 + p.CH < r_hi ? c0 + p.CH : r_hi;
        for (long row = c0; row < c1; ++row) {
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) qf[kk] = qn[kk];
            long next = row + 1 < c1 ? row + 1 : c0 + chunk_step;     // the row this workgroup takes next, if there is one
            if (next < r_hi) {
#pragma unroll
                for (int kk = 0; kk < 4; ++kk)
                    qn[kk] = lq < Tq ? *reinterpret_cast<const bf16x8*>(q_lane + next * q_row + 16 * kk) : xa_zero_frag();
            }
            f32x16 s[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
#pragma unroll
                for (int r = 0; r < 16; ++r) s[t][r] = 0.f;
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) s[t] = mfma_32x32x16_bf16(kf[t][kk], qf[kk], s[t]);
            }
            float mx = -3.0e38f;
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[t][r]);
            mx = fmaxf(mx, shfl_xor(mx, 32));
            if (hf == 0) st_m[w * XA_TQ + lq] = mx;
            __syncthreads();
            const float gm = fmaxf(fmaxf(st_m[lq], st_m[XA_TQ + lq]), fmaxf(st_m[2 * XA_TQ + lq], st_m[3 * XA_TQ + lq]));
            float sum = 0.f;
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float e = fast_exp2((s[t][r] - gm) * c2);
                    s[t][r] = e;
                    sum += e;
                }
            sum += shfl_xor(sum, 32);
            if (hf == 0) st_l[w * XA_TQ + lq] = sum;
            __syncthreads();
            const float total = st_l[lq] + st_l[XA_TQ + lq] + st_l[2 * XA_TQ + lq] + st_l[3 * XA_TQ + lq];
            const float inv = 1.0f / total;
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) s[t][r] = s[t][r] * inv;
            if (p.moments) {                                           // workgroup-uniform
                float m0 = 0.f, m1 = 0.f, m2 = 0.f, m3 = 0.f;
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    float px = 0.f, pxx = 0.f, ps = 0.f;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float x = (float)xa_acc_row(r, hf);
                        px += s[t][r] * x;
                        pxx += s[t][r] * (x * x);
                        ps += s[t][r];
                    }
                    const float y = (float)(2 * w + t);
                    m0 += px;
                    m1 += ps * y;
                    m2 += pxx;
                    m3 += ps * (y * y);
                }
                m0 += shfl_xor(m0, 32);
                m1 += shfl_xor(m1, 32);
                m2 += shfl_xor(m2, 32);
                m3 += shfl_xor(m3, 32);
                if (hf == 0) {
                    f32x4v v4;
                    v4.x = m0; v4.y = m1; v4.z = m2; v4.w = m3;
                    *reinterpret_cast<f32x4v*>(st_mom + (w * XA_TQ + lq) * 4) = v4;
                }
            }
            f32x16 o[2];
#pragma unroll
            for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {
                    bf16x8 pf;
#pragma unroll
                    for (int e = 0; e < 8; ++e) pf[e] = (short)f2bf(s[t][8 * s2 + e]);
                    const int ks = 2 * (2 * w + t) + s2;
#pragma unroll
                    for (int dt = 0; dt < 2; ++dt) {
                        const int d = 32 * dt + lq;
                        const bf16x8 vf = *reinterpret_cast<const bf16x8*>(vt_img + d * 512 + (((2 * ks + hf) ^ (d & 15)) * 16));
                        o[dt] = mfma_32x32x16_bf16(vf, pf, o[dt]);
                    }
                }
            float* mg = mg_all + w * XA_TQ * 68;                       // this wave's [32 q][68] partial output
#pragma unroll
            for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    f32x4v v4;
                    v4.x = o[dt][4 * g]; v4.y = o[dt][4 * g + 1]; v4.z = o[dt][4 * g + 2]; v4.w = o[dt][4 * g + 3];
                    *reinterpret_cast<f32x4v*>(mg + lq * 68 + 32 * dt + 8 * g + 4 * hf) = v4;
                }
            __syncthreads();
            {
                const int q = threadIdx.x >> 3, c = (threadIdx.x & 7) * 8;
                if (q < Tq) {
                    float acc[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
                    const float* base = mg_all + q * 68 + c;
#pragma unroll
                    for (int ww = 0; ww < 4; ++ww) {
                        const f32x4v a = *reinterpret_cast<const f32x4v*>(base + ww * XA_TQ * 68);
                        const f32x4v bq = *reinterpret_cast<const f32x4v*>(base + ww * XA_TQ * 68 + 4);
                        acc[0] += a.x; acc[1] += a.y; acc[2] += a.z; acc[3] += a.w;
                        acc[4] += bq.x; acc[5] += bq.y; acc[6] += bq.z; acc[7] += bq.w;
                    }
                    *reinterpret_cast<u32x4*>(p.out + (row * Tq + q) * p.ldo + h * XA_D + c) = pack8(acc);
                }
                if (p.moments && (int)threadIdx.x < 4 * Tq) {          // thread = (query, moment): the four waves in order
                    float m = 0.f;
#pragma unroll
                    for (int ww = 0; ww < 4; ++ww) m += st_mom[ww * XA_TQ * 4 + threadIdx.x];
                    p.moments[(row * p.H + h) * (long)(4 * Tq) + threadIdx.x] = m;
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------- word scores
constexpr int NWS_WAVES = 4;

// grid = ceil(R / 4), block = 256.  The launcher has checked 1 <= C <= 128, 2 <= T <= 128, end_idx in [0, C); moments: fp32
// [R, H, T, 4] or null (then char_pos is null too).
__global__ __launch_bounds__(64 * NWS_WAVES) void nrtr_word_score_kernel(const float* __restrict__ logits, long ldl, int C,
                                                                        const long long* __restrict__ seq, int R, int T, int end_idx,
                                                                        int pad_idx, const float* __restrict__ moments, int H,
                                                                        float* __restrict__ char_logp, float* __restrict__ score,
                                                                        int* __restrict__ length, float* __restrict__ char_pos) {
    __shared__ ctc_real row_s[NWS_WAVES][NRTR_MAX_C];
    __shared__ int tok_s[NWS_WAVES][NRTR_MAX_LEN];
    const int lane = lane_id(), w = threadIdx.x >> 6;
    const long r = (long)blockIdx.x * NWS_WAVES + w;
    if (r >= R) return;                                                    // wave-uniform; no workgroup barriers below
    const int c0 = lane, c1 = lane + 64;
    const bool has0 = c0 < C, has1 = c1 < C;
    const float ninf = -__builtin_inff();
    const long long* const q = seq + r * T;
    const long long t0 = c0 < T ? q[c0] : (long long)pad_idx, t1 = c1 < T ? q[c1] : (long long)pad_idx;
    // the first end_idx behind position 0, and the tokens in front of it that no class of the classifier is
    const unsigned long long e0 = ballot(c0 >= 1 && c0 < T && t0 == end_idx), e1 = ballot(c1 < T && t1 == end_idx);
    const int first = e0 ? __builtin_ctzll(e0) : (e1 ? 64 + __builtin_ctzll(e1) : -1);
    const bool bad0 = c0 >= 1 && c0 < first && (t0 < 0 || t0 >= C || t0 == pad_idx);
    const bool bad1 = c1 < first && (t1 < 0 || t1 >= C || t1 == pad_idx);
    const bool feasible = first >= 1 && ballot(bad0 || bad1) == 0ull;      // wave-uniform
    const int n = feasible ? first - 1 : -1;
    if (c0 < T) tok_s[w][c0] = feasible && c0 <= first ? (int)t0 : 0;
    if (c1 < T) tok_s[w][c1] = feasible && c1 <= first ? (int)t1 : 0;
    wave_lds_fence();
    ctc_real total = 0;
    float* const lp_out = char_logp + r * (T - 1);
    for (int t = 0; t <= n; ++t) {                                         // wave-uniform trip count
        const float* const x = logits + (r * T + t) * ldl;
        const CtcReal2 lp = beam_wave_log_probs(has0 ? x[c0] : ninf, has1 ? x[c1] : ninf, has0, has1, false, row_s[w], C);
        const int target = tok_s[w][t + 1];                                // in [0, C): checked above
        const ctc_real v = shfl(target < 64 ? lp.c0 : lp.c1, target & 63);
        total += v;
        if (lane == 0) lp_out[t] = (float)v;
    }
    if (c0 > n && c0 < T - 1) lp_out[c0] = 0.f;
    if (c1 > n && c1 < T - 1) lp_out[c1] = 0.f;
    if (lane == 0) {
        score[r] = feasible ? (float)total : ninf;
        length[r] = n;
    }
    if (char_pos) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int t = lane + 64 * i;
            if (t >= T - 1) continue;
            f32x4v o;
            o.x = 0.f; o.y = 0.f; o.z = 0.f; o.w = 0.f;
            if (t <= n) {
                double m0 = 0, m1 = 0, m2 = 0, m3 = 0;
                for (int h = 0; h < H; ++h) {
                    const float* const m = moments + ((r * H + h) * T + t) * 4;
                    m0 += (double)m[0];
                    m1 += (double)m[1];
                    m2 += (double)m[2];
                    m3 += (double)m[3];
                }
                m0 /= H; m1 /= H; m2 /= H; m3 /= H;
                const double vx = m2 - m0 * m0, vy = m3 - m1 * m1;
                o.x = (float)m0;
                o.y = (float)m1;
                o.z = (float)::sqrt(vx > 0 ? vx : 0);
                o.w = (float)::sqrt(vy > 0 ? vy : 0);
            }
            float* const dst = char_pos + (r * (T - 1) + t) * 4;
            dst[0] = o.x; dst[1] = o.y; dst[2] = o.z; dst[3] = o.w;
        }
    }
}

}  // namespace ccd
