// posattn.h - the parallel (position) attention recognition head of the reference (Dino/modules/attention.py:5-30): T <= 32 learned
// reading-order queries against the 256 image tokens of a sample, additive (tanh) scores over the FULL embedding width:
//   M = tanh(P + Q0)   A[s, t] = be[t] + sum_e M[s, e] We[t, e]   a[t, :] = softmax_s A[:, t]   G[t, e] = sum_s a[t, s] X[s, e]
// P = X Wv^T + bv comes from the existing GEMM, Q0 [256, E] is image-independent.  M is never written: it is formed chunk by chunk
// over E while the operand of the We product is built (forward) and re-derived from P + Q0 (backward).
//
// The nearest relative is decoder_xattn.h and the operand conventions are its: one workgroup (4 waves) per image, wave w owns tokens
// 64 w .. 64 w + 63, the transposed product leaves a lane holding the scores of ONE position, the exponentiated accumulators are
// directly the B operand of the next product, and the LDS-resident transposed images (att_stage_transposed, xa_stage_qt) carry the
// matching token / position permutation.
//   forward : per 64 columns of E a wave loads its P and Q0 rows as fragments straight from memory, applies tanh and splits M into a
//             bf16 head and a bf16 remainder (two MFMAs per fragment: the scores keep fp32 accuracy, the product is 7 % of the head's
//             work).  Softmax statistics of the four token slices are merged through LDS.  The probabilities of all 256 tokens are
//             then exchanged through LDS as B fragments and the token panel X is STREAMED 128 columns at a time through two
//             transposed images; wave w owns 32 of the 128 columns over all 256 tokens, so G needs no cross-wave sum.
//   backward: da = dG X^T is formed in both orientations from the same fragments (lane = position for the softmax row sums and dWe,
//             lane = token for dX1 and dM).  Per 64 columns: M^T is staged as a transposed image (tanh applied on the way), We^T and
//             dG^T as [64][32] images; dX1 and dP = dM (1 - M^2) leave as 16-byte row stores, the wave partials of dWe are merged
//             through LDS (overlaying the M^T image) into this workgroup's fp32 partial.  posattn_fold_kernel sums the partials of
//             dWe / dbe and dQ0 = sum_n dP_n over the images in a fixed order.
// No atomics anywhere: every sum has a fixed order, two runs give the same bits.  No index is derived from data.
// LDS: forward 2 x 32 KiB X^T images + 16 KiB probability fragments = 80 KiB exactly (the softmax statistics overlay the first image:
// two workgroups per CU), backward 34 KiB (M^T image / merge buffer) + 8 KiB (We^T, dG^T) + 1.5 KiB.  See DESIGN.md.
#pragma once

#include "decoder_xattn.h"

namespace ccd {

constexpr int PA_TOK = 256, PA_TQ = 32;
constexpr int PA_IMG = PA_TOK * 64 * 2;                                 // [64 e][256 tokens] bf16 transposed image
constexpr int PA_AFRAG = 16 * 64 * 16;                                  // probabilities as B fragments: [16 token groups][64 lanes] x 16 B
constexpr int PA_FWD_SMEM = 2 * PA_IMG + PA_AFRAG;                       // (softmax statistics overlay the first image)
constexpr int PA_BWD_SMEM = XA_MERGE + 2 * XA_QT_IMG + 3 * 4 * PA_TQ * 4;   // M^T image / merge buffer, We^T, dG^T, delta + dbe slices, delta
static_assert(XA_MERGE >= PA_IMG, "merge buffer overlays the M^T image");

struct PosAttnParams {
    const bf16_t *P, *X, *Q0, *We, *dG;
    const float* be;
    float* attn;                     // fp32 [N, T, 256]
    bf16_t *G, *dX1, *dP;
    float *dWe_part, *dbe_part;      // fp32 [N, 32, E], [N, 32]
    long ldp, ldx, ldg, lddx, lddp;
    int N, E, T;
};

// tanh through one v_exp_f32 and one v_rcp_f32: exactly +-1 once exp2 saturates (inf -> rcp 0, 0 -> 1 - 2), absolute error ~1e-7
__device__ __forceinline__ float pa_tanh(float x) {
    const float e = fast_exp2(x * 2.8853900817779268f);
    return 1.0f - 2.0f * fast_rcp(e + 1.0f);
}
// M of 8 neighbouring columns: P and Q0 words -> fp32
__device__ __forceinline__ void pa_m8(const u32x4& pw, const u32x4& qw, float* m) {
    float a[8], b[8];
    unpack8(pw, a);
    unpack8(qw, b);
#pragma unroll
    for (int e = 0; e < 8; ++e) m[e] = pa_tanh(a[e] + b[e]);
}

__global__ __launch_bounds__(256, 2) void posattn_fwd_kernel(PosAttnParams p) {
    char* smem = dynamic_smem();
    char* img0 = smem;
    char* img1 = smem + PA_IMG;
    char* afrag = smem + 2 * PA_IMG;
    float* st_m = reinterpret_cast<float*>(img0);                      // per-wave (max, sum): dead before the first image is staged
    float* st_l = st_m + 4 * PA_TQ;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, hf = lane >> 5, lq = lane & 31;
    const int n = blockIdx.x, T = p.T, E = p.E;
    const bf16_t* pb = p.P + (long)n * PA_TOK * p.ldp;
    const bf16_t* xb = p.X + (long)n * PA_TOK * p.ldx;
    // ---- scores: S^T[token][t] = sum_e M[token][e] We[t][e], a lane holds position lq
    f32x16 s[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) s[t][r] = 0.f;
    for (int c0 = 0; c0 < E; c0 += 64) {
        bf16x8 wf[4];
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) wf[kk] = *reinterpret_cast<const bf16x8*>(p.We + (long)lq * E + c0 + 16 * kk + 8 * hf);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const long row = 64 * w + 32 * t + lq;
            u32x4 pw[4], qw[4];
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                pw[kk] = *reinterpret_cast<const u32x4*>(pb + row * p.ldp + c0 + 16 * kk + 8 * hf);
                qw[kk] = *reinterpret_cast<const u32x4*>(p.Q0 + row * E + c0 + 16 * kk + 8 * hf);
            }
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                float m[8];
                pa_m8(pw[kk], qw[kk], m);
                bf16x8 hi, lo;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const bf16_t h = f2bf(m[e]);
                    hi[e] = (short)h;
                    lo[e] = (short)f2bf(m[e] - bf2f(h));
                }
                s[t] = mfma_32x32x16_bf16(hi, wf[kk], s[t]);
                s[t] = mfma_32x32x16_bf16(lo, wf[kk], s[t]);
            }
        }
    }
    const bool live = lq < T;
    const float bias = live ? p.be[lq] : 0.f;
    float mx = -3.0e38f;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            s[t][r] += bias;
            mx = fmaxf(mx, s[t][r]);
        }
    mx = fmaxf(mx, shfl_xor(mx, 32));
    if (hf == 0) st_m[w * PA_TQ + lq] = mx;
    __syncthreads();
    const float gm = fmaxf(fmaxf(st_m[lq], st_m[PA_TQ + lq]), fmaxf(st_m[2 * PA_TQ + lq], st_m[3 * PA_TQ + lq]));
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float e = fast_exp2((s[t][r] - gm) * 1.4426950408889634f);
            s[t][r] = e;
            sum += e;
        }
    sum += shfl_xor(sum, 32);
    if (hf == 0) st_l[w * PA_TQ + lq] = sum;
    __syncthreads();
    const float total = st_l[lq] + st_l[PA_TQ + lq] + st_l[2 * PA_TQ + lq] + st_l[3 * PA_TQ + lq];
    const float inv = live ? 1.0f / total : 0.f;                        // positions T..31: zero probabilities, zero rows of G
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
        for (int r = 0; r < 16; ++r) s[t][r] *= inv;
        if (live) {
            float* arow = p.attn + ((long)n * T + lq) * PA_TOK + 64 * w + 32 * t + 4 * hf;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                f32x4v v4;
                v4.x = s[t][4 * g]; v4.y = s[t][4 * g + 1]; v4.z = s[t][4 * g + 2]; v4.w = s[t][4 * g + 3];
                *reinterpret_cast<f32x4v*>(arow + 8 * g) = v4;
            }
        }
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            bf16x8 pf;
#pragma unroll
            for (int e = 0; e < 8; ++e) pf[e] = (short)f2bf(s[t][8 * s2 + e]);
            const int ks = 2 * (2 * w + t) + s2;
            *reinterpret_cast<bf16x8*>(afrag + (ks * 64 + lane) * 16) = pf;
        }
    }
    // ---- G^T[e][t] = sum_s X^T[e][s] a^T[s][t]: the token panel streamed 128 columns at a time, wave w owns 32 of them
    const int slab = w >> 1, dt = w & 1, d = 32 * dt + lq;
    for (int c0 = 0; c0 < E; c0 += 128) {
        const bool two = c0 + 64 < E;                                   // (block-uniform: E is a multiple of 64, not of 128)
        __syncthreads();                                                // every wave is done with the previous images (first trip: the statistics)
        att_stage_transposed(xb + c0, p.ldx, img0);
        if (two) att_stage_transposed(xb + c0 + 64, p.ldx, img1);
        __syncthreads();                                                // (first trip: also the probability fragments)
        if (slab == 0 || two) {
            const char* img = slab ? img1 : img0;
            f32x16 o;
#pragma unroll
            for (int r = 0; r < 16; ++r) o[r] = 0.f;
#pragma unroll
            for (int ks = 0; ks < 16; ++ks) {
                const bf16x8 xf = *reinterpret_cast<const bf16x8*>(img + d * 512 + (((2 * ks + hf) ^ (d & 15)) * 16));
                const bf16x8 pf = *reinterpret_cast<const bf16x8*>(afrag + (ks * 64 + lane) * 16);
                o = mfma_32x32x16_bf16(xf, pf, o);
            }
            bf16_t* grow = p.G + ((long)n * PA_TQ + lq) * p.ldg + c0 + 64 * slab + 32 * dt + 4 * hf;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                u32x2 v2;
                v2.x = pack_bf2(o[4 * g], o[4 * g + 1]);
                v2.y = pack_bf2(o[4 * g + 2], o[4 * g + 3]);
                *reinterpret_cast<u32x2*>(grow + 8 * g) = v2;
            }
        }
    }
}

// [64 e][256 tokens] transposed image of M = tanh(P + Q0) for 64 columns (att_stage_transposed with the tanh on the way)
__device__ __forceinline__ void pa_stage_mt(const bf16_t* __restrict__ ps, long ldp, const bf16_t* __restrict__ qs, long ldq, char* img) {
    u32x4 r[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int kq = 0; kq < 4; ++kq) {
            const u32x4 pw = *reinterpret_cast<const u32x4*>(att_transposed_src(ps, ldp, i, kq));
            const u32x4 qw = *reinterpret_cast<const u32x4*>(att_transposed_src(qs, ldq, i, kq));
            float m[8];
            pa_m8(pw, qw, m);
            r[i][kq] = pack8(m);
        }
    att_write_transposed(r, img);
}

__global__ __launch_bounds__(256, 2) void posattn_bwd_kernel(PosAttnParams p) {
    char* smem = dynamic_smem();
    char* mt_img = smem;                                               // later: the dWe merge buffer
    char* wet_img = smem + XA_MERGE;
    char* dgt_img = wet_img + XA_QT_IMG;
    float* del_s = reinterpret_cast<float*>(dgt_img + XA_QT_IMG);      // [4 waves][32]
    float* dbe_s = del_s + 4 * PA_TQ;                                  // [4 waves][32]
    float* del_t = dbe_s + 4 * PA_TQ;                                  // [32] merged
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, hf = lane >> 5, lq = lane & 31;
    const int n = blockIdx.x, T = p.T, E = p.E;
    const bf16_t* pb = p.P + (long)n * PA_TOK * p.ldp;
    const bf16_t* xb = p.X + (long)n * PA_TOK * p.ldx;
    const bf16_t* gb = p.dG + (long)n * PA_TQ * p.ldg;
    const bool live = lq < T;
    // ---- da = dG X^T in both orientations from the same fragments: d1 lane = position, d2 lane = token
    f32x16 d1[2], d2[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) { d1[t][r] = 0.f; d2[t][r] = 0.f; }
    for (int c0 = 0; c0 < E; c0 += 64) {
        bf16x8 gf[4];
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
            gf[kk] = live ? *reinterpret_cast<const bf16x8*>(gb + (long)lq * p.ldg + c0 + 16 * kk + 8 * hf) : xa_zero_frag();
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const long row = 64 * w + 32 * t + lq;
            bf16x8 xf[4];
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) xf[kk] = *reinterpret_cast<const bf16x8*>(xb + row * p.ldx + c0 + 16 * kk + 8 * hf);
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                d1[t] = mfma_32x32x16_bf16(xf[kk], gf[kk], d1[t]);
                d2[t] = mfma_32x32x16_bf16(gf[kk], xf[kk], d2[t]);
            }
        }
    }
    // ---- softmax backward, lane = position: delta[t] = sum_s a da, dA = a (da - delta); d1 becomes dA
    float part = 0.f;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const float* arow = p.attn + ((long)n * T + lq) * PA_TOK + 64 * w + 32 * t + 4 * hf;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            f32x4v v4 = {0.f, 0.f, 0.f, 0.f};
            if (live) v4 = *reinterpret_cast<const f32x4v*>(arow + 8 * g);
            const float a4[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                part += a4[j] * d1[t][4 * g + j];
                d1[t][4 * g + j] = a4[j] * d1[t][4 * g + j];           // a da for now
            }
        }
    }
    part += shfl_xor(part, 32);
    if (hf == 0) del_s[w * PA_TQ + lq] = part;
    __syncthreads();
    const float delta = del_s[lq] + del_s[PA_TQ + lq] + del_s[2 * PA_TQ + lq] + del_s[3 * PA_TQ + lq];
    if (w == 0 && hf == 0) del_t[lq] = delta;
    // dA = a da - a delta needs a again: reload (L1 / L2 hits) rather than hold 32 more registers
    float sb = 0.f;
    bf16x8 dA1f[2][2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const float* arow = p.attn + ((long)n * T + lq) * PA_TOK + 64 * w + 32 * t + 4 * hf;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            f32x4v v4 = {0.f, 0.f, 0.f, 0.f};
            if (live) v4 = *reinterpret_cast<const f32x4v*>(arow + 8 * g);
            const float a4[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float dA = d1[t][4 * g + j] - a4[j] * delta;
                d1[t][4 * g + j] = dA;
                sb += dA;
            }
        }
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
            for (int e = 0; e < 8; ++e) dA1f[t][s2][e] = (short)f2bf(d1[t][8 * s2 + e]);
    }
    sb += shfl_xor(sb, 32);
    if (hf == 0) dbe_s[w * PA_TQ + lq] = sb;
    __syncthreads();
    if (w == 0 && hf == 0)
        p.dbe_part[(long)n * PA_TQ + lq] = dbe_s[lq] + dbe_s[PA_TQ + lq] + dbe_s[2 * PA_TQ + lq] + dbe_s[3 * PA_TQ + lq];
    // ---- lane = token: a and dA as B fragments over the positions
    bf16x8 a2f[2][2], dA2f[2][2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int tt = xa_acc_row(r, hf);
            const float a = tt < T ? p.attn[((long)n * T + tt) * PA_TOK + 64 * w + 32 * t + lq] : 0.f;
            const float dA = a * (d2[t][r] - del_t[tt]);
            a2f[t][r >> 3][r & 7] = (short)f2bf(a);
            dA2f[t][r >> 3][r & 7] = (short)f2bf(dA);
        }
    // ---- per 64 columns: dX1, dP = dM (1 - M^2), this workgroup's partial of dWe
    for (int c0 = 0; c0 < E; c0 += 64) {
        if (c0) __syncthreads();                                       // the merge buffer of the previous chunk has been read
        pa_stage_mt(pb + c0, p.ldp, p.Q0 + c0, E, mt_img);
        xa_stage_qt(p.We + c0, E, PA_TQ, wet_img);
        xa_stage_qt(gb + c0, p.ldg, T, dgt_img);
        __syncthreads();
        f32x16 dwe[2];
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) dwe[dt][r] = 0.f;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            f32x16 dx[2], dm[2];
#pragma unroll
            for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                for (int r = 0; r < 16; ++r) { dx[dt][r] = 0.f; dm[dt][r] = 0.f; }
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
                for (int dt = 0; dt < 2; ++dt) {
                    dx[dt] = mfma_32x32x16_bf16(xa_qt_frag(dgt_img, 32 * dt + lq, s2, hf), a2f[t][s2], dx[dt]);
                    dm[dt] = mfma_32x32x16_bf16(xa_qt_frag(wet_img, 32 * dt + lq, s2, hf), dA2f[t][s2], dm[dt]);
                }
            const long row = 64 * w + 32 * t + lq;
#pragma unroll
            for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int col = c0 + 32 * dt + 8 * g + 4 * hf;
                    const u32x2 pw = *reinterpret_cast<const u32x2*>(pb + row * p.ldp + col);
                    const u32x2 qw = *reinterpret_cast<const u32x2*>(p.Q0 + row * E + col);
                    const float m0 = pa_tanh(bf_lo(pw.x) + bf_lo(qw.x)), m1 = pa_tanh(bf_hi(pw.x) + bf_hi(qw.x));
                    const float m2 = pa_tanh(bf_lo(pw.y) + bf_lo(qw.y)), m3 = pa_tanh(bf_hi(pw.y) + bf_hi(qw.y));
                    dm[dt][4 * g] *= 1.0f - m0 * m0;
                    dm[dt][4 * g + 1] *= 1.0f - m1 * m1;
                    dm[dt][4 * g + 2] *= 1.0f - m2 * m2;
                    dm[dt][4 * g + 3] *= 1.0f - m3 * m3;
                }
            attb_store_t(p.dP + ((long)n * PA_TOK + row) * p.lddp + c0, dm, hf);
            attb_store_t(p.dX1 + ((long)n * PA_TOK + row) * p.lddx + c0, dx, hf);
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                const int ks = 2 * (2 * w + t) + s2;
#pragma unroll
                for (int dt = 0; dt < 2; ++dt) {
                    const int d = 32 * dt + lq;
                    const bf16x8 mf = *reinterpret_cast<const bf16x8*>(mt_img + d * 512 + (((2 * ks + hf) ^ (d & 15)) * 16));
                    dwe[dt] = mfma_32x32x16_bf16(mf, dA1f[t][s2], dwe[dt]);
                }
            }
        }
        __syncthreads();                                               // every wave is done with the M^T image
        float* mg = reinterpret_cast<float*>(smem) + w * PA_TQ * 68;    // this wave's [32 t][68] partial
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                f32x4v v4;
                v4.x = dwe[dt][4 * g]; v4.y = dwe[dt][4 * g + 1]; v4.z = dwe[dt][4 * g + 2]; v4.w = dwe[dt][4 * g + 3];
                *reinterpret_cast<f32x4v*>(mg + lq * 68 + 32 * dt + 8 * g + 4 * hf) = v4;
            }
        __syncthreads();
        {
            const int q = threadIdx.x >> 3, c = (threadIdx.x & 7) * 8;
            f32x4v lo = {0.f, 0.f, 0.f, 0.f}, hi = {0.f, 0.f, 0.f, 0.f};
            const float* base = reinterpret_cast<const float*>(smem) + q * 68 + c;
#pragma unroll
            for (int ww = 0; ww < 4; ++ww) {
                const f32x4v a = *reinterpret_cast<const f32x4v*>(base + ww * PA_TQ * 68);
                const f32x4v b = *reinterpret_cast<const f32x4v*>(base + ww * PA_TQ * 68 + 4);
                lo.x += a.x; lo.y += a.y; lo.z += a.z; lo.w += a.w;
                hi.x += b.x; hi.y += b.y; hi.z += b.z; hi.w += b.w;
            }
            float* out = p.dWe_part + ((long)n * PA_TQ + q) * E + c0 + c;
            *reinterpret_cast<f32x4v*>(out) = lo;
            *reinterpret_cast<f32x4v*>(out + 4) = hi;
        }
    }
}

// The sums over the images, each in a fixed order: dQ0[s, e] = sum_n dP[n, s, e] (bf16 in, fp32 out), dWe = sum_n dWe_part[n],
// dbe = sum_n dbe_part[n].  A block takes 32 groups of 8 neighbouring columns; its 8 thread slices take every 8th image and are then
// added in slice order.  Blocks 0 .. E - 1: dQ0 (256 E / 8 groups), the next E / 8: dWe (32 E / 8 groups), the last one: dbe.
constexpr int PA_FOLD_SLICES = 8;
__global__ __launch_bounds__(256) void posattn_fold_kernel(const bf16_t* __restrict__ dP, long lddp, const float* __restrict__ dWe_part,
                                                          const float* __restrict__ dbe_part, float* __restrict__ dQ0,
                                                          float* __restrict__ dWe, float* __restrict__ dbe, int N, int E) {
    __shared__ float red[PA_FOLD_SLICES][32][8];
    const int cg = threadIdx.x & 31, sl = threadIdx.x >> 5;
    const int b = blockIdx.x;
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
    float* out = nullptr;
    bool active = true;
    if (b < E) {                                                       // dQ0: group g covers token s = 8 g / E, columns 8 g % E ..
        const long g = (long)b * 32 + cg, s = g * 8 / E, e0 = g * 8 % E;
        for (int n = sl; n < N; n += PA_FOLD_SLICES) {
            float v[8];
            unpack8(*reinterpret_cast<const u32x4*>(dP + ((long)n * PA_TOK + s) * lddp + e0), v);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] += v[e];
        }
        out = dQ0 + g * 8;
    } else if (b < E + E / 8) {
        const long g = (long)(b - E) * 32 + cg;
        for (int n = sl; n < N; n += PA_FOLD_SLICES) {
            const float* src = dWe_part + (long)n * PA_TQ * E + g * 8;
            const f32x4v a = *reinterpret_cast<const f32x4v*>(src), c = *reinterpret_cast<const f32x4v*>(src + 4);
            acc[0] += a.x; acc[1] += a.y; acc[2] += a.z; acc[3] += a.w;
            acc[4] += c.x; acc[5] += c.y; acc[6] += c.z; acc[7] += c.w;
        }
        out = dWe + g * 8;
    } else {
        active = cg < PA_TQ / 8;
        if (active) {
            for (int n = sl; n < N; n += PA_FOLD_SLICES)
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] += dbe_part[(long)n * PA_TQ + cg * 8 + e];
            out = dbe + cg * 8;
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) red[sl][cg][e] = acc[e];
    __syncthreads();
    if (active) {                                                      // thread (cg, sl) finishes column sl of its group
        float v = 0.f;
#pragma unroll
        for (int s2 = 0; s2 < PA_FOLD_SLICES; ++s2) v += red[s2][cg][sl];
        out[sl] = v;
    }
}

}  // namespace ccd
