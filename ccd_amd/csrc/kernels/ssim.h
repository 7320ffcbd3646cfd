// ssim.h - the super-resolution metrics of Dino/metric/eval_superpixel.py on the device:
//   ssim_fwd_kernel<NIMG, R>     SSIM (NIMG = 2) / TRI_SSIM (NIMG = 3) map of one 16x32 output tile, summed   -> one fp64 partial
//   ssim_reduce_kernel           partials -> per-image means and the batch mean (one workgroup, fixed order)
//   ssim_bwd_kernel<NIMG, R>     input gradients of one output tile (moments recomputed, adjoint blur, combination)
//   psnr_partial_kernel          sum of (255a - 255b)^2 over a slice of one of the planes 0..2 of an image      -> one fp64 partial
//   psnr_final_kernel            partials -> mse and 20 log10(255 / sqrt(mse))
// Inputs are fp32 [N][C][H][W] planes with contiguous rows; N and C strides are free (the [:, :3] view of an RGB + mask tensor is
// read in place).  The window is the separable Gaussian of odd size 2R + 1 <= 15 (taps from the host, symmetric); pixels outside
// the plane are zero (F.conv2d's padding = R), so every moment is sum_j g_j sum_i g_i f(x) in two passes through LDS.
// No float atomics: every sum has one fixed order, so results are bitwise repeatable and an image's values do not depend on the
// other images of the batch.
#pragma once

#include "common.h"

namespace ccd {

constexpr int SS_MAX_R = 7;                       // window_size 1..15
constexpr int SS_TW = 32;                         // output tile width (both kernels)
constexpr int SS_FWD_TH = 16;                     // forward tile height: 16 x 32 outputs, one 2-row strip per thread
constexpr int SS_PAD = 8;                         // an LDS row starts 8 columns left of what its pass needs (>= R, keeps 16-B loads aligned)
constexpr int SS_THREADS = 256;
constexpr int PSNR_CHUNK = 4096;                  // pixels of one plane per psnr_partial_kernel workgroup
constexpr float SS_C1 = (float)(0.01 * 0.01), SS_C2 = (float)(0.03 * 0.03);

struct SsimTaps {
    float g[2 * SS_MAX_R + 1];
};
// up to three inputs; element strides of N and C, rows contiguous with stride W
struct SsimPlanes {
    const float* x[3];
    long sn[3], sc[3];
};

template <int NIMG>
struct SsimShape {
    static constexpr int NM = NIMG + NIMG * (NIMG + 1) / 2;   // mu_i, E[x_i^2], E[x_i x_j] (pairs (0,1) for SSIM; (0,1) (1,2) (2,0))
    static constexpr float K = NIMG == 2 ? 2.0f : 1.0f;       // SSIM: 2 mu1 mu2 and 2 sigma12; TRI_SSIM: no factor 2
};

// f(x) of the moments at one pixel, in the order mu_i, e_ii, e_ij
template <int NIMG>
__device__ __forceinline__ void ss_products(const float (&x)[NIMG], float (&f)[SsimShape<NIMG>::NM]) {
#pragma unroll
    for (int i = 0; i < NIMG; ++i) {
        f[i] = x[i];
        f[NIMG + i] = x[i] * x[i];
    }
    f[2 * NIMG] = x[0] * x[1];
    if constexpr (NIMG == 3) {
        f[7] = x[1] * x[2];
        f[8] = x[2] * x[0];
    }
}

// the map from the blurred moments, in the reference's order of operations
template <int NIMG>
__device__ __forceinline__ float ss_map(const float (&m)[SsimShape<NIMG>::NM]) {
    if constexpr (NIMG == 2) {
        const float mu1_sq = m[0] * m[0], mu2_sq = m[1] * m[1], mu12 = m[0] * m[1];
        const float s1 = m[2] - mu1_sq, s2 = m[3] - mu2_sq, s12 = m[4] - mu12;
        return ((2.0f * mu12 + SS_C1) * (2.0f * s12 + SS_C2)) / ((mu1_sq + mu2_sq + SS_C1) * (s1 + s2 + SS_C2));
    } else {
        const float mu1_sq = m[0] * m[0], mu2_sq = m[1] * m[1], mu3_sq = m[2] * m[2];
        const float mu12 = m[0] * m[1], mu23 = m[1] * m[2], mu31 = m[2] * m[0];
        const float s1 = m[3] - mu1_sq, s2 = m[4] - mu2_sq, s3 = m[5] - mu3_sq;
        const float s12 = m[6] - mu12, s23 = m[7] - mu23, s31 = m[8] - mu31;
        return ((mu12 + mu23 + mu31 + SS_C1) * (s12 + s23 + s31 + SS_C2)) /
               ((mu1_sq + mu2_sq + mu3_sq + SS_C1) * (s1 + s2 + s3 + SS_C2));
    }
}

// g * d map / d moment.  With S = A B / (Cc D):  P_eii = g dS/dD,  P_eij = K g dS/dB,
// P_mu_i = g (K (sum_{j != i} mu_j) (dS/dA - dS/dB) + 2 mu_i (dS/dCc - dS/dD))
template <int NIMG>
__device__ __forceinline__ void ss_partials(const float (&m)[SsimShape<NIMG>::NM], float g, float (&p)[SsimShape<NIMG>::NM]) {
    constexpr float K = SsimShape<NIMG>::K;
    float A, B, Cc, D;
    if constexpr (NIMG == 2) {
        const float mu1_sq = m[0] * m[0], mu2_sq = m[1] * m[1], mu12 = m[0] * m[1];
        A = 2.0f * mu12 + SS_C1;
        B = 2.0f * (m[4] - mu12) + SS_C2;
        Cc = mu1_sq + mu2_sq + SS_C1;
        D = (m[2] - mu1_sq) + (m[3] - mu2_sq) + SS_C2;
    } else {
        const float mu12 = m[0] * m[1], mu23 = m[1] * m[2], mu31 = m[2] * m[0];
        const float mu1_sq = m[0] * m[0], mu2_sq = m[1] * m[1], mu3_sq = m[2] * m[2];
        A = mu12 + mu23 + mu31 + SS_C1;
        B = (m[6] - mu12) + (m[7] - mu23) + (m[8] - mu31) + SS_C2;
        Cc = mu1_sq + mu2_sq + mu3_sq + SS_C1;
        D = (m[3] - mu1_sq) + (m[4] - mu2_sq) + (m[5] - mu3_sq) + SS_C2;
    }
    const float inv = 1.0f / (Cc * D);
    const float S = A * B * inv;
    const float dA = g * B * inv, dB = g * A * inv, dC = -g * S / Cc, dD = -g * S / D;
    float musum = 0.0f;
#pragma unroll
    for (int i = 0; i < NIMG; ++i) musum += m[i];
#pragma unroll
    for (int i = 0; i < NIMG; ++i) {
        p[i] = K * (musum - m[i]) * (dA - dB) + 2.0f * m[i] * (dC - dD);
        p[NIMG + i] = dD;
    }
#pragma unroll
    for (int k = 2 * NIMG; k < SsimShape<NIMG>::NM; ++k) p[k] = K * dB;
}

// fp64 sum of one value per thread over the workgroup in a fixed tree order; valid in red[0] after the call
__device__ __forceinline__ void ss_block_sum(double v, double* red) {
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
#pragma unroll
    for (int s = SS_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
}

// rows [y_lo, y_lo + rows) x columns [x_lo, x_lo + cols) of one plane into dst[rows][cols] (cols % 4 == 0, x_lo % 4 == 0), zero
// outside the plane.  vec: the plane's rows are 16-byte aligned and W % 4 == 0, so an aligned 4-pixel chunk is wholly in or out.
__device__ __forceinline__ void ss_load_rows(const float* __restrict__ plane, int H, int W, int y_lo, int x_lo, int rows, int cols,
                                             bool vec, float* dst) {
    const int chunks = cols / 4;
    for (int i = threadIdx.x; i < rows * chunks; i += SS_THREADS) {
        const int r = i / chunks, q = i - r * chunks;
        const int y = y_lo + r, x = x_lo + 4 * q;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (y >= 0 && y < H) {
            const float* row = plane + (long)y * W;
            if (vec) {
                if (x >= 0 && x + 4 <= W) v = *reinterpret_cast<const f32x4*>(row + x);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (x + e >= 0 && x + e < W) v[e] = row[x + e];
            }
        }
        *reinterpret_cast<f32x4*>(dst + r * cols + 4 * q) = v;
    }
}

// horizontal pass over 4 consecutive outputs: acc[m][o] = sum_j g_j f_m(in[.][o + j]), where f are the moment products of NSRC
// images (PRODUCTS) or NOUT planes taken as they are.  in[s] points at the source column of output 0 minus R.
template <int NSRC, int NOUT, int R, bool PRODUCTS>
__device__ __forceinline__ void ss_hpass4(const float* const (&in)[NSRC], const SsimTaps& tp, float (&acc)[NOUT][4]) {
#pragma unroll
    for (int m = 0; m < NOUT; ++m)
#pragma unroll
        for (int o = 0; o < 4; ++o) acc[m][o] = 0.0f;
#pragma unroll
    for (int k = 0; k < 4 + 2 * R; ++k) {
        float f[NOUT];
        if constexpr (PRODUCTS) {
            float x[NSRC];
#pragma unroll
            for (int i = 0; i < NSRC; ++i) x[i] = in[i][k];
            ss_products<NSRC>(x, f);
        } else {
#pragma unroll
            for (int i = 0; i < NOUT; ++i) f[i] = in[i][k];
        }
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            const int j = k - o;
            if (j >= 0 && j <= 2 * R) {
#pragma unroll
                for (int m = 0; m < NOUT; ++m) acc[m][o] = fmaf(tp.g[j], f[m], acc[m][o]);
            }
        }
    }
}

// vertical pass over SV consecutive outputs of one column: acc[m][o] = sum_j g_j src[m * plane_stride + (o + j) * stride]
template <int NM, int R, int SV>
__device__ __forceinline__ void ss_vpass(const float* src, int plane_stride, int stride, const SsimTaps& tp, float (&acc)[NM][SV]) {
#pragma unroll
    for (int m = 0; m < NM; ++m)
#pragma unroll
        for (int o = 0; o < SV; ++o) acc[m][o] = 0.0f;
#pragma unroll
    for (int k = 0; k < SV + 2 * R; ++k) {
#pragma unroll
        for (int m = 0; m < NM; ++m) {
            const float v = src[m * plane_stride + k * stride];
#pragma unroll
            for (int o = 0; o < SV; ++o) {
                const int j = k - o;
                if (j >= 0 && j <= 2 * R) acc[m][o] = fmaf(tp.g[j], v, acc[m][o]);
            }
        }
    }
}

template <int NM>
__device__ __forceinline__ void ss_zero4(float (&acc)[NM][4]) {
#pragma unroll
    for (int m = 0; m < NM; ++m)
#pragma unroll
        for (int o = 0; o < 4; ++o) acc[m][o] = 0.0f;
}
template <int NM>
__device__ __forceinline__ void ss_store4(float* dst, int plane_stride, const float (&acc)[NM][4]) {
#pragma unroll
    for (int m = 0; m < NM; ++m) {
        const f32x4 v = {acc[m][0], acc[m][1], acc[m][2], acc[m][3]};
        *reinterpret_cast<f32x4*>(dst + m * plane_stride) = v;
    }
}

// ---- forward: one workgroup = one 16 x 32 output tile of one (image, channel) plane.
//   xs[NIMG][16 + 2R][48]  inputs, rows y0-R .. y0+16+R, columns x0-8 .. x0+40
//   hs[NM][16 + 2R][32]    horizontal moments of those rows at the 32 output columns (rows outside the plane: zero, not computed)
// then each thread blurs one column over 2 output rows and evaluates the map; the tile's fp64 sum goes to partials[blockIdx.x].
template <int NIMG, int R>
__global__ __launch_bounds__(SS_THREADS) void ssim_fwd_kernel(SsimPlanes p, int C, int H, int W, int tiles_x, int tiles, SsimTaps tp,
                                                              int vec, double* __restrict__ partials) {
    constexpr int NM = SsimShape<NIMG>::NM, TH = SS_FWD_TH, TW = SS_TW;
    constexpr int XR = TH + 2 * R, XW = TW + 2 * SS_PAD;
    static_assert(TH / 2 * TW == SS_THREADS, "one 2-row column strip per thread");
    __shared__ __attribute__((aligned(16))) float xs[NIMG * XR * XW];
    __shared__ __attribute__((aligned(16))) float hs[NM * XR * TW];
    __shared__ double red[SS_THREADS];
    const int t = threadIdx.x;
    const int plane = blockIdx.x / tiles, tile = blockIdx.x - plane * tiles;
    const int n = plane / C, c = plane - n * C;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int y0 = ty * TH, x0 = tx * TW;
#pragma unroll
    for (int i = 0; i < NIMG; ++i)
        ss_load_rows(p.x[i] + n * p.sn[i] + c * p.sc[i], H, W, y0 - R, x0 - SS_PAD, XR, XW, vec != 0, xs + i * XR * XW);
    __syncthreads();
    for (int i = t; i < XR * (TW / 4); i += SS_THREADS) {
        const int r = i / (TW / 4), q = i - r * (TW / 4);
        const int y = y0 - R + r;
        float acc[NM][4];
        if (y >= 0 && y < H) {
            const float* in[NIMG];
#pragma unroll
            for (int k = 0; k < NIMG; ++k) in[k] = xs + k * XR * XW + r * XW + SS_PAD - R + 4 * q;
            ss_hpass4<NIMG, NM, R, true>(in, tp, acc);
        } else {
            ss_zero4<NM>(acc);
        }
        ss_store4<NM>(hs + r * TW + 4 * q, XR * TW, acc);
    }
    __syncthreads();
    const int col = t % TW, r0 = 2 * (t / TW);
    float mom[NM][2];
    ss_vpass<NM, R, 2>(hs + r0 * TW + col, XR * TW, TW, tp, mom);
    double local = 0.0;
#pragma unroll
    for (int o = 0; o < 2; ++o) {
        const int y = y0 + r0 + o, x = x0 + col;
        if (y < H && x < W) {
            float m[NM];
#pragma unroll
            for (int k = 0; k < NM; ++k) m[k] = mom[k][o];
            local += (double)ss_map<NIMG>(m);
        }
    }
    ss_block_sum(local, red);
    if (t == 0) partials[blockIdx.x] = red[0];
}

// ---- per-image means (sum / count) and, if mean != nullptr, the batch mean; one workgroup, thread t owns images t, t + 256, ...
__global__ __launch_bounds__(SS_THREADS) void ssim_reduce_kernel(const double* __restrict__ partials, int images, int per_image,
                                                                 double count, float* __restrict__ per_img, float* __restrict__ mean) {
    __shared__ double red[SS_THREADS];
    double tot = 0.0;
    for (int n = threadIdx.x; n < images; n += SS_THREADS) {
        const double* pn = partials + (long)n * per_image;
        double s = 0.0;
        for (int k = 0; k < per_image; ++k) s += pn[k];
        per_img[n] = (float)(s / count);
        tot += s;
    }
    ss_block_sum(tot, red);
    if (threadIdx.x == 0 && mean) *mean = (float)(red[0] / (count * (double)images));
}

// ---- backward: one workgroup = one TH x 32 output tile (TH = 16 for SSIM, 8 for TRI_SSIM and its 9 moments).
//   1. inputs over the tile + 2R: rows y0-2R .. y0+TH+2R, columns x0-16 .. x0+48            -> A: xs[NIMG][TH+4R][64]
//   2. horizontal moments of those rows at columns x0-8 .. x0+40                             -> B: hs[NM][TH+4R][48]
//   3. vertical moments at rows y0-R .. y0+TH+R, then g dS/d(moment), zero outside the plane -> A: pp[NM][TH+2R][48]
//   4. horizontal blur of pp at the 32 output columns                                         -> B: hp[NM][TH+2R][32]
//   5. vertical blur (the window is symmetric: the adjoint of the zero-padded correlation is the same correlation), then
//      dx_i = W*P_mu_i + 2 x_i (W*P_eii) + sum_{j != i} x_j (W*P_eij), x re-read from memory
template <int NIMG, int R>
struct SsimBwdGeom {
    static constexpr int NM = SsimShape<NIMG>::NM;
    static constexpr int TH = NIMG == 2 ? 16 : 8, TW = SS_TW;
    static constexpr int SV = TH * TW / SS_THREADS;                  // output rows per thread in step 5
    static constexpr int XR = TH + 4 * R, XW = TW + 4 * SS_PAD;      // 1.
    static constexpr int HC = TW + 2 * SS_PAD;                       // 2. / 3. columns
    static constexpr int PR = TH + 2 * R;                            // 3. / 4. rows
    static constexpr int A_XS = NIMG * XR * XW, A_PP = NM * PR * HC;
    static constexpr int B_HS = NM * XR * HC, B_HP = NM * PR * TW;
    static constexpr int A = A_XS > A_PP ? A_XS : A_PP, B = B_HS > B_HP ? B_HS : B_HP;
};

template <int NIMG, int R>
__global__ __launch_bounds__(SS_THREADS) void ssim_bwd_kernel(SsimPlanes p, int C, int H, int W, int tiles_x, int tiles, SsimTaps tp,
                                                              int vec, const float* __restrict__ gscale, float* __restrict__ dx0,
                                                              float* __restrict__ dx1, float* __restrict__ dx2) {
    using G = SsimBwdGeom<NIMG, R>;
    constexpr int NM = G::NM, TH = G::TH, TW = G::TW, SV = G::SV, XR = G::XR, XW = G::XW, HC = G::HC, PR = G::PR;
    static_assert(SV * SS_THREADS == TH * TW && PR % 2 == 0, "step 5: SV rows of one column per thread");
    __shared__ __attribute__((aligned(16))) float lds[G::A + G::B];
    float* const bufA = lds;
    float* const bufB = lds + G::A;
    const int t = threadIdx.x;
    const int plane = blockIdx.x / tiles, tile = blockIdx.x - plane * tiles;
    const int n = plane / C, c = plane - n * C;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int y0 = ty * TH, x0 = tx * TW;
    const float g = gscale[n];
    // 1.
#pragma unroll
    for (int i = 0; i < NIMG; ++i)
        ss_load_rows(p.x[i] + n * p.sn[i] + c * p.sc[i], H, W, y0 - 2 * R, x0 - 2 * SS_PAD, XR, XW, vec != 0, bufA + i * XR * XW);
    __syncthreads();
    // 2. hs column j <-> x0 - 8 + j; its inputs from x0 - 8 + j - R are xs columns j + 8 - R ..
    for (int i = t; i < XR * (HC / 4); i += SS_THREADS) {
        const int r = i / (HC / 4), q = i - r * (HC / 4);
        const int y = y0 - 2 * R + r;
        float acc[NM][4];
        if (y >= 0 && y < H) {
            const float* in[NIMG];
#pragma unroll
            for (int k = 0; k < NIMG; ++k) in[k] = bufA + k * XR * XW + r * XW + SS_PAD - R + 4 * q;
            ss_hpass4<NIMG, NM, R, true>(in, tp, acc);
        } else {
            ss_zero4<NM>(acc);
        }
        ss_store4<NM>(bufB + r * HC + 4 * q, XR * HC, acc);
    }
    __syncthreads();
    // 3. pp row pr <-> y0 - R + pr (hs rows pr .. pr + 2R), column j <-> x0 - 8 + j; two rows per item
    for (int i = t; i < (PR / 2) * HC; i += SS_THREADS) {
        const int j = i % HC, pr = 2 * (i / HC);
        float mom[NM][2];
        ss_vpass<NM, R, 2>(bufB + pr * HC + j, XR * HC, HC, tp, mom);
        const int x = x0 - SS_PAD + j;
#pragma unroll
        for (int o = 0; o < 2; ++o) {
            const int y = y0 - R + pr + o;
            float m[NM], pv[NM];
#pragma unroll
            for (int k = 0; k < NM; ++k) m[k] = mom[k][o];
            ss_partials<NIMG>(m, g, pv);
            const bool inside = y >= 0 && y < H && x >= 0 && x < W;
#pragma unroll
            for (int k = 0; k < NM; ++k) bufA[k * PR * HC + (pr + o) * HC + j] = inside ? pv[k] : 0.0f;
        }
    }
    __syncthreads();
    // 4. hp column cc <-> x0 + cc; its pp columns are cc + 8 - R ..
    for (int i = t; i < PR * (TW / 4); i += SS_THREADS) {
        const int r = i / (TW / 4), q = i - r * (TW / 4);
        const float* in[NM];
#pragma unroll
        for (int k = 0; k < NM; ++k) in[k] = bufA + k * PR * HC + r * HC + SS_PAD - R + 4 * q;
        float acc[NM][4];
        ss_hpass4<NM, NM, R, false>(in, tp, acc);
        ss_store4<NM>(bufB + r * TW + 4 * q, PR * TW, acc);
    }
    __syncthreads();
    // 5. SV output rows of one column per thread; hp rows r .. r + 2R for output row r
    const int col = t % TW, r0 = SV * (t / TW);
    float wp[NM][SV];
    ss_vpass<NM, R, SV>(bufB + r0 * TW + col, PR * TW, TW, tp, wp);
    const int x = x0 + col;
#pragma unroll
    for (int o = 0; o < SV; ++o) {
        const int y = y0 + r0 + o;
        if (y >= H || x >= W) continue;
        float xv[NIMG];
#pragma unroll
        for (int i = 0; i < NIMG; ++i) xv[i] = p.x[i][n * p.sn[i] + c * p.sc[i] + (long)y * W + x];
        const long off = ((long)plane * H + y) * W + x;
#pragma unroll
        for (int i = 0; i < NIMG; ++i) {
            float* d = i == 0 ? dx0 : (i == 1 ? dx1 : dx2);
            if (!d) continue;
            float v = wp[i][o] + 2.0f * xv[i] * wp[NIMG + i][o];
            // pair k = (k, k + 1 mod NIMG) is moment 2 NIMG + k (SSIM: the single pair (0, 1))
#pragma unroll
            for (int k = 0; k < NM - 2 * NIMG; ++k) {
                const int a = k, b = (k + 1) % NIMG;
                if (i == a) v += xv[b] * wp[2 * NIMG + k][o];
                else if (i == b) v += xv[a] * wp[2 * NIMG + k][o];
            }
            d[off] = v;
        }
    }
}

// ---- PSNR: sum of (255 a - 255 b)^2 over the first `channels` (<= 3) channels; the two products and their difference are rounded to fp32 as in the
// reference, the square and the sum are fp64.  Workgroup = PSNR_CHUNK pixels of one (image, channel) plane, partial index
// plane * chunks + chunk.  vec: H*W % 4 == 0 and 16-byte aligned planes.
__global__ __launch_bounds__(SS_THREADS) void psnr_partial_kernel(const float* __restrict__ a, long an, long ac,
                                                                  const float* __restrict__ b, long bn, long bc, int channels, int HW,
                                                                  int chunks, int vec, double* __restrict__ partials) {
    __shared__ double red[SS_THREADS];
    const int plane = blockIdx.x / chunks, chunk = blockIdx.x - plane * chunks;
    const int n = plane / channels, c = plane - channels * n;
    const float* pa = a + n * an + c * ac;
    const float* pb = b + n * bn + c * bc;
    const int lo = chunk * PSNR_CHUNK, hi = lo + PSNR_CHUNK < HW ? lo + PSNR_CHUNK : HW;
    double s = 0.0;
    if (vec) {
        for (int i = lo + 4 * threadIdx.x; i < hi; i += 4 * SS_THREADS) {
            const f32x4 va = *reinterpret_cast<const f32x4*>(pa + i), vb = *reinterpret_cast<const f32x4*>(pb + i);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float d = va[e] * 255.0f - vb[e] * 255.0f;
                s += (double)d * (double)d;
            }
        }
    } else {
        for (int i = lo + threadIdx.x; i < hi; i += SS_THREADS) {
            const float d = pa[i] * 255.0f - pb[i] * 255.0f;
            s += (double)d * (double)d;
        }
    }
    ss_block_sum(s, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = red[0];
}

__global__ __launch_bounds__(SS_THREADS) void psnr_final_kernel(const double* __restrict__ partials, int count_partials, double count,
                                                                double* __restrict__ mse, float* __restrict__ psnr) {
    __shared__ double red[SS_THREADS];
    double s = 0.0;
    for (int i = threadIdx.x; i < count_partials; i += SS_THREADS) s += partials[i];
    ss_block_sum(s, red);
    if (threadIdx.x == 0) {
        const double m = red[0] / count;
        *mse = m;
        *psnr = (float)(20.0 * log10(255.0 / sqrt(m)));
    }
}

}  // namespace ccd
