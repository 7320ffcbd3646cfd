// sr.h - the kernels of the text super-resolution finetuning task (ccd_amd/superres.py, ccd_amd/loss/sr_loss.py):
//   sr_upsample_kernel       one workgroup per (image, channel) plane: the LR plane in LDS -> base = bicubic x2 (torch's
//                            F.interpolate(scale_factor=2, mode="bicubic", align_corners=False)) and (base - mean) / std, 16-byte stores
//   img_gather_fwd_kernel    the 3-channel twin of cls_gather_fwd_kernel: sr = base + bias + the 9-point gather of the 27 tap planes
//   img_grad_cols_kernel     the 3-channel twin of cls_grad_cols_kernel: g [pixels, 64], columns co*9+tap < 27
//   sr_loss_fwd_kernel       one workgroup per (image, channel) plane, sr and hr planes in LDS -> two fp64 partials (squared error,
//                            gradient-profile error) per plane
//   sr_loss_finish_kernel    one workgroup: the three planes of an image -> mse_n, gp_n; the images folded as a fixed-shape tree
//   sr_loss_bwd_kernel       one workgroup per plane, a gather: d sr(q) from the four pixels whose stencil contains q
// Bicubic at x2 (A = -0.75): output o reads source floor((o - 0.5) / 2) with fraction 0.75 (o even) or 0.25 (o odd); the taps of
// 0.25 are (-27, 225, 67, -9) / 256, those of 0.75 the same reversed - exact in fp32.  An interpolation is written around its
// second tap, x1 + w0 (x0 - x1) + w2 (x2 - x1) + w3 (x3 - x1), so a constant plane comes back bit for bit.
// The loss, per channel plane x with zero padding (TSRN's gradient map):
//   g(x) = sqrt((0.5 (x[y, x+1] - x[y, x-1]))^2 + (0.5 (x[y-1, x] - x[y+1, x]))^2 + 1e-6)
//   mse_n = mean (sr - hr)^2,  gp_n = mean |g(sr) - g(hr)| over the 3 H W elements of image n;  L = mean_n (mse_n + gp_weight gp_n)
// g is near sqrt(1e-6) on flat regions, where an fp32 rounding of a difference is a 1e-4 relative error of 1 / g: the stencil terms
// are fp64 (the inputs are exact in it), as every sum is - a lane's pixels in ascending order, the wave's butterfly, the four waves
// in order, the planes of an image in order, the images as a tree of fixed shape.  No atomics: two runs give the same bits.
#pragma once

#include "common.h"

namespace ccd {

constexpr int SR_THREADS = 256;
constexpr int SR_WAVES = SR_THREADS / 64;
constexpr int SR_CH = 3;
constexpr int SR_MAX_LR_PIX = 2048;               // h * w of one LR plane (TextZoom: 16 x 64)
constexpr int SR_MAX_H = 32, SR_MAX_W = 128;      // one plane of the loss: 2 x 16 KB of LDS
constexpr int SR_WS_PLANE = 2;                    // fp64 partials per plane: sum (sr - hr)^2, sum |g(sr) - g(hr)|
constexpr double SR_GP_EPS = 1e-6;
constexpr int IMG_ZROWS = 32, IMG_GCOLS = 64;     // tap planes / gradient columns of the image conv: conv.h's CLS_ZROWS / CLS_GCOLS

struct SrNorm { float mean[SR_CH], std[SR_CH]; };

// four taps around x1 at fraction 0.25 (REV = false) or 0.75 (REV = true)
template <bool REV>
__device__ __forceinline__ float sr_cubic(float x0, float x1, float x2, float x3) {
    constexpr float A = -27.0f / 256.0f, B = 67.0f / 256.0f, C = -9.0f / 256.0f;
    if (REV) return x2 + C * (x0 - x2) + B * (x1 - x2) + A * (x3 - x2);
    return x1 + A * (x0 - x1) + B * (x2 - x1) + C * (x3 - x1);
}

// grid = images * 3; lr [images][3][h][w] dense -> base, xin [images][3][2h][2w] dense; w even (an output row is whole 16-byte quads)
__global__ __launch_bounds__(SR_THREADS) void sr_upsample_kernel(const float* __restrict__ lr, int h, int w, SrNorm nrm,
                                                                 float* __restrict__ base, float* __restrict__ xin) {
    __shared__ float src[SR_MAX_LR_PIX];
    const int t = threadIdx.x, plane = blockIdx.x, c = plane % SR_CH, pix = h * w;
    const float* const in = lr + (long)plane * pix;
    for (int i = t; i < pix; i += SR_THREADS) src[i] = in[i];
    __syncthreads();
    const float mean = nrm.mean[c], sd = nrm.std[c];
    const int W = 2 * w, quads_row = W / 4, quads = 2 * h * quads_row;
    float* const ob = base + (long)plane * 4 * pix;
    float* const ox = xin + (long)plane * 4 * pix;
    for (int k = t; k < quads; k += SR_THREADS) {
        const int oy = k / quads_row, j = k - oy * quads_row;
        // output row oy: even -> source rows ky - 2 .. ky + 1 at fraction 0.75, odd -> ky - 1 .. ky + 2 at 0.25 (ky = oy / 2)
        const int ky = oy >> 1, y0 = (oy & 1) ? ky - 1 : ky - 2;
        // output columns 4j .. 4j + 3 read source columns 2j - 2 .. 2j + 3
        float hrow[4][4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            int sy = y0 + r;
            sy = sy < 0 ? 0 : (sy > h - 1 ? h - 1 : sy);
            float s[6];
#pragma unroll
            for (int q = 0; q < 6; ++q) {
                int sx = 2 * j - 2 + q;
                sx = sx < 0 ? 0 : (sx > w - 1 ? w - 1 : sx);
                s[q] = src[sy * w + sx];
            }
            hrow[r][0] = sr_cubic<true>(s[0], s[1], s[2], s[3]);
            hrow[r][1] = sr_cubic<false>(s[1], s[2], s[3], s[4]);
            hrow[r][2] = sr_cubic<true>(s[1], s[2], s[3], s[4]);
            hrow[r][3] = sr_cubic<false>(s[2], s[3], s[4], s[5]);
        }
        float o[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
            o[i] = (oy & 1) ? sr_cubic<false>(hrow[0][i], hrow[1][i], hrow[2][i], hrow[3][i])
                            : sr_cubic<true>(hrow[0][i], hrow[1][i], hrow[2][i], hrow[3][i]);
        const f32x4v vb = {o[0], o[1], o[2], o[3]};
        const f32x4v vx = {(o[0] - mean) / sd, (o[1] - mean) / sd, (o[2] - mean) / sd, (o[3] - mean) / sd};
        *reinterpret_cast<f32x4v*>(ob + 4 * (long)k) = vb;
        *reinterpret_cast<f32x4v*>(ox + 4 * (long)k) = vx;
    }
}

// ------------------------------------------------------------------------------- image conv 3x3, C -> 3 (see conv.h: C -> 2)
// sr[n,co,y,x] = base[n,co,y,x] + (bias[co] + sum_tap zT[co*9+tap, (n, y+dy, x+dx)]): zero weights and bias give sr = base bit for bit
__global__ __launch_bounds__(256) void img_gather_fwd_kernel(const float* __restrict__ zT, long ldz, const float* __restrict__ bias,
                                                             const float* __restrict__ base, float* __restrict__ sr,
                                                             int images, int H, int W) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= (long)images * H * W) return;
    const int n = (int)(p / (H * W)), yy = (int)(p / W) % H, xx = (int)(p % W);
    float a[SR_CH] = {bias[0], bias[1], bias[2]};
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
        const int dy = tap / 3 - 1, dx = tap % 3 - 1;
        const int sy = yy + dy, sx = xx + dx;
        if (sy >= 0 && sy < H && sx >= 0 && sx < W) {
            const long q = p + dy * W + dx;
#pragma unroll
            for (int co = 0; co < SR_CH; ++co) a[co] += zT[(co * 9 + tap) * ldz + q];
        }
    }
    const long plane = (long)H * W;
#pragma unroll
    for (int co = 0; co < SR_CH; ++co) {
        const long at = ((long)n * SR_CH + co) * plane + (long)yy * W + xx;
        sr[at] = base[at] + a[co];
    }
}

// g [pixels, 64] bf16: column co*9+tap (< 27) = d_sr[n, co, y-dy, x-dx] (0 outside), columns 27..63 = 0
__global__ __launch_bounds__(256) void img_grad_cols_kernel(const float* __restrict__ dl, bf16_t* __restrict__ g,
                                                            int images, int H, int W) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)images * H * W * 8) return;
    const long q = i >> 3;
    const int chunk = (int)(i & 7);
    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (chunk < 4) {
        const int n = (int)(q / (H * W)), yy = (int)(q / W) % H, xx = (int)(q % W);
        const long plane = (long)H * W;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int j = chunk * 8 + e;
            if (j < 9 * SR_CH) {
                const int co = j / 9, tap = j % 9;
                const int sy = yy - (tap / 3 - 1), sx = xx - (tap % 3 - 1);
                if (sy >= 0 && sy < H && sx >= 0 && sx < W) v[e] = dl[((long)n * SR_CH + co) * plane + (long)sy * W + sx];
            }
        }
    }
    *reinterpret_cast<u32x4*>(g + q * IMG_GCOLS + chunk * 8) = pack8(v);
}

// ------------------------------------------------------------------------------- the loss
__device__ __forceinline__ void sr_stage_plane(float* __restrict__ dst, const float* __restrict__ src, int quads, int t) {
    for (int k = t; k < quads; k += SR_THREADS)
        *reinterpret_cast<f32x4v*>(dst + 4 * k) = *reinterpret_cast<const f32x4v*>(src + 4 * (long)k);
}

// the two central differences (halved) and the gradient map of a staged plane at (y, x), zero outside the plane
struct SrGrad { double a, b, g; };
__device__ __forceinline__ SrGrad sr_grad_at(const float* __restrict__ p, int y, int x, int H, int W) {
    const double r = x + 1 < W ? (double)p[y * W + x + 1] : 0.0, l = x > 0 ? (double)p[y * W + x - 1] : 0.0;
    const double u = y > 0 ? (double)p[(y - 1) * W + x] : 0.0, d = y + 1 < H ? (double)p[(y + 1) * W + x] : 0.0;
    SrGrad o;
    o.a = 0.5 * (r - l);
    o.b = 0.5 * (u - d);
    o.g = sqrt(o.a * o.a + o.b * o.b + SR_GP_EPS);
    return o;
}

// grid = images * 3; sr, hr [images][3][H][W] dense, W % 4 == 0 -> ws[plane][2]
__global__ __launch_bounds__(SR_THREADS) void sr_loss_fwd_kernel(const float* __restrict__ sr, const float* __restrict__ hr,
                                                                 int H, int W, double* __restrict__ ws) {
    __shared__ float ps[SR_MAX_H * SR_MAX_W];
    __shared__ float ph[SR_MAX_H * SR_MAX_W];
    __shared__ double red[SR_WAVES][SR_WS_PLANE];
    const int t = threadIdx.x, plane = blockIdx.x, pix = H * W;
    sr_stage_plane(ps, sr + (long)plane * pix, pix / 4, t);
    sr_stage_plane(ph, hr + (long)plane * pix, pix / 4, t);
    __syncthreads();
    double se = 0.0, ge = 0.0;
    for (int i = t; i < pix; i += SR_THREADS) {
        const int y = i / W, x = i - y * W;
        const double d = (double)ps[i] - (double)ph[i];
        se += d * d;
        ge += fabs(sr_grad_at(ps, y, x, H, W).g - sr_grad_at(ph, y, x, H, W).g);
    }
#pragma unroll
    for (int msk = 32; msk >= 1; msk >>= 1) {
        se += shfl_xor(se, msk);
        ge += shfl_xor(ge, msk);
    }
    if (lane_id() == 0) {
        red[wave_id()][0] = se;
        red[wave_id()][1] = ge;
    }
    __syncthreads();
    if (t < SR_WS_PLANE) {
        double s = red[0][t];
#pragma unroll
        for (int w = 1; w < SR_WAVES; ++w) s += red[w][t];
        ws[(long)plane * SR_WS_PLANE + t] = s;
    }
}

// one workgroup: thread t takes images t, t + SR_FIN, ... in ascending order (mse_n, gp_n out), then the SR_FIN running sums fold as a
// binary tree whose shape does not depend on the batch.  images == 0: L = 0.
constexpr int SR_FIN = 256;
__global__ __launch_bounds__(SR_FIN) void sr_loss_finish_kernel(const double* __restrict__ ws, int images, int H, int W, float gp_weight,
                                                                double* __restrict__ per_image, float* __restrict__ loss,
                                                                double* __restrict__ parts) {
    __shared__ double tree[2][SR_FIN];
    const int t = threadIdx.x;
    const double inv = 1.0 / (double)(SR_CH * H * W);
    double m = 0.0, g = 0.0;
    for (int n = t; n < images; n += SR_FIN) {
        const double* const r = ws + (long)n * SR_CH * SR_WS_PLANE;
        const double mn = ((r[0] + r[2]) + r[4]) * inv, gn = ((r[1] + r[3]) + r[5]) * inv;
        per_image[2 * (long)n] = mn;
        per_image[2 * (long)n + 1] = gn;
        m += mn;
        g += gn;
    }
    tree[0][t] = m;
    tree[1][t] = g;
    __syncthreads();
    for (int s = SR_FIN / 2; s >= 1; s >>= 1) {
        if (t < s) {
            tree[0][t] += tree[0][t + s];
            tree[1][t] += tree[1][t + s];
        }
        __syncthreads();
    }
    if (t != 0) return;
    const double mse = images > 0 ? tree[0][0] / (double)images : 0.0, gp = images > 0 ? tree[1][0] / (double)images : 0.0;
    const double total = mse + (double)gp_weight * gp;
    loss[0] = (float)total;
    parts[0] = total;
    parts[1] = mse;
    parts[2] = gp;
}

// grid = images * 3.  With s(p) = sign(g_sr(p) - g_hr(p)) (sign(0) = 0) and a, b the halved differences of sr at p:
//   d sr(q) = k [ 2 (sr - hr)(q) + gp_weight 0.5 ( s a / g at q - ex  -  s a / g at q + ex  +  s b / g at q + ey  -  s b / g at q - ey ) ]
// over the neighbours inside the plane, k = grad_scale (d_grad ? d_grad[0] : 1) / (images 3 H W).  0.5 a = 0.25 (difference).
__global__ __launch_bounds__(SR_THREADS) void sr_loss_bwd_kernel(const float* __restrict__ sr, const float* __restrict__ hr, int images,
                                                                 int H, int W, float gp_weight, float grad_scale,
                                                                 const float* __restrict__ d_grad, float* __restrict__ d_sr) {
    __shared__ float ps[SR_MAX_H * SR_MAX_W];
    __shared__ float ph[SR_MAX_H * SR_MAX_W];
    const int t = threadIdx.x, plane = blockIdx.x, pix = H * W;
    sr_stage_plane(ps, sr + (long)plane * pix, pix / 4, t);
    sr_stage_plane(ph, hr + (long)plane * pix, pix / 4, t);
    __syncthreads();
    const double k = (double)grad_scale * (d_grad ? (double)d_grad[0] : 1.0) / ((double)images * SR_CH * pix);
    const double gw = 0.5 * (double)gp_weight;
    float* const out = d_sr + (long)plane * pix;
    for (int i = t; i < pix; i += SR_THREADS) {
        const int y = i / W, x = i - y * W;
        double acc = 0.0;
        if (gp_weight != 0.f) {
            const int ny[4] = {y, y, y + 1, y - 1}, nx[4] = {x - 1, x + 1, x, x};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (ny[j] < 0 || ny[j] >= H || nx[j] < 0 || nx[j] >= W) continue;
                const SrGrad s = sr_grad_at(ps, ny[j], nx[j], H, W);
                const double diff = s.g - sr_grad_at(ph, ny[j], nx[j], H, W).g;
                const double sgn = diff > 0.0 ? 1.0 : (diff < 0.0 ? -1.0 : 0.0);
                const double term = (j < 2 ? s.a : s.b) / s.g;
                acc += ((j & 1) ? -sgn : sgn) * term;
            }
        }
        out[i] = (float)(k * (2.0 * ((double)ps[i] - (double)ph[i]) + gw * acc));
    }
}

}  // namespace ccd
