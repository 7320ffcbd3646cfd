// seg_sup_loss.h - the supervised text-segmentation loss of the finetuning task (ccd_amd/loss/seg_loss.py: SegSupLoss):
//   seg_sup_loss_fwd_kernel      one workgroup per image: class- and edge-weighted cross entropy sums, the Dice sums, the 2 x 2
//                                confusion counts -> one row of fp64 partials; optionally a one-byte code per pixel for the backward
//   seg_sup_loss_finish_kernel   one workgroup: the rows (through LDS) in image order -> loss, parts [L, CE, Dice, Omega], confusion, the tail of ws
//   seg_sup_loss_bwd_kernel      elementwise: d_logits from the logits, the codes and the finished sums
// Logits are fp32 [N][2][H][W] planes (free image and channel strides, rows of a plane contiguous), gt is uint8 [N][H*W]: 0 =
// background, 1 = text, anything else is not scored.  With y = gt, d = z1 - z0, p = sigmoid(d):
//   l = -log softmax(z)[y] = softplus(y ? -d : d);    w = class_weight[y] * (1 + edge_weight * edge)
//   CE = sum w l / Omega, Omega = sum w (the batch);   Dice_n = 1 - (2 I + 1) / (P + G + 1), I = sum p y, P = sum p, G = sum y (image n)
// edge(q): q is scored and a scored pixel of the OTHER class lies within the (2r + 1)^2 square around it, inside the image.  The gt
// plane is staged in LDS as one presence mask per pixel (1 = background, 2 = text, 0 = not scored), four pixels to a word, and the
// square is two separable ORs over words: along the row (neighbour words shifted by whole bytes), then down the column - 2 (2r + 1)
// word reads per four pixels instead of (2r + 1)^2 byte reads per pixel.
// Per-pixel terms are fp32 (e = exp(-|d|) gives p, 1 - p and softplus(+-d) without cancellation), every sum is fp64 in one fixed
// order - a lane's quads in ascending order, the wave's butterfly, the four waves in order, the images in index order - and there
// are no atomics: two runs give the same bits.
#pragma once

#include "common.h"

namespace ccd {

constexpr int SSL_THREADS = 256;
constexpr int SSL_WAVES = SSL_THREADS / 64;
constexpr int SSL_MAX_PIX = 8192;                 // H * W of one image: its presence masks and their row-wise OR are 2 x 8 KB of LDS
constexpr int SSL_MAX_R = 4;                      // edge_radius: a neighbour word covers four pixels to either side
// one row of partials per image: sum w, sum w l, I, P, G, scored pixels, cm[0][0], cm[0][1], cm[1][0], cm[1][1], pixels whose value is
// neither 0, 1 nor ignore_index (counts are exact in fp64)
constexpr int SSL_FIELDS = 11;
constexpr int SSL_F_W = 0, SSL_F_WL = 1, SSL_F_I = 2, SSL_F_P = 3, SSL_F_G = 4, SSL_F_VALID = 5, SSL_F_CM = 6, SSL_F_BAD = 10;
constexpr int SSL_TAIL = 3;                       // behind the rows: Omega, N_v (images with a scored pixel), the batch's bad pixels
constexpr unsigned SSL_BG = 1, SSL_TEXT = 2, SSL_EDGE = 4;        // the code of a pixel: its presence mask, + 4 on the edge band

// p = sigmoid(d), 1 - p and softplus(|d|) - |d| from one exponential
struct SslTerms { float p, q, sp; };
__device__ __forceinline__ SslTerms ssl_terms(float d) {
    const float e = expf(-fabsf(d)), inv = 1.0f / (1.0f + e);
    SslTerms r;
    r.p = d >= 0.f ? inv : e * inv;
    r.q = d >= 0.f ? e * inv : inv;
    r.sp = log1pf(e);
    return r;
}

__global__ __launch_bounds__(SSL_THREADS) void seg_sup_loss_fwd_kernel(const float* __restrict__ z, long zn, long zc,
                                                                       const unsigned char* __restrict__ gt, long gt_stride, int gvec,
                                                                       int H, int W, int ignore, float cw0, float cw1, float edge_weight,
                                                                       int radius, double* __restrict__ ws,
                                                                       unsigned char* __restrict__ code) {
    __shared__ unsigned lab[SSL_MAX_PIX / 4];     // presence masks, four pixels of a row per word (W % 4 == 0)
    __shared__ unsigned hm[SSL_MAX_PIX / 4];      // their OR over [x - r, x + r] of the row
    __shared__ double red[SSL_WAVES][SSL_FIELDS];
    const int t = threadIdx.x, image = blockIdx.x, wq = W / 4, quads = H * wq;
    const unsigned char* const g = gt + (long)image * gt_stride;
    int bad = 0;
    for (int k = t; k < quads; k += SSL_THREADS) {
        unsigned v;
        if (gvec) v = *reinterpret_cast<const unsigned*>(g + 4 * k);
        else v = (unsigned)g[4 * k] | ((unsigned)g[4 * k + 1] << 8) | ((unsigned)g[4 * k + 2] << 16) | ((unsigned)g[4 * k + 3] << 24);
        unsigned m = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned b = (v >> (8 * j)) & 255u;
            m |= (b == 0u ? SSL_BG : (b == 1u ? SSL_TEXT : 0u)) << (8 * j);
            bad += (b > 1u && b != (unsigned)ignore) ? 1 : 0;
        }
        lab[k] = m;
    }
    __syncthreads();
    if (radius > 0) {
        for (int k = t; k < quads; k += SSL_THREADS) {
            const int col = k % wq;
            const unsigned cur = lab[k], prev = col > 0 ? lab[k - 1] : 0u, next = col + 1 < wq ? lab[k + 1] : 0u;
            const unsigned long long lo = (unsigned long long)prev | ((unsigned long long)cur << 32);      // pixels x0 - 4 .. x0 + 3
            const unsigned long long hi = (unsigned long long)cur | ((unsigned long long)next << 32);      // pixels x0 .. x0 + 7
            unsigned h = cur;
            for (int s = 1; s <= radius; ++s) h |= (unsigned)(lo >> (32 - 8 * s)) | (unsigned)(hi >> (8 * s));
            hm[k] = h;
        }
        __syncthreads();
    }
    double f[SSL_FIELDS];
#pragma unroll
    for (int i = 0; i < SSL_FIELDS; ++i) f[i] = 0.0;
    f[SSL_F_BAD] = (double)bad;
    const float* const z0 = z + (long)image * zn;
    for (int k = t; k < quads; k += SSL_THREADS) {
        const unsigned m = lab[k];
        unsigned around = 0;
        if (radius > 0) {
            const int row = k / wq;
            for (int dy = -radius; dy <= radius; ++dy)
                if (row + dy >= 0 && row + dy < H) around |= hm[k + dy * wq];
        }
        const f32x4v a = *reinterpret_cast<const f32x4v*>(z0 + 4 * k), b = *reinterpret_cast<const f32x4v*>(z0 + zc + 4 * k);
        const float za[4] = {a.x, a.y, a.z, a.w}, zb[4] = {b.x, b.y, b.z, b.w};
        unsigned out = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned mj = (m >> (8 * j)) & 3u;
            if (mj == 0u) continue;
            const bool y = mj == SSL_TEXT, edge = (((around >> (8 * j)) & 3u) & (mj ^ 3u)) != 0u;
            const float d = zb[j] - za[j];
            const SslTerms s = ssl_terms(d);
            const float l = fmaxf(y ? -d : d, 0.f) + s.sp;
            const float w = (y ? cw1 : cw0) * (edge ? 1.0f + edge_weight : 1.0f);
            f[SSL_F_W] += (double)w;
            f[SSL_F_WL] += (double)w * (double)l;
            f[SSL_F_I] += y ? (double)s.p : 0.0;
            f[SSL_F_P] += (double)s.p;
            f[SSL_F_G] += y ? 1.0 : 0.0;
            f[SSL_F_VALID] += 1.0;
            const int bin = (y ? 2 : 0) + (zb[j] > za[j] ? 1 : 0);              // [gt][pred], a tie predicts class 0
#pragma unroll
            for (int c = 0; c < 4; ++c) f[SSL_F_CM + c] += bin == c ? 1.0 : 0.0;
            out |= (mj | (edge ? SSL_EDGE : 0u)) << (8 * j);
        }
        if (code) *reinterpret_cast<unsigned*>(code + ((long)image * quads + k) * 4) = out;
    }
#pragma unroll
    for (int i = 0; i < SSL_FIELDS; ++i) {
#pragma unroll
        for (int msk = 32; msk >= 1; msk >>= 1) f[i] += shfl_xor(f[i], msk);
    }
    if (lane_id() == 0) {
#pragma unroll
        for (int i = 0; i < SSL_FIELDS; ++i) red[wave_id()][i] = f[i];
    }
    __syncthreads();
    if (t < SSL_FIELDS) {
        double s = red[0][t];
#pragma unroll
        for (int w = 1; w < SSL_WAVES; ++w) s += red[w][t];
        ws[(long)image * SSL_FIELDS + t] = s;
    }
}

// one workgroup: the rows come into LDS SSL_FIN_CHUNK images at a time (coalesced; a thread that walked the rows in memory paid one
// load latency per image, 105 us for 224 images), every thread turns one image's sums into its Dice term, then thread f <
// SSL_FIELDS adds field f and thread SSL_FIELDS the Dice terms - each in image order, so the order of every sum is fixed
constexpr int SSL_FIN_CHUNK = 256;
__global__ __launch_bounds__(SSL_FIN_CHUNK) void seg_sup_loss_finish_kernel(double* __restrict__ ws, int images, float dice_weight,
                                                                            float* __restrict__ loss, double* __restrict__ parts,
                                                                            long* __restrict__ confusion) {
    __shared__ double rows[SSL_FIN_CHUNK * SSL_FIELDS];
    __shared__ double dice_n[SSL_FIN_CHUNK];          // 1 - (2 I + 1) / (P + G + 1) of an image with a scored pixel, -1 of one without
    __shared__ double tot[SSL_FIELDS + 2];
    const int t = threadIdx.x;
    double acc = 0.0, nv = 0.0;
    for (int base = 0; base < images; base += SSL_FIN_CHUNK) {
        const int cnt = images - base < SSL_FIN_CHUNK ? images - base : SSL_FIN_CHUNK;
        for (int i = t; i < cnt * SSL_FIELDS; i += SSL_FIN_CHUNK) rows[i] = ws[(long)base * SSL_FIELDS + i];
        __syncthreads();
        if (t < cnt) {
            const double* const r = rows + t * SSL_FIELDS;
            dice_n[t] = r[SSL_F_VALID] > 0.0 ? 1.0 - (2.0 * r[SSL_F_I] + 1.0) / (r[SSL_F_P] + r[SSL_F_G] + 1.0) : -1.0;
        }
        __syncthreads();
        if (t < SSL_FIELDS) {
            for (int n = 0; n < cnt; ++n) acc += rows[n * SSL_FIELDS + t];
        } else if (t == SSL_FIELDS) {
            for (int n = 0; n < cnt; ++n) {
                const double d = dice_n[n];
                if (d >= 0.0) {                       // (a Dice term lies in [0, 1): -1 marks an image without a scored pixel)
                    acc += d;
                    nv += 1.0;
                }
            }
        }
        __syncthreads();
    }
    if (t <= SSL_FIELDS) tot[t] = acc;
    if (t == SSL_FIELDS) tot[SSL_FIELDS + 1] = nv;
    __syncthreads();
    if (t != 0) return;
    const double omega = tot[SSL_F_W], nimg = tot[SSL_FIELDS + 1];
    const double ce = omega > 0.0 ? tot[SSL_F_WL] / omega : 0.0;           // (no scored pixel: 0, not 0 / 0)
    const double dice = nimg > 0.0 ? tot[SSL_FIELDS] / nimg : 0.0;
    const double total = ce + (double)dice_weight * dice;
    loss[0] = (float)total;
    parts[0] = total;
    parts[1] = ce;
    parts[2] = dice;
    parts[3] = omega;
#pragma unroll
    for (int c = 0; c < 4; ++c) confusion[c] = (long)tot[SSL_F_CM + c];
    double* const tail = ws + (long)images * SSL_FIELDS;
    tail[0] = omega;
    tail[1] = nimg;
    tail[2] = tot[SSL_F_BAD];
}

// grid = images * blocks_per_image, one quad of four pixels per thread
//   dz1 = s [ w (p - y) / Omega - (dice_weight / N_v) (2 y S - (2 I + 1)) / S^2 p (1 - p) ],  S = P + G + 1;  dz0 = -dz1
// s = grad_scale * (d_grad ? d_grad[0] : 1); d_logits is dense [images][2][H * W]
__global__ __launch_bounds__(SSL_THREADS) void seg_sup_loss_bwd_kernel(const float* __restrict__ z, long zn, long zc,
                                                                       const unsigned char* __restrict__ code, int quads,
                                                                       int blocks_per_image, int images, float cw0, float cw1,
                                                                       float dice_weight, float edge_weight,
                                                                       const double* __restrict__ ws, float grad_scale,
                                                                       const float* __restrict__ d_grad, float* __restrict__ d_logits) {
    const int image = blockIdx.x / blocks_per_image, k = (blockIdx.x - image * blocks_per_image) * SSL_THREADS + threadIdx.x;
    if (k >= quads) return;
    const double* const row = ws + (long)image * SSL_FIELDS;
    const double* const tail = ws + (long)images * SSL_FIELDS;
    const double s = (double)grad_scale * (d_grad ? (double)d_grad[0] : 1.0);
    const double omega = tail[0], nv = tail[1];
    const double S = row[SSL_F_P] + row[SSL_F_G] + 1.0, top = 2.0 * row[SSL_F_I] + 1.0;
    const double ce_k = omega > 0.0 ? s / omega : 0.0;
    const double dk = nv > 0.0 ? s * (double)dice_weight / (nv * S * S) : 0.0;
    const double dice_k[2] = {dk * -top, dk * (2.0 * S - top)};           // by y
    const unsigned c = *reinterpret_cast<const unsigned*>(code + ((long)image * quads + k) * 4);
    const float* const z0 = z + (long)image * zn;
    const f32x4v a = *reinterpret_cast<const f32x4v*>(z0 + 4 * k), b = *reinterpret_cast<const f32x4v*>(z0 + zc + 4 * k);
    const float za[4] = {a.x, a.y, a.z, a.w}, zb[4] = {b.x, b.y, b.z, b.w};
    float g[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const unsigned cj = (c >> (8 * j)) & 7u, mj = cj & 3u;
        g[j] = 0.f;
        if (mj == 0u) continue;
        const bool y = mj == SSL_TEXT;
        const SslTerms r = ssl_terms(zb[j] - za[j]);
        const float w = (y ? cw1 : cw0) * ((cj & SSL_EDGE) ? 1.0f + edge_weight : 1.0f);
        const double pmy = y ? -(double)r.q : (double)r.p;
        g[j] = (float)(ce_k * (double)w * pmy - dice_k[y ? 1 : 0] * ((double)r.p * (double)r.q));
    }
    float* const out = d_logits + ((long)image * 2 * quads + k) * 4;
    const f32x4v g1 = {g[0], g[1], g[2], g[3]}, g0 = {-g[0], -g[1], -g[2], -g[3]};
    *reinterpret_cast<f32x4v*>(out) = g0;
    *reinterpret_cast<f32x4v*>(out + (long)quads * 4) = g1;
}

}  // namespace ccd
