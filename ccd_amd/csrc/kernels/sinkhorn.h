// sinkhorn.h - DINOLoss.sinkhorn_knopp_teacher on the device (Dino/loss/Dino_loss.py:157-184), in the log domain.
// The reference scales Q = exp(t / temp)^T alternately by prototype (our columns k) and by sample (our rows r); what it returns is
//   Q^T[r, k] = softmax_k(t[r, k] / temp + log beta_k)
// with beta the accumulated prototype scaling (its constants K, B and sum_Q cancel in the softmax).  With x = t / temp:
//   sinkhorn_colpass_kernel   log beta_k  = -log sum_r exp(x[r, k] + log alpha_r)     (first pass: alpha uniform)
//   sinkhorn_rowpass_kernel   log alpha_r = -log sum_k exp(x[r, k] + log beta_k)
//   sinkhorn_finish_kernel    log beta gauged to mean 0 (the softmax does not see the constant) and c_k = -temp * log beta_k: the
//                             vector the loss kernels take in place of the centre, softmax((t - c) / temp)
//   sinkhorn_assign_kernel    the assignment itself, for the callers that want the [rows, K] matrix
// Every sum is an fp32 sum of exp(v - max): no finite x overflows.  The column pass is split over strips of SK_STRIP columns and
// chunks of SK_ROW_CHUNK rows; a chunk's (max, sum) per column goes to a workspace by plain stores and sinkhorn_colmerge_kernel folds
// the chunks in ascending order - no atomics, two runs give the same bits.  Between merge and finish the host may all-reduce the
// column state across ranks (MAX of the shifts, sinkhorn_rescale_kernel, SUM of the sums: Dino_loss.py:174-175).
// HBM-bound: a pass reads rows * K * 4 B once; n iterations are 2n - 1 passes (the last row scaling is the loss's own softmax).
// Row count (rows_mul * d_rows[0]) is read from device memory; rows past it are never read.
#pragma once

namespace ccd {

constexpr int SK_THREADS = 256;
constexpr int SK_STRIP = 1024;          // columns per workgroup of the column pass: 4 per thread
constexpr int SK_ROW_CHUNK = 128;       // rows per workgroup of the column pass
constexpr int SK_FIN_THREADS = 1024;
constexpr float SK_EMPTY = -3.0e38f;    // the running maximum of an empty sum
#define SK_NEG_INF (-__builtin_inff())

// 1 / temp in two fp32 terms.  t / temp + a in two fused steps: the sum is rounded where it is small (the entries that carry weight sit
// within ~25 of 0 once the potential is added), not at the size of t / temp
struct SkScale { float hi, lo; };
__device__ __forceinline__ float sk_x(float t, SkScale sc, float a) { return fmaf(t, sc.hi, fmaf(t, sc.lo, a)); }

__device__ __forceinline__ int sk_live_rows(const int* __restrict__ d_rows, int rows_mul, int max_rows) {
    const long rows = (long)d_rows[0] * rows_mul;
    return rows < 0 ? 0 : rows < max_rows ? (int)rows : max_rows;
}

// running (max, sum of exp(v - max)); padding enters as -inf and adds exactly 0
struct SkLse {
    float m, s;
    __device__ __forceinline__ void init() { m = SK_EMPTY; s = 0.f; }
    __device__ __forceinline__ void add4(float v0, float v1, float v2, float v3) {
        const float vm = fmaxf(fmaxf(v0, v1), fmaxf(v2, v3));
        if (vm > m) { s *= expf(m - vm); m = vm; }
        s += (expf(v0 - m) + expf(v1 - m)) + (expf(v2 - m) + expf(v3 - m));
    }
    __device__ __forceinline__ void merge(float om, float os) {
        const float nm = fmaxf(m, om);
        s = s * expf(m - nm) + os * expf(om - nm);
        m = nm;
    }
};

// part_m / part_s [chunks, K]: chunk blockIdx.y's (max, sum) of exp(x[r, k] + log_alpha[r]) over its rows.  VEC: K % 4 == 0 and
// 16-byte aligned pointers, a thread owns four adjacent columns; otherwise columns tid, tid + 256, ... of the strip, loaded one by one
template <bool VEC>
__global__ __launch_bounds__(256) void sinkhorn_colpass_kernel(const float* __restrict__ t, int K, const int* __restrict__ d_rows,
                                                               int rows_mul, int max_rows, SkScale sc,
                                                               const float* __restrict__ log_alpha, float* __restrict__ part_m,
                                                               float* __restrict__ part_s) {
    const int rows = sk_live_rows(d_rows, rows_mul, max_rows);
    const int r0 = blockIdx.y * SK_ROW_CHUNK;
    if (r0 >= rows) return;
    const int r1 = r0 + SK_ROW_CHUNK < rows ? r0 + SK_ROW_CHUNK : rows;
    const int k0 = blockIdx.x * SK_STRIP;
    int kc[4];
    bool ok[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        kc[e] = VEC ? k0 + 4 * (int)threadIdx.x + e : k0 + (int)threadIdx.x + SK_THREADS * e;
        ok[e] = kc[e] < K;
    }
    if (!ok[0]) return;
    SkLse acc[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e].init();
    for (int r = r0; r < r1; r += 4) {                       // four rows in flight
        float v[4][4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const bool live = r + u < r1;
            const float* row = t + (long)(live ? r + u : r) * K;
            if (VEC) {
                const f32x4v q = *reinterpret_cast<const f32x4v*>(row + kc[0]);
                v[u][0] = q.x; v[u][1] = q.y; v[u][2] = q.z; v[u][3] = q.w;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[u][e] = ok[e] ? row[kc[e]] : 0.f;
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const bool live = r + u < r1;
            const float a = log_alpha && live ? log_alpha[r + u] : 0.f;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[u][e] = live && ok[e] ? sk_x(v[u][e], sc, a) : SK_NEG_INF;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e].add4(v[0][e], v[1][e], v[2][e], v[3][e]);
    }
    float* pm = part_m + (long)blockIdx.y * K;
    float* ps = part_s + (long)blockIdx.y * K;
    if (VEC) {
        const f32x4v m4 = {acc[0].m, acc[1].m, acc[2].m, acc[3].m}, s4 = {acc[0].s, acc[1].s, acc[2].s, acc[3].s};
        *reinterpret_cast<f32x4v*>(pm + kc[0]) = m4;
        *reinterpret_cast<f32x4v*>(ps + kc[0]) = s4;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (ok[e]) { pm[kc[e]] = acc[e].m; ps[kc[e]] = acc[e].s; }
    }
}

// col_m / col_s [K]: the live chunks of a column folded in ascending order
__global__ __launch_bounds__(256) void sinkhorn_colmerge_kernel(const float* __restrict__ part_m, const float* __restrict__ part_s, int K,
                                                                const int* __restrict__ d_rows, int rows_mul, int max_rows,
                                                                float* __restrict__ col_m, float* __restrict__ col_s) {
    const int k = blockIdx.x * SK_THREADS + threadIdx.x;
    if (k >= K) return;
    const int chunks = (sk_live_rows(d_rows, rows_mul, max_rows) + SK_ROW_CHUNK - 1) / SK_ROW_CHUNK;
    SkLse a;
    a.init();
    for (int c = 0; c < chunks; ++c) a.merge(part_m[(long)c * K + k], part_s[(long)c * K + k]);
    col_m[k] = a.m;
    col_s[k] = a.s;
}

// a rank's sums re-based on the shift every rank agreed on (shift >= col_m): linear in the rows, so the ranks' sums add up
__global__ __launch_bounds__(256) void sinkhorn_rescale_kernel(float* __restrict__ col_m, float* __restrict__ col_s,
                                                               const float* __restrict__ shift, int K) {
    const int k = blockIdx.x * SK_THREADS + threadIdx.x;
    if (k >= K) return;
    col_s[k] *= expf(col_m[k] - shift[k]);
    col_m[k] = shift[k];
}

__device__ __forceinline__ double sk_log_beta(float m, float s) { return s > 0.f ? -((double)m + log((double)s)) : 0.0; }

// ONE workgroup: log_beta[k] = -(m_k + log s_k) - mean, c[k] = -temp * log_beta[k] (either output may be null).  The mean is an fp64
// tree sum in a fixed order; the outputs are rounded once, from fp64, at the small magnitude the gauge leaves them with
__global__ __launch_bounds__(1024) void sinkhorn_finish_kernel(const float* __restrict__ col_m, const float* __restrict__ col_s, int K,
                                                               float temp, float* __restrict__ log_beta, float* __restrict__ c) {
    __shared__ double red[SK_FIN_THREADS];
    double acc = 0.0;
    for (int k = threadIdx.x; k < K; k += SK_FIN_THREADS) acc += sk_log_beta(col_m[k], col_s[k]);
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int st = SK_FIN_THREADS / 2; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
        __syncthreads();
    }
    const double mean = red[0] / (double)K;
    for (int k = threadIdx.x; k < K; k += SK_FIN_THREADS) {
        const double g = sk_log_beta(col_m[k], col_s[k]) - mean;
        if (log_beta) log_beta[k] = (float)g;
        if (c) c[k] = (float)(-(double)temp * g);
    }
}

// (max, sum) of exp(x[k] + log_beta[k]) over one row, in every thread of the workgroup.  red: 8 floats of LDS
template <bool VEC>
__device__ __forceinline__ SkLse sk_row_lse(const float* __restrict__ row, const float* __restrict__ log_beta, int K, SkScale sc,
                                            float* red) {
    SkLse a;
    a.init();
    if (VEC) {
        int k = threadIdx.x * 4;
        for (; k + SK_STRIP < K; k += 2 * SK_STRIP) {        // two trips' loads in front of the first exp
            f32x4v q[2], b[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                q[u] = *reinterpret_cast<const f32x4v*>(row + k + SK_STRIP * u);
                b[u] = *reinterpret_cast<const f32x4v*>(log_beta + k + SK_STRIP * u);
            }
#pragma unroll
            for (int u = 0; u < 2; ++u)
                a.add4(sk_x(q[u].x, sc, b[u].x), sk_x(q[u].y, sc, b[u].y), sk_x(q[u].z, sc, b[u].z), sk_x(q[u].w, sc, b[u].w));
        }
        for (; k < K; k += SK_STRIP) {
            const f32x4v q = *reinterpret_cast<const f32x4v*>(row + k), b = *reinterpret_cast<const f32x4v*>(log_beta + k);
            a.add4(sk_x(q.x, sc, b.x), sk_x(q.y, sc, b.y), sk_x(q.z, sc, b.z), sk_x(q.w, sc, b.w));
        }
    } else {
        for (int kb = threadIdx.x; kb < K; kb += SK_STRIP) {
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int k = kb + SK_THREADS * e;
                v[e] = k < K ? sk_x(row[k], sc, log_beta[k]) : SK_NEG_INF;
            }
            a.add4(v[0], v[1], v[2], v[3]);
        }
    }
#pragma unroll
    for (int msk = 32; msk >= 1; msk >>= 1) {
        const float om = shfl_xor(a.m, msk), os = shfl_xor(a.s, msk);
        a.merge(om, os);
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[2 * w] = a.m; red[2 * w + 1] = a.s; }
    __syncthreads();
    SkLse o;
    o.m = red[0]; o.s = red[1];
    for (int q = 1; q < SK_THREADS / 64; ++q) o.merge(red[2 * q], red[2 * q + 1]);
    return o;
}

// log_alpha[r] = -log sum_k exp(x[r, k] + log_beta[k]); one workgroup per row
template <bool VEC>
__global__ __launch_bounds__(256) void sinkhorn_rowpass_kernel(const float* __restrict__ t, int K, const int* __restrict__ d_rows,
                                                               int rows_mul, int max_rows, SkScale sc,
                                                               const float* __restrict__ log_beta, float* __restrict__ log_alpha) {
    __shared__ float red[2 * SK_THREADS / 64];
    const int r = blockIdx.x;
    if (r >= sk_live_rows(d_rows, rows_mul, max_rows)) return;
    const SkLse a = sk_row_lse<VEC>(t + (long)r * K, log_beta, K, sc, red);
    if (threadIdx.x == 0) log_alpha[r] = (float)-((double)a.m + log((double)a.s));
}

// q[r, k] = softmax_k(x[r, k] + log_beta[k]) of the live rows (the others are left as they are); one workgroup per row
template <bool VEC>
__global__ __launch_bounds__(256) void sinkhorn_assign_kernel(const float* __restrict__ t, int K, const int* __restrict__ d_rows,
                                                              int rows_mul, int max_rows, SkScale sc,
                                                              const float* __restrict__ log_beta, float* __restrict__ q) {
    __shared__ float red[2 * SK_THREADS / 64];
    const int r = blockIdx.x;
    if (r >= sk_live_rows(d_rows, rows_mul, max_rows)) return;
    const float* row = t + (long)r * K;
    float* out = q + (long)r * K;
    const SkLse a = sk_row_lse<VEC>(row, log_beta, K, sc, red);
    // the exponent in fp64: at |x| ~ 25 one fp32 rounding of it is 1e-6 of the probability, as much as the whole iteration costs
    // (this kernel is not on the training step's path, which never writes the probabilities)
    const double inv_t = (double)sc.hi + (double)sc.lo, m = (double)a.m, inv_s = 1.0 / (double)a.s;
    if (VEC) {
        for (int k = threadIdx.x * 4; k < K; k += SK_STRIP) {
            const f32x4v v = *reinterpret_cast<const f32x4v*>(row + k), b = *reinterpret_cast<const f32x4v*>(log_beta + k);
            const f32x4v o = {(float)(exp((double)v.x * inv_t + (double)b.x - m) * inv_s), (float)(exp((double)v.y * inv_t + (double)b.y - m) * inv_s),
                              (float)(exp((double)v.z * inv_t + (double)b.z - m) * inv_s), (float)(exp((double)v.w * inv_t + (double)b.w - m) * inv_s)};
            *reinterpret_cast<f32x4v*>(out + k) = o;
        }
    } else {
        for (int k = threadIdx.x; k < K; k += SK_THREADS) out[k] = (float)(exp((double)row[k] * inv_t + (double)log_beta[k] - m) * inv_s);
    }
}

}  // namespace ccd
