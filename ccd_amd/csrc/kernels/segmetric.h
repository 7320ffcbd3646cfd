// segmetric.h - the segmentation metrics of Dino/metric/eval_IOU.py on the device:
//   seg_confusion_kernel<Src, TG, P>   one pass over an eval / gt label-map pair (or over seg logits, arg-max folded in)
//                                      -> the 32 x 32 joint histogram cm[image][gt][eval] (int32) and a status word per image
//   seg_scores_kernel                  cm, status -> pixel_accuracy, mean_accuracy, mean_IU, fore_IU, frequency_weighted_IU (fp64)
// Labels are integers in [0, 32) held as uint8, int32, int64 or (integral) fp32.  A workgroup counts SEG_CHUNK pixels of one
// image.  A binary mask puts all 64 lanes of a wave on at most 4 of the 1024 bins, so equal keys are combined inside the wave
// before the table is touched: the wave picks a pending key (ballot + the first lane's key), every lane matches its P pixels
// against it, and one lane adds the popcount to the wave's private 4-KB table in LDS.  After SEG_ROUNDS distinct keys the rest of
// a step (many-class noise) goes to the table with LDS atomics.  The four tables are merged at the end: plain stores when the
// image is one chunk, integer atomicAdd of the non-zero bins when it is split (integer adds commute: the counts are the same
// whatever the arrival order).
#pragma once

#include "common.h"

namespace ccd {

constexpr int SEG_CLASSES = 32;
constexpr int SEG_BINS = SEG_CLASSES * SEG_CLASSES;
constexpr int SEG_THREADS = 256;
constexpr int SEG_WAVES = SEG_THREADS / 64;
constexpr int SEG_CHUNK = 4096;                   // pixels of one image per workgroup (32 x 128: one workgroup per image)
constexpr int SEG_ROUNDS = 8;                     // distinct keys a wave combines per step before it falls back to LDS atomics
constexpr int SEG_BAD = -1, SEG_NONE = -2;        // a label outside [0, 32) / not a number / not integral; a pixel past the end

// value -> label, or SEG_BAD
__device__ __forceinline__ int seg_label(unsigned char v) { return v < SEG_CLASSES ? (int)v : SEG_BAD; }
__device__ __forceinline__ int seg_label(int v) { return (unsigned)v < (unsigned)SEG_CLASSES ? v : SEG_BAD; }
__device__ __forceinline__ int seg_label(long long v) { return (unsigned long long)v < (unsigned long long)SEG_CLASSES ? (int)v : SEG_BAD; }
__device__ __forceinline__ int seg_label(float v) {
    if (!(v >= 0.0f && v < (float)SEG_CLASSES)) return SEG_BAD;      // (a NaN fails both comparisons)
    const int i = (int)v;
    return (float)i == v ? i : SEG_BAD;
}

// P consecutive elements from p: 16-byte (or, for four uint8, 4-byte) loads when `vec` says p is aligned for them and all P
// are inside the image, element by element otherwise; elements at n and beyond are not read
template <typename T, int P>
__device__ __forceinline__ void seg_read(const T* __restrict__ p, bool vec, int n, T (&v)[P]) {
    constexpr int BYTES = P * (int)sizeof(T);
    static_assert(BYTES == 4 || BYTES % 16 == 0, "");
    if (vec && n == P) {
        if constexpr (BYTES == 4) {
            const unsigned w = *reinterpret_cast<const unsigned*>(p);
            __builtin_memcpy(v, &w, 4);
        } else {
#pragma unroll
            for (int q = 0; q < BYTES / 16; ++q) {
                const u32x4 w = reinterpret_cast<const u32x4*>(p)[q];
                __builtin_memcpy(reinterpret_cast<char*>(v) + 16 * q, &w, 16);
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < P; ++j) v[j] = j < n ? p[j] : T(0);
    }
}

// a label map: element i of the image at p
template <typename T>
struct SegMapSrc {
    const T* p;
    long stride;          // elements between images
    int vec;
    template <int P>
    __device__ __forceinline__ void labels(int image, long i, int n, int (&lab)[P]) const {
        T v[P];
        seg_read<T, P>(p + (long)image * stride + i, vec != 0, n, v);
#pragma unroll
        for (int j = 0; j < P; ++j) lab[j] = j < n ? seg_label(v[j]) : SEG_NONE;
    }
};
// fp32 logits [image][class][pixel]: the label is the first maximum over the classes (torch.argmax; for two classes
// logit1 > logit0); a NaN among a pixel's logits makes it SEG_BAD
struct SegLogitSrc {
    const float* p;
    long stride, cstride;
    int classes, vec;
    template <int P>
    __device__ __forceinline__ void labels(int image, long i, int n, int (&lab)[P]) const {
        const float* q = p + (long)image * stride + i;
        float best[P];
        bool nan[P];
        seg_read<float, P>(q, vec != 0, n, best);
#pragma unroll
        for (int j = 0; j < P; ++j) {
            lab[j] = 0;
            nan[j] = best[j] != best[j];
        }
        for (int c = 1; c < classes; ++c) {
            float v[P];
            seg_read<float, P>(q + (long)c * cstride, vec != 0, n, v);
#pragma unroll
            for (int j = 0; j < P; ++j) {
                nan[j] = nan[j] || v[j] != v[j];
                if (v[j] > best[j]) {
                    best[j] = v[j];
                    lab[j] = c;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < P; ++j) lab[j] = j < n ? (nan[j] ? SEG_BAD : lab[j]) : SEG_NONE;
    }
};

// grid = images * chunks; P pixels per lane and step.  single (chunks == 1): cm and status of the image are written with plain
// stores; otherwise the caller has cleared them and the workgroups add.
template <typename Src, typename TG, int P>
__global__ __launch_bounds__(SEG_THREADS) void seg_confusion_kernel(Src ev, SegMapSrc<TG> gt, int pixels, int chunks,
                                                                    int* __restrict__ cm, int* __restrict__ status) {
    __shared__ int tbl[SEG_WAVES * SEG_BINS];
    __shared__ int any_bad;
    const int t = threadIdx.x, lane = lane_id();
    int* const mine = tbl + wave_id() * SEG_BINS;
    const int image = blockIdx.x / chunks, chunk = blockIdx.x - image * chunks;
    for (int b = t; b < SEG_WAVES * SEG_BINS; b += SEG_THREADS) tbl[b] = 0;
    if (t == 0) any_bad = 0;
    __syncthreads();
    const long lo = (long)chunk * SEG_CHUNK, hi = lo + SEG_CHUNK < pixels ? lo + SEG_CHUNK : pixels;      // (pixels < 2^31)
    bool bad = false;
    for (long s = lo; s < hi; s += SEG_THREADS * P) {        // (the same trip count for every lane: the wave votes inside)
        const long i = s + t * P;
        const int n = hi - i < 0 ? 0 : (hi - i < P ? (int)(hi - i) : P);
        int le[P], lg[P], key[P];
        ev.template labels<P>(image, i, n, le);
        gt.template labels<P>(image, i, n, lg);
        int top = -1;
#pragma unroll
        for (int j = 0; j < P; ++j) {
            bad = bad || le[j] == SEG_BAD || lg[j] == SEG_BAD;
            key[j] = (le[j] >= 0 && lg[j] >= 0) ? lg[j] * SEG_CLASSES + le[j] : -1;
            top = key[j] > top ? key[j] : top;
        }
        for (int r = 0; r < SEG_ROUNDS; ++r) {
            const unsigned long long pending = ballot(top >= 0);
            if (!pending) break;
            const int leader = __builtin_ctzll(pending);
            const int k = shfl(top, leader);
            int count = 0;
            top = -1;
#pragma unroll
            for (int j = 0; j < P; ++j) {
                const bool hit = key[j] == k;
                count += __builtin_popcountll(ballot(hit));
                key[j] = hit ? -1 : key[j];
                top = key[j] > top ? key[j] : top;
            }
            if (lane == leader) mine[k] += count;
        }
#pragma unroll
        for (int j = 0; j < P; ++j)
            if (key[j] >= 0) atomicAdd(&mine[key[j]], 1);
    }
    if (ballot(bad) && lane == 0) atomicMax(&any_bad, 1);
    __syncthreads();
    const bool single = chunks == 1;
    int* const out = cm + (long)image * SEG_BINS;
    for (int b = t; b < SEG_BINS; b += SEG_THREADS) {
        int c = 0;
#pragma unroll
        for (int w = 0; w < SEG_WAVES; ++w) c += tbl[w * SEG_BINS + b];
        if (single) out[b] = c;
        else if (c) atomicAdd(&out[b], c);
    }
    if (t == 0) {
        if (single) status[image] = any_bad;
        else if (any_bad) atomicMax(&status[image], 1);
    }
}

// ---- cm, status -> the five scores.  One wave per image, lane c < 32 owns class c: t_c = the row sum (gt pixels of the class),
// n_c = the column sum (eval pixels), d_c = the diagonal.  G = {t_c > 0}, E = {n_c > 0}:
//   pixel_accuracy = sum_G d / sum_G t                      mean_accuracy = (sum_G d / t) / |G|
//   mean_IU = (sum_{G and E} d / (t + n - d)) / |G|         frequency_weighted_IU = (sum_{G and E} t d / (t + n - d)) / sum t
//   fore_IU = d_k / (t_k + n_k - d_k + 1e-6), k the second-smallest class of G or E; none -> NaN and status bit 1
// Every lane runs the same sums over the classes in ascending order in fp64, lane 0 writes.  status bit 0 -> five NaNs.
__global__ __launch_bounds__(SEG_THREADS) void seg_scores_kernel(const int* __restrict__ cm, int* __restrict__ status, int images,
                                                                 double* __restrict__ scores) {
    const int image = blockIdx.x * SEG_WAVES + wave_id(), lane = lane_id();
    if (image >= images) return;                             // (whole waves)
    const int* const m = cm + (long)image * SEG_BINS;
    const int c = lane & (SEG_CLASSES - 1);
    long long tc = 0, nc = 0;
    for (int j = 0; j < SEG_CLASSES; ++j) {
        tc += m[c * SEG_CLASSES + j];
        nc += m[j * SEG_CLASSES + c];
    }
    const long long dc = m[c * SEG_CLASSES + c];
    long long sum_d = 0, sum_t = 0;
    double acc = 0.0, iu = 0.0, fw = 0.0, fore = 0.0;
    int n_gt = 0, n_union = 0;
    for (int k = 0; k < SEG_CLASSES; ++k) {
        const long long tk = shfl(tc, k), nk = shfl(nc, k), dk = shfl(dc, k);
        if (tk > 0 || nk > 0) {
            if (++n_union == 2) fore = (double)dk / ((double)(tk + nk - dk) + 1e-6);
        }
        if (tk > 0) {
            ++n_gt;
            sum_d += dk;
            sum_t += tk;
            acc += (double)dk / (double)tk;
        }
        if (tk > 0 && nk > 0) {
            const double u = (double)(tk + nk - dk);
            iu += (double)dk / u;
            fw += (double)(tk * dk) / u;
        }
    }
    if (lane != 0) return;
    const double nan = __builtin_nan("");
    const int st = status[image];
    double* const out = scores + (long)image * 5;
    if ((st & 1) || n_gt == 0) {
#pragma unroll
        for (int q = 0; q < 5; ++q) out[q] = nan;
        if (!(st & 1)) status[image] = st | 2;
        return;
    }
    out[0] = (double)sum_d / (double)sum_t;
    out[1] = acc / (double)n_gt;
    out[2] = iu / (double)n_gt;
    out[3] = n_union >= 2 ? fore : nan;
    out[4] = fw / (double)sum_t;
    if (n_union < 2) status[image] = st | 2;
}

}  // namespace ccd
