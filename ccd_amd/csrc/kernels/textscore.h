// textscore.h - the recognition scores of Dino/metric/eval_acc.py (TextAccuracy.update) on the device:
//   text_score_kernel        decoder scores [B, T, C] + ground-truth code points -> one record per sample
//                            {edit distance of the normalised strings, equal raw characters, raw gt length, word correct}
//   text_accumulate_kernel   records -> the running totals of an evaluation (int64 counts, fp64 normalised edit distance)
// One wavefront scores one sample and never leaves its registers but for 512 bytes of LDS.
//   decode      lane t (and t + 64) takes the arg-max over the C classes of step t, first maximum; the prediction is the classes
//               in front of the first end class, padding classes skipped (AttnConvertor.tensor2idx).
//   strings     a class stands for the code points of its table row (a row of -1-padded code points per class, one table for the
//               text as idx2str writes it, one for that text normalised: `<UKN>` is five raw and three normalised characters,
//               the end / padding classes none).  An exclusive prefix sum of the row lengths over the steps gives every step its
//               place in the two strings; the raw prediction is compared against the ground truth where it lies and is never
//               written, the normalised one goes to LDS and from there onto the lanes, two characters per lane.
//   normalise   per code point (ts_normalise) = re.sub('[^A-Z^a-z^0-9^\u4e00-\u9fa5]', '', s.lower()) for every string
//               (tests/test_textscore_cpu.py checks all 1 112 064 code points): 64 ground-truth characters at a time, one per lane.
//   distance    Levenshtein, one ground-truth character (row) at a time, columns j = 2 lane + 1, 2 lane + 2 of the row in
//               registers; column 0 (= the row number) is implicit.  With t[j] = min(D[i-1][j] + 1, D[i-1][j-1] + cost) the
//               left-neighbour recurrence D[i][j] = min(t[j], D[i][j-1] + 1) unrolls to D[i][j] = j + min_{k <= j} (t[k] - k):
//               a min-prefix scan over the lanes (6 shuffle steps) instead of a serial walk along the row.  Columns behind the
//               prediction's end hold a character that matches nothing; the answer is read at column n.
// Every loop that shuffles has a wave-uniform trip count (the ground-truth walk follows a ballot mask).
#pragma once

#include "common.h"

namespace ccd {

constexpr int TS_THREADS = 256;
constexpr int TS_WAVES = TS_THREADS / 64;
constexpr int TS_COLS = 128;          // normalised prediction characters of a sample: two DP columns per lane
constexpr int TS_MAX_WIDTH = 64;      // code points of one class (the packed prefix sum below keeps raw lengths under 2^16)
constexpr int TS_RECORD = 4;          // ints per sample: distance, equal raw characters, raw gt length, word correct

// code point -> its normalised form, or -1 when the metric drops it
__device__ __forceinline__ int ts_normalise(int c) {
    if (c >= 'A' && c <= 'Z') return c + ('a' - 'A');
    if (c == 0x212A) return 'k';                                  // KELVIN SIGN lower-cases to k
    if (c == 0x0130) return 'i';                                  // I WITH DOT ABOVE lower-cases to i + U+0307, the latter dropped
    const bool keep = (c >= 'a' && c <= 'z') || (c >= '0' && c <= '9') || c == '^' || (c >= 0x4E00 && c <= 0x9FA5);
    return keep ? c : -1;
}

// inclusive prefix over the lanes of a wave
__device__ __forceinline__ int ts_scan_add(int v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = shfl(v, lane >= d ? lane - d : lane);
        v = lane >= d ? v + o : v;
    }
    return v;
}
__device__ __forceinline__ int ts_scan_min(int v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = shfl(v, lane >= d ? lane - d : lane);
        v = lane >= d && o < v ? o : v;
    }
    return v;
}
// code points in front of the first -1 of a table row
__device__ __forceinline__ int ts_row_len(const int* __restrict__ row, int width) {
    int n = 0;
    while (n < width && row[n] >= 0) ++n;
    return n;
}

// grid = ceil(B / TS_WAVES).  The launcher has checked T * norm_width <= TS_COLS (hence T <= 128: two steps per lane).
// How a sample's classes are found (everything behind the decode step is shared):
//   TS_ATTN   (ccd_text_score)        the arg-max of every decoding step, up to the first end class, padding classes skipped;
//   TS_CTC    (ccd_text_score_ctc)    the steps are frames of a CTC head - a step counts where its arg-max class is not the blank
//                                     (class 0) and differs from the step before; no end class, nothing skipped as padding;
//   TS_PATHS  (ccd_text_score_paths)  the classes are given: `scores` is an int32 row per sample (ccd_ctc_beam_search's paths),
//                                     read up to the first negative entry; a class outside [1, C) is never an index and counts nothing.
// end_idx and pad_idx are used by TS_ATTN alone.
constexpr int TS_ATTN = 0, TS_CTC = 1, TS_PATHS = 2;
template <int MODE> struct TsInput { typedef float type; };
template <> struct TsInput<TS_PATHS> { typedef int type; };
template <int MODE>
__global__ __launch_bounds__(TS_THREADS) void text_score_kernel(const typename TsInput<MODE>::type* __restrict__ scores, long sample_stride, long step_stride,
                                                                int B, int T, int C, const int* __restrict__ tbl_raw, int raw_width,
                                                                const int* __restrict__ tbl_norm, int norm_width, int end_idx, int pad_idx,
                                                                const int* __restrict__ gt, long gt_stride, int gt_cols,
                                                                const int* __restrict__ gt_len, int* __restrict__ records) {
    __shared__ int pred_lds[TS_WAVES * TS_COLS];
    const int lane = lane_id(), b = blockIdx.x * TS_WAVES + wave_id();
    if (b >= B) return;                                           // (whole waves; no workgroup barrier below)
    int* const pred = pred_lds + wave_id() * TS_COLS;
    const int halves = T > 64 ? 2 : 1;

    // ---- decode: the class of steps lane and lane + 64 (-1 behind T)
    int cls[2] = {-1, -1};
    for (int h = 0; h < halves; ++h) {
        const int t = lane + 64 * h;
        if (t < T) {
            const auto* const p = scores + (long)b * sample_stride + (long)t * step_stride;
            if constexpr (MODE == TS_PATHS) {
                cls[h] = p[0] < 0 ? -1 : p[0];
            } else {
                float best = p[0];
                int arg = 0;
                for (int c = 1; c < C; ++c) {
                    const float v = p[c];
                    if (v > best) {
                        best = v;
                        arg = c;
                    }
                }
                cls[h] = arg;
            }
        }
    }
    int end = T;
    bool counts[2] = {cls[0] != pad_idx, cls[1] != pad_idx};
    if constexpr (MODE == TS_PATHS) {
        const unsigned long long e0 = ballot(cls[0] < 0), e1 = ballot(cls[1] < 0);      // (the lanes behind T hold -1)
        end = e0 ? __builtin_ctzll(e0) : (e1 ? 64 + __builtin_ctzll(e1) : T);
        counts[0] = cls[0] > 0 && cls[0] < C;
        counts[1] = cls[1] > 0 && cls[1] < C;
    } else if constexpr (MODE == TS_CTC) {
        const int before0 = shfl(cls[0], lane ? lane - 1 : 0), last0 = shfl(cls[0], 63), before1 = shfl(cls[1], lane ? lane - 1 : 0);
        counts[0] = cls[0] > 0 && (lane == 0 || cls[0] != before0);
        counts[1] = cls[1] > 0 && cls[1] != (lane == 0 ? last0 : before1);
    } else {
        const unsigned long long e0 = ballot(cls[0] == end_idx), e1 = ballot(cls[1] == end_idx);
        end = e0 ? __builtin_ctzll(e0) : (e1 ? 64 + __builtin_ctzll(e1) : T);
    }

    // ---- where each step's characters lie in the raw and in the normalised prediction (lengths packed: raw | norm << 16)
    int len[2] = {0, 0}, at[2] = {0, 0}, total = 0;
    for (int h = 0; h < halves; ++h) {
        const int t = lane + 64 * h;
        if (t < end && counts[h])
            len[h] = ts_row_len(tbl_raw + (long)cls[h] * raw_width, raw_width) | (ts_row_len(tbl_norm + (long)cls[h] * norm_width, norm_width) << 16);
        const int incl = ts_scan_add(len[h], lane);
        at[h] = total + incl - len[h];
        total += shfl(incl, 63);
    }
    const int n_norm = (total >> 16) < TS_COLS ? (total >> 16) : TS_COLS;

    // ---- raw strings: position-wise equal code points over min(len); normalised prediction -> LDS
    const int glen = gt_len[b] < 0 ? 0 : (gt_len[b] < gt_cols ? gt_len[b] : gt_cols);
    const int* const g = gt + (long)b * gt_stride;
    int equal = 0;
    for (int h = 0; h < halves; ++h) {
        const int nr = len[h] & 0xffff, nn = len[h] >> 16, r0 = at[h] & 0xffff, n0 = at[h] >> 16;
        for (int j = 0; j < nr; ++j)
            equal += (r0 + j < glen && tbl_raw[(long)cls[h] * raw_width + j] == g[r0 + j]) ? 1 : 0;
        for (int j = 0; j < nn; ++j)
            if (n0 + j < TS_COLS) pred[n0 + j] = tbl_norm[(long)cls[h] * norm_width + j];
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) equal += shfl_xor(equal, m);
    wave_lds_fence();
    const int ja = 2 * lane + 1, jb = 2 * lane + 2;               // this lane's columns; their characters are pred[j - 1]
    const int pa = ja <= n_norm ? pred[ja - 1] : -1, pb = jb <= n_norm ? pred[jb - 1] : -1;

    // ---- edit distance against the normalised ground truth, row by row
    int da = ja, db = jb, rows = 0;                               // row 0: D[0][j] = j
    for (int base = 0; base < glen; base += 64) {
        const int i = base + lane;
        const int mine = i < glen ? ts_normalise(g[i]) : -1;
        unsigned long long kept = ballot(mine >= 0);
        while (kept) {
            const int c = shfl(mine, __builtin_ctzll(kept));
            kept &= kept - 1;
            ++rows;
            int diag = shfl(db, lane ? lane - 1 : 0);             // D[rows - 1][ja - 1]
            if (lane == 0) diag = rows - 1;
            const int ta = da + 1 < diag + (pa != c) ? da + 1 : diag + (pa != c);
            const int tb = db + 1 < da + (pb != c) ? db + 1 : da + (pb != c);
            const int ua = ta - ja, ub = tb - jb, uab = ua < ub ? ua : ub;
            int before = shfl(uab, lane ? lane - 1 : 0);          // -> min over the columns in front of ja, column 0 (t = rows) included
            if (lane == 0) before = rows;
            before = ts_scan_min(before, lane);
            da = ja + (before < ua ? before : ua);
            db = jb + (before < uab ? before : uab);
        }
    }
    const int last = n_norm > 0 ? n_norm - 1 : 0;
    const int at_n = shfl((last & 1) ? db : da, last >> 1);
    if (lane == 0) {
        const int distance = n_norm > 0 ? at_n : rows;
        int* const r = records + (long)b * TS_RECORD;
        r[0] = distance;
        r[1] = equal;
        r[2] = glen;
        r[3] = distance == 0 ? 1 : 0;                             // (distance 0 <=> the normalised strings are equal)
    }
}

// One workgroup.  Thread t adds records t, t + 256, ... in ascending order, the 256 partial sums meet in a tree in LDS, thread 0
// adds the result to the running totals with a plain read-modify-write (launches on a stream are ordered): no atomics, the same
// batches in the same order give the same bits.  totals = {correct_char, total_char, correct_word, words, total_ed},
// total_ned += sum distance / max(raw gt length, 1).
__global__ __launch_bounds__(TS_THREADS) void text_accumulate_kernel(const int* __restrict__ records, int B, long* __restrict__ totals,
                                                                     double* __restrict__ total_ned) {
    __shared__ long counts[4 * TS_THREADS];
    __shared__ double ned[TS_THREADS];
    const int t = threadIdx.x;
    long ed = 0, cc = 0, tc = 0, cw = 0;
    double nd = 0.0;
    for (int i = t; i < B; i += TS_THREADS) {
        const int* const r = records + (long)i * TS_RECORD;
        ed += r[0];
        cc += r[1];
        tc += r[2];
        cw += r[3];
        nd += (double)r[0] / (double)(r[2] > 1 ? r[2] : 1);
    }
    counts[t] = ed;
    counts[TS_THREADS + t] = cc;
    counts[2 * TS_THREADS + t] = tc;
    counts[3 * TS_THREADS + t] = cw;
    ned[t] = nd;
    __syncthreads();
    for (int s = TS_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) {
#pragma unroll
            for (int q = 0; q < 4; ++q) counts[q * TS_THREADS + t] += counts[q * TS_THREADS + t + s];
            ned[t] += ned[t + s];
        }
        __syncthreads();
    }
    if (t == 0) {
        totals[0] += counts[TS_THREADS];
        totals[1] += counts[2 * TS_THREADS];
        totals[2] += counts[3 * TS_THREADS];
        totals[3] += B;
        totals[4] += counts[0];
        total_ned[0] += ned[0];
    }
}

}  // namespace ccd
