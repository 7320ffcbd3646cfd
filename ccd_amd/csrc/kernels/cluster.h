// cluster.h - the three public clusterers of Dino/utils/DBSCAN.py on the device, one 32x128 mask per workgroup held in LDS:
//   dbscan_label_kernel          DBSCAN_cluster.forward   Dino/utils/DBSCAN.py:14-59    -> id map (clusters are disjoint)
//   region_boxes_kernel          region_cluster.forward   Dino/utils/DBSCAN.py:110-141  -> up to 26 boxes (planes may overlap)
//   idmap_to_planes_u8_kernel    id map -> the reference's uint8 [26, 32, 128] planes (DBSCAN_cluster, label_cluster)
//   boxes_to_planes_u8_kernel    boxes  -> the reference's uint8 [26, 32, 128] planes (region_cluster)
// label_cluster itself is ccl_label_kernel (charmap.h).  All decisions are integer (the one fp32 compare is the DBSCAN
// foreground threshold), so the outputs are bit-exact against the reference wherever its own order is defined.
#pragma once

#include "charmap.h"

namespace ccd {

constexpr int CL_MAX_CAND = CM_PIX / CM_MIN_AREA + 1;   // disjoint clusters of >= 30 pixels in 4096: at most 136
constexpr int CL_MIN_BOX_AREA = 100;                    // region_cluster's area test (DBSCAN.py:132)
constexpr int CL_NONE = 0x7fffffff;

// ---- sklearn DBSCAN(eps=1.5, min_samples=4) on the (row, col) list of the pixels with mask > 0.1, restated on the grid:
//   foreground  x > 0.1f (fp32 compare);  core = foreground with >= 3 foreground 8-neighbours (min_samples counts the point,
//   sqrt(2) <= eps < 2);  clusters = 8-connected components of the core pixels, numbered by their first core pixel in raster
//   order (sklearn's discovery order);  border = non-core foreground pixel with a core 8-neighbour: it joins the lowest-numbered
//   of those clusters (sklearn expands one cluster completely before the next);  every other foreground pixel is noise.
// Post-processing (DBSCAN.py:31-49): clusters of < 30 pixels (border pixels included) are dropped, ALL the others are ordered by
// mean column (exact rational compare, ties -> lower cluster number; the reference's np.argsort is unstable on ties) and the
// first 26 of that order get planes 0..25 (np.argsort(index)[:26]: the 26 leftmost, not the first 26 found).
__global__ __launch_bounds__(256) void dbscan_label_kernel(const float* __restrict__ mask, unsigned char* __restrict__ idmap,
                                                           int images) {
    __shared__ int label[CM_PIX];
    __shared__ int area[CM_PIX];
    __shared__ int colsum[CM_PIX];
    __shared__ unsigned char fg[CM_PIX];
    __shared__ int cand_root[CL_MAX_CAND];
    __shared__ int cand_rank[CL_MAX_CAND];
    __shared__ int changed;
    __shared__ int ncand;
    const int t = threadIdx.x;
    const float* m = mask + (long)blockIdx.x * CM_PIX;
    for (int i = t; i < CM_PIX; i += 256) {
        fg[i] = m[i] > 0.1f ? 1 : 0;
        area[i] = 0;
        colsum[i] = 0;
    }
    if (t == 0) ncand = 0;
    __syncthreads();
    // core pixels enter the labelling (label = own index), every other pixel stays out (-1)
    for (int i = t; i < CM_PIX; i += 256) {
        int n = 0;
        if (fg[i]) {
            const int y = i >> 7, x = i & 127;
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) {
                    const int yy = y + dy, xx = x + dx;
                    if ((dy | dx) == 0 || yy < 0 || yy >= CM_H || xx < 0 || xx >= CM_W) continue;
                    n += fg[yy * CM_W + xx];
                }
        }
        label[i] = n >= 3 ? i : -1;
    }
    __syncthreads();
    cm_components(label, &changed);
    // border pixels: the lowest cluster number (= root) among the core neighbours.  Decided from the core labels only, written
    // after the barrier, so a border pixel never sees another border pixel's assignment.
    int own[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int i = t + 256 * k;
        int l = label[i];
        if (l < 0 && fg[i]) {
            const int y = i >> 7, x = i & 127;
            int best = CL_NONE;
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) {
                    const int yy = y + dy, xx = x + dx;
                    if (yy < 0 || yy >= CM_H || xx < 0 || xx >= CM_W) continue;
                    const int ln = label[yy * CM_W + xx];
                    if (ln >= 0 && ln < best) best = ln;
                }
            l = best != CL_NONE ? best : -1;
        }
        own[k] = l;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int i = t + 256 * k, l = own[k];
        label[i] = l;
        if (l >= 0) {
            atomicAdd(&area[l], 1);
            atomicAdd(&colsum[l], i & 127);
        }
    }
    __syncthreads();
    // every qualifying cluster is a candidate (slot order is irrelevant: the rank below is a total order)
    for (int i = t; i < CM_PIX; i += 256)
        if (label[i] == i && area[i] >= CM_MIN_AREA) cand_root[atomicAdd(&ncand, 1)] = i;
    __syncthreads();
    const int nc = ncand;
    for (int c = t; c < nc; c += 256) {
        const int ra = cand_root[c];
        const long long sa = colsum[ra], aa = area[ra];
        int rank = 0;
        for (int o = 0; o < nc; ++o) {
            const int rb = cand_root[o];
            const long long lhs = (long long)colsum[rb] * aa, rhs = sa * (long long)area[rb];   // mean_b ? mean_a
            if (lhs < rhs || (lhs == rhs && rb < ra)) ++rank;
        }
        cand_rank[c] = rank;
    }
    __syncthreads();
    // reuse area[] as root -> plane map (-1 = dropped)
    for (int i = t; i < CM_PIX; i += 256) area[i] = -1;
    __syncthreads();
    for (int c = t; c < nc; c += 256)
        if (cand_rank[c] < CM_PLANES) area[cand_root[c]] = cand_rank[c];
    __syncthreads();
    unsigned char* out = idmap + (long)blockIdx.x * CM_PIX;
    for (int i = t; i < CM_PIX; i += 256) {
        const int l = label[i];
        const int p = l >= 0 ? area[l] : -1;
        out[i] = p >= 0 ? (unsigned char)p : CM_BG;
    }
}

// ---- region_cluster: skimage measure.label (8-connected components of mask != 0, raster label order, no area filter) +
// ndi.find_objects bounding boxes, sorted by xmin + xmax (twice the reference's "centroid", an integer in [1, 255]; Python's
// sorted is stable, so ties keep label order), cut to the first 26, then boxes of area (xmax-xmin)*(ymax-ymin) < 100 are
// skipped - they use up one of the 26 slots and produce no plane.  boxes [images][26][4] int32 = (ymin, xmin, ymax, xmax) with
// half-open stops, slots >= count[image] zero.
// The first 26 of the sorted order are found by 26 rounds of a block-wide minimum over the unique composite key
// (sort key << 12 | root): round r takes the smallest key above round r-1's, so ~1 000 components (checkerboard-like masks) cost
// the same as 26.
__global__ __launch_bounds__(256) void region_boxes_kernel(const float* __restrict__ mask, int* __restrict__ boxes,
                                                           int* __restrict__ count, int images) {
    __shared__ int label[CM_PIX];
    __shared__ int xmin[CM_PIX];
    __shared__ int xmax[CM_PIX];
    __shared__ int ymax[CM_PIX];
    __shared__ int win[3];
    __shared__ int sel[CM_PLANES];
    __shared__ int changed;
    const int t = threadIdx.x;
    const float* m = mask + (long)blockIdx.x * CM_PIX;
    for (int i = t; i < CM_PIX; i += 256) {
        label[i] = m[i] != 0.0f ? i : -1;
        xmin[i] = CM_W;
        xmax[i] = -1;
        ymax[i] = -1;
    }
    if (t == 0) win[0] = CL_NONE;
    __syncthreads();
    cm_components(label, &changed);
    for (int i = t; i < CM_PIX; i += 256) {
        const int l = label[i];
        if (l >= 0) {
            atomicMin(&xmin[l], i & 127);
            atomicMax(&xmax[l], i & 127);
            atomicMax(&ymax[l], i >> 7);
        }
    }
    __syncthreads();
    // this thread's roots (pixels 16t .. 16t+15) as composite keys; ymin of a component is its root's row
    int key[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int i = 16 * t + k;
        key[k] = label[i] == i ? ((xmin[i] + xmax[i] + 1) << 12) | i : CL_NONE;
    }
    // round r reduces into win[r % 3] and clears win[(r + 1) % 3] for the next round; the slot cleared in round r was last read
    // in round r - 2, before the barrier of round r - 1
    int prev = -1, nsel = 0;
    for (int r = 0; r < CM_PLANES; ++r) {
        int best = CL_NONE;
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (key[k] > prev && key[k] < best) best = key[k];
        if (best != CL_NONE) atomicMin(&win[r % 3], best);
        if (t == 0) win[(r + 1) % 3] = CL_NONE;
        __syncthreads();
        const int w = win[r % 3];
        if (w == CL_NONE) break;                 // uniform: every thread reads the same reduced value
        if (t == 0) sel[r] = w;
        prev = w;
        nsel = r + 1;
    }
    __syncthreads();
    if (t == 0) {
        int* bx = boxes + (long)blockIdx.x * CM_PLANES * 4;
        int num = 0;
        for (int r = 0; r < nsel; ++r) {
            const int root = sel[r] & (CM_PIX - 1);
            const int y0 = root >> 7, x0 = xmin[root], y1 = ymax[root] + 1, x1 = xmax[root] + 1;
            if ((x1 - x0) * (y1 - y0) < CL_MIN_BOX_AREA) continue;
            bx[4 * num + 0] = y0;
            bx[4 * num + 1] = x0;
            bx[4 * num + 2] = y1;
            bx[4 * num + 3] = x1;
            ++num;
        }
        for (int s = 4 * num; s < 4 * CM_PLANES; ++s) bx[s] = 0;
        count[blockIdx.x] = num;
    }
}

// ---- dense uint8 planes [images][26][32][128]: one block per (image, plane), 16 pixels per thread (one 16-byte load, one store)
__device__ __forceinline__ unsigned cl_byte_eq(unsigned w, unsigned v) {          // per byte: 1 where the byte of w == v
    unsigned r = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) r |= (((w >> (8 * j)) & 0xffu) == v ? 1u : 0u) << (8 * j);
    return r;
}
__global__ __launch_bounds__(256) void idmap_to_planes_u8_kernel(const unsigned char* __restrict__ idmap,
                                                                 unsigned char* __restrict__ planes) {
    const long img = blockIdx.x / CM_PLANES;
    const unsigned plane = blockIdx.x % CM_PLANES;
    const int off = threadIdx.x * 16;
    const u32x4 ids = *reinterpret_cast<const u32x4*>(idmap + img * CM_PIX + off);
    u32x4 o;
    o.x = cl_byte_eq(ids.x, plane);
    o.y = cl_byte_eq(ids.y, plane);
    o.z = cl_byte_eq(ids.z, plane);
    o.w = cl_byte_eq(ids.w, plane);
    *reinterpret_cast<u32x4*>(planes + (long)blockIdx.x * CM_PIX + off) = o;
}
__global__ __launch_bounds__(256) void boxes_to_planes_u8_kernel(const int* __restrict__ boxes, const int* __restrict__ count,
                                                                 unsigned char* __restrict__ planes) {
    const long img = blockIdx.x / CM_PLANES;
    const int plane = blockIdx.x % CM_PLANES;
    const int off = threadIdx.x * 16, y = off >> 7, x0 = off & 127;
    unsigned w[4] = {0u, 0u, 0u, 0u};
    if (plane < count[img]) {
        const int* bx = boxes + (img * CM_PLANES + plane) * 4;
        if (y >= bx[0] && y < bx[2]) {
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int x = x0 + j;
                if (x >= bx[1] && x < bx[3]) w[j >> 2] |= 1u << (8 * (j & 3));
            }
        }
    }
    u32x4 o;
    o.x = w[0];
    o.y = w[1];
    o.z = w[2];
    o.w = w[3];
    *reinterpret_cast<u32x4*>(planes + (long)blockIdx.x * CM_PIX + off) = o;
}

}  // namespace ccd
