// attention_probs.h - the attention probabilities themselves, P = softmax(Q K^T * scale) as fp32 [views, heads, 256, 256]
// (vision_transformer.py:85-86): what Block.forward(return_attention=True) hands to get_last_selfattention (:107-113, 253-260).
// Inspection only - the training path (attention_fwd.h) never materialises P.
//
// One workgroup (4 waves) per (view, head, strip of 128 queries): the head's K (256 keys x 64 d, 32 KiB) is staged in LDS once per
// strip, in attention_fwd.h's swizzled row image; each wave owns 32 queries and holds their whole score rows as eight 32x32
// accumulators (128 registers).  S is computed NON-transposed - A = the wave's Q rows straight from HBM, B = K rows from LDS - so
// accumulator register r of key tile kt holds keys 32 kt .. + 31 of query row (r & 3) + 8 (r >> 2) in lanes < 32 and of that row + 4
// in lanes >= 32: one dword store per register covers two 128-B row segments, the full-rate store shape (the transposed layout of
// attention_fwd.h, a lane per query, would put 64 rows under every store instruction).  Each probability is written once: the
// kernel is bound by those stores.  Row max and row sum are the kernel's own (in-register over the 8 tiles, then a butterfly over
// the 32 lanes of a half wave); the forward's LSE is not used.  No atomics and a fixed reduction order: the result is bitwise
// repeatable, and a view's probabilities depend on that view's q and k only.
#pragma once

namespace ccd {

constexpr int ATTP_STRIP = 128;                          // queries per workgroup
constexpr int ATTP_SMEM_BYTES = ATT_T * ATT_D * 2;       // the K image: 32 KiB

__global__ __launch_bounds__(256, 2) void attention_probs_kernel(const bf16_t* __restrict__ qkv, float* __restrict__ probs, int heads,
                                                                 float scale) {
    char* k_img = dynamic_smem();
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, hf = lane >> 5, lq = lane & 31;
    const int strip = blockIdx.x & 1, vh = blockIdx.x >> 1;            // vh = view * heads + head
    const int view = vh / heads, head = vh % heads;
    const int E = heads * ATT_D;
    const long row_stride = 3L * E;
    const bf16_t* q_base = qkv + (long)view * ATT_T * row_stride + head * ATT_D;
    const bf16_t* k_base = q_base + E;
    const int q0 = ATTP_STRIP * strip + 32 * w;                         // the wave's first query

    // A fragments: Q[q0 + lq][16 kk + 8 hf .. + 7] (requested in front of the staging loads)
    bf16x8 qf[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
        qf[kk] = *reinterpret_cast<const bf16x8*>(q_base + (long)(q0 + lq) * row_stride + 16 * kk + 8 * hf);
    att_stage_rows(k_base, row_stride, k_img);
    __syncthreads();

    // S[q0 + row][32 kt + lq]: B fragment (kt, kk) = K row 32 kt + lq, 16-B slot 2 kk + hf of the swizzled image
    f32x16 s[8];
#pragma unroll
    for (int kt = 0; kt < 8; ++kt) {
        const char* krow = k_img + (32 * kt + lq) * 128;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const bf16x8 kf = *reinterpret_cast<const bf16x8*>(krow + (((2 * kk + hf) ^ ((lq >> 1) & 7)) << 4));
            if (kk == 0) s[kt] = mfma_32x32x16_bf16(qf[0], kf, f32x16{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f});
            else s[kt] = mfma_32x32x16_bf16(qf[kk], kf, s[kt]);
        }
    }

    // softmax along each row: register r of every tile is one row (of the lane's half wave), its 256 keys are the 8 tiles x 32 lanes.
    // (butterfly reductions: every lane of the half wave ends with the same bits - a + b == b + a)
    const float c2 = scale * 1.4426950408889634f;                      // exp(x) = 2^(x log2 e)
    float inv[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        float m = s[0][r];
#pragma unroll
        for (int kt = 1; kt < 8; ++kt) m = fmaxf(m, s[kt][r]);
#pragma unroll
        for (int o = 1; o < 32; o <<= 1) m = fmaxf(m, shfl_xor(m, o));
        float sum = 0.f;
#pragma unroll
        for (int kt = 0; kt < 8; ++kt) {
            const float p = fast_exp2((s[kt][r] - m) * c2);
            s[kt][r] = p;
            sum += p;
        }
#pragma unroll
        for (int o = 1; o < 32; o <<= 1) sum += shfl_xor(sum, o);
        inv[r] = 1.0f / sum;
    }

    // register r of tile kt -> row q0 + (r & 3) + 8 (r >> 2) + 4 hf, keys 32 kt + lq: 32 lanes x 4 B = one 128-B segment per half wave
    float* out = probs + ((long)vh * ATT_T + q0 + 4 * hf) * ATT_T + lq;
#pragma unroll
    for (int r = 0; r < 16; ++r)
#pragma unroll
        for (int kt = 0; kt < 8; ++kt) out[((r & 3) + 8 * (r >> 2)) * ATT_T + 32 * kt] = s[kt][r] * inv[r];
}

}  // namespace ccd
