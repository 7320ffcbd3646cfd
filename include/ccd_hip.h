/* ccd_hip.h - C ABI of libccd_hip.so: the MI355X (gfx950) kernels of the CCD pretraining step.
 *
 * The reference (TongkunGuan/CCD) is pure Python on stock PyTorch and has no FFI boundary;
 * every entry point below replaces the ATen/cuDNN kernels that one reference call site launches implicitly.
 * The reference line each one stands in for is cited per function (paths relative to /root/reference).
 *
 * Conventions
 *   - plain pointers to DEVICE memory, explicit sizes, `void* stream` = hipStream_t (0 = default stream);
 *   - bf16 tensors are raw uint16 storage, fp32 tensors float; all tensors dense row-major unless a leading
 *     dimension (ld*) is passed, 16-byte aligned;
 *   - returns 0 on success, a negative CCD_E* code for argument errors, a positive hipError_t otherwise;
 *   - never allocates, never synchronises, re-entrant; work is enqueued on `stream`.
 *   - dynamic shapes (number of selected character rows) stay on the device: kernels take `const int* d_rows`
 *     where noted and are launched for the worst case.
 */
#ifndef CCD_HIP_H
#define CCD_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CCD_OK 0
#define CCD_EINVAL (-1)   /* bad pointer / size / alignment */
#define CCD_ESHAPE (-2)   /* shape not supported by this kernel (documented per function) */

typedef uint16_t ccd_bf16;

/* library identification; abi version is bumped on any signature change */
int ccd_abi_version(void);
const char* ccd_build_info(void);

/* Kernel-selection policy.  Which tile shape serves a product is decided by a small table of integers that is read ONCE
 * from the environment (CCD_GEMM_256, CCD_GEMM_256_MIN_M, CCD_GEMM_256_MIN_N, CCD_GEMM_256_F32, CCD_GEMM_256_DEEP,
 * CCD_GEMM_ROW384, CCD_ROWGEMM, CCD_LN_BWD_BPC, CCD_DEC_ATTN_SIMT, CCD_ATTN_SKEW, CCD_CU_RESERVE, CCD_LAB) and can be
 * changed at run time by key (lower case, without the prefix) - the launch path never calls getenv.  Unknown key:
 * CCD_EINVAL.  No reference counterpart: the reference leaves kernel selection to ATen / cuDNN heuristics.
 *   rowgemm    0: the row-wise epilogues (ccd_gemm_nt_resid_ln / _lnbwd) on gemm_row384.h's tile (N <= 384 only)
 *              1 (default): LayerNorm-backward product on rowgemm.h (N = 128, 256, 384, 512);
 *                 residual + LayerNorm on gemm_row384.h (N <= 384) / rowgemm.h (N = 512)
 *              2: rowgemm.h for both epilogues wherever its shapes allow (tests)
 *   attn_skew  cycles / 64 by which waves 4..7 of the attention-backward kernels trail waves 0..3 (lab, default 0)
 *   attn_tr    1 (default): dK / dV kernel on double-buffered LDS-DMA row images with transposing LDS reads; 0: four register-staged images
 *   gemm_tn384 1 (default): ViT weight gradients (P % 384 == 0, Q % 192 == 0) on the XCD-grouped kernel of gemm_tn384.h, 0: 128-square
 *              kernel, 2: never as a pair;  gemm_tn384_min_tiles (6): smallest single product it takes;  gemm_tn384_geom 2: also
 *              512x128 tiles for the E = 512 shapes (tested, no gain)
 *   cu_reserve compute units the persistent grids leave free (set while an RCCL gradient reducer is attached)
 *   cu_reserve_window -1 (default): every launch leaves them free; N >= 0: only the next cu_reserve_left launches do - the
 *              gradient reducer sets cu_reserve_left = N whenever it starts a bucket's all-reduce (ccd_amd/parallel.py)
 *   lab        scratch switch of the lab harnesses under tools/ (0 in production) */
int ccd_policy_set(const char* key, int value);
int ccd_policy_get(const char* key, int* value);

/* ---------------------------------------------------------------- GEMM family (nn.Linear / conv-as-GEMM)
 * epilogue codes (ccd_gemm_*: `epilogue`):                                                              */
#define CCD_EPI_BF16 0     /* C(bf16) = acc + bias                                                       */
#define CCD_EPI_GELU 1     /* C(bf16) = u = acc + bias, C2(bf16) = gelu(u)   Mlp.fc1+act, vit.py:59-61    */
#define CCD_EPI_RESID 2    /* C(f32) = resid + (acc + bias) * rowscale[row / rows_per_sample]  Block :109 */
#define CCD_EPI_F32 3      /* C(f32) = acc + bias                                                        */
#define CCD_EPI_ATOMIC 4   /* C(f32) += acc   (split-K partial sums; NT: K >= 16384 is cut into slices of 8192)   */
#define CCD_EPI_DGELU 5    /* C(bf16) = acc * gelu'(aux); C2 (optional, bf16) = gelu(aux)                */

/* C[M,N] = A[M,K] . B[N,K]^T   (F.linear(x, W): Dino/modules/vision_transformer.py:60,63,82,90,325-327)
 * K % 64 == 0, N % 8 == 0.  m_fastest: tile order hint (1 when B is the large operand). */
int ccd_gemm_nt(const ccd_bf16* A, long lda, const ccd_bf16* B, long ldb, int M, int N, int K, int epilogue,
                void* C, long ldc, void* C2, long ldc2, const float* bias, const float* resid, long ldr,
                const float* rowscale, int rows_per_sample, const ccd_bf16* aux, long ldaux, float alpha,
                int m_fastest, const int* d_rows, int rows_mul, float* colsum, void* stream);
/* Residual product with the NEXT LayerNorm folded into its epilogue (Block.forward, vision_transformer.py:107-113:
 * x = x + drop_path(f(...)); the following norm1 / norm2 / norm of the stream):
 *   C[M,N] (f32) = resid + (A . B^T + bias) * rowscale[row / rows_per_sample]
 *   y[M,N] (bf16) = (C - mean) * rstd * ln_gamma + ln_beta,  mean / rstd [M] saved for ccd_ln_bwd
 * One workgroup owns whole rows: N in {128, 256, 384, 512} with K % 128 == 0 (K % 192 at N = 384) runs the row-owner
 * kernel (rowgemm.h), any other N <= 384 (N % 8 == 0, K % 64 == 0) the 128 x 384 tile of gemm_row384.h;
 * replaces ccd_gemm_nt(EPI_RESID) + ccd_ln_fwd. */
int ccd_gemm_nt_resid_ln(const ccd_bf16* A, long lda, const ccd_bf16* B, long ldb, int M, int N, int K, float* C, long ldc,
                         const float* bias, const float* resid, long ldr, const float* rowscale, int rows_per_sample,
                         const float* ln_gamma, const float* ln_beta, float ln_eps, ccd_bf16* y, long ldy, float* mean,
                         float* rstd, void* stream);
/* A data-gradient product whose result IS the gradient of a LayerNorm output, with that LayerNorm's backward pass in the
 * epilogue (autograd of nn.LayerNorm(eps=1e-6) in Block.forward, vision_transformer.py:99,103,107-113):
 *   dy = A . B^T  (never written);  xhat = (x - mean) * rstd;  dx = rstd * (dy*gamma - mean_row(dy*gamma) - xhat * mean_row(dy*gamma*xhat))
 *   g (f32) = (accumulate ? g : 0) + dx;  dgamma += colsum(dy * xhat);  dbeta += colsum(dy)
 *   optional tail: gb (bf16) = g_new * rowscale[row / rows_per_sample], dbias += colsum(gb)
 * Same shape rules as ccd_gemm_nt_resid_ln.  Replaces ccd_gemm_nt(EPI_BF16) + ccd_ln_bwd. */
int ccd_gemm_nt_lnbwd(const ccd_bf16* A, long lda, const ccd_bf16* B, long ldb, int M, int N, int K, const float* x, long ldx,
                      const float* mean, const float* rstd, const float* gamma, float* g, long ldg, int accumulate,
                      float* dgamma, float* dbeta, ccd_bf16* gb, long ldgb, const float* rowscale, int rows_per_sample,
                      float* dbias, void* stream);
/* The same with the residual-gradient stream g in bf16 (ABI 10; N in {128, 256, 384} - CCD_ESHAPE otherwise): g is read as bf16,
 * accumulated in fp32 and rounded once per writer - half the bytes of the stream that every LayerNorm backward of a transformer
 * block reads and rewrites (the reference keeps that gradient in fp32 under autocast; gated by the parity tests). */
int ccd_gemm_nt_lnbwd_g16(const ccd_bf16* A, long lda, const ccd_bf16* B, long ldb, int M, int N, int K, const float* x, long ldx,
                          const float* mean, const float* rstd, const float* gamma, ccd_bf16* g, long ldg, int accumulate,
                          float* dgamma, float* dbeta, ccd_bf16* gb, long ldgb, const float* rowscale, int rows_per_sample,
                          float* dbias, void* stream);
/* The same with a SECOND LayerNorm of the same rows folded into the epilogue (ABI 11; N == 384 only - CCD_ESHAPE otherwise): a
 * segmentation tap (Dino/modules/vision_transformer.py:245-249: norm_seg[j](x) of the rows that norm1 of the next block also
 * normalises - same mean / rstd, other gamma).  LayerNorm's backward is linear in dy * gamma, so
 *   dx = core(dy * gamma + tap_dy * tap_gamma);  tap_dgamma += colsum(tap_dy * xhat);  tap_dbeta += colsum(tap_dy)
 * and x, g, gb move once instead of twice.  Replaces ccd_gemm_nt_lnbwd_g16 + ccd_ln_bwd of the tap (tap_dy: [M, N] bf16). */
int ccd_gemm_nt_lnbwd_tap_g16(const ccd_bf16* A, long lda, const ccd_bf16* B, long ldb, int M, int N, int K, const float* x, long ldx,
                              const float* mean, const float* rstd, const float* gamma, ccd_bf16* g, long ldg, int accumulate,
                              float* dgamma, float* dbeta, ccd_bf16* gb, long ldgb, const float* rowscale, int rows_per_sample,
                              float* dbias, const ccd_bf16* tap_dy, long ld_tap, const float* tap_gamma, float* tap_dgamma,
                              float* tap_dbeta, void* stream);
/* The whole MLP branch of a transformer block in one launch (Mlp.forward + the residual of Block.forward,
 * Dino/modules/vision_transformer.py:59-65,107-113, and the LayerNorm that consumes the stream next, :99/:156):
 *   h = gelu(bf16(y . W1^T + b1)) ;  out (f32) = resid + (h . W2^T + b2) * rowscale[row / rows_per_sample]
 *   ln_y (bf16) = (out - mean) * rstd * ln_gamma + ln_beta ;  ln_mean / ln_rstd [M] saved for ccd_ln_bwd
 * The [M, H] hidden activation stays on chip; `u` (optional, [M, H] bf16) receives the pre-activation the backward
 * pass needs, `gact` (optional, only with u) gelu(u) - the operand of the weight-gradient product dW2 = gb^T . gelu(u): stored
 * here, the backward's gelu'(u) product (CCD_EPI_DGELU) neither looks Phi up a second time nor writes gelu(u).
 * W1 = fc1.weight [H, E], W2 = fc2.weight [E, H] (bf16).  E in {128, 256, 384, 512}, H % 64 == 0.
 * Replaces ccd_gemm_nt(EPI_GELU) + ccd_gemm_nt_resid_ln. */
int ccd_mlp_fused(const ccd_bf16* y, long ldy, const ccd_bf16* w1, long ld1, const float* b1, const ccd_bf16* w2, long ld2,
                  const float* b2, const float* resid, long ldr, const float* rowscale, int rows_per_sample, float* out,
                  long ldc, const float* ln_gamma, const float* ln_beta, float ln_eps, ccd_bf16* ln_y, long ld_y,
                  float* ln_mean, float* ln_rstd, ccd_bf16* u, long ldu, ccd_bf16* gact, long ldga, int M, int E, int H, void* stream);
/* The whole second half of a transformer block in one launch (round 5): the tail of the attention branch in front of the fused MLP,
 *     x_mid = resid + rowscale1[row / rps] * (a . Wp^T + bp)            vision_transformer.py:91 (proj), :108 (residual + DropPath)
 *     y2    = LayerNorm(x_mid) * ln2_gamma + ln2_beta                   :109 (norm2)
 *     out   = x_mid + rowscale2[row / rps] * (gelu(y2 . W1^T + b1) . W2^T + b2);   ln_y = LayerNorm(out) * ln_gamma + ln_beta
 * x_mid never leaves the accumulator registers and y2 never leaves the operand registers: a forward pass that keeps nothing
 * (xmid = y2 = mean2 = rstd2 = u = NULL: the teacher) reads a and resid and writes out and ln_y - 604 MB per 131 072 rows instead
 * of the 1 208 MB of ccd_gemm_nt_resid_ln + ccd_mlp_fused.  With xmid / y2 / mean2 / rstd2 / u (all five or none) the tensors
 * the backward pass needs are written on the way.  E in {128, 256, 384}; with a DropPath scale rows_per_sample % 128 == 0
 * (CCD_ESHAPE otherwise: the caller takes the two separate launches); rowscale2 needs xmid (a dropped MLP branch still runs its
 * products - no branch around the weight ring - and reads x_mid back: out == x_mid exactly, u holds the real pre-activation).
 * tap_y (optional, with tap_gamma / tap_beta): a second LayerNorm of the same output rows, LayerNorm(out) * tap_gamma + tap_beta - the
 * segmentation tap that follows some blocks (vision_transformer.py:245-249) - instead of a ccd_ln_fwd pass over out.
 * Replaces ccd_gemm_nt_resid_ln + ccd_mlp_fused (+ ccd_ln_fwd). */
int ccd_proj_mlp_fused(const ccd_bf16* a, long lda, const ccd_bf16* wp, long ldp, const float* bp, const float* resid, long ldr,
                       const float* rowscale1, const float* ln2_gamma, const float* ln2_beta, float* xmid, long ldxm, ccd_bf16* y2,
                       long ldy2, float* mean2, float* rstd2, const ccd_bf16* w1, long ld1, const float* b1, const ccd_bf16* w2,
                       long ld2, const float* b2, const float* rowscale2, int rows_per_sample, float* out, long ldc,
                       const float* ln_gamma, const float* ln_beta, float ln_eps, ccd_bf16* ln_y, long ld_y, float* ln_mean,
                       float* ln_rstd, ccd_bf16* u, long ldu, const float* tap_gamma, const float* tap_beta, ccd_bf16* tap_y, long ld_tap,
                       int M, int E, int H, void* stream);
/* The same, and gelu(u) [M, H] bf16 is stored too (ABI 12; u required): the packed second-product operands of the forward kernel ARE that
 * tensor, so the backward pass neither gathers Phi a second time nor writes gelu(u) - what ccd_mlp_bwd_fused expects of its caller. */
int ccd_proj_mlp_fused_gact(const ccd_bf16* a, long lda, const ccd_bf16* wp, long ldp, const float* bp, const float* resid, long ldr,
                       const float* rowscale1, const float* ln2_gamma, const float* ln2_beta, float* xmid, long ldxm, ccd_bf16* y2,
                       long ldy2, float* mean2, float* rstd2, const ccd_bf16* w1, long ld1, const float* b1, const ccd_bf16* w2,
                       long ld2, const float* b2, const float* rowscale2, int rows_per_sample, float* out, long ldc,
                       const float* ln_gamma, const float* ln_beta, float ln_eps, ccd_bf16* ln_y, long ld_y, float* ln_mean,
                       float* ln_rstd, ccd_bf16* u, long ldu, ccd_bf16* gact, long ldga, const float* tap_gamma, const float* tap_beta, ccd_bf16* tap_y, long ld_tap,
                       int M, int E, int H, void* stream);
/* The data-gradient chain of the MLP branch in one launch - the backward of the block half above (Mlp.forward + LayerNorm-2,
 * Dino/modules/vision_transformer.py:59-65,110 in autograd order; ABI 12):
 *   dh = gb . W2 ;  du = dh * gelu'(u) ;  dy2 = du . W1 ;  LayerNorm-2 backward of dy2 as in ccd_gemm_nt_lnbwd_g16
 *   (g (+)= dx on the bf16 stream, dgamma / dbeta +=, gb_out = bf16(g * rowscale[row / rows_per_sample]), dbias += colsum(gb_out))
 * w2t = fc2.weight^T [H, E], w1t = fc1.weight^T [E, H] (the transposed bf16 mirrors), u [M, H] the stored pre-activation.  du [M, H] is
 * written ONCE, for the weight-gradient pair that follows (ccd_gemm_tn_pair: {gb, gelu(u)}, {du, y2}), and never read back; db1 +=
 * column sums of du (fc1.bias gradient).  gb_out must not alias gb.  E in {256, 384}, H % 128 == 0; CCD_ESHAPE otherwise: the caller
 * takes ccd_gemm_nt(EPI_DGELU) + ccd_gemm_nt_lnbwd_g16.  Replaces those two. */
int ccd_mlp_bwd_fused(const ccd_bf16* gb, long ldgb, const ccd_bf16* w2t, long ld2, const ccd_bf16* w1t, long ld1, const ccd_bf16* u,
                      long ldu, ccd_bf16* du, long lddu, float* db1, const float* x, long ldx, const float* mean, const float* rstd,
                      const float* gamma, ccd_bf16* g, long ldg, int accumulate, float* dgamma, float* dbeta, ccd_bf16* gb_out, long ld_gbo,
                      const float* rowscale, int rows_per_sample, float* dbias, int M, int E, int H, void* stream);

/* colsum (optional, epilogues BF16 / DGELU): [N] fp32, += column sums of the output (bias gradient of the producer).
 * CCD_EPI_GELU accepts C == NULL (only gelu(u) is stored: forward passes that keep no activations). */
/* C[P,Q] (+)= sum_m A[m,P] * B[m,Q]   (weight gradients dW = dY^T X of every Linear; autograd of the above)
 * P % 8 == 0, Q % 8 == 0; epilogue CCD_EPI_ATOMIC accumulates into fp32 C (split over m), CCD_EPI_F32 stores. */
int ccd_gemm_tn(const ccd_bf16* A, long lda, const ccd_bf16* B, long ldb, int P, int Q, int Mc, int epilogue,
                float* C, long ldc, float alpha, int splits, const int* d_rows, int rows_mul, void* stream);
/* The same weight-gradient product with the BIAS gradient of the same Linear in one pass over dY:
 * C[P,Q] += A^T . B (fp32 atomics, split over m) and colsum_a[P] += column sums of A - the rows of dY are summed while they
 * pass through the loader's registers (replaces ccd_gemm_tn + ccd_colsum_bf16: one read of dY less). */
int ccd_gemm_tn_colsum(const ccd_bf16* A, long lda, const ccd_bf16* B, long ldb, int P, int Q, int Mc, float* C, long ldc,
                       float* colsum_a, int splits, void* stream);
/* Two weight-gradient products over the SAME contraction rows in one launch: C1[P1,Q1] += A1^T . B1 and C2[P2,Q2] += A2^T . B2
 * (fp32 atomics) - the pairs autograd produces together: {fc2.weight, fc1.weight} once gelu'(u) is applied, {proj.weight,
 * qkv.weight} once the attention backward has run (Dino/modules/svtr.py:92-145).  With P % 384 == 0, Q % 192 == 0 and
 * Mc % 32 == 0 both run in gemm_tn384.h's XCD-grouped launch and share ONE atomic epilogue per workgroup; any other shape
 * falls back to two ccd_gemm_tn calls.  Results are those of the two separate calls up to fp32 summation order. */
int ccd_gemm_tn_pair(const ccd_bf16* A1, long lda1, const ccd_bf16* B1, long ldb1, int P1, int Q1, float* C1, long ldc1,
                     const ccd_bf16* A2, long lda2, const ccd_bf16* B2, long ldb2, int P2, int Q2, float* C2, long ldc2, int Mc,
                     void* stream);
/* The same with a caller-owned fp32 WORKSPACE (round 4): each contraction slice stores its partial tile into its own plane of ws
 * (plain stores) and one reduction pass adds the planes to C1 / C2 - replaces 75 MB of fp32 atomics per MLP pair.  ws_floats >=
 * ccd_gemm_tn_pair_ws_floats(P1, Q1, P2, Q2) guarantees the path is taken (0 = shapes the grouped kernel does not cover); a null or
 * too small workspace falls back to ccd_gemm_tn_pair's atomics.  The workspace is scratch: its contents are undefined afterwards and
 * launches that share it must be ordered on one stream. */
long ccd_gemm_tn_pair_ws_floats(int P1, int Q1, int P2, int Q2);
int ccd_gemm_tn_pair_ws(const ccd_bf16* A1, long lda1, const ccd_bf16* B1, long ldb1, int P1, int Q1, float* C1, long ldc1,
                        const ccd_bf16* A2, long lda2, const ccd_bf16* B2, long ldb2, int P2, int Q2, float* C2, long ldc2, int Mc,
                        float* ws, long ws_floats, void* stream);
/* d_rows (optional, both GEMMs): device int; the effective row count (NT: M, TN: Mc) is
 * min(static value, d_rows[0] * rows_mul) so data-dependent row counts never reach the host. */

/* ---------------------------------------------------------------- LayerNorm (eps 1e-6), vit.py:99,103,156,162-166 */
int ccd_ln_fwd(const float* x, const float* gamma, const float* beta, ccd_bf16* y, float* mean, float* rstd,
               int rows, int E, float eps, void* stream);
/* g (+)= dx ; dgamma += ..., dbeta += ... (fp32 atomics; caller zeroes them once per step).
 * Optional fused tail: gb(bf16) = g_new * rowscale[row / rows_per_sample] (the gradient entering the next residual
 * branch, DropPath scale applied) and dbias += column sums of gb. */
int ccd_ln_bwd(const ccd_bf16* dy, const float* x, const float* mean, const float* rstd, const float* gamma,
               float* g, int accumulate, float* dgamma, float* dbeta, ccd_bf16* gb, const float* rowscale,
               int rows_per_sample, float* dbias, int rows, int E, void* stream);

int ccd_ln_bwd_g16(const ccd_bf16* dy, const float* x, const float* mean, const float* rstd, const float* gamma,
                   ccd_bf16* g /* bf16 stream, see ccd_gemm_nt_lnbwd_g16 */, int accumulate, float* dgamma, float* dbeta, ccd_bf16* gb,
                   const float* rowscale, int rows_per_sample, float* dbias, int rows, int E, void* stream);

/* ---------------------------------------------------------------- attention, vit.py:80-92 (T = 256, head_dim = 64)
 * qkv [views, 256, 3, heads, 64] bf16 (the layout Attention.forward reshapes to), out [views, 256, heads*64]  */
int ccd_attention_fwd(const ccd_bf16* qkv, ccd_bf16* out, float* lse, int views, int heads, float scale,
                      void* stream);
/* The attention probabilities themselves (ABI 15): probs [views, heads, 256, 256] fp32 = softmax(q k^T * scale) per row, what
 * Attention.forward returns as `attn` (vit.py:85-86, 92) and get_last_selfattention hands out (vit.py:253-260).  Inspection only:
 * the training path never materialises them.  The kernel computes its own row max / sum (no LSE).  heads in {2, 3, 6, 8, 12}
 * (E = 128, 192, 384, 512, 768) - CCD_ESHAPE otherwise.  No atomics: bitwise repeatable, each view independent of the others. */
int ccd_attention_probs(const ccd_bf16* qkv, float* probs, int views, int heads, float scale, void* stream);
/* d_qkv_bias (nullable, fp32 [3 * heads * 64], ACCUMULATED): the gradient of the qkv bias (vit.py:75 `qkv_bias`; what autograd's
 * Linear backward computes as grad_output.sum(0) over d_qkv) without a pass over d_qkv:
 *   q part  column sums of the fp32 dQ tiles, inside the dQ kernel; needs bias_ws = ccd_attention_bwd_ws_floats(views, heads)
 *           floats of scratch (per-workgroup partial rows, plain stores)
 *   k part  identically zero (the softmax is shift invariant): nothing is added
 *   v part  = column sums of d_out (every softmax row sums to 1), which the caller supplies WITHOUT touching d_out:
 *           dout_colsum_mat == null: dout_colsum_vec [E] IS colsum(d_out);
 *           otherwise colsum(d_out) = dout_colsum_vec [E] . dout_colsum_mat [E, E] (row-major, ld_mat) - for d_out = gb . Wproj
 *           (vit.py:90-91) that is (proj.bias gradient) . (proj.weight).
 * A third, tiny launch adds the partial rows up and forms the matvec. */
long ccd_attention_bwd_ws_floats(int views, int heads);
int ccd_attention_bwd(const ccd_bf16* qkv, const ccd_bf16* out, const ccd_bf16* d_out, const float* lse,
                      float* delta_ws, ccd_bf16* d_qkv, int views, int heads, float scale, float* d_qkv_bias, float* bias_ws,
                      const float* dout_colsum_vec, const float* dout_colsum_mat, long ld_mat, void* stream);

/* ---------------------------------------------------------------- patch embedding, vit.py:128-131,225-236
 * img [views,3,32,128] fp32 NCHW; w [E,3,4,4]; pos [256,E] = the bicubically resampled pos_embed; out fp32 [views*256,E] */
int ccd_patch_embed_fwd(const float* img, const float* w, const float* bias, const float* pos, float* out, int views,
                        int E, void* stream);
/* g = d(out) fp32 [views*256,E]; d_w [E,48], d_bias [E], d_pos [256,E] are ACCUMULATED (fp32 atomics).
 * Caller-provided workspaces: ws_g bf16 [views*256, E] (receives bf16(g)), ws_patches bf16 [views*256, 48].
 * d_w = bf16(g)^T . bf16(patches) on the MFMA path (TN GEMM), d_bias = column sums of bf16(g). */
int ccd_patch_embed_bwd(const float* img, const float* g, float* d_w, float* d_bias, float* d_pos, ccd_bf16* ws_g,
                        ccd_bf16* ws_patches, int views, int E, void* stream);
/* the same on a bf16 stream g: it is the TN product's operand as it lies (no ws_g) */
int ccd_patch_embed_bwd_g16(const float* img, const ccd_bf16* g, float* d_w, float* d_bias, float* d_pos, ccd_bf16* ws_patches, int views,
                            int E, void* stream);
/* C[M,N] (+)= op(A) . B, fp32, tiny problems (bicubic pos-embed resampling = fixed 256x256 linear map, vit.py:182-201) */
int ccd_small_matmul_f32(const float* A, const float* B, float* C, int M, int N, int K, int trans_a, int accumulate,
                         void* stream);
/* out[n] += sum_rows x[row,n] (bias gradients) */
int ccd_colsum_bf16(const ccd_bf16* x, long ld, int rows, int N, const int* d_rows, int rows_mul, float* out,
                    void* stream);
/* bf16 mirrors (and transposed mirrors) of a batch of fp32 matrices */
typedef struct ccd_mirror_desc {
    const float* src;
    ccd_bf16* dst;    /* [rows, cols] or NULL */
    ccd_bf16* dst_t;  /* [cols, rows] or NULL */
    int rows, cols;
    int tile_begin;   /* first 64x64 tile of this matrix in the launch (prefix sum over ceil(rows/64) * ceil(cols/64); ABI 9: was 32x32) */
    int pad_;
} ccd_mirror_desc;
int ccd_mirror_bf16(const ccd_mirror_desc* d_descs, int ndesc, int total_tiles, void* stream);
int ccd_cast_bf16(const float* src, ccd_bf16* dst, long n, void* stream);
/* dst(bf16)[r,:] = src(f32)[r,:] * rowscale[r / rows_per_sample] (rowscale may be NULL): residual gradient -> branch */
int ccd_scale_cast_rows(const float* src, ccd_bf16* dst, const float* rowscale, int rows_per_sample, long rows, int E,
                        void* stream);

/* ---------------------------------------------------------------- character-region path (id maps: uint8, 255 = none)
 * label_cluster.forward, Dino/utils/DBSCAN.py:65-103: mask [images,32,128] (nonzero = text) -> idmap            */
int ccd_ccl_label(const float* mask, uint8_t* idmap, int images, void* stream);
int ccd_mask_to_idmap(const float* mask, uint8_t* idmap, int images, void* stream);
/* softmax(seg)[:,1] > 0.5 of the first `images` images (dino_vision.py:65-66); seg [>=images,2,32,128] fp32 */
int ccd_seg_to_mask(const float* seg_logits, float* mask, int images, void* stream);
/* ---------------------------------------------------------------- data pipeline
 * clusterpixels(im, 2), mask_create/generate_mask.py:13-29 (= Dino/utils/kmeans.py:7-23): 2-means of the gray values of a
 * word image + "the cluster that owns the border is background".  A RAGGED batch: image i is gray[offsets[i] ..
 * offsets[i+1]) with hw[2i] rows x hw[2i+1] columns (device arrays; offsets has images + 1 entries); mask gets 0 / 1
 * at the same offsets.  Integer / fp64 arithmetic with a fixed operation order: bit-exact against oracle/datapipe_np.py. */
int ccd_kmeans2_mask(const uint8_t* gray, const long* offsets, const int* hw, uint8_t* mask, int images, void* stream);
/* The three views of ImageDatasetSelfSupervisedKmeans._process_training (datasetsupervised_kmeans.py:48-87) from resized
 * uint8 images img [B,H,W,3]: out fp32 [B,3,3,H,W] = (plain, augment(params[b,0]), warp_theta(augment(params[b,1]))),
 * each normalised with mean3 / std3 (HOST arrays of 3 floats; dataset.py:79-80).  params fp32 [B,2,96] (layout in
 * kernels/datapipe.h), theta fp32 [B,3,3] = the `metrics` tensor the model receives (identity = no warp).
 * Two launches.  (1) The reference's imgaug chain (augmentation_pipelines.py:120-205): one workgroup per (sample, view) holds
 * the uint8 image in LDS and applies ONE member of each group in the reference's order - `arithmetic` (noises, dropouts,
 * JpegCompression, Emboss / EdgeDetect / DirectedEdgeDetect, the PIL filter presets ...), `color` (cv2's 8-bit HSV members,
 * Grayscale, quantisation ...), `Blur` (Gaussian / average / median / motion / bilateral blur, Sharpen), `contrast` (gamma,
 * linear, sigmoid, log, per-channel histogram equalisation) - rounding to uint8 between the groups like imgaug, and stages the
 * result in staged_ws [B,2,H,W,3] (caller-allocated scratch).  (2) Normalisation and the affine warp of view 2 read those.
 * H * W is bounded by the chain's LDS images (CCD_ESHAPE beyond).
 * overlay (optional): fp16 [overlay_layers, 2, H, W] = (alpha, intensity) planes of imgaug's cloud layers (`weather` group: Fog,
 * Clouds - augmentation_pipelines.py:192-193); a parameter row with params[81] = n > 0 blends its layers params[82] .. + n - 1 after
 * the contrast group: out = trunc(clip((1 - alpha) * v + alpha * intensity, 0, 255)).  The planes are drawn on the host
 * (ccd_amd/dataset/weather.py: frequency noise by FFT, a few hundred microseconds per layer).
 * warp_maps (optional): fp32 [warp_count, 2, H, W] = the SOURCE position (x, y), in pixels, of every output pixel of a
 * piecewise-affine warp (imgaug PiecewiseAffine, the finetuning geometry's second member, dataset_pretrain.py:156; drawn on the
 * host); a sample whose view-2 row has params[84] = m > 0 samples map m - 1 (bilinear, zero fill) instead of theta. */
int ccd_augment_views(const uint8_t* img, const float* params, const float* theta, float* out, uint8_t* staged_ws, int batch,
                      int height, int width, const float* mean3, const float* std3, const uint16_t* overlay, int overlay_layers,
                      const float* warp_maps, int warp_count, void* stream);
/* affine_grid(theta[:, :2]) + grid_sample(bilinear) > 0.1, dino_vision.py:72-77 / train.py:234-236; theta row stride in floats */
int ccd_warp_idmap(const uint8_t* src, const float* theta, int theta_stride, uint8_t* dst, int images, void* stream);
/* ABIDINOModel.attention, dino_vision.py:38-49, in sparse form: per token up to 4 (plane, normalised weight) pairs -
 * tok_plane [views,256,4] (255 = unused slot), tok_coef [views,256,4]; the central 2x2 of a 4x4 cell touches one plane in
 * the labelled view, possibly several in the warped view (components one pixel apart can end up side by side) */
int ccd_region_stats(const uint8_t* idmap, uint8_t* tok_plane, float* tok_coef, uint8_t* present, int views,
                     void* stream);
/* dino_vision.py:82-85: nsel[b], offset[b], total[0] = M, new_index [batch,26] */
int ccd_select_scan(const uint8_t* present, int batch, int* nsel, int* offset, int* total, uint8_t* new_index,
                    void* stream);
/* rows [2M,E] bf16 = gathered pooled character vectors of both views (dino_vision.py:44-47,87); views = 2*batch */
int ccd_region_pool_fwd(const ccd_bf16* feat, const uint8_t* tok_plane, const float* tok_coef, const int* nsel,
                        const int* offset, const int* total, ccd_bf16* rows, int batch, int E, void* stream);
int ccd_region_pool_bwd(const ccd_bf16* d_rows, const uint8_t* tok_plane, const float* tok_coef, const int* nsel,
                        const int* offset, const int* total, ccd_bf16* d_feat, int batch, int E, void* stream);
int ccd_idmap_to_planes(const uint8_t* idmap, float* planes, int images, void* stream);
int ccd_planes_to_idmap(const float* planes, uint8_t* idmap, int images, void* stream);

/* ---------------------------------------------------------------- the public clusterers of Dino/utils/DBSCAN.py
 * One workgroup per 32x128 mask, images masks per launch; images == 0 is a no-op.  Outputs are bit-exact against the
 * reference wherever its own order is defined (mean-column ties: lower cluster number first).
 * DBSCAN_cluster.forward, Dino/utils/DBSCAN.py:14-59 (sklearn DBSCAN(eps=1.5, min_samples=4) on the pixels with mask > 0.1,
 * restated on the grid: core = >= 3 foreground 8-neighbours, clusters = 8-connected core components, border pixels join the
 * lowest-numbered neighbouring cluster; clusters of < 30 pixels dropped, the 26 with the smallest mean column kept, in that
 * order): mask [images,32,128] fp32 -> idmap uint8 [images,32,128] (plane index, 255 = none)                          */
int ccd_dbscan_label(const float* mask, uint8_t* idmap, int images, void* stream);
/* region_cluster.forward, Dino/utils/DBSCAN.py:110-141 (8-connected components of mask != 0 + their bounding boxes, stable
 * sort by xmin + xmax, first 26, boxes of area < 100 skipped): mask [images,32,128] fp32 -> boxes int32 [images,26,4]
 * (ymin, xmin, ymax, xmax; half-open stops; slots >= count zero), count int32 [images]                               */
int ccd_region_boxes(const float* mask, int* boxes, int* count, int images, void* stream);
/* the reference's uint8 [26,32,128] planes per image (DBSCAN.py:25,56,78,127): from an id map (DBSCAN_cluster,
 * label_cluster) or from boxes + count (region_cluster, planes may overlap); idmap and planes 16-byte aligned       */
int ccd_idmap_to_planes_u8(const uint8_t* idmap, uint8_t* planes, int images, void* stream);
int ccd_boxes_to_planes_u8(const int* boxes, const int* count, uint8_t* planes, int images, void* stream);

/* ---------------------------------------------------------------- the super-resolution metrics of Dino/metric/eval_superpixel.py
 * Inputs are fp32 [images, channels, H, W] with contiguous rows (row stride W); n* / c* are the element strides of the image and
 * channel dimensions, so a channel slice such as the [:, :3] view of an RGB + mask batch is read in place.  16-byte loads are used
 * when every input is 16-byte aligned with W, n* and c* multiples of 4, scalar loads otherwise.  window: odd, 1..15 (CCD_ESHAPE
 * otherwise); taps: HOST memory, the window's 1-D Gaussian (eval_superpixel.py:17-20, symmetric), applied as two separable passes
 * with zero padding window / 2 (F.conv2d's padding).  images == 0 is a no-op.  No float atomics: results are bitwise repeatable
 * and an image's values do not depend on the rest of the batch. */
/* doubles of ccd_ssim_fwd's partials (one per (plane, 16x32 tile)); -1 on a bad shape */
long ccd_ssim_ws_doubles(int images, int channels, int H, int W);
/* _ssim / _tri_ssim, eval_superpixel.py:29-49,91-120 without the final mean: x3 == NULL -> SSIM of (x1, x2) (5 moments),
 * else TRI_SSIM of (x1, x2, x3) (9 moments, no factor 2).  partials[ccd_ssim_ws_doubles] fp64: the sum of the map over each tile */
int ccd_ssim_fwd(const float* x1, long n1, long c1, const float* x2, long n2, long c2, const float* x3, long n3, long c3, int images,
                 int channels, int H, int W, int window, const float* taps, double* partials, void* stream);
/* partials -> per_image fp32 [images] (the mean over channels x H x W, size_average=False) and, if mean != NULL, fp32 [1] the mean
 * over the batch (size_average=True); one workgroup, fixed order */
int ccd_ssim_reduce(const double* partials, int images, int channels, int H, int W, float* per_image, float* mean, void* stream);
/* gradients of sum_n gscale[n] * sum over image n of the map (gscale fp32 [images] on the device: the upstream gradient over the
 * count of the mean) w.r.t. each input whose dx* is non-NULL: fp32 contiguous [images, channels, H, W], overwritten.  One launch;
 * the moments are recomputed, dS/d(moment) is blurred back with the same window (its adjoint) */
int ccd_ssim_bwd(const float* x1, long n1, long c1, const float* x2, long n2, long c2, const float* x3, long n3, long c3, int images,
                 int channels, int H, int W, int window, const float* taps, const float* gscale, float* dx1, float* dx2, float* dx3,
                 void* stream);
/* doubles of ccd_psnr_fwd's partials; -1 on a bad shape */
long ccd_psnr_ws_doubles(int images, int channels, int H, int W);
/* calculate_psnr, eval_superpixel.py:8-14, on the first `channels` (1..3: the caller's min(C, 3)) channels of a and b: mse fp64 [1] =
 * the mean of (255 a - 255 b)^2 (products and difference rounded to fp32, square and sum in fp64), psnr fp32 [1] =
 * 20 log10(255 / sqrt(mse)) (+inf for mse == 0, where the reference returns float('inf'): the caller's test) */
int ccd_psnr_fwd(const float* a, long an, long ac, const float* b, long bn, long bc, int images, int channels, int H, int W,
                 double* partials, double* mse, float* psnr, void* stream);

/* ---------------------------------------------------------------- the segmentation metrics of Dino/metric/eval_IOU.py
 * Labels are integers in [0, CCD_SEG_CLASSES).  A label map is [images, pixels] with the pixels of an image contiguous and a free
 * image stride in elements (>= 0), so x[:, 0] and out[:B] views are read in place; its element type is a dtype code: uint8, int32,
 * int64 or fp32 holding integral values.  16-byte loads (4-byte loads for uint8 beside a wider map) are used where the base and
 * the image stride are aligned for them, element loads otherwise.  The caller allocates everything; the calls clear what they
 * write.  images == 0 is a no-op.  CCD_EINVAL: a missing pointer or a negative stride; CCD_ESHAPE: pixels < 1, pixels >= 2^31,
 * an unknown dtype code, classes outside 2..32.  Counts are integers and integer adds commute: results are bitwise repeatable
 * and an image's values do not depend on the rest of the batch. */
#define CCD_SEG_CLASSES 32
#define CCD_SEG_U8 0
#define CCD_SEG_I32 1
#define CCD_SEG_I64 2
#define CCD_SEG_F32 3
/* cm int32 [images, 32, 32]: cm[i, g, e] = the pixels of image i with gt label g and eval label e; status int32 [images]: bit 0 =
 * the image has a label outside [0, 32), a non-integral value or a NaN (those pixels are not counted).  An image of at most 4096
 * pixels is one workgroup; a larger one is split over several that add their non-zero bins with integer atomics. */
int ccd_seg_confusion(const void* eval, int eval_dtype, long eval_stride, const void* gt, int gt_dtype, long gt_stride, int images,
                      long pixels, int* cm, int* status, void* stream);
/* the same with eval = the arg-max over `classes` (2..32) channels of fp32 logits [images, classes, pixels] (image and channel
 * strides in elements, pixels contiguous); the first maximum wins as in torch.argmax (two classes: logit1 > logit0, which is
 * ccd_seg_to_mask's rule); a NaN logit sets status bit 0.  The logits are read once, the prediction is never written. */
int ccd_seg_confusion_logits(const float* logits, long image_stride, long channel_stride, int classes, const void* gt, int gt_dtype,
                             long gt_stride, int images, long pixels, int* cm, int* status, void* stream);
/* cm, status -> scores fp64 [images, 5] = pixel_accuracy, mean_accuracy, mean_IU, fore_IU, frequency_weighted_IU
 * (eval_IOU.py:4-137; t_c / n_c / d_c = row sum / column sum / diagonal of cm, class sums in ascending class order in fp64).
 * Sets status bit 1 where fore_IU is undefined (fewer than two classes in the union of the two maps): that column is NaN.  An
 * image with status bit 0 gets five NaNs. */
int ccd_seg_scores(const int* cm, int* status, int images, double* scores, void* stream);

/* ---------------------------------------------------------------- the recognition scores of Dino/metric/eval_acc.py (ABI 18)
 * TextAccuracy's scoring loop (eval_acc.py:33-56) from the decoder's output, without the strings ever existing on the host.
 * ccd_text_score, one wavefront per sample:
 *   scores      fp32 [batch, steps, classes], classes contiguous, sample and step strides in elements (>= 0): greedy decoding's
 *               probs[:, :done] view is read in place.  The class of a step is its first maximum; the prediction ends in front of
 *               the first end_idx step and skips pad_idx steps (Dino/convertor/attn.py:133-154); a pad_idx outside [0, classes)
 *               skips nothing (NRTRDecoder has no padding output: classes = num_classes - 1).
 *   table_raw   int32 [>= classes, raw_width], table_norm int32 [>= classes, norm_width]: the code points a class stands for, as
 *               idx2str writes them and after the metric's normalisation, each row padded with -1 (a row may be empty: the end and
 *               padding classes; or hold several code points: `<UKN>`).  Widths 1..64; steps * norm_width <= CCD_TEXT_COLS.
 *   gt          int32 [batch, gt_cols] code points of the ground truth (row stride gt_stride), gt_len int32 [batch] (clamped to
 *               0..gt_cols); any length.  The ground truth is normalised on the device, code point by code point: A-Z -> a-z,
 *               U+212A -> k, U+0130 -> i, [a-z0-9^] and U+4E00..U+9FA5 kept, everything else dropped - what
 *               re.sub('[^A-Z^a-z^0-9^\u4e00-\u9fa5]', '', s.lower()) gives for every string.
 *   records     int32 [batch, CCD_TEXT_RECORD] = {Levenshtein distance of the normalised strings, position-wise equal code points of
 *               the raw strings over the shorter one, raw ground-truth length, 1 if the normalised strings are equal}.
 * ccd_text_accumulate, one workgroup: totals int64 [5] += {equal characters, ground-truth characters, correct words, words, edit
 * distance}, total_ned fp64 [1] += sum of distance / max(raw ground-truth length, 1), summed in a fixed order (no atomics: the same
 * batches in the same order give the same bits); launches that share the totals must be ordered on one stream.
 * batch == 0 is a no-op.  CCD_EINVAL: a missing pointer, a negative stride or size; CCD_ESHAPE: steps or classes < 1, a width outside
 * 1..64, steps * norm_width > CCD_TEXT_COLS, end_idx outside [0, classes). */
#define CCD_TEXT_COLS 128
#define CCD_TEXT_RECORD 4
int ccd_text_score(const float* scores, long sample_stride, long step_stride, int batch, int steps, int classes, const int* table_raw,
                   int raw_width, const int* table_norm, int norm_width, int end_idx, int pad_idx, const int* gt, long gt_stride,
                   int gt_cols, const int* gt_len, int* records, void* stream);
int ccd_text_accumulate(const int* records, int batch, long* totals, double* total_ned, void* stream);
/* The same records from the logits of a CTC head (ABI 20; no reference counterpart: the reference has no CTC head).  scores fp32
 * [batch, steps, classes] are frames; the class of a frame is its first maximum, a frame counts where its class is not the blank
 * (class 0) and differs from the frame before.  There is no end class and no padding class; tables, ground truth, records, error
 * codes and limits as for ccd_text_score (row 0 of the tables, the blank, is never read).  The records feed ccd_text_accumulate. */
int ccd_text_score_ctc(const float* scores, long sample_stride, long step_stride, int batch, int steps, int classes, const int* table_raw,
                       int raw_width, const int* table_norm, int norm_width, const int* gt, long gt_stride, int gt_cols, const int* gt_len,
                       int* records, void* stream);
/* The same records for classes that are already decoded (ABI 21): paths int32 [batch, >= steps] with row stride path_stride, a
 * sample's classes in front of its first negative entry (at most `steps` of them) - a rank of ccd_ctc_beam_search's paths, row
 * stride beam * steps.  A class outside [1, classes) is never an index and counts no characters.  Tables, ground truth, records,
 * error codes and limits as for ccd_text_score. */
int ccd_text_score_paths(const int* paths, long path_stride, int batch, int steps, int classes, const int* table_raw, int raw_width,
                         const int* table_norm, int norm_width, const int* gt, long gt_stride, int gt_cols, const int* gt_len, int* records,
                         void* stream);

/* ---------------------------------------------------------------- CTC recognition head (ABI 20)
 * No reference counterpart (the reference has no CTC head); the semantics are those of
 * torch.nn.CTCLoss(blank=0, reduction='mean', zero_infinity=True) applied to log_softmax(logits).
 * ccd_ctc_pool_fwd: tokens bf16 [images, rows * cols, E] (token = row * cols + column) -> frames bf16 [images * cols, E], frame c = the
 *   mean over the rows of column c, summed in fp32.  ccd_ctc_pool_bwd: d_tokens bf16 [images, rows * cols, E] = d_frames / rows at
 *   every row.  E % 8 == 0, rows 1..64 (CCD_ESHAPE otherwise); images == 0 is a no-op.
 * ccd_ctc_loss_fwd, one wavefront per sample, lane s = state s of the extended label sequence:
 *   logits   fp32 [batch * steps, ldl], `classes` valid columns (the columns behind them are never read), class 0 = blank;
 *   targets  int64 [batch, max_len], zero-padded: the label length L is the number of leading non-zero entries (found on the device);
 *   nll      fp32 [batch]: -log p(target | logits), 0 for an infeasible sample: L + adjacent equal labels > steps, a label outside
 *            [1, classes) (never used as an index), or no alignment of finite probability;
 *   acc      fp32 [3] = {sum of nll / max(L, 1) over the feasible samples, batch, infeasible samples}: the loss is acc[0] / acc[1].
 *            Folded by one workgroup in a fixed order, no atomics: the same inputs give the same bits;
 *   ws       ccd_ctc_loss_ws_bytes(batch, steps) bytes, 8-byte aligned: the forward variables, the frames' log-sum-exp and the
 *            per-sample result, read by ccd_ctc_loss_bwd.
 * ccd_ctc_loss_bwd: d_logits bf16 [batch * steps, ldd] = (softmax[t, c] - posterior of class c at frame t) * upstream / (max(L, 1) *
 *   batch), columns classes..ldd-1 and the rows of an infeasible sample zero; upstream = optional device scalar (NULL: 1).  The
 *   posterior of a class is the sum over the states that carry it (the blanks, a repeated character), formed in a fixed order.
 * ccd_ctc_greedy: arg-max class per frame (first maximum), repeats collapsed, blanks dropped -> path int32 [batch, steps]
 *   left-aligned, padded with -1; length int32 [batch]; conf fp32 [batch, steps] = the softmax probability of the first frame of each
 *   kept run, padded with 0.  logits fp32 [batch, steps, classes] with sample / step strides in elements.
 * The recursion runs in the log domain in fp64 (kernels/ctc.h says why); log-sum-exp of nothing is -inf, never NaN.
 * batch == 0 is a no-op.  CCD_EINVAL: a missing pointer, a negative size or stride; CCD_ESHAPE: classes outside
 * 1..CCD_CTC_MAX_CLASSES, steps outside 1..CCD_CTC_MAX_STEPS, max_len > CCD_CTC_MAX_LABELS, ldl or ldd < classes. */
#define CCD_CTC_MAX_STEPS 64
#define CCD_CTC_MAX_CLASSES 128
#define CCD_CTC_MAX_LABELS 31
int ccd_ctc_pool_fwd(const ccd_bf16* tokens, ccd_bf16* frames, int images, int rows, int cols, int E, void* stream);
int ccd_ctc_pool_bwd(const ccd_bf16* d_frames, ccd_bf16* d_tokens, int images, int rows, int cols, int E, void* stream);
long ccd_ctc_loss_ws_bytes(int batch, int steps);
int ccd_ctc_loss_fwd(const float* logits, long ldl, int batch, int steps, int classes, const int64_t* targets, int max_len, float* nll,
                     float* acc, void* ws, void* stream);
int ccd_ctc_loss_bwd(const float* logits, long ldl, int batch, int steps, int classes, const int64_t* targets, int max_len, const void* ws,
                     const float* upstream, ccd_bf16* d_logits, long ldd, void* stream);
int ccd_ctc_greedy(const float* logits, long sample_stride, long step_stride, int batch, int steps, int classes, int* path, int* length,
                   float* conf, void* stream);
/* CTC prefix beam search (ABI 21; kernels/ctc_beam.h, restated in numpy in tests/ctc_beam_np.py), one wavefront per sample:
 *   scores      fp32 [batch, steps, classes], classes contiguous, sample and step strides in elements; class 0 = blank.
 *               normalized = 0: logits, lp = x - max - log sum exp(x - max); normalized = 1: probabilities (CTCDecoder.forward_test),
 *               lp = log p - log sum p, a zero probability gives -inf.  Both in fp64 from the fp32 values, the sum over the classes in
 *               ascending order.  -inf masks a class.
 *   beam        1..CCD_CTC_MAX_BEAM entries.  An entry is a prefix of classes 1..classes-1 with pb / pnb, the log mass of its alignments
 *               ending in the blank / a non-blank; the start is the empty prefix (pb 0, pnb -inf).  Per frame, tot = logaddexp(pb, pnb):
 *               stay: pb' = tot + lp[0], pnb' = pnb + lp[last]; extend by c: pb' = -inf, pnb' = (c == last ? pb : tot) + lp[c]; an
 *               extension that spells a live entry's prefix is log-added into that entry's stay pnb' and disappears.  The `beam` best
 *               candidates of finite score logaddexp(pb', pnb') survive, by score descending, then parent rank * classes + class
 *               ascending (stay = class 0).  fp64 throughout; log-sum-exp of nothing is -inf, never NaN.
 *   paths       int32 [batch, beam, steps] by rank, padded with -1; lengths int32 [batch, beam], -1 for an unused slot (fewer than
 *               `beam` finite candidates: steps = 1, an all -inf frame); hyp_scores fp32 [batch, beam] = logaddexp(pb, pnb) rounded
 *               once, -inf for an unused slot: a lower bound of the word's log CTC probability, exact when nothing was pruned.
 * No atomics: the same input gives the same bits.  batch == 0 is a no-op.  CCD_EINVAL: a missing pointer, a negative size or stride;
 * CCD_ESHAPE: beam outside 1..CCD_CTC_MAX_BEAM, steps outside 1..CCD_CTC_MAX_STEPS, classes outside 2..CCD_CTC_MAX_CLASSES, normalized
 * not 0 or 1.  Nothing is launched on an error. */
#define CCD_CTC_MAX_BEAM 16
int ccd_ctc_beam_search(const float* scores, long sample_stride, long step_stride, int batch, int steps, int classes, int normalized,
                        int beam, int* paths, int* lengths, float* hyp_scores, void* stream);
/* CTC prefix beam search fused with a character n-gram language model (ABI 24; kernels/ctc_beam.h: ctc_beam_kernel<CTC_BEAM_LM>, restated in
 * numpy in tests/ctc_beam_lm_np.py): the open-vocabulary decoder that prefers plausible spellings.  scores, beam and the outputs as
 * ccd_ctc_beam_search; one wavefront per sample.
 *   lm          fp32 [classes^(order-1), classes], row-major, order in 1..CCD_CTC_LM_MAX_ORDER.  The row of a prefix p is built from its
 *               last order - 1 classes, the most recent last, a missing position being 0 (the blank's number: "start of word"):
 *               order 1: row 0; order 2: row p[-1]; order 3: row p[-2] * classes + p[-1].  Column c >= 1: the log-probability of
 *               character c behind that context; column 0: that of the word ending there, read only with eos.  Values are finite or
 *               -inf (NaN is outside the specification); rows need not be normalised.
 *   weight, bonus   fp32.  The term of extending a prefix by c is
 *                   g = lm[row, c] == -inf ? -inf : (double)weight * (double)lm[row, c] + (double)bonus     (the product, then the sum).
 *   Per frame everything is as ccd_ctc_beam_search states it, with one exception: an extend candidate (i, c) has
 *               pnb' = ((c == last_i ? pb_i : tot_i) + lp[c]) + g(i, c), and that same number is what a merge log-adds into entry j's
 *               stay candidate.  Stay candidates, the selection key and the tie rule are unchanged.  pb and pnb of a prefix both carry
 *               Lambda(prefix) = the sum of g over its characters, so a word's score is
 *               log p_ctc(word | kept alignments) + weight * sum lm + bonus * |word|.
 *   eos = 1     behind the last frame every entry's score gets (double)weight * lm[row, 0] (no bonus), -inf where the table entry is
 *               -inf; the entries are ranked again by (score descending, previous rank ascending), and a -inf entry becomes an unused
 *               slot (length -1, score -inf, path all -1).  The term does not steer the pruning.  eos = 0: the last selection's order.
 *   weight 0, bonus 0 and a table without -inf reproduce ccd_ctc_beam_search bit for bit; weight 0 with -inf entries is a hard
 *   character-set constraint.  A score is comparable with ccd_ctc_beam_search's and ccd_ctc_lexicon_score's only after Lambda (and the
 *   eos term) is subtracted.
 * No atomics, no workspace: the same input gives the same bits.  batch == 0 is a no-op.  CCD_EINVAL: a missing pointer (lm included), a
 * negative size or stride; CCD_ESHAPE: everything ccd_ctc_beam_search refuses, order outside 1..CCD_CTC_LM_MAX_ORDER, eos not 0 or 1, a
 * weight or bonus that is not finite.  Nothing is launched on an error. */
#define CCD_CTC_LM_MAX_ORDER 3
int ccd_ctc_beam_search_lm(const float* scores, long sample_stride, long step_stride, int batch, int steps, int classes, int normalized,
                           int beam, const float* lm, int order, float weight, float bonus, int eos,
                           int* paths, int* lengths, float* hyp_scores, void* stream);
/* CTC prefix beam search along a lexicon's prefix tree (ABI 26; kernels/ctc_beam.h: ctc_beam_kernel<CTC_BEAM_TRIE>, restated in numpy in
 * tests/ctc_trie_np.py): the closed-vocabulary proposer whose cost does not grow with the lexicon.  scores, beam, paths, lengths and
 * hyp_scores as ccd_ctc_beam_search; one wavefront per sample.
 *   nodes       int32 [n_nodes, 8], 32 bytes per node, breadth-first: the root is node 0, the children of a node are contiguous in
 *               ascending class order.  Words 0..3: the 128-bit child mask, bit c & 31 of word c >> 5 set iff the node has a child by
 *               class c (bit 0 never); word 4: first_child, the node of the child with the lowest class - the child by class c is
 *               first_child + popcount(mask bits below c); word 5: word_id, the lexicon row that ends here (the lowest of duplicate
 *               rows) or -1; word 6: the parent, -1 for the root; word 7: the class on the edge from the parent, 0 for the root.  The
 *               kernel reads words 0..5.  An empty lexicon is the root alone.
 *   Every beam entry carries a node; the empty prefix carries node 0.  An extend candidate (i, c) exists iff bit c of mask[node_i] is
 *               set - otherwise it is -inf: never selected, never merged - and scores what ccd_ctc_beam_search gives it, with no added
 *               term; the selected extension carries child(node_i, c), a stay keeps the node.  Merges, the selection key and the tie rule
 *               are unchanged.  Prefixes that end no word compete for the beam's slots during the search.
 *   Behind the last frame the score of an entry is logaddexp(pb, pnb) where word_id[node] >= 0 and -inf otherwise; the entries are
 *               ranked again by (score descending, previous rank ascending), and a -inf entry becomes an unused slot (length -1, score
 *               -inf, path all -1, word id -1).  With a narrow beam a sample may end with no word at all.
 *   word_ids    int32 [batch, beam]: word_id of every hypothesis, -1 for an unused slot.  hyp_scores is a lower bound of the word's
 *               ccd_ctc_lexicon_score: the sum over the alignments the beam kept.
 *   Every node id the kernel derives is clamped to [0, n_nodes) before it addresses the table, and mask bits of classes >= `classes`
 *   are never scanned: a malformed table gives wrong words, never an access outside it; a word with a class outside the scores is
 *   unreachable, as it is -inf for ccd_ctc_lexicon_score.
 * No atomics, no workspace: the same input gives the same bits.  batch == 0 is a no-op.  CCD_EINVAL: a missing pointer (nodes and word_ids
 * included), a negative size or stride; CCD_ESHAPE: everything ccd_ctc_beam_search refuses, n_nodes < 1.  Nothing is launched on an error. */
int ccd_ctc_beam_search_trie(const float* scores, long sample_stride, long step_stride, int batch, int steps, int classes, int normalized,
                             int beam, const int* nodes, int n_nodes, int* paths, int* lengths, float* hyp_scores, int* word_ids,
                             void* stream);

/* Lexicon-constrained decoding of the CTC head (ABI 23; kernels/ctc_lexicon.h, restated in numpy in tests/ctc_lexicon_np.py): of THESE
 * words, which is the most probable given the frames, and how probable is each.
 * ccd_ctc_lexicon_score, a workgroup per (sample, strip of 64 words), lane = CTC state with 4 / 2 / 1 words packed into a wave:
 *   scores      fp32 [batch, steps, classes] with sample / step strides in elements, logits (normalized = 0) or probabilities
 *               (normalized = 1): the frame log-probabilities are exactly those of ccd_ctc_beam_search, so a lexicon score and a beam
 *               score of the same word are comparable numbers.
 *   words       int64 [n_words, max_len], zero-padded (the layout of ccd_ctc_loss_fwd's targets): the label length L is the number of
 *               leading non-zero entries, found on the device; an all-zero row is the empty word (the sum of the blanks).
 *   out         fp32 [batch, ld_out]: out[b, v] = log p(words[v] | scores[b]), the log of the summed probability of all alignments of
 *               the word over the frames - the alpha recursion of ccd_ctc_loss_fwd in fp64, rounded once.  -inf where that kernel calls
 *               the target infeasible (a label outside [1, classes) - never used as an index -, L + adjacent equal labels > steps) and
 *               where every alignment meets a masked class; never NaN.
 *   columns     optional int32 [n_words]: word v writes out[b, columns[v]] instead (a column outside [0, ld_out) writes nothing) - a
 *               lexicon split by length class still fills the caller's order.
 *   subset      optional int32 [batch, subset_cols]: sample b scores only words[subset[b, k]] into out[b, k]; an entry < 0 (the
 *               padding of a ragged per-image list) or >= n_words gives -inf.  columns and subset together: CCD_EINVAL.
 *   Lanes per word: the smallest of 16 / 32 / 64 that holds 2 max_len + 1 states - chosen from max_len alone.
 * ccd_ctc_lexicon_best, one wavefront per sample: word_scores fp32 [batch, ld], `cols` valid columns -> index int32 [batch, nbest],
 *   best fp32 [batch, nbest]: the nbest best columns by score descending, then column ascending (a word that appears twice gives two
 *   columns of identical bits, the lower one first).  -inf is never selected; an unused slot has index -1 and score -inf.
 * No atomics: the same input gives the same bits.  No workspace.  batch == 0 or n_words == 0 is a no-op.  CCD_EINVAL: a missing
 * pointer, a negative size or stride, columns with subset; CCD_ESHAPE: steps outside 1..CCD_CTC_MAX_STEPS, classes outside
 * 2..CCD_CTC_MAX_CLASSES, max_len outside 1..CCD_CTC_MAX_LABELS, normalized not 0 or 1, nbest outside 1..CCD_CTC_LEXICON_MAX_NBEST,
 * ld_out < n_words (< subset_cols with subset; not checked with columns), ld < cols.  Nothing is launched on an error. */
#define CCD_CTC_LEXICON_MAX_NBEST 16
int ccd_ctc_lexicon_score(const float* scores, long sample_stride, long step_stride, int batch, int steps, int classes, int normalized,
                          const int64_t* words, int n_words, int max_len, const int* columns, const int* subset, int subset_cols,
                          float* out, long ld_out, void* stream);
int ccd_ctc_lexicon_best(const float* word_scores, long ld, int batch, int cols, int nbest, int* index, float* best, void* stream);

/* CTC forced alignment (ABI 25; kernels/ctc_align.h, restated in numpy in tests/ctc_align_np.py): the best SINGLE alignment of a given
 * word over the frames - the Viterbi / max-plus twin of ccd_ctc_loss_fwd's sum - WHERE its characters sit and how sure the network is of
 * each.  One wavefront per target row, lane s = state s of (blank, l_1, blank, ..., l_L, blank), S = 2 L + 1 <= 63.
 *   scores      fp32 [batch, steps, classes] with sample / step strides in elements, class 0 the blank; logits (normalized = 0) or
 *               probabilities (normalized = 1).  The frame log-probabilities lp are exactly those of ccd_ctc_beam_search (fp64 over the
 *               fp32 row, the sum over the classes in ascending order; a zero probability or a -inf logit masks a class): an alignment
 *               score is comparable with a beam, a lexicon and a loss number of the same word, and never above them.
 *   targets     int64 [n_rows, max_len], zero-padded (ccd_ctc_loss_fwd's layout): the length L is the number of leading non-zero
 *               entries, found on the device.  An all-zero row is the empty word: every frame blank, score = sum lp[t, 0].
 *   rows        optional int32 [n_rows]: row n is aligned against sample rows[n] - the W hypotheses of a beam or the k best words of a
 *               lexicon against one copy of the scores.  NULL: n_rows == batch (CCD_EINVAL otherwise), row n goes with sample n.  An
 *               entry outside [0, batch) makes its row infeasible; it is never used as an index.
 *   Recursion   v_0(s) = lp[0, l'_s] for s < 2, -inf behind; v_t(s) = max(v_{t-1}(s), v_{t-1}(s-1), v_{t-1}(s-2) where the loss allows
 *               that skip) + lp[t, l'_s], in fp64.
 *   Tie rule    (part of the contract: it makes the integers reproducible) the candidates are taken in the order s, s - 1, s - 2 and a
 *               later one replaces the current one only if it is STRICTLY greater; the path ends in state S - 1 unless v(S - 2) is
 *               strictly greater.  With all frames uniform the word `ab` over five frames aligns as a b _ _ _.
 *   frame_char  int32 [n_rows, steps]: the index j of the character emitted at frame t, -1 for a blank frame.
 *   spans       int32 [n_rows, max_len, 2]: first and last frame (inclusive) of character j; -1, -1 for j >= L.  A span is where the
 *               network EMITS the character - CTC is peaky, often one frame -, not the character's inked extent.
 *   char_logp   fp32 [n_rows, max_len]: the sum of lp over the character's frames, added in ascending frame order in fp64; 0 for j >= L.
 *   score       fp32 [n_rows]: the log-probability of the best alignment = the sum of lp over all frames of that path, in frame order.
 *   Infeasible  a label outside [1, classes) (never used as an index), L + adjacent equal labels > steps, no alignment of finite
 *               probability, a bad rows entry: score = -inf, frame_char and spans -1, char_logp 0.
 * No exp or log inside the recursion (logits; the emission of a probability takes its own log, off the dependent chain); backpointers
 * are 2 bits per state and frame in two 64-bit registers of the state's lane: no workspace, no LDS.  No atomics: the same input gives
 * the same bits.  n_rows == 0 is a no-op.  CCD_EINVAL: a missing pointer (scores may be
 * NULL only with batch == 0), a negative size or stride, rows == NULL with n_rows != batch; CCD_ESHAPE: steps outside
 * 1..CCD_CTC_MAX_STEPS, classes outside 1..CCD_CTC_MAX_CLASSES, max_len outside 1..CCD_CTC_MAX_LABELS, normalized not 0 or 1.  Nothing
 * is launched on an error. */
int ccd_ctc_align(const float* scores, long sample_stride, long step_stride, int batch, int steps, int classes, int normalized,
                  const int64_t* targets, int n_rows, int max_len, const int* rows, int* frame_char, int* spans, float* char_logp,
                  float* score, void* stream);

/* Beam search over the NRTR attention decoder (ABI 22; kernels/nrtr_beam.h, restated in numpy in tests/nrtr_beam_np.py).  The decode
 * loop (finetune_engine.beam_decode) runs the incremental decoder on batch * beam rows, row b * beam + r = slot r of sample b, and calls
 * these two at the end of every step.
 * State of a sample, slots ordered by rank:
 *   seq     int64 [batch * beam, seq_len]: the tokens of every slot as ccd_dec_embed_fwd / ccd_dec_attn_fwd read them; position 0 holds
 *           the start token, positions behind the last decoded one the padding token.  Tokens are < 65536.
 *   score   fp64 [batch, beam]: the sum of log_softmax(logits)[token] over the slot's steps; -inf for an unused slot.
 *   state   int32 [batch, beam]: CCD_NRTR_UNUSED (0), CCD_NRTR_LIVE (1), CCD_NRTR_FINISHED (2).
 *   Before step 0: slot 0 live with score 0, the others unused with score -inf; every row of seq = start, padding, padding, ...
 * ccd_nrtr_beam_step, one wavefront per sample, updates the state in place for decoding position `step` (it writes seq[:, step + 1]):
 *   logits  fp32 [batch * beam, ldl >= classes]; only the rows of live slots are read.
 *   A live slot r gives the candidates (r, c), c < classes, of score[r] + log_softmax(logits[r])[c]: fp64 over the fp32 row, the sum
 *   over the classes in ascending order; a -inf logit gives no candidate.  A finished slot gives (r, end_idx) alone: score unchanged,
 *   still finished, pad_idx is the token written.  An unused slot gives none.  The new slots are the `beam` best candidates by score
 *   descending, then r * classes + c ascending; slots left over are unused (score -inf, parent -1, token pad_idx).  Class end_idx
 *   finishes a hypothesis; the end_idx token is written.  A new slot's sequence is its parent's positions 0..step and the new token.
 *   parent  int32 [batch, beam], written: the old slot every new slot continues, -1 for an unused one.
 *   paths / lengths / hyp_scores: all three or none (pass them with the last step); written as ccd_ctc_beam_search writes them from the
 *   new state: paths int32 [batch, beam, seq_len - 1], the classes in front of the first end_idx behind position 0, padded with -1;
 *   lengths int32 [batch, beam], step + 1 for a hypothesis that has not finished, -1 for an unused slot; hyp_scores fp32 [batch, beam],
 *   the score rounded once (the end_idx term included), -inf for an unused slot.
 * ccd_nrtr_beam_reorder permutes the cache of the incremental decoder by `parent`, in place:
 *   cache   bf16 [layers, batch * beam * positions, 3 D], 16-byte aligned, D % 8 == 0: the q | k | v columns of position t of slot r of
 *           sample b in row (b * beam + r) * positions + t.  For every position <= step the K and V columns (D .. 3 D) of slot r become
 *           those slot parent[r] held before the call, whatever cycles or shared parents the permutation has; the Q columns (never read
 *           again) and the positions behind `step` stay.  A slot with parent[r] == r or outside [0, beam) moves nothing.
 * No atomics: the same input gives the same bits.  batch == 0 (or layers == 0) is a no-op.  CCD_EINVAL: a missing pointer, a negative
 * size, stride or step, paths / lengths / hyp_scores given in part, a misaligned cache; CCD_ESHAPE: beam outside 1..CCD_NRTR_MAX_BEAM,
 * classes outside 1..128, ldl < classes, seq_len outside 2..128, step + 2 > seq_len (step >= positions for the reorder), end_idx outside
 * [0, classes), pad_idx outside [0, 65536), D not a positive multiple of 8.  Nothing is launched on an error. */
#define CCD_NRTR_MAX_BEAM 16
#define CCD_NRTR_UNUSED 0
#define CCD_NRTR_LIVE 1
#define CCD_NRTR_FINISHED 2
int ccd_nrtr_beam_step(const float* logits, long ldl, int batch, int beam, int classes, int step, int end_idx, int pad_idx, int64_t* seq,
                       int seq_len, double* score, int* state, int* parent, int* paths, int* lengths, float* hyp_scores, void* stream);
int ccd_nrtr_beam_reorder(ccd_bf16* cache, const int* parent, int layers, int batch, int beam, int positions, int D, int step, void* stream);
/* Beam search over the NRTR decoder along a lexicon's prefix tree (ABI 27; kernels/nrtr_beam.h: nrtr_beam_step_kernel<true>, restated
 * in numpy in tests/nrtr_trie_np.py): ccd_nrtr_beam_step with a trie node per slot.  Everything ccd_nrtr_beam_step takes means what it
 * means there, and a finished or unused slot behaves as it does there.
 *   nodes         int32 [n_nodes, 8]: the table of ccd_ctc_beam_search_trie (the layout is stated there).  Class c of the decoder is
 *                 bit c + class_offset of a node's child mask; class_offset is 1 where the lexicon's rows are class + 1 (the decoder's
 *                 class 0 is a character and the trie never sets bit 0), 0 where they are the classes themselves.
 *   node          int32 [batch, beam], read and written in place like score and state: the node of every slot.  Before step 0: all 0,
 *                 the root (a caller may start a sample at another node).  A value outside [0, n_nodes) is clamped into it.
 *   A live slot r at node n gives the candidate (r, c), c != end_idx, iff c + class_offset <= 127 and that bit of mask[n] is set, and
 *                 (r, end_idx) iff word_id[n] >= 0; every other candidate is -inf: never selected.  The score of an allowed candidate
 *                 is ccd_nrtr_beam_step's - the log-softmax runs over all `classes` and is not renormalised - so the score of a finished
 *                 slot is the exact log p(word <EOS> | image).  The selection key and the tie rule are unchanged.  A sample whose live
 *                 slots have no allowed candidate of finite score ends with unused slots only.
 *   A selected extension carries first_child[n] + popcount(mask[n] bits below c + class_offset), clamped to [0, n_nodes): a malformed
 *                 table gives wrong words, never an access outside it.  A selected end_idx and a carried finished slot keep their node;
 *                 an unused slot's node is 0.
 *   word_ids      int32 [batch, beam], written with paths / lengths / hyp_scores (all four or none): word_id[node] of a finished slot, -1
 *                 for an unused slot and for a slot that is still live - a prefix, no word.
 * No atomics: the same input gives the same bits.  batch == 0 is a no-op.  CCD_EINVAL: a missing pointer (nodes and node included), a
 * negative size, stride or step, paths / lengths / hyp_scores / word_ids given in part; CCD_ESHAPE: everything ccd_nrtr_beam_step
 * refuses, n_nodes < 1, class_offset outside 0..1.  Nothing is launched on an error. */
int ccd_nrtr_beam_step_trie(const float* logits, long ldl, int batch, int beam, int classes, int step, int end_idx, int pad_idx,
                            int64_t* seq, int seq_len, double* score, int* state, int* parent, int* paths, int* lengths,
                            float* hyp_scores, const int* nodes, int n_nodes, int class_offset, int* node, int* word_ids, void* stream);
/* Joint CTC / attention decoding (ABI 29; kernels/nrtr_joint.h, restated in numpy in tests/nrtr_joint_np.py): ccd_nrtr_beam_step whose
 * candidates are rescored with the CTC prefix probability an auxiliary CTC head gives them.  Everything ccd_nrtr_beam_step takes means
 * what it means there; `score` holds the joint score S.
 * ccd_nrtr_joint_begin, once per batch, one wavefront per sample:
 *   frames     fp32, frame t of sample b at frames + b * sample_stride + t * step_stride, ctc_classes dense values: logits, or -
 *              normalized = 1 - probabilities.  Class 0 is the blank.
 *   log_probs  fp64 [batch, ctc_steps, ctc_classes], written: the log-probabilities of every frame, in fp64 with the class sum in
 *              ascending order (-inf for a -inf logit or a probability <= 0).  A workspace the caller owns and hands to every step.
 *   prefix     fp64 [batch, beam, 2, ctc_steps], written: the prefix state of every slot, rn = prefix[b, r, 0], rb = prefix[b, r, 1] - the
 *              log-probability that the frames 0..t spell exactly the slot's prefix and end in a non-blank / in a blank.  Here the
 *              root's: rn = -inf, rb[t] = log_probs[b, 0, 0] + .. + log_probs[b, t, 0], added in that order.
 * ccd_nrtr_beam_step_joint, one wavefront per sample, in place:
 *   att        fp64 [batch, beam], in and out like score: the attention score A of every slot, ccd_nrtr_beam_step's score.  Before step
 *              0 as score: 0, -inf, ..
 *   weight     w in [0, 1].  Decoder class c != end_idx is CTC class k = c + class_offset (class_offset in {0, 1}).
 *   A live slot r with prefix g gives (r, c), c != end_idx: S = (1 - w) (A_r + la[c]) + w psi(g.k), and (r, end_idx): S = (1 - w) (A_r +
 *              la[end_idx]) + w full(g); la = log_softmax(logits[r]) as in ccd_nrtr_beam_step, psi the log-probability that the CTC
 *              output starts with g.k, full that it is g (the recursion: kernels/nrtr_joint.h).  A candidate exists iff its attention
 *              part is finite and (w == 0 or its CTC part > -inf); a class with k >= ctc_classes has no CTC part.  At w == 0 S is the
 *              attention part: the bits of ccd_nrtr_beam_step.  A finished slot gives (r, end_idx) with S and A unchanged.  Selection
 *              and ties are ccd_nrtr_beam_step's, over S.  A selected extension takes the extended prefix state, a finished or carried
 *              slot keeps its parent's, an unused slot holds -inf.
 *   att_scores fp32 [batch, beam], written with paths / lengths / hyp_scores (all four or none): A rounded once, -inf for an unused slot;
 *              hyp_scores is S.
 * No atomics: the same input gives the same bits.  batch == 0 is a no-op.  CCD_EINVAL: a missing pointer, a negative size, stride or
 * step, the four outputs given in part; CCD_ESHAPE: everything ccd_nrtr_beam_step refuses, ctc_steps outside 1..CCD_NRTR_JOINT_MAX_STEPS,
 * ctc_classes outside 1..128, class_offset outside 0..1, weight outside [0, 1] or not finite, normalized not 0 or 1.  Nothing is
 * launched on an error. */
#define CCD_NRTR_JOINT_MAX_STEPS 64
int ccd_nrtr_joint_begin(const float* frames, long sample_stride, long step_stride, int batch, int ctc_steps, int ctc_classes, int normalized,
                         int beam, double* log_probs, double* prefix, void* stream);
int ccd_nrtr_beam_step_joint(const float* logits, long ldl, int batch, int beam, int classes, int step, int end_idx, int pad_idx,
                             int64_t* seq, int seq_len, double* score, int* state, int* parent, int* paths, int* lengths,
                             float* hyp_scores, const double* log_probs, int ctc_steps, int ctc_classes, int class_offset, double weight,
                             double* prefix, double* att, float* att_scores, void* stream);
/* Scoring GIVEN words with the NRTR decoder (ABI 28; kernels/nrtr_score.h, the second kernel restated in numpy in
 * tests/nrtr_score_np.py).  Inference only: no dropout, no mask, no backward.
 *
 * ccd_xattn_rows_fwd: the encoder-decoder attention of `rows` word rows against the keys and values of the sample that owns each row.
 *   q        bf16 [rows * Tq, ldq]: row r holds Tq queries (1 <= Tq <= 32), head h at column 64 h
 *   k, v     bf16 [batch * 256, ldk / ldv]: the 256 image tokens of every sample, head h at column 64 h (ccd_dec_attn_fwd's layout)
 *   row_ptr  int32 [batch + 1], DEVICE memory, CSR: sample b owns the rows row_ptr[b] .. row_ptr[b + 1] - 1; non-decreasing, row_ptr[0]
 *            = 0, row_ptr[batch] = rows; a sample may own none.  The entry point does not read it (the caller, who built it, checks
 *            it); the kernel clamps what it reads into [0, rows], so a malformed table gives wrong results, never an access outside q / out.
 *   max_rows the caller's upper bound on the rows of one sample (<= rows): the grid holds ceil(max_rows / chunk) chunk slots per
 *            (sample, head); a sample with more rows is still computed in full, by workgroups that walk several chunks.
 *   out      bf16 [rows * Tq, ldo]: BIT-EQUAL to ccd_dec_attn_fwd (Tk = 256, no mask, p = 0) on k / v gathered per row.
 *   moments  optional fp32 [rows, heads, Tq, 4]: sum_j p_j x_j, sum_j p_j y_j, sum_j p_j x_j^2, sum_j p_j y_j^2 over the 256 keys, x = j & 31,
 *            y = j >> 5 - the moments of the attention map over the 8 x 32 token grid, p the fp32 probabilities ccd_dec_attn_fwd would
 *            write as `probs`.  Summed in a fixed order, no atomics: |error| <= 23 * 2^-24 * value.
 * ccd_xattn_rows_chunk(rows, heads): the rows of one sample that a workgroup takes, max(1, ceil(rows * heads / (4 * compute units))).  It
 *            sizes the grid and nothing else: results do not depend on it.  Negative on an error.
 * rows == 0, batch == 0 or max_rows == 0 is a no-op.  CCD_EINVAL: a missing or misaligned (16 B) pointer, a negative size, max_rows >
 * rows; CCD_ESHAPE: Tq outside 1..32, a leading dimension that is no multiple of 8 or below 64 * heads.
 *
 * ccd_nrtr_word_score, one wavefront per row: logits fp32 [rows * seq_len, ldl >= classes] of the teacher-forced decoder, seq int64
 * [rows, seq_len] = <BOS> c1 .. cn <EOS> <PAD> .. (the layout of ccd_nrtr_beam_step's seq).  The first end_idx behind position 0 ends the
 * word; n is the number of tokens in front of it.
 *   char_logp fp32 [rows, seq_len - 1]: entry t = log_softmax(logits[r * seq_len + t, :classes])[seq[r, t + 1]] for t = 0 .. n (entry n is
 *             the <EOS>), in fp64 by the routine of ccd_nrtr_beam_step, rounded once; 0 behind it
 *   score     fp32 [rows]: the fp64 sum of those entries in position order, rounded once = log p(word <EOS> | image), the number
 *             ccd_nrtr_beam_step gives the same path
 *   length    int32 [rows]: n
 *   char_pos  fp32 [rows, seq_len - 1, 4], with moments fp32 [rows, heads, seq_len, 4] of ccd_xattn_rows_fwd (both or none): mean_x,
 *             mean_y, std_x, std_y of the head-averaged attention map of position t, in token units (variance clamped at 0); 0 behind
 *             the <EOS>
 *   An INFEASIBLE row - no end_idx behind position 0 (a word longer than seq_len - 2), or one of c1 .. cn outside [0, classes) or equal
 *   to pad_idx - gives score -inf, length -1 and zeros elsewhere; nothing is addressed through such a token.  A -inf logit at a target
 *   gives -inf in char_logp and score, the length stays.
 * rows == 0 is a no-op.  CCD_EINVAL: a missing pointer, moments without char_pos or the reverse, a negative size; CCD_ESHAPE: classes
 * outside 1..128, ldl < classes, seq_len outside 2..128, end_idx outside [0, classes), moments with heads < 1. */
int ccd_xattn_rows_chunk(long rows, int heads);
int ccd_xattn_rows_fwd(const ccd_bf16* q, long ldq, const ccd_bf16* k, long ldk, const ccd_bf16* v, long ldv, const int* row_ptr,
                       ccd_bf16* out, long ldo, float* moments, int rows, int batch, int heads, int Tq, int max_rows, float scale,
                       void* stream);
int ccd_nrtr_word_score(const float* logits, long ldl, int classes, const int64_t* seq, int rows, int seq_len, int end_idx, int pad_idx,
                        const float* moments, int heads, float* char_logp, float* score, int* length, float* char_pos, void* stream);
/* Two-pass decoding (ABI 30; kernels/nrtr_twopass.h, restated in numpy in tests/nrtr_twopass_np.py): the words a CTC decoder proposes
 * become rows of the NRTR decoder's teacher-forced pass and of ccd_ctc_lexicon_score's word table, and the two exact scores rank them
 * again.  One wavefront per image, no workspace, no atomics: the same input gives the same bits.
 * Both take the proposals as ccd_ctc_beam_search returns them: paths int32, slot k of image b at paths + b * sample_stride + k *
 * slot_stride, path_len dense entries, -1-padded CTC classes (class 0, the blank, is never part of a word); lengths int32 [batch, beam],
 * -1 for an unused slot.  CTC class c is decoder class d = c - class_offset (class_offset in {0, 1}).
 * ccd_nrtr_twopass_rows: slot k of image b is ELIGIBLE iff its length n lies in 0..min(path_len, seq_len - 2, max_labels) and every one
 *   of its n classes has c >= 1, 0 <= d < classes, d != end_idx, d != pad_idx.  Row b * beam + k of
 *   seq      int64 [batch * beam, seq_len]: <BOS> d1 .. dn <EOS> <PAD>.. when eligible, <BOS> <PAD>.. when not (ccd_nrtr_word_score reports
 *            that row as -inf, -1).  May be null: the CTC side alone; end_idx and pad_idx may then be -1 (no such class).
 *   targets  int64 [batch * beam, max_labels]: c1 .. cn 0.. when eligible, zeros when not - ccd_ctc_lexicon_score's `words`
 *   subset   int32 [batch, beam]: b * beam + k when eligible, -1 when not - ccd_ctc_lexicon_score's `subset`
 *   The proposals are not trusted: a class is read only in front of a length that fits, and seq holds nothing but start_idx, end_idx,
 *   pad_idx and classes in [0, classes).  The empty word (n = 0) is eligible.
 * ccd_nrtr_twopass_select: att fp32 [batch * beam] (ccd_nrtr_word_score's score of the rows above), ctc fp32 [batch, beam]
 *   (ccd_ctc_lexicon_score's), subset as above.  Slot k is eligible iff subset >= 0, its length lies in 0..min(path_len, max_seq_len) and
 *   att and ctc are both finite.  S = (1 - weight) att + weight ctc in fp64; a term whose weight is exactly 0 is left out.  Rank by (S
 *   descending, slot ascending), ccd_nrtr_beam_step's comparison.  Rank r of image b:
 *   out_paths int32 [batch, beam, max_seq_len] the word in decoder classes, -1-padded; out_lengths int32 [batch, beam]; scores fp32 [batch,
 *   beam] = S rounded once; att_scores, ctc_scores fp32 [batch, beam] its two parts; source int32 [batch, beam] its proposal slot.  A rank
 *   left over holds (-1.., -1, -inf, -inf, -inf, -1).
 * batch == 0 is a no-op.  CCD_EINVAL: a missing pointer, a negative size or stride; CCD_ESHAPE: beam outside 1..CCD_NRTR_MAX_BEAM,
 * path_len outside 1..128, class_offset outside 0..1, classes outside 1..128, seq_len outside 2..128, max_labels outside
 * 1..CCD_CTC_MAX_LABELS, start_idx / end_idx / pad_idx outside [0, 65536) (end_idx, pad_idx: [-1, 65536) without seq), max_seq_len
 * outside 1..128, weight outside [0, 1] or not finite.  Nothing is launched on an error. */
int ccd_nrtr_twopass_rows(const int* paths, long sample_stride, long slot_stride, const int* lengths, int batch, int beam, int path_len,
                          int class_offset, int classes, int start_idx, int end_idx, int pad_idx, int64_t* seq, int seq_len,
                          int64_t* targets, int max_labels, int* subset, void* stream);
int ccd_nrtr_twopass_select(const int* paths, long sample_stride, long slot_stride, const int* lengths, int batch, int beam, int path_len,
                            int class_offset, const float* att, const float* ctc, const int* subset, double weight, int max_seq_len,
                            int* out_paths, int* out_lengths, float* scores, float* att_scores, float* ctc_scores, int* source,
                            void* stream);

/* ---------------------------------------------------------------- DINOHead pieces, vit.py:313,326 */
int ccd_l2norm_fwd(const ccd_bf16* x, ccd_bf16* y, float* inv, int max_rows, const int* d_rows, int rows_mul, int D,
                   void* stream);
int ccd_l2norm_bwd(const ccd_bf16* x, const float* inv, const ccd_bf16* dy, ccd_bf16* dx, int max_rows,
                   const int* d_rows, int rows_mul, int D, void* stream);
int ccd_weightnorm_fwd(const float* v, const float* g, ccd_bf16* w, ccd_bf16* w_t, float* inv, int K, int D,
                       void* stream);
int ccd_weightnorm_bwd(const float* v, const float* g, const float* inv, const float* dw, float* dv, float* dg, int K,
                       int D, void* stream);

/* ---------------------------------------------------------------- DINOLoss, Dino/loss/Dino_loss.py:59-143
 * student/teacher logits fp32 [>=2M, K]; d_m = device M; stats [max_rows,4]; loss_out accumulates the scalar */
int ccd_dino_loss_fwd(const float* s_logits, const float* t_logits, const float* center, int K, const int* d_m,
                      int max_rows, float student_temp, float teacher_temp, float* stats, float* loss_out,
                      void* stream);
int ccd_dino_loss_bwd(const float* s_logits, const float* t_logits, const float* center, int K, const int* d_m,
                      int max_rows, float student_temp, float teacher_temp, const float* stats, float grad_scale,
                      const float* d_grad_scale /* optional device scalar, multiplied in */, ccd_bf16* d_logits,
                      void* stream);
/* The head's last layer AND the distillation loss in one pass, the [2M, K] logits never written (ABI 10; replaces the chain
 * ccd_gemm_nt(EPI_F32) x 2 -> ccd_dino_loss_fwd / _bwd of vision_transformer.py:326-327 + Dino_loss.py:81-105 where D == 256 and
 * K % 512 == 0): logits s = zs . ws^T, t = zt . wt^T are formed tile by tile in registers and folded into per-row online-softmax
 * state; the backward entry recomputes the same tiles and writes the bf16 logit gradient d_logits [>= 2M, K] that the head's
 * weight / data gradient products read.  zs / zt [max_rows, 256] bf16 (L2-normalised rows), ws / wt [K, 256] bf16 (weight-normed
 * last layers), center [K] fp32, d_m = device M, ws_part = workspace of ccd_head_loss_ws_floats(max_rows, K) floats,
 * stats [max_rows, 4] (written by _fwd, read by _bwd; base-2 domain: m_s, 1 / l_s, m_t, 1 / l_t), loss_out accumulates the scalar.
 * CCD_ESHAPE for other shapes: the caller takes the unfused chain. */
long ccd_head_loss_ws_floats(int max_rows, int K);
int ccd_head_loss_fwd(const ccd_bf16* zs, long ld_zs, const ccd_bf16* zt, long ld_zt, const ccd_bf16* ws, long ld_ws,
                      const ccd_bf16* wt, long ld_wt, const float* center, int K, int D, const int* d_m, int max_rows,
                      float student_temp, float teacher_temp, float* ws_part, float* stats, float* loss_out, void* stream);
int ccd_head_loss_bwd(const ccd_bf16* zs, long ld_zs, const ccd_bf16* zt, long ld_zt, const ccd_bf16* ws, long ld_ws,
                      const ccd_bf16* wt, long ld_wt, const float* center, int K, int D, const int* d_m, int max_rows,
                      float student_temp, float teacher_temp, const float* stats, float grad_scale,
                      const float* d_grad_scale /* optional device scalar, multiplied in */, ccd_bf16* d_logits, long ld_d,
                      void* stream);
int ccd_colsum_f32(const float* x, int K, const int* d_rows, int rows_mul, int max_rows, float* out, void* stream);
/* out[k] += sum_d w[k, d] * v[d]  (w [K, D] bf16, D % 256 == 0, v and out fp32).  The teacher centre of Dino_loss.py:133-143 without a
 * pass over the [2M, K] teacher logits: their column sums are (sum of the rows of zn) . W^T - ccd_colsum_bf16 of the l2-normalised
 * bottleneck rows, then this product against the weight-normed last layer (33 MB read instead of 865). */
int ccd_matvec_bf16(const ccd_bf16* w, long ldw, const float* v, int K, int D, float* out, void* stream);
int ccd_center_ema(float* center, const float* batch_sum, int K, const int* d_m, int world, float momentum,
                   void* stream);
/* DINOLoss.sinkhorn_knopp_teacher, Dino_loss.py:157-184 (ABI 19): the SwAV / DINOv2 equal-partition assignment of the teacher logits
 * [max_rows, K] fp32, dense row-major, live rows = rows_mul * d_rows[0] (device side; rows past them are never read).  What the
 * reference returns is softmax_k(t[r, k] / temp + log beta_k) with beta its accumulated prototype scaling; these entries iterate the
 * two scalings in the log domain (x = t / temp, every sum shifted by its maximum: no finite x overflows) and hand the loss kernels
 *   c[k] = -temp * log beta[k],  gauged to mean_k c = 0,
 * which ccd_dino_loss_fwd / _bwd and ccd_head_loss_fwd / _bwd take in place of `center`: softmax((t - c) / temp) IS the assignment.
 * One iteration = colpass -> [all-reduce] -> finish -> rowpass; the last iteration stops at finish (the loss's own softmax scales
 * the rows), so n iterations read the matrix 2n - 1 times.
 *   colpass  col_m[k], col_s[k]: sum_r exp(x[r,k] + log_alpha[r]) = col_s[k] * exp(col_m[k])  (log_alpha NULL: uniform, the first pass).
 *            Strips of CCD_SINKHORN_STRIP columns x chunks of CCD_SINKHORN_ROW_CHUNK rows; the chunks' partial (max, sum) pairs go
 *            through `ws` (ccd_sinkhorn_ws_floats(max_rows, K) floats) and are folded in ascending order: bit-reproducible, no atomics.
 *   rescale  col_s[k] *= exp(col_m[k] - shift[k]), col_m[k] = shift[k]: between ranks, shift = all_reduce(MAX) of col_m, then
 *            all_reduce(SUM) of col_s (the reference's all_reduce of the prototype sums, :174-175); ranks may hold different row counts.
 *   finish   log_beta[k] = -(col_m[k] + log col_s[k]) - mean_k(...), c[k] = -temp * log_beta[k]; either output may be NULL.
 *   rowpass  log_alpha[r] = -log sum_k exp(x[r,k] + log_beta[k])                                     (live rows only)
 *   assign   q[r,k] = softmax_k(x[r,k] + log_beta[k]), the [max_rows, K] assignment itself            (live rows only)
 * Any K >= 1 and any 4-byte aligned pointers; K % 4 == 0 with 16-byte aligned matrices takes 16-byte loads.  CCD_ESHAPE: K, rows_mul,
 * max_rows or temp not positive, max_rows > 65535 * CCD_SINKHORN_ROW_CHUNK. */
#define CCD_SINKHORN_STRIP 1024
#define CCD_SINKHORN_ROW_CHUNK 128
long ccd_sinkhorn_ws_floats(int max_rows, int K);
int ccd_sinkhorn_colpass(const float* logits, int K, const int* d_rows, int rows_mul, int max_rows, float temp, const float* log_alpha,
                         float* ws, float* col_m, float* col_s, void* stream);
int ccd_sinkhorn_rescale(float* col_m, float* col_s, const float* shift, int K, void* stream);
int ccd_sinkhorn_finish(const float* col_m, const float* col_s, int K, float temp, float* log_beta, float* c, void* stream);
int ccd_sinkhorn_rowpass(const float* logits, int K, const int* d_rows, int rows_mul, int max_rows, float temp, const float* log_beta,
                         float* log_alpha, void* stream);
int ccd_sinkhorn_assign(const float* logits, int K, const int* d_rows, int rows_mul, int max_rows, float temp, const float* log_beta,
                        float* q, void* stream);
/* softmax -> cross_entropy (double softmax) of the seg logits [2*half,2,32,128]; d_logits may be NULL */
int ccd_seg_loss(const float* logits, const float* mask_a, const uint8_t* idmap_b, int half, float grad_scale,
                 float* loss_out, float* d_logits, void* stream);
/* The supervised text-segmentation loss of the finetuning task (ccd_amd/loss/seg_loss.py; no reference counterpart: the reference
 * names the task and ships no training code for it).  These three entry points were added WITHOUT raising ccd_abi_version(): they
 * change no existing signature, so every caller of ABI 30 keeps working, and the version is pinned by the two-pass decoder's checks;
 * detect the feature by the presence of the symbols.
 *   logits fp32 [images, 2, H, W]: image and channel strides in elements, the rows of a plane contiguous; base and strides 16-byte
 *          aligned (CCD_EINVAL otherwise)
 *   gt     uint8 [images, H * W], image stride in elements: 0 background, 1 text, ignore_index (2..255) not scored; any other value is
 *          treated as not scored as well and counted in the tail of ws
 * With y = gt, p = sigmoid(z1 - z0), l = -log softmax(z)[y], edge(q) = q is scored and a scored pixel of the other class lies inside
 * the image within the (2 edge_radius + 1)^2 square around q, w = weight[y] (1 + edge_weight edge(q)) (0 where not scored):
 *   Omega = sum w (batch);  CE = sum w l / Omega (0 when Omega = 0: no NaN, unlike F.cross_entropy)
 *   Dice_n = 1 - (2 I + 1) / (P + G + 1), I = sum p y, P = sum p, G = sum y over the scored pixels of image n; Dice = the mean over the
 *   N_v images with a scored pixel (0 when there are none);  L = CE + dice_weight Dice
 * fwd:  loss fp32 [1] = L, parts fp64 [4] = L, CE, Dice, Omega, confusion int64 [2, 2] = the batch's [gt, pred] counts over the scored
 *       pixels (pred = z1 > z0: a tie is class 0, as in ccd_seg_confusion_logits); ws fp64 [ccd_seg_sup_loss_ws_doubles(images)] =
 *       CCD_SEG_SUP_WS_ROW partial sums per image, then Omega, N_v and the number of pixels that are neither 0, 1 nor ignore_index;
 *       code uint8 [images, H * W] (optional, needed by bwd): 0 not scored, 1 background, 2 text, + 4 on the edge band.
 * bwd:  d_logits fp32 [images, 2, H, W] dense = (grad_scale * (d_grad ? d_grad[0] : 1)) dL/dlogits from logits, code and the ws fwd left:
 *       dz1 = w (p - y) / Omega - (dice_weight / N_v) (2 y (P + G + 1) - (2 I + 1)) / (P + G + 1)^2 p (1 - p), dz0 = -dz1, 0 where not scored.
 * One workgroup per image with the gt plane in LDS, one small finishing workgroup, an elementwise backward.  Every sum is fp64 in a fixed
 * order without atomics: results are bitwise repeatable.  CCD_ESHAPE: channels != 2, images < 1, W % 4 != 0, H * W >
 * CCD_SEG_SUP_MAX_PIXELS, edge_radius outside 0..CCD_SEG_SUP_MAX_RADIUS; CCD_EINVAL: a missing pointer, a negative stride or weight, a
 * misaligned operand, ignore_index outside 2..255.  On either nothing is launched. */
#define CCD_SEG_SUP_MAX_PIXELS 8192
#define CCD_SEG_SUP_MAX_RADIUS 4
#define CCD_SEG_SUP_WS_ROW 11
#define CCD_SEG_SUP_WS_TAIL 3
long ccd_seg_sup_loss_ws_doubles(int images);
int ccd_seg_sup_loss_fwd(const float* logits, long image_stride, long channel_stride, int channels, const uint8_t* gt, long gt_stride,
                         int images, int H, int W, int ignore_index, float weight_bg, float weight_text, float dice_weight,
                         float edge_weight, int edge_radius, double* ws, uint8_t* code, float* loss, double* parts, long* confusion,
                         void* stream);
int ccd_seg_sup_loss_bwd(const float* logits, long image_stride, long channel_stride, int channels, const uint8_t* code, int images,
                         int H, int W, float weight_bg, float weight_text, float dice_weight, float edge_weight, const double* ws,
                         float grad_scale, const float* d_grad, float* d_logits, void* stream);

/* ---------------------------------------------------------------- optimiser, train.py:244-272 */
typedef struct ccd_seg_hyper { float lr_wd, step_size, inv_sqrt_bc2, active; } ccd_seg_hyper;
int ccd_seg_sumsq(const float* grad, const int* chunk_seg, const long* chunk_begin, const int* chunk_len, int nchunks,
                  float* norm2, void* stream);
int ccd_adamw(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, ccd_bf16* mirror,
              const int* chunk_seg, const long* chunk_begin, const int* chunk_len, int nchunks,
              const ccd_seg_hyper* hyper, const float* norm2, float clip, float beta1, float beta2, float eps,
              void* stream);
/* torch.optim.SGD(momentum) and the reference's LARS (Dino/modules/utils.py:564-602) behind the same per-tensor clip, over the same
 * chunk tables (ABI 16).  One table row per tensor, read when the kernel runs: lr, the tensor's weight decay, adapt (LARS: 1 = the
 * tensor has ndim != 1, so weight decay and the trust ratio apply) and active (0 = no gradient this iteration: nothing is touched).
 *   d = c g + wd p  (c = the clip coefficient);  LARS, adapt: d *= eta |p| / |d| unless either norm is 0;  LARS, 1-D: d = c g
 *   buf = momentum buf + d;  p -= lr buf;  mirror = bf16(p)
 * ccd_seg_moments: moments[3 s + {0, 1, 2}] += {sum g^2, sum p^2, sum g p} of tensor s (zero the table first), from which ccd_lars
 * forms c and |c g + wd p|^2 = c^2 sum g^2 + 2 c wd sum g p + wd^2 sum p^2.  ccd_sgd_momentum reads ccd_seg_sumsq's norm2 table. */
typedef struct ccd_seg_mom_hyper { float lr, wd, adapt, active; } ccd_seg_mom_hyper;
int ccd_seg_moments(const float* grad, const float* param, const int* chunk_seg, const long* chunk_begin, const int* chunk_len,
                    int nchunks, float* moments, void* stream);
int ccd_sgd_momentum(float* param, const float* grad, float* buf, ccd_bf16* mirror, const int* chunk_seg,
                     const long* chunk_begin, const int* chunk_len, int nchunks, const ccd_seg_mom_hyper* hyper,
                     const float* norm2, float clip, float momentum, void* stream);
int ccd_lars(float* param, const float* grad, float* mu, ccd_bf16* mirror, const int* chunk_seg, const long* chunk_begin,
             const int* chunk_len, int nchunks, const ccd_seg_mom_hyper* hyper, const float* moments, float clip,
             float momentum, float eta, void* stream);
int ccd_clip_scale(float* grad, const int* chunk_seg, const long* chunk_begin, const int* chunk_len, int nchunks,
                   const float* norm2, float clip, void* stream);
/* d_m (optional, device, 2 floats {m, 1 - m}): read at run time instead of the two launch arguments (HIP-graph replays of the step) */
int ccd_ema(float* teacher, const float* student, ccd_bf16* mirror, long n, float m, float one_minus_m, const float* d_m,
            void* stream);

/* ---- segmentation head (Dino/modules/segmentor.py:38-95): channels-last bf16 activations [pixels, C] ----------- */
/* Gather description of an implicit-GEMM convolution: output row r = (n, oy, ox) on a 2^g_h_log2 x 2^g_w_log2 grid;
 * contraction index k = tap*cin + c reads source pixel (oy*s_mul + dy[tap], ox*s_mul + dx[tap]) of an s_h x s_w image
 * (zero outside).  Covers Conv2d 3x3/1x1 forward (segmentor.py:42-45), its data gradient (flipped taps), one output
 * parity class of ConvTranspose2d(4,2,1) (segmentor.py:82,85; c_map scatters row (n,oy,ox) to (n,2oy+c_py,2ox+c_px))
 * and that layer's data gradient (s_mul = 2, 16 taps). */
typedef struct ccd_conv_desc {
    int g_h_log2, g_w_log2, s_h, s_w, s_mul, cin, ntaps;
    signed char dy[16], dx[16];
    int c_map, c_py, c_px;
} ccd_conv_desc;
/* C[rows(->c_map), N] (bf16) = gather(src)[M, ntaps*cin] . W[N, ntaps*cin]^T + bias; optional fp32 column sums /
 * sums of squares of the output (+=) = the BatchNorm batch statistics (replaces F.conv2d / F.conv_transpose2d +
 * the statistics pass of F.batch_norm). */
int ccd_conv_gemm(const ccd_bf16* src, long src_ld, const ccd_conv_desc* desc, const ccd_bf16* W, long ldw, int M, int N,
                  ccd_bf16* C, long ldc, const float* bias, float* colsum, float* colsumsq, void* stream);
/* out[P, ntaps*cin] (fp32) += A[rows, P]^T . gather(src)[rows, ntaps*cin]: the weight gradient of the convolution
 * `desc` describes, contracted over pixels and split over them (fp32 atomics); the patch matrix is never materialised.
 * Conv2d: A = dY, src = layer input.  ConvTranspose2d: A = layer input, src = dY (desc of the data gradient). */
int ccd_conv_wgrad(const ccd_bf16* A, long lda, int P, const ccd_bf16* src, long src_ld, const ccd_conv_desc* desc,
                   long rows, float* out, long ldo, void* stream);
/* cols[rows, ntaps*cin] = gather(src): explicit patch matrix for the weight gradients (TN GEMM operand). */
int ccd_im2col(const ccd_bf16* src, long src_ld, const ccd_conv_desc* desc, long rows, ccd_bf16* cols, void* stream);
/* Train-mode BatchNorm2d + ReLU (segmentor.py:43-44,83-84).  stats = [sum x | sum x^2] over `count` pixels (reduced
 * over ranks by the caller for SyncBatchNorm); finalize writes mean_rstd = [mean | 1/sqrt(var+eps)] and updates the
 * running statistics with torch's rule (unbiased variance). */
int ccd_bn_finalize(const float* stats, float count, float eps, float momentum, float* mean_rstd, float* running_mean,
                    float* running_var, int C, void* stream);
int ccd_bn_relu_fwd(const ccd_bf16* x, long ldx, const float* mean_rstd, const float* gamma, const float* beta,
                    ccd_bf16* y, long ldy, long rows, int C, void* stream);
/* red[0:C] += sum dy*[y>0], red[C:2C] += sum dy*[y>0]*xhat */
int ccd_bn_relu_bwd_reduce(const ccd_bf16* dy, long lddy, const ccd_bf16* x, long ldx, const float* mean_rstd,
                           const float* gamma, const float* beta, float* red, long rows, int C, void* stream);
/* dx = gamma*rstd*(dy*[y>0] - red0/count - xhat*red1/count); dgamma += red_local[C:2C], dbeta += red_local[0:C] */
int ccd_bn_relu_bwd_apply(const ccd_bf16* dy, long lddy, const ccd_bf16* x, long ldx, const float* mean_rstd,
                          const float* gamma, const float* beta, const float* red, float count, const float* red_local,
                          float* dgamma, float* dbeta, ccd_bf16* dx, long lddx, long rows, int C, void* stream);
/* Classifier Conv2d(C, 2, 3, padding=1) (segmentor.py:86) factored through pixel-wise GEMMs:
 *   forward : zT[co*9+tap, q] = sum_c w[co,c,tap] x[q,c] by ccd_gemm_nt (fp32, row stride ldz), then
 *             logits[n,co,y,x] = bias[co] + sum_tap zT[co*9+tap, (n,y+dy,x+dx)]            (ccd_cls_gather_fwd)
 *   backward: g[q, co*9+tap] = dlogits[n,co,(y,x)-(dy,dx)], bf16 [pixels, 64], columns >= 18 zero (ccd_cls_grad_cols);
 *             dx = g . Wd^T (ccd_gemm_nt), dW = g^T . x (ccd_gemm_tn), db = column sums of the centre taps. */
int ccd_cls_gather_fwd(const float* zT, long ldz, const float* bias, float* logits, int images, int H, int W,
                       void* stream);
int ccd_cls_grad_cols(const float* dlogits, ccd_bf16* g, int images, int H, int W, void* stream);
/* Text super-resolution finetuning (ccd_amd/superres.py, kernels/sr.h; no reference counterpart: the reference names the task and
 * ships the metrics, no training code).  These seven entry points were added WITHOUT raising ccd_abi_version(): they change no
 * existing signature, so every caller of ABI 30 keeps working, and the version is pinned by the two-pass decoder's checks; detect the
 * feature by the presence of the symbols.
 * ccd_sr_upsample: lr fp32 [images, 3, h, w] dense -> base fp32 [images, 3, 2h, 2w] = torch's F.interpolate(lr, scale_factor=2,
 *   mode="bicubic", align_corners=False) (A = -0.75, border indices clamped, result not clamped) and xin = (base - mean[c]) / std[c],
 *   one launch, one workgroup per plane.  At x2 the fractions are 0.25 and 0.75 only, whose taps (-27, 225, 67, -9) / 256 are
 *   constants; an interpolation is written around its heaviest tap, so a constant plane comes back bit for bit.
 *   CCD_ESHAPE: w odd, h * w > CCD_SR_MAX_LR_PIXELS; CCD_EINVAL: a missing or misaligned pointer, std <= 0, a NaN.
 * ccd_img_gather_fwd / ccd_img_grad_cols: the 3-channel twins of ccd_cls_gather_fwd / ccd_cls_grad_cols for a head whose last
 *   convolution Conv2d(C, 3, 3, padding=1) writes a residual image: zT rows co*9+tap < 27, g columns co*9+tap < 27 (>= 27 zero);
 *   sr[n,co,y,x] = base[n,co,y,x] + (bias[co] + sum_tap zT[co*9+tap, (n,y+dy,x+dx)]) - zero weights and bias give sr = base bit for bit.
 * The loss, per channel plane x with zero padding (TSRN's gradient map):
 *   g(x) = sqrt((0.5 (x[y,x+1] - x[y,x-1]))^2 + (0.5 (x[y-1,x] - x[y+1,x]))^2 + 1e-6)
 *   mse_n = mean (sr - hr)^2, gp_n = mean |g(sr) - g(hr)| over the 3 H W elements of image n;  L = mean_n (mse_n + gp_weight gp_n)
 * sr, hr fp32 [images, 3, H, W] dense and 16-byte aligned, H <= CCD_SR_MAX_H, W <= CCD_SR_MAX_W, W % 4 == 0, any number of images.
 * fwd:  one workgroup per plane (both planes in LDS) -> ws fp64 [ccd_sr_loss_ws_doubles(images)] = (sum of squared errors, sum of
 *       gradient-map errors) per plane; one finishing workgroup -> per_image fp64 [images, 2] = mse_n, gp_n, loss fp32 [1] = L,
 *       parts fp64 [3] = L, mean mse_n, mean gp_n.  images == 0: L = 0, ws and per_image may be NULL.
 * bwd:  d_sr fp32 [images, 3, H, W] = (grad_scale * (d_grad ? d_grad[0] : 1) / (images 3 H W)) [2 (sr - hr) + gp_weight * the four
 *       neighbour terms 0.25 sign(g(sr) - g(hr)) (difference) / g(sr) of the pixels whose stencil contains the pixel], sign(0) = 0;
 *       a gather from the LDS planes, reads no ws.  images == 0: nothing to write.
 * The stencil terms and every sum are fp64, in a fixed order (the images fold as a tree of fixed shape) without atomics: results are
 * bitwise repeatable.  CCD_ESHAPE: H, W outside the limits, W % 4 != 0, images < 0; CCD_EINVAL: a missing or misaligned pointer, a
 * negative or NaN gp_weight.  On either nothing is launched. */
#define CCD_SR_MAX_LR_PIXELS 2048
#define CCD_SR_MAX_H 32
#define CCD_SR_MAX_W 128
#define CCD_SR_WS_IMAGE 6
int ccd_sr_upsample(const float* lr, int images, int h, int w, float mean0, float mean1, float mean2, float std0, float std1,
                    float std2, float* base, float* xin, void* stream);
int ccd_img_gather_fwd(const float* zT, long ldz, const float* bias, const float* base, float* sr, int images, int H, int W,
                       void* stream);
int ccd_img_grad_cols(const float* d_sr, ccd_bf16* g, int images, int H, int W, void* stream);
long ccd_sr_loss_ws_doubles(int images);
int ccd_sr_loss_fwd(const float* sr, const float* hr, int images, int H, int W, float gp_weight, double* ws, double* per_image,
                    float* loss, double* parts, void* stream);
int ccd_sr_loss_bwd(const float* sr, const float* hr, int images, int H, int W, float gp_weight, float grad_scale, const float* d_grad,
                    float* d_sr, void* stream);
/* The same tail - unpool2's BatchNorm2d + ReLU, then `cls` (segmentor.py:84-95) - FUSED for the reference's own head shape
 * (C = 128 channels, H x W = 32 x 128 pixels per image, 2 classes; anything else: CCD_ESHAPE, take the kernels above).
 * y: the transposed conv's output before its BatchNorm, bf16 [images*H*W, ldy]; w: cls.weight fp32 [2, C, 3, 3] (the
 * parameter itself, no re-laid operand); relu(bn(y)) is never materialised (kernels/cls_tail.h).
 *   ccd_cls_tail_fwd        : logits fp32 [images, 2, H, W] = cls(relu(bn(y)))
 *   ccd_cls_tail_bwd_reduce : red[0:C] += sum d*[a>0], red[C:2C] += sum d*[a>0]*xhat with d = d(a) of cls computed on
 *                             the fly from dlogits fp32 [images, 2, H, W]; db_cls[2] += sum dlogits
 *   ccd_cls_tail_bwd_apply  : dy bf16 [images*H*W, lddy] = gamma*rstd*(d*[a>0] - red0/count - xhat*red1/count)  (red: summed
 *                             over the ranks by the caller); dgamma += red_local[C:2C], dbeta += red_local[0:C];
 *                             dbias_t[C] += column sums of dy (the transposed conv's bias gradient);
 *                             dw_cls fp32 [2, C, 3, 3] += sum_pixels g (x) a                                              */
int ccd_cls_tail_fwd(const ccd_bf16* y, long ldy, const float* mean_rstd, const float* gamma, const float* beta,
                     const float* w, const float* bias, float* logits, int images, int H, int W, int C, void* stream);
int ccd_cls_tail_bwd_reduce(const float* dlogits, const ccd_bf16* y, long ldy, const float* mean_rstd, const float* gamma,
                            const float* beta, const float* w, float* red, float* db_cls, int images, int H, int W, int C,
                            void* stream);
int ccd_cls_tail_bwd_apply(const float* dlogits, const ccd_bf16* y, long ldy, const float* mean_rstd, const float* gamma,
                           const float* beta, const float* w, const float* red, float count, const float* red_local,
                           float* dgamma, float* dbeta, float* dw_cls, float* dbias_t, ccd_bf16* dy, long lddy, int images,
                           int H, int W, int C, void* stream);
/* dst[sum_i idx_i*dst_strides[i]] <- src[sum_i idx_i*src_strides[i]] over dims[4] (host arrays); accumulate = 0: dst
 * is bf16 (cast), accumulate = 1: dst is fp32 and += (conv weights <-> GEMM operand layouts, weight gradients back). */
int ccd_permute4(const float* src, const long* src_strides, const long* dst_strides, const int* dims, void* dst,
                 int accumulate, void* stream);

/* Several re-layouts / BatchNorm finalisations in ONE launch (the segmentation head issued 27 + 16 launches of ~5 us per step for
 * them).  jobs: host array, n <= 24 (permute) / n <= 4 (finalize; the layers of one level, whose statistics arrive together).
 * ccd_bn_finalize_multi also adds 1 to *batches (nn.BatchNorm2d.num_batches_tracked, int64 on the device) where given. */
typedef struct { const float* src; void* dst; long src_strides[4]; long dst_strides[4]; int dims[4]; } ccd_permute4_job;
int ccd_permute4_multi(const ccd_permute4_job* jobs, int n, int accumulate, void* stream);
typedef struct {
    const float* stats; float* mean_rstd; float* running_mean; float* running_var; long* batches;
    float count, eps, momentum; int C;
} ccd_bn_finalize_job;
int ccd_bn_finalize_multi(const ccd_bn_finalize_job* jobs, int n, void* stream);

/* ---- finetune path: DINO_Finetune = ViT encoder + Mlp + NRTR decoder + TFLoss ---------------
 * Reference: Dino/model/dino_vision.py:134-246, Dino/decoder/nrtr_decoder.py:92-170, transformer_module.py:8-97,
 * transformer_layers.py:150-163, Dino/loss/ce_loss.py:94-128, train_finetune.py:262-289.  The Linear layers run on
 * ccd_gemm_nt / ccd_gemm_tn, the LayerNorms on ccd_ln_fwd / ccd_ln_bwd. */
/* nn.Dropout(p) without a mask tensor: element i is kept iff hash(seed, i) >= p * 2^32 and scaled by 1/(1-p); the
 * backward pass calls the same function on the gradient with the same seed.  dst = (resid ? resid : 0) + drop(src).
 * src / dst: fp32 or bf16 (flags), resid fp32 or NULL; n % 4 == 0; dst may alias src. */
int ccd_dropout(const void* src, int src_bf16, const float* resid, void* dst, int dst_bf16, long n, uint64_t seed, float p,
                void* stream);
/* DropPath scales of one backbone pass (vision_transformer.py:27-35,107-113): out[blk*per_block + j] = keep_j / keep[blk]
 * with keep_j ~ Bernoulli(keep[blk]) from the same counter-based generator (keep: device array [nblocks]). */
/* d_seed (optional, device): added to `seed` at run time (HIP-graph replays draw new masks) */
int ccd_droppath_scales(const float* keep, float* out, int per_block, int nblocks, uint64_t seed, const uint64_t* d_seed,
                        void* stream);
/* x[r,:] = dropout(trg_word_emb[tokens[r]] + position_table[r % T])   (nrtr_decoder.py:93-95); D % 4 == 0 */
int ccd_dec_embed_fwd(const int64_t* tokens, const float* emb, const float* pos, float* x, int rows, int T, int D,
                      int num_classes, uint64_t seed, float p, void* stream);
/* demb[c,:] += sum_{r: tokens[r]==c} drop(dx[r,:]) for c != padding_idx (nn.Embedding(padding_idx)); D <= 1024 */
int ccd_dec_embed_bwd(const int64_t* tokens, const float* dx, float* demb, int rows, int D, int num_classes, int padding_idx,
                      uint64_t seed, float p, void* stream);
/* MultiHeadAttention core (transformer_module.py:22-32, 84-92) for Tq <= 32 queries, Tk <= 256 keys, d_k = d_v = 64:
 *   out[b*Tq+t, 64h:64h+64] = dropout(softmax(mask(scale * q.k^T))) . v      lse[b,h,t] saved for the backward pass
 * q rows b*Tq+t (stride ldq), k / v rows b*Tk+j (strides ldk / ldv), head h at column 64h of each.  Mask: key j is
 * hidden from query t if causal && j > t, if tokens && tokens[b,j] == pad_idx (get_pad_mask & get_subsequent_mask,
 * nrtr_decoder.py:77-90), or if key_len && j >= key_len[b] (_get_mask :113-127).  probs (optional, fp32
 * [B,H,Tq,Tk]) receives the attention weights after dropout - what MultiHeadAttention returns as `attn`. */
int ccd_dec_attn_fwd(const ccd_bf16* q, long ldq, const ccd_bf16* k, long ldk, const ccd_bf16* v, long ldv, ccd_bf16* out,
                     long ldo, float* lse, float* probs, const int64_t* tokens, const int* key_len, int pad_idx, int causal,
                     int B, int H, int Tq, int Tk, float scale, uint64_t seed, float p, void* stream);
int ccd_dec_attn_bwd(const ccd_bf16* q, long ldq, const ccd_bf16* k, long ldk, const ccd_bf16* v, long ldv,
                     const ccd_bf16* out, const ccd_bf16* d_out, long ldo, const float* lse, const int64_t* tokens,
                     const int* key_len, int pad_idx, int causal, int B, int H, int Tq, int Tk, float scale, uint64_t seed,
                     float p, ccd_bf16* dq, long lddq, ccd_bf16* dk, long lddk, ccd_bf16* dv, long lddv, void* stream);
/* TFLoss (ce_loss.py:94-128): rows r = (b,t) of logits [B*T, ldl] (C <= 128 classes) against targets[b,t+1]; rows with
 * t == T-1 or target == pad_idx do not count.  fwd: acc[0] = sum of -log softmax[target], acc[1] = count (acc is
 * cleared first), row_lse[r] saved; the loss is acc[0]/acc[1].  bwd: d_logits (bf16 [B*T, ldd], zero beyond C) =
 * (softmax - onehot) * upstream[0] / count (upstream: device scalar, NULL = 1). */
int ccd_tf_loss_fwd(const float* logits, long ldl, int C, const int64_t* targets, int rows, int T, int pad_idx,
                    float* row_lse, float* acc, void* stream);
int ccd_tf_loss_bwd(const float* logits, long ldl, int C, const int64_t* targets, int rows, int T, int pad_idx,
                    const float* row_lse, const float* acc, const float* upstream, ccd_bf16* d_logits, long ldd, void* stream);
/* One greedy decoding position (nrtr_decoder.py:160-168): probs[b,step,:] = softmax(logits[b,:C]),
 * seq[b,step+1] = argmax (first maximum). */
int ccd_greedy_step(const float* logits, long ldl, int C, int B, float* probs, int steps, int step, int64_t* seq,
                    int seq_len, void* stream);
/* Parallel (position) attention recognition head (Dino/modules/attention.py:5-30, kernels/posattn.h), per image n of 256 tokens:
 *   M = tanh(P + Q0)   A[s, t] = be[t] + sum_e M[s, e] We[t, e]   attn[n, t, :] = softmax over the tokens s   G[t, :] = sum_s attn[t, s] X[s, :]
 * P = X Wv^T + bv and X are bf16 2-D views [N * 256, E] with row strides ldp / ldx (multiples of 8, >= E, 16-byte aligned rows),
 * Q0 bf16 [256, E] and We bf16 [32, E] (rows T.. zero) dense, be fp32 [T].  tokens must be 256, E a multiple of 64 up to 768,
 * 1 <= T <= 32: anything else is CCD_ESHAPE before any launch; N = 0 returns without a launch.
 * ccd_posattn_fwd writes attn fp32 [N, T, 256] and G bf16 [N * 32, E] (row stride ldg; rows T..31 of every image zero).
 * ccd_posattn_bwd: given dG (bf16 [N * 32, E], row stride lddg; rows T.. are not read) writes dX1[s, :] = sum_t attn[t, s] dG[t, :] and
 *   dP = dM (1 - M^2), dM[s, :] = sum_t dA[s, t] We[t, :], dA[s, t] = attn[t, s] (da[t, s] - sum_s' attn[t, s'] da[t, s']), da = dG X^T
 *   (bf16 [N * 256, E] views, row strides lddx / lddp), and this image's fp32 partials dWe_part [N, 32, E] = dA^T M, dbe_part [N, 32].
 * ccd_posattn_fold sums over the images in a fixed order: dQ0 fp32 [256, E] = sum_n dP_n, dWe fp32 [32, E], dbe fp32 [32] (all
 *   overwritten; zeros for N = 0).  No atomics in any of the three: two runs give the same bits. */
int ccd_posattn_fwd(const ccd_bf16* P, long ldp, const ccd_bf16* X, long ldx, const ccd_bf16* Q0, const ccd_bf16* We, const float* be,
                    float* attn, ccd_bf16* G, long ldg, int N, int tokens, int E, int T, void* stream);
int ccd_posattn_bwd(const ccd_bf16* dG, long lddg, const ccd_bf16* X, long ldx, const ccd_bf16* P, long ldp, const ccd_bf16* Q0,
                    const ccd_bf16* We, const float* attn, ccd_bf16* dX1, long lddx, ccd_bf16* dP, long lddp, float* dWe_part,
                    float* dbe_part, int N, int tokens, int E, int T, void* stream);
int ccd_posattn_fold(const ccd_bf16* dP, long lddp, const float* dWe_part, const float* dbe_part, float* dQ0, float* dWe, float* dbe,
                     int N, int E, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CCD_HIP_H */
