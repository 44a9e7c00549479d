/*
 * m3p_hip.h — C ABI of libm3p_hip.so: the MI355X (gfx950) kernels behind M3P's
 * pre-training hot path (TransformerModel.jointfwd / predict, Adam, clip).
 *
 * The reference (microsoft/M3P) has no native code: every entry point below replaces
 * a chain of ATen ops launched from Python at the cited reference file:line
 * (paths relative to the reference checkout).  INTEGRATION.md shows the ctypes binding
 * a reference maintainer would add.
 *
 * Conventions (all entry points):
 *   - extern "C", plain pointers + sizes, no torch / C++ types in any signature;
 *   - every pointer is DEVICE memory owned by the caller (no ownership transfer, the
 *     library never allocates); activations are bf16 unless noted, parameters and
 *     parameter gradients are fp32 ("master" precision), statistics fp32;
 *   - `stream` is a hipStream_t passed as void*; kernels are enqueued asynchronously;
 *   - return value: 0 = enqueued OK; <0 = M3P_E* (bad shape / alignment, nothing was
 *     launched); >0 = a hipError_t.  Nothing throws across the ABI;
 *   - the library never allocates and keeps no per-call state: re-entrant (the autograd engine calls from its
 *     own thread).  What IS process-global: idempotent one-time initialisation (the CU count, the dynamic-LDS
 *     attribute of each kernel), the two schedule setters m3p_set_persistent_grid / m3p_set_tile_queue and the developer
 *     switches m3p_debug_set_variant / m3p_debug_attn_variant (tests and A/B tools; never called by the product).
 */
#ifndef M3P_HIP_H
#define M3P_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define M3P_API __attribute__((visibility("default")))

#define M3P_OK 0
#define M3P_EINVAL (-1)
#define M3P_ENOTIMPL (-2)
#define M3P_ENOMEM (-3)   /* an internal scratch allocation failed */

/* library / build identification: returns a static string "m3p_hip <ver> gfx950" */
M3P_API const char* m3p_version(void);

/* ------------------------------------------------------------------------------------
 * Dense contractions on MFMA (v_mfma_f32_16x16x32_bf16), fp32 accumulate.
 * ---------------------------------------------------------------------------------- */

/* epilogue selectors for m3p_gemm_nt_bf16 */
enum {
  M3P_EPI_NONE = 0,          /* C = alpha*acc                                            */
  M3P_EPI_BIAS = 1,          /* C = alpha*acc + bias[n]; cols n < scale_cols are *= scale */
  M3P_EPI_BIAS_GELU = 2,     /* u = acc + bias -> out2 (bf16); C = gelu_erf(u)           */
  M3P_EPI_BIAS_DROP_RES = 3, /* C = dropout(acc + bias) + aux                            */
  M3P_EPI_RES = 4,           /* C = alpha*acc + aux                                      */
  M3P_EPI_DGELU = 5,         /* C = acc * gelu_erf'(aux); colsum[n] += sum_m C (optional) */
  M3P_EPI_MUL = 6,           /* C = acc * aux;            colsum[n] += sum_m C (optional) */
  /* round 4 - the three below run on the eight-wave 256 x 256 kernel only: M, N multiples of 256, M >= 1024, N >= 512,
   * K % 64 == 0, 16-byte aligned bases; anything else returns M3P_EINVAL */
  M3P_EPI_MULQ = 7,          /* C = acc * decode(aux); colsum[n] += sum_m C (optional).  aux = uint8 [M * N]: the one-byte
                                gelu_erf' codes of this [M, N] in the GEMM's fragment order (written by M3P_EPI_BIAS_GELUQ
                                or m3p_gelu_fwd_gq): the FFN data gradient through GELU, autograd of transformer.py:223-225 */
  M3P_EPI_BIAS_GELUQ = 8,    /* u = acc + bias (fp32, NOT stored); C = gelu_erf(u); out2 = uint8 [M * N]: gelu_erf'(u) as one-byte
                                codes in the fragment order M3P_EPI_MULQ reads (bias required): the FFN's lin1 + activation of
                                transformer.py:223 (gelu :48-56) with what backward needs of u kept in a byte */
  M3P_EPI_BIAS_LSE = 9       /* C = acc + bias (M3P_EPI_BIAS without alpha / column scale) and, for the cross-entropy over the
                                N columns (PredLayer, transformer.py:104-117): out2 = float2 [N / 64][M], the (maximum, sum of
                                exp(x - maximum)) of every row over each 64-column block, columns >= ld_out2 (= V, the valid
                                vocabulary) left out; m3p_ce_lse_from_blocks folds them into the rows' log-sum-exp.
                                With M3PEpilogue::row_ref set, the shifted-exponential form: C = bf16(exp(acc + bias - c_n)) with
                                an exact 0 at the target column y_n and at the columns >= ld_out2, out2 = float [N / 64][M], the
                                fp32 sum of the rounded values of every 64-column block (m3p_ce_shift_* below) */
};

typedef struct M3PEpilogue {
  const float* bias;  /* [N] fp32 or NULL                                             */
  const void* aux;    /* bf16 [M, ld_aux]: residual (DROP_RES, RES) / pre-activation (DGELU); uint8 codes (MULQ) */
  void* out2;         /* bf16 [M, ld_out2]: pre-activation output (BIAS_GELU); uint8 codes (BIAS_GELUQ); float2 block
                         statistics (BIAS_LSE, with ld_out2 = the number of valid columns)    */
  float* colsum;      /* fp32 [N] accumulated with atomics, or NULL (DGELU)            */
  int32_t ld_aux;
  int32_t ld_out2;
  int32_t scale_cols; /* BIAS: number of leading output columns multiplied by `scale`   */
  float scale;
  float alpha;        /* accumulator multiplier (NONE, BIAS, RES); 0 is treated as 1    */
  uint32_t seed;      /* dropout stream key (DROP_RES)                                 */
  uint32_t thresh24;  /* round(p * 2^24); 0 = no dropout.  Element i of a stream is dropped iff the low (i even) / high (i odd)
                         16 bits of hash32(i >> 1, seed) are < thresh24 >> 8 (csrc/common.hpp; NumPy twin m3p_amd/rng.py)  */
  float inv_keep;     /* 1 / (1 - p)                                                   */
  const float* descale_a;  /* m3p_gemm_nt_fp8 only: device scalars, the accumulators are multiplied by    */
  const float* descale_b;  /* (*descale_a) * (*descale_b) (NULL = 1) before the epilogue                  */
  /* round 6 - BIAS_GELUQ and MULQ only: the epilogue also leaves an 8-BIT COPY of C for the fp8 product that consumes it
   * (lin2 forward reads gelu(u), the dx1 data gradient reads dU): out8 [M, ld_out8] bytes, row-major,
   * = sat(C_fp32 * (*scale8)) in e4m3 (out8_bf8 = 0) or e5m2 (1), and *amax8 is raised to max |C| (atomic max; the
   * caller zeroes it) - what m3p_quant_fp8 would make of C in a pass of its own.  NULL = no copy.  ld_out8 % 16 == 0,
   * 16-byte aligned base.  BIAS_GELUQ (an activation) takes out8_bf8 = 0 only, MULQ (a gradient) out8_bf8 = 1 only. */
  void* out8;
  const float* scale8;
  float* amax8;
  int32_t ld_out8;
  int32_t out8_bf8;
  /* BIAS_DROP_RES on a row subset: rng_rows[m] (int32 [M], device) is the number row m of this launch has in the full
   * tensor the dropout stream is indexed by - the keep decision of element (m, n) is that of element rng_rows[m] * N + n,
   * so a launch over gathered rows drops exactly what the launch over all rows drops there.  NULL = m itself. */
  const int32_t* rng_rows;
  /* BIAS_LSE, shifted-exponential form: row_ref[m] = {float c_m, int32 y_m} (8 bytes per row, device, 8-byte aligned; written
   * by m3p_ce_shift_target): the shift subtracted from row m's logits before the exponential and the column left out of
   * it.  NULL = the plain form (logits and (maximum, sum) pairs). */
  const void* row_ref;
} M3PEpilogue;

/* C[M,N] (bf16, row pitch ldc) = epilogue( A[M,K] (bf16, pitch lda) x W[N,K]^T (bf16, pitch ldw) ).
 * The nn.Linear shape: replaces F.linear at transformer.py:178-181 (q/k/v_lin as one
 * N=3d GEMM), :208 (out_lin), :223/:225 (FFN lin1/lin2, with :56 gelu and :226 dropout
 * and the residual adds of :951-957 folded into the epilogue), :257 (region
 * projection), :111 (tied vocabulary projection) and, with transposed weight copies,
 * every data-gradient GEMM of their backward.
 * Requires K % 64 == 0, lda/ldw % 8 == 0, ldc % 4 == 0, 16-byte aligned bases. */
M3P_API int m3p_gemm_nt_bf16(const void* A, int lda, const void* W, int ldw, void* C, int ldc,
                             int M, int N, int K, int epilogue, const M3PEpilogue* ep, void* stream);

/* The same contraction with 8-bit operands on the K = 128 MFMA (BASELINE configs[3], "fp8 MFMA GEMMs"):
 * C[M,N] (bf16) = epilogue( (*ep->descale_a) * (*ep->descale_b) * A8[M,K] x W8[N,K]^T ), fp32 accumulate.
 * A8: OCP fp8 e4m3, or bf8 e5m2 when a_is_bf8 (gradients); W8: fp8 e4m3; row pitches lda / ldw in BYTES.
 * Operands come from m3p_quant_fp8 (per-tensor scale, delayed: m3p_amd/fp8.py).  Epilogues NONE, BIAS, BIAS_DROP_RES,
 * RES, DGELU.  Requires M % 256 == 0, N % 256 == 0, K % 128 == 0, lda/ldw % 16 == 0, ldc % 8 == 0, 16-byte bases. */
M3P_API int m3p_gemm_nt_fp8(const void* A8, int lda, int a_is_bf8, const void* W8, int ldw, void* C, int ldc,
                            int M, int N, int K, int epilogue, const M3PEpilogue* ep, void* stream);

/* Per-tensor quantisation for the above: dst[r, c] (8-bit, pitch ld_dst bytes) = sat(src[r, c] * (*scale)) for a bf16
 * matrix [rows, cols] (pitch ld_src elements), format e4m3 (bf8 = 0, saturates at +-448) or e5m2 (bf8 = 1, +-57344),
 * round to nearest even; *amax (fp32, device) is raised to max |src| (atomic max over the launch; the caller zeroes it).
 * scale NULL = 1.  cols % 8 == 0, ld_src % 8 == 0, ld_dst % 8 == 0. */
M3P_API int m3p_quant_fp8(const void* src, int ld_src, void* dst, int ld_dst, int rows, int cols, const float* scale,
                          float* amax, int bf8, void* stream);

/* The same for many contiguous matrices in one launch (the layers' weights, once per optimizer step): desc = n_desc rows
 * of five int64 {src bf16*, dst uint8*, const float* scale, float* amax or 0, elements / 8}, device memory; e4m3. */
M3P_API int m3p_quant_fp8_batch(const long long* desc, int n_desc, int blocks_per_matrix, void* stream);

/* Stream-K variant with fp32 accumulate output: Cf[M,N] (fp32, pitch ldc) += alpha * A Wᵀ.
 * For few-tile / very-long-K problems — the data gradient of the tied vocabulary
 * projection (autograd of transformer.py:111: M = n_pred, N = d, K = V_pad). */
M3P_API int m3p_gemm_nt_streamk_f32(const void* A, int lda, const void* W, int ldw, float* C, int ldc,
                                    int M, int N, int K, float alpha, void* stream);
/* Same with the second operand given as W[K, N] (row = contraction index): Cf += alpha * A W.
 * This is how the vocabulary data gradient dH = dlogits . E reads the embedding matrix E[V, d]
 * in place (no transposed copy).  K may exceed the number of valid rows of W (V padded to a
 * multiple of 64): rows >= k_valid are not read - the matching columns of A must be zeros. */
M3P_API int m3p_gemm_nn_streamk_f32(const void* A, int lda, const void* W, int ldw, int k_valid, float* C,
                                    int ldc, int M, int N, int K, float alpha, void* stream);
/* The same product for whole-tile shapes on the four-wave kernel (round 4): Cf[M,N] (fp32) += alpha * A[M,K] x W[K,N], A read as
 * an NT activation panel (K contiguous), W through transposing LDS reads, (tile, K-chunk) segments dealt to the CUs, partial
 * tiles folded through the caller's weight-gradient workspace (m3p_gemm_wgrad_workspace_bytes) - no atomics.  ALL K rows of W
 * are read (unlike k_valid above): where A holds zero columns, W must still hold finite numbers.  M % 256 == 0, N % 256 == 0,
 * K % 64 == 0, K >= 4096, lda / ldw % 8 == 0; anything else returns M3P_ENOTIMPL (use the stream-K form). */
M3P_API int m3p_gemm_nn_w4_f32(const void* A, int lda, const void* W, int ldw, float* C, int ldc, int M, int N, int K, float alpha,
                               void* workspace, size_t workspace_bytes, void* stream);

/* Weight gradient: dW[N,K] (fp32, pitch lddw) += alpha * sum_m dY[m,n] * X[m,k]
 * (dY bf16 [M,N] pitch lddy, X bf16 [M,K] pitch ldx).  Accumulates with fp32 atomics
 * (split over M to fill 256 CUs), so dW must hold the running gradient (zero after
 * zero_grad).  Replaces autograd's addmm-backward for every nn.Linear weight above.
 * Requires N % 16 == 0 ... see source; lddy/ldx % 8 == 0.
 * workspace (optional, device memory, 16-byte aligned, >= m3p_gemm_wgrad_workspace_bytes()): scratch for the
 * four-wave kernel's partial tiles (one 256-KB slot per CU, folded into dW by a reduce kernel in slot order, no atomics:
 * bit-reproducible).  It belongs to the caller - the library never allocates - and must not be shared by launches that can
 * run concurrently (different streams).  NULL: partial tiles are added to dW with atomics instead.
 * (Round 5 built the reduction INTO the launch - write-through partials, an arrival counter per tile, every chunk's
 * workgroup summing a 1/C stripe in slot order - correct and slower: DESIGN.md section 4, profiles/r05_wgrad_inkernel_*.) */
M3P_API size_t m3p_gemm_wgrad_workspace_bytes(void);
M3P_API int m3p_gemm_wgrad_bf16(const void* dY, int lddy, const void* X, int ldx, float* dW, int lddw,
                                int M, int N, int K, float alpha, void* workspace, size_t workspace_bytes,
                                void* stream);
/* The same product STORED instead of accumulated: dW = alpha * dY^T X, for a gradient the caller knows to be all zeros (the
 * first product of a step into it).  Only for shapes the four-wave kernel deals out as whole tiles (N, K multiples of 256,
 * M % 64 == 0, more 256 x 256 tiles than persistent workgroups - the tied vocabulary matrix, autograd of transformer.py:111): every tile
 * is then flushed exactly once and a plain store replaces 4-byte atomic read-modify-writes of a 768-MB matrix no cache holds.
 * Anything else returns M3P_ENOTIMPL and the caller accumulates with m3p_gemm_wgrad_bf16. */
M3P_API int m3p_gemm_wgrad_store_bf16(const void* dY, int lddy, const void* X, int ldx, float* dW, int lddw, int M, int N, int K,
                                      float alpha, void* workspace, size_t workspace_bytes, void* stream);
/* The whole-tile product (stored: store != 0, or accumulated) that also leaves the weighted column sums of its first operand,
 * bsum[i] = sum_m w[m] dY[m, i] (w fp32 [M], bsum fp32 [N], every element written once with a plain store): the output-bias
 * gradient of the vocabulary projection from the fragments the K loop already holds, instead of a pass of its own over the
 * 2.4-GB operand (m3p_ce_shift_colsum); the weights enter rounded to bf16, the sums are fp32.  dW is bit-identical to m3p_gemm_wgrad_store_bf16 / m3p_gemm_wgrad_bf16 on the same
 * operands.  bsum must not overlap dW.  Returns M3P_ENOTIMPL - and launches nothing - wherever the four-wave kernel would not
 * deal out whole tiles (see m3p_gemm_wgrad_store_bf16), for M > 16384 (the weights live in LDS) or a misaligned operand. */
/* The same through the existing entry points: arms the calling thread's NEXT m3p_gemm_wgrad_store_bf16 / m3p_gemm_wgrad_bf16 call - if
 * that call runs the whole-tile schedule (and M <= 16384) it is the launch above with these operands, otherwise it is what it
 * always was.  Returns 1 if a launch has taken the operands armed before this call, else 0, and replaces them: (NULL, NULL)
 * disarms.  Arm, call, then disarm and read whether the sums were written. */
M3P_API int m3p_gemm_wgrad_bias_arm(const float* w, float* bsum);
M3P_API int m3p_gemm_wgrad_bias_bf16(const void* dY, int lddy, const void* X, int ldx, float* dW, int lddw, int M, int N, int K,
                                     float alpha, const float* w, float* bsum, int store, void* stream);
/* Two weight gradients over the same M rows in ONE launch of the four-wave kernel (and one reduction): dWa += dYa^T Xa,
 * dWb += dYb^T Xb.  The attention sub-layer's out_lin (768 x 768: 9 output tiles) and q/k/v (27 tiles) gradients of
 * MultiHeadAttention (transformer.py:178-181, :208) together fill the 256 CUs as evenly as one FFN gradient does - apart they
 * end in two end-of-kernel flushes and two reductions.  Falls back to two m3p_gemm_wgrad_bf16 calls when the shapes are not
 * whole 256 x 256 tiles, M % 64 != 0, the tiles of both together exceed half the CUs, or there is no workspace. */
M3P_API int m3p_gemm_wgrad_pair_bf16(const void* dYa, int lddya, const void* Xa, int ldxa, float* dWa, int lddwa, int Na, int Ka,
                                     const void* dYb, int lddyb, const void* Xb, int ldxb, float* dWb, int lddwb, int Nb, int Kb,
                                     int M, float alpha, void* workspace, size_t workspace_bytes, void* stream);
/* Up to M3P_WGRAD_GROUP_MAX weight gradients over the same M rows in ONE launch of the four-wave kernel, one workgroup per
 * 256 x 256 output tile over the WHOLE of M: dW_k += alpha * dY_k^T X_k.  Where the pair above splits M over nwg / tiles
 * chunks and folds the chunks' partial tiles through the workspace, a group that brings about one tile per CU (seven 36-tile
 * products: the layer weight gradients of 2 1/3 encoder layers) has no partial tiles at all: every tile is a single running
 * fp32 sum, added to dW once by its only writer - no workspace, no reduce kernel, no atomics, bit-reproducible.
 * Accepted when every item is a whole-tile shape of the four-wave kernel (N % 256 == 0, K % 256 == 0, M % 64 == 0, M >= 4096,
 * lddy / ldx % 8 == 0 and >= N / K, 16-byte aligned operands), lddw >= K, lddw % 4 == 0, dW 16-byte aligned, and the tiles of
 * all items together are at most the persistent grid (the CU count, or what m3p_set_persistent_grid left of it).  Anything
 * else returns M3P_ENOTIMPL (M3P_EINVAL for null pointers, non-positive sizes, n_items outside 1 .. M3P_WGRAD_GROUP_MAX) and
 * writes nothing: the caller runs the products through the calls above.  The items' dW must not overlap. */
#define M3P_WGRAD_GROUP_MAX 12
typedef struct M3PWgradItem {
  const void* dY; const void* X; float* dW;
  int lddy, ldx, lddw, N, K;
} M3PWgradItem;
M3P_API int m3p_gemm_wgrad_group_bf16(const M3PWgradItem* items, int n_items, int M, float alpha, void* stream);
/* The group's placement (host only, no device access): place[w], w < workgroups (a multiple of 8, at most 256), is what
 * workgroup w of the launch computes - item << 16 | tile row << 8 | tile column, or 0xffffffff for none.  Workgroup w runs on
 * XCD w % 8; tiles of one product share operand panels only through their XCD's L2, so a product's tiles are dealt to as few
 * XCDs as possible: whole XCDs first, the remainders best-fit into what is left.  tiles_i / tiles_j: N / 256, K / 256 per
 * item.  Returns M3P_ENOTIMPL when the tiles do not fit. */
M3P_API int m3p_gemm_wgrad_group_place(const int* tiles_i, const int* tiles_j, int n_items, int workgroups, uint32_t* place);

/* ------------------------------------------------------------------------------------
 * LayerNorm (eps = 1e-12 in the reference: transformer.py:244,660,694,709)
 * ---------------------------------------------------------------------------------- */

/* y[r,:] = LN(x[r,:]) * gamma + beta, then * rowmask[r] if rowmask != NULL
 * (the `tensor *= mask` of transformer.py:958).  x,y bf16 [rows,d]; gamma,beta fp32;
 * mean,rstd fp32 [rows] saved for backward.  d % 4 == 0, d <= 2048. */
M3P_API int m3p_layernorm_fwd(const void* x, const float* gamma, const float* beta, const uint8_t* rowmask,
                              void* y, float* mean, float* rstd, int rows, int d, float eps, void* stream);

/* Backward of the above.  dy = dy_a (+ dy_b if not NULL), multiplied by rowmask[r] if given.
 *   dx        : bf16 [rows,d] gradient wrt the LayerNorm input (always written)
 *   dx_drop   : if not NULL, also dx * keep/(1-p) with the dropout stream (seed,thresh24)
 *               indexed by r*d+c — i.e. the gradient pushed through the dropout that
 *               produced the residual branch (transformer.py:951 / :226)
 *   dgamma,dbeta : fp32 [d], accumulated with atomics
 *   dbias_drop: if not NULL fp32 [d] += column sums of dx_drop (the bias gradient of the
 *               Linear feeding that dropout: out_lin.bias / lin2.bias). */
M3P_API int m3p_layernorm_bwd(const void* dy_a, const void* dy_b, const void* x, const float* gamma,
                              const float* mean, const float* rstd, const uint8_t* rowmask,
                              void* dx, void* dx_drop, float* dgamma, float* dbeta, float* dbias_drop,
                              int rows, int d, uint32_t seed, uint32_t thresh24, float inv_keep, void* stream);
/* The same on a row subset of a larger tensor: the dropout stream of dx_drop is indexed by rng_rows[r]*d+c (int32 [rows],
 * device; NULL = r) - M3PEpilogue::rng_rows of the forward launch that drew the mask. */
M3P_API int m3p_layernorm_bwd_rows(const void* dy_a, const void* dy_b, const void* x, const float* gamma,
                                   const float* mean, const float* rstd, const uint8_t* rowmask,
                                   void* dx, void* dx_drop, float* dgamma, float* dbeta, float* dbias_drop,
                                   int rows, int d, uint32_t seed, uint32_t thresh24, float inv_keep,
                                   const int32_t* rng_rows, void* stream);

/* ------------------------------------------------------------------------------------
 * Fused multi-head self-attention (transformer.py:149-210, self-attention branch)
 * ---------------------------------------------------------------------------------- */

/* qkv bf16 [B*S, 3*H*dh] token-major (q | k | v column blocks, q already scaled by
 * 1/sqrt(dh) — M3P_EPI_BIAS scale_cols); keylen int32 [B]: keys >= keylen[b] are masked
 * to -inf (get_masks, transformer.py:59-78, non-causal).  Softmax in fp32, dropout on the
 * probabilities with stream (seed, thresh24) indexed ((b*H+h)*S+q)*S+key, context = P v.
 * ctx bf16 [B*S, H*dh] token-major; lse fp32 [B,H,S] = log-sum-exp saved for backward.
 * dh in {32, 64}, S <= 512. */
M3P_API int m3p_attn_fwd(const void* qkv, const int32_t* keylen, void* ctx, float* lse, uint64_t* keepmask,
                         int B, int S, int H, int dh, uint32_t seed, uint32_t thresh24, float inv_keep,
                         void* stream);
/* keepmask (nullable): if given and thresh24 != 0, the forward also leaves the dropout keep
 * bits, [B*H][nt][nt][4] 64-bit words with nt = ceil(S/16); word [qb][t][r] bit l is the
 * keep decision of (query 16qb + (l & 15), key 16t + 4(l >> 4) + r).  m3p_attn_bwd tests these bits
 * (it needs them whenever dropout is on). */

/* Backward: given dctx (bf16 [B*S, H*dh]) writes dqkv (bf16 [B*S, 3*H*dh]; the q block is
 * multiplied by qscale = 1/sqrt(dh) so it is the gradient of the *unscaled* projection)
 * and, if dbias_qkv != NULL, accumulates (atomics) the column sums of the q and v blocks of
 * dqkv into the fp32 [3*H*dh] bias gradient of the fused q/k/v projection.  The k block of
 * the bias gradient is left untouched: it is identically 0 (softmax is invariant to a
 * per-query shift of the scores; the reference's value there is fp32 noise).  Scores are recomputed from
 * qkv + lse (nothing S x S is ever stored).  S <= 512.  With dropout on (thresh24 != 0) keepmask - the words m3p_attn_fwd
 * left - is REQUIRED (M3P_EINVAL without; round 6: the instantiations that re-drew the decisions from (seed, thresh24) served
 * tests only); seed is unused. */
M3P_API int m3p_attn_bwd(const void* qkv, const int32_t* keylen, const void* ctx, const void* dctx,
                         const float* lse, const uint64_t* keepmask, void* dqkv, float* dbias_qkv, int B, int S,
                         int H, int dh, float qscale, uint32_t seed, uint32_t thresh24, float inv_keep,
                         void* stream);

/* Decoder inference (transformer.py:149-210 with the key / value cache of :187-195): every query row
 * attends a prefix of a cached key / value sequence.  q bf16 [B*Tq, ld_q] (scaled and biased by the projection's
 * epilogue); key j of sequence b, head h at kv + b*kv_bstride + j*ld_kv + h*dh, its value H*dh elements further
 * (bf16; element strides, multiples of 8); klen int32 [B] or NULL (= Lk keys everywhere); causal != 0: query t sees keys
 * 0 .. pos0 + t only (pos0 = tokens cached before this call).  fp32 softmax, no dropout (inference), ctx bf16
 * [B*Tq, H*dh].  dh in {32, 64}, Lk <= 1024. */
M3P_API int m3p_attn_query_fwd(const void* q, int ld_q, const void* kv, long long kv_bstride, int ld_kv,
                               const int32_t* klen, void* ctx, int B, int Tq, int H, int dh, int Lk, int causal,
                               int pos0, void* stream);

/* m3p_attn_query_fwd over key / value rows that stay where they were written (beam search without re-ordering the caches):
 * key j of query sequence b - and its value - is read from kv row owner[b*owner_bstride + j*owner_kstride] instead of row b
 * (kv + row*kv_bstride + j*ld_kv + h*dh).  owner_kstride = 1: one row per (sequence, key) - the self-attention cache, where
 * position j of a hypothesis lives in the row of the beam that wrote it; owner_kstride = 0: one row per sequence - an
 * encoder-attention cache kept once per sentence.  klen stays indexed by b.  The arithmetic and its order are
 * m3p_attn_query_fwd's: the result equals that call on the gathered copy bit for bit.  Entries of owner outside the kv
 * tensor are the caller's error (they are not checked). */
M3P_API int m3p_attn_query_owner_fwd(const void* q, int ld_q, const void* kv, long long kv_bstride, int ld_kv,
                                     const int32_t* klen, void* ctx, int B, int Tq, int H, int dh, int Lk, int causal,
                                     int pos0, const int32_t* owner, int owner_bstride, int owner_kstride, void* stream);

/* Word selection of the decoding loops from the bf16 logits of the vocabulary projection (csrc/select.hip).
 * logits bf16 [n, ld], n = bs*beam rows (the beams of a sentence are consecutive rows), ld >= V, ld % 8 == 0, 16-byte
 * aligned; columns V .. ld-1 may hold anything.  beam_scores fp32 [n] or NULL (zeros).
 *   lse[r]                       fp32 log-sum-exp of row r over its V columns
 *   score of entry (r, w)        fl32(fl32(float(logits[r, w]) - lse[r]) + beam_scores[r])
 *   scores [bs, k], flat_idx [bs, k] (= beam*V + w)   per sentence the first k of its beam*V entries under the total
 *                                order: score descending, then beam ascending, then logit descending, then word ascending.
 * Two launches, no atomics, every logit read once; bit-reproducible.  workspace: m3p_vocab_select_workspace_bytes(n, V, k)
 * bytes, 16-byte aligned, contents irrelevant.  k <= m3p_vocab_select_max_k() (16), beam <= 64, k <= beam*V; larger k or
 * beam returns M3P_ENOTIMPL.  m3p_vocab_select_plan answers what the launcher would (M3P_OK / M3P_ENOTIMPL / M3P_EINVAL)
 * for a shape, without launching. */
M3P_API int m3p_vocab_select_max_k(void);
M3P_API int m3p_vocab_select_plan(int n, int V, int ld, int beam, int k);
M3P_API size_t m3p_vocab_select_workspace_bytes(int n, int V, int k);
M3P_API int m3p_vocab_select(const void* logits, int ld, int n, int V, const float* beam_scores, int beam, int k,
                             void* workspace, size_t workspace_bytes, float* scores, long long* flat_idx, float* lse,
                             void* stream);

/* m3p_vocab_select for wider beams (csrc/select.hip): the same contract word for word - lse, the score of an entry, the total
 * order, flat_idx, -0 folded into +0, columns V .. ld-1 never looked at - for 1 <= k <= m3p_vocab_select_wide_max_k() (64) and
 * beam <= 32.  lse has the bits m3p_vocab_select writes for the same logits, so for k <= 16 all three outputs are bit-equal to
 * that entry's.  A row's first k words under (logit descending, word ascending) come from the exact count selection of
 * m3p_vocab_sample_wide (integer atomics: counts do not depend on their order), a sentence's beam*k entries are then sorted
 * under the total order by one workgroup in LDS: the same inputs give the same bits.  k > V is M3P_EINVAL here (a row supplies
 * at most V entries to its own first k), like every malformed shape of m3p_vocab_select_plan; k > 64, beam > 32 or 32-bit block
 * indices that would overflow return M3P_ENOTIMPL.  workspace: m3p_vocab_select_wide_workspace_bytes(n, V, beam, k) bytes,
 * 16-byte aligned, contents irrelevant.  m3p_vocab_select_wide_plan answers what the launcher would, without launching. */
M3P_API int m3p_vocab_select_wide_max_k(void);
M3P_API int m3p_vocab_select_wide_plan(int n, int V, int ld, int beam, int k);
M3P_API size_t m3p_vocab_select_wide_workspace_bytes(int n, int V, int beam, int k);
M3P_API int m3p_vocab_select_wide(const void* logits, int ld, int n, int V, const float* beam_scores, int beam, int k,
                                  void* workspace, size_t workspace_bytes, float* scores, long long* flat_idx, float* lse,
                                  void* stream);

/* Seeded temperature / top-k sampling of the next word from the same logits (csrc/select.hip), by Gumbel-max: one pass, no
 * prefix sums, and every random number is a pure function of (seed, row, word), so a draw can be replayed and checked
 * (NumPy twin: m3p_amd/rng.py sample_uniform / sample_keys / sample_words).  For row r and word w < V:
 *   m = m3p_hash32(r*V + w, seed) >> 8      (24 bits; the hash of csrc/common.hpp)
 *   u = (m + 0.5) * 2^-24                   in (0, 1)
 *   E = -log(u)
 *   key(r, w) = float(logits[r, w]) * inv_t - log(E)
 * words[r] = the argmax of key(r, .) over the allowed set, ties to the lowest word: a sample of softmax(float(logits[r, :V]) *
 * inv_t) restricted to that set and renormalised.  The one deviation is the 24-bit grid of u: log(E) spans [-17.33, 2.85],
 * so a word whose probability is below about 2^-24 of the most likely word's is never drawn.
 *   allowed set   top_k = 0: all V words; 1 <= top_k <= m3p_vocab_select_max_k() (16): the row's first top_k entries under
 *                 (logit descending, word ascending); larger top_k returns M3P_ENOTIMPL, top_k > V M3P_EINVAL.
 *   words   int64 [n]
 *   logprob fp32 [n]   x_w*inv_t - lse_T, lse_T = log-sum-exp of float(logits[r, w])*inv_t over the allowed set
 *   key     fp32 [n]   the winning key; may be NULL
 * logits as for m3p_vocab_select (bf16 [n, ld], ld >= V, ld % 8 == 0, 16-byte aligned); columns V .. ld-1 may hold anything
 * (NaN, inf) and are never chosen; a -inf logit below V has probability 0 and is never chosen while the row holds a finite
 * one.  Preconditions: n*V < 2^32 (the hash counter; M3P_ENOTIMPL otherwise), inv_t > 0 and finite (M3P_EINVAL otherwise),
 * every row holds at least one finite logit and no NaN in its V columns (not checked).  The row index of the counter is the
 * row of THIS call: the draw of a row depends on its position in the batch.  Two launches, no atomics, sums in a fixed
 * order: the same inputs give the same bits.  workspace: m3p_vocab_sample_workspace_bytes(n, V, top_k) bytes, 16-byte
 * aligned, contents irrelevant.  m3p_vocab_sample_plan answers what the launcher would for a shape, without launching. */
M3P_API int m3p_vocab_sample_plan(int n, int V, int ld, int top_k);
M3P_API size_t m3p_vocab_sample_workspace_bytes(int n, int V, int top_k);
M3P_API int m3p_vocab_sample(const void* logits, int ld, int n, int V, float inv_t, int top_k, uint32_t seed, void* workspace,
                             size_t workspace_bytes, long long* words, float* logprob, float* key, void* stream);

/* Nucleus (top-p) sampling: m3p_vocab_sample with a probability-mass cut on its allowed set (csrc/select.hip; NumPy twin:
 * m3p_amd/rng.py nucleus_cut / sample_allowed / sample_words with top_p).  All masses are over the candidate set K of a row:
 * top_k = 0 every word w < V; 1 <= top_k <= 16 the row's first top_k words under (logit descending, word ascending) - exactly
 * the allowed set of m3p_vocab_sample.  With x_w = float(logits[r, w]), y_w = x_w*inv_t and m = max over K of y:
 *   mass(v)    = #{w in K : x_w == v} * exp(v*inv_t - m)      for each distinct logit value v of the row
 *   C(v)       = the sum of mass(v') over v' >= v;  C_above(v) the same over v' > v;  Z = C(-inf)
 *   cut x*     = max{ v : C(v) >= top_p*Z }
 *   allowed set A = { w in K : x_w >= x* }
 * Words of equal logit are treated alike - the whole class at the cut is in: A has mass >= top_p, is the smallest union of
 * whole classes that does, and always holds the row's maximum.  The draw, logprob and key are m3p_vocab_sample's with A as the
 * allowed set: words[r] = the argmax over A of key(r, w) = x_w*inv_t - log(-log u), u from m3p_hash32(r*V + w, seed) (the
 * counter does not change), ties to the lowest word; logprob = y_w - log-sum-exp of y over A.
 *   cut     fp32 [n]   the bf16 value x*; may be NULL
 * 0 < top_p (M3P_EINVAL otherwise, NaN included); top_p >= 1 is "off": the call is m3p_vocab_sample itself - its bits in
 * words, logprob and key - and cut = -inf.  The device sums fixed-point integers (top_k = 0) or fp32 in a fixed order (top_k
 * >= 1) where the definition is exact: a row whose cumulated mass lands on top_p*Z to within 4e-6 Z may cut one class earlier
 * or later (the bound is derived in tests/test_vocab_nucleus.py).  Integer atomics only, no floating-point atomics: the same
 * inputs give the same bits.  A -inf logit has mass 0 and never enters A before a finite one.  Limits, preconditions, logits
 * and workspace as for m3p_vocab_sample, with m3p_vocab_nucleus_plan and m3p_vocab_nucleus_workspace_bytes(n, V, top_k). */
M3P_API int m3p_vocab_nucleus_plan(int n, int V, int ld, int top_k);
M3P_API size_t m3p_vocab_nucleus_workspace_bytes(int n, int V, int top_k);
M3P_API int m3p_vocab_nucleus_sample(const void* logits, int ld, int n, int V, float inv_t, int top_k, float top_p, uint32_t seed,
                                     void* workspace, size_t workspace_bytes, long long* words, float* logprob, float* key,
                                     float* cut, void* stream);

/* Seeded top-k sampling over more than 16 candidates, nucleus cut included (csrc/select.hip; the NumPy twin is the same:
 * rng.sample_allowed / nucleus_cut / sample_words take any top_k <= V).  The semantics are m3p_vocab_nucleus_sample's with
 * 1 <= top_k <= m3p_vocab_sample_wide_max_k() (1024):
 *   candidate set K   the row's first top_k words under (logit descending, word ascending): with v_k the k-th logit value,
 *                     every word above v_k and, of the words equal to v_k, as many as still fit - the lowest word ids
 *   key(r, w)         fma(x_w, inv_t, -log E), E = -log u, u from m3p_hash32(r*V + w, seed) as above: the counter, the
 *                     logarithms and so the key bits of m3p_vocab_sample
 *   top_p >= 1        no cut: the allowed set is K, cut = -inf
 *   0 < top_p < 1     the allowed set is { w in K : x_w >= x* }, x* = max{ v : C(v) >= top_p*Z } with mass, C and Z over K as
 *                     defined above; where the class at v_k is only partly inside K it counts the words that are in K
 *   words[r]          the argmax of key over the allowed set, ties to the lowest word
 *   logprob[r]        x_w*inv_t - log-sum-exp of x*inv_t over the allowed set;  key[r] the winning key (may be NULL);
 *   cut[r]            x* or -inf (may be NULL)
 * top_k > max_k returns M3P_ENOTIMPL; top_k < 1 or top_k > V M3P_EINVAL; the pointer, alignment, ld % 8, n*V < 2^32, inv_t and
 * top_p checks are those of m3p_vocab_nucleus_sample.  Columns at or past V may hold NaN or inf and are never chosen; a -inf
 * logit below V has mass 0, may sit in K when the row has fewer than top_k finite logits, and never wins while the row holds
 * a finite one.  K is found by an exact two-level count selection over the 65 536 bf16 values, compacted to [n, top_k] and
 * finished per row in one workgroup; the masses are integers on a 2^-40 grid, summed exactly, so a row whose cumulated mass
 * lands on top_p*Z to within 2e-6 Z may cut one class earlier or later (the bound is derived in
 * tests/test_vocab_sample_wide_cpu.py).  Integer atomics only, no floating-point atomics: the same inputs give the same bits.
 * workspace: m3p_vocab_sample_wide_workspace_bytes(n, V, top_k) bytes, 16-byte aligned, contents irrelevant.  The entry takes
 * top_k <= 16 too (the words and key bits of m3p_vocab_sample; logprob to rounding) - the decoding loop sends only top_k > 16. */
M3P_API int m3p_vocab_sample_wide_max_k(void);
M3P_API int m3p_vocab_sample_wide_plan(int n, int V, int ld, int top_k);
M3P_API size_t m3p_vocab_sample_wide_workspace_bytes(int n, int V, int top_k);
M3P_API int m3p_vocab_sample_wide(const void* logits, int ld, int n, int V, float inv_t, int top_k, float top_p, uint32_t seed,
                                  void* workspace, size_t workspace_bytes, long long* words, float* logprob, float* key,
                                  float* cut, void* stream);

/* Decoding constraints (csrc/constrain.hip; torch twin: m3p_amd/decoder.py constrain_scores_): edits the bf16 logits of a
 * decoding step IN PLACE, in front of m3p_vocab_select / m3p_vocab_sample / m3p_vocab_nucleus_sample, which take a -inf logit
 * as "never chosen, mass 0".  ONE rule for every route of the search loops:
 * At the step that decodes position cur_len, row r has the history H = generated[1:cur_len, r] of length L = cur_len - 1; the
 * <EOS> that serves as <BOS> at position 0 is NOT part of H.  The row's V logits x[w] are changed in this order:
 *   1. repetition penalty theta (finite, > 0; 1 is off): every DISTINCT word w of H with 0 <= w < V, once however often it
 *      occurs:  x[w] <- bf16_rne(fl32(x[w] * (x[w] > 0 ? inv_theta : theta))).  theta and inv_theta = fl32(1 / theta) are both
 *      formed by the caller: one fp32 multiply, no divide.  0, -0 and -inf keep their bits.
 *   2. no repeated n-gram, ngram = n >= 1 (0 is off): for every j in [0, L - n] with H[j + i] == H[L - n + 1 + i] for all i in
 *      [0, n - 2], the word H[j + n - 1] gets -inf.  n = 1 bans every word of H; nothing happens while L < n.
 *   3. minimum length: x[eos_or_minus1] <- -inf unless eos_or_minus1 is -1 (the caller passes <EOS> while cur_len <= min_len).
 *   4. banned words: every id of banned[0 .. n_banned - 1] gets -inf.
 * Everything else keeps its bits: the other words, the columns V .. ld-1, the other rows.  A history word or banned id outside
 * [0, V) is skipped.  Under beam search the edit happens before the row's log-sum-exp: the scores are log_softmax of the
 * constrained logits plus the beam score; the log-probabilities of a sampled word are those of the constrained row.
 *   logits  bf16 [n, ld], ld >= V, written in place
 *   hist    int64, points at generated[1]: element (p, r) at hist[p*hist_ld + r], hist_ld >= n, p < hist_len = L; row r of the
 *           logits reads COLUMN r.  May be NULL when hist_len is 0.
 *   banned  int64 [n_banned] on the device; may be NULL when n_banned is 0.
 * One launch (none when the step has nothing to edit), a workgroup per row, plain 2-byte stores, no atomics; every penalised
 * word has one writer.  Limits: hist_len <= 1024, ngram <= 16, n_banned <= 4096 - above them M3P_ENOTIMPL (the caller applies
 * the twin); M3P_EINVAL for a malformed shape, theta or inv_theta not finite and > 0, eos_or_minus1 outside [-1, V).
 * m3p_logits_constrain_plan answers what the launcher would for a shape, without launching; it depends on shapes alone. */
M3P_API int m3p_logits_constrain_plan(int n, int V, int ld, int hist_len, int ngram, int n_banned);
M3P_API int m3p_logits_constrain(void* logits, int ld, int n, int V, const long long* hist, long long hist_ld, int hist_len,
                                 float theta, float inv_theta, int ngram, int eos_or_minus1, const long long* banned,
                                 int n_banned, void* stream);

/* Hypothesis bookkeeping of one beam-search step (csrc/beam.hip; host twin: m3p_amd/decoder.py beam_advance_host, which the
 * kernel equals bit for bit): from the step's candidates to the sentences' lists of finished hypotheses, the next beams and, in
 * the same launch, the re-ordered token matrix and owner table.  Per sentence s, with n = bs*beam rows in all:
 *   next_scores fp32 [bs, k], flat_idx int64 [bs, k]   the candidates in the selection's order (m3p_vocab_select: score
 *               descending, so entry 0 is the maximum); flat_idx = b*V + word, 0 <= b < beam; the candidate's row is s*beam + b
 *   norm        fp64 [max_len + 1] on the device, norm[l] = (double)l ** length_penalty; norm_max = (double)(max_len - 1) **
 *               length_penalty; both formed by the host
 *   done[s] |= hyp_count[s] >= beam and (early_stopping or min_j hyp_score[s, j] >= (double)next_scores[s, 0] / norm_max)
 *   a done sentence emits beam x (0.0, pad, row 0) and nothing of its state changes.  Otherwise the candidates are walked in
 *   order: one whose word is eos - every one when cur_len + 1 == max_len - is OFFERED to the list: score = (double)value /
 *   norm[cur_len], arrival = arrivals[s]++; while hyp_count[s] < beam it takes slot hyp_count[s]++, afterwards the slot minimal
 *   by (hyp_score, hyp_arrival), and only if score > that slot's score.  An accepted one writes hyp_tok[s, slot, 0 .. cur_len-1]
 *   = gen_in[0 .. cur_len-1, row], hyp_len = cur_len, hyp_score = score, hyp_sum = value, hyp_arrival = arrival.  Every other
 *   candidate is the next continuation (value, word, row); the walk ends at `beam` of them; missing ones are (0.0, pad, row 0),
 *   and when cur_len + 1 < max_len that sets status[s] |= 1.  A flat_idx outside [0, beam*V) sets status[s] |= 2 and is read
 *   as beam 0.
 *   beam_scores fp32 [n], beam_words int64 [n], beam_idx int64 [n]   the continuations, row r = s*beam + j
 *   gen_in / gen_out   int64 [max_len, gen_ld >= n] row-major (the layout m3p_logits_constrain reads): gen_out[p, r] =
 *               gen_in[p, beam_idx[r]] for p < cur_len, gen_out[cur_len, r] = beam_words[r]; positions past cur_len untouched
 *   owner_in / owner_out   int32 [n, owner_ld >= max_len]: owner_out[r, p] = owner_in[beam_idx[r], p] for p < max_len, except
 *               owner_out[r, cur_len] = r  (the owner table of m3p_attn_query_owner_fwd after the step)
 *   state       hyp_tok int64 [bs, beam, max_len] (pad behind hyp_len), hyp_len int32, hyp_score fp64, hyp_sum fp32, hyp_arrival
 *               int32 [bs, beam]; hyp_count, arrivals, status int32 [bs]; done uint8 [bs].  Zeros (hyp_tok: pad) before step 1.
 * gen_in != gen_out and owner_in != owner_out (M3P_EINVAL): a done sentence reads row 0, which another workgroup writes.  One
 * launch, one wave per sentence, no atomics; the fp64 work is one conversion, one division and comparisons - IEEE, so the
 * bits are the host's.  1 <= cur_len < max_len.  Limits: beam <= 32, k <= 64, max_len <= 1025 - above them M3P_ENOTIMPL (the
 * caller keeps the host twin).  m3p_beam_advance_plan answers what the launcher would for a shape, without launching. */
M3P_API int m3p_beam_advance_plan(int bs, int beam, int k, int max_len);
M3P_API int m3p_beam_advance(const float* next_scores, const long long* flat_idx, int bs, int beam, int k, int V, int cur_len,
                             int max_len, int eos, int pad, int early_stopping, const double* norm, double norm_max,
                             const long long* gen_in, long long* gen_out, long long gen_ld, const int32_t* owner_in,
                             int32_t* owner_out, int owner_ld, float* beam_scores, long long* beam_words, long long* beam_idx,
                             long long* hyp_tok, int32_t* hyp_len, double* hyp_score, float* hyp_sum, int32_t* hyp_arrival,
                             int32_t* hyp_count, int32_t* arrivals, uint8_t* done, int32_t* status, void* stream);

/* The same attention for the TRAINING of the causal / cross-attention sub-layers (teacher forcing: Tq = the whole target
 * sequence, pos0 = 0): dropout on the probabilities (stream (seed, thresh24) indexed ((b*H + h)*Tq + t)*Lk + key) and the
 * log-sum-exp lse fp32 [B, H, Tq] kept for backward.  B*H*Tq*Lk < 2^32. */
M3P_API int m3p_attn_rows_fwd(const void* q, int ld_q, const void* kv, long long kv_bstride, int ld_kv, const int32_t* klen,
                              void* ctx, float* lse, int B, int Tq, int H, int dh, int Lk, int causal, int pos0,
                              uint32_t seed, uint32_t thresh24, float inv_keep, void* stream);
/* Backward: dq bf16 [B*Tq, ld_dq] = gradient of the UNSCALED query projection (the scaled gradient x qscale, like
 * m3p_attn_bwd); the key / value gradients are ADDED (fp32 atomics) into dkv [B, Lk, 2*H*dh] (keys | values per position),
 * which the caller zeroes. */
M3P_API int m3p_attn_rows_bwd(const void* q, int ld_q, const void* kv, long long kv_bstride, int ld_kv, const int32_t* klen,
                              const void* dctx, const float* lse, void* dq, int ld_dq, float* dkv, int B, int Tq, int H,
                              int dh, int Lk, int causal, int pos0, float qscale, uint32_t seed, uint32_t thresh24,
                              float inv_keep, void* stream);

/* Causal SELF-attention of a decoder-only training pass (the causal language-model objective, xtrainer.py:694-732) on
 * tiled MFMA kernels: exactly m3p_attn_rows_fwd / _bwd(causal = 1, klen = NULL, pos0 = 0, Lk = T) - query t sees keys 0 .. t
 * by position only, fp32 softmax, the same dropout stream index ((b*H + h)*T + t)*T + key - without atomics.
 * qkv bf16 [B*T, ld_qkv] is the fused projection (d = H*dh): q at column h*dh (biased and scaled by 1/sqrt(dh)), k at
 * d + h*dh, v at 2*d + h*dh.  ctx bf16 [B*T, d], lse fp32 [B, H, T] (natural log).
 * dh in {32, 64}, 1 <= T <= 512, B*H*T*T < 2^32, ld % 8 == 0 and 16-byte aligned pointers; any other shape returns
 * M3P_ENOTIMPL (the caller then takes the rows kernels). */
M3P_API int m3p_attn_causal_fwd(const void* qkv, int ld_qkv, void* ctx, float* lse, int B, int T, int H, int dh,
                                uint32_t seed, uint32_t thresh24, float inv_keep, void* stream);
/* Backward: dqkv bf16 [B*T, ld_dqkv] laid out dq | dk | dv like qkv; dq is the gradient of the UNSCALED projection
 * (x qscale, like m3p_attn_rows_bwd).  Every element of the B*T rows' 3*d columns is written: no fp32 buffer, nothing for
 * the caller to zero.  (While the call runs, the first four bytes of each (row, head) dq slot hold an intermediate.) */
M3P_API int m3p_attn_causal_bwd(const void* qkv, int ld_qkv, const void* dctx, const float* lse, void* dqkv, int ld_dqkv,
                                int B, int T, int H, int dh, float qscale, uint32_t seed, uint32_t thresh24,
                                float inv_keep, void* stream);

/* Attention over a SOURCE ENCODING in a teacher-forced decoder pass (the encoder-attention sub-layer of the seq2seq steps)
 * on tiled MFMA kernels: exactly m3p_attn_rows_fwd / _bwd(causal = 0, pos0 = 0) - the same layouts (q bf16 [B*Tq, ld_q],
 * biased and scaled; key j of sequence b, head h at kv + b*kv_bstride + j*ld_kv + h*dh, its value H*dh elements further;
 * klen int32 [B] or NULL), fp32 softmax over the first nk = min(klen[b], Lk) keys, the same dropout stream index
 * ((b*H + h)*Tq + t)*Lk + key - without atomics.  Key / value rows at or past nk are never used and may hold anything
 * (NaN included).  ctx bf16 [B*Tq, H*dh], lse fp32 [B, H, Tq] (natural log); klen[b] == 0 gives ctx = 0 and lse = 0.
 * dh in {32, 64}, 1 <= Tq <= 512, 1 <= Lk <= 1024, B*H*Tq*Lk < 2^32, strides multiples of 8 and 16-byte aligned pointers;
 * any other shape returns M3P_ENOTIMPL (the caller then takes the rows kernels). */
M3P_API int m3p_attn_cross_fwd(const void* q, int ld_q, const void* kv, long long kv_bstride, int ld_kv, const int32_t* klen,
                               void* ctx, float* lse, int B, int Tq, int H, int dh, int Lk, uint32_t seed, uint32_t thresh24,
                               float inv_keep, void* stream);
/* PREFILL of a prompted decoding call on the same tiled MFMA body: causal attention of a block of Tq new queries over a
 * key / value cache that already holds their own rows - exactly m3p_attn_query_fwd(causal = 1, klen = NULL,
 * Lk = pos0 + Tq, pos0).  Layouts as m3p_attn_cross_fwd: q bf16 [B*Tq, ld_q], biased and scaled; key j of sequence b, head h
 * at kv + b*kv_bstride + j*ld_kv + h*dh, its value H*dh elements further.  Query t (position pos0 + t) sees keys
 * 0 .. pos0 + t; fp32 softmax, no dropout, no klen.  ctx bf16 [B*Tq, H*dh]; lse fp32 [B, H, Tq] (natural log) or NULL.
 * Cache rows at or past pos0 + Tq are never read and may hold anything (NaN included).  With pos0 = 0 over a packed
 * q | k | v buffer (kv = qkv + H*dh, ld_kv = ld_qkv, kv_bstride = T*ld_qkv) ctx and lse equal m3p_attn_causal_fwd without
 * dropout bit for bit.  Forward only.
 * dh in {32, 64}, 1 <= Tq <= 512, pos0 >= 0, pos0 + Tq <= 1024, strides multiples of 8 and 16-byte aligned q, kv, ctx; any
 * other shape returns M3P_ENOTIMPL (the caller then keeps m3p_attn_query_fwd, a complete fallback). */
M3P_API int m3p_attn_prefix_fwd(const void* q, int ld_q, const void* kv, long long kv_bstride, int ld_kv, void* ctx, float* lse,
                                int B, int Tq, int H, int dh, int pos0, void* stream);
/* Backward: dq bf16 [B*Tq, ld_dq] = gradient of the UNSCALED query projection (x qscale, like m3p_attn_rows_bwd); dkv BF16
 * [B, Lk, ld_dkv] (keys | values per position, ld_dkv >= 2*H*dh): every one of the Lk rows' 2*H*dh columns is written
 * exactly once - fp32 accumulators rounded once, exact zeros for keys >= nk - so the caller zeroes nothing and casts
 * nothing.  klen[b] == 0 gives dq = 0 and dkv = 0.  (While the call runs, the first four bytes of each (row, head) dq slot
 * hold an intermediate.) */
M3P_API int m3p_attn_cross_bwd(const void* q, int ld_q, const void* kv, long long kv_bstride, int ld_kv, const int32_t* klen,
                               const void* dctx, const float* lse, void* dq, int ld_dq, void* dkv, int ld_dkv, int B, int Tq,
                               int H, int dh, int Lk, float qscale, uint32_t seed, uint32_t thresh24, float inv_keep,
                               void* stream);

/* ------------------------------------------------------------------------------------
 * Input assembly of jointfwd (transformer.py:901-943) and its backward
 * ---------------------------------------------------------------------------------- */

/* fp32 -> bf16 (the region features / any fp32 input that feeds a GEMM). n % 4 == 0. */
M3P_API int m3p_cast_f32_bf16(const float* src, void* dst, long long n, void* stream);

/* Builds the encoder input h[B*S, d] (bf16, batch-major rows b*S+s, S = R+T):
 *   image rows s<R : LN_img(img_proj[s*B+b] + W_loc loc[s,b] + b_loc) -> dropout(seed_img)
 *                    (BertImageEmbeddings.forward, transformer.py:257-268; img_proj is the
 *                    W_img x + b GEMM output in the caller's sequence-major row order)
 *   token rows     : emb[tok[t,b]]                                       (:913)
 *   then + pos[s], * (s < totlen[b]), LN_emb, dropout(seed_emb)          (:936-943)
 * Saves z (LN_emb input) / e (LN_img input) and the LayerNorm statistics for backward.
 * tok int64 (T,B); emb bf16 [V,d]; pos,w_loc,b_loc,gammas,betas fp32; loc fp32 (R,B,5).
 * img_rows (nullable): bf16 [B*R, d], row b*R + r - the image rows to use INSTEAD of computing them
 * (jointfwd with refine_image=True, transformer.py:905-906: m3p_embed_image_rows_fwd -> AoA refiner ->
 * here); e / mean_img / rstd_img are then left untouched. */
M3P_API int m3p_embed_assemble_fwd(const int64_t* tok, const void* emb_bf16, const float* pos,
                                   const void* img_proj, const float* loc, const float* w_loc,
                                   const float* b_loc, const float* g_img, const float* be_img,
                                   const float* g_emb, const float* be_emb, const int32_t* totlen,
                                   void* h, void* z, float* mean_emb, float* rstd_emb, void* e,
                                   float* mean_img, float* rstd_img, int B, int T, int R, int d,
                                   uint32_t seed_img, uint32_t seed_emb, uint32_t thresh24, float inv_keep,
                                   const void* img_rows, void* stream);

/* The image rows alone: img_rows[b*R + r, :] = dropout(LN_img(img_proj[r*B+b] + W_loc loc[r,b] + b_loc))
 * (BertImageEmbeddings.forward, transformer.py:247-269) as their own bf16 [B*R, d] tensor, batch-major - the
 * input of the AoA refiner (refine_image=True).  Saves e / mean_img / rstd_img like m3p_embed_assemble_fwd. */
M3P_API int m3p_embed_image_rows_fwd(const void* img_proj, const float* loc, const float* w_loc, const float* b_loc,
                                     const float* g_img, const float* be_img, void* e, float* mean_img,
                                     float* rstd_img, void* img_rows, int B, int R, int d, uint32_t seed_img,
                                     uint32_t thresh24, float inv_keep, void* stream);

/* Backward of the above given dh[B*S,d].  Accumulates (fp32 atomics) into the parameter
 * gradients d_g_emb,d_be_emb [d], d_pos [S,d] (first S rows of position_embeddings),
 * d_emb [V,d] (scatter-add over token ids, rows of pad_index skipped like
 * nn.Embedding(padding_idx)), d_g_img,d_be_img,d_b_img,d_b_loc [d], d_w_loc [d,5]; writes
 * de [R*B,d] (bf16, gradient of img_proj, rows s*B+b) for the W_img weight-gradient GEMM.
 * dz_scratch: bf16 [B*S,d] workspace.
 * d_tok_rows (optional, bf16 [T*B,d]): when set, the token rows' gradients are WRITTEN there (row t*B+b, zero rows
 * for pad / masked tokens) instead of being scatter-added into d_emb - data parallelism exchanges these rows between
 * ranks and applies them with m3p_scatter_add_token_rows (the 768-MB dense matrix is then reduced early, see
 * m3p_amd/distributed.py).
 * phase: 0 = everything.  With the AoA refiner between the image rows and the assembly the two halves run
 * separately: 1 = LN_emb / position / token part only - leaves the gradient of the image rows in
 * dz_scratch[b*S + r]; the caller takes it through the refiner's backward, writes the result back to the same
 * rows, then 2 = image part only (dropout + LN_img + location embedding -> de and their parameter gradients). */
M3P_API int m3p_embed_assemble_bwd(const void* dh, const void* z, const float* mean_emb, const float* rstd_emb,
                                   const float* g_emb, const void* e, const float* mean_img,
                                   const float* rstd_img, const float* g_img, const int64_t* tok,
                                   const int32_t* totlen, const float* loc, void* dz_scratch, void* de,
                                   float* d_g_emb, float* d_be_emb, float* d_pos, float* d_emb,
                                   void* d_tok_rows, float* d_g_img, float* d_be_img, float* d_b_img, float* d_b_loc,
                                   float* d_w_loc, int B, int T, int R, int d, int pad_index,
                                   uint32_t seed_img, uint32_t seed_emb, uint32_t thresh24, float inv_keep,
                                   int phase, void* stream);

/* ------------------------------------------------------------------------------------
 * Heads (TransformerModel.predict, transformer.py:1183-1214; PredLayer :104-117)
 * ---------------------------------------------------------------------------------- */

/* dst[i,:] = src[idx[i],:] — the boolean-mask gather of :1208 with precomputed row indices */
M3P_API int m3p_gather_rows(const void* src, const int32_t* idx, void* dst, int n, int d, void* stream);
/* dst[r,:] (bf16 [rows, d]) = src[inv[r],:] where inv[r] >= 0 (bf16 [n, d]), else the bf16 bit pattern fill_bits (0 = zero,
 * 0x7FC0 = NaN): a filled full-size tensor with n compact rows placed in it, written in one pass (inv = the inverse of the
 * row list; entries outside [0, n) count as "not selected").  d % 8 == 0, 16-byte aligned bases. */
M3P_API int m3p_place_rows(const void* src, const int32_t* inv, void* dst, int rows, int d, int n, uint32_t fill_bits,
                           void* stream);
/* dst[idx[i],:] += src[i,:] (idx unique) — its backward */
M3P_API int m3p_scatter_add_rows(const void* src, const int32_t* idx, void* dst, int n, int d, void* stream);
/* dst[ids[i],:] (fp32 [V,d]) += rows[i,:] (bf16 [n,d], row pitch ld_rows elements); ids may repeat (atomics), rows with
 * ids[i] == pad_index are skipped (nn.Embedding(padding_idx), transformer.py:21-26).  The embedding-lookup gradient of token
 * rows gathered from the data-parallel ranks (m3p_embed_assemble_bwd with d_tok_rows); the pitch lets the exchange carry each
 * row's id in extra columns behind it - one collective instead of two. */
M3P_API int m3p_scatter_add_token_rows(const void* rows, int ld_rows, const int64_t* ids, float* dst, int n, int d,
                                       int pad_index, void* stream);

/* ----------------------------------------------------------------------------------
 * ITM head: transformer.py:546-558 (BertPooler: tanh(dense(hidden[:, 0]))) followed by
 * :1194-1197 (seq_relationship Linear(d, 1)); position 0 of a joint sequence is the first
 * image region.  The d x d products run on the GEMMs above:
 *   forward   pre = m3p_gemm_nt_bf16(h0 [B,d], W1 [d,d], M3P_EPI_BIAS b1)            (bf16 [B,d])
 *             m3p_itm_score_fwd: pooled = tanh(pre) (fp32 [B,d], saved), scores = w2 . pooled + b2
 *   backward  m3p_itm_score_bwd(dscores [B]): dpre = dscore w2 (1 - pooled^2) as bf16 [B,d] and
 *             transposed [d, ldt >= B]; ACCUMULATES db1, dw2 [d], db2 [1] (fp32)
 *             dW1 += m3p_gemm_wgrad_bf16(dY = dpre16, X = h0);  dh0 = m3p_gemm_wgrad_bf16(dY = dpreT16, X = W1)
 * ---------------------------------------------------------------------------------- */
M3P_API int m3p_itm_score_fwd(const void* pre, const float* w2, const float* b2, float* pooled, float* scores, int B,
                              int d, void* stream);
M3P_API int m3p_itm_score_bwd(const float* dscores, const float* pooled, const float* w2, void* dpre16, void* dpreT16,
                              int ldt, float* db1, float* dw2, float* db2, int B, int d, void* stream);

/* F.cross_entropy over bf16 logits [n_rows, ld] (V valid columns), per-row loss to
 * row_loss, loss_sum += loss_scale * sum(row losses) if loss_sum != NULL, and IN PLACE
 * logits <- (softmax - onehot(target)) * grad_scale, padding columns [V, ld) zeroed.
 * ld % 8 == 0, logits 16-byte aligned. */
M3P_API int m3p_ce_fwd_bwd(void* logits, int ld, int n_rows, int V, const int64_t* target, float* row_loss,
                           float* loss_sum, float loss_scale, float grad_scale, void* stream);

/* The same cross-entropy with the column sums of the gradient - the gradient of the output bias (PredLayer.proj.bias,
 * transformer.py:111) - produced by the pass that writes the gradient, instead of a second pass over it: colsum[c]
 * (fp32 [ld], OVERWRITTEN) = sum over rows of the rounded bf16 gradient; row_lse [n_rows] receives the log-sum-exp.
 * workspace: m3p_ce_colsum_workspace_bytes(ld, n_rows) bytes owned by the caller (16-byte aligned). */
/* Log-sum-exp and loss of every row from the 64-column block statistics the vocabulary projection left behind
 * (M3P_EPI_BIAS_LSE): row_lse[r] = log sum_c exp(logit[r, c]), row_loss[r] = row_lse[r] - logits[r, target[r]].
 * stats float2 [n_blocks][n_rows]; scratch: float2 [32][n_rows] (caller-owned).  Replaces the first pass of m3p_ce_fwd_bwd_colsum;
 * follow with m3p_ce_bwd_colsum. */
M3P_API int m3p_ce_lse_from_blocks(const void* stats, int n_blocks, int n_rows, const void* logits, int ld, const int64_t* target,
                                   float* row_loss, float* row_lse, void* scratch, void* stream);
/* The second half of m3p_ce_fwd_bwd_colsum alone: logits <- grad_scale * (softmax - onehot) in place given the rows' log-sum-exp,
 * colsum [ld] <- column sums of the rounded gradient.  Same workspace. */
M3P_API int m3p_ce_bwd_colsum(void* logits, int ld, int n_rows, int V, const int64_t* target, const float* row_lse,
                              float grad_scale, float* colsum, void* workspace, size_t workspace_bytes, void* stream);
M3P_API size_t m3p_ce_colsum_workspace_bytes(int ld, int n_rows);
M3P_API int m3p_ce_fwd_bwd_colsum(void* logits, int ld, int n_rows, int V, const int64_t* target, float* row_loss,
                                  float* row_lse, float grad_scale, float* colsum, void* workspace,
                                  size_t workspace_bytes, void* stream);

/* Cross-entropy of the tied vocabulary projection WITHOUT a gradient pass over the logits (PredLayer, transformer.py:104-117, and
 * its autograd).  Softmax is invariant under a per-row shift and its normaliser is a per-row scalar, so the projection stores
 * e[n, v] = bf16(exp(x[n, v] - c_n)) once (M3P_EPI_BIAS_LSE with row_ref; exact 0 at v = y_n and v >= V) and 1 / sum(e) is applied
 * to the small [n, d] operands of the two gradient products.  With t_n = h_n . E[y_n] + b[y_n] in fp32, c_n = t_n + 40 (the row
 * maximum is at least t_n: the largest stored value of a row is at least e^-40, bf16's normal range reaches e^-87; the fp32 row sum
 * overflows only past a loss of ~116 nats and then yields a NON-FINITE loss, never a finite wrong one), gs = grad_scale:
 *   Sigma_n = sum_v e[n, v] + exp(-40),  loss_n = 40 + log Sigma_n,  s_n = gs / Sigma_n,  q_n = gs * expm1(-loss_n)
 *   db = g * (sum_n s_n e[n, :]) ; db[y_n] += g q_n        dE = e^T x bf16(g s_n H[n, :]) ; dE[y_n, :] += g q_n H[n, :]
 *   dH[n, :] = bf16(g * (s_n (e x E)[n, :] + q_n E[y_n, :]))         (g = the upstream gradient, a device scalar)
 * Every entry point is one launch (m3p_ce_shift_colsum: the tile pass + its fold), reads g from device memory where it needs it
 * and never synchronises with the host. */
/* (a) row_t[n] = t_n, row_ref[n] = {t_n + 40, y_n}: one wave per row.  h bf16 [n_rows, d], emb bf16 [V, d], bias fp32 [V]; d % 4 == 0 */
M3P_API int m3p_ce_shift_target(const void* h, const void* emb, const float* bias, const int64_t* target, float* row_t, void* row_ref,
                                int n_rows, int d, void* stream);
/* (b) folds the block sums (float [n_blocks][n_rows], n_rows % 64 == 0) into row_loss, row_s, row_q [n_rows]; scratch: float
 * [32][n_rows] owned by the caller */
M3P_API int m3p_ce_shift_rows(const void* stats, int n_blocks, int n_rows, float grad_scale, float* row_loss, float* row_s,
                              float* row_q, void* scratch, void* stream);
/* (c) colsum[v] (fp32 [ld], OVERWRITTEN) = sum_n row_s[n] * e[n, v]: one read-only pass over e (bf16 [n_rows, ld]); workspace as
 * for m3p_ce_bwd_colsum (m3p_ce_colsum_workspace_bytes) */
M3P_API int m3p_ce_shift_colsum(const void* e, int ld, int n_rows, const float* row_s, float* colsum, void* workspace,
                                size_t workspace_bytes, void* stream);
/* (d) out[n, :] = bf16(g[0] * row_s[n] * h[n, :]) - the second operand of the weight-gradient product.  d % 4 == 0 */
M3P_API int m3p_ce_shift_scale_rows(const void* h, const float* row_s, const float* g, void* out, int n_rows, int d, void* stream);
/* (e) the target's term: demb[y_n, :] (fp32 [V, d]) += g[0] * row_q[n] * h[n, :] and dbias[y_n] += g[0] * row_q[n], fp32 atomics (ids
 * repeat), one wave per row.  Runs AFTER the (stored) weight gradient. */
M3P_API int m3p_ce_shift_target_rows(const void* h, const int64_t* target, const float* row_q, const float* g, float* demb, float* dbias,
                                     int n_rows, int d, void* stream);
/* (f) dh[n, :] = bf16(g[0] * (row_s[n] * dh32[n, :] + row_q[n] * emb[y_n, :])); dh32 fp32 [n_rows, d] = e x E.  d % 4 == 0 */
M3P_API int m3p_ce_shift_dh(const float* dh32, const void* emb, const int64_t* target, const float* row_s, const float* row_q,
                            const float* g, void* dh, int n_rows, int d, void* stream);

/* Label smoothing of the tied vocabulary head (PyTorch's cross_entropy(label_smoothing = eps)) without a pass over the logits
 * (csrc/smooth.hip; not a reference feature).  With e_bar = mean_v E[v, :], b_bar = mean_v b[v] and c = eps / n:
 *   loss_eps = loss + c sum_r (z[r, y_r] - h_r . e_bar - b_bar),   dh_r += c (E[y_r] - e_bar),
 *   dE[v, :] += c (sum_{r: y_r = v} h_r - (1 / V) sum_r h_r),        db[v] += c (count_v - n / V).
 * The target parts of dE and db go through m3p_ce_shift_target_rows, z[r, y_r] comes from m3p_ce_shift_target.
 *
 * m3p_vocab_mean: mean[0 .. d) = e_bar, mean[d] = b_bar from emb bf16 [V, d] (16-byte aligned; exactly V rows are read) and
 * bias fp32 [V].  Two stages in a fixed order, no atomics: the same bits on every run.  m3p_vocab_mean_plan = the number of
 * partial sums per (row of a period of lcm(d, 8) elements, column) the second stage adds up (0: bad shape);
 * workspace >= m3p_vocab_mean_workspace_bytes(V, d), 16-byte aligned, caller owned. */
M3P_API int m3p_vocab_mean_plan(int V, int d);
M3P_API size_t m3p_vocab_mean_workspace_bytes(int V, int d);
M3P_API int m3p_vocab_mean(const void* emb, const float* bias, int V, int d, float* mean, void* workspace, size_t workspace_bytes,
                           void* stream);
/* out[0 .. d) = scale * sum_r h[r, :] (h bf16 [n_rows, d]) in the same fixed order; plan and workspace of
 * m3p_vocab_mean_*(n_rows, d) */
M3P_API int m3p_ls_colsum_rows(const void* h, int n_rows, int d, float scale, float* out, void* workspace, size_t workspace_bytes,
                               void* stream);
/* aux[r] = row_t[r] - h[r, :] . mean[0 .. d) - mean[d]  (fp32; row_t = m3p_ce_shift_target's target logits).  d % 4 == 0 */
M3P_API int m3p_ls_row_aux(const void* h, const float* mean, const float* row_t, float* aux, int n_rows, int d, void* stream);
/* out[0] = scale * sum_r v[r] (fp32), one block in a fixed order: the rows' aux terms into the loss, the same bits on every run */
M3P_API int m3p_ls_sum_rows(const float* v, int n, float scale, float* out, void* stream);
/* m3p_ce_shift_dh with the smoothing operand: dh[n, :] = bf16(g[0] * (row_s[n] * dh32[n, :] + (row_q[n] + c) * emb[y_n, :]
 * - c * mean[0 .. d))), one rounding per element.  row_s / row_q NULL: 1 / 0 (dh32 is the plain routes' dlogits x E). */
M3P_API int m3p_ce_shift_dh_smooth(const float* dh32, const void* emb, const int64_t* target, const float* row_s, const float* row_q,
                                   const float* g, const float* mean, float c, void* dh, int n_rows, int d, void* stream);
/* dst[v, :] (fp32 [V, d], 16-byte aligned) += g[0] * u[0 .. d) and dbias[v] += g[0] * db for v < V: one grid-stride stream of
 * 16-byte accesses; nothing at or behind row V is touched.  d % 4 == 0.  m3p_ls_uniform_add_plan = the grid's blocks of 256
 * threads (0: bad shape) - a shape with more than 256 * blocks chunks of four floats takes a second trip. */
M3P_API int m3p_ls_uniform_add_plan(int V, int d);
M3P_API int m3p_ls_uniform_add(float* dst, float* dbias, const float* u, const float* g, float db, int V, int d, void* stream);

/* Validation scoring in one read-only pass over bf16 logits [n_rows, ld] (V valid columns): what the reference's evaluators take
 * from predict(..., get_scores=True) per batch - `loss.item() * len(y)` and `(word_scores.max(1)[1] == y).sum()`
 * (evaluation/xevaluator.py:433-438, :530-535, :654-659, :757-762, :861-866, :1165-1170; evaluator.py:240-270).
 *   row_loss[r]   = logsumexp(logits[r, :V]) - logits[r, target[r]]                          (fp32)
 *   row_argmax[r] = the LOWEST column c < V at which row r's maximum is attained              (int32)
 * Columns [V, ld) may hold anything (the ragged projection leaves them unwritten): they enter neither the maximum, the sum
 * nor the argmax.  The logits are not written.  No atomics: the caller reduces the per-row outputs.
 * Preconditions of m3p_ce_fwd_bwd: ld % 8 == 0, ld >= V, logits 16-byte aligned, 0 <= target[r] < V; M3P_EINVAL otherwise
 * (the targets are not inspected). */
M3P_API int m3p_ce_eval(const void* logits, int ld, int n_rows, int V, const int64_t* target, float* row_loss,
                        int32_t* row_argmax, void* stream);

/* out[c] += scale * sum_r x[r,c] for c < ncols (x bf16 [n, ld]); scale read from the
 * device scalar *scale_ptr (NULL = 1): the vocabulary-bias gradient colsum(dlogits). */
M3P_API int m3p_colsum_bf16(const void* x, int ld, int n, int ncols, float* out, const float* scale_ptr,
                            void* stream);

/* ------------------------------------------------------------------------------------
 * Optimizer path (Trainer.optimize xtrainer.py:205-243; Adam.step optim.py:45-86)
 * ---------------------------------------------------------------------------------- */

/* *out += sum(g^2) in double (clip_grad_norm_, xtrainer.py:225). n % 4 == 0. */
M3P_API int m3p_sumsq_f32(const float* g, long long n, double* out, void* stream);

/* The same over n_ranges pieces base[starts[r] .. starts[r] + counts[r]) of one buffer (starts / counts: HOST arrays, element
 * units, counts % 4 == 0, pieces 16-byte aligned) in one launch: the sharded data-parallel step (m3p_amd/distributed.py, zero1)
 * owns a piece of every gradient bucket.  clip_grad_norm_, xtrainer.py:225. */
M3P_API int m3p_sumsq_ranges_f32(const float* base, const long long* starts, const long long* counts, int n_ranges, double* out,
                                 void* stream);

/* One fused pass over a flat fp32 range:  g' = g * grad_scale * clip_coef,
 *   clip_coef = min(1, max_norm / (sqrt(*gnorm_sq) * grad_scale + 1e-6))   (if gnorm_sq && max_norm > 0)
 *   m = b1 m + (1-b1) g';  v = b2 v + (1-b2) g'^2;  p -= wd*lr*p;  p -= step_size * m / (sqrt(v) + eps)
 * step_size = lr * sqrt(1-b2^t)/(1-b1^t) is computed by the caller (optim.py:78-80).
 * Also refreshes the bf16 working copy w16 (if not NULL) and zeroes g (if zero_grad). */
M3P_API int m3p_adam_step(float* p, float* g, float* m, float* v, void* w16, long long n, float lr, float beta1,
                          float beta2, float eps, float weight_decay, float step_size, const double* gnorm_sq,
                          float max_norm, float grad_scale, int zero_grad, void* stream);
/* The same update over n_ranges pieces [starts[r], starts[r] + counts[r]) (elements, multiples of 4) of the SAME flat arenas in
 * one launch; step_sizes / zero_grad per piece (pieces of parameters with different update counts have different bias
 * corrections; a piece whose gradient the next step overwrites need not be zeroed).  starts / counts / step_sizes / zero_grad
 * are HOST arrays, read before the call returns.  p, g, m, v, w16 are the arenas' bases. */
M3P_API int m3p_adam_step_ranges(float* p, float* g, float* m, float* v, void* w16, const long long* starts,
                                 const long long* counts, const float* step_sizes, const int* zero_grad, int n_ranges,
                                 float lr, float beta1, float beta2, float eps, float weight_decay, const double* gnorm_sq,
                                 float max_norm, float grad_scale, void* stream);

/* LAMB on the flat arenas: Adam's moments, then a layer-wise trust ratio on the update.  The rule, for every parameter tensor t
 * that received a gradient since the last zero_grad (Adam's "touched" rule), s = the tensor's step count after the increment,
 * coef = grad_scale * clip_coef exactly as m3p_adam_step forms it:
 *
 *   g' = coef * g
 *   m  = beta1 * m + (1 - beta1) * g'
 *   v  = beta2 * v + (1 - beta2) * g' * g'
 *   r  = (m / (1 - beta1^s)) / (sqrt(v / (1 - beta2^s)) + eps)  +  wd_t * p
 *   phi_t = ||p_t||_2 / ||r_t||_2    if adapt_t and both norms > 0, else 1
 *   p  = p - lr * phi_t * r
 *
 * ||p_t|| is taken on the fp32 master BEFORE the update.  A tensor is one parameter's range of the arena (its zero padding
 * may be included: it adds nothing to either norm); under the sharded data-parallel exchange a tensor's norms are the sums
 * over all ranks' shards.  Excluded tensors (by default those with fewer than two dimensions: biases, LayerNorm weights, the
 * ITM score vector - the BERT convention) have wd_t = 0 and adapt_t = 0.  Untouched tensors are skipped entirely.
 *
 * Three launches however many tensors are active: m3p_lamb_update (m, v; r written over the gradient, which is dead after
 * this pass; one (sum p^2, sum r^2) pair per workgroup), m3p_lamb_norms (each tensor's pairs added in a fixed order to one
 * fp64 pair; no floating-point atomics - the same state and gradients give the same bits), m3p_lamb_apply (p, the bf16
 * working copy, zeros over r where the piece says so).  Between norms and apply a sharded rank sums the norms table over the
 * ranks.
 *
 * The pieces - ranges [start, start + count) of the arenas, each inside one tensor; a tensor is cut where the lazily zeroed
 * vocabulary range or a shard of the sharded exchange begins or ends - are described by a table in DEVICE memory that the
 * caller keeps for as long as the set of pieces stays the same.  m3p_lamb_table_build (host only, no GPU call) validates
 * the pieces and fills the table's host image; the caller copies both arrays to the device:
 *   pieces_out       n_pieces entries of M3P_LAMB_PIECE_BYTES: { int64 first quad; int64 quads; int32 tensor; int32 zero_grad;
 *                    int32 class; int32 first workgroup }
 *   tensor_blk0_out  int32 [n_tensors + 1]: tensor t's workgroups are [tensor_blk0[t], tensor_blk0[t + 1])
 *   *n_blocks_out    workgroups of the update and apply launches; the workspace `partials` holds 2 doubles for each
 * Pieces must come in arena order, disjoint, with borders on multiples of 4 elements, inside [0, arena_elems), the pieces of
 * one tensor adjacent (tensor_ids non-decreasing); class_ids < n_classes <= M3P_LAMB_MAX_CLASSES.  Anything else returns
 * M3P_EINVAL and nothing has run.  max_blocks <= 0: the default cap of 4096 workgroups (every piece gets at least one).
 *
 * The scalars that differ between the tensors of one launch travel by value, one set per class (HOST arrays of n_classes):
 * rbc1 = 1 / (1 - beta1^s), rbc2 = 1 / (1 - beta2^s), wd = wd_t, adapt = adapt_t. */
#define M3P_LAMB_PIECE_BYTES 32
#define M3P_LAMB_MAX_CLASSES 32
M3P_API int m3p_lamb_table_build(const long long* starts, const long long* counts, const int* tensor_ids, const int* zero_grad,
                                 const int* class_ids, int n_pieces, int n_tensors, int n_classes, long long arena_elems,
                                 int max_blocks, void* pieces_out, int* tensor_blk0_out, int* n_blocks_out);
/* p, g, m, v: the arenas' bases (16-byte aligned); pieces: the DEVICE copy of pieces_out; partials: double [n_blocks][2]. */
M3P_API int m3p_lamb_update(float* p, float* g, float* m, float* v, const void* pieces, int n_pieces, int n_blocks,
                            const float* rbc1, const float* rbc2, const float* wd, const int* adapt, int n_classes, float beta1,
                            float beta2, float eps, const double* gnorm_sq, float max_norm, float grad_scale, double* partials,
                            void* stream);
/* norms[t] = (sum p^2, sum r^2) of tensor t's workgroups, double [n_tensors][2]; tensor_blk0: the DEVICE copy. */
M3P_API int m3p_lamb_norms(const double* partials, const int* tensor_blk0, int n_tensors, double* norms, void* stream);
/* r: the gradient arena's base, holding r since m3p_lamb_update; w16 nullable. */
M3P_API int m3p_lamb_apply(float* p, float* r, void* w16, const void* pieces, int n_pieces, int n_blocks, const double* norms,
                           const int* adapt, int n_classes, float lr, void* stream);

/* Non-finite guard of the optimizer step: the decision "skip this step" taken on the device from the reduced gradient norm,
 * with no host read.  m3p_step_guard is one single-thread launch in front of a step's update launches:
 *   gnorm_sq   HOST array of n_arenas DEVICE pointers, each to the double that m3p_sumsq_* reduced for one arena of the
 *              optimizer (all ranks' shards summed where the gradients are sharded).  1 <= n_arenas <= M3P_GUARD_MAX_ARENAS;
 *              more returns M3P_ENOTIMPL.
 *   attempt    the step's attempt index (the host counts every step() call, skipped or not), >= 0.
 * It writes, with plain stores from one thread (device memory, all of it caller-zeroed before the first attempt):
 *   *skip                         1 if any of the sums is NaN or +-inf as a double, else 0
 *   ring[attempt & 63]            the same value (M3P_GUARD_RING entries)
 *   norm_ring[attempt & 63]       sqrt(sum of the sums) * grad_scale, the global gradient norm (non-finite on a skipped step)
 *   counters[0 .. 2]              attempts, skipped_total, skipped_in_a_row (+1 each as they apply; a finite step resets the last)
 * The _guarded forms of the update launches below take that `skip`.  skip == NULL is the unguarded launch, the same kernel and
 * the same bits.  With *skip == 0 the update is the unguarded one, bit for bit.  With *skip != 0 a launch stores nothing to p,
 * m, v, w16, partials or norms; the pieces whose zero_grad flag is set get zeros STORED over their gradient (by
 * m3p_adam_step_ranges_guarded, and by m3p_lamb_apply_guarded for LAMB - the update and norms launches return at once), pieces
 * whose flag is clear are not touched.  The branch is uniform per workgroup and comes before the first load of an arena: a
 * skipped step costs one write of the gradient arena and no read. */
#define M3P_GUARD_MAX_ARENAS 8
#define M3P_GUARD_RING 64
M3P_API int m3p_step_guard(const double* const* gnorm_sq, int n_arenas, float grad_scale, long long attempt, int* skip, int* ring,
                           double* norm_ring, long long* counters, void* stream);
M3P_API int m3p_adam_step_ranges_guarded(float* p, float* g, float* m, float* v, void* w16, const long long* starts,
                                         const long long* counts, const float* step_sizes, const int* zero_grad, int n_ranges,
                                         float lr, float beta1, float beta2, float eps, float weight_decay, const double* gnorm_sq,
                                         float max_norm, float grad_scale, const int* skip, void* stream);
M3P_API int m3p_lamb_update_guarded(float* p, float* g, float* m, float* v, const void* pieces, int n_pieces, int n_blocks,
                                    const float* rbc1, const float* rbc2, const float* wd, const int* adapt, int n_classes,
                                    float beta1, float beta2, float eps, const double* gnorm_sq, float max_norm, float grad_scale,
                                    double* partials, const int* skip, void* stream);
M3P_API int m3p_lamb_norms_guarded(const double* partials, const int* tensor_blk0, int n_tensors, double* norms, const int* skip,
                                   void* stream);
M3P_API int m3p_lamb_apply_guarded(float* p, float* r, void* w16, const void* pieces, int n_pieces, int n_blocks,
                                   const double* norms, const int* adapt, int n_classes, float lr, const int* skip, void* stream);

/* Exponential moving average (Polyak averaging) of the fp32 master on the flat arenas.  Both calls stream over n_ranges pieces
 * [starts[r], starts[r] + counts[r]) of the arenas whose bases they are given, laid out like m3p_adam_step_ranges: starts /
 * counts are HOST arrays in elements, read before the call returns; every start and count a multiple of 4, counts >= 0 (a
 * zero-length piece is skipped); bases 16-byte aligned (w16: 8).  Anything else returns M3P_EINVAL and nothing has run.  32
 * pieces go into one launch, a longer list into several.  Nothing outside the pieces is read or written.
 *
 * m3p_ema_update:  ema[i] = ema[i] + w * (p[i] - ema[i]),  w = (float)(1.0 - decay) formed in double by the caller.  The
 * difference is rounded to fp32, then product and sum are ONE fused multiply-add, fma(w, p[i] - ema[i], ema[i]), whatever
 * the build's contraction setting: the rule is one fixed fp32 arithmetic (w = 1 does NOT give ema = p for every pair; a
 * caller that wants a copy copies).  skip: the non-finite guard's device word (m3p_step_guard) or NULL.  A non-NULL word that reads non-zero makes
 * every workgroup return before it loads anything: ema keeps its bits.
 *
 * m3p_ema_swap:  p[i] <-> ema[i], and w16[i] = bf16(new p[i]) (round to nearest even, the conversion m3p_adam_step_ranges
 * uses; w16 nullable) - one pass that reads two streams and writes three.  Values are moved, never computed with: NaN
 * payloads, infinities, denormals and signed zeros pass through, and two swaps in a row restore p, ema and w16 to the bit. */
M3P_API int m3p_ema_update(const float* p, float* ema, const long long* starts, const long long* counts, int n_ranges, float w,
                           const int* skip, void* stream);
M3P_API int m3p_ema_swap(float* p, float* ema, void* w16, const long long* starts, const long long* counts, int n_ranges,
                         void* stream);

/* h = gelu_erf(u) elementwise (transformer.py:56 applied to the lin1 output :223-224), bf16,
 * n % 8 == 0.  Used instead of M3P_EPI_BIAS_GELU when the GEMM is persistent.
 * dh (nullable, may alias u): also writes gelu_erf'(u) in bf16, which the backward FFN dgrad
 * then applies with M3P_EPI_MUL instead of recomputing the derivative in the GEMM epilogue. */
M3P_API int m3p_gelu_fwd(const void* u, void* h, void* dh, long long n, void* stream);
/* The same activation for the persistent-GEMM FFN (transformer.py:223-225, gelu :48-56) leaving what backward needs in ONE
 * byte per element: h (bf16 [M, N], contiguous) = gelu_erf(u), gq (uint8, M * N bytes) = gelu_erf'(u) quantised to the
 * grid (code - 27) / 200 (0 and 1 exact, |error| <= 2.5e-3), stored in the fragment order of the eight-wave NT GEMM's 256 x 256 tiles
 * so that the FFN data gradient m3p_gemm_nt_bf16(..., M3P_EPI_MULQ, aux = gq) multiplies by it without a layout change.
 * u itself is not needed after this call.  M % 256 == 0, N % 256 == 0; u, h contiguous and 16-byte aligned. */
M3P_API int m3p_gelu_fwd_gq(const void* u, void* h, void* gq, int M, int N, void* stream);
/* The same pass also writing h8 = e4m3(scale * h) (uint8 [n]) and raising *amax to max |h| (nullable): the operand of the
 * fp8 lin2 product without a second pass over h (m3p_quant_fp8 of h gives the same bytes). */
M3P_API int m3p_gelu_fwd_q8(const void* u, void* h, void* h8, long long n, const float* scale, float* amax, void* stream);

/* du = dy * gelu_erf'(u) elementwise (backward of the GELU inside BertPredictionHeadTransform,
 * transformer.py:595-606, for the masked-region classification head), bf16, n % 8 == 0. */
M3P_API int m3p_gelu_bwd(const void* dy, const void* u, void* du, long long n, void* stream);

/* Masked-region feature regression loss (F.mse_loss of xtrainer.py:2346 on the gathered masked rows):
 * row_sq[i] = sum_j (pred[i][j] - tgt[i][j])^2 (the caller divides the total by rows*cols) and
 * dpred[i][j] = 2 (pred - tgt) * grad_scale.  pred/dpred bf16 (pitch ld_pred), tgt fp32 (pitch ld_tgt). */
M3P_API int m3p_mse_fwd_bwd(const void* pred, int ld_pred, const float* tgt, int ld_tgt, void* dpred, float* row_sq,
                            int rows, int cols, float grad_scale, void* stream);

/* ------------------------------------------------------------------------------------
 * AoA image refiner (AoA_Refiner_Core, transformer.py:287-422): the elementwise passes its GEMMs,
 * LayerNorms, attention and GELU (all the encoder's kernels) leave over.
 * ---------------------------------------------------------------------------------- */

/* y[r][c] = (res ? res[r][c] : 0) + dropout(x[r][c]) on a [rows, cols] bf16 view (pitches ldx / ldres / ldy,
 * cols % 4 == 0).  The keep decision of element (r, c) is m3p_keep(r * rng_ld + rng_col0 + c, seed, thresh24)
 * (thresh24 = 0: no dropout), so the two halves of torch.cat([x, q], -1) can be dropped by two calls into one
 * [rows, 2d] buffer (rng_ld = 2d, rng_col0 = 0 / d) and backward regenerates the same mask.  y may alias x.
 * SublayerConnection.forward (:392-394), MultiHeadedDotAttention's dropout_aoa (:366), TransformerFFN (:226). */
M3P_API int m3p_dropout_rows(const void* x, int ldx, const void* res, int ldres, void* y, int ldy, int rows, int cols,
                             uint32_t rng_ld, uint32_t rng_col0, uint32_t seed, uint32_t thresh24, float inv_keep,
                             void* stream);

/* nn.GLU of the AoA layer (:317): ab bf16 [rows, 2d] (pitch ld_ab) -> y[rows, d] = ab[:, :d] * sigmoid(ab[:, d:]) */
M3P_API int m3p_glu_fwd(const void* ab, int ld_ab, void* y, int rows, int d, void* stream);
/* dab[:, :d] = dy * sigmoid(b);  dab[:, d:] = dy * a * sigmoid(b) * (1 - sigmoid(b))   (dab pitch = ld_ab) */
M3P_API int m3p_glu_bwd(const void* ab, int ld_ab, const void* dy, void* dab, int rows, int d, void* stream);

/* Batched form of m3p_transpose_bf16: desc = n_desc x {src ptr, dst ptr, rows, cols, ld_src,
 * ld_dst} as int64 in device memory; max_tiles >= max over matrices of ceil(rows/64)*ceil(cols/64). */
M3P_API int m3p_transpose_batch_bf16(const long long* desc, int n_desc, int max_tiles, void* stream);

/* dst[c, r] = src[r, c] (bf16): transposed weight copies for the data-gradient GEMMs */
M3P_API int m3p_transpose_bf16(const void* src, void* dst, int rows, int cols, int ld_src, int ld_dst,
                               void* stream);

/* Size of the persistent GEMM grids (process-wide; 0 = one workgroup per CU, the default; a multiple of 8: tiles are dealt
 * out per XCD).  Data parallelism sets num_CUs - r so that RCCL's r channels find free CUs while a GEMM runs - a persistent
 * workgroup fills its CU's LDS and registers, nothing co-resides with it (m3p_amd/distributed.py). */
M3P_API int m3p_set_persistent_grid(int workgroups);
/* Dynamic tile queues for the persistent NT GEMM (process-wide; counters = NULL switches back to the static schedule).
 * counters: n_slots x 8 int32 in device memory, zeroed by the caller once; every eligible m3p_gemm_nt_bf16 launch (eight-wave
 * kernel, more output tiles than workgroups, K >= 512) takes the next slot - one counter per XCD - and its workgroups pop
 * their output tiles from per-XCD queues instead of a fixed round-robin share, so a CU that runs slower (a collective's kernel
 * resident beside the GEMM under data parallelism) takes fewer tiles instead of stretching the launch.  The ring binds to the
 * stream of the first queued launch after this call and is cleared by a memset on that stream when it wraps; launches on any
 * other stream take the static schedule (never a slot another stream's kernel may still be popping from).  Slot hand-out is
 * serialised inside the library; call this setter with no GEMM of the old ring in flight.  Results are the static schedule's. */
M3P_API int m3p_set_tile_queue(int32_t* counters, int n_slots);

/* Which kernel a product of this shape WOULD run on, given the process-wide switches above (no launch, no device access): the
 * dispatch tables in csrc/gemm.hip (nt_plan / wgrad_plan) are the single place that decides, the launchers switch on the same
 * value.  Tests use it to assert that a model-level parity case really exercised the kernel family the benchmark runs on
 * (tests/test_model_parity.py[tiles]) and that a launch under the two switches really ran the schedule it is checked for
 * (tests/test_gemm_schedules.py).  Returns an M3P_KERN_* id, or M3P_EINVAL for a shape the entry point would refuse.
 * m3p_gemm_wgrad_plan assumes 16-byte aligned operands with pitches that are multiples of 8. */
enum {
  M3P_KERN_NT_SKINNY = 1,        /* M <= 128: fragments straight from global memory                       */
  M3P_KERN_NT_W8 = 2,            /* eight waves, 256 x 256 tile, 128 x 64 per wave                         */
  M3P_KERN_NT_W8_QUEUE = 3,      /* the same with per-XCD dynamic tile queues (m3p_set_tile_queue)         */
  M3P_KERN_NT_W4 = 4,            /* four waves, 256 x 256 tile, 128 x 128 per wave (K >= 2048)             */
  M3P_KERN_NT_RING = 5,          /* eight waves, 256 x 128 tile, three-stage ring: ragged shapes           */
  M3P_KERN_NT_128 = 6,           /* 128 x 128, two stages: M < 1024                                        */
  M3P_KERN_WGRAD_W4_CHUNKS = 10, /* four waves, one (tile, M-chunk) segment per workgroup + ordered reduce kernel */
  M3P_KERN_WGRAD_W4_TILES = 11,  /* four waves, whole tiles round-robin (the vocabulary matrix)            */
  M3P_KERN_WGRAD_RING = 12,      /* stream-K 256 x 128 with fp32 atomics: ragged N / K                     */
  M3P_KERN_WGRAD_128 = 13        /* 128 x 128 split-M: small M                                             */
};
M3P_API int m3p_gemm_nt_plan(int M, int N, int K, int epilogue);
M3P_API int m3p_gemm_wgrad_plan(int M, int N, int K);

/* Developer switch (process-wide, NEVER called by the product; tests/test_gemm.py and tools/ab_*.py use it): 1 = the tables
 * above (default), 2 = four-wave NT wherever it applies, 6 = eight-wave NT wherever it applies; any other value means 1.
 * Every launch reads it: set it only with no GEMM call in flight. */
M3P_API void m3p_debug_set_variant(int v);
/* The same kind of switch for the attention backward of the M3P sequence (tests/test_attention.py, tools/ab_attn.py):
 * 0 = the persistent one-pass form (default), bit 0 = the two-phase form (scores recomputed in both phases, rounds 1-4),
 * bit 1 = the plain one-pass form. */
M3P_API void m3p_debug_attn_variant(int v);

/* ------------------------------------------------------------------------------------
 * Host-glue kernels (csrc/glue.hip): index / mask / loss arithmetic the reference does with chains of elementwise
 * tensor ops around the hot path; one launch each, no host reads.
 * ---------------------------------------------------------------------------------- */
/* get_masks (transformer.py:59-78) for the prefix mask of jointfwd (:917-919): totlen[b] = lengths[b] (+ lengths_b[b]
 * when given), rowmask[b*S + s] = s < totlen[b] */
M3P_API int m3p_seq_masks(const int64_t* lengths, const int64_t* lengths_b, int B, int S, int32_t* totlen,
                          uint8_t* rowmask, void* stream);
/* The boolean gather of :1208 as row numbers: the k-th True entry (flat order i = t * inner + b) of mask [n_mask] ->
 * rows[k] = (soff + t * s0 + b * s1) / d, the row of that position in the [*, d] buffer under a strided (T, B, d) view
 * (element strides s0, s1, storage offset soff).  n_rows = the caller's count of True entries (host knowledge); a
 * shorter mask leaves the tail at row 0.  n_mask <= 2^20. */
M3P_API int m3p_mask_to_rows(const uint8_t* mask, int n_mask, int inner, long long s0, long long s1, long long soff,
                             int d, int32_t* rows, int n_rows, void* stream);
/* out[(i0 * n1 + i1), :] (bf16, contiguous) = in[i0 * s0 + i1 * s1 + (0 .. cols)] (fp32): the region features through
 * the transposed view the model is handed (transformer.py:897-898) without materialising it.  cols, s0, s1 % 4 == 0 */
M3P_API int m3p_cast_rows_f32_bf16(const float* in, long long s0, long long s1, int n0, int n1, int cols, void* out,
                                   void* stream);
/* out (bf16) = g[0] * in (bf16, or fp32 when in_is_f32), g a DEVICE scalar (an upstream gradient); n % 4 == 0 */
M3P_API int m3p_scale_bf16_dev(const void* in, int in_is_f32, const float* g, void* out, long long n, void* stream);
/* dst += g[0] * src (fp32), g a device scalar */
M3P_API int m3p_axpy_dev_f32(float* dst, const float* src, const float* g, long long n, void* stream);
/* ITM loss of xtrainer.py:2357-2372 on the device: scores fp32 [n_groups * sample_n], pos int64 [n_groups];
 * loss[0] = w_ce * CE(scores.view(-1, sample_n), pos) + w_bce * BCEWithLogits(scores, one_hot(pos)) (both means);
 * dscores = d loss / d scores */
M3P_API int m3p_itm_loss_fwd_bwd(const float* scores, const int64_t* pos, int n_groups, int sample_n, float w_ce,
                                 float w_bce, float* loss, float* dscores, void* stream);

/* ------------------------------------------------------------------------------------
 * Hardware-semantics probes (used by tests/test_hw_probes.py only): each fills `out`
 * with what the instruction delivered so the test can compare with the documented map.
 * ---------------------------------------------------------------------------------- */
M3P_API int m3p_probe_mfma_16x16x32(const void* a_rowmajor_16x32, const void* b_colmajor_32x16,
                                    float* d_16x16, int* d_rowcol, void* stream);
/* v_mfma_scale_f32_16x16x128_f8f6f4 with unit block scales: a, w row-major 8-bit [16,128] (a: fp8 e4m3, or bf8 e5m2
 * when a_is_bf8; w: fp8 e4m3), d fp32 [16,16] = a w^T written through the 16x16 result map */
M3P_API int m3p_probe_mfma_fp8_16x16x128(const void* a_16x128, const void* w_16x128, float* d_16x16, int a_is_bf8,
                                         void* stream);
M3P_API int m3p_probe_tr16(const void* tile_bf16_64x16, void* out_64x4, void* stream);
/* v_permlane16_swap_b32 x, y with (x, y) = (lane, 100 + lane): out[lane] = x, out[64 + lane] = y afterwards - the odd 16-lane rows
 * of x trade places with the even rows of y (what the persistent attention backward's widened row stores rest on) */
M3P_API int m3p_probe_permlane16_swap(void* out_2x64_u32, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* M3P_HIP_H */
