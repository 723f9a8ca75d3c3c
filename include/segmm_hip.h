/* segmm_hip.h -- C ABI of libsegmm_hip.so, the MI355X (gfx950) kernels of the segment-interest training path.
 *
 * The reference (hezy18/SegMMInterest) is pure Python/PyTorch and has NO native boundary; its boundary is the
 * Python plugin surface `MMinterest/models/__init__.py:1-5`.  This header defines the native layer UNDERNEATH that
 * surface: each entry point replaces the chain of stock ATen ops the reference executes at the
 * cited file:line.  Host bindings: `segmminterest_amd/hipabi.py` (ctypes); INTEGRATION.md shows the stub a
 * maintainer of the reference adds.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer owned by the caller (PyTorch); the library allocates nothing persistent,
 *    keeps no mutable global state and never synchronises: it only enqueues on `stream` (a hipStream_t);
 *  - fp32 row-major everywhere; feature/leading dimensions must be multiples of 4 floats and 16-byte aligned;
 *  - return value 0 = ok, negative = error (message via segmm_last_error(), thread local); nothing throws;
 *  - re-entrant: forward runs on the Python thread, backward on an autograd-engine thread;
 *  - dropout is a counter-based hash stream addressed by (seed, site, element index): with p = 0 results are
 *    bitwise reproducible run to run; with p > 0 they are reproducible for a fixed (seed, site).
 */
#ifndef SEGMM_HIP_H
#define SEGMM_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef void* segmm_stream_t; /* hipStream_t */

const char* segmm_last_error(void);
#define SEGMM_ABI_VERSION 30
int segmm_abi_version(void); /* SEGMM_ABI_VERSION of the header the library was built from */

/* a1 -- trainer L1 normalisation  x / (sum|x| + 1e-6)  (main_for_seq_leave_earlystop_SegMM.py:272-273).
 * y may be NULL: then only inv_scale[row] = 1/(sum|x|+1e-6) is produced, for the fused a1+a2 GEMM (row_scale) -- or, with a
 * plane output, the normalised rows are written as planes only (|y| <= 1: with *scale_in = 2^14 the planes can neither overflow
 * nor fall below the fp16 window, so their consumers need no fp32 copy to fall back on).
 * amax: optional zeroed [SEGMM_AMAX_SLOTS] array receiving the partial maxima of |y| (see segmm_gemm_h). */
int segmm_l1norm(const float* x, float* y, float* inv_scale, int64_t rows, int D, float* amax, uint16_t* planes, int ld2, float* hdr,
                 const float* scale_in, segmm_stream_t stream);
/* 16-BIT INPUT FEATURES.  The two kernels at the front of the step -- this normalisation (host-fed batches) and segmm_gather_l1 (the
 * resident table) -- also take their INPUT as IEEE half or bfloat16: half the bytes over PCIe, half the table in HBM.  `elem` names
 * the element type of the 16-bit words; any other value is an error return, never a launch.  Every element is widened to fp32
 * exactly (both formats embed in fp32) and the fp32 kernel's arithmetic follows, so the outputs -- fp32 rows, masks, maxima, planes
 * -- are those of the fp32 entry point on the widened input, bit for bit.  x / table: 8-byte aligned, D % 4 == 0 (rows of a 16-bit
 * tensor are 8-byte aligned only); every other argument as in the fp32 entry point. */
#define SEGMM_ELEM_F16 1
#define SEGMM_ELEM_BF16 2
int segmm_l1norm_h(const uint16_t* x, int elem, float* y, float* inv_scale, int64_t rows, int D, float* amax, uint16_t* planes, int ld2,
                   float* hdr, const float* scale_in, segmm_stream_t stream);
/* 8-BIT INPUT FEATURES.  The same two kernels take their input as OCP e4m3fn, OCP e5m2 (gfx950's fp8 / bf8; not MI300's fnuz
 * encodings) or int8: a quarter of float32's bytes.  Every code of the three formats is an exact fp32 value, so the definition of the
 * 16-bit forms carries over unchanged: every output is the fp32 entry point's on the exactly widened input, bit for bit (NaN codes
 * widen to NaN, e5m2's inf codes to inf).  No scale travels with a row: the rows are L1-normalised as they are read, which cancels
 * a per-row scale up to the 1e-6 of the denominator; with normalize == 0 (segmm_gather_l1_b) the codes ARE the values.  `elem` is
 * one of the three constants below; 1 and 2 belong to the _h forms, which keep refusing everything else.  x / table: 4-byte aligned,
 * D % 4 == 0 (rows of an 8-bit tensor are 4-byte aligned only); every other argument as in the fp32 entry point. */
#define SEGMM_ELEM_E4M3 3
#define SEGMM_ELEM_E5M2 4
#define SEGMM_ELEM_I8 5
int segmm_l1norm_b(const uint8_t* x, int elem, float* y, float* inv_scale, int64_t rows, int D, float* amax, uint16_t* planes, int ld2,
                   float* hdr, const float* scale_in, segmm_stream_t stream);
/* The loader of an 8-bit table: float32 rows x [rows, D] -> codes q [rows, D] of type `elem`, one wave per row.  With a = max|x_j|
 * (a < 2^-100 or not finite: all-zero codes, scale 0), the row is multiplied by s = 2^(8-e) (e4m3) / 2^(15-e) (e5m2), a = m 2^e with
 * 0.5 <= m < 1 -- exact, |x s| < 256 / 32768, far inside either format -- or by r = 127 / a (int8), and every product is rounded to
 * nearest, ties to even.  scale_out: optional, one float per row, the factor the row was multiplied by (the codes do not need it under
 * L1 normalisation).  x: 16-byte aligned, q: 4-byte aligned, D % 4 == 0. */
int segmm_quantize_rows(const float* x, int64_t rows, int D, int elem, uint8_t* q, float* scale_out, segmm_stream_t stream);
/* PLANE OUTPUTS of producers (the four trailing arguments `planes, ld2, hdr, scale_in` of segmm_l1norm, segmm_gather_l1,
 * segmm_layernorm_fwd / _bwd; segmm_attn_planes_t; c_planes / c_hdr / c_scale_in of segmm_gemm_p): a kernel that writes a
 * tensor some GEMM reads can also write that tensor's P32 fp16 planes (format: segmm_gemm_p) with the DELAYED scale
 * *scale_in -- a device scalar, the power of two that segmm_scales_update derived from the maxima the tensor site had on
 * earlier passes.  The kernel stores the scale it used in hdr[0], folds the partial maxima of what it wrote into the header's
 * slots and raises hdr[1] if an element left the fp16 range (consumers then read the fp32 copy).  planes == NULL, scale_in ==
 * NULL or *scale_in == 0: no planes are written (the caller runs segmm_split_p32 with the exact scale instead). */

/* K2/K3/K5/K6 -- every nn.Linear of the path and its gradients (encoder.py:95-104,163-167,183-184,438,445;
 * kn_util/nn_utils/layers/mlp.py:17-23), on the f32 MFMA.
 *   layout 0 (NT): C[M,N] = A[M,K] . B[N,K]^T    forward, B = Linear.weight
 *   layout 1 (NN): C[M,N] = A[M,K] . B[K,N]      dgrad
 *   layout 2 (TN): C[M,N] = A[K,M]^T . B[K,N]    wgrad (use splits > 1: K is the token dimension)
 * epilogue, in this order: * row_scale[m]; + bias[n]; activation (0 none, 1 erf-GELU saving the pre-activation to
 * aux, 2 multiply by GELU'(aux), 3 ReLU, 4 zero where aux <= 0 -- ReLU backward, aux = the forward output); dropout(p, seed, site) on element m*N+n; + residual[(m % res_period), n].
 * residual may alias C (accumulate).  splits > 1: partial slabs in `workspace` (splits*M*N floats), then a
 * deterministic combine; only `accumulate` (C += result) applies in that mode.
 * engine 0: v_mfma_f32_32x32x2_f32 (exact fp32 products).  engine 1: "bf16x6" -- operands are split exactly into
 * three bf16 terms on the fly and six v_mfma_f32_32x32x16_bf16 partial products are accumulated in fp32 (error below
 * that of a plain fp32 GEMM, 2.67x less matrix-pipe time); same layouts, epilogue and split-K. */
int segmm_gemm(int layout, int M, int N, int K, const float* A, int lda, const float* B, int ldb, float* C, int ldc,
               const float* bias, const float* row_scale, const float* residual, int ldr, int res_period,
               int activation, float* aux, int ldaux, float drop_p, uint64_t seed, uint32_t site, int splits,
               float* workspace, int accumulate, int engine, segmm_stream_t stream);

/* Same GEMM on the bf16x6 engine with optional PRE-SPLIT operands: a_planes / b_planes point at bf16 planes
 * [nplanes][rows][ld] (plane p at base + p*pstride elements, rows k-contiguous, NT layout only) produced by
 * segmm_split3 / segmm_split3_transpose -- the main loop then does no conversion work for that operand.  Weights are
 * split once per optimizer step; W^T planes turn the dgrad (dX = dY.W) into the NT form as well.
 * nplanes = 2 keeps only hi and mid (three partial products, ~2e-5 relative error): offered for weight gradients,
 * which are leaves of the backward graph. */
int segmm_gemm_x(int layout, int M, int N, int K, const float* A, int lda, const float* B, int ldb, float* C, int ldc,
                 const float* bias, const float* row_scale, const float* residual, int ldr, int res_period,
                 int activation, float* aux, int ldaux, float drop_p, uint64_t seed, uint32_t site, int splits,
                 float* workspace, int accumulate, const uint16_t* a_planes, int64_t a_pstride,
                 const uint16_t* b_planes, int64_t b_pstride, int nplanes, segmm_stream_t stream);

/* fp16x3 engine: x*s = hi + lo in two fp16 terms (22 mantissa bits), s a per-tensor power of two derived inside the
 * kernel from PARTIAL MAXIMA of |x| (a_amax[0..a_namax), b_amax[0..b_namax), device arrays written by
 * segmm_absmax or by the operand's producer; no host sync); three products hh + hl + lh on
 * v_mfma_f32_32x32x16_f16, per-product error <= 3 * 2^-22.  Half the matrix-pipe work of segmm_gemm_x.
 * Optional pre-split operands are fp16 planes [2][rows][ld] from segmm_split2h / segmm_split2h_transpose made with
 * the SAME partial maxima that are passed here.  All layouts, epilogues and split-K as segmm_gemm. */
int segmm_gemm_h(int layout, int M, int N, int K, const float* A, int lda, const float* B, int ldb, float* C, int ldc,
                 const float* bias, const float* row_scale, const float* residual, int ldr, int res_period,
                 int activation, float* aux, int ldaux, float drop_p, uint64_t seed, uint32_t site, int splits,
                 float* workspace, int accumulate, const uint16_t* a_planes, int64_t a_pstride,
                 const uint16_t* b_planes, int64_t b_pstride, const float* a_amax, int a_namax, const float* b_amax,
                 int b_namax, float* c_amax, segmm_stream_t stream);

/* Plane-operand GEMM: the fp16x3 arithmetic of segmm_gemm_h with operands that arrive PRE-SPLIT by their producers.
 * P32 plane format of a matrix X[R][C], C % 32 == 0: one fp16 array with row stride ld2 (halves); per row and per block
 * of 32 columns [32 hi | 32 lo] (128 bytes) -- element (r, c): hi at r*ld2 + (c/32)*64 + c%32, lo 32 further.
 * Site header `hdr` of a plane tensor: SEGMM_SITE_HDR floats followed by SEGMM_AMAX_SLOTS partial maxima:
 *   hdr[0] scale s the planes were written with (power of two; 0 = no planes written),
 *   hdr[1] != 0 (as integer): an element left the fp16 range under s (delayed scaling) -> consumers read the fp32 copy.
 * a_f32 / b_f32 (optional): fp32 copy of the operand; taken (exact split on the fly, slow) whenever the planes are not
 * usable -- results are never silently wrong.  Replaces the same reference ops as segmm_gemm (encoder.py:95-104,
 * 163-167,183-184,438,445; kn_util/nn_utils/layers/mlp.py:17-23).
 *   layout 0 (NT): C[M,N] = A[M,K] . B[N,K]^T  A planes [M][2K], B planes [N][2K]          (forward; dgrad on W^T planes)
 *   layout 2 (TN): C[M,N] = A[K,M]^T . B[K,N]  A planes [K][2M], B planes [K][2N], split-K  (weight gradients)
 * Output: fp32 C (unless bit 0 of write_c is clear) and/or P32 planes c_planes written with the scale *c_scale_in; the partial
 * maxima of |C|, the overflow flag and the scale used are folded into c_hdr (caller zeroes the header).  Epilogue as
 * segmm_gemm.  NT: K % 32 == 0; TN: M, N % 32 == 0 (token tails are zero-filled).
 * PLANES-ONLY outputs (round 5; NT, write_c = 0: the projection outputs the planes-in attention kernels read): with no fp32 copy
 * a consumer cannot fall back when the delayed scale turns out wrong, so the caller enqueues the SAME call once more with bit 1
 * of write_c set -- the REPAIR launch: every workgroup judges the output site from c_hdr (scale, flag, complete maxima) and
 * leaves at once when the planes are usable; otherwise it recomputes its tile and rewrites the planes with the exact scale of
 * the recorded maxima, leaving c_hdr untouched.  Consumers judge the same header and derive the same scale. */
#define SEGMM_SITE_HDR 8
int segmm_gemm_p(int layout, int M, int N, int K, const uint16_t* a_planes, int lda2, const float* a_hdr, const float* a_f32, int ldaf,
                 const uint16_t* b_planes, int ldb2, const float* b_hdr, const float* b_f32, int ldbf, float* C, int ldc,
                 uint16_t* c_planes, int ldc2, float* c_hdr, const float* c_scale_in, int write_c, const float* bias, const float* row_scale,
                 const float* residual, int ldr, int res_period, int activation, float* aux, int ldaux, float drop_p,
                 uint64_t seed, uint32_t site, int splits, float* workspace, int accumulate, float* colsum_out, segmm_stream_t stream);
/* colsum_out (TN only, optional): [M] floats receiving sum_k A[k, m] -- the bias gradient of the Linear whose weight gradient
 * the call computes (dW = dY^T . X, db = column sums of dY), formed inside the same kernel (+)= with `accumulate`; with
 * splits > 1 the workspace must hold splits * (M * N + M) floats. */
/* segmm_gemm_p with a PRODUCT COUNT (opt-in mixed precision).  products = 3: segmm_gemm_p itself, which is this call with 3 --
 * same launcher, same kernels, same bits.  products = 1: every plane operand is its hi term, x ~= hi / s (11-bit significand:
 * relative representation error <= 2^-11 while hi is a normal fp16 number); one v_mfma_f32_16x16x32_f16 per k-block, fp32
 * accumulate; the column sums are sum hi / s.  Everything around the products is unchanged: the P32 operands (the lo halves are
 * staged and not read), the operand-state verdicts and the fp32 fallback (split at the exact scale, then one product as well), the
 * epilogue, the outputs (plane outputs carry both planes of the fp32 result), split-K and the combine.  Any other value is an error
 * return that names it, never a launch.  The choice of kernel does not depend on `products`; a launch that falls through to a
 * round-2 kernel (gemm_pl_nt / gemm_pl_tn: row-scaled outputs, a residual together with a d-activation, an extent >= 2^31, TN
 * shapes that are no whole 128 x 256 tiles, the PL_VAR / TN_VAR settings that ask for them) RUNS WITH THREE PRODUCTS whatever is
 * passed.  A repair launch passes the `products` of the launch it repairs. */
int segmm_gemm_pq(int layout, int M, int N, int K, const uint16_t* a_planes, int lda2, const float* a_hdr, const float* a_f32, int ldaf,
                  const uint16_t* b_planes, int ldb2, const float* b_hdr, const float* b_f32, int ldbf, float* C, int ldc,
                  uint16_t* c_planes, int ldc2, float* c_hdr, const float* c_scale_in, int write_c, const float* bias, const float* row_scale,
                  const float* residual, int ldr, int res_period, int activation, float* aux, int ldaux, float drop_p,
                  uint64_t seed, uint32_t site, int splits, float* workspace, int accumulate, float* colsum_out, int products,
                  segmm_stream_t stream);
/* fp32 [rows, cols] (row stride ld) -> P32 planes.  mode 0: exact scale from the header's partial maxima (complete when
 * this runs), written to hdr[0], flag cleared.  mode 1: scale = hdr[0] as given; maxima and flag folded into hdr. */
int segmm_split_p32(const float* x, int64_t rows, int cols, int ld, uint16_t* planes, int ld2, float* hdr, int mode,
                    segmm_stream_t stream);
/* All GEMM weight matrices of a model in two launches per optimizer step (absmax; exact split + transposed split).
 * desc: device array of n_mats records {int64 flat offset (floats); int32 R, C, needs_transpose, first_tile, tile_cols}
 * (32 x 32 tiles, n_tiles in total, matrices in ascending first_tile order); hdr: [n_mats][SEGMM_SITE_HDR +
 * SEGMM_AMAX_SLOTS] zeroed site headers (receive maxima and scale); W planes at wpl + 2 * offset (ld2 = 2 C), W^T planes
 * at wTpl + 2 * offset (ld2 = 2 R).  C % 32 == 0 (and R % 32 == 0 for transposed matrices).  Every record's offset is a
 * multiple of 4 floats (the absmax pass reads 16 bytes at a time; the plane blocks of a matrix then start 16-byte aligned
 * too).  wTpl may be NULL only if no record asks for a transpose.  The headers need no zero-fill between calls: every call
 * rewrites all SEGMM_AMAX_SLOTS maxima, the scale and the flag of every matrix. */
int segmm_wsplit_p32(const float* flat, const void* desc, int n_mats, int n_tiles, float* hdr, uint16_t* wpl, uint16_t* wTpl,
                     segmm_stream_t stream);
/* P32 planes of the transpose of x[R, C]: plane row c holds x[:, c] (R % 32 == 0), scale hdr[0]. */
int segmm_split_p32_transpose(const float* x, int R, int C, int ld, uint16_t* planes, int ld2, const float* hdr,
                              segmm_stream_t stream);
/* Producer side of those partial maxima.  segmm_gemm_h (c_amax), segmm_layernorm_fwd/bwd (amax), segmm_attn_fwd
 * (amax_o) and segmm_attn_bwd (amax_q / amax_ka / amax_kb) take OPTIONAL arrays of SEGMM_AMAX_SLOTS floats that
 * the CALLER HAS ZEROED; each wave folds the maximum of what it stored into one slot with an integer atomic max on
 * the float bits (exact, order-independent, so results stay bitwise reproducible).  Several producers may share
 * one array (the attention backward of both sides writes column blocks of the same dY buffer). */
#define SEGMM_AMAX_SLOTS 256
/* out[0..nparts) = partial maxima of |x| over the [rows, cols] view with row stride ld (1 <= nparts <= 1024). */
int segmm_absmax(const float* x, int64_t rows, int cols, int ld, float* out, int nparts, segmm_stream_t stream);
int segmm_split2h(const float* x, uint16_t* planes, int64_t n, int64_t pstride, const float* amax, int namax,
                  segmm_stream_t stream);
int segmm_split2h_transpose(const float* x, int R, int Cc, int ld, uint16_t* planes, int64_t pstride,
                            const float* amax, int namax, segmm_stream_t stream);
/* exact split x = hi + mid + lo into three bf16 planes: planes[p*pstride + i] (flat), or the transposed copy
 * planes[p*pstride + c*R + r] of an [R, C] row-major matrix with leading dimension ld. */
int segmm_split3(const float* x, uint16_t* planes, int64_t n, int64_t pstride, segmm_stream_t stream);
int segmm_split3_transpose(const float* x, int R, int C, int ld, uint16_t* planes, int64_t pstride, segmm_stream_t stream);

/* LayerNorm(d, eps) forward/backward (encoder.py:39-40,170-171,185-186,203,206,383-385,455,465).
 * forward: optional dropout on the output (embedding dropout, encoder.py:461,471).  y == NULL with a plane output (round 5):
 * PLANES ONLY -- the planes are written with the scale of the output's bound (max|gamma| sqrt(d) + max|beta|) / (1 - p), derived
 * in the kernel (scale_in is ignored) and recorded in hdr[0]: no input can overflow it, so the consumers need no fp32 fallback.
 * backward: dy is first multiplied by the forward's output-dropout mask (drop_y_*); dx_drop (may be NULL) receives
 * dx times the mask of the residual-branch dropout "x = res + dropout(branch)" (drop_b_*), i.e. d(branch).
 * part_dgamma/part_dbeta: [nparts, d] per-workgroup partials, nparts = segmm_layernorm_bwd_parts(rows, d)
 * (one round of the workgroups that are resident at that row width: 768 at d = 768).
 * part_dsum (optional, same shape): partial column sums of the forwarded gradient (dx_drop if given, else dx) =
 * the bias gradient of the Linear whose output entered the LayerNorm through the residual branch. */
int segmm_layernorm_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd,
                        int64_t rows, int d, float eps, float drop_p, uint64_t seed, uint32_t site, float* amax,
                        uint16_t* planes, int ld2, float* hdr, const float* scale_in, segmm_stream_t stream);
/* segmm_layernorm_fwd that also returns dot_out[row] = y[row, :] . dot_w (+ dot_b[0]): the Linear(d, 1) interest head
 * (decoder_leave_focal.py:451,596) applied to the backbone's last LayerNorm output without a second pass over it. */
int segmm_layernorm_fwd_dot(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd,
                            int64_t rows, int d, float eps, float drop_p, uint64_t seed, uint32_t site, float* amax,
                            uint16_t* planes, int ld2, float* hdr, const float* scale_in, const float* dot_w, const float* dot_b,
                            float* dot_out, segmm_stream_t stream);
int segmm_layernorm_bwd_parts(int64_t rows, int d);
int segmm_layernorm_bwd(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma,
                        float* dx, float* dx_drop, float* part_dgamma, float* part_dbeta, float* part_dsum, int64_t rows,
                        int d, float drop_y_p, uint32_t drop_y_site, float drop_b_p, uint32_t drop_b_site, uint64_t seed,
                        float* amax, uint16_t* planes, int ld2, float* hdr, const float* scale_in, segmm_stream_t stream);
/* segmm_layernorm_bwd whose incoming gradient is the outer product dy[row, c] = dy_row[row] * dy_col[c]: what the Linear(d, 1)
 * interest head (decoder_leave_focal.py:451,596) sends into the last LayerNorm of the backbone -- formed inside the launch
 * instead of by segmm_rowscale_bcast (same products, bit-identical results). */
int segmm_layernorm_bwd_outer(const float* dy_row, const float* dy_col, const float* x, const float* mean, const float* rstd, const float* gamma,
                              float* dx, float* dx_drop, float* part_dgamma, float* part_dbeta, float* part_dsum, int64_t rows,
                              int d, float drop_y_p, uint32_t drop_y_site, float drop_b_p, uint32_t drop_b_site, uint64_t seed,
                              float* amax, uint16_t* planes, int ld2, float* hdr, const float* scale_in, segmm_stream_t stream);
/* The embedding LayerNorms' backward (encoder.py:450-471: y = LN(proj(x) + pe[s])): the same launch on a grid of
 * segmm_layernorm_bwd_pos_parts(rows, period, d) workgroups (0: no such grid; part_dgamma / part_dbeta / part_dsum then have that
 * many rows) whose waves each walk rows of ONE position s = row mod period, and leave their sum of dx in part_pos[4 * parts, d]
 * (partial row p holds position p mod period).  segmm_colsum_pos: out[s, :] = sum of the partial rows p = s (mod period), in
 * index order -- the positional-embedding gradient without a second pass over dx. */
int segmm_layernorm_bwd_pos_parts(int64_t rows, int period, int d);
int segmm_layernorm_bwd_pos(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma,
                            float* dx, float* dx_drop, float* part_dgamma, float* part_dbeta, float* part_dsum, int64_t rows,
                            int d, float drop_y_p, uint32_t drop_y_site, float drop_b_p, uint32_t drop_b_site, uint64_t seed,
                            float* amax, uint16_t* planes, int ld2, float* hdr, const float* scale_in, float* part_pos, int period,
                            segmm_stream_t stream);
/* PLANES ONLY: the three entry points above take dx == NULL when planes, hdr and scale_in are given and dx_drop == NULL (anything
 * else fails): no fp32 dx is stored; planes, header, maxima and partials are bit for bit those of the launch with dx.  The
 * consumer of such planes has no fp32 copy to fall back on, so the protocol of the attention gradients applies: after the
 * producers, segmm_site_fixup judges the site (hdr[2] != 0: unusable, hdr[0] = the exact scale), then this REPAIR launch -- same
 * arguments as the segmm_layernorm_bwd_pos launch it follows -- leaves at once when hdr[2] == 0 and otherwise recomputes the rows
 * and rewrites ONLY the planes with hdr[0].  It writes no dx, no partial buffer, no maxima and no flag (those pointers may be
 * NULL); dx_drop must be NULL.  Knob DPRE_PLANES_ONLY (segmm_config_set) tells the engine where to use it. */
int segmm_layernorm_bwd_pos_repair(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma,
                                   float* dx, float* dx_drop, float* part_dgamma, float* part_dbeta, float* part_dsum, int64_t rows,
                                   int d, float drop_y_p, uint32_t drop_y_site, float drop_b_p, uint32_t drop_b_site, uint64_t seed,
                                   float* amax, uint16_t* planes, int ld2, float* hdr, const float* scale_in, float* part_pos, int period,
                                   segmm_stream_t stream);
int segmm_colsum_pos(const float* part, int n_rows, int period, int d, float* out, segmm_stream_t stream);

/* out[n] (+)= sum_m w[m] * X[m,n]  (bias gradients, LayerNorm partial combine, head weight gradient).
 * workspace: segmm_colsum_chunks(M) * N floats. */
int segmm_colsum_chunks(int64_t M);
int segmm_colsum(const float* X, int ld, const float* w, int64_t M, int N, float* out, int accumulate,
                 float* workspace, segmm_stream_t stream);

/* K4 -- joint self+cross attention of one side (encoder.py:44-73,138-161).  Queries Qa/Qb (two projections of the
 * same Lq tokens) against key blocks a (La tokens) and b (Lb tokens); all tensors are [B*L, ld] with head h at
 * columns [h*dh, (h+1)*dh).  Masks are uint8 (torch.bool).  lse: [2, B, H, Lq] floats
 * (plane 0 = softmax row max, plane 1 = 1/row sum, written by the forward); Dvec: [B, H, Lq] floats.
 * One key block may be empty (La == 0 or Lb == 0, its pointers null): the CrossAtt / SelfAtt ablations.
 * Head dims: dh in {4, 8, 16, 32, 48, 64, 96, 128}.  The wide heads (96, 128) run the fp32-view forms only -- direct and
 * streamed forward, the D kernels, the dQ / dK-dV pair and a fused backward of their own (at most 8 waves per workgroup, a key
 * block of more tiles in passes) -- with every plane OUTPUT; input planes (*_in) are refused there.
 * Sizes: Lq <= 256, La <= 256, Lb <= 256.  Up to 192 padded keys (each key block rounded up to a multiple of 16) every form
 * below is available.  Beyond that the forward and phases 0-3 of the backward run on the streamed kernels (key tiles in a
 * run-time loop, online softmax; fp32 views, plane OUTPUT of the forward still written); the fused phases 4-6 and input
 * planes (*_in) are refused there.  Knob ATT_STREAM = 1 sends every fp32-view forward and every phase 0-3 backward to
 * the streamed kernels at any size; with them phases 1 + 2 + 3 give the bits of phase 0.
 * segmm_attn_bwd phase: 0 = whole backward on `stream` (dQ kernel, which also writes Dvec, then dK/dV kernel);
 * 1 = Dvec = rowsum(dO * O) only; 2 = dQa/dQb only (Dvec not written); 3 = dKa/dVa/dKb/dVb only (reads Dvec) -- phases 2
 * and 3 are independent once phase 1 is complete and may run concurrently on two streams; 4 = dQ, dK and dV in ONE kernel
 * (one workgroup per (b, h, key block), query side staged in LDS in chunks of 48 rows, D formed inside -- Dvec is not
 * used; <= 12 key tiles per block; wide heads: a launch that takes a block in several passes carries the dQ partial sums in
 * the fp32 dQ buffer, which it therefore writes under any flags); 5 / 6 = the same kernel for key block a / b only (the two launches of phase 4 are
 * independent: disjoint outputs, shared maxima slots are integer atomic maxima -- they may run on two streams). */
/* optional plane outputs of the attention kernels (see "PLANE OUTPUTS of producers"): the forward's O; in the fused backward
 * (phase 4) the query-side gradients dQa / dQb (one site: they are columns of the same buffer) and the key-side gradients
 * of block a (dKa, dVa) and block b (dKb, dVb).  Each plane pointer addresses the same column slice as its fp32 twin. */
typedef struct {
    uint16_t* o; int ldo2; float* hdr_o; const float* sin_o;
    uint16_t *dqa, *dqb; int lddq2;
    uint16_t *dka, *dva; int lddka2;
    uint16_t *dkb, *dvb; int lddkb2;
    float *hdr_q, *hdr_ka, *hdr_kb;
    const float *sin_q, *sin_ka, *sin_kb;
    /* fused backward only.  bit 0 (SEGMM_ATTN_PLANES_ONLY): gradients whose planes are written get no fp32 copy -- the caller
     * then passes the consumers no fp32 fallback for that site and, after EVERY producer of the site has been enqueued, calls
     * segmm_site_fixup on the site headers and then segmm_attn_bwd again with the same arguments and bit 1
     * (SEGMM_ATTN_REPAIR) set: the repair launch ends at once unless segmm_site_fixup found the planes of a site unusable
     * (overflow flag, maximum below the fp16 window, or no scale yet), in which case it rewrites them with the exact scale of
     * the recorded maxima. */
    int flags;
    /* forward and fused backward (round 5): INPUT planes -- the P32 planes of the Q / K / V column slices as their producers
     * (the fused projection GEMMs) wrote them, each addressing the same columns as its fp32 twin, with the headers of the sites
     * they belong to (queries; key block a: K and V of one buffer; key block b).  When qa_in / qb_in are given (all of the *_in
     * fields must be, for the non-empty key blocks) and the shape qualifies (dh in {16, 32, 48}, La % 4 == 0, Lb % 4 == 0, at most
     * 112 tokens per side), segmm_attn_fwd stages K / V by LDS-DMA and segmm_attn_bwd (fused phases 4-6) loads the fragments
     * straight from the planes; every product runs on the fp16 matrix cores (three partial products, the GEMM engine's
     * arithmetic).  The fp32 views (Qa ... Vb) may then be NULL -- a caller whose projection GEMMs write planes ONLY: a site
     * whose planes are unusable under its header's scale must have been rewritten by its producer's repair launch
     * (segmm_gemm_p, write_c bit 1), and the kernels take the exact scale of the recorded maxima like that launch did.  With
     * fp32 views given, the forward stages such a site from them inside the same launch.  Shapes that do not qualify run the
     * fp32-view kernels and refuse a call without views. */
    const uint16_t *qa_in, *qb_in; int ldq2_in; const float* hdr_q_in;
    const uint16_t *ka_in, *va_in; int ldka2_in; const float* hdr_ka_in;
    const uint16_t *kb_in, *vb_in; int ldkb2_in; const float* hdr_kb_in;
} segmm_attn_planes_t;
#define SEGMM_ATTN_PLANES_ONLY 1
#define SEGMM_ATTN_REPAIR 2
/* Between the producers of planes-only sites and their repair launches: for each non-NULL site header whose planes are
 * unusable under hdr[0], put the exact scale of the recorded maxima in hdr[0], clear the overflow flag, set hdr[2] (the repair
 * launches act on it) and count the site in stats[0] (the counter segmm_scales_update keeps for refused planes; may be NULL). */
int segmm_site_fixup(float* hdr0, float* hdr1, float* hdr2, float* hdr3, float* stats, segmm_stream_t stream);
int segmm_attn_fwd(int B, int H, int dh, int Lq, int La, int Lb, const float* Qa, const float* Qb, int ldq,
                   const float* Ka, const float* Va, int ldka, const float* Kb, const float* Vb, int ldkb,
                   const uint8_t* mq, const uint8_t* mka, const uint8_t* mkb, float* O, int ldo, float* lse,
                   float drop_p, uint64_t seed, uint32_t site, float* amax_o, const segmm_attn_planes_t* planes,
                   segmm_stream_t stream);
int segmm_attn_bwd(int B, int H, int dh, int Lq, int La, int Lb, const float* Qa, const float* Qb, int ldq,
                   const float* Ka, const float* Va, int ldka, const float* Kb, const float* Vb, int ldkb,
                   const uint8_t* mq, const uint8_t* mka, const uint8_t* mkb, const float* lse, const float* O, int ldo,
                   const float* dO, int lddo, float* Dvec, float* dQa, float* dQb, int lddq, float* dKa, float* dVa, int lddka,
                   float* dKb, float* dVb, int lddkb, float drop_p, uint64_t seed, uint32_t site,
                   float* amax_q, float* amax_ka, float* amax_kb, int phase, const segmm_attn_planes_t* planes,
                   segmm_stream_t stream);

/* K7 -- interest head Linear(d,1) (decoder_leave_focal.py:451,596): out[m] (+)= x[m,:].w (+ bias[0]) and
 * dx[m,:] (+)= g[m]*w.  segmm_vecsum: deterministic out[0] (+)= sum v. */
int segmm_rowdot(const float* x, int ld, const float* w, const float* bias, float* out, int64_t rows, int d,
                 int accumulate, segmm_stream_t stream);
int segmm_rowscale_bcast(const float* g, const float* w, float* dx, int ld, int64_t rows, int d, int accumulate,
                         segmm_stream_t stream);
int segmm_vecsum(const float* v, int64_t n, float* out, int accumulate, segmm_stream_t stream);
/* bilinear fusion head InteractionAggregation (decoder_leave_focal.py:392-423): out[m] (+)= sum_n a[m,n]*b[m,n] and
 * out[m,:] (+)= g[m]*X[m,:]; the per-head x_h W_h products run on segmm_gemm. */
int segmm_rowdot_pair(const float* a, int lda, const float* b, int ldb, float* out, int64_t rows, int d,
                      int accumulate, segmm_stream_t stream);
int segmm_rowscale_mat(const float* g, const float* X, int ldx, float* out, int ldo, int64_t rows, int d,
                       int accumulate, segmm_stream_t stream);

/* K2' -- id-mode embeddings (encoder.py:426-435,445,484-486), pre-LayerNorm:
 *   vid[b,s,:] = cat(item_table[item_id[b]], frame_w*pos[b,s] + frame_b) + vid_pe[s];   usr[b,0,:] = user_table[uid[b]] + usr_pe[0]
 *   (frame_pos = null: pos[b,s] = s; the 'noPos' ablation passes per-row shuffled positions [B*S], encoder.py:428-429;
 *   pe = null: no positional embedding is added -- the trainers' --use_pe 0, encoder.py:450-471 else branches)
 * backward: dense table gradients accumulated deterministically over batch rows grouped by id
 * (order = batch rows sorted by id, from a host-side torch.sort; no data-dependent sizes, no sync),
 * and dpe[s,:] = sum_b dpre[b,s,:].  n_rows = rows of the table: an id outside [0, n_rows) (torch.nn.Embedding raises
 * on it) never touches memory -- its forward row is filled with NaN so the loss shows it, its backward is skipped. */
int segmm_embed_id_vid(const int64_t* item_id, const float* table, int dhalf, const float* frame_w,
                       const float* frame_b, const float* pe, const float* frame_pos, float* out, int B, int S,
                       int64_t n_rows, segmm_stream_t stream);
int segmm_embed_id_usr(const int64_t* user_id, const float* table, int d, const float* pe, float* out, int B,
                       int64_t n_rows, segmm_stream_t stream);
int segmm_embed_id_bwd(const float* dpre, int tokens_per_row, int ld, int col0, int width, const int32_t* order,
                       const int64_t* ids, float* dtable, int B, int64_t n_rows, segmm_stream_t stream);
/* order[k] = index of the k-th smallest id, equal ids in index order (torch.argsort(ids, stable=True), which
 * segmm_embed_id_bwd needs as `order`); n <= 8192, one workgroup, no host sync. */
int segmm_argsort_ids(const int64_t* ids, int n, int32_t* order, segmm_stream_t stream);
/* The same for any n <= 2^24: beyond 8192 ids the bitonic network runs over `keys_ws` (caller-owned, next power of two >= n
 * 64-bit words), chunks of 8192 keys per workgroup in LDS, larger strides as global compare-exchange launches (round 6: the
 * gathered id list of a data-parallel node outgrows one workgroup from 8 ranks x 2048 rows on). */
int segmm_argsort_ids_ws(const int64_t* ids, int n, int32_t* order, uint64_t* keys_ws, segmm_stream_t stream);
/* table[ids[k], :] = 0 for k < n (ids outside [0, n_rows) are skipped): the rows a previous segmm_embed_id_bwd scattered into a
 * dense [n_rows, width] table gradient, cleared without re-filling the table. */
int segmm_zero_rows(float* table, int width, const int64_t* ids, int n, int64_t n_rows, segmm_stream_t stream);
/* Data parallel: the all-gathered label statistics of G ranks -- G records [v (B) | v2 (B) | norms (3)] in rank order -- split into
 * v_all / v2_all [G * B] (what segmm_loss_fwd_bwd takes as the global view lengths, decoder_leave_focal.py:163-221 on the GLOBAL
 * batch) and the three normalisers summed over the ranks in rank order.  One launch; no torch kernel inside the DP step. */
int segmm_label_stats_unpack(const float* gathered, int G, int B, float* v_all, float* v2_all, float* norms, segmm_stream_t stream);
int segmm_pe_grad(const float* dpre, int ld, int B, int S, int d, float* dpe, int accumulate, segmm_stream_t stream);

/* The loss scalars of compute_loss (decoder_leave_focal.py:490-572) from the per-row terms segmm_loss_fwd_bwd wrote:
 * losses[c] = sum_b parts[b][c] for the 12 loss slots and total[0] = sum_c coef[c] * losses[c] (the weighted sum of
 * :560-571), one launch, fixed summation order.  dlogits != NULL (the n_dl values of d loss / d logits): also gmax[0] = their
 * largest magnitude, and site_scale[i] for every i < n_sites with gain[i] > 0 becomes the power of two that puts gain[i] * gmax at
 * 2^target -- the delayed scales of the BACKWARD tensors, which are linear in d loss / d logits (see segmm_scales_update). */
int segmm_loss_finish(const float* parts, int B, const float* coef, float* losses, float* total, const float* dlogits, int64_t n_dl,
                      float* site_scale, const float* gain, int n_sites, float* gmax, int target, segmm_stream_t stream);

/* K8 -- compute_loss forward + backward in one launch (decoder_leave_focal.py:490-572).
 * part order: 0 interestBPR 1 focal 2 surviveCE 3 interestCE 4 interestKL 5 huber 6 hazard 7 mse 8 mse2.
 * coef/enabled are host arrays of 9; parts: [B, 12] (row stride 12, columns 9..11 zero) per-row contributions already divided by the GLOBAL
 * normalisers, so a column sum (segmm_colsum) over rows -- and over data-parallel ranks -- gives each loss.
 * segmm_label_stats fills v[B] = #(gt==1), v2[B] = #(gt>=0) (after the optional focal rewrite) and the device
 * array norms[3] = {#rows with v < S, B, #(gt != -2)}; a data-parallel trainer all-gathers v/v2 and sums norms
 * over ranks before the loss call, so every rank normalises by the GLOBAL counts without a host sync.
 * Segment count: 1 <= S <= 256 (anything else is refused).  One kernel, one wave per row: a lane owns R = ceil(S / 64) segments,
 * segment j in lane j & 63 (csrc/loss.h: loss_fwd_bwd_kernel<R>; R = 1, a row of up to 64 segments, gives the bits of every
 * earlier release). */
int segmm_label_stats(const int64_t* gt, int B, int S, int rewritten, float* v, float* v2, float* norms,
                      segmm_stream_t stream);
int segmm_loss_fwd_bwd(int B, int S, const float* logits, const int64_t* gt, const float* bias_w,
                       const float* bias_b, const float* exposure, const float* coef, const int* enabled,
                       int rewritten_ce, int rewritten_kl, int use_mask, const float* norms, const float* v_all,
                       const float* v2_all, int Bg, float* logits_out, float* dlogits, float* parts,
                       segmm_stream_t stream);

/* K9 -- fused AdamW over one flat fp32 range (torch.optim.AdamW semantics; main_for_seq_leave_earlystop_SegMM.py:226,299).
 * lr >= 0 travels by value.  lr < 0 (pass SEGMM_LIVE_LR) is a sentinel: the kernel takes the rate from the bound device step
 * state (segmm_step_schedule below), the value segmm_step_advance evaluated for this step; it needs step == -1 and is refused
 * otherwise.  The same holds for segmm_adamw_table (both phases), segmm_adamw_scaled and segmm_adamw_table_scaled. */
#define SEGMM_LIVE_LR (-1)
int segmm_adamw(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                float eps, float weight_decay, int step, segmm_stream_t stream);
/* AdamW over an id-embedding table [n_rows, width] (encoder.py:352-362: nn.Embedding inputs) whose gradient is zero outside the
 * rows listed in ids -- the batch's rows (duplicates allowed; ids outside [0, n_rows) are ignored) -- in TWO passes that together
 * are the dense torch.optim.AdamW step (moments and weights of rows without a gradient still decay), element for element with the
 * arithmetic of segmm_adamw:
 *   phase 0: marks the listed rows in `flags`, then updates every UNMARKED row with g = 0.  It reads no gradient, so it can be
 *            enqueued at the START of the step on a stream of its own (the forward and backward only read the listed rows of
 *            the table): 28 B x 90 M parameters of HBM traffic leave the end of the step (config 3's 352 494 x 256 item table);
 *   phase 1: the listed rows, each once (a mark is claimed and cleared by whoever updates the row), with their gradient rows
 *            from g (the dense [n_rows, width] gradient).  Enqueue it after phase 0 AND the backward have completed.
 * flags: n_rows 32-bit words owned by the caller, zero before the first call; zero again after phase 1.  step and lr (the
 * SEGMM_LIVE_LR sentinel included: phase 0 at the head of a step reads the rate of that same step) as in segmm_adamw. */
int segmm_adamw_table(float* p, const float* g, float* m, float* v, int64_t n_rows, int width, const int64_t* ids, int n_ids,
                      uint32_t* flags, float lr, float beta1, float beta2, float eps, float weight_decay, int step, int phase,
                      segmm_stream_t stream);
/* Global-norm gradient clipping without a host sync: torch.nn.utils.clip_grad_norm_(params, max_norm) followed by AdamW
 * (main_for_seq_leave_earlystop_SegMM.py:298), everything on the device.
 * segmm_grad_norm: total_norm = the 2-norm of g[0, n) (any float offset, any n >= 0), summed in fp64 per workgroup into `scratch`
 *   (1024 doubles, caller-owned) and then in a fixed order: the same gradient gives the same bits every run.  Writes
 *   out2[0] = total_norm and out2[1] = coef = min(1, max_norm / (total_norm + 1e-6)), both fp32, coef evaluated as torch does
 *   (reciprocal, then product; a NaN norm gives a NaN coef).  max_norm > 0; max_norm = inf reports the norm and gives coef = 1.
 * segmm_adamw_scaled / segmm_adamw_table_scaled: segmm_adamw / phase 1 of segmm_adamw_table with the gradient multiplied by *coef
 *   (device memory, e.g. out2 + 1) and rounded to fp32 first -- bit for bit segmm_adamw on fp32(g * coef).  The table's phase 0
 *   (g = 0) takes no scale.  lr < 0 (SEGMM_LIVE_LR) with step == -1: the device state's rate, as in segmm_adamw. */
int segmm_grad_norm(const float* g, int64_t n, float max_norm, double* scratch, float* out2, segmm_stream_t stream);
int segmm_adamw_scaled(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                       float eps, float weight_decay, int step, const float* coef, segmm_stream_t stream);
int segmm_adamw_table_scaled(float* p, const float* g, float* m, float* v, int64_t n_rows, int width, const int64_t* ids, int n_ids,
                             uint32_t* flags, float lr, float beta1, float beta2, float eps, float weight_decay, int step, const float* coef,
                             segmm_stream_t stream);
/* Parameter groups: per-group learning-rate scale, weight decay and freezing inside the one-launch step.  The flat buffers are cut
 * into n_seg SEGMENTS, device arrays of n_seg entries each: segment s covers the floats [seg_end[s - 1], seg_end[s]) counted from
 * the buffers' BASE (seg_end[-1] = 0; ends ascending; every end but the last a multiple of 4; floats at or beyond the last end go
 * with the last segment), steps at the rate fp32(lr * seg_lr_scale[s]) with the decay seg_weight_decay[s], and with
 * seg_frozen[s] != 0 is left alone.
 * segmm_adamw_groups: ONE launch over the floats [start, start + n) of p, g, m, v (base pointers, 16-byte aligned; start a
 *   multiple of 4; the range may begin and end inside a segment; the n % 4 tail belongs to the last segment the range touches).
 *   For every element the result is bit for bit that of segmm_adamw (coef == NULL) or segmm_adamw_scaled (coef: the device float
 *   the gradient is multiplied by first) launched on that element's segment alone with lr = fp32(lr * seg_lr_scale[s]) and
 *   weight_decay = seg_weight_decay[s]; with one segment of scale 1 that is segmm_adamw itself.  Elements of frozen segments are
 *   neither read nor written: no p, no g, no m, no v.  seg_frozen == NULL says that no segment is frozen (the kernel then need not
 *   wait for the table before it loads its elements: the faster form when nothing is frozen).  lr = SEGMM_LIVE_LR with step == -1:
 *   lr is the device step state's rate (the scale applies to it), the bias corrections the state's, as in segmm_adamw.
 * segmm_grad_norm_groups: segmm_grad_norm over g[0, n) (g the 16-byte aligned base the ends count from) WITHOUT the elements of
 *   frozen segments, which are not read: a NaN or inf there does not reach out2.  fp64 partials, fixed order, the coefficient
 *   arithmetic of segmm_grad_norm.
 * segmm_adamw_table_lrs: segmm_adamw_table (phase 0 and 1, coef == NULL) and segmm_adamw_table_scaled (phase 1, coef != NULL) at
 *   the rate fp32(lr * lr_scale) -- lr the argument or, with SEGMM_LIVE_LR, the device state's; lr_scale finite and >= 0.  The
 *   same row kernels; lr_scale = 1 gives the bits of the two older entry points. */
int segmm_adamw_groups(float* p, const float* g, float* m, float* v, int64_t start, int64_t n, const int64_t* seg_end,
                       const float* seg_lr_scale, const float* seg_weight_decay, const uint8_t* seg_frozen, int n_seg, float lr,
                       float beta1, float beta2, float eps, int step, const float* coef, segmm_stream_t stream);
int segmm_grad_norm_groups(const float* g, int64_t n, const int64_t* seg_end, const uint8_t* seg_frozen, int n_seg, float max_norm,
                           double* scratch, float* out2, segmm_stream_t stream);
int segmm_adamw_table_lrs(float* p, const float* g, float* m, float* v, int64_t n_rows, int width, const int64_t* ids, int n_ids,
                          uint32_t* flags, float lr, float lr_scale, float beta1, float beta2, float eps, float weight_decay, int step,
                          int phase, const float* coef, segmm_stream_t stream);
/* Lazy exact AdamW of an id-embedding table: only the batch's rows are touched per step.  The step of a row WITHOUT a gradient is
 * a function of the row's own (p, m, v) and that step's scalars, so it is taken later, in order, with the same fp32 operations:
 * after a flush the table holds the bits of the dense update (segmm_adamw_table phase 0 + 1 every step).  Three pieces of state,
 * all caller-owned device memory:
 *   stamps  n_rows int32: the number of optimizer steps already applied to each row;
 *   hist    a ring of cap entries of four floats {rate, bc1, bc2_sqrt, 0} (16-byte aligned), the entry of step t in slot t % cap:
 *           what moves from step to step.  The rate is the one the step used BEFORE any lr_scale;
 *   the other hyperparameters (betas, eps, decay, lr_scale) are arguments of the replay: the caller flushes before it changes one.
 * segmm_adamw_hist_push: one thread writes the entry of `step` (>= 1: bias corrections computed as in segmm_adamw; -1: count,
 *   corrections and -- with lr = SEGMM_LIVE_LR -- the rate of the bound device step state), so it can sit in a recorded step.
 * segmm_adamw_table_catchup: every listed row (ids, n_ids; duplicates allowed, ids outside [0, n_rows) ignored, as in
 *   segmm_adamw_table) whose stamp is below the target replays the steps stamp + 1 .. target with g = 0 from the ring and is
 *   written once; its stamp becomes the target (an atomic max claims the row: a duplicate, or a row already at the target, is
 *   neither read nor written).  target - stamp <= cap must hold for every row reached.  ids == NULL: the FLUSH, every row of the
 *   table.  flags != NULL (listed rows only): every valid listed row is marked for a following phase 1 of segmm_adamw_table,
 *   which a lazy step runs without a phase 0.  target: by value (relative == 0, target >= 0), or the bound device step count plus
 *   target (relative != 0, target 0 or -1: -1 at the head of a step, behind segmm_step_advance, is "every step before this one").
 * segmm_adamw_table_stamp: the listed rows' stamps become at least the target (after phase 1 has stepped them); ids == NULL:
 *   all n_rows stamps are SET to the target (a loaded checkpoint, a rebuilt buffer).
 * One lazy step T: catchup(ids, target T - 1, flags) ahead of the forward; hist_push(T); phase 1 of segmm_adamw_table on the same
 * ids; stamp(ids, T).  With cap = F the caller flushes (catchup with ids == NULL to the step count) whenever F steps have passed
 * since the last flush, before the next step begins.
 * Data parallel, a rank knows only its OWN ids at the head of a step; the rows the other ranks touch are known after the row
 * exchange.  One lazy step T there: catchup(own ids, target T - 1) ahead of the forward (no flags); hist_push(T);
 * segmm_adamw_table_lazy_rows(all ranks' ids, T).  lazy_rows claims every listed row with an atomic max of its stamp with T
 * (T: step >= 1 by value, or step == -1: the bound device step state's count, with its bias corrections and -- lr = SEGMM_LIVE_LR --
 * its rate); a row whose stamp was already T or more (a duplicate entry, a row stepped before) is neither read nor written, ids
 * outside [0, n_rows) are ignored.  The winner replays old + 1 .. T - 1 with g = 0 from the ring, then takes step T with its row
 * of g (times *coef when coef != NULL) and step T's own scalars, and writes p, m, v once: bit for bit catchup(ids, T - 1, flags),
 * hist_push(T), phase 1 of segmm_adamw_table_lrs, stamp(ids, T) on the same list.  T - 1 - stamp <= cap is the caller's rule. */
int segmm_adamw_hist_push(float* hist, int cap, float lr, float beta1, float beta2, int step, segmm_stream_t stream);
int segmm_adamw_table_catchup(float* p, float* m, float* v, int64_t n_rows, int width, const int64_t* ids, int n_ids, int32_t* stamps,
                              uint32_t* flags, const float* hist, int cap, int target, int relative, float lr_scale, float beta1,
                              float beta2, float eps, float weight_decay, segmm_stream_t stream);
int segmm_adamw_table_stamp(const int64_t* ids, int n_ids, int64_t n_rows, int32_t* stamps, int target, int relative,
                            segmm_stream_t stream);
int segmm_adamw_table_lazy_rows(float* p, const float* g, float* m, float* v, int64_t n_rows, int width, const int64_t* ids, int n_ids,
                                int32_t* stamps, const float* hist, int cap, float lr, float lr_scale, float beta1, float beta2, float eps,
                                float weight_decay, int step, const float* coef, segmm_stream_t stream);
/* The same with the weight average (segmm_ema_update) of the table kept exact; added under ABI version 30, nothing that existed
 * changed.  A row's shadow obeys shadow_t = shadow_{t-1} + (p_t - shadow_{t-1}) w_t: it depends on the row's own p_t and on step
 * t's weight only, so it is replayed WITH the row, in order, with segmm_ema_update's three rounded fp32 operations.  After a flush
 * the shadow holds the bits of segmm_ema_update run over the densely stepped table after every step.  `shadow`: the table's
 * n_rows x width floats of the EMA shadow, 16-byte aligned and disjoint from p.
 * segmm_adamw_hist_push_ema: segmm_adamw_hist_push, and the entry's fourth float is w_t -- ema_weight, or with ema_warmup != 0
 *   max(ema_weight, (float)(9.0 / (10.0 + (double)t))), t = step by value or the bound device step state's count: exactly the w of
 *   segmm_ema_update(weight, warmup, step).  (segmm_adamw_hist_push goes on writing 0 there, the replays above go on ignoring it.)
 *   The ring holds the weight each step USED: the decay may change between two steps without a flush.
 * segmm_adamw_table_catchup_ema: segmm_adamw_table_catchup without flags (this mode runs no phase 1).  A claimed row replays, for
 *   s = stamp + 1 .. target: the g = 0 AdamW step with the ring's entry of s, then shadow <- shadow + (p - shadow) w_s.  p, m, v and
 *   shadow are each read once and written once.  ids == NULL: the flush.  Claim, duplicates, ids out of range and target as above.
 * segmm_adamw_table_lazy_rows_ema: segmm_adamw_table_lazy_rows plus the shadow: the replay of old + 1 .. T - 1 as above, step T
 *   with the row of g (coef, lr_scale as above), then shadow <- shadow + (p_T - shadow) w_T.  w_T is READ FROM THE RING's entry of
 *   T: segmm_adamw_hist_push_ema for step T must have been enqueued on the same stream ahead of this call.  A row already at T is
 *   neither read nor written.
 * One lazy step T in this mode: catchup_ema(own ids, target T - 1) ahead of the forward; hist_push_ema(T); lazy_rows_ema(the
 * step's ids, T); segmm_ema_update over everything but the table. */
int segmm_adamw_hist_push_ema(float* hist, int cap, float lr, float beta1, float beta2, int step, float ema_weight, int ema_warmup,
                              segmm_stream_t stream);
int segmm_adamw_table_catchup_ema(float* p, float* m, float* v, float* shadow, int64_t n_rows, int width, const int64_t* ids, int n_ids,
                                  int32_t* stamps, const float* hist, int cap, int target, int relative, float lr_scale, float beta1,
                                  float beta2, float eps, float weight_decay, segmm_stream_t stream);
int segmm_adamw_table_lazy_rows_ema(float* p, const float* g, float* m, float* v, float* shadow, int64_t n_rows, int width,
                                    const int64_t* ids, int n_ids, int32_t* stamps, const float* hist, int cap, float lr, float lr_scale,
                                    float beta1, float beta2, float eps, float weight_decay, int step, const float* coef,
                                    segmm_stream_t stream);
/* Device-side step state, so that a whole training step (main_for_seq_leave_earlystop_SegMM.py:265-300) can be replayed from its
 * recorded launch sequences with unchanged kernel arguments: two dropout seed words and the optimizer's step count with its bias
 * corrections live in device memory -- a struct of segmm_step_state_bytes() bytes in CALLER-OWNED, 16-byte aligned device memory
 * that segmm_step_bind names for the calls that follow (host-side: each launch carries the pointer in its arguments, the library
 * keeps no __device__ state; several trainers in one process bind their own state before they step).  With nothing bound (or
 * segmm_step_bind(NULL)) the calls use one default state the library allocates on first use.  segmm_step_set initialises the
 * bound state, segmm_step_advance (one thread; the first launch of a
 * step) increments the count, derives new seed words and the corrections 1 - beta^t, segmm_step_get reads them back (it
 * synchronises the stream).  A dropout seed argument with bit 63 set is "live": the kernel XORs the device words into it;
 * segmm_adamw with step == -1 takes the corrections from the device state. */
int segmm_step_state_bytes(void);
int segmm_step_bind(void* state);
int segmm_step_set(uint64_t seed, int step, float beta1, float beta2, segmm_stream_t stream);
int segmm_step_advance(float beta1, float beta2, segmm_stream_t stream);
int segmm_step_get(uint64_t* seed, int* step, float* bias_corrections, segmm_stream_t stream);
/* The learning rate of the step, in the same state: a recorded step carries every AdamW argument by value, so a rate that moves
 * from step to step lives on the device next to the bias corrections.  The state holds a schedule descriptor and `lr`, the rate
 * of its current step; segmm_step_advance re-evaluates lr as it increments the count (no further launch), segmm_step_set for the
 * count it is given, and the AdamW entry points read it when their lr argument is SEGMM_LIVE_LR.  With k = the number of
 * COMPLETED optimizer steps (torch's opt.step(); sched.step() loop: step t runs at k = t - 1), W = warmup_steps, D = decay_steps,
 * j = max(k - W, 0), r = eta_min / base_lr:
 *     lr = base_lr * warm(k) * dec(j),   warm(k) = start_factor + (1 - start_factor) k / W for k < W, else 1 (W = 0: no warm-up)
 *     SEGMM_LR_CONSTANT dec = 1                                    SEGMM_LR_STEP dec = gamma^floor(j / step_size)
 *     SEGMM_LR_COSINE   dec = r + (1 - r)(1 + cos(pi min(j, D) / D)) / 2      SEGMM_LR_EXP  dec = gamma^j
 *     SEGMM_LR_LINEAR   dec = 1 - (1 - r) min(j, D) / D            (cosine and linear hold eta_min after D steps)
 * evaluated in double from the descriptor's floats and rounded once to fp32: torch.optim.lr_scheduler's LinearLR warm-up followed
 * (SequentialLR) by ConstantLR / CosineAnnealingLR / LinearLR / StepLR / ExponentialLR.  A zeroed state has no schedule
 * (SEGMM_LR_NONE) and lr = 0.
 * segmm_step_schedule installs a descriptor in the bound state and sets lr for the state's current count (at count 0: the rate
 *   of step 1).  base_lr > 0; warmup_steps >= 0 and, with a warm-up, 0 < start_factor <= 1; decay_steps >= 1 for cosine and
 *   linear; 0 <= eta_min <= base_lr; 0 < gamma <= 1; step_size >= 1 (fields a kind does not use must still be in range: pass
 *   start_factor = gamma = 1, step_size = 1, eta_min = 0).  SEGMM_LR_NONE is what a zeroed state holds, not a kind to install.
 * segmm_step_set_base_lr changes base_lr alone and re-evaluates lr: with SEGMM_LR_CONSTANT the hook of any host-driven scheduler
 *   (reduce-on-plateau), legal between any two steps, eager or replayed.
 * segmm_step_get_lr reads {lr, base_lr} back (either pointer may be null); like segmm_step_get it takes HOST pointers and
 *   synchronises the stream. */
enum { SEGMM_LR_NONE = 0, SEGMM_LR_CONSTANT = 1, SEGMM_LR_COSINE = 2, SEGMM_LR_LINEAR = 3, SEGMM_LR_STEP = 4, SEGMM_LR_EXP = 5 };
int segmm_step_schedule(int kind, float base_lr, int warmup_steps, float start_factor, int decay_steps, float eta_min, float gamma,
                        int step_size, segmm_stream_t stream);
int segmm_step_set_base_lr(float base_lr, segmm_stream_t stream);
int segmm_step_get_lr(float* lr, float* base_lr, segmm_stream_t stream);
/* THE NON-FINITE GUARD (added under ABI version 30: additive exports keep the version; nothing that existed changed, and no older entry point reads or writes the two
 * words below).  Two words of the step state that were spare -- its size is unchanged -- hold `skip`, the verdict of the current
 * step (1: the global 2-norm of its gradient is NaN or +-inf), and `skipped`, the number of steps skipped so far: the int32 words
 * SEGMM_STEP_SKIP_WORD and SEGMM_STEP_SKIP_WORD + 1 of the state.  The state's step count goes on counting ATTEMPTED steps, and with
 * it the scheduled rate, the EMA warm-up and the dropout seed words (torch: sched.step() runs every iteration); the bias
 * corrections of step t are those of the APPLIED index t - skipped (torch: GradScaler.step leaves state["step"] alone when it skips).
 * A guarded step: segmm_step_advance_guarded at its head; segmm_grad_norm / segmm_grad_norm_groups and then segmm_step_guard on the
 * stream that holds the complete gradient; every update of the step through a *_guarded entry point behind them on that stream.
 * segmm_step_advance_guarded: segmm_step_advance with the corrections of t - skipped; clears skip.  skipped == 0: the same bits.
 * segmm_step_guard: one thread; skip = !finite(out2[0]), skipped += skip.  out2: the {norm, coef} the norm wrote.  The norm is
 *   finite iff every element that enters it is: its fp64 partials of fp32 squares cannot overflow.
 * segmm_step_set_skipped: skipped = the argument, skip = 0 (a loaded checkpoint).  segmm_step_get_skipped reads {skip, skipped}
 *   back (either pointer may be null); like segmm_step_get it takes HOST pointers and synchronises the stream.
 * segmm_adamw_guarded (coef may be null: segmm_adamw; else segmm_adamw_scaled), segmm_adamw_groups_guarded,
 *   segmm_adamw_table_lrs_guarded (both phases; a skipped phase 0 marks no row) and segmm_ema_update_guarded: the arguments, checks
 *   and arithmetic of the entry point they are named after, bit for bit, behind ONE wave-uniform read of skip in the bound state: a
 *   workgroup of a skipped step returns before it loads anything, so p, m, v, the shadow and the flags keep every bit.  They read
 *   the LIVE state: step must be -1, anything else is refused. */
#define SEGMM_STEP_SKIP_WORD 14
int segmm_step_advance_guarded(float beta1, float beta2, segmm_stream_t stream);
int segmm_step_guard(const float* out2, segmm_stream_t stream);
int segmm_step_set_skipped(uint32_t skipped, segmm_stream_t stream);
int segmm_step_get_skipped(uint32_t* skip, uint32_t* skipped, segmm_stream_t stream);
int segmm_adamw_guarded(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                        float weight_decay, int step, const float* coef, segmm_stream_t stream);
int segmm_adamw_groups_guarded(float* p, const float* g, float* m, float* v, int64_t start, int64_t n, const int64_t* seg_end,
                               const float* seg_lr_scale, const float* seg_weight_decay, const uint8_t* seg_frozen, int n_seg, float lr,
                               float beta1, float beta2, float eps, int step, const float* coef, segmm_stream_t stream);
int segmm_adamw_table_lrs_guarded(float* p, const float* g, float* m, float* v, int64_t n_rows, int width, const int64_t* ids, int n_ids,
                                  uint32_t* flags, float lr, float lr_scale, float beta1, float beta2, float eps, float weight_decay,
                                  int step, int phase, const float* coef, segmm_stream_t stream);
int segmm_ema_update_guarded(float* shadow, const float* p, int64_t n, float weight, int warmup, int step, segmm_stream_t stream);


/* ---- the callers either side of the training step -------------------------------------------
 * (f)-2 on-device evaluation (my_evaluation.py:73-231, SegRec/main.py:101-117).  Integer results only: for the same
 * float inputs they are bit-exact against numpy/sklearn.
 * segmm_rank_leave: TOP_K_leave (masked = 0: row valid iff view_len < seq_valid) / TOP_K_leave_mask (masked = 1: row
 *   valid iff view_len != #unpadded, padded positions score 1.1).  x [B, ldx] interests, gt [B, S] in {1,0,-1,-2},
 *   perm [B, S] int32 candidate permutations or null.  ranks[B]: 1-based rank of the leave segment in ascending
 *   order with ties by the lower candidate index (np.argsort), 0 for invalid rows; hist[S + 1] (caller-zeroed) is
 *   incremented at [rank].
 * segmm_auc_counts: per segment s (elements seg_off[s] .. seg_off[s+1]) out[s] = {U2, npos, nneg}, U2 = sum over
 *   positives of 2 * #(negatives below) + #(negatives equal); AUC = U2 / (2 npos nneg) = sklearn.roc_auc_score.
 *   label: 1 positive, 0 negative, other values ignored.  One segment = ProbAUC of a batch; one per user = wuAUC.
 * segmm_survival: surv = exp(cumsum(log interest)) (sequential fp32 sum) and the AUC label of each cell. */
int segmm_rank_leave(const float* x, int ldx, const int64_t* gt, const int32_t* perm, int B, int S, int masked, int seq_valid,
                     int32_t* ranks, int32_t* hist, segmm_stream_t stream);
int segmm_auc_counts(const float* score, const int8_t* label, const int64_t* seg_off, int n_seg, int64_t* out,
                     segmm_stream_t stream);
int segmm_survival(const float* interest, int ld, const int64_t* gt, float* surv, int8_t* label, int B, int S,
                   segmm_stream_t stream);
/* The tail of a validation batch in ONE launch (Trainer.valid_model(recorded=True); additive to ABI 30): what the eager pass does
 * with sigmoid, * exposure, one host permutation per valid row and segmm_rank_leave.
 * segmm_valid_rows: logits [B, ld] (ld >= S), exposure [S], gt [B, S] in {1,0,-1,-2}.  interest[b, s] = sigmoid(logits[b, s]) *
 *   exposure[s] in fp32 (the loss kernels' sigmoid); validity, the 1.1 fill (masked), the target and ranks[B] are segmm_rank_leave's
 *   on those interests (0 <= seq_valid <= S).  permute != 0 (S <= 256): the candidates of row b are shuffled by a permutation of
 *   0 .. S-1 drawn in the kernel from the library's counter hash, keyed by (seed, site, row0 + b) -- segmm_rand_perm_rows' draw for
 *   row row0 + b: the reference's distribution, not numpy's bit stream; a row draws the same permutation in whichever batch it sits.
 *   interests [B, S] and perm_out [B, S] (the permutation used: candidate j is position perm_out[b, j]; the identity without
 *   permute) are optional outputs.  Any S >= 1 without permute; B == 0 launches nothing; row0 >= 0. */
int segmm_valid_rows(const float* logits, int ld, const float* exposure, const int64_t* gt, int B, int S, int masked, int seq_valid,
                     int permute, uint64_t seed, uint32_t site, int64_t row0, int32_t* ranks, float* interests, int32_t* perm_out,
                     segmm_stream_t stream);
/* Per-row metrics of the test phase (main_eval_batch, my_evaluation.py:249-266; TOP_K_leave(test=1); --eval_cold,
 * --count_view_completion).  Floating-point results, unlike the three above; one thread per row with segmm_survival's
 * sequential fp32 recurrence, so surv is bit-identical to it.
 * segmm_row_metrics: interest [B, ld] (ld >= S), gt [B, S] in {1,0,-1,-2}; photo_id [B] and seen [n_seen] bytes or both
 *   null.  One record per row, stored field-major:
 *     irec [4, B] int32: view_length = #(gt == 1) | duration = #(gt != -2) | top1 = argmin interest, lowest index on ties |
 *                        group = 1 (cold: photo_id outside [0, n_seen) or seen[photo_id] == 0), else 0 (hot; no table: 0)
 *     frec [4, B] float: jaccard = (sum_{t < view_length} (1 - |gt[t] - surv[t]|) + duration - view_length) / duration
 *                        (NaN for duration == 0) | pred_view_length = sum_{gt[t] != -2} surv[t] |
 *                        leave_ctr = 1 - interest[k] | leave_ctr_view = 1 - surv[k], k = view_length - 1, S - 1 for view_length 0
 *   Any S >= 1; B == 0 launches nothing.
 * segmm_row_metrics_accumulate: acc [3, 10] double (caller-owned and -zeroed; groups: all, cold, hot rows) += over the B
 *   records of {1, jaccard, pred, (pred - vl)^2, |pred - vl|, leave_ctr, leave_ctr_view, (top1 - vl)^2, |top1 - vl|,
 *   vl == duration}.  One workgroup, fixed summation order, no floating-point atomics: bit-identical from run to run;
 *   stream order serialises the batches.  S = the segment count the records were made with (checked only). */
int segmm_row_metrics(const float* interest, int ld, const int64_t* gt, const int64_t* photo_id, const uint8_t* seen, int64_t n_seen,
                      int B, int S, int32_t* irec, float* frec, segmm_stream_t stream);
int segmm_row_metrics_accumulate(const int32_t* irec, const float* frec, int B, int S, double* acc, segmm_stream_t stream);
/* (f)-1 resident-table feature gather (dataloader_SegMM.py:271-362 + the trainer's L1 normalisation): out[r, :] =
 * table[idx[r], :] (/ (sum|.| + 1e-6) if normalize), mask[r] = 1, for idx[r] in [0, n_lines); zeros / 0 otherwise. */
int segmm_gather_l1(const float* table, int64_t n_lines, int D, const int64_t* idx, int64_t rows, int normalize, float* out,
                    uint8_t* mask, float* amax, uint16_t* planes, int ld2, float* hdr, const float* scale_in, segmm_stream_t stream);
/* the same from a table of 16-bit elements (SEGMM_ELEM_F16 / SEGMM_ELEM_BF16, see segmm_l1norm_h): out, mask, maxima and planes are
 * those of segmm_gather_l1 on the widened table, bit for bit.  table: 8-byte aligned, D % 4 == 0. */
int segmm_gather_l1_h(const uint16_t* table, int elem, int64_t n_lines, int D, const int64_t* idx, int64_t rows, int normalize,
                      float* out, uint8_t* mask, float* amax, uint16_t* planes, int ld2, float* hdr, const float* scale_in,
                      segmm_stream_t stream);
/* the same from a table of 8-bit elements (SEGMM_ELEM_E4M3 / _E5M2 / _I8, see segmm_l1norm_b), with either `normalize`.  table: 4-byte
 * aligned, D % 4 == 0. */
int segmm_gather_l1_b(const uint8_t* table, int elem, int64_t n_lines, int D, const int64_t* idx, int64_t rows, int normalize,
                      float* out, uint8_t* mask, float* amax, uint16_t* planes, int ld2, float* hdr, const float* scale_in,
                      segmm_stream_t stream);
/* (f)-1, the step before the gather: index batches assembled on the device from a COMPILED interaction table
 * (FrameDatasetSeq_SegMM._getitem, dataloader_SegMM.py:295-357, as an integer function of data resolved once on the host;
 * segmminterest_amd/feature_store.py: InteractionTable.compile builds the table, DeviceBatches drives this entry point).
 * The descriptor is a HOST struct of DEVICE pointers, read when the call is made:
 *   items   item_ptr [n_items + 1], item_line [item_ptr[n_items]]: line of frame f of item i at item_line[item_ptr[i] + f], -1 = the
 *           key "item-f" is not in the line map (a hole);
 *   users   own_ptr [n_users + 1], own_line [...]: the user's own frames as lines, unresolvable ones already dropped (no -1);
 *   rows    row_info [n_rows, 4] = {item of the video, number of video frames n, user, 0}; row_cols [n_rows, 7] = photo_id,
 *           photo_identity_id, user_id, user_identity_id, time_ms, play_time, duration; hist_ptr [n_rows + 1] and hist_pair [..., 2] =
 *           the history as (item, watched frames nf) pairs; label [n_rows, label_S] padded with -2 or cut to label_S;
 *   max_cand  the largest candidate count (video frames or user candidates) of any row; selects the kernel instance.
 * Per batch slot b with r = row_ids[b]:
 *   video   candidates = the lines of frames 0 .. n-1 of the row's item (n is cut to the item's length).  n <= S: photo_idx[b, :n] =
 *           them in order, the rest -1.  n > S: S of them, drawn as below.
 *   user    candidates = for each history pair in order the lines of frames 0 .. min(nf, item length) - 1 of its item, holes
 *           skipped, then the user's own lines; m of them.  m <= Lt: user_idx[b, :m] = them in order, the rest -1 (m = 0: all
 *           -1).  m > Lt: Lt of them, drawn as below.
 *   label[b, :] = the row's label, cols[k, b] = row_cols[r, k] (cols is [7, B]: every column a contiguous tensor).
 *   r outside [0, n_rows), or a row with more candidates than SEGMM_ASSEMBLE_MAX_CAND (InteractionTable.compile refuses such
 *   a table): an all-padding slot -- indices -1, label -2, columns 0 (segmm_gather_l1's convention for bad indices).
 * The draw (count candidates, cap = S or Lt, count > cap): candidate j -- its position in the hole-free candidate list -- gets the
 *   32-bit key  SECOND word of the dropout counter hash at counter q = (r << 13) | (stream << 12) | j,  stream = 0 for the video
 *   and 1 for the user list:  k = seed_lo ^ (site * 0x9E3779B9) ^ ((q >> 32) * 0x85EBCA6B), a = mix32((q & 0xFFFFFFFF) ^ k),
 *   key = mix32(a ^ seed_hi ^ 0x68E31DA4);  seed_lo = bits 0..31 and seed_hi = bits 32..62 of `seed`, all arithmetic mod 2^32,
 *   mix32(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16.
 *   Chosen are the cap smallest (key, j) pairs; a chosen candidate is written at its rank among them.  That is a uniformly random
 *   cap-subset in uniformly random order (np.random.choice(n, S, replace=False) / random.sample: the reference's distributions,
 *   not its bit streams), a function of (seed, site, r) only -- not of the batch, the slot or the rank that assembles the row.
 *   Lists that fit (count <= cap) never touch the hash.  The device step state is never read: a seed with bit 63 set is refused.
 * Limits: 1 <= S <= 256, S == label_S, 1 <= Lt <= SEGMM_ASSEMBLE_MAX_CAND, max_cand <= SEGMM_ASSEMBLE_MAX_CAND = 4096 (the
 *   row's keys and lines sit in LDS: 8 bytes per candidate and wave), n_rows <= 2^50 (q has 64 bits), lines < 2^31.
 * One wave per row; instances of 1024 candidates (4 rows per workgroup, 32 KB LDS) and 4096 (2 rows, 64 KB), by max_cand. */
#define SEGMM_ASSEMBLE_MAX_CAND 4096
typedef struct {
    const int64_t *item_ptr; const int32_t *item_line;
    const int64_t *own_ptr; const int32_t *own_line;
    const int64_t *hist_ptr; const int32_t *hist_pair;
    const int32_t *row_info; const int64_t *row_cols; const int8_t *label;
    int64_t n_rows; int n_items; int n_users; int label_S; int max_cand;
} segmm_itable_t;
int segmm_assemble_rows(const segmm_itable_t* table, const int64_t* row_ids, int B, int S, int Lt, uint64_t seed, uint32_t site,
                        int64_t* photo_idx, int64_t* user_idx, int64_t* label, int64_t* cols, segmm_stream_t stream);
/* Delayed scaling, end of a pass: arena = the pass's n_rows site headers, site_idx[r] = index of row r's tensor site in
 * site_scale (< 0: none).  site_scale[idx] = the power of two s with max|x| * s in [2^(target-1), 2^target) for every row
 * that was produced; stats[0] += number of rows whose planes were outside the fp16 window.  gain / gmax non-NULL (backward pass):
 * also gain[idx] = max|x| / gmax[0] (segmm_loss_finish turns it into the next step's scale). */
int segmm_scales_update(const float* arena, const int32_t* site_idx, int n_rows, float* site_scale, float* stats, int target,
                        float* gain, const float* gmax, segmm_stream_t stream);
/* DIAGNOSTIC, not part of the reference path: launches `workgroups` x 512 threads that issue `iters` x 48 v_mfma_f32_16x16x32_f16
 * per wave on random operand bits (registers only, the plane GEMM's accumulator order and occupancy); *flops_out = the fp16 MFMA
 * FLOPs of the launch.  bench.py times it to report the SUSTAINED matrix-core rate of the part beside the datasheet peak
 * (power management clocks a random-data MFMA stream down; constant operands do not show it). */
int segmm_probe_mfma_rate(int workgroups, int iters, float* scratch, double* flops_out, segmm_stream_t stream);

/* Arithmetic of the attention kernels (models/encoder.py:44-73,138-161): 0 = exact-fp32 matrix-core products everywhere,
 * 1 = fp16x3 products (22-bit operands, the GEMM engine's arithmetic) where that form is built and measured faster (default;
 * env SEGMM_ATTN=f32|f16|f16all sets the initial value), 2 = fp16x3 wherever it is built.  Returns the previous mode; mode < 0
 * only queries.  Results of the two forms agree to ~1e-6 relative; both are deterministic. */
int segmm_attn_mode(int mode);

/* Tuning / A-B knobs of the library (tile shapes, kernel forms, probes that change occupancy -- none changes results beyond the
 * documented equivalences).  They are read from the environment ONCE, at the first use of the library (SEGMM_<NAME>), and live
 * in one table: segmm_config_dump writes "SEGMM_<NAME>=<value>  # what it selects" lines into buf (at most n bytes incl. the
 * terminator) and returns the length the full listing needs; segmm_config_set changes a knob by its name (without the SEGMM_
 * prefix) and returns its previous value, or a negative error code for an unknown name.  No launch path reads the environment.
 * Timing probes whose results are wrong exist in -DSEGMM_ATT_PROBE / -DSEGMM_GEMM_PROBE builds only. */
int segmm_config_set(const char* name, int value);
int segmm_config_dump(char* buf, int n);

/* (f)-3 SegRec weighted head (ClipRec.forward, SegRec/models/context/ClipRec.py:163-181): out[r] = sum_seg pred[r, seg] *
 * weight[r, seg] * (seg < duration[r]); weight == null: ones, duration == null: no duration mask. */
int segmm_segment_weighted_sum(const float* pred, const float* weight, const int64_t* duration, int64_t rows, int S, float* out,
                               segmm_stream_t stream);

/* (f)-3 on the device: the logit store the inference pass fills (inference/save_logits_for_all_leave_SegMM.py:105-146) answers the
 * recommender's 'c_interest_weight' lookups (SegRec/models/BaseModel.py:241-286) and feeds ClipRec's sum without a [B, I, S] tensor.
 * Index of a store (device tensors): keys int64 [n, 3] = (user, item, time_ms), sorted lexicographically (signed) and unique; rows
 *   int32 [n], rows[k] = the row of the value matrix vals (float32 [m, S], m >= n) of key k.  A key added more than once is listed
 *   once, with the row of its LAST occurrence (the reference's dict assignment).
 * segmm_store_lookup: queries user [B], item [B, I] (column 0 = the target), time [B], int64; the target index (keys, rows, n >= 0);
 *   a negatives index (neg_keys, neg_rows, n_neg >= 0), n_neg < 0 = none given; dense id maps user_map [n_um] / item_map [n_im]
 *   (int64, null = identity) applied to the ids first (the non-KuaiRand branch, :264-286).  rowidx int32 [B, I], miss int64 [2], which
 *   the caller initialises to INT64_MAX.  Per row b, t = the row of (user, item[b, 0], time) in the target index:
 *     t absent                                -> rowidx[b, :] = -1 ("ones");
 *     t present, no negatives index or I <= 2 -> rowidx[b, :] = t (the reference's len(item_ids) > 2: at I == 2 a negatives file
 *                                                is ignored);
 *     t present, negatives index and I > 2    -> rowidx[b, 0] = t, rowidx[b, j] = -2 - r with r = the row of (user, item[b, j], time)
 *                                                in the negatives index; that key absent: rowidx[b, j] = -1, miss[0] = min(miss[0], b * I + j).
 *   An id outside its map or a map entry < 0 counts as an absent key -- a bad user or target: t absent, miss[1] = min(miss[1], b * I);
 *   a bad item j >= 1 (every item is mapped when item_map is given, as the reference does): rowidx[b, j] = -1, miss[1] =
 *   min(miss[1], b * I + j).  Both slots are minima: deterministic, the first offender in row-major order.
 *   One workgroup per row b; the target key is searched once per workgroup; a search compares three 64-bit words.  B == 0 launches nothing.
 * segmm_store_head: out[r] = sum_s pred[r, s] * w(r)[s] * (s < duration[r]) over the rows r = (b, i) of pred [rows, S], with
 *   w(r) = ones for rowidx[r] == -1, vals[rowidx[r]] for rowidx[r] >= 0, neg_vals[-2 - rowidx[r]] for rowidx[r] <= -2 (vals [m, S],
 *   neg_vals [m_neg, S]).  duration int64 [rows] or null (no mask).  weight_out non-null: also weight_out[r, :] = w(r) (float32
 *   [rows, S]); pred == null and out == null: only that.  A rowidx outside its value matrix (or into a null one) touches no memory:
 *   its weight is NaN, so the result shows it (segmm_embed_id_vid's convention for bad ids).  Any S >= 1; rows == 0 launches nothing.
 *   Each product is rounded once and multiplied by the mask's 0 or 1; the summation order is a function of S and the pointers'
 *   alignment only: bit-identical from run to run.  m, m_neg < 2^31 - 1.
 * segmm_store_head_bwd: dpred[r, s] = (g[r] * w(r)[s]) * (s < duration[r]) -- one rounded product, then a multiplication by 0 or 1.
 *   w(r) from rowidx + the value matrices as above, or from an explicit weight [rows, S] (rowidx null), or ones (both null). */
int segmm_store_lookup(const int64_t* user, const int64_t* item, const int64_t* time, int B, int I, const int64_t* keys,
                       const int32_t* rows, int64_t n, const int64_t* neg_keys, const int32_t* neg_rows, int64_t n_neg,
                       const int64_t* user_map, int64_t n_um, const int64_t* item_map, int64_t n_im, int32_t* rowidx, int64_t* miss,
                       segmm_stream_t stream);
int segmm_store_head(const float* pred, const int32_t* rowidx, const float* vals, int64_t m, const float* neg_vals, int64_t m_neg,
                     const int64_t* duration, int64_t rows, int S, float* out, float* weight_out, segmm_stream_t stream);
int segmm_store_head_bwd(const float* g, const int32_t* rowidx, const float* vals, int64_t m, const float* neg_vals, int64_t m_neg,
                         const float* weight, const int64_t* duration, int64_t rows, int S, float* dpred, segmm_stream_t stream);

/* The store's writer and its index build on the device; added under ABI version 30: nothing that existed changed.
 * segmm_store_append: one batch of the inference pass into preallocated tables -- keys[row0 + r] = (user[r], photo[r], time_ms[r]) and
 *   vals[row0 + r, 0 .. S) = logits[r * ld .. r * ld + S) for r < B, bit copies (keys int64 [capacity, 3], vals float32 [capacity, S]).
 *   Any S >= 1, ld >= S and alignment of the rows (4-byte floats, 8-byte ids): 16-byte accesses where S % 4 == 0, ld % 4 == 0 and both
 *   value bases are 16-byte aligned, one dword per lane otherwise.  Nothing outside rows [row0, row0 + B) is written.  B == 0 launches
 *   nothing.  Refused by name: row0 < 0, row0 + B > capacity, a null pointer, S < 1, ld < S.  One launch, a recordable command: the recorded
 *   dump (Trainer.dump_logits(recorded=True)) rewrites row0 / capacity / keys / vals per replay.
 * segmm_store_index: the index of a store (the format stated above segmm_store_lookup) from its unsorted key rows keys [n, 3]:
 *   out_keys [n, 3] / out_rows [n] hold, in their first *n_unique entries, the distinct keys in lexicographic SIGNED order and the row
 *   of each key's LAST occurrence; *n_unique (device int64) = their number; the entries behind them are not written.  The order (user,
 *   item, time, row) is total, so the result is the one of any correct comparison sort (bridge.LogitStore._build_index on the host).
 *   The rows are sorted as 4-word tuples by a bitonic network in `ws` (segmm_store_index_ws(&bytes, n) gives its size -- a helper without a stream, not a command; 16-byte
 *   aligned): chunks of 2048 tuples in LDS, every larger stride one global compare-exchange launch; padding slots compare above
 *   every real tuple by a flag, never by a key value (any int64 triple is a legal key).  Then the last-of-run flags are counted per
 *   block, the counts scanned by one workgroup, and the flagged tuples scattered to their ranks: separate launches, no workgroup
 *   waits for another.  Deterministic.  n == 0 launches no kernel and clears *n_unique.  0 <= n <= 2^24 (SEGMM_STORE_INDEX_MAX);
 *   beyond, the call is refused by name (the host-side index build, DeviceLogitStore.finalize() without on_device, has no limit). */
#define SEGMM_STORE_INDEX_MAX 16777216
int segmm_store_append(const int64_t* user, const int64_t* photo, const int64_t* time_ms, const float* logits, int ld, int B, int S,
                       int64_t row0, int64_t capacity, int64_t* keys, float* vals, segmm_stream_t stream);
int segmm_store_index_ws(int64_t* ws_bytes, int64_t n);
int segmm_store_index(const int64_t* keys, int64_t n, void* ws, int64_t ws_bytes, int64_t* out_keys, int32_t* out_rows,
                      int64_t* n_unique, segmm_stream_t stream);

/* up to three column sums out_i[n] = sum_m X_i[m, n] of same-shaped matrices in one launch pair (X1/X2 may be null);
 * workspace: 3 * segmm_colsum_chunks(M) * N floats.  Used for the partial buffers of segmm_layernorm_bwd. */
int segmm_colsum3(const float* X0, const float* X1, const float* X2, int ld, int64_t M, int N, float* out0, float* out1,
                  float* out2, float* workspace, segmm_stream_t stream);

/* CrossMLP ablation (encoder.py:392-396,503-506): nn.AdaptiveAvgPool1d(bins) over the token axis of cat(U[B,Lu,d], V[B,Lv,d]):
 * out[b,i,:] = mean of tokens [floor(i T/bins), ceil((i+1) T/bins)), T = Lu+Lv; and its backward (dU, dV overwritten). */
int segmm_pool_tokens(const float* U, int Lu, const float* V, int Lv, float* out, int B, int d, int bins, segmm_stream_t stream);
int segmm_pool_tokens_bwd(const float* dOut, float* dU, int Lu, float* dV, int Lv, int B, int d, int bins, segmm_stream_t stream);

/* Spatial-reduction attention (sr_ratio r > 1, encoder.py:23-31,84-102; added under ABI version 30: nothing that existed changed).
 * The reducing Conv1d(d, d, r, stride = r, padding = p = (r - 1) / 2) has non-overlapping windows: packed side by side they make the
 * conv one NT GEMM with the weight [d, d, r] read, as stored, as a row-major [d, r d] matrix (K index c r + t).
 * Ls = S / r must equal the conv length (S + 2 p - r) / r + 1 and be >= 1; 2 <= r <= 8; d % 4 == 0: anything else is refused by name.
 * segmm_sr_pack:   A[b Ls + j, c r + t] = x[(b S + j r - p + t) ldx + c] if 0 <= j r - p + t < S else 0   (A: [B Ls, r d], dense);
 *   amax: optional zeroed [SEGMM_AMAX_SLOTS] array receiving the partial maxima of |A|; m_sr (optional, needs m [B, S]):
 *   m_sr[b, j] = OR over t < r of m[b, j r + t] -- the pooled key mask, NOT shifted by p (the reference's max_pool1d).
 * segmm_sr_unpack: G[b, i, c] = res[b, i, c] + dA[b Ls + (i + p) / r, c r + (i + p) % r] if (i + p) / r < Ls, else res[b, i, c]; res may
 *   be NULL (then the dA element itself, or 0).  G, res: [B S, d] dense; one fp32 add per element: deterministic.  G is neither operand. */
int segmm_sr_pack(const float* x, int ldx, const uint8_t* m, float* A, uint8_t* m_sr, float* amax, int B, int S, int d, int r,
                  segmm_stream_t stream);
int segmm_sr_unpack(const float* dA, const float* res, float* G, int B, int S, int d, int r, segmm_stream_t stream);

/* ---- Recorded launch sequences: the training step (main_for_seq_leave_earlystop_SegMM.py:265-300) enqueued from C -----------
 * SURVEY.md 8(b) asks for coarse entry points (embedding, encoder layer, head + loss, optimizer tail) so that a host language
 * does not pay a foreign-function call per kernel.  A PHASE is the resolved launch list of one such part of the step: an array
 * of commands, each naming one stream-taking entry point of this header (op = index into segmm_cmd_op_name) with its arguments
 * in declaration order as 8-byte slots (pointers and integers in .i / .p, float parameters as double in .f) and the stream slot
 * it is enqueued on (0 = main stream, 1 = side stream, 2 = auxiliary stream).  Two pseudo-ops order a stream s >= 1 against the
 * main stream: SEGMM_OP_FORK (stream s waits for everything enqueued on the main stream so far) and SEGMM_OP_JOIN (the main
 * stream waits for stream s); s travels in the command's `stream` field.
 * The host builds a phase ONCE per workload shape -- segmminterest_amd/hipabi.py records the per-op calls of one eager step --
 * and replays it every step: kernel arguments do not change from step to step when the per-step state lives on the device
 * (segmm_step_advance: dropout seed words, optimizer step count) and buffers are persistent; the few that do (the batch's
 * tensors) are patched in place by the host before the call.  Ownership: the command array, structs and host arrays its
 * pointer arguments name (segmm_attn_planes_t, the loss coefficient arrays) belong to the caller and must outlive the call.
 * segmm_run_phase returns the first non-zero return code of a command (0 = everything enqueued); it never synchronises.
 * The named entry points are segmm_run_phase restricted to one kind of phase (they refuse a descriptor of another kind):
 * they are what a maintainer binds per part of the reference's step -- _get_embedding (encoder.py:425-473), one
 * SegFormerXEncoderLayer (encoder.py:189-208) forward / backward, head + compute_loss (decoder_leave_focal.py:490-658),
 * optimizer.step (main...SegMM.py:299). */
#define SEGMM_CMD_MAX_ARGS 48
typedef union { int64_t i; double f; void* p; } segmm_arg_t;
typedef struct { int32_t op; int32_t stream; segmm_arg_t a[SEGMM_CMD_MAX_ARGS]; } segmm_cmd_t;
#define SEGMM_OP_FORK (-1)
#define SEGMM_OP_JOIN (-2)
enum { SEGMM_PHASE_STEP_BEGIN = 0, SEGMM_PHASE_EMBED_FWD = 1, SEGMM_PHASE_LAYER_FWD = 2, SEGMM_PHASE_HEAD_LOSS_FWD = 3,
       SEGMM_PHASE_HEAD_LOSS_BWD = 4, SEGMM_PHASE_LAYER_BWD = 5, SEGMM_PHASE_EMBED_BWD = 6, SEGMM_PHASE_STEP_TAIL = 7, SEGMM_PHASE_KINDS = 8 };
typedef struct {
    int32_t kind;          /* SEGMM_PHASE_* */
    int32_t backbone;      /* 0 / 1: which backbone of a two-tower ('both') model; 0 otherwise */
    int32_t layer;         /* encoder layer of a LAYER_* phase, else 0 */
    int32_t n_cmds;
    const segmm_cmd_t* cmds;
} segmm_phase_t;
/* number of dispatchable entry points / the name of op `op` (NULL outside [0, n)): hosts map names to op ids at load time */
int segmm_cmd_op_count(void);
const char* segmm_cmd_op_name(int op);
/* streams[0 .. n_streams): hipStream_t of the slots (streams[0] = main; n_streams <= SEGMM_MAX_STREAMS); events[2 (s - 1)] and
 * events[2 (s - 1) + 1]: two hipEvent_t of the caller (disable-timing events) per stream s >= 1, used by its fork / join pseudo-ops */
#define SEGMM_MAX_STREAMS 3
int segmm_run_phase(const segmm_phase_t* phase, const segmm_stream_t* streams, int n_streams, void* const* events);
int segmm_step_begin(const segmm_phase_t* phase, const segmm_stream_t* streams, int n_streams, void* const* events);
int segmm_embed_fwd(const segmm_phase_t* phase, const segmm_stream_t* streams, int n_streams, void* const* events);
int segmm_layer_fwd(const segmm_phase_t* phase, const segmm_stream_t* streams, int n_streams, void* const* events);
int segmm_head_loss_fwd(const segmm_phase_t* phase, const segmm_stream_t* streams, int n_streams, void* const* events);
int segmm_head_loss_bwd(const segmm_phase_t* phase, const segmm_stream_t* streams, int n_streams, void* const* events);
int segmm_layer_bwd(const segmm_phase_t* phase, const segmm_stream_t* streams, int n_streams, void* const* events);
int segmm_embed_bwd(const segmm_phase_t* phase, const segmm_stream_t* streams, int n_streams, void* const* events);
int segmm_step_tail(const segmm_phase_t* phase, const segmm_stream_t* streams, int n_streams, void* const* events);
/* bytes of p[0 .. bytes) = 0 on `stream` (the clears of the step path as a recordable command) */
/* Small launches that keep the reference's remaining step variants free of host-side tensor ops, so that they can be recorded
 * and replayed like the default step (round 5):
 * segmm_bias_grad: learnable_bias (decoder_leave_focal.py:497-504,649-658) -- g_bias_bias[s] = sum_b dl[b, s] (rows in index
 *   order), g_bias_weight[s] = (s + 1) g_bias_bias[s];
 * segmm_focal_relabel: focal loss first in the loss list rewrites the labels in place (:534-535): gt > 0 -> 1, gt == -1 -> 0;
 * segmm_rand_uniform / segmm_rand_ids: the noUser ablations' random user features in [0, 1) and random user ids in [lo, hi)
 *   (main_for_seq_leave_earlystop_SegMM.py:275-280), segmm_rand_perm_rows: the noPos ablation's fresh permutation of 0 .. S-1 per
 *   row (encoder.py:428-429; 1 <= S <= 256, written as floats; one kernel, a lane ranks the keys of R = ceil(S / 64) indices; rows
 *   of S <= 64 keep the bit stream of earlier releases, longer rows draw from a stream of their own) -- drawn from the counter
 *   hash of the dropout streams (seed with bit 63 set: the device-side step words are XORed in): the reference's distributions,
 *   not torch's bit streams. */
int segmm_bias_grad(const float* dl, int B, int S, float* g_bias_weight, float* g_bias_bias, segmm_stream_t stream);
int segmm_focal_relabel(int64_t* gt, int64_t n, segmm_stream_t stream);
int segmm_rand_uniform(float* out, int64_t n, uint64_t seed, uint32_t site, segmm_stream_t stream);
int segmm_rand_ids(int64_t* out, int64_t n, int64_t lo, int64_t hi, uint64_t seed, uint32_t site, segmm_stream_t stream);
int segmm_rand_perm_rows(float* out, int rows, int S, uint64_t seed, uint32_t site, segmm_stream_t stream);
int segmm_fill_zero(void* p, int64_t bytes, segmm_stream_t stream);
/* dst[0 .. bytes) = src[0 .. bytes), device to device, on `stream` (non-overlapping ranges) */
int segmm_copy_bytes(void* dst, const void* src, int64_t bytes, segmm_stream_t stream);

/* test hook: multiplier (0 or 1/(1-p)) of elements [0,n) of a dropout site */
int segmm_dropout_mult(float* out, int64_t n, float p, uint64_t seed, uint32_t site, segmm_stream_t stream);

/* The weight average of Trainer(ema=...), placed in front of segmm_vec_add; added under ABI version 30: nothing that existed changed.
 * segmm_ema_update: shadow[i] = shadow[i] + (p[i] - shadow[i]) * w for i < n, three IEEE fp32 operations, nothing contracted, in place.
 *   w = weight (0 < weight <= 1), or with warmup != 0: w = max(weight, (float)(9.0 / (10.0 + (double)t))) -- decay_t = min(decay,
 *   (1 + t) / (10 + t)), written as its complement -- t = step (>= 1, by value) or, with step == -1, the step count of the bound
 *   device step state (the count segmm_step_advance left: that of the step just taken).  shadow and p 16-byte aligned and
 *   disjoint, any n >= 0 (n % 4 tail included); anything else is refused by name.  (Knob EMA_NT: the shadow's traffic nontemporal; same bits.)
 * segmm_vec_swap: a[i] <-> b[i] for i < n; 16-byte aligned, disjoint (an overlap is refused by name), any n >= 0. */
int segmm_ema_update(float* shadow, const float* p, int64_t n, float weight, int warmup, int step, segmm_stream_t stream);
int segmm_vec_swap(float* a, float* b, int64_t n, segmm_stream_t stream);

/* out[i] = a[i] + b[i] (one IEEE fp32 add, nothing contracted), i < n; n >= 0; out may be exactly a or exactly b; any other overlap
 * of out with an operand is refused (nothing is written).  The gradient sum of a micro-batched step (Trainer(micro_batch=m)): 16-byte
 * accesses where the three pointers share their offset from a 16-byte boundary (scalar head and tail), one dword per lane otherwise;
 * pointers need 4-byte alignment only.  Added under ABI version 30: nothing that existed changed. */
int segmm_vec_add(float* out, const float* a, const float* b, int64_t n, segmm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
