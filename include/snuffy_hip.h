/*
 * snuffy_hip.h -- C ABI of libsnuffy_hip.so: hand-written HIP (gfx950 / CDNA4) kernels for the hot path of
 * jafarinia/snuffy: the sparse-attention MIL aggregator (snuffy.py) and, in later rounds, the ViT extractor.
 *
 * The reference has NO native layer: its boundary is the Python nn.Module API.  This header is
 * the FFI a maintainer would bind *underneath* that API (INTEGRATION.md shows the ctypes stub).  Each entry point
 * names the reference code it replaces (file:line, relative to the reference repo).
 *
 * Conventions (all entry points):
 *   - plain pointers + sizes; every buffer (inputs, outputs, workspace) is DEVICE memory owned by the caller;
 *   - row-major, contiguous unless a leading dimension is passed; index tensors are int64 (torch.long);
 *   - asynchronous on `stream` (a hipStream_t passed as void*); never synchronises, never allocates;
 *   - returns 0 on success, a negative SNF_E* code on failure; message via snf_last_error() (thread-local);
 *   - stateless, re-entrant, thread-safe; results are deterministic run-to-run (no float atomics).  The ONE exception is the block
 *     of snf_debug_* switches at the end of this header: process-wide kernel-variant selectors for the parity tests and the A / B
 *     timing tools (atomic ints read once at the entry of a call; every variant computes the same function, so a racing switch
 *     can change which kernel runs, never what a call returns beyond the documented rounding order).  Nothing in snuffy_amd/
 *     touches them; an embedding that wants the contract above without the footnote simply never calls them.
 */
#ifndef SNUFFY_HIP_H
#define SNUFFY_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* snf_stream_t; /* hipStream_t */

#define SNF_OK 0
#define SNF_EINVAL (-1)      /* bad argument (null pointer, unsupported shape) */
#define SNF_ELAUNCH (-2)     /* hipLaunch / runtime error */
#define SNF_EUNSUPPORTED (-3) /* shape outside what the fast kernel handles; caller picks the generic entry */
#define SNF_EWORKSPACE (-4)  /* workspace too small */

/* activation codes: PositionwiseFeedForward activation_dictionary, snuffy.py:215-221 */
#define SNF_ACT_RELU 0
#define SNF_ACT_GELU 1       /* erf form (nn.GELU default) */
#define SNF_ACT_LEAKYRELU 2  /* slope 0.01 (nn.LeakyReLU default) */
#define SNF_ACT_SELU 3
#define SNF_ACT_NONE 4

/* element types of q / v^T operands of the MFMA attention kernel */
#define SNF_DT_F32 0
#define SNF_DT_BF16 1
#define SNF_DT_BF16_SPLIT3 2 /* [hi | hi | lo] bf16 image of an fp32 value (snf_gemm_bf16 output, snf_layernorm_rows_split3_f32) */
#define SNF_DT_BF16_HL 3     /* interleaved bf16 image: every 32 columns as [hi(32) | lo(32)], 2 n columns (snf_gemm_hl_bf16) */

const char* snf_version(void);
const char* snf_last_error(void);
/* Number of compute units of the current device (grid sizing on the host side); <0 on error. */
int snf_device_cu_count(void);

/* ---------------------------------------------------------------------------------------------------------
 * K1  critic scores  c = x w^T + b            replaces FCLayer.forward, snuffy.py:39-41 (nn.Linear(D, C))
 *     plus column max over the bag             replaces torch.max(ins_prediction, 1), train.py:831-834
 *   x [n, d] f32, w [c_out, d], b [c_out] (nullable) -> scores [n, c_out]
 *   colmax_val [c_out] f32 / colmax_idx [c_out] i64 nullable (first index on ties, as torch.max on CPU).
 * --------------------------------------------------------------------------------------------------------- */
int snf_critic_f32(const float* x, int64_t n, int d, const float* w, const float* b, int c_out, float* scores,
                   float* colmax_val, int64_t* colmax_idx, snf_stream_t stream);
/* K1 + K5 in one pass over the bag: the critic scores AND xhat [n, d] bf16 = (x - mean) * rstd, the affine-free LayerNorm
 * of SublayerConnection 'attn' (snuffy.py:97,107) whose gamma/beta the bf16 path folds into the Q|V projection weights.
 * Same arithmetic as snf_critic_f32 and snf_layernorm_rows_f32(gamma = beta = NULL, out_bf16): identical outputs. */
int snf_critic_ln_f32(const float* x, int64_t n, int d, const float* w, const float* b, int c_out, float* scores,
                      float eps, void* xhat_bf16, snf_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * K2  top-k patch selector                    replaces torch.sort(c,1,descending=True)[:k], snuffy.py:128-130
 *   scores: n values at stride `stride` (elements).  idx_out [k] int64: the k largest, in descending score
 *   order, ties by ascending index (== torch.sort(stable=True, descending=True)[:k]); -0.0 == +0.0; NaN sorts
 *   first like torch.  Requires 1 <= k <= n, k <= SNF_TOPK_MAX_K.  One-workgroup radix select on the orderable 32-bit keys (three counting
 *   passes over register-resident keys, LDS integer atomics) + rank sort of the survivors: exact, deterministic.
 *   Above 65536 scores (and with a workspace of snf_topk_workspace_bytes): histogram launch + the multi-workgroup
 *   select of the fused selector below.
 * K4  fused gather  xs[j,:] = x[idx[j],:]      replaces index_select/cat, snuffy.py:131,145-147,103-106
 *   snf_topk_gather_f32 = selector then gather in one call (x, xs nullable -> selector only).
 * --------------------------------------------------------------------------------------------------------- */
#define SNF_TOPK_MAX_K 2048
size_t snf_topk_workspace_bytes(int64_t n, int k); /* bytes the selector needs for this shape (may be 0) */
int snf_topk_f32(const float* scores, int64_t n, int64_t stride, int k, int64_t* idx_out, void* workspace,
                 size_t workspace_bytes, snf_stream_t stream);
int snf_topk_gather_f32(const float* scores, int64_t n, int64_t stride, int k, int64_t* idx_out, const float* x,
                        int d, float* xs, void* workspace, size_t workspace_bytes, snf_stream_t stream);
int snf_gather_rows_f32(const float* x, int64_t n, int d, const int64_t* idx, int k, float* out,
                        snf_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * K1 + K2 fused selector                         FCLayer.forward + torch.sort(...)[:k], snuffy.py:39-41,128-130
 *   The critic pass already touches every score it writes: snf_critic_select_f32 (one class; xhat_bf16 nullable, as
 *   snf_critic_ln_f32 when given) also counts the first radix digit (top 11 bits of the orderable key) of each score
 *   into a small replicated histogram inside `selector_state` -- integer atomics, exact and order-independent.
 *   snf_topk_select_f32 then runs ceil(n / 4096) workgroups: each reads the histogram, finds the threshold digit,
 *   classifies its slice and appends the scores above / inside the threshold bin to two short lists; the workgroup
 *   that arrives last finishes the radix selection on the lists and writes idx_out (same order and tie rule as
 *   snf_topk_f32, bit for bit).  A crowded threshold bin (> 4096 keys: massive ties) or a histogram whose total is
 *   not n falls back, inside the same launch, to the exact one-workgroup selection on the scores.
 *   selector_state: snf_selector_state_bytes() of device memory, 16-byte aligned, zeroed ONCE by the caller; every
 *   snf_topk_select_f32 leaves it zeroed for the next bag (no memset in the pipeline).  One state per stream.
 * --------------------------------------------------------------------------------------------------------- */
size_t snf_selector_state_bytes(void);
int snf_critic_select_f32(const float* x, int64_t n, int d, const float* w, const float* b, float* scores, float eps,
                          void* xhat_bf16, void* selector_state, snf_stream_t stream);
int snf_topk_select_f32(const float* scores, int64_t n, int k, int64_t* idx_out, void* selector_state,
                        snf_stream_t stream);
/* the same selection for scores that did NOT come out of snf_critic_select_f32 (any stride): clears the counted part of
 * `state` (scratch, snf_selector_state_bytes), counts the first digit in its own launch, then selects.  snf_topk_f32
 * takes this route above 65536 scores. */
int snf_topk_hist_select_f32(const float* scores, int64_t n, int64_t stride, int k, int64_t* idx_out, void* state,
                             snf_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * K9  scatter of the K updated rows            replaces y = x.clone(); y[:, S, :] = x_sel, snuffy.py:152-155
 *   snf_scatter_rows_f32 : y = x (skipped when y == x) then y[idx[j],:] = rows[j,:]
 *   snf_scatter_add_rows_f32 : z[idx[j],:] += delta[j,:]   (idx distinct)
 *   snf_slot_map_i32 : map[i] = j if idx[j] == i else -1   (row -> slot lookup used by the fused row passes)
 * --------------------------------------------------------------------------------------------------------- */
int snf_scatter_rows_f32(const float* x, int64_t n, int d, const int64_t* idx, int k, const float* rows, float* y,
                         snf_stream_t stream);
int snf_scatter_add_rows_f32(float* z, int64_t n, int d, const int64_t* idx, int k, const float* delta,
                             snf_stream_t stream);
int snf_slot_map_i32(const int64_t* idx, int k, int64_t n, int32_t* map, snf_stream_t stream);
/* K4 + slot map in one launch: xs[j] = x[idx[j]] and map[i] = j if idx[j] == i else -1 (k <= 2048, idx duplicate-free).
 * Same results as snf_gather_rows_f32 + snf_slot_map_i32.  xs_bf16 (nullable): a second copy of xs rounded to bf16
 * [k, d] -- the operand of the bf16 key projection that feeds snf_sparse_attn_fwd_mfma. */
int snf_gather_slot_map_f32(const float* x, int64_t n, int d, const int64_t* idx, int k, float* xs, int32_t* map,
                            void* xs_bf16, snf_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * K5  LayerNorm over rows, with the K9 scatter fused into the read
 *     replaces SublayerConnection.norm, snuffy.py:97,107,110 (nn.LayerNorm(size), eps 1e-5)
 *   src row i = (slot_map && slot_map[i] >= 0) ? patch_rows[slot_map[i]] : x[i]      (slot_map nullable)
 *   out = (src - mean) * rstd * gamma + beta   (gamma/beta nullable -> plain normalisation, affine folded into
 *   the following GEMM's weights by the host).  Any of out_f32 / out_bf16 / mean / rstd may be null.
 *   out_row_idx (nullable): output row of input row i is out_row_idx[i] (re-normalising the K patched rows in place).
 * --------------------------------------------------------------------------------------------------------- */
int snf_layernorm_rows_f32(const float* x, int64_t n, int d, const int32_t* slot_map, const float* patch_rows,
                           const float* gamma, const float* beta, float eps, float* out_f32, void* out_bf16,
                           float* mean, float* rstd, const int64_t* out_row_idx, snf_stream_t stream);
/* Same rows, written as the split image out_bf16 [n, 3 d] = [hi | hi | lo] (hi = bf16(v), lo = bf16(v - hi)): the A operand
 * of the fp32-class projection  v W^T ~ hi Wh^T + hi Wl^T + lo Wh^T  run as ONE bf16 GEMM over the tripled K axis against
 * W3 = [Wh | Wl | Wh] (snf_gemm_bf16; products to 2^-17 relative, fp32 accumulate). */
/* Backward of the same LayerNorm (loss.backward() of train.py:259 through snuffy.py:86,97,107,110); statistics are recomputed
 * from x, nothing is saved by the forward:
 *   dxhat = dy * gamma;  dx = residual + rstd * (dxhat - mean_d(dxhat) - xhat * mean_d(dxhat * xhat))
 *   dy [n, d] f32 or bf16 (dy_dtype) with row pitch dy_stride; dy_stride = 0 broadcasts ONE row (the mean-pooled head).
 *   gamma, residual, dx, dx_bf16, partials nullable.  partials [snf_layernorm_bwd_blocks(n), 2, d] f32: per-workgroup
 *   (sum dy * xhat, sum dy) in a fixed order -- dgamma / dbeta are their sums over the first axis. */
int snf_layernorm_bwd_blocks(int64_t n);
int snf_layernorm_rows_bwd_f32(const float* x, int64_t n, int d, const void* dy, int dy_dtype, int64_t dy_stride,
                               const float* gamma, float eps, const float* residual, float* dx, void* dx_bf16,
                               float* partials, snf_stream_t stream);
/* Host-only query, no launch: the register form the row passes above (critic, LayerNorm rows and their backward, the mean-pooled
 * head) run a row of d floats in.  *vec = 4 (16-byte vectors: d % 4 == 0 and every operand 16-byte aligned -- all_aligned != 0) or 1;
 * *nv = the 64-lane vector groups a wave holds per row.  vec / nv nullable.  SNF_EUNSUPPORTED when d is too wide for the
 * register-resident passes (d > 2048). */
int snf_row_form(int d, int all_aligned, int* vec, int* nv);
/* bf16 path: the LayerNorm affine of SublayerConnection (snuffy.py:97,107,110) folded into the projection that follows it
 * (LN(x) W^T + b = xhat (W * gamma)^T + (W beta + b)), and the gradients of the folded weights taken back to (W, b, gamma, beta):
 *   fold:    wf_bf16[r, c] = bf16(w[r, c] * gamma[c]) (row pitch ldwf);  bf[r] = sum_c w[r, c] * beta[c] + bias[r] (f32 / bf16, nullable)
 *   unfold:  dw[r, c] = dwf[r, c] * gamma[c] + dbf[r] * beta[c];  partial [snf_fold_blocks(r), 2, c] = per-workgroup
 *            (sum_r dwf * w, sum_r dbf[r] * w): dgamma / dbeta are their sums over the first axis.   c <= 2048. */
int snf_fold_blocks(int r);
int snf_fold_linear_f32(const float* w, int r, int c, const float* gamma, const float* beta, const float* bias, void* wf_bf16,
                        int64_t ldwf, float* bf_f32, void* bf_bf16, snf_stream_t stream);
int snf_unfold_linear_f32(const float* dwf, const float* w, int r, int c, const float* gamma, const float* beta, const float* dbf,
                          float* dw, float* partial, snf_stream_t stream);
/* x [m, k] f32 (row pitch ldx) -> out [m, 3 k] bf16 = [hi | hi | lo]: the activation image of an fp32-class projection whose
 * producer is not one of the kernels that can emit it directly (ViT fp32 path: patch columns, attention output). */
int snf_split3_f32(const float* x, int64_t ldx, int64_t m, int k, void* out_bf16, snf_stream_t stream);
/* w [m, k] f32 (row pitch ldw; the nn.Linear layout) -> out [m, 3 k] bf16 = [Wh | Wl | Wh], the weight operand of the same products;
 * colscale [k] (nullable): W' = W diag(colscale) formed in fp32 first (a LayerNorm gamma folded into the projection that follows it). */
/* The loss head of a training step in one launch each way (reference train.py: _run_model of the single-weight trainer -- max over the instance
 * scores, two BCEWithLogits terms (optional pos_weight) mixed by the weight w, the bag prediction):
 *   ins [n, c] f32 contiguous, logits [c], label [c], w [1], pos_weight [c] and weight [c] of BCEWithLogitsLoss (nullable; the reference passes
 *   its class weights POSITIONALLY, i.e. as `weight`: train.py:246), c <= 8
 *   out [2 + 4 c] = {loss, d loss / d w, bag_pred [c], d loss / d logits [c], d loss / d max [c], max [c]};  argmax [c] (first index on ties)
 *   _bwd: d_ins [n, c] = grad_out * (d loss / d max) at the argmax rows, 0 elsewhere; d_small [c + 1] = grad_out * {d loss / d logits, d loss / d w}.
 * A NaN instance score never wins the max (torch.max would return it): documented in DESIGN.md section 7. */
int snf_mil_loss_f32(const float* ins, int64_t n, int c, const float* logits, const float* label, const float* w, const float* pos_weight,
                     const float* weight, float* out, int64_t* argmax, snf_stream_t stream);
int snf_mil_loss_bwd_f32(const float* grad_out, const float* fwd_out, const int64_t* argmax, int64_t n, int c, float* d_ins, float* d_small,
                         snf_stream_t stream);
int snf_split3_weight_f32(const float* w, int64_t ldw, int64_t m, int k, const float* colscale, void* out_bf16, snf_stream_t stream);
/* Column sums of a [n, d] matrix fused with the elementwise step of the same pass (training: bias gradients next to the ReLU
 * mask / the bf16 cast / the critic's weight gradient; backward of snuffy.py:39-41, 224-225):
 *   v = src[i, c] (f32 or bf16) * row_weight[i * weight_stride] (nullable) ; v = 0 where gate_bf16[i, c] <= 0 (nullable: the ReLU
 *   mask from the activation output) ; dst_bf16[i, c] = bf16(v) (nullable, may alias src) ; partial[b, c] = sum over the rows
 *   of workgroup b (of the rounded values when dst is given).  partial [snf_colsum_blocks(n), d] f32, summed by the caller.
 *   d % 8 == 0, d <= 8192, 16-byte aligned buffers. */
int snf_colsum_blocks(int64_t n);
int snf_colsum_fused(const void* src, int src_dtype, int64_t n, int d, const float* row_weight, int64_t weight_stride,
                     const void* gate_bf16, void* dst_bf16, float* partial, snf_stream_t stream);
/* Encoder dropout of the bf16 training chain (snuffy.py:225, 110) outside a GEMM epilogue.  M = the Philox keep-mask of the matrix
 * (snf_dropout_mask_f32 with h = 1 and the matrix's rows / columns), regenerated in registers, never stored; dropout_p in [0, 1).
 *   snf_dropout_rows_bf16              x[i, c] = bf16(float(x[i, c]) * M[i, c]) in place, x bf16 [m, n] with row pitch ldx (n % 8 == 0,
 *                                      16-byte rows): the FFN hidden layer behind a library GEMM.  dropout_p == 0: nothing is launched.
 *   snf_residual_assemble_dropout_f32  z_out = x + M o (float(add_bf16) + add_bias) (+ delta_rows[slot_map[i]] where slot_map[i] >= 0) in one
 *                                      launch (x, z_out f32 [n, d], add_bf16 bf16 [n, d], add_bias f32 [d] nullable, slot_map int32 [n]
 *                                      nullable, d % 4 == 0).  Every step is rounded on its own, in this order: t = add_bf16 + add_bias,
 *                                      t = t * m, z = x + t, z = z + delta.  dropout_p == 0: z = ((x + add_bf16) + add_bias) + delta, the
 *                                      order of snf_ln_mean_head_f32's z_out.
 *   snf_colsum_fused_dropout           snf_colsum_fused of M o src without row weight and gate: dst_bf16 = bf16(src o M) (nullable) and the
 *                                      partial column sums (of the rounded values when dst is given) -- the backward of the line above:
 *                                      df = M o dz as the operand of the weight / input gradient GEMMs, and db2.  dropout_p == 0 = snf_colsum_fused. */
int snf_dropout_rows_bf16(void* x, int64_t ldx, int64_t m, int n, float dropout_p, uint64_t seed, uint64_t offset, snf_stream_t stream);
int snf_residual_assemble_dropout_f32(const float* x, int64_t n, int d, const void* add_bf16, const float* add_bias,
                                      const int32_t* slot_map, const float* delta_rows, float dropout_p, uint64_t seed, uint64_t offset,
                                      float* z_out, snf_stream_t stream);
int snf_colsum_fused_dropout(const void* src, int src_dtype, int64_t n, int d, float dropout_p, uint64_t seed, uint64_t offset,
                             void* dst_bf16, float* partial, snf_stream_t stream);
/* The backward of an fp32-class training step (train.py:259 through snuffy.py:187-190, 224-225) needs each gradient matrix as a split
 * image (operand of the next GEMM and of the weight-gradient contractions) AND its column sums (the bias gradient), the FFN one behind
 * the ReLU mask: one pass.   v = x[i, c] (f32, row pitch ldx) ; v = 0 where gate_bf16[i, c] <= 0 (nullable; row pitch ldg: the hi
 * plane of the activation's own split image) ; out[i, c] = out[i, plane + c] = hi(v), out[i, 2 plane + c] = lo(v) (bf16, row pitch
 * ldo: with plane = k and ldo = 3 k the image of snf_split3_f32; a wider plane lets several matrices share one image, e.g.
 * [dQ | dV]) ; partial[b, c] (nullable) = sum of v over the rows of workgroup b, [snf_colsum_blocks(m), k] f32, summed by the caller.
 * k % 8 == 0, k <= 8192, 16-byte aligned rows. */
int snf_split3_colsum_f32(const float* x, int64_t ldx, int64_t m, int k, const void* gate_bf16, int64_t ldg, void* out_bf16,
                          int64_t ldo, int64_t plane, float* partial, snf_stream_t stream);
/* The same pass writing the INTERLEAVED image ([hi(32) | lo(32)] per 32 columns, 2 k columns: the operand format of snf_gemm_hl_bf16 and of
 * snf_gemm_tn_f32's hl layout); gate_hl (nullable): the activation's own hl image, its hi values decide.  k % 32 == 0. */
int snf_split_hl_colsum_f32(const float* x, int64_t ldx, int64_t m, int k, const void* gate_hl, int64_t ldg, void* out_hl, int64_t ldo,
                            float* partial, snf_stream_t stream);
/* Skinny fp32-class projection for the K selected rows of a bag (key / output projections, snuffy.py:190, 205; the tile GEMMs
 * need thousands of rows): out [r, c] (f32 or bf16: out_dtype) = x [r, k] f32 . w [c, k]^T f32 + bias, every product as split-bf16 x3
 * on the matrix cores with the split done in registers.  r <= 8192, k % 16 == 0, rows 16-byte aligned. */
int snf_linear_rows_x3_f32(const float* x, int64_t ldx, const float* w, int64_t ldw, const float* bias, int r, int c, int k, void* out,
                           int64_t ldo, int out_dtype, snf_stream_t stream);
/* The same with a second output out2 [r, c] = out + resid [r, c]: delta = o Wo^T + bo and x_sel = xs + delta (snuffy.py:205, 108) in
 * one launch (round 6) */
int snf_linear_rows_x3_resid_f32(const float* x, int64_t ldx, const float* w, int64_t ldw, const float* bias, const float* resid, int64_t ldr,
                                 int r, int c, int k, float* out, int64_t ldo, float* out2, int64_t ldo2, snf_stream_t stream);
/* critic scores + LayerNorm (with affine) of the same rows in one pass, the normalised rows as the interleaved hi / lo image
 * (= snf_critic_f32 + snf_layernorm_rows_hl_f32 with one read of x; FCLayer.forward snuffy.py:39-41 + SublayerConnection.norm
 * snuffy.py:107).  d % 32 == 0; selector_state nullable (one class: also counts the selector's first radix digit); gamma and beta
 * both NULL = the affine-free image (x - mean) * rstd (one normalised image for both sublayers, affines folded into the projections). */
int snf_critic_ln_hl_f32(const float* x, int64_t n, int d, const float* w, const float* b, int c_out, float* scores,
                         const float* gamma, const float* beta, float eps, void* out_hl, void* selector_state,
                         snf_stream_t stream);
int snf_layernorm_rows_split3_f32(const float* x, int64_t n, int d, const int32_t* slot_map, const float* patch_rows,
                                  const float* gamma, const float* beta, float eps, void* out_bf16, snf_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * K10 epilogue  h = act(h + bias) in place     replaces activation(w_1(x)) of snuffy.py:224-225
 *   h [n, f] f32 or bf16 (dtype = SNF_DT_*), bias [f] f32 nullable.
 * --------------------------------------------------------------------------------------------------------- */
int snf_bias_act(void* h, int dtype, int64_t n, int f, const float* bias, int act, snf_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * K11 head: logits = W_head * mean_n(LayerNorm_f(z)) + b_head
 *     replaces Encoder.norm + x.mean(dim=1) + BClassifier.linear, snuffy.py:86,71
 *   row value = z[i] (+ add_bf16[i]) (+ add_bias) (+ delta_rows[slot_map[i]] when slot_map[i] >= 0): the FFN
 *   residual  z = y + W2(...) + b2  of snuffy.py:110 and the K9 scatter are fused into this read; z_out (nullable)
 *   receives the assembled rows (needed only when another layer follows).
 *   workspace: snf_ln_mean_head_workspace_bytes(d) bytes.  pooled [d] nullable output (= mean_n LN(z) before the
 *   head).  Deterministic two-stage column reduction.
 * --------------------------------------------------------------------------------------------------------- */
size_t snf_ln_mean_head_workspace_bytes(int d);
int snf_ln_mean_head_f32(const float* z, int64_t n, int d, const void* add_bf16, const float* add_bias,
                         const int32_t* slot_map, const float* delta_rows, float* z_out, const float* gamma,
                         const float* beta, float eps, const float* w_head, const float* b_head, int c_out,
                         float* logits, float* pooled, void* workspace, size_t workspace_bytes, snf_stream_t stream);
/* The same with one more addend, read FIRST: the deferred K part of snf_gemm_hl_deferred_f32.  For row i and 256-column block cb a
 * non-zero tile_map[(i / 256) * tiles_n + cb] = s + 1 adds row i % 256 of slab s (slabs [..][256][256] fp32) to z[i, 256 cb ..] before
 * the other addends: logits, pooled and z_out are bit for bit those of snf_ln_mean_head_f32 on the summed z.  d <= 256 * tiles_n. */
int snf_ln_mean_head_deferred_f32(const float* z, int64_t n, int d, const float* slabs, const int32_t* tile_map, int tiles_n,
                                  const void* add_bf16, const float* add_bias, const int32_t* slot_map, const float* delta_rows,
                                  float* z_out, const float* gamma, const float* beta, float eps, const float* w_head,
                                  const float* b_head, int c_out, float* logits, float* pooled, void* workspace,
                                  size_t workspace_bytes, snf_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * K7  sparse attention forward                 replaces attention(), snuffy.py:160-168 (+ head split/merge of
 *                                              MultiHeadedAttention.forward, snuffy.py:187-203)
 *   For every head a (column block a*dk..(a+1)*dk):
 *       P_a = softmax_j( Q_a Kp_a^T * scale )   [n, k]   softmax over the k selected keys
 *       O_a = P_a^T V_a                         [k, dk]
 *   out [k, d] = heads concatenated.  attn [h, n, k] f32 (nullable) = P;  lse [h, n] f32 (nullable) =
 *   log-sum-exp of the scaled scores (saved for backward).
 *
 *   snf_sparse_attn_fwd_f32 : exact fp32 arithmetic, any n/k/h/dk.  q, v [n, d]; kp [k, d].
 *   snf_sparse_attn_fwd_mfma: bf16 MFMA (fp32 accumulate), softmax in fp32.  q [n, ldq] and v [n, ldv] row-major
 *       (ldq, ldv >= d in elements, rows 16-byte aligned: q and v may be the two column halves of ONE fused
 *       projection output [n, 2d]), both of dtype qv_dtype (f32 converted in registers, or bf16); kp [k, d] of
 *       dtype kp_dtype: bf16 is read as it is, f32 is rounded to bf16 into the workspace first (one small launch).
 *       One launch holds 256 (dk == 64) / 224 (dk == 128) / 128 (dk == 192) keys (Kp + P + V images share the 160 KiB LDS); more
 *       keys -- up to 8 such chunks, k <= 2048 / 1792 / 1024 -- run as key chunks: a statistics launch per chunk (row max / sum) and a
 *       full launch per chunk normalising with the statistics of all chunks, so the softmax stays exact.
 *       Other dk / larger k: SNF_EUNSUPPORTED, the caller picks snf_sparse_attn_fwd_f32.
 *   workspace: deterministic cross-workgroup reduction of the [h, k, dk] accumulators.
 * --------------------------------------------------------------------------------------------------------- */
size_t snf_sparse_attn_fwd_workspace_bytes(int64_t n, int k, int h, int dk, int mfma);
int snf_sparse_attn_fwd_f32(const float* q, const float* kp, const float* v, int64_t n, int k, int h, int dk,
                            float scale, float* out, float* attn, float* lse, void* workspace,
                            size_t workspace_bytes, snf_stream_t stream);
/* The same attention with the scores in the fp32-CLASS arithmetic of snf_sparse_attn_fwd_x3 (every product as three bf16 MFMAs of the
 * operands' hi / lo halves, fp32 accumulate / softmax) for head widths the pipelined kernels do not take: dk % 16 == 0, dk <= 256 (the
 * README recipe D = 768 / h = 4 of reference README.md:661-669: dk = 192), k <= 1024; other shapes SNF_EUNSUPPORTED.  P^T V is exact
 * fp32 on the f32 matrix cores.  Two launches + the fixed-order reduction like snf_sparse_attn_fwd_f32 (same workspace:
 * snf_sparse_attn_fwd_workspace_bytes(.., 0)), operands split on the fly; P is materialised (`attn`, or in the workspace).  q / v take
 * row pitches ldq / ldv (elements, >= h dk, ldq % 4 == 0): the halves of a fused [Q | V] projection output are used in place. */
int snf_sparse_attn_fwd_x3u_f32(const float* q, int64_t ldq, const float* kp, const float* v, int64_t ldv, int64_t n, int k, int h, int dk,
                                float scale, float* out, float* attn, float* lse, void* workspace, size_t workspace_bytes,
                                snf_stream_t stream);
/* ... and its training forward: out = (P o M)^T V with M the keep-mask of snf_dropout_mask_f32 for the same (dropout_p, seed, offset),
 * regenerated in registers by the pooling pass (the LDS-staged P^T V kernel draws one Philox group per 16-byte load of P); no mask tensor.
 * `attn` is required and receives the UNDROPPED P (the convention of snf_sparse_attn_fwd_x3_dropout: snf_sparse_attn_bwd_dropout_f32
 * regenerates M from the same state); `lse` stays nullable.  dropout_p == 0 is the plain entry; dropout_p outside [0, 1) SNF_EINVAL.
 * Only the LDS-staged pooling pass has the form: k % 4 == 0, ldv % 4 == 0, 16-byte aligned attn / v and h <= 1023 on top of the plain
 * entry's limits, anything else SNF_EUNSUPPORTED before any launch (the caller applies the mask tensor to the plain entry's P).
 * Workspace: the plain entry's with `attn` given (the slice partials). */
int snf_sparse_attn_fwd_x3u_dropout_f32(const float* q, int64_t ldq, const float* kp, const float* v, int64_t ldv, int64_t n, int k, int h,
                                        int dk, float scale, float dropout_p, uint64_t seed, uint64_t offset, float* out, float* attn,
                                        float* lse, void* workspace, size_t workspace_bytes, snf_stream_t stream);
int snf_sparse_attn_fwd_mfma(const void* q, int64_t ldq, const void* v, int64_t ldv, int qv_dtype, const void* kp,
                             int kp_dtype, int64_t n, int k, int h, int dk, float scale, float* out, float* attn,
                             float* lse, void* workspace, size_t workspace_bytes, snf_stream_t stream);

/* Attention dropout (training; nn.Dropout(p = 0.1) on p_attn, snuffy.py:166-167,173).  The keep-mask is a pure function of
 * (seed, offset, head, row, key) -- Philox4x32-10, one call per 4 consecutive keys of a row (csrc/philox.h; host restatement
 * oracle/philox_ref.py) -- regenerated in registers by the forward and the backward kernel, never stored:
 *   forward : the normalised probabilities are multiplied by the mask (0 or 1 / (1 - p)) before they are pooled; `out` and the
 *             returned `attn` are those of the dropped P, as in the reference.  Needs lse (or attn) requested.
 *   backward: pass mask == NULL and the forward's (dropout_p, seed, offset).
 * More keys than one launch holds (key chunks, see snf_sparse_attn_fwd_mfma): with dropout the main passes' chunks start on multiples
 * of 4 keys (one Philox call covers 4 consecutive keys), the main pass of a chunk regenerates the mask with the key index among ALL
 * keys, and the cross-chunk statistics, lse and the undropped P are, bit for bit, those of the launch without dropout.
 * snf_dropout_mask_f32 writes the same mask as a tensor [h, n, k] (exact-fp32 training path, tests). */
int snf_sparse_attn_fwd_mfma_dropout(const void* q, int64_t ldq, const void* v, int64_t ldv, int qv_dtype, const void* kp,
                                     int kp_dtype, int64_t n, int k, int h, int dk, float scale, float* out, float* attn,
                                     float* lse, float dropout_p, uint64_t seed, uint64_t offset, void* workspace,
                                     size_t workspace_bytes, snf_stream_t stream);
int snf_sparse_attn_bwd_mfma_dropout(const void* q, int64_t ldq, const void* v, int64_t ldv, int qv_dtype, const float* kp,
                                     const float* dout, const float* lse, const float* mask, float dropout_p, uint64_t seed,
                                     uint64_t offset, int64_t n, int k, int h, int dk, float scale, float* dq, float* dv,
                                     void* ds, int ds_dtype, snf_stream_t stream);
int snf_dropout_mask_f32(float dropout_p, uint64_t seed, uint64_t offset, int h, int64_t n, int k, float* mask,
                         snf_stream_t stream);

/* K7, fp32-class on the matrix cores: q, v, kp fp32; every operand split into hi + lo bf16 halves and every product taken as
 * three bf16 MFMAs (ah bh + ah bl + al bh, fp32 accumulate); softmax / normalisation fp32.  Same outputs as
 * snf_sparse_attn_fwd_f32 to ~3e-6 on P, 1e-5 on O (the reference's own arithmetic class, north-star bound 1e-3), ~10x its speed.
 * q [n, ldq], v [n, ldv] row-major (row pitches in elements, 16-byte aligned rows: column halves of a fused projection are
 * taken in place); dk in {64, 128}; 256 / 224 keys fit one launch, more keys (up to 8 x 256 / 8 x 224) run as key chunks: a
 * statistics pass per chunk (row max / sum), then the chunks' main passes with the softmax exact over all keys -- other shapes
 * SNF_EUNSUPPORTED (the caller keeps the exact kernel).
 * workspace: snf_sparse_attn_fwd_x3_workspace_bytes (deterministic cross-workgroup reduction, as the bf16 kernel). */
size_t snf_sparse_attn_fwd_x3_workspace_bytes(int64_t n, int k, int h, int dk);
int snf_sparse_attn_fwd_x3(const float* q, int64_t ldq, const float* v, int64_t ldv, const float* kp, int64_t n, int k, int h,
                           int dk, float scale, float* out, float* attn, float* lse, void* workspace, size_t workspace_bytes,
                           snf_stream_t stream);
/* Training forward (snuffy.py:166-167: nn.Dropout on p_attn): the same launch with the Philox keep-mask of snf_dropout_mask_f32 -- the
 * same (seed, offset) give the same mask, bit for bit -- applied to P in registers: out = (P o M)^T V, while `attn` receives the
 * UNDROPPED probabilities P (what snf_sparse_attn_bwd_f32 wants next to the mask tensor).  One key chunk only (k <= 224 at dk = 128,
 * <= 256 at dk = 64; more keys: SNF_EUNSUPPORTED, the caller multiplies and contracts itself); dropout_p == 0 is snf_sparse_attn_fwd_x3. */
int snf_sparse_attn_fwd_x3_dropout(const float* q, int64_t ldq, const float* v, int64_t ldv, const float* kp, int64_t n, int k, int h,
                                   int dk, float scale, float dropout_p, uint64_t seed, uint64_t offset, float* out, float* attn,
                                   float* lse, void* workspace, size_t workspace_bytes, snf_stream_t stream);

/* K7 (fp32-class, pre-split operands)    the same attention() of snuffy.py:160-168, same arithmetic (split-bf16 x3, fp32
 * softmax / accumulate), for operands that already ARE split: q_hl, v_hl = interleaved "hl" images [n, ld] bf16 (every 32 true
 * columns c .. c + 31 of the fp32 tensor stored as [hi(32) | lo(32)], hi = bf16(x), lo = bf16(x - hi): what snf_gemm_hl_bf16
 * writes with out_dtype SNF_DT_BF16_HL and snf_split_hl_f32 makes of an fp32 tensor; 4 bytes per element like the fp32 tensor);
 * row pitches in bf16 elements (>= 2 h dk, 16-byte aligned rows: the halves of a fused [Q | V] image are taken in place);
 * kp [k, h dk] f32.  Software-pipelined kernel: LDS-DMA of full lines, one wave per key block, GEMM1 / GEMM2 MFMAs interleaved
 * with the softmax vector work in every wave's own instruction stream (csrc/sparse_attn_x3p.hip).  dk = 128, 97 <= k <= 2048: up to 256 keys
 * (4 .. 8 key blocks) in one launch, more as up to 8 key chunks -- a statistics pass per chunk, then the chunks' main passes; other shapes SNF_EUNSUPPORTED (the caller keeps snf_sparse_attn_fwd_x3).  Outputs as snf_sparse_attn_fwd_x3. */
size_t snf_sparse_attn_fwd_x3_hl_workspace_bytes(int64_t n, int k, int h, int dk);
int snf_sparse_attn_fwd_x3_hl(const void* q_hl, int64_t ldq, const void* v_hl, int64_t ldv, const float* kp, int64_t n, int k, int h,
                              int dk, float scale, float* out, float* attn, float* lse, void* workspace, size_t workspace_bytes,
                              snf_stream_t stream);
/* The same with the key projection fused in front (snuffy.py:190 + 160-168): snf_linear_rows_x3_kpfrag_f32 computes
 * Kp = x w^T + bias for the k selected rows (fp32-class, as snf_linear_rows_x3_f32) and writes it, scaled by scale * log2(e) and
 * split into bf16 hi / lo, as the MFMA fragment image the attention kernel keeps in registers -- no fp32 Kp tensor, no prep
 * launch; snf_sparse_attn_fwd_x3_hl_kpfrag then takes that image instead of kp (the scale is already in it).  Results are
 * bit-identical to the two-step form.  snf_sparse_attn_x3_hl_kpfrag_bytes: size of the image, 0 where the fused form does not
 * apply (dk != 128, k outside 97 .. 2048, or key chunks that do not start on 32-key boundaries: use the two-step form). */
size_t snf_sparse_attn_x3_hl_kpfrag_bytes(int k, int h, int dk);
int snf_linear_rows_x3_kpfrag_f32(const float* x, int64_t ldx, const float* w, int64_t ldw, const float* bias, int k_keys, int h, int dk,
                                  int kdim, float scale, void* kp_frag, size_t kp_frag_bytes, snf_stream_t stream);
/* The same with the gather of the selected rows fused in (snuffy.py:131,145-147 + 190 in ONE launch, round 6): input row i of the
 * projection is row idx[i] of the bag x [n, ldx].  xs (nullable) [k_keys, kdim] receives the gathered rows, slot_map (nullable) [n] the
 * row -> slot map of snf_gather_slot_map_f32 -- the two launches this call replaces write the same bytes. */
int snf_gather_linear_rows_x3_kpfrag_f32(const float* x, int64_t ldx, int64_t n, const int64_t* idx, const float* w, int64_t ldw,
                                         const float* bias, int k_keys, int h, int dk, int kdim, float scale, void* kp_frag,
                                         size_t kp_frag_bytes, float* xs, int32_t* slot_map, snf_stream_t stream);
int snf_sparse_attn_fwd_x3_hl_kpfrag(const void* q_hl, int64_t ldq, const void* v_hl, int64_t ldv, const void* kp_frag, int64_t n, int k,
                                     int h, int dk, float* out, float* attn, float* lse, void* workspace, size_t workspace_bytes,
                                     snf_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * K7-bwd  sparse attention backward, exact fp32    replaces autograd through attention(), snuffy.py:160-168
 *   p [h, n, k] = the probabilities the forward returned (attn);  mask [h, n, k] nullable = dropout keep-mask already
 *   divided by (1 - p_drop) (the forward used p o mask);  dout [k, d] = gradient of the attention output.
 *       dV = (P o M) dO        dS = P o (dP - rowsum(dP o P)) * scale,  dP = (V dO^T) o M
 *       dQ = dS Kp             dKp = dS^T Q   (deterministic slice reduction, as the forward's P^T V)
 *   dq, dv [n, d], dkp [k, d] f32.  workspace: snf_sparse_attn_bwd_workspace_bytes (holds dS [h, n, k]).
 * --------------------------------------------------------------------------------------------------------- */
size_t snf_sparse_attn_bwd_workspace_bytes(int64_t n, int k, int h, int dk);
int snf_sparse_attn_bwd_f32(const float* q, const float* kp, const float* v, const float* p, const float* mask,
                            const float* dout, int64_t n, int k, int h, int dk, float scale, float* dq, float* dkp,
                            float* dv, void* workspace, size_t workspace_bytes, snf_stream_t stream);
/* The same with row pitches for q / v (elements, >= h dk; round 5): the halves of a fused [Q | V] projection output are read in place.
 * Pitches other than h dk need the matrix-core kernels (dk % 8 == 0, k <= 1024, 16-byte aligned rows), else SNF_EUNSUPPORTED. */
int snf_sparse_attn_bwd_ld_f32(const float* q, int64_t ldq, const float* kp, const float* v, int64_t ldv, const float* p, const float* mask,
                               const float* dout, int64_t n, int k, int h, int dk, float scale, float* dq, float* dkp, float* dv,
                               void* workspace, size_t workspace_bytes, snf_stream_t stream);
/* ... with the forward's dropout mask REGENERATED in the kernels from its Philox state (dropout_p, seed, offset: the arguments
 * snf_sparse_attn_fwd_x3_dropout was given) instead of read from a [h, n, k] tensor (round 6: the tensor was 157 MB written once and
 * read twice per config-B training step).  Only on the matrix-core route (k <= 1024, k % 4 == 0, dk % 8 == 0, 16-byte aligned operands);
 * SNF_EUNSUPPORTED otherwise -- hand the mask over as a tensor then. */
int snf_sparse_attn_bwd_dropout_f32(const float* q, int64_t ldq, const float* kp, const float* v, int64_t ldv, const float* p, float dropout_p,
                                    uint64_t seed, uint64_t offset, const float* dout, int64_t n, int k, int h, int dk, float scale, float* dq,
                                    float* dkp, float* dv, void* workspace, size_t workspace_bytes, snf_stream_t stream);
/* Fast form of the backward for dk == 128 with k <= 224 or dk == 64 with k <= 256 (bf16 MFMA operands, fp32 accumulate): P is recomputed from q, kp
 * and the forward's lse [h, n] (never read back), dQ / dV rows are owned by one wave (no reduction), dS [h, n, k] is
 * written out (ds_dtype f32, or bf16) -- the caller contracts it with q for dKp (snf_sparse_attn_dkp_f32 on f32, or a
 * bf16 library batched GEMM).  q, v as in
 * snf_sparse_attn_fwd_mfma (row-strided views allowed); mask as in snf_sparse_attn_bwd_f32.  Other shapes:
 * SNF_EUNSUPPORTED, the caller uses snf_sparse_attn_bwd_f32. */
int snf_sparse_attn_bwd_mfma(const void* q, int64_t ldq, const void* v, int64_t ldv, int qv_dtype, const float* kp,
                             const float* dout, const float* lse, const float* mask, int64_t n, int k, int h, int dk,
                             float scale, float* dq, float* dv, void* ds, int ds_dtype, snf_stream_t stream);
/* Same kernel with the gradients written where the caller wants them: dq / dv f32 or bf16 (dqv_dtype) with row pitch ldd
 * (elements) -- e.g. the two column halves of ONE [n, 2 d] bf16 buffer, the operand of the fused Q|V weight-gradient GEMM. */
int snf_sparse_attn_bwd_mfma_ex(const void* q, int64_t ldq, const void* v, int64_t ldv, int qv_dtype, const float* kp,
                                const float* dout, const float* lse, const float* mask, float dropout_p, uint64_t seed,
                                uint64_t offset, int64_t n, int k, int h, int dk, float scale, void* dq, void* dv, int64_t ldd,
                                int dqv_dtype, void* ds, int ds_dtype, snf_stream_t stream);
/* The same backward for MORE keys than one launch holds: dk == 128 with k <= 8 x 224 or dk == 64 with k <= 8 x 256 (the key chunks of
 * snf_sparse_attn_fwd_mfma's domain; chunk starts are multiples of 32).  The forward's lse is global, so P of a chunk is recomputed on
 * its own.  Series A, one launch per chunk: dV summed in fp32 over the chunks, then D = V . dV per head and row (= rowsum(P o dP), with
 * or without a mask).  Series B, one launch per chunk: dS = P o (dP - D) * scale at the chunk's columns of the full-width ds
 * [h, n, k], dQ summed the same way.  A wave owns its rows in every launch and the chunks are added in launch order: no atomics,
 * bit-reproducible.  The dropout mask -- tensor or (dropout_p, seed, offset) -- is keyed on the key index among ALL keys, as
 * snf_dropout_mask_f32 writes it.  Arguments as snf_sparse_attn_bwd_mfma_ex, plus the workspace (D, and the fp32 sums when dq / dv
 * leave as bf16; fp32 dq / dv are summed in place).  One chunk: forwards to snf_sparse_attn_bwd_mfma_ex (workspace may be NULL).
 * dk == 192 with k <= 8 x 128 (the forward's domain there) exists in this form only: chunks of up to 192 keys (two images of 144 KiB),
 * one launch per series even for a single chunk (the workspace is always needed); snf_sparse_attn_bwd_mfma[_ex] refuse dk == 192.
 * There dS = (bf16(P o M) o dPd - P D) * scale, the rounded factor being the one D was summed with: rows of dS sum to 0 in fp32.
 * dk == 256 with k <= 8 x 128 is the same case: chunks of up to 128 keys (two images of 128 KiB), this form only, the dS of dk == 192;
 * snf_sparse_attn_bwd_mfma[_ex] refuse dk == 256. */
size_t snf_sparse_attn_bwd_mfma_chunked_workspace_bytes(int64_t n, int k, int h, int dk, int dqv_dtype);
int snf_sparse_attn_bwd_mfma_chunked(const void* q, int64_t ldq, const void* v, int64_t ldv, int qv_dtype, const float* kp,
                                     const float* dout, const float* lse, const float* mask, float dropout_p, uint64_t seed,
                                     uint64_t offset, int64_t n, int k, int h, int dk, float scale, void* dq, void* dv, int64_t ldd,
                                     int dqv_dtype, void* ds, int ds_dtype, void* workspace, size_t workspace_bytes,
                                     snf_stream_t stream);
/* dKp [k, d] = dS^T Q per head (deterministic slice reduction); ds [h, n, k], q [n, d] f32.
 * workspace: snf_sparse_attn_bwd_workspace_bytes. */
int snf_sparse_attn_dkp_f32(const float* ds, const float* q, int64_t n, int k, int h, int dk, float* dkp, void* workspace,
                            size_t workspace_bytes, snf_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * K6 / K10 / K13  dense projection on the matrix cores      replaces nn.Linear (+ activation):
 *     snuffy.py:187-190 (Q | V and key projections), snuffy.py:224-225 (w_1 + activation, w_2),
 *     utils_ssls_cf/vision_transformer_with_adapter_dino_version.py:51-67 (Mlp), :82-94 (qkv / proj), :141-146 (patch embed)
 *   C[m, n] = act(A[m, k] W[n, k]^T + bias[n])   A, W bf16 row-major with row pitches lda / ldw (elements), bias f32 [n]
 *   (nullable), act = SNF_ACT_* (GELU = erf form, as nn.GELU), C bf16 or f32 (out_dtype = SNF_DT_*), row pitch ldc.
 *   Hand-written v_mfma_f32_16x16x32_bf16 kernel, fp32 accumulate; 256 x 256 or 256 x 128 output tiles (tile_n = 256 / 128,
 *   anything else = chosen from the shape).  Domain: k % 32 == 0, k >= 64, n % 8 == 0, rows 16-byte aligned, m * lda and
 *   n * ldw < 2^31; outside it SNF_EUNSUPPORTED (the caller keeps its library GEMM).
 *   out_dtype = SNF_DT_BF16_SPLIT3: C is the bf16 image [hi | hi | lo] of the fp32 result, [m, 3 n] (ldc >= 3 n) -- the
 *   hidden activations of the fp32-class FFN go from the first GEMM to the second without an fp32 round trip.
 *   out_dtype = SNF_DT_BF16_HL: C is the interleaved hl image of the fp32 result, [m, 2 n] (n % 32 == 0, ldc >= 2 n): the Q | V
 *   projection of bags too small for the one-pass kernel hands its result to snf_sparse_attn_fwd_x3_hl in this form.
 * --------------------------------------------------------------------------------------------------------- */
int snf_gemm_bf16(const void* a, int64_t lda, const void* w, int64_t ldw, const float* bias, int64_t m, int n, int k,
                  int act, void* c, int64_t ldc, int out_dtype, int tile_n, snf_stream_t stream);
/* Encoder dropout inside the FFN of a bf16 training step (nn.Dropout(encoder_dropout) of snuffy.py:225) in the epilogue of snf_gemm_bf16:
 *   C = bf16(M o relu(A W^T + bias)),  M[i, j] = 0 or 1 / (1 - dropout_p)
 * M is the Philox keep-mask of snf_dropout_mask_f32(dropout_p, seed, offset, h = 1, n = m, k = n), element (i, j) of it whatever the
 * tiling, regenerated in registers and applied to the fp32 value before the single bf16 rounding.  The one form that exists is
 * act = SNF_ACT_RELU with out_dtype = SNF_DT_BF16; anything else is SNF_EUNSUPPORTED.  dropout_p in [0, 1); 0 = the plain launch. */
int snf_gemm_bf16_dropout(const void* a, int64_t lda, const void* w, int64_t ldw, const float* bias, int64_t m, int n, int k, int act,
                          void* c, int64_t ldc, int out_dtype, int tile_n, float dropout_p, uint64_t seed, uint64_t offset,
                          snf_stream_t stream);
/* fp32 output with a residual in the epilogue: c = act(a w^T + bias) + resid [m, ldr] -- z = x + W2 act(W1 LN(y)) of snuffy.py:110 for
 * bags too small for the one-pass kernel (round 6; snf_gemm_hl_resid_bf16 is the large-bag twin) */
int snf_gemm_bf16_resid_f32(const void* a, int64_t lda, const void* w, int64_t ldw, const float* bias, const float* resid, int64_t ldr,
                            int64_t m, int n, int k, int act, float* c, int64_t ldc, int tile_n, snf_stream_t stream);
/* The ViT block without LayerNorm / residual passes (round 6; vd:97-127 "x = x + attn(norm1(x)); x = x + mlp(norm2(x)) + adapter(x)"):
 *   snf_gemm_bf16_lnfold   the consumer's LayerNorm folded into its GEMM: a = the RAW rows x rounded to bf16, w = W0 diag(gamma) (bf16),
 *                          c [m, ldc] bf16 = act(rstd[m] (a w^T - mean[m] colsum[n]) + bias[n]);  colsum[n] = sum_k w[n, k] of the ROUNDED w,
 *                          bias = W0 beta + b0, rowstats [m][2] = (mean, rstd) of the fp32 rows (snf_vit_row_stats).  act: none, gelu.
 *   snf_gemm_bf16_resid    the residual stream updated by the producer: x [m, ldx] fp32 IN PLACE  x += a w^T + bias; the bf16 copy of
 *                          the new x goes to x_bf16 [m, ldxb]; stats_part [m][n / 32][2] receives (sum, sum of squares) of the new
 *                          row over every 32-column group -- summed in group order by snf_vit_row_stats (bit-reproducible).
 *                          (256-wide tiles; 128-wide ones where the last 256-wide column tile would be at most half used: n = 384.)
 *   domain of both: k % 32 == 0, k >= 96, n % 64 == 0, 16-byte aligned rows. */
int snf_gemm_bf16_lnfold(const void* a, int64_t lda, const void* w, int64_t ldw, const float* colsum, const float* bias,
                         const float* rowstats, int64_t m, int n, int k, int act, void* c, int64_t ldc, snf_stream_t stream);
int snf_gemm_bf16_resid(const void* a, int64_t lda, const void* w, int64_t ldw, const float* bias, int64_t m, int n, int k, float* x,
                        int64_t ldx, void* x_bf16, int64_t ldxb, float* stats_part, snf_stream_t stream);
/* The same product in fp32-class arithmetic, ONE pass over the operands.  Both operands are INTERLEAVED split images ("hl"): a
 * row of 2 k bf16 in which every 32 true columns are stored as [hi(32) | lo(32)] (hi = bf16(v), lo = bf16(v - hi)) -- one
 * 128-byte line per K step and the same 4 bytes per element as the fp32 tensor.  C = act(A W^T + bias) with every product taken
 * as hi hi + hi lo + lo hi, fp32 accumulate (~1e-5 per product).  A K step stages ONE line per operand row by full-line LDS-DMA
 * and issues 96 MFMAs per wave out of 24 fragment reads.  256 x 256 tiles; k % 32 == 0; out_dtype SNF_DT_F32 / SNF_DT_BF16 /
 * SNF_DT_BF16_HL (the hl image of the result, [m, 2 n], n % 32 == 0: the A operand of the next such GEMM).
 *   snf_split_hl_f32            x [m, k] f32 (row pitch ldx) -> its hl image [m, 2 k]
 *   snf_layernorm_rows_hl_f32   snf_layernorm_rows_f32 whose output is written as the hl image (d % 32 == 0)
 * nn.Linear of snuffy.py:187-190,224-225 and of the ViT blocks in the reference's fp32 arithmetic. */
int snf_gemm_hl_bf16(const void* a_hl, int64_t lda, const void* w_hl, int64_t ldw, const float* bias, int64_t m, int n, int k,
                     int act, void* c, int64_t ldc, int out_dtype, snf_stream_t stream);
/* fp32 output with a residual: C = act(A W^T + bias) + resid [m, ldr] -- z = x + W2 act(W1 LN(y)) of snuffy.py:110 in one pass */
int snf_gemm_hl_resid_bf16(const void* a_hl, int64_t lda, const void* w_hl, int64_t ldw, const float* bias, const float* resid,
                           int64_t ldr, int64_t m, int n, int k, int act, void* c, int64_t ldc, int out_dtype, snf_stream_t stream);
/* The same with split-K of the LAST, partly filled round of 256 x 256 tiles (e.g. the FFN output projection of config B: 384 tiles on
 * 256 CUs): each tile of that round goes to 2..4 workgroups, a K range each; the last one to finish adds the others' fp32 partial tiles
 * in a fixed order and runs the epilogue (bit-reproducible; any activation / output type / residual).  workspace: at least
 * snf_gemm_hl_ws_bytes(m, n, k) bytes (0 = this shape does not split; workspace may then be NULL); plain scratch memory -- the call
 * zeroes its own tickets, nothing is expected in the buffer before a call or kept in it after one, so concurrent calls on different
 * streams only need different buffers.  NULL workspace = snf_gemm_hl_resid_bf16. */
size_t snf_gemm_hl_ws_bytes(int64_t m, int n, int k);
/* The FFN input gradient of the training step behind its ReLU (backward of snuffy.py:224-225: dhid = (dz W2) o [hid > 0]) in ONE pass:
 * c_hl [m, 2 n] = the hl image of (a w^T) with every element zeroed whose gate value -- the hi half of gate_hl [m, 2 n], the activation's own
 * hl image -- is not > 0.  Domain of snf_gemm_hl_bf16 with an hl output (n % 32 == 0). */
int snf_gemm_hl_gated_bf16(const void* a_hl, int64_t lda, const void* w_hl, int64_t ldw, const void* gate_hl, int64_t ldg, int64_t m, int n,
                           int k, void* c_hl, int64_t ldc, snf_stream_t stream);
/* The weight-gradient contraction of the training step (round 6; the autograd of nn.Linear under train.py:259,468-473: dW = dY^T X):
 *   c [p, ldc] f32 = A^T B over the n rows of two row-major bf16 images, on the matrix cores straight from those images (transposing
 *   LDS reads; no transposed copy).  A's operand is the p columns starting at column a_hi of a [n, lda], B's the q columns at b_hi of
 *   b [n, ldb].  a_lo, b_lo >= 0: the operands are split images with a lo plane at those column offsets (the [hi | hi | lo] images of
 *   snf_split3_colsum_f32 / snf_layernorm_rows_split3_f32 / a split3 GEMM output) and the product is fp32-class, hi hi + hi lo + lo hi;
 *   both -1: one bf16 product.  Tiles of 256 x 256 cut into row parts (one workgroup each), summed in part order (bit-reproducible).
 *   hl != 0: both operands are INTERLEAVED images instead ([hi(32) | lo(32)] per 32 columns; a_hi / b_hi = the image column where the
 *   operand starts, a multiple of 64; a_lo, b_lo ignored; p % 32 == 0, q % 32 == 0) -- full 128-byte lines all the way.
 *   workspace: snf_gemm_tn_ws_bytes(n, p, q) bytes of plain scratch memory.  Domain: n >= 1 (the rows are consumed in steps of 32; a
 *   last step of n % 32 rows stages only those rows and zeros for the others -- nothing beyond row n - 1 of a or b is read, the
 *   buffers may end there), p % 8 == 0, q % 8 == 0, plane offsets % 8 == 0, 16-byte aligned rows. */
size_t snf_gemm_tn_ws_bytes(int64_t n, int p, int q);
int snf_gemm_tn_f32(const void* a, int64_t lda, int a_hi, int a_lo, const void* b, int64_t ldb, int b_hi, int b_lo, int hl, int64_t n, int p,
                    int q, float* c, int64_t ldc, void* workspace, size_t workspace_bytes, snf_stream_t stream);
int snf_gemm_hl_ws_bf16(const void* a_hl, int64_t lda, const void* w_hl, int64_t ldw, const float* bias, const float* resid,
                        int64_t ldr, int64_t m, int n, int k, int act, void* c, int64_t ldc, int out_dtype, void* workspace,
                        size_t workspace_bytes, snf_stream_t stream);
/* The split of the last round WITHOUT its sum, for an fp32 result with exactly one reader that can add as it reads (the eval forward's last
 * FFN output projection, read by snf_ln_mean_head_deferred_f32): same geometry, two K parts at most.  Part 0 of a split tile runs the
 * ordinary epilogue (bias, residual) into c; part 1 writes its bare partial tile into a 256 x 256 fp32 slab of the workspace.  No
 * tickets, no slab reads, nobody waits.  After the call
 *     result tile t = c tile t + (map[t] ? slab[map[t] - 1] : 0),   t = (row / 256) * ceil(n / 256) + col / 256
 * with the int32 tile map at workspace offset 0 (written in full by every call) and the slabs [..][256][256] at *slab_offset (private
 * to their tiles: rows / columns past m / n hold values nobody reads).  snf_gemm_hl_deferred_ws_bytes: workspace size, 0 = the shape does
 * not split (use snf_gemm_hl_resid_bf16); slab_offset nullable.  The workspace is part of the RESULT: it lives as long as c is read.
 * act must be SNF_ACT_NONE and out_dtype SNF_DT_F32 (anything else: SNF_EUNSUPPORTED); workspace 128-byte aligned. */
size_t snf_gemm_hl_deferred_ws_bytes(int64_t m, int n, int k, size_t* slab_offset);
int snf_gemm_hl_deferred_f32(const void* a_hl, int64_t lda, const void* w_hl, int64_t ldw, const float* bias, const float* resid,
                             int64_t ldr, int64_t m, int n, int k, int act, float* c, int64_t ldc, int out_dtype, void* workspace,
                             size_t workspace_bytes, snf_stream_t stream);
/* Encoder dropout of a training step (nn.Dropout(encoder_dropout) of snuffy.py:225 and :110) in the epilogue of the one-pass GEMM:
 *   C = M o act(A W^T + bias) (+ resid: the residual is NOT masked),  M[i, j] = 0 or 1 / (1 - dropout_p)
 * M is the Philox keep-mask of snf_dropout_mask_f32(dropout_p, seed, offset, h = 1, n = m, k = n) -- element (i, j) of it whatever the tiling
 * and whichever workgroup runs the epilogue (split-K included), regenerated in registers and never stored; the product is rounded before
 * the residual is added, so the result is bit for bit (undropped result) * (mask tensor) (+ resid).  Two forms:
 *   act = SNF_ACT_RELU, out_dtype = SNF_DT_BF16_HL, resid = NULL   the FFN hidden layer as its hl image (masked before the hi / lo split)
 *   act = SNF_ACT_NONE, out_dtype = SNF_DT_F32 (resid nullable)    z = x + dropout(W2 hid + b2)
 * anything else is SNF_EUNSUPPORTED.  dropout_p in [0, 1); 0 = the plain launch.  _ws_: with the split-K workspace of snf_gemm_hl_ws_bf16. */
int snf_gemm_hl_dropout_bf16(const void* a_hl, int64_t lda, const void* w_hl, int64_t ldw, const float* bias, const float* resid,
                             int64_t ldr, int64_t m, int n, int k, int act, void* c, int64_t ldc, int out_dtype, float dropout_p,
                             uint64_t seed, uint64_t offset, snf_stream_t stream);
int snf_gemm_hl_ws_dropout_bf16(const void* a_hl, int64_t lda, const void* w_hl, int64_t ldw, const float* bias, const float* resid,
                                int64_t ldr, int64_t m, int n, int k, int act, void* c, int64_t ldc, int out_dtype, float dropout_p,
                                uint64_t seed, uint64_t offset, void* workspace, size_t workspace_bytes, snf_stream_t stream);
/* Its backward: snf_split_hl_colsum_f32 of M o x with the same mask M [m, k] regenerated from (dropout_p, seed, offset) in the same pass --
 * the hl image of df = M o dz and its column sums, no [m, k] mask tensor. */
int snf_split_hl_colsum_dropout_f32(const float* x, int64_t ldx, int64_t m, int k, const void* gate_hl, int64_t ldg, float dropout_p,
                                    uint64_t seed, uint64_t offset, void* out_hl, int64_t ldo, float* partial, snf_stream_t stream);
int snf_split_hl_f32(const float* x, int64_t ldx, int64_t m, int k, void* out_bf16, snf_stream_t stream);
int snf_layernorm_rows_hl_f32(const float* x, int64_t n, int d, const int32_t* slot_map, const float* patch_rows,
                              const float* gamma, const float* beta, float eps, void* out_bf16, snf_stream_t stream);
/* The K patched rows of a bag, re-normalised INTO an existing hl image (snuffy.py:108 + 110 for the selected rows only): row j of
 * (x [n, d] + addend [n, d] or NULL) is layer-normalised (gamma / beta NULL = no affine) and written as the hl row out_row_idx[j]
 * of out_hl [*, 2 d].  With one normalised image serving both sublayers of an encoder layer (LayerNorm affines folded into the
 * projections) this replaces the second full LayerNorm pass over the bag. */
int snf_layernorm_rows_hl_patch_f32(const float* x, const float* addend, int64_t n, int d, const int64_t* out_row_idx,
                                    const float* gamma, const float* beta, float eps, void* out_hl, snf_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * K12-K14  ViT patch-embedding extractor (compute_feats.py:239-247 -> IClassifier -> VisionTransformer.forward)
 *   reference model files: utils_ssls_cf/vision_transformer_with_adapter_dino_version.py (vd), vision_transformer_dino.py,
 *   adapter.py, models_adapter_mae.py.  The dense projections are snf_gemm_bf16 (above) or library GEMMs by a measured shape policy; these entry points are the rest.
 *
 *   snf_vit_patchify         im2col of PatchEmbed's Conv2d(3, D, p, p)                vd:141-146
 *       img [b, c, hgt, wid] f32 -> cols [b * (hgt/p) * (wid/p), c*p*p] (f32 or bf16), column order (c, i, j) = the
 *       flattening of the conv weight [D, c, p, p].
 *   snf_vit_assemble_tokens  tokens[b,0] = cls + pos[0]; tokens[b,1+i] = patch_emb[b*P+i] + pos[1+i]   vd:218-229
 *       (identical arithmetic for the MAE encoder, models_adapter_mae.py:176-186).  tokens [b, P+1, d] f32.
 *   snf_vit_residual_ln      x += add1 + scale2 * add2 (bf16 addends, nullable); ln_out = LayerNorm(x) (bf16, nullable);
 *       x_bf16 = x (nullable): the two residual adds of Block.forward fused with the following norm      vd:120-127
 *   snf_vit_attention_f32    exact multi-head self-attention  softmax(q k^T * scale) v                  vd:82-94
 *       qkv [b*t, 3*h*dk] f32 laid out as the reference's qkv Linear output (q | k | v, each [h][dk]);
 *       out [b*t, h*dk]; attn [b, h, t, t] nullable.  dk in {32, 64, 96, 128}.
 *   snf_vit_attention_mfma   same on the matrix cores, bf16 in / bf16 out, dk == 64, t <= SNF_VIT_MFMA_MAX_T (else
 *       SNF_EUNSUPPORTED).  t <= 256: the keys of an (image, head) sit in one LDS image; above (the reference's patch-8 recipe,
 *       README.md:552-565: t = 785) they are staged 256 at a time and a workgroup keeps its query tiles' softmax state across the chunks.
 *   snf_vit_attention_x3_f32 same program in the fp32-class arithmetic (every product hi hi + hi lo + lo hi on the bf16 matrix
 *       cores, fp32 accumulate): fp32 in, dk == 64, t <= SNF_VIT_MFMA_MAX_T; out [b*t, h*dk] f32 (out_dtype SNF_DT_F32) or its
 *       interleaved hl image [b*t, 2*h*dk] bf16 (SNF_DT_BF16_HL: the operand of the one-pass proj GEMM).  Does not materialise attn.
 * --------------------------------------------------------------------------------------------------------- */
int snf_vit_patchify(const float* img, int b, int c, int hgt, int wid, int patch, void* cols, int out_dtype,
                     snf_stream_t stream);
int snf_vit_assemble_tokens(const void* patch_emb, int pe_dtype, const float* cls_token, const float* pos_embed, int b,
                            int num_patches, int d, float* tokens, snf_stream_t stream);
int snf_vit_residual_ln(float* x, int64_t n, int d, const void* add1_bf16, const void* add2_bf16, float scale2,
                        const float* gamma, const float* beta, float eps, void* ln_out_bf16, void* x_bf16,
                        snf_stream_t stream);
/* (mean, rstd) [n][2] of LayerNorm(eps) for snf_gemm_bf16_lnfold: from the fp32 rows x [n, ldx] (then x_bf16, nullable, receives
 * their bf16 copy -- the GEMM's operand) or from the moment pairs part [n][slots][2] a snf_gemm_bf16_resid left.  Exactly one of x / part. */
int snf_vit_row_stats(const float* x, int64_t ldx, const float* part, int slots, int64_t n, int d, float eps, float* stats,
                      void* x_bf16, int64_t ldxb, snf_stream_t stream);
int snf_vit_attention_f32(const float* qkv, int b, int t, int h, int dk, float scale, float* out, float* attn,
                          snf_stream_t stream);
#define SNF_VIT_MFMA_MAX_T 4096
int snf_vit_attention_mfma(const void* qkv_bf16, int b, int t, int h, int dk, float scale, void* out_bf16,
                           snf_stream_t stream);
int snf_vit_attention_x3_f32(const float* qkv, int b, int t, int h, int dk, float scale, void* out, int out_dtype, snf_stream_t stream);
/* Training pair of the MFMA self-attention (adapter pre-training, snuffy_amd/ssl_pretrain.py): O(b h t) saved state.
 *   snf_vit_attention_fwd_lse  the forward above with one more output, lse [b, h, t] f32 = log sum_j exp(scale q_i . k_j) (natural
 *       log).  dtype SNF_DT_BF16: the program of snf_vit_attention_mfma (bf16 in / out); SNF_DT_F32: the program of
 *       snf_vit_attention_x3_f32 (fp32 in / out).  `out` is bit for bit what those entry points write; same shape domain.
 *   snf_vit_attention_bwd      qkv as given to the forward, dout [b*t, h*dk], lse from the forward -> dqkv [b*t, 3*h*dk] laid out as
 *       qkv (dQ | dK | dV), every element written.  SNF_DT_F32: fp32 tensors, every product hi hi + hi lo + lo hi on the bf16 matrix
 *       cores with fp32 accumulation (P and dS split in registers); SNF_DT_BF16: bf16 tensors, P and dS rounded to bf16 as operands,
 *       fp32 accumulation.  Neither the probabilities nor the forward's output are needed: P is rebuilt from q, k and lse, and
 *       D_i = sum_j P_ij dP_ij.  Deterministic (no atomics, one summation order).  dk == 64, 1 <= t <= SNF_VIT_BWD_MAX_T (the keys
 *       of an (image, head) in one LDS image), b <= 65535, qkv / dout / dqkv 16-byte aligned; anything else: SNF_EUNSUPPORTED.
 *   snf_vit_attention_bwd_long the same backward for SNF_VIT_BWD_MAX_T < t <= SNF_VIT_BWD_LONG_MAX_T, as two launches on `stream`
 *       (D and dQ per query tile over 256-key chunks, then dK and dV per key tile over 256-query chunks).  dwork [b, h, t] f32 is
 *       scratch the first launch fills (D, every row) and the second reads.  Same operands, arithmetics, determinism and refusals
 *       otherwise; t <= SNF_VIT_BWD_MAX_T is SNF_EUNSUPPORTED here (snf_vit_attention_bwd serves it). */
#define SNF_VIT_BWD_MAX_T 256
#define SNF_VIT_BWD_LONG_MAX_T 4096
int snf_vit_attention_fwd_lse(const void* qkv, int dtype, int b, int t, int h, int dk, float scale, void* out, float* lse,
                              snf_stream_t stream);
int snf_vit_attention_bwd(const void* qkv, const void* dout, const float* lse, int dtype, int b, int t, int h, int dk, float scale,
                          void* dqkv, snf_stream_t stream);
int snf_vit_attention_bwd_long(const void* qkv, const void* dout, const float* lse, int dtype, int b, int t, int h, int dk,
                               float scale, float* dwork /* [b, h, t] f32, scratch, fully overwritten for rows < t */,
                               void* dqkv, snf_stream_t stream);
/* The same training pair at head width 32 (the MAE decoder of adapter pre-training: 512 wide, 16 heads, t = 197), csrc/vit_attn_dk32.hip.
 *   snf_vit_attention_dk32_fwd_lse  qkv [b*t, 3*h*32] (q | k | v) -> out [b*t, h*32] and lse [b, h, t] f32 (natural log, required).
 *       One workgroup per (image, head), online softmax over 32-key blocks.  SNF_DT_BF16: bf16 in / out; SNF_DT_F32: fp32 in / out
 *       in the fp32-class arithmetic (hi hi + hi lo + lo hi on the bf16 matrix cores, fp32 accumulation).
 *   snf_vit_attention_dk32_bwd      qkv as given to the forward, dout [b*t, h*32], lse from the forward -> dqkv [b*t, 3*h*32] laid out
 *       as qkv (dQ | dK | dV), every element written.  The arithmetics, the rebuilt P, D_i = sum_j P_ij dP_ij and the determinism
 *       (no atomics, one summation order) are those of snf_vit_attention_bwd; t == 1 is an exact copy (dQ = dK = 0, dV = dout).
 *   Both: dk == 32 (the argument is kept so the call shape matches the 64-wide pair), 1 <= t <= SNF_VIT_DK32_MAX_T, b <= 65535,
 *       qkv / out / dout / dqkv 16-byte aligned; anything else: SNF_EUNSUPPORTED. */
#define SNF_VIT_DK32_MAX_T 256
int snf_vit_attention_dk32_fwd_lse(const void* qkv, int dtype, int b, int t, int h, int dk, float scale,
                                   void* out, float* lse, snf_stream_t stream);
int snf_vit_attention_dk32_bwd(const void* qkv, const void* dout, const float* lse, int dtype, int b, int t,
                               int h, int dk, float scale, void* dqkv, snf_stream_t stream);
/* Row passes of the frozen-trunk training route (adapter pre-training in fp32, csrc/vit_train.hip): the erf GELU between the two GEMMs
 * of a frozen MLP, written as the operand image of the next fp32-class GEMM; the fp32 value exists in registers only.
 *   snf_gelu_image_f32      pre [m, n] f32 (row pitch ldp) -> the image of gelu(pre) = 0.5 pre (1 + erf(pre / sqrt 2))
 *   snf_gelu_bwd_image_f32  da [m, n] f32 (row pitch ldda) and pre -> the image of da * gelu'(pre), gelu'(x) = Phi(x) + x phi(x)
 *   out_dtype SNF_DT_BF16_HL: out_img [m, 2 n] as snf_split_hl_f32 writes it, n % 32 == 0; SNF_DT_BF16_SPLIT3: out_img [m, 3 n] =
 *   [hi | hi | lo] as snf_split3_f32 writes it, n % 8 == 0.  hi = bf16(v), lo = bf16(v - hi), the same values in both images.
 *   m >= 1, m * n < 2^33, pitches multiples of 4 floats, every buffer 16-byte aligned, out_img contiguous; else SNF_EINVAL. */
int snf_gelu_image_f32(const float* pre, int64_t ldp, int64_t m, int n, void* out_img, int out_dtype, snf_stream_t stream);
int snf_gelu_bwd_image_f32(const float* da, int64_t ldda, const float* pre, int64_t ldp, int64_t m, int n, void* out_img,
                           int out_dtype, snf_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * Tile preprocessing for the extractor, batched on the device     replaces the per-tile CPU transforms of
 *     compute_feats.py:104-152,173-177: Resize(224) (PIL bilinear + antialiasing), ToTensor (/ 255), NormalizeImage
 *   img_u8 [b, h, w, c] uint8 (decoded tiles, channels last, c <= 4).  The resize is Pillow's 8-bit resampler: horizontal
 *   then vertical pass with the integer coefficient tables computed by the caller (snuffy_amd/tiles.py restates Pillow's
 *   precompute_coeffs / normalize_coeffs_8bpc): hbounds [ow][2] = (first input column, count), hcoef [ow][hks]; vbounds /
 *   vcoef likewise for rows (device int32 arrays).  mean / std: HOST arrays of c floats (used when normalize != 0).
 *   Outputs, either nullable: out_f32 [b, c, oh, ow]; cols_bf16 [b * (oh/patch) * (ow/patch), c * patch * patch] = the
 *   patch-embedding GEMM operand (column order (c, i, j)).  Bit-exact against PIL + torch on the same tiles.
 * --------------------------------------------------------------------------------------------------------- */
int snf_tile_preprocess_u8(const void* img_u8, int b, int h, int w, int c, int oh, int ow, const int* hbounds, const int* hcoef,
                           int hks, const int* vbounds, const int* vcoef, int vks, int normalize, const float* mean,
                           const float* std_, float* out_f32, void* cols_bf16, int patch, snf_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * Training augmentations, batched on the device     replaces the per-crop PIL transforms of DataAugmentationDINO
 *     (main_dino_adapter.py:674-745) and of the MAE pre-training loader (main_pretrain_adapter.py: RandomResizedCrop + flip)
 *   tiles_u8 [b, h, w, 3] uint8 (decoded tiles, RGB).  records: n_records 64-byte records (n_records a multiple of b, record r
 *   crops tile r % b), 16 little-endian words each:
 *     int32 top, left, ch, cw (crop box), flip, jitter (colour jitter applied), order (jitter operation k in bits 2k .. 2k + 1:
 *     0 brightness, 1 contrast, 2 saturation, 3 hue), gray; float brightness, contrast, saturation, hue factors, blur (Gaussian
 *     radius, <= 0: none); int32 solarize, fallback (written by the draw: the centred crop was taken), pad.
 *   snf_augment_apply_u8: crop -> bicubic resize to size x size -> flip -> jitter -> grayscale -> blur -> solarise, every stage
 *     uint8 and bit-identical to Pillow, then (u8 / 255 - mean) / std -> out_f32 [n_records, 3, size, size].  mean / std: HOST
 *     arrays of 3 floats.  workspace: snf_augment_workspace_bytes(h, w, size, n_records) bytes, 16-byte aligned (SNF_EWORKSPACE if
 *     smaller).  Bounds: size <= 256, h, w <= 1024 and <= 8 * size (every crop then reduces by at most 8: 33 taps); outside:
 *     SNF_EUNSUPPORTED before any launch.  A record outside the tile is clamped into it, not reported: check tables on the host.
 *   snf_augment_draw: fills views * b records (record v * b + i = view v of tile i) from Philox4x32-10 (key = state[0], counter =
 *     (record, block, state[1])); state as for snf_sampler_advance, which the caller runs behind the draw.  policies: HOST array
 *     of views * 20 doubles: scale lo, hi; p_flip; p_jitter; brightness lo, hi; contrast lo, hi; saturation lo, hi; hue lo, hi;
 *     p_gray; p_blur; blur radius lo, hi; p_solarize; 3 unused.  views <= 16.  The blocks and words: DESIGN.md 4.
 * --------------------------------------------------------------------------------------------------------- */
size_t snf_augment_workspace_bytes(int h, int w, int size, int n_records);
int snf_augment_draw(const void* state, const double* policies, int views, int b, int h, int w, void* records, snf_stream_t stream);
int snf_augment_apply_u8(const void* tiles_u8, int b, int h, int w, const void* records, int n_records, int size, const float* mean,
                         const float* std_, float* out_f32, void* workspace, size_t workspace_bytes, snf_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * Varlen path: MANY bags in one launch (bags of <= 8 k patches are launch-latency bound).
 *     The reference runs one bag per forward (train.py:468-473 batch_size 1; snuffy.py:130-131 indexes with a 1-D tensor); this
 *     is the same per-bag arithmetic with the bags' rows PACKED into one [T, .] tensor, offsets[bags + 1] = first row of each bag.
 *     Row-wise kernels (critic, LayerNorm, the projections, the FFN) already take packed rows; the three per-bag reductions get
 *     segmented forms.  Every segmented launch is the CONCATENATION of per-bag grids (workgroup wg0 + i of bag b does what
 *     workgroup i of a launch of that bag alone does): a bag's result never depends on what it is packed with, bit for bit.
 *     top-k and the head are also bit-identical to the single-bag entry points above; the attention launches give small bags
 *     more rows per workgroup than a lone launch would (fewer partial tiles), so against snf_sparse_attn_fwd_mfma / _x3 the
 *     fp32 summation order of the [k, dk] partial tiles can differ (<= 1e-6 relative).
 *   snf_topk_segmented_f32       K2 of every bag (offsets in DEVICE memory; idx_out [bags, k] = indices inside the bag; a bag
 *                                with fewer than k rows fills its first n_b entries only).
 *   snf_sparse_attn_varlen_plan / snf_sparse_attn_x3_varlen_plan
 *                                host-side geometry of a varlen attention launch: offsets in HOST memory; call with
 *                                table = NULL for the sizes, then with a host buffer of *table_ints_needed int32 words, upload
 *                                it once per batch composition and pass the device copy to the launch.
 *   snf_sparse_attn_fwd_mfma_varlen   K7 bf16 form: q, v [T, ld] bf16, kp [bags * k, h * dk] (bag b's keys in rows b k ..),
 *                                out [bags * k, h * dk] f32, attn [h, T, k] / lse [h, T] nullable.  Single key chunk
 *                                (k <= 224 at dk = 128, 256 at dk = 64), inference only (no dropout).
 *   snf_sparse_attn_fwd_x3_varlen     K7 fp32-class form on f32 q, v, kp; same layout and limits.
 *   snf_ln_mean_head_varlen_plan / snf_ln_mean_head_varlen_f32
 *                                K11 for every bag: logits [bags, c_out], pooled [bags, d] nullable.
 * --------------------------------------------------------------------------------------------------------- */
int snf_topk_segmented_f32(const float* scores, const int64_t* offsets_dev, int bags, int64_t max_n, int k, int64_t* idx_out,
                           snf_stream_t stream);
/* ---------------------------------------------------------------------------------------------------------
 * K2m class-union selection of the multiclass model          replaces snuffy_multiclass.py:136-141 (per class torch.sort, top
 *     rows, flatten, torch.unique) for every batch row in ONE launch.
 *   snf_multiclass_select_f32: scores [b, n, c] f32 contiguous.  For row i and every class j the k1 highest of scores[i, :, j]
 *     (descending score, ties by ascending index: the rule of snf_topk_f32, the same for +-0 / +-inf / NaN); the union of those
 *     indices, ascending and duplicate-free, goes to uniq_out[i, 0 .. count_out[i]) (uniq_out [b, c * k1] int64, count_out [b]
 *     int32, both in device memory; entries past the count are not written).
 *   One workgroup per batch row, the classes looped inside it; no workgroup waits for another and nothing but plain stores
 *     reaches global memory: bit-identical on every run.
 *   Domain: 1 <= k1 <= min(n, 2048), c * k1 <= 4096, n < 2^30; outside it SNF_EUNSUPPORTED / SNF_EINVAL.
 * --------------------------------------------------------------------------------------------------------- */
int snf_multiclass_select_f32(const float* scores, int b, int64_t n, int c, int k1, int64_t* uniq_out, int32_t* count_out,
                              snf_stream_t stream);
int snf_sparse_attn_varlen_plan(const int64_t* offsets, int bags, int k, int h, int dk, int32_t* table, size_t table_ints,
                                size_t* table_ints_needed, size_t* workspace_bytes);
int snf_sparse_attn_fwd_mfma_varlen(const void* q, int64_t ldq, const void* v, int64_t ldv, const void* kp, int kp_dtype,
                                    const int64_t* offsets, int bags, int k, int h, int dk, float scale, float* out, float* attn,
                                    float* lse, const int32_t* table_dev, void* workspace, size_t workspace_bytes,
                                    snf_stream_t stream);
int snf_sparse_attn_x3_varlen_plan(const int64_t* offsets, int bags, int k, int h, int dk, int32_t* table, size_t table_ints,
                                   size_t* table_ints_needed, size_t* workspace_bytes);
int snf_sparse_attn_fwd_x3_varlen(const float* q, int64_t ldq, const float* v, int64_t ldv, const float* kp, const int64_t* offsets,
                                  int bags, int k, int h, int dk, float scale, float* out, float* attn, float* lse,
                                  const int32_t* table_dev, void* workspace, size_t workspace_bytes, snf_stream_t stream);
/* Varlen attention ABOVE ONE KEY CHUNK (k up to 8 x 224 at dk = 128, 8 x 256 at dk = 64; dk = 192: the _dk192 pair below).  The keys run as the
 * chunks of the single-bag entry point of the same family (bf16: ceil(k / chunks) keys; fp32-class: that, rounded up to a multiple
 * of 4; the last chunk is shorter): one statistics launch per chunk over all bags, then the chunks' main launches, each normalising
 * with the statistics of all chunks -- a bag's attn and lse are those of snf_sparse_attn_fwd_mfma / _x3 on that bag alone, bit for bit,
 * out within the fp32 order of the partial sums, and nothing depends on what a bag is packed with.
 *   ..._chunked_plan   as the plans above (one table serves every chunk: a bag's tile geometry depends on n and h only; word 3 of a
 *                      descriptor stays b k), plus the chunk count and the size of all chunks but the last (either nullable).
 *                      Workspace = partial tiles at the largest chunk's key-block count | statistics [chunks][h][T] (max, sum) pairs
 *                      over all T packed rows, 8 bytes each (none with one chunk) | bf16 form: Kp staging.  At k within one chunk: one
 *                      chunk and the table of the plan above, integer for integer.  SNF_EUNSUPPORTED: k > 8 chunks, dk outside
 *                      {64, 128}, an empty bag.
 *   ..._varlen_chunked the launches; arguments and layouts as snf_sparse_attn_fwd_mfma_varlen / _x3_varlen, table and workspace from
 *                      the chunked plan.  With one chunk they are those entry points. */
int snf_sparse_attn_varlen_chunked_plan(const int64_t* offsets, int bags, int k, int h, int dk, int32_t* table, size_t table_ints,
                                        size_t* table_ints_needed, size_t* workspace_bytes, int* n_chunks, int* chunk_k);
int snf_sparse_attn_fwd_mfma_varlen_chunked(const void* q, int64_t ldq, const void* v, int64_t ldv, const void* kp, int kp_dtype,
                                            const int64_t* offsets, int bags, int k, int h, int dk, float scale, float* out,
                                            float* attn, float* lse, const int32_t* table_dev, void* workspace,
                                            size_t workspace_bytes, snf_stream_t stream);
int snf_sparse_attn_x3_varlen_chunked_plan(const int64_t* offsets, int bags, int k, int h, int dk, int32_t* table, size_t table_ints,
                                           size_t* table_ints_needed, size_t* workspace_bytes, int* n_chunks, int* chunk_k);
int snf_sparse_attn_fwd_x3_varlen_chunked(const float* q, int64_t ldq, const float* v, int64_t ldv, const float* kp,
                                          const int64_t* offsets, int bags, int k, int h, int dk, float scale, float* out, float* attn,
                                          float* lse, const int32_t* table_dev, void* workspace, size_t workspace_bytes,
                                          snf_stream_t stream);
/* Varlen bf16 attention at HEAD WIDTH 192 (the reference README's MAE recipe: D = 768, h = 4, Lambda = 500).  The plan functions above
 * keep answering SNF_EUNSUPPORTED at dk = 192; the width has entry points of its own, with the protocol of the chunked pair.  One launch
 * holds 128 keys (Kp 48 + P 40 + V 48 KiB of LDS at 4 key blocks); more keys run as the chunks of snf_sparse_attn_fwd_mfma at dk = 192
 * (ceil(k / chunks) keys, the last chunk shorter): one statistics launch per chunk over all bags, then the chunks' main launches.  A
 * bag's attn and lse are those of snf_sparse_attn_fwd_mfma on that bag alone, bit for bit, out within the fp32 order of the partial
 * sums, and nothing depends on what a bag is packed with.  bf16 q | v only; inference only (no dropout).
 *   snf_sparse_attn_varlen_dk192_plan      1 <= k <= 8 x 128.  table = NULL sizes the table; n_chunks / chunk_k nullable.  Workspace =
 *                      partial tiles at the largest chunk's key-block count | statistics [chunks][h][T] (max, sum) pairs over all T
 *                      packed rows, 8 bytes each (none with one chunk) | Kp staging (used when kp is f32).  SNF_EUNSUPPORTED: k above
 *                      8 chunks, an empty bag, a chunk whose key-block count is not built (one chunk: 1, 2, 4; chunked: 2, 4).
 *   snf_sparse_attn_fwd_mfma_varlen_dk192  arguments and layouts of snf_sparse_attn_fwd_mfma_varlen_chunked without dk. */
int snf_sparse_attn_varlen_dk192_plan(const int64_t* offsets, int bags, int k, int h, int32_t* table, size_t table_ints,
                                      size_t* table_ints_needed, size_t* workspace_bytes, int* n_chunks, int* chunk_k);
int snf_sparse_attn_fwd_mfma_varlen_dk192(const void* q, int64_t ldq, const void* v, int64_t ldv, const void* kp, int kp_dtype,
                                          const int64_t* offsets, int bags, int k, int h, float scale, float* out, float* attn,
                                          float* lse, const int32_t* table_dev, void* workspace, size_t workspace_bytes,
                                          snf_stream_t stream);
/* fp32-class (split-bf16 x 3) attention at HEAD WIDTH 192, FUSED: softmax and P^T V in one kernel, no materialised [h, n, k]
 * probabilities in between (snf_sparse_attn_fwd_x3u_f32 is the unfused pair).  snf_sparse_attn_fwd_x3 and the x3 plan functions above
 * keep answering SNF_EUNSUPPORTED at dk = 192; the width has entry points of its own.  One launch holds 128 keys (1, 2 or 4 key blocks;
 * Q 48 + P 40 + V 48 + statistics 4 KiB of LDS at 4 blocks, the Kp fragments in registers); more keys run as up to 8 chunks of
 * ceil(k / chunks) keys rounded up to a multiple of 4 (the last chunk shorter; chunked launches run at 2 or 4 key blocks): one
 * statistics launch per chunk, then the chunks' main launches, each normalising with the statistics of all chunks.  Inference only.
 *   ..._x3_dk192_workspace_bytes  0 = unsupported (k outside 1 .. 8 x 128, n < 1, h < 1).
 *   snf_sparse_attn_fwd_x3_dk192  arguments, layouts, alignment rules and error codes of snf_sparse_attn_fwd_x3 without dk.
 *   snf_sparse_attn_x3_varlen_dk192_plan  as snf_sparse_attn_x3_varlen_chunked_plan without dk: one table for all chunks, descriptor
 *                      word 3 = b k with the full key count, workspace = partial tiles at the largest chunk's key-block count |
 *                      statistics [chunks][h][T] (none with one chunk).  SNF_EUNSUPPORTED: k outside 1 .. 8 x 128, an empty bag.
 *   snf_sparse_attn_fwd_x3_varlen_dk192   arguments and layouts of snf_sparse_attn_fwd_x3_varlen_chunked without dk.  A bag's attn and
 *                      lse are those of snf_sparse_attn_fwd_x3_dk192 on that bag alone, bit for bit, out within the fp32 order of the
 *                      partial sums, and nothing depends on what a bag is packed with. */
size_t snf_sparse_attn_fwd_x3_dk192_workspace_bytes(int64_t n, int k, int h);
int snf_sparse_attn_fwd_x3_dk192(const float* q, int64_t ldq, const float* v, int64_t ldv, const float* kp, int64_t n, int k, int h,
                                 float scale, float* out, float* attn, float* lse, void* workspace, size_t workspace_bytes,
                                 snf_stream_t stream);
int snf_sparse_attn_x3_varlen_dk192_plan(const int64_t* offsets, int bags, int k, int h, int32_t* table, size_t table_ints,
                                         size_t* table_ints_needed, size_t* workspace_bytes, int* n_chunks, int* chunk_k);
int snf_sparse_attn_fwd_x3_varlen_dk192(const float* q, int64_t ldq, const float* v, int64_t ldv, const float* kp,
                                        const int64_t* offsets, int bags, int k, int h, float scale, float* out, float* attn,
                                        float* lse, const int32_t* table_dev, void* workspace, size_t workspace_bytes,
                                        snf_stream_t stream);
/* The same at HEAD WIDTH 256 (D = 512, h = 2: the SimCLR ResNet-18 recipe, Lambda = 900): the protocol, arguments, layouts, alignment
 * rules and error codes of the four _x3_dk192 entry points above, with kp / out rows of h * 256 floats.  The plan functions of
 * dk = 64 / 128 and of 192 keep answering SNF_EUNSUPPORTED at dk = 256.  One launch holds 128 keys (1, 2 or 4 key blocks); a workgroup
 * is four waves (the Kp fragments of a key block are 128 registers per lane) over 32-row tiles: Q 32 + P 20 + V 2 x 32 + statistics
 * 1 KiB of LDS at 4 blocks.  More keys run as up to 8 chunks of ceil(k / chunks) keys rounded up to a multiple of 4 (the last chunk
 * shorter; chunked launches run at 2 or 4 key blocks), so 1 <= k <= 8 x 128, the key range of snf_sparse_attn_fwd_x3u_f32.
 * Inference only. */
size_t snf_sparse_attn_fwd_x3_dk256_workspace_bytes(int64_t n, int k, int h);
int snf_sparse_attn_fwd_x3_dk256(const float* q, int64_t ldq, const float* v, int64_t ldv, const float* kp, int64_t n, int k, int h,
                                 float scale, float* out, float* attn, float* lse, void* workspace, size_t workspace_bytes,
                                 snf_stream_t stream);
int snf_sparse_attn_x3_varlen_dk256_plan(const int64_t* offsets, int bags, int k, int h, int32_t* table, size_t table_ints,
                                         size_t* table_ints_needed, size_t* workspace_bytes, int* n_chunks, int* chunk_k);
int snf_sparse_attn_fwd_x3_varlen_dk256(const float* q, int64_t ldq, const float* v, int64_t ldv, const float* kp,
                                        const int64_t* offsets, int bags, int k, int h, float scale, float* out, float* attn,
                                        float* lse, const int32_t* table_dev, void* workspace, size_t workspace_bytes,
                                        snf_stream_t stream);
/* The bf16 family at HEAD WIDTH 256 (the same recipe in precision="bf16"; the training form is ..._dk256_dropout below): q and v are bf16 ONLY (row pitches ldq / ldv
 * in elements, so the two halves of one [N, 2D] projection are passed in place), kp is f32 or bf16 (kp_dtype; an f32 Kp is rounded to
 * bf16 once, round to nearest even, into the workspace: both give the same bits), out / attn / lse are f32.  snf_sparse_attn_fwd_mfma and
 * the varlen plan functions of dk = 64 / 128 and of 192 keep answering SNF_EUNSUPPORTED at dk = 256.  One launch holds 128 keys (1, 2 or
 * 4 key blocks); a workgroup is four waves (the Kp fragments of a key block stay in 64 registers per lane for a whole head) over 32-row
 * tiles: Q 16 + P 10 + V 2 x 16 + statistics 1 KiB of LDS at 4 blocks.  More keys run as up to 8 near-equal chunks of
 * ceil(k / chunks) keys (the family's rule; chunked launches run at 2 or 4 key blocks): a statistics pass per chunk into
 * [chunks][h][n][2], then the main passes, which combine the chunks' statistics exactly.  So 1 <= k <= 8 x 128.
 *   ..._mfma_dk256_workspace_bytes  partial tiles | statistics | bf16 copy of an f32 Kp; 0 = unsupported (k outside 1 .. 1024, n < 1 or
 *                      above 0xffff00, h < 1).
 *   snf_sparse_attn_fwd_mfma_dk256  alignment rules and error codes of snf_sparse_attn_fwd_mfma (16-byte aligned q / v / kp and row
 *                      pitches of a multiple of 8 elements: SNF_EINVAL; pitches of 2^24 elements or n * pitch of 2^31 - 1 elements and
 *                      more: SNF_EUNSUPPORTED; a short workspace: SNF_EWORKSPACE).  A repeated call is bit-identical (no atomics).
 *   snf_sparse_attn_varlen_dk256_plan / snf_sparse_attn_fwd_mfma_varlen_dk256  signatures and protocol of the two _dk192 entry points
 *                      above.  SNF_EUNSUPPORTED: k outside 1 .. 1024, h < 1, an empty bag.  A bag's attn and lse are those of
 *                      snf_sparse_attn_fwd_mfma_dk256 on that bag alone, bit for bit, out within the fp32 order of the partial sums, and
 *                      nothing depends on what a bag is packed with. */
size_t snf_sparse_attn_fwd_mfma_dk256_workspace_bytes(int64_t n, int k, int h);
int snf_sparse_attn_fwd_mfma_dk256(const void* q, int64_t ldq, const void* v, int64_t ldv, const void* kp, int kp_dtype, int64_t n, int k,
                                   int h, float scale, float* out, float* attn, float* lse, void* workspace, size_t workspace_bytes,
                                   snf_stream_t stream);
/* Training form: snf_sparse_attn_fwd_mfma_dk256 with attention dropout applied inside the kernel (Philox, the mask of
 * snf_dropout_mask_f32; never read from memory).  lse and the normalised P are, bit for bit, those of the launch without dropout; attn
 * (when asked for) is P o M with M the keep-mask / (1 - p), out = (P o M)^T V with P o M rounded to bf16.  Single bag only; the workspace
 * is snf_sparse_attn_fwd_mfma_dk256_workspace_bytes'.  Above one key chunk every pass keeps the chunks of that launch (this kernel's P
 * depends on which keys share a 32-key block); a chunk that starts off a multiple of 4 draws two Philox groups per 4 keys.  SNF_EINVAL: dropout_p outside [0, 1),
 * dropout_p > 0 with neither lse nor attn.  dropout_p == 0 is snf_sparse_attn_fwd_mfma_dk256 itself. */
int snf_sparse_attn_fwd_mfma_dk256_dropout(const void* q, int64_t ldq, const void* v, int64_t ldv, const void* kp, int kp_dtype, int64_t n,
                                           int k, int h, float scale, float* out, float* attn, float* lse, void* workspace,
                                           size_t workspace_bytes, snf_stream_t stream, float dropout_p, uint64_t seed, uint64_t offset);
int snf_sparse_attn_varlen_dk256_plan(const int64_t* offsets, int bags, int k, int h, int32_t* table, size_t table_ints,
                                      size_t* table_ints_needed, size_t* workspace_bytes, int* n_chunks, int* chunk_k);
int snf_sparse_attn_fwd_mfma_varlen_dk256(const void* q, int64_t ldq, const void* v, int64_t ldv, const void* kp, int kp_dtype,
                                          const int64_t* offsets, int bags, int k, int h, float scale, float* out, float* attn,
                                          float* lse, const int32_t* table_dev, void* workspace, size_t workspace_bytes,
                                          snf_stream_t stream);
/* Ragged form for SMALL bags (exact fp32, any head width, every bag with its own key count: a bag shorter than Lambda selects
 * all of its rows -- snuffy.py:129 `min(ceil(...), n)` -- as the MIL benchmark sets do).  desc_dev [bags][4] int32 in DEVICE
 * memory = (first packed row, rows, first key row, keys) per bag; kp / out [sum of keys, h * dk]; attn [h, T, kmax] nullable
 * (bag b's A = attn[:, row0 : row0 + n, :k]).  kmax <= 256 and (16 + dk) * kmax floats of LDS <= 160 KiB. */
int snf_sparse_attn_fwd_ragged_f32(const float* q, int64_t ldq, const float* v, int64_t ldv, const float* kp, const int32_t* desc_dev,
                                   int bags, int64_t n_total, int kmax, int h, int dk, float scale, float* out, float* attn,
                                   float* lse, snf_stream_t stream);
int snf_ln_mean_head_varlen_plan(const int64_t* offsets, int bags, int d, int32_t* table, size_t table_ints,
                                 size_t* table_ints_needed, size_t* workspace_bytes);
int snf_ln_mean_head_varlen_f32(const float* z, const int64_t* offsets, int bags, int d, const void* add_bf16,
                                const float* add_bias, const int32_t* slot_map, const float* delta_rows, float* z_out,
                                const float* gamma, const float* beta, float eps, const float* w_head, const float* b_head,
                                int c_out, float* logits, float* pooled, const int32_t* table_dev, void* workspace,
                                size_t workspace_bytes, snf_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * K3  device-side random patch share (opt-in fast mode)       replaces snuffy.py:136-147 (np.random.choice on the host behind a
 *     device -> host copy of the selected rows) when the caller asks for it; the reference's own MT19937 draws stay the default.
 *   snf_random_share_keys_f32: keys[r] = the non-negative float whose bit pattern is a 30-bit Philox4x32-10 output for row r (key =
 *     state[0] = seed, counter = (r / 4, state[1] + (layer << 48)), element r & 3), keys[exclude_rows[i]] = -1.  The k2 largest keys
 *     (snf_topk_f32) are a uniform sample without replacement of the rows not excluded, in random order.
 *   state: 16-byte device record {u64 seed, u64 offset}, owned by the caller; snf_sampler_advance adds 1 to the offset ON THE DEVICE,
 *     so a captured graph (advance, keys, top-k) draws fresh rows on every replay.  Host twin: oracle/philox_ref.py.
 *   snf_random_share_keys_batched_f32: the same for b batch rows in two launches (keys, then excludes): keys [b, n], row i draws
 *     from stream layer + 64 i (row 0 is the single-row stream; layer < 64, b <= 64), keys[i, exclude[i, j]] = -1 for
 *     j < counts_dev[i] (exclude [b, pitch] int64, counts_dev [b] int32, both in DEVICE memory: the counts are never read on the host).
 *     The k2 largest keys of every row: snf_topk_segmented_f32 over the b rows of n keys.
 *   snf_random_share_draw_segmented_f32: the draws of every bag and every layer of a PACKED batch (varlen path).  offsets_dev [bags + 1]
 *     and top [bags, k1] as snf_topk_segmented_f32 takes / writes them (a bag with n_b < k1 rows: its first n_b entries are read);
 *     rnd_out [layers, bags, k2] int64, indices inside each bag: bag b's first k2_b = min(k2, max(0, n_b - k1)) entries are its draw
 *     (descending key, ties by ascending row), the rest of the row is padding.  Bag b draws from offset state[1] + 1 + b, layer l from
 *     stream l << 48 -- what the b-th of `bags` single-bag forwards (advance, keys, top-k) draws -- and the record is advanced by `bags`
 *     on the device behind the draws.  max_n (the longest bag) <= 32768: ONE launch, one workgroup per (bag, layer), the keys are made in
 *     registers and never reach memory.  Up to 65536: per layer a key image of the packed rows in `workspace` (total_rows floats,
 *     snf_random_share_draw_workspace_bytes) and snf_topk_segmented_f32 on it.  layers > 4096, k2 > 2048, longer bags or a missing
 *     workspace: SNF_EUNSUPPORTED.
 * --------------------------------------------------------------------------------------------------------- */
int snf_sampler_advance(void* state, snf_stream_t stream);
size_t snf_random_share_draw_workspace_bytes(int64_t max_n, int64_t total_rows);
int snf_random_share_draw_segmented_f32(void* state, int layers, const int64_t* offsets_dev, int bags, int64_t max_n, int64_t total_rows,
                                        const int64_t* top, int k1, int k2, int64_t* rnd_out, void* workspace, size_t workspace_bytes,
                                        snf_stream_t stream);
int snf_random_share_keys_f32(const void* state, int layer, int64_t n, const int64_t* exclude_rows, int n_exclude, float* keys,
                              snf_stream_t stream);
int snf_random_share_keys_batched_f32(const void* state, int layer, int b, int64_t n, const int64_t* exclude, const int32_t* counts_dev,
                                      int pitch, float* keys, snf_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * ResNet-18 patch extractor (csrc/resnet.hip): the reference's SimCLR recipe, torchvision resnet18 with InstanceNorm2d (or eval-mode
 * BatchNorm2d) and fc = Identity; inference only.  Activations are NHWC ([b, h, w, c] row-major), conv outputs fp32.
 *   snf_conv2d_nhwc_plan      pure host (needs no GPU): output dims, m = b ho wo output pixels, the 128-row x 64-column tile counts and the
 *                             workspace bytes (0: the statistics are a pass of their own) of a kh x kh / stride convolution with padding
 *                             kh / 2.  Kernels exist for 3x3 / 1, 3x3 / 2 and 1x1 / 2 over cin, cout in {64, 128, 256, 512} and for the
 *                             7x7 / 2 stem from 3 to 64 channels; anything else SNF_EUNSUPPORTED.  Output pointers are nullable.
 *   snf_conv_pack_weight_f32  w [cout, cin, kh, kw] f32 -> image [cout, kp] bf16 in the kernels' K order (tap-major, channel-minor; kp >=
 *                             kh kw cin, a multiple of 64, zero beyond the taps); lo (nullable) = bf16(w - hi), the second half of the
 *                             fp32-class operand.  kp = kh kw cin for the body convolutions, 192 for the stem.
 *   snf_conv2d_nhwc           implicit-GEMM convolution on the matrix cores, no bias, no im2col matrix in memory.  x f32 or bf16
 *                             (x_dtype = SNF_DT_*); w_lo = NULL: one bf16 product (f32 x is rounded to bf16 on the way in); w_lo given:
 *                             hi hi + hi lo + lo hi of the split fp32 operands (x must be f32).  out [m, cout] f32.
 *   snf_conv_stem             the 7x7 / 2 pad-3 stem, 3 -> 64: x is f32 [b, 3, h, w] (src_u8_nhwc = 0) or uint8 [b, h, w, 3]
 *                             (src_u8_nhwc = 1, value / 255.0f as to_tensor divides: both entries give the same bits).
 *   snf_instnorm_stats_nhwc   mean [b, c] and rstd [b, c] = 1 / sqrt(var + eps) (biased variance) per (image, channel) of x [b, hw, c] f32,
 *                             two passes, fixed summation order (no atomics).  c % 64 == 0.
 *   snf_norm_act_nhwc         out = (x - mean) rstd gamma + beta (+ identity) (ReLU if relu): mean / rstd [b, c] (per_image = 1) or [c]
 *                             (per_image = 0: eval-mode BatchNorm constants); gamma, beta [c] and identity [b, hw, c] f32 nullable; out
 *                             f32 or bf16 (out_dtype = SNF_DT_*).
 *   snf_maxpool3x3s2_nhwc     3x3 / 2 pad-1 max-pool (padding is -inf), x [b, h, w, c] f32 -> [b, (h - 1) / 2 + 1, (w - 1) / 2 + 1, c].
 *   snf_avgpool_nhwc          x [b, hw, c] f32 -> mean over hw [b, c], fixed summation order.  c % 64 == 0.
 * Every pointer 16-byte aligned; b <= 65535 per call for the per-image kernels.
 * --------------------------------------------------------------------------------------------------------- */
int snf_conv2d_nhwc_plan(int b, int h, int w, int cin, int cout, int kh, int stride, int* ho, int* wo, int64_t* m, int* tiles_m,
                         int* tiles_n, size_t* workspace_bytes);
int snf_conv_pack_weight_f32(const float* w, int cout, int cin, int kh, int kw, int kp, void* hi_bf16, void* lo_bf16, snf_stream_t stream);
int snf_conv2d_nhwc(const void* x, int x_dtype, const void* w_hi, const void* w_lo, int b, int h, int w, int cin, int cout, int kh,
                    int stride, float* out, snf_stream_t stream);
int snf_conv_stem(const void* x, int src_u8_nhwc, const void* w_hi, const void* w_lo, int b, int h, int w, float* out,
                  snf_stream_t stream);
int snf_instnorm_stats_nhwc(const float* x, int b, int64_t hw, int c, float eps, float* mean, float* rstd, snf_stream_t stream);
int snf_norm_act_nhwc(const float* x, int b, int64_t hw, int c, const float* mean, const float* rstd, int per_image, const float* gamma,
                      const float* beta, const float* identity, int relu, void* out, int out_dtype, snf_stream_t stream);
int snf_maxpool3x3s2_nhwc(const float* x, int b, int h, int w, int c, float* out, snf_stream_t stream);
int snf_avgpool_nhwc(const float* x, int b, int64_t hw, int c, float* out, snf_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * Debug hooks -- PROCESS-WIDE state, outside the stateless / re-entrant contract at the top of this header (see there).  Callers:
 * tests/ (cross-checks of kernel variants against each other) and tools/ (A / B timing, traces); nothing in snuffy_amd/ calls them.
 * snf_debug_attn_trace(buf): device buffer of u64 that dev builds of the attention kernels (X3P_TRACE / SNF_ATTN_TRACE defines)
 * fill with s_memtime stamps of workgroup snf_debug_attn_trace_wg(wg); null switches the stamps off.  Shipped builds carry no
 * stamp code: the calls only set two host-side variables. */
void snf_debug_attn_trace(void* buf);
void snf_debug_attn_trace_wg(int wg);
/* snf_debug_x3p_kbw(kbw): key blocks per wave of the dk = 128 family of snf_sparse_attn_fwd_x3_hl for 129 .. 256 keys per launch --
 * 1 (default: one wave per key block, two per SIMD) or 2 (one wave per SIMD carrying two key blocks, round 5); same arithmetic,
 * results equal up to the fp32 order of the row sums.  For A / B timing (tools/x3p_dev.py) and the parity tests of the second form. */
void snf_debug_x3p_kbw(int kbw);
/* snf_debug_exact_attn_mfma(on): the exact-fp32 attention kernels (snf_sparse_attn_fwd_f32, the dKp contraction of the backward) on
 * v_mfma_f32_32x32x2_f32 (1, default; head widths % 8 == 0, <= 1024 keys for the scores) or on the vector ALUs for every shape (0);
 * 2 = the matrix-core forms with the dQ / dV kernel of the backward reading its operands straight from L2 instead of staging them through
 * LDS (the round-5 A / B partner; same fmaf chains, bit-identical results). */
void snf_debug_exact_attn_mfma(int on);

#ifdef __cplusplus
}
#endif
#endif /* SNUFFY_HIP_H */
