// K7 (fast form, bf16) at head width 256 (the SimCLR ResNet-18 recipe, D = 512, h = 2): the one-launch forms at 1, 2, 4 key blocks,
// single bag and varlen, and the four C entry points of the width (the kernel and the width's description A256 are in
// sparse_attn_mfma_dk256_impl.h; the key-chunked forms build in sparse_attn_mfma_dk256_chunks.hip).  snf_sparse_attn_fwd_mfma and the
// varlen plan functions of dk = 64 / 128 and of 192 keep refusing this width.  The bodies of the entry points are in attn_width.h, the
// driver behind them is attn_drive.h.
#include "sparse_attn_mfma_dk256_impl.h"

using E = snf_attn::Width<A256>;

extern "C" {

// partial tiles | chunk statistics | bf16 copy of an f32 Kp
size_t snf_sparse_attn_fwd_mfma_dk256_workspace_bytes(int64_t n, int k, int h) { return snf_attn::entry_workspace_bytes<E>(n, k, h); }

// q, v [n, ld] bf16, kp [k, h * 256] f32 | bf16, out [k, h * 256] f32, attn [h, n, k] / lse [h, n] or null
int snf_sparse_attn_fwd_mfma_dk256(const void* q, int64_t ldq, const void* v, int64_t ldv, const void* kp, int kp_dtype, int64_t n, int k,
                                   int h, float scale, float* out, float* attn, float* lse, void* workspace, size_t workspace_bytes,
                                   snf_stream_t stream) {
    return snf_attn::entry_forward_bag<E>("snf_sparse_attn_fwd_mfma_dk256", q, ldq, v, ldv, kp, kp_dtype, n, k, h, scale, out, attn, lse,
                                          workspace, workspace_bytes, stream);
}

int snf_sparse_attn_varlen_dk256_plan(const int64_t* offsets, int bags, int k, int h, int32_t* table, size_t table_ints,
                                      size_t* table_ints_needed, size_t* workspace_bytes, int* n_chunks, int* chunk_k) {
    return snf_attn::entry_varlen_plan<E>("snf_sparse_attn_varlen_dk256_plan", offsets, bags, k, h, table, table_ints, table_ints_needed,
                                          workspace_bytes, n_chunks, chunk_k);
}

// q, v [T, ld] bf16 packed rows, kp [bags * k, h * 256] f32 | bf16, out [bags * k, h * 256] f32, attn [h, T, k] / lse [h, T] or null;
// table_dev / workspace from snf_sparse_attn_varlen_dk256_plan
int snf_sparse_attn_fwd_mfma_varlen_dk256(const void* q, int64_t ldq, const void* v, int64_t ldv, const void* kp, int kp_dtype,
                                          const int64_t* offsets, int bags, int k, int h, float scale, float* out, float* attn,
                                          float* lse, const int32_t* table_dev, void* workspace, size_t workspace_bytes,
                                          snf_stream_t stream) {
    return snf_attn::entry_forward_varlen<E>("snf_sparse_attn_fwd_mfma_varlen_dk256", q, ldq, v, ldv, kp, kp_dtype, offsets, bags, k, h, scale,
                                             out, attn, lse, table_dev, workspace, workspace_bytes, stream);
}

}  // extern "C"
