// K7 (fp32-class form) at head width 192 (the MAE recipe, D = 768, h = 4): the one-launch forms at 1, 2, 4 key blocks, single bag and
// varlen, and the four C entry points of the width (the kernel and the width's description X3W are in sparse_attn_x3_dk192_impl.h; the
// key-chunked forms build in sparse_attn_x3_dk192_chunks.hip).  The plan functions of dk = 64 / 128 keep refusing this width.  The
// bodies of the entry points are in attn_width.h, the driver behind them is attn_drive.h.
#include "sparse_attn_x3_dk192_impl.h"

using E = snf_attn::Width<X3W>;

extern "C" {

size_t snf_sparse_attn_fwd_x3_dk192_workspace_bytes(int64_t n, int k, int h) { return snf_attn::entry_workspace_bytes<E>(n, k, h); }

// q, v [n, ld] f32, kp [k, h * 192] f32, out [k, h * 192], attn [h, n, k] / lse [h, n] or null
int snf_sparse_attn_fwd_x3_dk192(const float* q, int64_t ldq, const float* v, int64_t ldv, const float* kp, int64_t n, int k, int h,
                                 float scale, float* out, float* attn, float* lse, void* workspace, size_t workspace_bytes,
                                 snf_stream_t stream) {
    return snf_attn::entry_forward_bag<E>("snf_sparse_attn_fwd_x3_dk192", q, ldq, v, ldv, kp, SNF_DT_F32, n, k, h, scale, out, attn, lse,
                                          workspace, workspace_bytes, stream);
}

int snf_sparse_attn_x3_varlen_dk192_plan(const int64_t* offsets, int bags, int k, int h, int32_t* table, size_t table_ints,
                                         size_t* table_ints_needed, size_t* workspace_bytes, int* n_chunks, int* chunk_k) {
    return snf_attn::entry_varlen_plan<E>("snf_sparse_attn_x3_varlen_dk192_plan", offsets, bags, k, h, table, table_ints, table_ints_needed,
                                          workspace_bytes, n_chunks, chunk_k);
}

// q, v [T, ld] f32 packed rows, kp [bags * k, h * 192] f32, out [bags * k, h * 192], attn [h, T, k] / lse [h, T] or null;
// table_dev / workspace from snf_sparse_attn_x3_varlen_dk192_plan
int snf_sparse_attn_fwd_x3_varlen_dk192(const float* q, int64_t ldq, const float* v, int64_t ldv, const float* kp,
                                        const int64_t* offsets, int bags, int k, int h, float scale, float* out, float* attn,
                                        float* lse, const int32_t* table_dev, void* workspace, size_t workspace_bytes,
                                        snf_stream_t stream) {
    return snf_attn::entry_forward_varlen<E>("snf_sparse_attn_fwd_x3_varlen_dk192", q, ldq, v, ldv, kp, SNF_DT_F32, offsets, bags, k, h, scale,
                                             out, attn, lse, table_dev, workspace, workspace_bytes, stream);
}

}  // extern "C"
