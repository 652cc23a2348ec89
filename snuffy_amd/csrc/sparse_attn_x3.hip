// K7 (fp32-class form on the matrix cores): the single-bag and single-chunk varlen variants and the C entry points of dk = 64 / 128 (the
// kernels are in sparse_attn_x3_impl.h; the key-chunked varlen variants build in sparse_attn_x3_varlen_chunks.hip).  The driver behind
// the entry points is attn_drive.h; this file describes the family to it.
#include "sparse_attn_x3_impl.h"

namespace {
using namespace snf_attn;   // the driver (attn_drive.h)

struct X3 : X3Drive {
    static constexpr bool BAG_NKB_OF_LARGEST = true;   // single bag: every chunk launches at the plan's (largest chunk's) key-block count
    static constexpr const char* DK_TEXT = "dk";
    int dk, h;
    bool chunks(int k, X3Chunks* c) const { return x3_chunks(k, dk, c); }
    bool plan(int64_t n, int kc, X3Plan* pl, bool packed) const { return x3_plan(n, kc, h, dk, pl, packed); }
    bool built(bool chunked, int nkb) const { return !chunked || x3_varlen_chunk_built(dk, nkb); }   // one chunk: every count is built
};

int x3_forward(const float* q, int64_t ldq, const float* v, int64_t ldv, const float* kp, int64_t n, int k, int h, int dk, float scale,
               float* out, float* attn, float* lse, void* workspace, size_t workspace_bytes, snf_stream_t stream,
               const snf::DropoutState* drop) {
    const char* me = "snf_sparse_attn_fwd_x3";
    if (int rc = require(me, q && v && kp && out, "null pointer")) return rc;
    if (int rc = require(me, n >= 1 && k >= 1 && h >= 1, "bad shape")) return rc;
    const X3 f{{}, dk, h};
    BagLaunch b;
    if (!plan_bag(f, n, k, h, &b)) {
        snf::set_error("snf_sparse_attn_fwd_x3: unsupported shape k=%d dk=%d (dk in {64, 128}, k <= 8 x 256 / 8 x 224)", k, dk);
        return SNF_EUNSUPPORTED;
    }
    X3Params P;
    hipStream_t s = snf::as_stream(stream);
    const Operands<float, float> o{q, v, ldq, ldv, 4, kp, false, k, h, scale, out, attn, lse, workspace, workspace_bytes, s};
    return forward_bag(me, f, b, o, n, b.chunks.size, P, [&](bool stats_pass, X3Params& P, const X3Plan& pl, float* out_c) {
        if (drop) {
            if (P.nchunks != 1) {
                snf::set_error("snf_sparse_attn_fwd_x3_dropout: k=%d needs key chunks; the in-kernel mask covers one launch (k <= %d)", k,
                               dk == 128 ? 224 : 256);
                return (int)SNF_EUNSUPPORTED;
            }
            P.drop = *drop;
            return dk == 128 ? x3_dispatch_dropout<128>(P, pl, out_c, s) : x3_dispatch_dropout<64>(P, pl, out_c, s);
        }
        const int mode = stats_pass ? 1 : P.nchunks > 1 ? 2 : 0;   // key chunks: statistics, then main passes exact over all keys
        return dk == 128 ? x3_dispatch<128>(P, pl, out_c, s, mode) : x3_dispatch<64>(P, pl, out_c, s, mode);
    });
}

// the launch of the two varlen entry points: one chunk runs the MODE 0 varlen kernels, more run MODE 1 and MODE 2
int x3_varlen_launch(const char* me, const X3& f, const VarlenLaunch& vl, const Operands<float, float>& o, const int64_t* offsets, int bags,
                     const int32_t* table_dev) {
    X3Params P;
    return forward_varlen(me, f, vl, o, offsets, bags, table_dev, P, [&](bool stats_pass, X3Params& P, const X3Plan& pl, float* out_c) {
        if (vl.chunks.count > 1) return snf::x3_launch_varlen_chunk(f.dk, stats_pass ? 1 : 2, P, pl, out_c, o.stream);
        return f.dk == 128 ? x3_dispatch_varlen<128>(P, pl, out_c, o.stream) : x3_dispatch_varlen<64>(P, pl, out_c, o.stream);
    });
}
}  // namespace

extern "C" {

size_t snf_sparse_attn_fwd_x3_workspace_bytes(int64_t n, int k, int h, int dk) {
    BagLaunch b;
    return (h >= 1 && plan_bag(X3{{}, dk, h}, n, k, h, &b)) ? b.partial_bytes + b.stats_bytes : 0;
}

int snf_sparse_attn_fwd_x3(const float* q, int64_t ldq, const float* v, int64_t ldv, const float* kp, int64_t n, int k, int h,
                           int dk, float scale, float* out, float* attn, float* lse, void* workspace, size_t workspace_bytes,
                           snf_stream_t stream) {
    return x3_forward(q, ldq, v, ldv, kp, n, k, h, dk, scale, out, attn, lse, workspace, workspace_bytes, stream, nullptr);
}

int snf_sparse_attn_fwd_x3_dropout(const float* q, int64_t ldq, const float* v, int64_t ldv, const float* kp, int64_t n, int k, int h,
                                   int dk, float scale, float dropout_p, uint64_t seed, uint64_t offset, float* out, float* attn,
                                   float* lse, void* workspace, size_t workspace_bytes, snf_stream_t stream) {
    SNF_REQUIRE(dropout_p >= 0.f && dropout_p < 1.f, "snf_sparse_attn_fwd_x3_dropout: dropout_p=%g outside [0, 1)", (double)dropout_p);
    const snf::DropoutState st = snf::make_dropout(dropout_p, seed, offset);
    return x3_forward(q, ldq, v, ldv, kp, n, k, h, dk, scale, out, attn, lse, workspace, workspace_bytes, stream, st.thresh ? &st : nullptr);
}

// ---- varlen (see snf_sparse_attn_varlen_plan in sparse_attn_mfma.hip for the protocol; this is the fp32-class kernel's plan) ----
int snf_sparse_attn_x3_varlen_plan(const int64_t* offsets, int bags, int k, int h, int dk, int32_t* table, size_t table_ints,
                                   size_t* table_ints_needed, size_t* workspace_bytes) {
    const char* me = "snf_sparse_attn_x3_varlen_plan";
    if (int rc = require(me, offsets && bags >= 1 && k >= 1 && h >= 1, "bad arguments")) return rc;
    return varlen_plan_reply(me, X3{{}, dk, h}, offsets, bags, k, h, 1, table, table_ints, table_ints_needed, workspace_bytes, nullptr, nullptr,
                             [&] {
        snf::set_error("snf_sparse_attn_x3_varlen_plan: unsupported shape (bags=%d k=%d dk=%d: dk in {64, 128}, k <= %d, non-empty "
                       "bags)", bags, k, dk, dk == 128 ? 224 : 256);
    });
}

// q, v [T, ld] f32 packed rows, kp [bags * k, h * dk] f32, out [bags * k, h * dk], attn [h, T, k] / lse [h, T] or null
int snf_sparse_attn_fwd_x3_varlen(const float* q, int64_t ldq, const float* v, int64_t ldv, const float* kp, const int64_t* offsets,
                                  int bags, int k, int h, int dk, float scale, float* out, float* attn, float* lse,
                                  const int32_t* table_dev, void* workspace, size_t workspace_bytes, snf_stream_t stream) {
    const char* me = "snf_sparse_attn_fwd_x3_varlen";
    if (int rc = require(me, q && v && kp && out && offsets && table_dev, "null pointer")) return rc;
    const X3 f{{}, dk, h};
    VarlenLaunch vl;
    if (!plan_varlen(f, offsets, bags, k, h, 1, &vl, nullptr, 0)) {
        snf::set_error("snf_sparse_attn_fwd_x3_varlen: unsupported shape (bags=%d k=%d dk=%d)", bags, k, dk);
        return SNF_EUNSUPPORTED;
    }
    return x3_varlen_launch(me, f, vl, {q, v, ldq, ldv, 4, kp, false, k, h, scale, out, attn, lse, workspace, workspace_bytes,
                                        snf::as_stream(stream)}, offsets, bags, table_dev);
}

// ---- varlen above one key chunk: the chunks of x3_chunks (the single-bag driver's rule, so a packed bag's P and lse are those of its own
// launch bit for bit), a statistics launch (MODE 1) per chunk over all bags, then the chunks' main launches (MODE 2).
int snf_sparse_attn_x3_varlen_chunked_plan(const int64_t* offsets, int bags, int k, int h, int dk, int32_t* table, size_t table_ints,
                                           size_t* table_ints_needed, size_t* workspace_bytes, int* n_chunks, int* chunk_k) {
    const char* me = "snf_sparse_attn_x3_varlen_chunked_plan";
    if (int rc = require(me, offsets && bags >= 1 && k >= 1 && h >= 1, "bad arguments")) return rc;
    return varlen_plan_reply(me, X3{{}, dk, h}, offsets, bags, k, h, 8, table, table_ints, table_ints_needed, workspace_bytes, n_chunks, chunk_k,
                             [&] {
        snf::set_error("snf_sparse_attn_x3_varlen_chunked_plan: unsupported shape (bags=%d k=%d dk=%d: dk in {64, 128}, k <= 8 x %d, "
                       "non-empty bags)", bags, k, dk, dk == 64 ? 256 : 224);
    });
}

// layouts as snf_sparse_attn_fwd_x3_varlen; table_dev / workspace from snf_sparse_attn_x3_varlen_chunked_plan
int snf_sparse_attn_fwd_x3_varlen_chunked(const float* q, int64_t ldq, const float* v, int64_t ldv, const float* kp,
                                          const int64_t* offsets, int bags, int k, int h, int dk, float scale, float* out, float* attn,
                                          float* lse, const int32_t* table_dev, void* workspace, size_t workspace_bytes,
                                          snf_stream_t stream) {
    const char* me = "snf_sparse_attn_fwd_x3_varlen_chunked";
    if (int rc = require(me, q && v && kp && out && offsets && table_dev, "null pointer")) return rc;
    if (int rc = require(me, k >= 1 && h >= 1, "bad shape")) return rc;
    const X3 f{{}, dk, h};
    VarlenLaunch vl;
    if (!plan_varlen(f, offsets, bags, k, h, 8, &vl, nullptr, 0)) {
        snf::set_error("snf_sparse_attn_fwd_x3_varlen_chunked: unsupported shape (bags=%d k=%d dk=%d)", bags, k, dk);
        return SNF_EUNSUPPORTED;
    }
    if (vl.chunks.count == 1)   // one chunk: the launch, the table (integer for integer) and the refusals of the single-chunk entry point
        return snf_sparse_attn_fwd_x3_varlen(q, ldq, v, ldv, kp, offsets, bags, k, h, dk, scale, out, attn, lse, table_dev, workspace,
                                             workspace_bytes, stream);
    return x3_varlen_launch(me, f, vl, {q, v, ldq, ldv, 4, kp, false, k, h, scale, out, attn, lse, workspace, workspace_bytes,
                                        snf::as_stream(stream)}, offsets, bags, table_dev);
}

}  // extern "C"
