// K7 (fp32-class form) at head width 256 (the SimCLR ResNet-18 recipe, D = 512, h = 2): the one-launch forms at 1, 2, 4 key blocks,
// single bag and varlen, and the four C entry points of the width (the kernel is in sparse_attn_x3_dk256_impl.h; the key-chunked forms
// build in sparse_attn_x3_dk256_chunks.hip).  The plan functions of dk = 64 / 128 and of 192 keep refusing this width.  The driver behind
// the entry points is attn_drive.h; this file describes the width to it.
#include "sparse_attn_x3_dk256_impl.h"

namespace {

using namespace snf_attn;   // the driver (attn_drive.h)
constexpr int DK = X3Y_DK;

template <bool VL>
int x3y_dispatch(const X3Params& P, const X3Plan& pl, float* out, hipStream_t s) {
    const bool aux = P.attn != nullptr || P.lse != nullptr;
    switch (pl.nkb) {
        case 1: return aux ? x3y_launch<1, true, 0, VL>(P, pl, out, s) : x3y_launch<1, false, 0, VL>(P, pl, out, s);
        case 2: return aux ? x3y_launch<2, true, 0, VL>(P, pl, out, s) : x3y_launch<2, false, 0, VL>(P, pl, out, s);
        case 4: return aux ? x3y_launch<4, true, 0, VL>(P, pl, out, s) : x3y_launch<4, false, 0, VL>(P, pl, out, s);
        default: break;
    }
    snf::set_error("sparse_attn_x3_dk256: key-block count %d not built", pl.nkb);
    return SNF_EUNSUPPORTED;
}

// key-block count of a chunk of kc keys (0: none)
int x3y_chunk_nkb(int kc) {
    X3Plan one;
    return x3y_plan(1, kc, 1, &one, true) ? one.nkb : 0;
}
// the chunks of k keys, every one at a key-block count that is built (the plan is the one refusal point)
bool x3y_chunks_built(int k, X3Chunks* ch) {
    if (!x3y_chunks(k, ch)) return false;
    if (ch->count > 1)
        for (int c = 0; c < ch->count; ++c) {
            const int kc = k - c * ch->size < ch->size ? k - c * ch->size : ch->size;
            if (kc < 1 || !x3y_chunk_built(x3y_chunk_nkb(kc))) return false;
        }
    return true;
}

// The fp32-class family at dk = 256: the chunks of x3y_chunks for single bag and varlen alike (a packed bag's P and lse are those of its
// own launch bit for bit), every chunk launched at its own key-block count
struct X3Y : X3Drive {
    static constexpr bool BAG_NKB_OF_LARGEST = false;
    static constexpr const char* DK_TEXT = "256";
    static constexpr int dk = DK;
    int h;
    bool chunks(int k, X3Chunks* c) const { return x3y_chunks_built(k, c); }
    bool plan(int64_t n, int kc, X3Plan* pl, bool packed) const { return x3y_plan(n, kc, h, pl, packed); }
    bool built(bool, int) const { return true; }   // chunks() has looked: the single-bag plan refuses unbuilt chunks too
};

// one chunk: the MODE 0 kernels; more: MODE 1 per chunk, then MODE 2
template <bool VL>
int x3y_launch_pass(bool stats_pass, const X3Params& P, const X3Plan& pl, float* out, hipStream_t s) {
    if (P.nchunks == 1) return x3y_dispatch<VL>(P, pl, out, s);
    return snf::x3_dk256_launch_chunk(stats_pass ? 1 : 2, P, pl, out, s);
}

}  // namespace

extern "C" {

size_t snf_sparse_attn_fwd_x3_dk256_workspace_bytes(int64_t n, int k, int h) {
    BagLaunch b;
    return (h >= 1 && n >= 1 && plan_bag(X3Y{{}, h}, n, k, h, &b)) ? b.partial_bytes + b.stats_bytes : 0;
}

// q, v [n, ld] f32, kp [k, h * 256] f32, out [k, h * 256], attn [h, n, k] / lse [h, n] or null
int snf_sparse_attn_fwd_x3_dk256(const float* q, int64_t ldq, const float* v, int64_t ldv, const float* kp, int64_t n, int k, int h,
                                 float scale, float* out, float* attn, float* lse, void* workspace, size_t workspace_bytes,
                                 snf_stream_t stream) {
    const char* me = "snf_sparse_attn_fwd_x3_dk256";
    if (int rc = require(me, q && v && kp && out, "null pointer")) return rc;
    if (int rc = require(me, n >= 1 && k >= 1 && h >= 1, "bad shape")) return rc;
    const X3Y f{{}, h};
    BagLaunch b;
    if (!plan_bag(f, n, k, h, &b)) {
        snf::set_error("snf_sparse_attn_fwd_x3_dk256: unsupported shape k=%d (k <= %d x %d)", k, X3Y_MAX_CHUNKS, X3Y_KMAX);
        return SNF_EUNSUPPORTED;
    }
    X3Params P;
    const Operands<float, float> o{q, v, ldq, ldv, 4, kp, false, k, h, scale, out, attn, lse, workspace, workspace_bytes, snf::as_stream(stream)};
    return forward_bag(me, f, b, o, n, b.chunks.size, P, [&](bool stats_pass, X3Params& P, const X3Plan& pl, float* out_c) {
        return x3y_launch_pass<false>(stats_pass, P, pl, out_c, o.stream);
    });
}

// ---- varlen (see snf_sparse_attn_varlen_plan in sparse_attn_mfma.hip for the protocol) ----
int snf_sparse_attn_x3_varlen_dk256_plan(const int64_t* offsets, int bags, int k, int h, int32_t* table, size_t table_ints,
                                         size_t* table_ints_needed, size_t* workspace_bytes, int* n_chunks, int* chunk_k) {
    const char* me = "snf_sparse_attn_x3_varlen_dk256_plan";
    if (int rc = require(me, offsets && bags >= 1 && h >= 1, "bad arguments")) return rc;   // k < 1: an unsupported shape here
    return varlen_plan_reply(me, X3Y{{}, h}, offsets, bags, k, h, X3Y_MAX_CHUNKS, table, table_ints, table_ints_needed, workspace_bytes, n_chunks,
                             chunk_k, [&] {
        snf::set_error("snf_sparse_attn_x3_varlen_dk256_plan: unsupported shape (bags=%d k=%d: need 1 <= k <= %d = %d chunks of %d, "
                       "non-empty bags)", bags, k, X3Y_MAX_CHUNKS * X3Y_KMAX, X3Y_MAX_CHUNKS, X3Y_KMAX);
    });
}

// q, v [T, ld] f32 packed rows, kp [bags * k, h * 256] f32, out [bags * k, h * 256], attn [h, T, k] / lse [h, T] or null;
// table_dev / workspace from snf_sparse_attn_x3_varlen_dk256_plan
int snf_sparse_attn_fwd_x3_varlen_dk256(const float* q, int64_t ldq, const float* v, int64_t ldv, const float* kp,
                                        const int64_t* offsets, int bags, int k, int h, float scale, float* out, float* attn,
                                        float* lse, const int32_t* table_dev, void* workspace, size_t workspace_bytes,
                                        snf_stream_t stream) {
    const char* me = "snf_sparse_attn_fwd_x3_varlen_dk256";
    if (int rc = require(me, q && v && kp && out && offsets && table_dev, "null pointer")) return rc;
    if (int rc = require(me, bags >= 1 && h >= 1, "bad shape")) return rc;
    const X3Y f{{}, h};
    VarlenLaunch vl;
    if (!plan_varlen(f, offsets, bags, k, h, X3Y_MAX_CHUNKS, &vl, nullptr, 0)) {
        snf::set_error("snf_sparse_attn_fwd_x3_varlen_dk256: unsupported shape (bags=%d k=%d)", bags, k);
        return SNF_EUNSUPPORTED;
    }
    X3Params P;
    const Operands<float, float> o{q, v, ldq, ldv, 4, kp, false, k, h, scale, out, attn, lse, workspace, workspace_bytes, snf::as_stream(stream)};
    return forward_varlen(me, f, vl, o, offsets, bags, table_dev, P, [&](bool stats_pass, X3Params& P, const X3Plan& pl, float* out_c) {
        return x3y_launch_pass<true>(stats_pass, P, pl, out_c, o.stream);
    });
}

}  // extern "C"
