// K7 (fast form), translation unit 1: the dk = 128 kernel variants, the width switch, and the C entry points of the bf16 family at
// dk = 64 / 128 (single bag: also 192).  The driver behind the entry points is attn_drive.h; this file describes the family to it.
#include "sparse_attn_mfma_impl.h"

namespace snf {
unsigned long long* g_attn_trace = nullptr;  // debug hook, see snf_debug_attn_trace (also read by sparse_attn_x3p.hip)
int g_attn_trace_wg = 0;
}  // namespace snf
using snf::g_attn_trace;
using snf::g_attn_trace_wg;

namespace snf {
int attn_launch_dk128(int qv_dtype, bool stats_pass, const AttnParams& P, const Plan& pl, float* out, hipStream_t s) {
    if (stats_pass)
        return qv_dtype == SNF_DT_F32 ? launch_stats<128, float>(P, pl, s) : launch_stats<128, unsigned short>(P, pl, s);
    return qv_dtype == SNF_DT_F32 ? launch_nkb<128, float>(P, pl, out, s) : launch_nkb<128, unsigned short>(P, pl, out, s);
}
}  // namespace snf

// the translation unit of the head width (make_chunks admitted dk: 64, 128 or 192)
static int attn_launch(int dk, int qv_dtype, bool stats_pass, const AttnParams& P, const Plan& pl, float* out, hipStream_t s) {
    if (dk == 128) return snf::attn_launch_dk128(qv_dtype, stats_pass, P, pl, out, s);
    if (dk == 192) return snf::attn_launch_dk192(qv_dtype, stats_pass, P, pl, out, s);
    return snf::attn_launch_dk64(qv_dtype, stats_pass, P, pl, out, s);
}

namespace {
using namespace snf_attn;   // the driver (attn_drive.h)

// The bf16 family as this file's entry points plan it.  Varlen serves dk = 64 / 128 only (make_plan refuses a packed bag at dk = 192:
// that width's varlen forms have a description of their own in sparse_attn_mfma_varlen_dk192.hip).
struct Mfma : MfmaDrive {
    int dk, h;
    bool varlen;
    bool chunks(int k, Chunks* c) const { return (!varlen || dk == 64 || dk == 128) && make_chunks(k, dk, c); }
    bool plan(int64_t n, int kc, Plan* pl, bool packed) const { return make_plan(n, kc, h, dk, pl, packed); }
    bool built(bool chunked, int nkb) const { return !chunked || varlen_chunk_built(dk, nkb); }   // one chunk: every count is built
};

// the launch of the two varlen entry points: one chunk runs the plain varlen kernels, more run the statistics and EXT forms
int mfma_varlen_launch(const char* me, const Mfma& f, const VarlenLaunch& vl, const Operands<void, void>& o, const int64_t* offsets, int bags,
                       const int32_t* table_dev) {
    AttnParams P;
    P.trace = nullptr, P.trace_wg = 0, P.drop = snf::make_dropout(0.f, 0, 0);
    return forward_varlen(me, f, vl, o, offsets, bags, table_dev, P, [&](bool stats_pass, AttnParams& P, const Plan& pl, float* out_c) {
        if (vl.chunks.count == 1)
            return f.dk == 128 ? snf::attn_launch_varlen_dk128(P, pl, out_c, o.stream) : snf::attn_launch_varlen_dk64(P, pl, out_c, o.stream);
        return f.dk == 128 ? snf::attn_launch_varlen_chunk_dk128(stats_pass, P, pl, out_c, o.stream)
                           : snf::attn_launch_varlen_chunk_dk64(stats_pass, P, pl, out_c, o.stream);
    });
}
}  // namespace

extern "C" {

// debug only (not part of the public header): device buffer of >= 64*8*4 u64 receiving s_memtime stamps of workgroup 0
void snf_debug_attn_trace(void* buf) { g_attn_trace = reinterpret_cast<unsigned long long*>(buf); }
void snf_debug_attn_trace_wg(int wg) { g_attn_trace_wg = wg; }

size_t snf_sparse_attn_fwd_workspace_bytes(int64_t n, int k, int h, int dk, int mfma) {
    if (n < 1 || k < 1 || h < 1 || dk < 1) return 0;
    if (!mfma) return snf::generic_attn_workspace_bytes(n, k, h, dk);
    BagLaunch b;   // partial tiles | chunk statistics | bf16 copy of an f32 Kp
    return plan_bag(Mfma{{}, dk, h, false}, n, k, h, &b) ? b.partial_bytes + b.stats_bytes + b.staging_bytes : 0;
}

int snf_sparse_attn_fwd_mfma(const void* q, int64_t ldq, const void* v, int64_t ldv, int qv_dtype, const void* kp,
                             int kp_dtype, int64_t n, int k, int h, int dk, float scale, float* out, float* attn,
                             float* lse, void* workspace, size_t workspace_bytes, snf_stream_t stream) {
    return snf_sparse_attn_fwd_mfma_dropout(q, ldq, v, ldv, qv_dtype, kp, kp_dtype, n, k, h, dk, scale, out, attn, lse, 0.f, 0, 0,
                                            workspace, workspace_bytes, stream);
}

int snf_sparse_attn_fwd_mfma_dropout(const void* q, int64_t ldq, const void* v, int64_t ldv, int qv_dtype, const void* kp,
                                     int kp_dtype, int64_t n, int k, int h, int dk, float scale, float* out, float* attn,
                                     float* lse, float dropout_p, uint64_t seed, uint64_t offset, void* workspace,
                                     size_t workspace_bytes, snf_stream_t stream) {
    const char* me = "snf_sparse_attn_fwd_mfma";
    if (int rc = require(me, q && v && kp && out, "null pointer")) return rc;
    SNF_REQUIRE(dropout_p >= 0.f && dropout_p < 1.f, "snf_sparse_attn_fwd_mfma: dropout_p=%f outside [0, 1)", dropout_p);
    SNF_REQUIRE(!(dropout_p > 0.f) || attn || lse, "snf_sparse_attn_fwd_mfma: dropout needs the lse (or attn) output -- "
                "the backward regenerates the mask and recomputes P from lse");
    if (int rc = require(me, n >= 1 && k >= 1 && h >= 1, "bad shape")) return rc;
    SNF_REQUIRE(qv_dtype == SNF_DT_F32 || qv_dtype == SNF_DT_BF16, "snf_sparse_attn_fwd_mfma: bad dtype %d", qv_dtype);
    SNF_REQUIRE(kp_dtype == SNF_DT_F32 || kp_dtype == SNF_DT_BF16, "snf_sparse_attn_fwd_mfma: bad kp dtype %d", kp_dtype);
    const Mfma f{{}, dk, h, false};
    BagLaunch b;
    if (!plan_bag(f, n, k, h, &b)) {
        snf::set_error("snf_sparse_attn_fwd_mfma: unsupported shape k=%d dk=%d (need dk in {64, 128, 192} and k <= %d keys "
                       "= %d chunks of %d)", k, dk, MAX_CHUNKS * attn_kmax(dk), MAX_CHUNKS, attn_kmax(dk));
        return SNF_EUNSUPPORTED;
    }
    // one Philox call covers 4 consecutive keys of a row: with dropout the MAIN passes' chunks start on multiples of 4.  Rounding the
    // chunk length up changes neither the chunk count nor the key blocks of a chunk (the workspace), and every chunk keeps a built
    // key-block count (the last one holds more than size - 4 count keys).  The statistics passes keep the chunks they always
    // had, and a main pass only sees the statistics combined over ALL chunks: lse and the normalised P are, bit for bit, those of
    // the launch without dropout.
    const int main_size = (dropout_p > 0.f && b.chunks.count > 1) ? (b.chunks.size + 3) & ~3 : b.chunks.size;
    AttnParams P;
    P.trace = g_attn_trace, P.trace_wg = g_attn_trace_wg, P.drop = snf::make_dropout(dropout_p, seed, offset);
    const Operands<void, void> o{q, v, ldq, ldv, qv_dtype == SNF_DT_BF16 ? 8 : 4, kp, kp_dtype == SNF_DT_F32, k, h, scale, out, attn, lse,
                                 workspace, workspace_bytes, snf::as_stream(stream)};
    return forward_bag(me, f, b, o, n, main_size, P, [&](bool stats_pass, AttnParams& P, const Plan& pl, float* out_c) {
        return attn_launch(dk, qv_dtype, stats_pass, P, pl, out_c, o.stream);
    });
}

// ---- varlen: many bags in one launch (small bags are launch-latency bound: SURVEY 7 step 8) ---------------------------------
// offsets[bags + 1] (HOST memory) = first packed row of every bag.  Sizes of the plan table (int32 words, built on the host by
// this call when `table` is given and uploaded by the caller once per batch composition) and of the launch workspace.
int snf_sparse_attn_varlen_plan(const int64_t* offsets, int bags, int k, int h, int dk, int32_t* table, size_t table_ints,
                                size_t* table_ints_needed, size_t* workspace_bytes) {
    const char* me = "snf_sparse_attn_varlen_plan";
    if (int rc = require(me, offsets && bags >= 1 && k >= 1 && h >= 1, "bad arguments")) return rc;
    return varlen_plan_reply(me, Mfma{{}, dk, h, true}, offsets, bags, k, h, 1, table, table_ints, table_ints_needed, workspace_bytes, nullptr,
                             nullptr, [&] {
        snf::set_error("snf_sparse_attn_varlen_plan: unsupported shape (bags=%d k=%d dk=%d: need dk in {64, 128}, k <= %d, "
                       "non-empty bags)", bags, k, dk, dk == 128 ? 224 : 256);
    });
}

// q, v [T, ld] bf16 (T = offsets[bags] packed rows), kp [bags * k, h * dk] (bag b's keys in rows b k .. b k + k - 1),
// out [bags * k, h * dk] f32, attn [h, T, k] / lse [h, T] or null.  table_dev = the uploaded plan table.
int snf_sparse_attn_fwd_mfma_varlen(const void* q, int64_t ldq, const void* v, int64_t ldv, const void* kp, int kp_dtype,
                                    const int64_t* offsets, int bags, int k, int h, int dk, float scale, float* out, float* attn,
                                    float* lse, const int32_t* table_dev, void* workspace, size_t workspace_bytes,
                                    snf_stream_t stream) {
    const char* me = "snf_sparse_attn_fwd_mfma_varlen";
    if (int rc = require(me, q && v && kp && out && offsets && table_dev, "null pointer")) return rc;
    SNF_REQUIRE(kp_dtype == SNF_DT_F32 || kp_dtype == SNF_DT_BF16, "snf_sparse_attn_fwd_mfma_varlen: bad kp dtype %d", kp_dtype);
    const Mfma f{{}, dk, h, true};
    VarlenLaunch vl;
    if (!plan_varlen(f, offsets, bags, k, h, 1, &vl, nullptr, 0)) {
        snf::set_error("snf_sparse_attn_fwd_mfma_varlen: unsupported shape (bags=%d k=%d dk=%d)", bags, k, dk);
        return SNF_EUNSUPPORTED;
    }
    return mfma_varlen_launch(me, f, vl, {q, v, ldq, ldv, 8, kp, kp_dtype == SNF_DT_F32, k, h, scale, out, attn, lse, workspace,
                                          workspace_bytes, snf::as_stream(stream)}, offsets, bags, table_dev);
}

// ---- varlen above one key chunk: the chunks of make_chunks (the single-bag driver's rule, so a packed bag's P and lse are those of its
// own launch bit for bit), a statistics launch per chunk over all bags, then the chunks' main launches normalising over all chunks.
int snf_sparse_attn_varlen_chunked_plan(const int64_t* offsets, int bags, int k, int h, int dk, int32_t* table, size_t table_ints,
                                        size_t* table_ints_needed, size_t* workspace_bytes, int* n_chunks, int* chunk_k) {
    const char* me = "snf_sparse_attn_varlen_chunked_plan";
    if (int rc = require(me, offsets && bags >= 1 && k >= 1 && h >= 1, "bad arguments")) return rc;
    return varlen_plan_reply(me, Mfma{{}, dk, h, true}, offsets, bags, k, h, MAX_CHUNKS, table, table_ints, table_ints_needed, workspace_bytes,
                             n_chunks, chunk_k, [&] {
        snf::set_error("snf_sparse_attn_varlen_chunked_plan: unsupported shape (bags=%d k=%d dk=%d: need dk in {64, 128}, k <= %d "
                       "= %d chunks of %d, non-empty bags)", bags, k, dk, MAX_CHUNKS * attn_kmax(dk == 64 ? 64 : 128), MAX_CHUNKS,
                       attn_kmax(dk == 64 ? 64 : 128));
    });
}

// layouts as snf_sparse_attn_fwd_mfma_varlen; table_dev / workspace from snf_sparse_attn_varlen_chunked_plan
int snf_sparse_attn_fwd_mfma_varlen_chunked(const void* q, int64_t ldq, const void* v, int64_t ldv, const void* kp, int kp_dtype,
                                            const int64_t* offsets, int bags, int k, int h, int dk, float scale, float* out,
                                            float* attn, float* lse, const int32_t* table_dev, void* workspace,
                                            size_t workspace_bytes, snf_stream_t stream) {
    const char* me = "snf_sparse_attn_fwd_mfma_varlen_chunked";
    if (int rc = require(me, q && v && kp && out && offsets && table_dev, "null pointer")) return rc;
    SNF_REQUIRE(kp_dtype == SNF_DT_F32 || kp_dtype == SNF_DT_BF16, "snf_sparse_attn_fwd_mfma_varlen_chunked: bad kp dtype %d", kp_dtype);
    if (int rc = require(me, k >= 1 && h >= 1, "bad shape")) return rc;
    const Mfma f{{}, dk, h, true};
    VarlenLaunch vl;
    if (!plan_varlen(f, offsets, bags, k, h, MAX_CHUNKS, &vl, nullptr, 0)) {
        snf::set_error("snf_sparse_attn_fwd_mfma_varlen_chunked: unsupported shape (bags=%d k=%d dk=%d)", bags, k, dk);
        return SNF_EUNSUPPORTED;
    }
    if (vl.chunks.count == 1)   // one chunk: the launch, the table (integer for integer) and the refusals of the single-chunk entry point
        return snf_sparse_attn_fwd_mfma_varlen(q, ldq, v, ldv, kp, kp_dtype, offsets, bags, k, h, dk, scale, out, attn, lse, table_dev,
                                               workspace, workspace_bytes, stream);
    return mfma_varlen_launch(me, f, vl, {q, v, ldq, ldv, 8, kp, kp_dtype == SNF_DT_F32, k, h, scale, out, attn, lse, workspace,
                                          workspace_bytes, snf::as_stream(stream)}, offsets, bags, table_dev);
}

}  // extern "C"
