// K7 (fast form, bf16) at head width 256 (the SimCLR ResNet-18 recipe, D = 512, h = 2): the one-launch forms at 1, 2, 4 key blocks,
// single bag and varlen, and the four C entry points of the width (the kernel is in sparse_attn_mfma_dk256_impl.h; the key-chunked forms
// build in sparse_attn_mfma_dk256_chunks.hip).  snf_sparse_attn_fwd_mfma and the varlen plan functions of dk = 64 / 128 and of 192 keep
// refusing this width.  The driver behind the entry points is attn_drive.h; this file describes the width to it.
#include "sparse_attn_mfma_dk256_impl.h"

namespace {

using namespace snf_attn;   // the driver (attn_drive.h)
constexpr int DK = A256_DK;

template <bool VL>
int a256_dispatch(const AttnParams& P, const Plan& pl, float* out, hipStream_t s) {
    const bool aux = P.attn != nullptr || P.lse != nullptr;
    switch (pl.nkb) {
        case 1: return aux ? a256_launch<1, true, 0, VL>(P, pl, out, s) : a256_launch<1, false, 0, VL>(P, pl, out, s);
        case 2: return aux ? a256_launch<2, true, 0, VL>(P, pl, out, s) : a256_launch<2, false, 0, VL>(P, pl, out, s);
        case 4: return aux ? a256_launch<4, true, 0, VL>(P, pl, out, s) : a256_launch<4, false, 0, VL>(P, pl, out, s);
        default: break;
    }
    snf::set_error("sparse_attn_mfma_dk256: key-block count %d not built", pl.nkb);
    return SNF_EUNSUPPORTED;
}

// The bf16 family at dk = 256: the family's chunk rule at 128 keys per launch for single bag and varlen alike (a packed bag's P and lse
// are those of its own launch bit for bit), every chunk launched at its own key-block count
struct A256 : MfmaDrive {
    static constexpr const char* DK_TEXT = "256";
    static constexpr int dk = DK;
    int h;
    // every chunk at a key-block count that is built: the single-bag plan refuses here what the varlen plan refuses through built()
    bool chunks(int k, Chunks* c) const {
        if (!a256_chunks(k, c)) return false;
        for (int i = 0; i < c->count; ++i) {
            const int kc = k - i * c->size < c->size ? k - i * c->size : c->size;
            Plan one;
            if (kc < 1 || !a256_plan(1, kc, 1, &one, true) || !a256_built(c->count > 1, one.nkb)) return false;
        }
        return true;
    }
    bool plan(int64_t n, int kc, Plan* pl, bool packed) const { return a256_plan(n, kc, h, pl, packed); }
    bool built(bool chunked, int nkb) const { return a256_built(chunked, nkb); }
};

// one chunk: the MODE 0 kernels; more: MODE 1 per chunk, then MODE 2
template <bool VL>
int a256_launch_pass(bool stats_pass, const AttnParams& P, const Plan& pl, float* out, hipStream_t s) {
    if (P.n_chunks == 1) return a256_dispatch<VL>(P, pl, out, s);
    return snf::attn_dk256_launch_chunk(stats_pass ? 1 : 2, P, pl, out, s);
}

}  // namespace

extern "C" {

// partial tiles | chunk statistics | bf16 copy of an f32 Kp
size_t snf_sparse_attn_fwd_mfma_dk256_workspace_bytes(int64_t n, int k, int h) {
    BagLaunch b;
    return (h >= 1 && n >= 1 && plan_bag(A256{{}, h}, n, k, h, &b)) ? b.partial_bytes + b.stats_bytes + b.staging_bytes : 0;
}

// q, v [n, ld] bf16, kp [k, h * 256] f32 | bf16, out [k, h * 256] f32, attn [h, n, k] / lse [h, n] or null
int snf_sparse_attn_fwd_mfma_dk256(const void* q, int64_t ldq, const void* v, int64_t ldv, const void* kp, int kp_dtype, int64_t n, int k,
                                   int h, float scale, float* out, float* attn, float* lse, void* workspace, size_t workspace_bytes,
                                   snf_stream_t stream) {
    const char* me = "snf_sparse_attn_fwd_mfma_dk256";
    if (int rc = require(me, q && v && kp && out, "null pointer")) return rc;
    if (int rc = require(me, n >= 1 && k >= 1 && h >= 1, "bad shape")) return rc;
    SNF_REQUIRE(kp_dtype == SNF_DT_F32 || kp_dtype == SNF_DT_BF16, "snf_sparse_attn_fwd_mfma_dk256: bad kp dtype %d", kp_dtype);
    const A256 f{{}, h};
    BagLaunch b;
    if (!plan_bag(f, n, k, h, &b)) {
        snf::set_error("snf_sparse_attn_fwd_mfma_dk256: unsupported shape n=%lld k=%d (k <= %d = %d chunks of %d)", (long long)n, k,
                       A256_MAX_CHUNKS * A256_KMAX, A256_MAX_CHUNKS, A256_KMAX);
        return SNF_EUNSUPPORTED;
    }
    AttnParams P;
    P.trace = nullptr, P.trace_wg = 0, P.drop = snf::make_dropout(0.f, 0, 0);
    const Operands<void, void> o{q, v, ldq, ldv, 8, kp, kp_dtype == SNF_DT_F32, k, h, scale, out, attn, lse, workspace, workspace_bytes,
                                 snf::as_stream(stream)};
    return forward_bag(me, f, b, o, n, b.chunks.size, P, [&](bool stats_pass, AttnParams& P, const Plan& pl, float* out_c) {
        return a256_launch_pass<false>(stats_pass, P, pl, out_c, o.stream);
    });
}

// ---- varlen (see snf_sparse_attn_varlen_plan in sparse_attn_mfma.hip for the protocol) ----
int snf_sparse_attn_varlen_dk256_plan(const int64_t* offsets, int bags, int k, int h, int32_t* table, size_t table_ints,
                                      size_t* table_ints_needed, size_t* workspace_bytes, int* n_chunks, int* chunk_k) {
    const char* me = "snf_sparse_attn_varlen_dk256_plan";
    if (int rc = require(me, offsets && bags >= 1, "bad arguments")) return rc;   // k < 1, h < 1: an unsupported shape here
    const auto refuse = [&] {
        snf::set_error("snf_sparse_attn_varlen_dk256_plan: unsupported shape (bags=%d k=%d h=%d: need 1 <= k <= %d = %d chunks of %d, "
                       "h >= 1, non-empty bags)", bags, k, h, A256_MAX_CHUNKS * A256_KMAX, A256_MAX_CHUNKS, A256_KMAX);
    };
    // sizes first: a table that is too short is this entry point's own refusal (SNF_EUNSUPPORTED, nothing written)
    size_t need = 0;
    if (int rc = varlen_plan_reply(me, A256{{}, h}, offsets, bags, k, h, A256_MAX_CHUNKS, nullptr, 0, &need, workspace_bytes, n_chunks, chunk_k,
                                   refuse))
        return rc;
    if (table_ints_needed) *table_ints_needed = need;
    if (!table) return SNF_OK;
    if (table_ints < need) {
        snf::set_error("snf_sparse_attn_varlen_dk256_plan: unsupported table of %zu ints (the plan needs %zu)", table_ints, need);
        return SNF_EUNSUPPORTED;
    }
    return varlen_plan_reply(me, A256{{}, h}, offsets, bags, k, h, A256_MAX_CHUNKS, table, table_ints, table_ints_needed, workspace_bytes,
                             n_chunks, chunk_k, refuse);
}

// q, v [T, ld] bf16 packed rows, kp [bags * k, h * 256] f32 | bf16, out [bags * k, h * 256] f32, attn [h, T, k] / lse [h, T] or null;
// table_dev / workspace from snf_sparse_attn_varlen_dk256_plan
int snf_sparse_attn_fwd_mfma_varlen_dk256(const void* q, int64_t ldq, const void* v, int64_t ldv, const void* kp, int kp_dtype,
                                          const int64_t* offsets, int bags, int k, int h, float scale, float* out, float* attn,
                                          float* lse, const int32_t* table_dev, void* workspace, size_t workspace_bytes,
                                          snf_stream_t stream) {
    const char* me = "snf_sparse_attn_fwd_mfma_varlen_dk256";
    if (int rc = require(me, q && v && kp && out && offsets && table_dev, "null pointer")) return rc;
    SNF_REQUIRE(kp_dtype == SNF_DT_F32 || kp_dtype == SNF_DT_BF16, "snf_sparse_attn_fwd_mfma_varlen_dk256: bad kp dtype %d", kp_dtype);
    if (int rc = require(me, bags >= 1 && k >= 1 && h >= 1, "bad shape")) return rc;
    const A256 f{{}, h};
    VarlenLaunch vl;
    if (!plan_varlen(f, offsets, bags, k, h, A256_MAX_CHUNKS, &vl, nullptr, 0)) {
        snf::set_error("snf_sparse_attn_fwd_mfma_varlen_dk256: unsupported shape (bags=%d k=%d)", bags, k);
        return SNF_EUNSUPPORTED;
    }
    AttnParams P;
    P.trace = nullptr, P.trace_wg = 0, P.drop = snf::make_dropout(0.f, 0, 0);
    const Operands<void, void> o{q, v, ldq, ldv, 8, kp, kp_dtype == SNF_DT_F32, k, h, scale, out, attn, lse, workspace, workspace_bytes,
                                 snf::as_stream(stream)};
    return forward_varlen(me, f, vl, o, offsets, bags, table_dev, P, [&](bool stats_pass, AttnParams& P, const Plan& pl, float* out_c) {
        return a256_launch_pass<true>(stats_pass, P, pl, out_c, o.stream);
    });
}

}  // extern "C"
