// K7 (fast form), translation unit 8: every varlen (many bags per launch) form at dk = 192 -- the forward at 1, 2, 4 key blocks, its
// key-chunked forms at 2, 4 key blocks and the statistics pass -- with the two C entry points of the width (see sparse_attn_mfma_impl.h).
// The kernels are sparse_attn_mfma_kernel<192, NKB, bf16, AUX, EXT, 8, VL = true> / sparse_attn_stats_kernel<192, NKB, bf16, VL = true>
// under names of their own: the varlen plan functions of dk = 64 / 128 keep refusing this width, and the single-bag kernels of dk = 192
// keep their symbols (and the counts tests/test_attn_dk192_host.py holds them to) to themselves.  The driver is attn_drive.h.
#define SNF_ATTN_MFMA_KERNEL sparse_attn_mfma_vl192_kernel
#define SNF_ATTN_STATS_KERNEL sparse_attn_stats_vl192_kernel
#include "sparse_attn_mfma_impl.h"

namespace {

using namespace snf_attn;   // the driver (attn_drive.h)
constexpr int DK = 192;
using QT = unsigned short;   // bf16 Q | V

template <int NKB, bool AUX, bool EXT>
int launch_vl192(const AttnParams& P, const Plan& pl, float* out, hipStream_t s) {
    return launch_variant<DK, NKB, QT, AUX, EXT, 8, true>(P, pl, out, s);   // 136 KiB of LDS at 4 key blocks: Kp 48 + P 40 + V 48
}
template <int NKB>
int launch_stats_vl192(const AttnParams& P, const Plan& pl, hipStream_t s) {
    return launch_stats_variant<DK, NKB, QT, true>(P, pl, s);
}

// key-block counts the launches are built for: one chunk 1, 2, 4; a chunk of a key-chunked launch (65 .. 128 keys, 64 as the last of
// two) 2, 4
constexpr bool vl192_built(bool chunked, int nkb) { return nkb == 2 || nkb == 4 || (nkb == 1 && !chunked); }

// pass 0 of a key-chunked launch: the chunk's statistics; otherwise the forward (P.stats: normalising over all chunks)
int launch_nkb_vl192(bool stats_pass, const AttnParams& P, const Plan& pl, float* out, hipStream_t s) {
    const bool aux = P.attn != nullptr || P.lse != nullptr;
    if (stats_pass) {
        switch (pl.nkb) {
            case 2: return launch_stats_vl192<2>(P, pl, s);
            case 4: return launch_stats_vl192<4>(P, pl, s);
            default: break;
        }
    } else if (P.stats) {
        switch (pl.nkb) {
            case 2: return aux ? launch_vl192<2, true, true>(P, pl, out, s) : launch_vl192<2, false, true>(P, pl, out, s);
            case 4: return aux ? launch_vl192<4, true, true>(P, pl, out, s) : launch_vl192<4, false, true>(P, pl, out, s);
            default: break;
        }
    } else {
        switch (pl.nkb) {
            case 1: return aux ? launch_vl192<1, true, false>(P, pl, out, s) : launch_vl192<1, false, false>(P, pl, out, s);
            case 2: return aux ? launch_vl192<2, true, false>(P, pl, out, s) : launch_vl192<2, false, false>(P, pl, out, s);
            case 4: return aux ? launch_vl192<4, true, false>(P, pl, out, s) : launch_vl192<4, false, false>(P, pl, out, s);
            default: break;
        }
    }
    snf::set_error("sparse_attn_mfma (varlen, dk = 192): key-block count %d not built", pl.nkb);
    return SNF_EUNSUPPORTED;
}

// The bf16 family at dk = 192, varlen: the chunks of make_chunks (the single-bag driver's rule: a packed bag's P and lse are those of its own
// launch bit for bit), planned by make_plan_any (make_plan keeps refusing the width to the 64 / 128 entry points)
struct Vl192 : MfmaDrive {
    static constexpr int dk = DK;
    int h;
    bool chunks(int k, Chunks* c) const { return make_chunks(k, DK, c); }
    bool plan(int64_t n, int kc, Plan* pl, bool packed) const { return make_plan_any(n, kc, h, DK, pl, packed); }
    bool built(bool chunked, int nkb) const { return vl192_built(chunked, nkb); }   // asked of a single chunk too
};

}  // namespace

extern "C" {

int snf_sparse_attn_varlen_dk192_plan(const int64_t* offsets, int bags, int k, int h, int32_t* table, size_t table_ints,
                                      size_t* table_ints_needed, size_t* workspace_bytes, int* n_chunks, int* chunk_k) {
    const char* me = "snf_sparse_attn_varlen_dk192_plan";
    if (int rc = require(me, offsets && bags >= 1 && k >= 1 && h >= 1, "bad arguments")) return rc;
    return varlen_plan_reply(me, Vl192{{}, h}, offsets, bags, k, h, MAX_CHUNKS, table, table_ints, table_ints_needed, workspace_bytes, n_chunks,
                             chunk_k, [&] {
        snf::set_error("snf_sparse_attn_varlen_dk192_plan: unsupported shape (bags=%d k=%d: need k <= %d = %d chunks of %d, non-empty "
                       "bags)", bags, k, MAX_CHUNKS * attn_kmax(DK), MAX_CHUNKS, attn_kmax(DK));
    });
}

// layouts as snf_sparse_attn_fwd_mfma_varlen at dk = 192; table_dev / workspace from snf_sparse_attn_varlen_dk192_plan
int snf_sparse_attn_fwd_mfma_varlen_dk192(const void* q, int64_t ldq, const void* v, int64_t ldv, const void* kp, int kp_dtype,
                                          const int64_t* offsets, int bags, int k, int h, float scale, float* out, float* attn,
                                          float* lse, const int32_t* table_dev, void* workspace, size_t workspace_bytes,
                                          snf_stream_t stream) {
    const char* me = "snf_sparse_attn_fwd_mfma_varlen_dk192";
    if (int rc = require(me, q && v && kp && out && offsets && table_dev, "null pointer")) return rc;
    SNF_REQUIRE(kp_dtype == SNF_DT_F32 || kp_dtype == SNF_DT_BF16, "snf_sparse_attn_fwd_mfma_varlen_dk192: bad kp dtype %d", kp_dtype);
    if (int rc = require(me, k >= 1 && h >= 1, "bad shape")) return rc;
    const Vl192 f{{}, h};
    VarlenLaunch vl;
    if (!plan_varlen(f, offsets, bags, k, h, MAX_CHUNKS, &vl, nullptr, 0)) {
        snf::set_error("snf_sparse_attn_fwd_mfma_varlen_dk192: unsupported shape (bags=%d k=%d)", bags, k);
        return SNF_EUNSUPPORTED;
    }
    AttnParams P;
    P.trace = nullptr, P.trace_wg = 0, P.drop = snf::make_dropout(0.f, 0, 0);
    const Operands<void, void> o{q, v, ldq, ldv, 8, kp, kp_dtype == SNF_DT_F32, k, h, scale, out, attn, lse, workspace, workspace_bytes,
                                 snf::as_stream(stream)};
    return forward_varlen(me, f, vl, o, offsets, bags, table_dev, P, [&](bool stats_pass, AttnParams& P, const Plan& pl, float* out_c) {
        return launch_nkb_vl192(stats_pass, P, pl, out_c, o.stream);
    });
}

}  // extern "C"
