// K7 (fast form), translation unit 8: every varlen (many bags per launch) form at dk = 192 -- the forward at 1, 2, 4 key blocks, its
// key-chunked forms at 2, 4 key blocks and the statistics pass -- with the two C entry points of the width (see sparse_attn_mfma_impl.h).
// The kernels are sparse_attn_mfma_kernel<192, NKB, bf16, AUX, EXT, 8, VL = true> / sparse_attn_stats_kernel<192, NKB, bf16, VL = true>
// under names of their own: the varlen plan functions of dk = 64 / 128 keep refusing this width, and the single-bag kernels of dk = 192
// keep their symbols (and the counts tests/test_attn_dk192_host.py holds them to) to themselves.  The driver is attn_drive.h.
#define SNF_ATTN_MFMA_KERNEL sparse_attn_mfma_vl192_kernel
#define SNF_ATTN_STATS_KERNEL sparse_attn_stats_vl192_kernel
#include "sparse_attn_mfma_impl.h"
#include "attn_width.h"

namespace {

using namespace snf_attn;   // the driver (attn_drive.h) and the entry bodies (attn_width.h)
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

// What the entry bodies of attn_width.h ask: the family, the kernel switch above and the wording of the two entry points
struct E {
    using Family = Vl192;
    static constexpr int MAX_CHUNKS = ::MAX_CHUNKS;
    static constexpr bool SHORT_TABLE_UNSUPPORTED = false;
    static bool plan_args_ok(int bags, int k, int h) { return bags >= 1 && k >= 1 && h >= 1; }
    static bool varlen_shape_ok(int, int k, int h) { return k >= 1 && h >= 1; }
    static void refuse_plan(const char* me, int bags, int k, int) {
        snf::set_error("%s: unsupported shape (bags=%d k=%d: need k <= %d = %d chunks of %d, non-empty bags)", me, bags, k,
                       MAX_CHUNKS * attn_kmax(DK), MAX_CHUNKS, attn_kmax(DK));
    }
    template <bool VL>
    static int pass(bool, bool stats_pass, const AttnParams& P, const Plan& pl, float* out, hipStream_t s) {
        return launch_nkb_vl192(stats_pass, P, pl, out, s);
    }
};

}  // namespace

extern "C" {

int snf_sparse_attn_varlen_dk192_plan(const int64_t* offsets, int bags, int k, int h, int32_t* table, size_t table_ints,
                                      size_t* table_ints_needed, size_t* workspace_bytes, int* n_chunks, int* chunk_k) {
    return entry_varlen_plan<E>("snf_sparse_attn_varlen_dk192_plan", offsets, bags, k, h, table, table_ints, table_ints_needed,
                                workspace_bytes, n_chunks, chunk_k);
}

// layouts as snf_sparse_attn_fwd_mfma_varlen at dk = 192; table_dev / workspace from snf_sparse_attn_varlen_dk192_plan
int snf_sparse_attn_fwd_mfma_varlen_dk192(const void* q, int64_t ldq, const void* v, int64_t ldv, const void* kp, int kp_dtype,
                                          const int64_t* offsets, int bags, int k, int h, float scale, float* out, float* attn,
                                          float* lse, const int32_t* table_dev, void* workspace, size_t workspace_bytes,
                                          snf_stream_t stream) {
    return entry_forward_varlen<E>("snf_sparse_attn_fwd_mfma_varlen_dk192", q, ldq, v, ldv, kp, kp_dtype, offsets, bags, k, h, scale, out,
                                   attn, lse, table_dev, workspace, workspace_bytes, stream);
}

}  // extern "C"
