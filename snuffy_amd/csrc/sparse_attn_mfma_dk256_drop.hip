// K7 (fast form, bf16) at head width 256, third translation unit: the TRAINING forward -- attention dropout inside the kernel.  The kernel
// text is sparse_attn_mfma_dk256_impl.h's under the name sparse_attn_mfma_dk256_drop_kernel<NKB, AUX, MODE> with the Philox mask compiled
// in: single bag, AUX only, one launch (MODE 0) at 1, 2, 4 key blocks and the main pass of a key chunk (MODE 2) at 2, 4.  The statistics
// passes of a chunked launch never see the mask: they are the width's existing ones (sparse_attn_mfma_dk256_chunks.hip).
#define SNF_ATTN_DK256_KERNEL sparse_attn_mfma_dk256_drop_kernel
#define SNF_ATTN_DK256_DROP true
#include "sparse_attn_mfma_dk256_impl.h"

namespace {
using namespace snf_attn;
using F = WidthFamily<A256>;

template <int MODE>
int drop_launch(const AttnParams& P, const TilePlan& pl, float* out, hipStream_t s) {
    switch (pl.nkb) {
        case 1:
            if constexpr (MODE == 0) return width_launch<A256, 1, true, 0, false>(P, pl, out, s);
            break;
        case 2: return width_launch<A256, 2, true, MODE, false>(P, pl, out, s);
        case 4: return width_launch<A256, 4, true, MODE, false>(P, pl, out, s);
        default: break;
    }
    snf::set_error("sparse_attn_mfma_dk256 (dropout): key-block count %d not built", pl.nkb);
    return SNF_EUNSUPPORTED;
}
}  // namespace

extern "C" {

// snf_sparse_attn_fwd_mfma_dk256 with attention dropout: attn (when asked for) is P o M, out = (P o M)^T V, lse is that of P.  The
// workspace is snf_sparse_attn_fwd_mfma_dk256_workspace_bytes'.
int snf_sparse_attn_fwd_mfma_dk256_dropout(const void* q, int64_t ldq, const void* v, int64_t ldv, const void* kp, int kp_dtype, int64_t n,
                                           int k, int h, float scale, float* out, float* attn, float* lse, void* workspace,
                                           size_t workspace_bytes, snf_stream_t stream, float dropout_p, uint64_t seed, uint64_t offset) {
    const char* me = "snf_sparse_attn_fwd_mfma_dk256_dropout";
    SNF_REQUIRE(dropout_p >= 0.f && dropout_p < 1.f, "%s: dropout_p=%f outside [0, 1)", me, dropout_p);
    if (!(dropout_p > 0.f))   // the existing launch, bit for bit
        return snf_sparse_attn_fwd_mfma_dk256(q, ldq, v, ldv, kp, kp_dtype, n, k, h, scale, out, attn, lse, workspace, workspace_bytes, stream);
    if (int rc = require(me, q && v && kp && out, "null pointer")) return rc;
    SNF_REQUIRE(attn || lse, "%s: dropout needs the lse (or attn) output -- the backward regenerates the mask and recomputes P from lse", me);
    if (int rc = require(me, n >= 1 && k >= 1 && h >= 1, "bad shape")) return rc;
    AttnParams P;
    bool kp_f32;
    if (int rc = F::open(me, kp_dtype, P, &kp_f32)) return rc;
    P.drop = snf::make_dropout(dropout_p, seed, offset);
    const F f{{}, h};
    BagLaunch b;
    if (!plan_bag(f, n, k, h, &b)) {
        A256::refuse_bag(me, n, k);
        return SNF_EUNSUPPORTED;
    }
    // Every pass runs on the chunks of the launch without dropout (the same key blocks, the same workspace): this kernel's P depends on
    // which keys share a 32-key block, so lse AND the normalised P are that launch's bit for bit only on its own chunks.  The family's
    // entry rounds the main passes' chunks to a multiple of 4 instead (one Philox call covers 4 keys); here a chunk that starts off a
    // multiple of 4 draws the two groups its lanes' keys straddle.
    const bool chunked = b.chunks.count > 1;
    const Operands<void, void> o{q, v, ldq, ldv, F::ROW_ALIGN, kp, kp_f32, k, h, scale, out, attn, lse, workspace, workspace_bytes,
                                 snf::as_stream(stream)};
    return forward_bag(me, f, b, o, n, b.chunks.size, P, [&](bool stats_pass, AttnParams& P, const TilePlan& pl, float* out_c) {
        if (stats_pass) return snf::attn_dk256_launch_chunk(1, P, pl, out_c, o.stream);
        return chunked ? drop_launch<2>(P, pl, out_c, o.stream) : drop_launch<0>(P, pl, out_c, o.stream);
    });
}

}  // extern "C"
