// K7 (fp32-class form) at head width 192 (the MAE recipe, D = 768, h = 4): the one-launch forms at 1, 2, 4 key blocks, single bag and
// varlen, and the four C entry points of the width (the kernel is in sparse_attn_x3_dk192_impl.h; the key-chunked forms build in
// sparse_attn_x3_dk192_chunks.hip).  The plan functions of dk = 64 / 128 keep refusing this width.
#include "sparse_attn_x3_dk192_impl.h"

namespace {

constexpr int DK = X3W_DK, NCB = DK / 32;

template <bool VL>
int x3w_dispatch(const X3Params& P, const X3Plan& pl, float* out, hipStream_t s) {
    const bool aux = P.attn != nullptr || P.lse != nullptr;
    switch (pl.nkb) {
        case 1: return aux ? x3w_launch<1, true, 0, VL>(P, pl, out, s) : x3w_launch<1, false, 0, VL>(P, pl, out, s);
        case 2: return aux ? x3w_launch<2, true, 0, VL>(P, pl, out, s) : x3w_launch<2, false, 0, VL>(P, pl, out, s);
        case 4: return aux ? x3w_launch<4, true, 0, VL>(P, pl, out, s) : x3w_launch<4, false, 0, VL>(P, pl, out, s);
        default: break;
    }
    snf::set_error("sparse_attn_x3_dk192: key-block count %d not built", pl.nkb);
    return SNF_EUNSUPPORTED;
}

// key-block count of a chunk of kc keys (0: none)
int x3w_chunk_nkb(int kc) {
    X3Plan one;
    return x3w_plan(1, kc, 1, &one, true) ? one.nkb : 0;
}
// the chunks of k keys, every one at a key-block count that is built (the plan is the one refusal point)
bool x3w_chunks_built(int k, X3Chunks* ch) {
    if (!x3w_chunks(k, ch)) return false;
    if (ch->count > 1)
        for (int c = 0; c < ch->count; ++c) {
            const int kc = k - c * ch->size < ch->size ? k - c * ch->size : ch->size;
            if (kc < 1 || !x3w_chunk_built(x3w_chunk_nkb(kc))) return false;
        }
    return true;
}

// The chunks of x3w_chunks (the single-bag driver's rule, so a packed bag's P and lse are those of its own launch bit for bit) and the
// table at the chunk size.  One table serves every chunk (a bag's tile geometry depends on n and h only); descriptor word 3 stays
// b * k with the FULL key count.
struct X3WVarlen {
    X3Chunks ch;
    X3VarlenPlan vp;           // geometry at the LARGEST chunk's key-block count (sizes the partial tiles)
    size_t partial_bytes, stats_bytes;
};
bool x3w_varlen_plan(const int64_t* offsets, int bags, int k, int h, X3WVarlen* vc, int32_t* table, size_t table_ints) {
    if (bags < 1 || h < 1 || !x3w_chunks_built(k, &vc->ch)) return false;
    const int size = vc->ch.size;
    if (!snf_attn::make_varlen_table(offsets, bags, k, &vc->vp, table, table_ints,
                                     [&](int64_t n, X3Plan* pl) { return x3w_plan(n, size, h, pl, true); }))
        return false;
    vc->partial_bytes = (size_t)vc->vp.partial_slots * (size_t)(vc->vp.nkb * NCB) * 1024 * sizeof(float);
    vc->stats_bytes = vc->ch.count > 1 ? (size_t)vc->ch.count * h * (size_t)offsets[bags] * sizeof(f32x2) : 0;
    return true;
}

}  // namespace

extern "C" {

size_t snf_sparse_attn_fwd_x3_dk192_workspace_bytes(int64_t n, int k, int h) {
    X3Plan pl;
    X3Chunks ch;
    if (h < 1 || n < 1 || !x3w_chunks_built(k, &ch) || !x3w_plan(n, ch.size, h, &pl)) return 0;
    const size_t stats = ch.count > 1 ? (size_t)ch.count * h * n * sizeof(f32x2) : 0;
    return x3w_workspace(pl) + stats;
}

// q, v [n, ld] f32, kp [k, h * 192] f32, out [k, h * 192], attn [h, n, k] / lse [h, n] or null
int snf_sparse_attn_fwd_x3_dk192(const float* q, int64_t ldq, const float* v, int64_t ldv, const float* kp, int64_t n, int k, int h,
                                 float scale, float* out, float* attn, float* lse, void* workspace, size_t workspace_bytes,
                                 snf_stream_t stream) {
    SNF_REQUIRE(q && v && kp && out, "snf_sparse_attn_fwd_x3_dk192: null pointer");
    SNF_REQUIRE(n >= 1 && k >= 1 && h >= 1, "snf_sparse_attn_fwd_x3_dk192: bad shape");
    X3Plan pl;
    X3Chunks ch;
    if (!x3w_chunks_built(k, &ch) || !x3w_plan(n, ch.size, h, &pl)) {
        snf::set_error("snf_sparse_attn_fwd_x3_dk192: unsupported shape k=%d (k <= %d x %d)", k, X3W_MAX_CHUNKS, X3W_KMAX);
        return SNF_EUNSUPPORTED;
    }
    const int64_t d = (int64_t)h * DK;
    SNF_REQUIRE(ldq >= d && ldv >= d && (ldq % 4) == 0 && (ldv % 4) == 0, "snf_sparse_attn_fwd_x3_dk192: ldq=%lld / ldv=%lld must be >= "
                "h*192 and keep rows 16-byte aligned", (long long)ldq, (long long)ldv);
    SNF_REQUIRE(((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(v) | reinterpret_cast<uintptr_t>(kp)) & 15) == 0,
                "snf_sparse_attn_fwd_x3_dk192: q / v / kp must be 16-byte aligned");
    const size_t part_bytes = x3w_workspace(pl);
    const size_t need = part_bytes + (ch.count > 1 ? (size_t)ch.count * h * n * sizeof(f32x2) : 0);
    if (!workspace || workspace_bytes < need) {
        snf::set_error("snf_sparse_attn_fwd_x3_dk192: workspace %zu < %zu", workspace_bytes, need);
        return SNF_EWORKSPACE;
    }
    X3Params P;
    P.q = q, P.v = v, P.kp = kp;
    P.n = n, P.ldq = ldq, P.ldv = ldv, P.ldkp = d;
    P.k = k, P.h = h, P.scale = scale;
    P.attn = attn, P.attn_ld = k, P.lse = lse;
    P.partial = reinterpret_cast<float*>(workspace);
    P.stats = reinterpret_cast<f32x2*>(reinterpret_cast<unsigned char*>(workspace) + part_bytes);
    P.nchunks = ch.count, P.chunk = 0;
    P.tiles_per_head = pl.tiles_per_head, P.tiles_per_wg = pl.tiles_per_wg, P.total_tiles = pl.total_tiles;
    P.seg_count = pl.seg_count;
    P.n_stride = n, P.vl = nullptr, P.vl_bags = 0, P.out_direct = nullptr;
    hipStream_t s = snf::as_stream(stream);
    if (ch.count == 1) return x3w_dispatch<false>(P, pl, out, s);
    // key chunks: statistics of every chunk first, then the chunks' main passes with the softmax exact over all keys
    for (int pass = 1; pass <= 2; ++pass)
        for (int c = 0; c < ch.count; ++c) {
            const int k0 = c * ch.size, kc = k - k0 < ch.size ? k - k0 : ch.size;
            X3Params C = P;
            C.kp = kp + (int64_t)k0 * d;
            C.k = kc, C.chunk = c;
            C.attn = (pass == 2 && attn) ? attn + k0 : nullptr;
            C.lse = (pass == 2 && c == 0) ? lse : nullptr;
            X3Plan cpl = pl;
            cpl.nkb = x3w_chunk_nkb(kc);   // the chunk's own key-block count, as in the varlen form
            int rc = snf::x3_dk192_launch_chunk(pass, C, cpl, out + (int64_t)k0 * d, s);
            if (rc) return rc;
        }
    return SNF_OK;
}

// ---- varlen (see snf_sparse_attn_varlen_plan in sparse_attn_mfma.hip for the protocol) ----
int snf_sparse_attn_x3_varlen_dk192_plan(const int64_t* offsets, int bags, int k, int h, int32_t* table, size_t table_ints,
                                         size_t* table_ints_needed, size_t* workspace_bytes, int* n_chunks, int* chunk_k) {
    SNF_REQUIRE(offsets && bags >= 1 && h >= 1, "snf_sparse_attn_x3_varlen_dk192_plan: bad arguments");
    X3WVarlen vc;
    if (!x3w_varlen_plan(offsets, bags, k, h, &vc, nullptr, 0)) {
        snf::set_error("snf_sparse_attn_x3_varlen_dk192_plan: unsupported shape (bags=%d k=%d: need 1 <= k <= %d = %d chunks of %d, "
                       "non-empty bags)", bags, k, X3W_MAX_CHUNKS * X3W_KMAX, X3W_MAX_CHUNKS, X3W_KMAX);
        return SNF_EUNSUPPORTED;
    }
    const size_t need = (size_t)VL_DESC * bags + (size_t)vc.vp.total_wg;
    if (table_ints_needed) *table_ints_needed = need;
    if (workspace_bytes) *workspace_bytes = vc.partial_bytes + vc.stats_bytes;
    if (n_chunks) *n_chunks = vc.ch.count;
    if (chunk_k) *chunk_k = vc.ch.size;
    if (table) {
        SNF_REQUIRE(table_ints >= need, "snf_sparse_attn_x3_varlen_dk192_plan: table %zu < %zu ints", table_ints, need);
        x3w_varlen_plan(offsets, bags, k, h, &vc, table, table_ints);
    }
    return SNF_OK;
}

// q, v [T, ld] f32 packed rows, kp [bags * k, h * 192] f32, out [bags * k, h * 192], attn [h, T, k] / lse [h, T] or null;
// table_dev / workspace from snf_sparse_attn_x3_varlen_dk192_plan
int snf_sparse_attn_fwd_x3_varlen_dk192(const float* q, int64_t ldq, const float* v, int64_t ldv, const float* kp,
                                        const int64_t* offsets, int bags, int k, int h, float scale, float* out, float* attn,
                                        float* lse, const int32_t* table_dev, void* workspace, size_t workspace_bytes,
                                        snf_stream_t stream) {
    SNF_REQUIRE(q && v && kp && out && offsets && table_dev, "snf_sparse_attn_fwd_x3_varlen_dk192: null pointer");
    SNF_REQUIRE(bags >= 1 && h >= 1, "snf_sparse_attn_fwd_x3_varlen_dk192: bad shape");
    X3WVarlen vc;
    if (!x3w_varlen_plan(offsets, bags, k, h, &vc, nullptr, 0)) {
        snf::set_error("snf_sparse_attn_fwd_x3_varlen_dk192: unsupported shape (bags=%d k=%d)", bags, k);
        return SNF_EUNSUPPORTED;
    }
    const int64_t d = (int64_t)h * DK, total = offsets[bags];
    SNF_REQUIRE(ldq >= d && ldv >= d && (ldq % 4) == 0 && (ldv % 4) == 0, "snf_sparse_attn_fwd_x3_varlen_dk192: ldq=%lld / ldv=%lld "
                "must be >= h*192 and keep rows 16-byte aligned", (long long)ldq, (long long)ldv);
    SNF_REQUIRE(((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(v) | reinterpret_cast<uintptr_t>(kp)) & 15) == 0,
                "snf_sparse_attn_fwd_x3_varlen_dk192: q / v / kp must be 16-byte aligned");
    const size_t need = vc.partial_bytes + vc.stats_bytes;
    if (need && (!workspace || workspace_bytes < need)) {
        snf::set_error("snf_sparse_attn_fwd_x3_varlen_dk192: workspace %zu < %zu", workspace_bytes, need);
        return SNF_EWORKSPACE;
    }
    X3Params P;
    P.q = q, P.v = v, P.kp = kp;
    P.n = total, P.ldq = ldq, P.ldv = ldv, P.ldkp = d;
    P.k = k, P.h = h, P.scale = scale;
    P.attn = attn, P.attn_ld = k, P.lse = lse;
    P.partial = reinterpret_cast<float*>(workspace);
    P.stats = reinterpret_cast<f32x2*>(reinterpret_cast<unsigned char*>(workspace) + vc.partial_bytes);   // [count][h][total]
    P.nchunks = vc.ch.count, P.chunk = 0;
    P.tiles_per_head = P.tiles_per_wg = P.total_tiles = P.seg_count = 0;   // per bag, from the table
    P.n_stride = total, P.vl = table_dev, P.vl_bags = bags, P.out_direct = out;
    X3Plan pl;
    pl.num_wg = (int)vc.vp.total_wg, pl.nkb = vc.vp.nkb;
    pl.tiles_per_wg = pl.total_tiles = pl.seg_count = 0;
    pl.tiles_per_head = vc.vp.all_direct ? -1 : 0;   // x3w_launch: -1 = no reduction pass
    hipStream_t s = snf::as_stream(stream);
    if (vc.ch.count == 1) return x3w_dispatch<true>(P, pl, out, s);
    for (int pass = 1; pass <= 2; ++pass)
        for (int c = 0; c < vc.ch.count; ++c) {
            const int k0 = c * vc.ch.size, kc = k - k0 < vc.ch.size ? k - k0 : vc.ch.size;
            pl.nkb = x3w_chunk_nkb(kc);
            // bag b's keys of this chunk: rows b k + k0 .. of Kp and of the output (the descriptor adds b k)
            P.kp = kp + (int64_t)k0 * d;
            P.k = kc, P.chunk = c;
            P.attn = (pass == 2 && attn) ? attn + k0 : nullptr;
            P.lse = (pass == 2 && c == 0) ? lse : nullptr;
            float* out_c = out + (int64_t)k0 * d;
            P.out_direct = out_c;
            int rc = snf::x3_dk192_launch_chunk(pass, P, pl, out_c, s);
            if (rc) return rc;
        }
    return SNF_OK;
}

}  // extern "C"
