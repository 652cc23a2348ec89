// Host shell of a "native-width" sparse-attention kernel -- a head width with a kernel template, two translation units and four C
// entry points of its own (fp32-class 192 and 256, bf16 256; the bf16 varlen form at 192 takes the entry bodies only) -- written down
// once.  Host code only: no kernel, nothing __device__.  It sits on attn_drive.h, which holds the chunk loop and the workspace carve.
//
// A width is described by a traits struct W next to its kernel (a plain struct of constants and static functions):
//   Drive                   the family description every width of the family shares (X3Drive | MfmaDrive: attn_drive.h lists its members;
//                           the shell also asks it for In, ROW_ALIGN, open() and reduce<DK, NKB>())
//   DK, ROWS, THREADS       head width, query rows per tile, threads per workgroup
//   KMAX, MAX_CHUNKS        keys per launch, chunks per forward
//   CHUNK_MULTIPLE          chunk sizes are rounded up to it (fp32-class 4, bf16 1)
//   MAX_ROWS                the family's own row limit (bf16: 32-bit element offsets)
//   PACKED_TILES, PACKED_FORCED   tiles per workgroup of a bag inside a packed launch: a floor for small bags (192), or the count
//                           whatever the bag's length (256, where the partial tiles are the bulk of the traffic)
//   lds_bytes(nkb)          dynamic LDS of one instantiation
//   kernel<NKB, AUX, MODE, VL>()   the kernel template
//   launch_chunk(mode, ...) the width's second translation unit (the MODE 1 / MODE 2 instantiations)
//   NAME, KERNEL, DK_TEXT   the names used in messages
// and the wording of its entry points E (Width<W> for a width):
//   plan_args_ok(), varlen_shape_ok()   what the varlen plan calls "bad arguments" and the varlen forward "bad shape"
//   SHORT_TABLE_UNSUPPORTED the varlen plan words the refusal of a short table itself (bf16 256)
//   refuse_bag(), refuse_plan()   the shape refusals
#pragma once
#include "attn_drive.h"

namespace snf_attn {

// ---- geometry --------------------------------------------------------------------------------------------------------------------------
// one launch of kc <= KMAX keys: key blocks 1, 2, 4
template <class W>
bool width_plan(int64_t n, int kc, int h, TilePlan* pl, bool packed) {
    if (kc < 1 || kc > W::KMAX || n < 1 || h < 1 || n > W::MAX_ROWS) return false;
    const int need = (kc + 31) / 32;
    pl->nkb = need <= 1 ? 1 : need <= 2 ? 2 : 4;
    if (!make_tile_plan(n, h, W::ROWS, W::PACKED_TILES, packed, pl)) return false;
    if (packed && W::PACKED_FORCED) {
        const int tph = pl->tiles_per_head, tpw = tph < W::PACKED_TILES ? tph : W::PACKED_TILES;
        pl->tiles_per_wg = tpw;
        pl->num_wg = (pl->total_tiles + tpw - 1) / tpw;
        pl->seg_count = (tpw + tph - 1) / tph + 1;
    }
    return true;
}
// key-block counts the launches are built for: one chunk 1, 2, 4; a chunk of a key-chunked launch 2, 4 (the width's chunk rule leaves
// no chunk of 32 keys or fewer)
constexpr bool width_built(bool chunked, int nkb) { return nkb == 2 || nkb == 4 || (nkb == 1 && !chunked); }
// ceil(k / KMAX) chunks of equal size, every one at a key-block count that is built: the single-bag plan refuses here what the varlen
// plan refuses through built()
template <class W>
bool width_chunks(int k, Chunks* c) {
    if (k < 1 || k > W::MAX_CHUNKS * W::KMAX) return false;
    c->count = (k + W::KMAX - 1) / W::KMAX;
    const int even = (k + c->count - 1) / c->count;
    c->size = c->count == 1 ? k : (even + W::CHUNK_MULTIPLE - 1) / W::CHUNK_MULTIPLE * W::CHUNK_MULTIPLE;
    if (c->size > W::KMAX) return false;
    for (int i = 0; i < c->count; ++i) {
        const int kc = k - i * c->size < c->size ? k - i * c->size : c->size;
        TilePlan one;
        if (kc < 1 || !width_plan<W>(1, kc, 1, &one, true) || !width_built(c->count > 1, one.nkb)) return false;
    }
    return true;
}

// The family description attn_drive.h asks for: the width's chunks for single bag and varlen alike (a packed bag's P and lse are those
// of its own launch bit for bit), every chunk launched at its own key-block count
template <class W>
struct WidthFamily : W::Drive {
    static constexpr bool BAG_NKB_OF_LARGEST = false;
    static constexpr const char* DK_TEXT = W::DK_TEXT;
    static constexpr int dk = W::DK;
    int h;
    bool chunks(int k, Chunks* c) const { return width_chunks<W>(k, c); }
    bool plan(int64_t n, int kc, TilePlan* pl, bool packed) const { return width_plan<W>(n, kc, h, pl, packed); }
    bool built(bool chunked, int nkb) const { return width_built(chunked, nkb); }
};

// ---- launches --------------------------------------------------------------------------------------------------------------------------
// the LDS opt-in, the launch, and the reduction pass unless every bag stored its own heads
template <class W, int NKB, bool AUX, int MODE, bool VL>
int width_launch(const typename W::Drive::Params& P, const TilePlan& pl, float* out, hipStream_t s) {
    constexpr int lds = W::lds_bytes(NKB);
    static_assert(lds <= 160 * 1024, "LDS budget");
    auto kern = W::template kernel<NKB, AUX, MODE, VL>();
    static thread_local unsigned long long attr_set_mask = 0;   // devices (bit = device id) that have the opt-in
    if (int rc = snf::lds_opt_in(reinterpret_cast<const void*>(kern), lds, &attr_set_mask, W::NAME)) return rc;
    hipLaunchKernelGGL(kern, dim3(pl.num_wg), dim3(W::THREADS), lds, s, P);
    int rc = snf::check_launch(W::KERNEL);
    if (rc || MODE == 1) return rc;
    if (VL && P.out_direct && pl.tiles_per_head == -1) return SNF_OK;   // every bag stored its heads itself
    return W::Drive::template reduce<W::DK, NKB>(P, pl, out, VL, s);
}

// one launch holds all keys: the MODE 0 kernels at 1, 2, 4 key blocks (the width's first translation unit)
template <class W, bool VL>
int width_launch_all(const typename W::Drive::Params& P, const TilePlan& pl, float* out, hipStream_t s) {
    const bool aux = P.attn != nullptr || P.lse != nullptr;
    switch (pl.nkb) {
        case 1: return aux ? width_launch<W, 1, true, 0, VL>(P, pl, out, s) : width_launch<W, 1, false, 0, VL>(P, pl, out, s);
        case 2: return aux ? width_launch<W, 2, true, 0, VL>(P, pl, out, s) : width_launch<W, 2, false, 0, VL>(P, pl, out, s);
        case 4: return aux ? width_launch<W, 4, true, 0, VL>(P, pl, out, s) : width_launch<W, 4, false, 0, VL>(P, pl, out, s);
        default: break;
    }
    snf::set_error("%s: key-block count %d not built", W::NAME, pl.nkb);
    return SNF_EUNSUPPORTED;
}

// one chunk's statistics pass (mode 1) or main pass (mode 2) at 2, 4 key blocks, single bag (P.vl null) or varlen: the body of the
// width's *_launch_chunk (its second translation unit)
template <class W, int NKB, bool VL>
int width_chunk_modes(int mode, const typename W::Drive::Params& P, const TilePlan& pl, float* out, hipStream_t s) {
    const bool aux = P.attn != nullptr || P.lse != nullptr;
    if (mode == 1) return width_launch<W, NKB, false, 1, VL>(P, pl, out, s);
    return aux ? width_launch<W, NKB, true, 2, VL>(P, pl, out, s) : width_launch<W, NKB, false, 2, VL>(P, pl, out, s);
}
template <class W>
int width_launch_chunk(int mode, const typename W::Drive::Params& P, const TilePlan& pl, float* out, hipStream_t s) {
    const bool vl = P.vl != nullptr;
    switch (pl.nkb) {
        case 2: return vl ? width_chunk_modes<W, 2, true>(mode, P, pl, out, s) : width_chunk_modes<W, 2, false>(mode, P, pl, out, s);
        case 4: return vl ? width_chunk_modes<W, 4, true>(mode, P, pl, out, s) : width_chunk_modes<W, 4, false>(mode, P, pl, out, s);
        default: break;
    }
    snf::set_error("%s (key chunks): key-block count %d not built", W::NAME, pl.nkb);
    return SNF_EUNSUPPORTED;
}

// The entry description of a width: its wording (W), its family, and its kernel switch -- one chunk: the MODE 0 kernels; more: MODE 1 per
// chunk, then MODE 2
template <class W>
struct Width : W {
    using Family = WidthFamily<W>;
    template <bool VL>
    static int pass(bool chunked, bool stats_pass, const typename Family::Params& P, const TilePlan& pl, float* out, hipStream_t s) {
        if (!chunked) return width_launch_all<W, VL>(P, pl, out, s);
        return W::launch_chunk(stats_pass ? 1 : 2, P, pl, out, s);
    }
};

// ---- the four entry points of an entry description E -------------------------------------------------------------------------------------
// partial tiles | chunk statistics | the family's Kp staging area
template <class E>
size_t entry_workspace_bytes(int64_t n, int k, int h) {
    BagLaunch b;
    return (h >= 1 && n >= 1 && plan_bag(typename E::Family{{}, h}, n, k, h, &b)) ? b.partial_bytes + b.stats_bytes + b.staging_bytes : 0;
}

// q, v [n, ld], kp [k, h * dk], out [k, h * dk] f32, attn [h, n, k] / lse [h, n] or null; kp_dtype: bf16 family only
template <class E>
int entry_forward_bag(const char* me, const typename E::Family::In* q, int64_t ldq, const typename E::Family::In* v, int64_t ldv,
                      const typename E::Family::In* kp, int kp_dtype, int64_t n, int k, int h, float scale, float* out, float* attn,
                      float* lse, void* workspace, size_t workspace_bytes, snf_stream_t stream) {
    using F = typename E::Family;
    if (int rc = require(me, q && v && kp && out, "null pointer")) return rc;
    if (int rc = require(me, n >= 1 && k >= 1 && h >= 1, "bad shape")) return rc;
    typename F::Params P;
    bool kp_f32;
    if (int rc = F::open(me, kp_dtype, P, &kp_f32)) return rc;
    const F f{{}, h};
    BagLaunch b;
    if (!plan_bag(f, n, k, h, &b)) {
        E::refuse_bag(me, n, k);
        return SNF_EUNSUPPORTED;
    }
    const Operands<typename F::In, typename F::In> o{q, v, ldq, ldv, F::ROW_ALIGN, kp, kp_f32, k, h, scale, out, attn, lse, workspace,
                                                     workspace_bytes, snf::as_stream(stream)};
    const bool chunked = b.chunks.count > 1;
    return forward_bag(me, f, b, o, n, b.chunks.size, P, [&](bool stats_pass, typename F::Params& P, const TilePlan& pl, float* out_c) {
        return E::template pass<false>(chunked, stats_pass, P, pl, out_c, o.stream);
    });
}

// ---- varlen (see snf_sparse_attn_varlen_plan in sparse_attn_mfma.hip for the protocol) ----
template <class E>
int entry_varlen_plan(const char* me, const int64_t* offsets, int bags, int k, int h, int32_t* table, size_t table_ints,
                      size_t* table_ints_needed, size_t* workspace_bytes, int* n_chunks, int* chunk_k) {
    if (int rc = require(me, offsets && E::plan_args_ok(bags, k, h), "bad arguments")) return rc;
    const typename E::Family f{{}, h};
    const auto refuse = [&] { E::refuse_plan(me, bags, k, h); };
    if (!E::SHORT_TABLE_UNSUPPORTED)
        return varlen_plan_reply(me, f, offsets, bags, k, h, E::MAX_CHUNKS, table, table_ints, table_ints_needed, workspace_bytes, n_chunks,
                                 chunk_k, refuse);
    // sizes first: a table that is too short is this entry point's own refusal (SNF_EUNSUPPORTED, nothing written)
    size_t need = 0;
    if (int rc = varlen_plan_reply(me, f, offsets, bags, k, h, E::MAX_CHUNKS, nullptr, 0, &need, workspace_bytes, n_chunks, chunk_k, refuse))
        return rc;
    if (table_ints_needed) *table_ints_needed = need;
    if (!table) return SNF_OK;
    if (table_ints < need) {
        snf::set_error("%s: unsupported table of %zu ints (the plan needs %zu)", me, table_ints, need);
        return SNF_EUNSUPPORTED;
    }
    return varlen_plan_reply(me, f, offsets, bags, k, h, E::MAX_CHUNKS, table, table_ints, table_ints_needed, workspace_bytes, n_chunks, chunk_k,
                             refuse);
}

// q, v [T, ld] packed rows, kp [bags * k, h * dk], out [bags * k, h * dk] f32, attn [h, T, k] / lse [h, T] or null; table_dev / workspace
// from the plan entry point
template <class E>
int entry_forward_varlen(const char* me, const typename E::Family::In* q, int64_t ldq, const typename E::Family::In* v, int64_t ldv,
                         const typename E::Family::In* kp, int kp_dtype, const int64_t* offsets, int bags, int k, int h, float scale,
                         float* out, float* attn, float* lse, const int32_t* table_dev, void* workspace, size_t workspace_bytes,
                         snf_stream_t stream) {
    using F = typename E::Family;
    if (int rc = require(me, q && v && kp && out && offsets && table_dev, "null pointer")) return rc;
    typename F::Params P;
    bool kp_f32;
    if (int rc = F::open(me, kp_dtype, P, &kp_f32)) return rc;
    if (int rc = require(me, E::varlen_shape_ok(bags, k, h), "bad shape")) return rc;
    const F f{{}, h};
    VarlenLaunch vl;
    if (!plan_varlen(f, offsets, bags, k, h, E::MAX_CHUNKS, &vl, nullptr, 0)) {
        snf::set_error("%s: unsupported shape (bags=%d k=%d)", me, bags, k);
        return SNF_EUNSUPPORTED;
    }
    const Operands<typename F::In, typename F::In> o{q, v, ldq, ldv, F::ROW_ALIGN, kp, kp_f32, k, h, scale, out, attn, lse, workspace,
                                                     workspace_bytes, snf::as_stream(stream)};
    const bool chunked = vl.chunks.count > 1;
    return forward_varlen(me, f, vl, o, offsets, bags, table_dev, P, [&](bool stats_pass, typename F::Params& P, const TilePlan& pl, float* out_c) {
        return E::template pass<true>(chunked, stats_pass, P, pl, out_c, o.stream);
    });
}

}  // namespace snf_attn
