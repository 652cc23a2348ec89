// Host driver of the tiled sparse-attention forward, written down once for the bf16 family (sparse_attn_mfma*.hip) and the fp32-class
// family (sparse_attn_x3*.hip), single bag and varlen, one key chunk or many.  Host code only: no kernel, nothing __device__.
//
// An entry point validates what is its own (dtypes, dropout), plans (plan_bag / plan_varlen), words its refusal, and hands the
// operands to forward_bag / forward_varlen with its kernel switch as the `launch` callable.  Everything in which the families differ
// is a member of the family description F (a plain struct, no virtual call, nothing on the heap):
//   using Params, Kp        AttnParams | X3Params; element type of the Kp the kernels read (bf16 bits | float)
//   int dk                  head width
//   chunks(k, Chunks*)      the family's chunk rule (make_chunks | x3_chunks | width_chunks of attn_width.h: they differ on purpose)
//   plan(n, kc, pl, packed) geometry of one launch of kc keys over n rows (packed: a bag inside a varlen launch)
//   built(chunked, nkb)     is a varlen launch at this key-block count instantiated?  64/128: asked of chunked launches only;
//                           bf16 192: asked of a single chunk too
//   ROUND                   bf16 256: the workspace areas start on 256 bytes; fp32-class 1: the areas are packed
//   STAGE_KP                bf16: room for the bf16 copy of an f32 Kp behind the statistics; fp32-class reads Kp as given
//   OFFSETS32               bf16: the kernels form rows * pitch in 32 bits, so the driver checks it; fp32-class does not check
//   BAG_NKB_OF_LARGEST      fp32-class 64/128, single bag: every chunk launches at the key-block count of the largest chunk; all
//                           other drivers launch a chunk at its own count
//   DK_TEXT                 how the pitch refusal names the width ("dk", or "192" at the fp32-class entry points of that width)
//   kp(...)                 bf16: rounds an f32 Kp into the staging area; fp32-class: the pointer itself
//   chunk(P, ...)           the per-chunk fields only this Params has (bf16: key0, stats / stats_out; fp32-class: chunk, stats)
// Both families keep one (max, sum) float pair per row, head and chunk.  Of a single bag the statistics area is not rounded (it
// is the last but for the staging area, which rounds itself); of a varlen launch it is rounded to ROUND.
#pragma once
#include "attn_plan.h"

namespace snf_attn {

struct Chunks {
    int count, size;   // chunk c covers keys [c * size, min(k, (c + 1) * size))
};

// ---- operand checks: `me` is the entry point's name ----------------------------------------------------------------------------------
inline int require(const char* me, bool ok, const char* what) {   // what: "null pointer", "bad shape", "bad arguments"
    if (ok) return SNF_OK;
    snf::set_error("%s: %s", me, what);
    return SNF_EINVAL;
}
// rows hold all heads and start on 16 bytes: align = 4 elements for f32 rows, 8 for bf16
inline int require_pitch(const char* me, int64_t ldq, int64_t ldv, int64_t d, int align, const char* dk_text) {
    if (ldq >= d && ldv >= d && (ldq % align) == 0 && (ldv % align) == 0) return SNF_OK;
    snf::set_error("%s: ldq=%lld / ldv=%lld must be >= h*%s and keep rows 16-byte aligned", me, (long long)ldq, (long long)ldv, dk_text);
    return SNF_EINVAL;
}
inline int require_base16(const char* me, const void* q, const void* v, const void* kp) {
    if (((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(v) | reinterpret_cast<uintptr_t>(kp)) & 15) == 0) return SNF_OK;
    snf::set_error("%s: q / v / kp must be 16-byte aligned", me);
    return SNF_EINVAL;
}
// rows = the rows of the bag (varlen: of the longest bag)
inline int require_offsets32(const char* me, int64_t rows, int64_t ldq, int64_t ldv, bool varlen) {
    const int64_t elems = rows * (ldq > ldv ? ldq : ldv);
    if (ldq < (1 << 24) && ldv < (1 << 24) && elems < 0x7fffffffll) return SNF_OK;
    if (varlen) snf::set_error("%s: bag rows * row pitch exceeds the 32-bit offsets of the kernel", me);
    else snf::set_error("%s: n * row pitch = %lld elements exceeds the 32-bit offsets of the kernel", me, (long long)elems);
    return SNF_EUNSUPPORTED;
}
inline int require_workspace(const char* me, const void* workspace, size_t bytes, size_t need) {
    if (workspace && bytes >= need) return SNF_OK;
    snf::set_error("%s: workspace %zu < %zu", me, bytes, need);
    return SNF_EWORKSPACE;
}

// ---- plans: chunks, geometry at the LARGEST chunk's key-block count, and the workspace carve partials | statistics | bf16 Kp ---------
inline size_t round_up(size_t bytes, size_t to) { return (bytes + to - 1) / to * to; }
inline size_t partial_tile_bytes(int64_t slots, int nkb, int dk) { return (size_t)slots * (size_t)(nkb * (dk / 32)) * 1024 * sizeof(float); }
constexpr size_t STATS_PAIR = 2 * sizeof(float);

struct BagLaunch {
    Chunks chunks;
    TilePlan pl;
    size_t partial_bytes, stats_bytes, staging_bytes;
};
template <class F>
bool plan_bag(const F& f, int64_t n, int k, int h, BagLaunch* b) {
    if (!f.chunks(k, &b->chunks) || !f.plan(n, b->chunks.size, &b->pl, false)) return false;
    b->partial_bytes = round_up(partial_tile_bytes((int64_t)b->pl.num_wg * b->pl.seg_count, b->pl.nkb, f.dk), F::ROUND);
    b->stats_bytes = b->chunks.count > 1 ? (size_t)b->chunks.count * h * n * STATS_PAIR : 0;
    b->staging_bytes = F::STAGE_KP ? round_up((size_t)k * h * f.dk * 2, 256) : 0;
    return true;
}

struct VarlenLaunch {
    Chunks chunks;
    VarlenPlan vp;
    size_t partial_bytes, stats_bytes, staging_bytes;
};
// One table serves every chunk (a bag's tile geometry depends on n and h only); descriptor word 3 (first Kp / output row of bag b)
// stays b * k with the FULL key count: the chunk loop offsets the pointers.  The plan is the one refusal point: every chunk's
// key-block count is one the launches are built for.  max_chunks = 1: the single-chunk entry points keep refusing more.
template <class F>
bool plan_varlen(const F& f, const int64_t* offsets, int bags, int k, int h, int max_chunks, VarlenLaunch* vl, int32_t* table,
                 size_t table_ints) {
    if (bags < 1 || !f.chunks(k, &vl->chunks) || vl->chunks.count > max_chunks) return false;
    const Chunks ch = vl->chunks;
    for (int c = 0; c < ch.count; ++c) {
        const int kc = k - c * ch.size < ch.size ? k - c * ch.size : ch.size;
        TilePlan one;
        if (kc < 1 || !f.plan(1, kc, &one, true) || !f.built(ch.count > 1, one.nkb)) return false;
    }
    if (!make_varlen_table(offsets, bags, k, &vl->vp, table, table_ints, [&](int64_t n, TilePlan* pl) { return f.plan(n, ch.size, pl, true); }))
        return false;
    vl->partial_bytes = round_up(partial_tile_bytes(vl->vp.partial_slots, vl->vp.nkb, f.dk), F::ROUND);
    vl->stats_bytes = ch.count > 1 ? round_up((size_t)ch.count * h * (size_t)offsets[bags] * STATS_PAIR, F::ROUND) : 0;
    vl->staging_bytes = F::STAGE_KP ? round_up((size_t)(k * bags) * h * f.dk * 2, 256) : 0;
    return true;
}

// The sizing reply of the *_plan entry points: sizes first (table null), then the same call fills the table.  refuse() words the
// entry point's refusal; n_chunks / chunk_k may be null.
template <class F, class Refuse>
int varlen_plan_reply(const char* me, const F& f, const int64_t* offsets, int bags, int k, int h, int max_chunks, int32_t* table,
                      size_t table_ints, size_t* table_ints_needed, size_t* workspace_bytes, int* n_chunks, int* chunk_k, Refuse refuse) {
    VarlenLaunch vl;
    if (!plan_varlen(f, offsets, bags, k, h, max_chunks, &vl, nullptr, 0)) {
        refuse();
        return SNF_EUNSUPPORTED;
    }
    const size_t need = (size_t)VL_DESC * bags + (size_t)vl.vp.total_wg;
    if (table_ints_needed) *table_ints_needed = need;
    if (workspace_bytes) *workspace_bytes = vl.partial_bytes + vl.stats_bytes + vl.staging_bytes;
    if (n_chunks) *n_chunks = vl.chunks.count;
    if (chunk_k) *chunk_k = vl.chunks.size;
    if (table) {
        SNF_REQUIRE(table_ints >= need, "%s: table %zu < %zu ints", me, table_ints, need);
        plan_varlen(f, offsets, bags, k, h, max_chunks, &vl, table, table_ints);
    }
    return SNF_OK;
}

// ---- the launch ------------------------------------------------------------------------------------------------------------------------
template <class Q, class KpIn>
struct Operands {
    const Q *q, *v;
    int64_t ldq, ldv;
    int row_align;       // elements per 16 bytes of a Q | V row
    const KpIn* kp;
    bool kp_f32;         // bf16 family: Kp arrives as f32 and is staged
    int k, h;
    float scale;
    float *out, *attn, *lse;
    void* workspace;
    size_t workspace_bytes;
    hipStream_t stream;
};

// Param fillers: the fields both structs have (the family's own ones are set by the entry point and by F::chunk)
template <class P, class O>
void fill_shared(P& p, const O& o, int64_t rows, int dk) {
    p.q = o.q, p.v = o.v;
    p.n = rows, p.ldq = o.ldq, p.ldv = o.ldv, p.ldkp = (int64_t)o.h * dk;
    p.k = o.k, p.h = o.h, p.scale = o.scale;
    p.attn_ld = o.k;
    p.partial = reinterpret_cast<float*>(o.workspace);
    p.n_stride = rows;
}
template <class P, class O>
void fill_bag(P& p, const O& o, int64_t n, int dk, const TilePlan& pl) {
    fill_shared(p, o, n, dk);
    p.tiles_per_head = pl.tiles_per_head, p.tiles_per_wg = pl.tiles_per_wg, p.total_tiles = pl.total_tiles, p.seg_count = pl.seg_count;
    p.vl = nullptr, p.vl_bags = 0, p.out_direct = nullptr;
}
template <class P, class O>
void fill_varlen(P& p, const O& o, int64_t total, int dk, const int32_t* table_dev, int bags) {
    fill_shared(p, o, total, dk);
    p.tiles_per_head = p.tiles_per_wg = p.total_tiles = p.seg_count = 0;   // per bag, from the table
    p.vl = table_dev, p.vl_bags = bags;                                   // out_direct: per chunk, below
}
inline TilePlan varlen_tile_plan(const VarlenPlan& vp) {
    TilePlan pl;
    pl.num_wg = (int)vp.total_wg, pl.nkb = vp.nkb;
    pl.tiles_per_wg = pl.total_tiles = pl.seg_count = 0;
    pl.tiles_per_head = vp.all_direct ? -1 : 0;   // the launch templates: -1 = every bag stores its own heads, no reduction pass
    return pl;
}

// The pass-by-chunk loop.  One chunk: its forward alone.  More: the statistics of every chunk, then the chunks' main passes, which
// normalise over all chunks; lse is written at chunk 0.  main_size is the chunk length of the MAIN passes: the bf16 single-bag
// driver rounds it up to a multiple of 4 under dropout (one Philox call covers 4 keys), every other driver passes ch.size.
// launch(stats_pass, P, pl, out_c) is the family's kernel switch.
template <class F, class O, class Launch>
int run_chunks(const F& f, typename F::Params& P, const Chunks& ch, int main_size, TilePlan pl, bool varlen, const O& o, int64_t kp_elems,
               size_t partial_bytes, size_t stats_bytes, Launch launch) {
    unsigned char* ws = reinterpret_cast<unsigned char*>(o.workspace);
    const typename F::Kp* kp;
    if (int rc = F::kp(o.kp, o.kp_f32, kp_elems, ws + partial_bytes + stats_bytes, o.stream, &kp)) return rc;
    const int64_t d = P.ldkp;
    for (int pass = ch.count > 1 ? 0 : 1; pass < 2; ++pass)
        for (int c = 0; c < ch.count; ++c) {
            const int size = pass ? main_size : ch.size;
            const int k0 = c * size, kc = o.k - k0 < size ? o.k - k0 : size;
            if (varlen || !F::BAG_NKB_OF_LARGEST) {
                TilePlan one;
                if (!f.plan(1, kc, &one, varlen)) return SNF_EUNSUPPORTED;
                pl.nkb = one.nkb;
            }
            // keys k0 .. k0 + kc - 1: rows k0 .. of Kp and of the output (varlen: of every bag; the descriptor adds b k)
            P.kp = kp + (int64_t)k0 * d;
            P.k = kc;
            P.attn = (pass && o.attn) ? o.attn + k0 : nullptr;
            P.lse = (pass && c == 0) ? o.lse : nullptr;
            float* out_c = o.out + (int64_t)k0 * d;
            if (varlen) P.out_direct = out_c;
            F::chunk(P, pass == 0, c, k0, ch.count, ws + partial_bytes);
            if (int rc = launch(pass == 0, P, pl, out_c)) return rc;
        }
    return SNF_OK;
}

template <class F, class O>
int check_operands(const char* me, const O& o, int64_t d, size_t need) {
    if (int rc = require_pitch(me, o.ldq, o.ldv, d, o.row_align, F::DK_TEXT)) return rc;
    if (int rc = require_base16(me, o.q, o.v, o.kp)) return rc;
    return require_workspace(me, o.workspace, o.workspace_bytes, need);
}

// P arrives with the family's own launch-wide fields set (bf16: drop, trace)
template <class F, class O, class Launch>
int forward_bag(const char* me, const F& f, const BagLaunch& b, const O& o, int64_t n, int main_size, typename F::Params& P, Launch launch) {
    if (F::OFFSETS32)
        if (int rc = require_offsets32(me, n, o.ldq, o.ldv, false)) return rc;
    if (int rc = check_operands<F>(me, o, (int64_t)o.h * f.dk, b.partial_bytes + b.stats_bytes + (o.kp_f32 ? b.staging_bytes : 0))) return rc;
    fill_bag(P, o, n, f.dk, b.pl);
    return run_chunks(f, P, b.chunks, main_size, b.pl, false, o, (int64_t)o.k * o.h * f.dk, b.partial_bytes, b.stats_bytes, launch);
}
template <class F, class O, class Launch>
int forward_varlen(const char* me, const F& f, const VarlenLaunch& vl, const O& o, const int64_t* offsets, int bags, const int32_t* table_dev,
                   typename F::Params& P, Launch launch) {
    if (F::OFFSETS32) {
        int64_t nmax = 0;
        for (int b = 0; b < bags; ++b) nmax = offsets[b + 1] - offsets[b] > nmax ? offsets[b + 1] - offsets[b] : nmax;
        if (int rc = require_offsets32(me, nmax, o.ldq, o.ldv, true)) return rc;
    }
    if (int rc = check_operands<F>(me, o, (int64_t)o.h * f.dk, vl.partial_bytes + vl.stats_bytes + (o.kp_f32 ? vl.staging_bytes : 0))) return rc;
    fill_varlen(P, o, offsets[bags], f.dk, table_dev, bags);
    return run_chunks(f, P, vl.chunks, vl.chunks.size, varlen_tile_plan(vl.vp), true, o, (int64_t)o.k * bags * o.h * f.dk, vl.partial_bytes,
                      vl.stats_bytes, launch);
}

}  // namespace snf_attn
