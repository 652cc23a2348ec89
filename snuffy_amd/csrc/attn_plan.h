// Launch geometry shared by the tiled sparse-attention families at every head width (bf16: sparse_attn_mfma_impl.h at dk = 64 / 128 / 192;
// fp32-class: sparse_attn_x3_impl.h at 64 / 128, sparse_attn_x3_dk192_impl.h at 192; the fragment-image form sparse_attn_x3p plans for
// itself): how the (head, row-tile) work items of a bag are cut into workgroups, and the descriptor table of a varlen (many bags)
// launch.  The host driver built on it -- chunks, workspace carve, operand checks, the pass-by-chunk loop -- is attn_drive.h.
#pragma once
#include "common.h"

namespace snf_attn {

// row pitch (bytes) of a bf16 P image in LDS: 64 bytes per key block, an ODD number of 64-byte units (bank rule of the transpose-read)
constexpr int p_row_bytes(int nkb) { return 64 * (nkb | 1); }

struct TilePlan {
    int num_wg, tiles_per_head, tiles_per_wg, total_tiles, seg_count, nkb;
};

// Everything of a plan but the key-block count: tiles of `tile_rows` query rows, one persistent workgroup per CU walking a contiguous
// range of (head, row-tile) items.  False: more than 2^31 - 1 tiles.
// A bag inside a PACKED (varlen) launch does not have the chip to itself: at least `small_bag_tiles` tiles (1024 rows) per
// workgroup, so a head of a small bag is one or two partial tiles instead of one per tile -- the partial tiles are the
// bulk of such a launch's bytes (measured, bf16: 64 bags x 1000 rows, 87 -> 54 us + reduction 40 -> 29 us).  A bag launched ALONE
// keeps one tile per workgroup: its tiles run side by side on idle CUs (8 in a row cost it ~25 us of latency, measured).
inline bool make_tile_plan(int64_t n, int h, int tile_rows, int64_t small_bag_tiles, bool packed, TilePlan* pl) {
    const int64_t tph = (n + tile_rows - 1) / tile_rows, total = tph * h;
    if (total > 0x7fffffff) return false;
    const int cus = snf::cu_count();
    int64_t num_wg = total < cus ? total : cus;
    int64_t tpw = (total + num_wg - 1) / num_wg;
    if (packed && total <= cus) tpw = tph < small_bag_tiles ? tph : small_bag_tiles;
    num_wg = (total + tpw - 1) / tpw;
    pl->num_wg = (int)num_wg;
    pl->tiles_per_head = (int)tph;
    pl->tiles_per_wg = (int)tpw;
    pl->total_tiles = (int)total;
    pl->seg_count = (int)((tpw + tph - 1) / tph + 1);
    return true;
}

// Varlen launch (many bags in one grid, single key chunk).  The grid is the concatenation of per-bag grids: every bag keeps a plan of
// its own (the family's planner with packed = true, a function of the bag's length only) and workgroup wg0 + i does what workgroup i
// of a launch of that bag alone would do (same tiles, same partial tiles, same summation order in the reduction) -- a bag's result
// does not depend on what it is packed with, bit for bit.  Against the single-bag entry points (latency plan: one tile per workgroup
// for small bags) only the fp32 summation order of the partial tiles can differ.
// Descriptor of bag b, VL_DESC ints: d[0] wg0 (first workgroup), d[1] row0 (first Q / V row), d[2] n, d[3] out_row0 (= first Kp /
// output row, b k), d[4] tiles_per_head, d[5] tiles_per_wg, d[6] total_tiles, d[7] seg_count, d[8] part0 (first partial slot),
// d[9] num_wg, d[10] direct (tiles_per_wg == tiles_per_head: workgroup i of the bag is head i, whole), d[11] 0.
constexpr int VL_DESC = 12;
struct VarlenPlan {
    int64_t total_wg, partial_slots;   // workgroups of the whole launch; partial tile slots (num_wg * seg_count summed)
    int nkb;
    bool all_direct;                   // every bag has one workgroup per head: no reduction pass at all
};
// table (host memory, may be null to size it) = [bags][VL_DESC] descriptors, then the bag index of every workgroup.
// plan_bag(n, &plan) is the family's per-bag planner (packed form).
template <typename PlanBag>
inline bool make_varlen_table(const int64_t* offsets, int bags, int k, VarlenPlan* vp, int32_t* table, size_t table_ints,
                              PlanBag plan_bag) {
    vp->total_wg = 0, vp->partial_slots = 0, vp->nkb = 0, vp->all_direct = true;
    for (int b = 0; b < bags; ++b) {
        const int64_t n = offsets[b + 1] - offsets[b];
        TilePlan pl;
        if (n < 1 || offsets[b] > 0x7fffffffll || !plan_bag(n, &pl)) return false;
        const bool direct = pl.tiles_per_wg == pl.tiles_per_head;
        vp->all_direct = vp->all_direct && direct;
        if (table) {
            if ((size_t)(VL_DESC * bags) + (size_t)(vp->total_wg + pl.num_wg) > table_ints) return false;
            int32_t* d = table + (size_t)VL_DESC * b;
            d[0] = (int32_t)vp->total_wg, d[1] = (int32_t)offsets[b], d[2] = (int32_t)n, d[3] = b * k;
            d[4] = pl.tiles_per_head, d[5] = pl.tiles_per_wg, d[6] = pl.total_tiles, d[7] = pl.seg_count;
            d[8] = (int32_t)vp->partial_slots, d[9] = pl.num_wg, d[10] = direct ? 1 : 0, d[11] = 0;
            for (int i = 0; i < pl.num_wg; ++i) table[(size_t)VL_DESC * bags + vp->total_wg + i] = b;
        }
        vp->total_wg += pl.num_wg;
        vp->partial_slots += (int64_t)pl.num_wg * pl.seg_count;
        vp->nkb = pl.nkb;
        if (vp->total_wg > 0x3fffffff || vp->partial_slots > 0x3fffffff) return false;
    }
    return bags >= 1;
}

}  // namespace snf_attn
