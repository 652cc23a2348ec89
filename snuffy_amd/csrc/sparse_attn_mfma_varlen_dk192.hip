// K7 (fast form), translation unit 8: every varlen (many bags per launch) form at dk = 192 -- the forward at 1, 2, 4 key blocks, its
// key-chunked forms at 2, 4 key blocks and the statistics pass -- with the two C entry points of the width (see sparse_attn_mfma_impl.h).
// The kernels are sparse_attn_mfma_kernel<192, NKB, bf16, AUX, EXT, 8, VL = true> / sparse_attn_stats_kernel<192, NKB, bf16, VL = true>
// under names of their own: the varlen plan functions of dk = 64 / 128 keep refusing this width, and the single-bag kernels of dk = 192
// keep their symbols (and the counts tests/test_attn_dk192_host.py holds them to) to themselves.
#define SNF_ATTN_MFMA_KERNEL sparse_attn_mfma_vl192_kernel
#define SNF_ATTN_STATS_KERNEL sparse_attn_stats_vl192_kernel
#include "sparse_attn_mfma_impl.h"

namespace {

constexpr int DK = 192, NCB = DK / 32;
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

// The chunks of make_chunks (the single-bag driver's rule: a packed bag's P and lse are those of its own launch bit for bit) and the
// table at the chunk size.  One table serves every chunk; descriptor word 3 stays b * k with the FULL key count.
struct Vl192Plan {
    ChunkPlan cp;
    VarlenPlan vp;             // geometry at the LARGEST chunk's key-block count (sizes the partial tiles)
    size_t partial_bytes, stats_bytes, staging_bytes;
};
bool vl192_plan(const int64_t* offsets, int bags, int k, int h, Vl192Plan* vc, int32_t* table, size_t table_ints) {
    if (bags < 1 || !make_chunks(k, DK, &vc->cp)) return false;
    const int ck = vc->cp.chunk_k;
    for (int c = 0; c < vc->cp.n_chunks; ++c) {   // the plan is the one refusal point: every chunk's key-block count is a built one
        const int kc = k - c * ck < ck ? k - c * ck : ck;
        Plan one;
        if (kc < 1 || !make_plan_any(1, kc, h, DK, &one, true) || !vl192_built(vc->cp.n_chunks > 1, one.nkb)) return false;
    }
    if (!snf_attn::make_varlen_table(offsets, bags, k, &vc->vp, table, table_ints,
                                     [&](int64_t n, Plan* pl) { return make_plan_any(n, ck, h, DK, pl, true); }))
        return false;
    vc->partial_bytes = ((size_t)vc->vp.partial_slots * (size_t)(vc->vp.nkb * NCB) * 1024 * sizeof(float) + 255) / 256 * 256;
    vc->stats_bytes = vc->cp.n_chunks > 1 ? ((size_t)vc->cp.n_chunks * h * (size_t)offsets[bags] * 2 * sizeof(float) + 255) / 256 * 256 : 0;
    vc->staging_bytes = kp_staging_bytes(k * bags, h, DK);
    return true;
}

}  // namespace

extern "C" {

int snf_sparse_attn_varlen_dk192_plan(const int64_t* offsets, int bags, int k, int h, int32_t* table, size_t table_ints,
                                      size_t* table_ints_needed, size_t* workspace_bytes, int* n_chunks, int* chunk_k) {
    SNF_REQUIRE(offsets && bags >= 1 && k >= 1 && h >= 1, "snf_sparse_attn_varlen_dk192_plan: bad arguments");
    Vl192Plan vc;
    if (!vl192_plan(offsets, bags, k, h, &vc, nullptr, 0)) {
        snf::set_error("snf_sparse_attn_varlen_dk192_plan: unsupported shape (bags=%d k=%d: need k <= %d = %d chunks of %d, non-empty "
                       "bags)", bags, k, MAX_CHUNKS * attn_kmax(DK), MAX_CHUNKS, attn_kmax(DK));
        return SNF_EUNSUPPORTED;
    }
    const size_t need = (size_t)snf_attn::VL_DESC * bags + (size_t)vc.vp.total_wg;
    if (table_ints_needed) *table_ints_needed = need;
    if (workspace_bytes) *workspace_bytes = vc.partial_bytes + vc.stats_bytes + vc.staging_bytes;
    if (n_chunks) *n_chunks = vc.cp.n_chunks;
    if (chunk_k) *chunk_k = vc.cp.chunk_k;
    if (table) {
        SNF_REQUIRE(table_ints >= need, "snf_sparse_attn_varlen_dk192_plan: table %zu < %zu ints", table_ints, need);
        vl192_plan(offsets, bags, k, h, &vc, table, table_ints);
    }
    return SNF_OK;
}

// layouts as snf_sparse_attn_fwd_mfma_varlen at dk = 192; table_dev / workspace from snf_sparse_attn_varlen_dk192_plan
int snf_sparse_attn_fwd_mfma_varlen_dk192(const void* q, int64_t ldq, const void* v, int64_t ldv, const void* kp, int kp_dtype,
                                          const int64_t* offsets, int bags, int k, int h, float scale, float* out, float* attn,
                                          float* lse, const int32_t* table_dev, void* workspace, size_t workspace_bytes,
                                          snf_stream_t stream) {
    SNF_REQUIRE(q && v && kp && out && offsets && table_dev, "snf_sparse_attn_fwd_mfma_varlen_dk192: null pointer");
    SNF_REQUIRE(kp_dtype == SNF_DT_F32 || kp_dtype == SNF_DT_BF16, "snf_sparse_attn_fwd_mfma_varlen_dk192: bad kp dtype %d", kp_dtype);
    SNF_REQUIRE(k >= 1 && h >= 1, "snf_sparse_attn_fwd_mfma_varlen_dk192: bad shape");
    Vl192Plan vc;
    if (!vl192_plan(offsets, bags, k, h, &vc, nullptr, 0)) {
        snf::set_error("snf_sparse_attn_fwd_mfma_varlen_dk192: unsupported shape (bags=%d k=%d)", bags, k);
        return SNF_EUNSUPPORTED;
    }
    const int64_t d = (int64_t)h * DK, total = offsets[bags];
    int64_t nmax = 0;
    for (int b = 0; b < bags; ++b) nmax = offsets[b + 1] - offsets[b] > nmax ? offsets[b + 1] - offsets[b] : nmax;
    if (ldq >= (1 << 24) || ldv >= (1 << 24) || nmax * (ldq > ldv ? ldq : ldv) >= 0x7fffffffll) {
        snf::set_error("snf_sparse_attn_fwd_mfma_varlen_dk192: bag rows * row pitch exceeds the 32-bit offsets of the kernel");
        return SNF_EUNSUPPORTED;
    }
    SNF_REQUIRE(ldq >= d && ldv >= d && (ldq % 8) == 0 && (ldv % 8) == 0,
                "snf_sparse_attn_fwd_mfma_varlen_dk192: ldq=%lld / ldv=%lld must be >= h*dk and keep rows 16-byte aligned",
                (long long)ldq, (long long)ldv);
    SNF_REQUIRE((reinterpret_cast<uintptr_t>(q) & 15) == 0 && (reinterpret_cast<uintptr_t>(v) & 15) == 0 &&
                    (reinterpret_cast<uintptr_t>(kp) & 15) == 0,
                "snf_sparse_attn_fwd_mfma_varlen_dk192: q / v / kp must be 16-byte aligned");
    const size_t need = vc.partial_bytes + vc.stats_bytes + (kp_dtype == SNF_DT_F32 ? vc.staging_bytes : 0);
    if (!workspace || workspace_bytes < need) {
        snf::set_error("snf_sparse_attn_fwd_mfma_varlen_dk192: workspace %zu < %zu", workspace_bytes, need);
        return SNF_EWORKSPACE;
    }
    hipStream_t s = snf::as_stream(stream);
    unsigned char* wsp = reinterpret_cast<unsigned char*>(workspace);
    const unsigned short* kp16 = reinterpret_cast<const unsigned short*>(kp);
    if (kp_dtype == SNF_DT_F32) {
        unsigned short* stage = reinterpret_cast<unsigned short*>(wsp + vc.partial_bytes + vc.stats_bytes);
        const int64_t groups = (int64_t)k * bags * d / 8;
        hipLaunchKernelGGL(kp_to_bf16_kernel, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, s,
                           reinterpret_cast<const float*>(kp), stage, groups);
        int rc = snf::check_launch("kp_to_bf16_kernel");
        if (rc) return rc;
        kp16 = stage;
    }
    const bool chunked = vc.cp.n_chunks > 1;
    float* stats = chunked ? reinterpret_cast<float*>(wsp + vc.partial_bytes) : nullptr;   // [n_chunks][h][total][2]
    AttnParams P;
    P.q = q, P.v = v;
    P.n = total, P.ldq = ldq, P.ldv = ldv, P.ldkp = d;
    P.h = h, P.scale = scale;
    P.attn_ld = k;
    P.n_chunks = vc.cp.n_chunks;
    P.partial = reinterpret_cast<float*>(workspace);
    P.tiles_per_head = P.tiles_per_wg = P.total_tiles = P.seg_count = 0;   // per bag, from the table
    P.trace = nullptr, P.trace_wg = 0;
    P.drop = snf::make_dropout(0.f, 0, 0);
    P.n_stride = total;
    P.vl = table_dev, P.vl_bags = bags;
    Plan pl;
    pl.num_wg = (int)vc.vp.total_wg;
    pl.tiles_per_wg = pl.total_tiles = pl.seg_count = 0;
    pl.tiles_per_head = vc.vp.all_direct ? -1 : 0;   // launch_vl192: -1 = no reduction pass
    // one chunk: the forward alone.  More: every chunk's statistics launch, then every chunk's forward
    for (int pass = chunked ? 0 : 1; pass < 2; ++pass)
        for (int c = 0; c < vc.cp.n_chunks; ++c) {
            const int k0 = c * vc.cp.chunk_k;
            const int kc = (k - k0 < vc.cp.chunk_k) ? k - k0 : vc.cp.chunk_k;
            Plan one;
            if (!make_plan_any(1, kc, h, DK, &one, true)) return SNF_EUNSUPPORTED;   // the chunk's key-block count
            pl.nkb = one.nkb;
            // bag b's keys of this chunk: rows b k + k0 .. of Kp and of the output (the descriptor adds b k)
            P.kp = kp16 + (int64_t)k0 * d;
            P.k = kc, P.key0 = k0;
            float* out_c = out + (int64_t)k0 * d;
            P.out_direct = out_c;
            if (pass == 0) {
                P.attn = nullptr, P.lse = nullptr, P.stats = nullptr;
                P.stats_out = stats + (size_t)c * h * total * 2;
            } else {
                P.attn = attn ? attn + k0 : nullptr;
                P.lse = c == 0 ? lse : nullptr;
                P.stats = stats, P.stats_out = nullptr;
            }
            int rc = launch_nkb_vl192(pass == 0, P, pl, out_c, s);
            if (rc) return rc;
        }
    return SNF_OK;
}

}  // extern "C"
