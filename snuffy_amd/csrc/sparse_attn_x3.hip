// K7 (fp32-class form on the matrix cores): the single-bag and single-chunk varlen variants and the C entry points (the kernels are in
// sparse_attn_x3_impl.h; the key-chunked varlen variants build in sparse_attn_x3_varlen_chunks.hip).
#include "sparse_attn_x3_impl.h"

extern "C" {

size_t snf_sparse_attn_fwd_x3_workspace_bytes(int64_t n, int k, int h, int dk) {
    X3Plan pl;
    X3Chunks ch;
    if (h < 1 || !x3_chunks(k, dk, &ch) || !x3_plan(n, ch.size, h, dk, &pl)) return 0;
    const size_t stats = ch.count > 1 ? (size_t)ch.count * h * n * sizeof(f32x2) : 0;
    return x3_workspace(pl, dk) + stats;
}

static int x3_forward(const float* q, int64_t ldq, const float* v, int64_t ldv, const float* kp, int64_t n, int k, int h, int dk,
                      float scale, float* out, float* attn, float* lse, void* workspace, size_t workspace_bytes, snf_stream_t stream,
                      const snf::DropoutState* drop);

int snf_sparse_attn_fwd_x3(const float* q, int64_t ldq, const float* v, int64_t ldv, const float* kp, int64_t n, int k, int h,
                           int dk, float scale, float* out, float* attn, float* lse, void* workspace, size_t workspace_bytes,
                           snf_stream_t stream) {
    return x3_forward(q, ldq, v, ldv, kp, n, k, h, dk, scale, out, attn, lse, workspace, workspace_bytes, stream, nullptr);
}

int snf_sparse_attn_fwd_x3_dropout(const float* q, int64_t ldq, const float* v, int64_t ldv, const float* kp, int64_t n, int k, int h,
                                   int dk, float scale, float dropout_p, uint64_t seed, uint64_t offset, float* out, float* attn,
                                   float* lse, void* workspace, size_t workspace_bytes, snf_stream_t stream) {
    SNF_REQUIRE(dropout_p >= 0.f && dropout_p < 1.f, "snf_sparse_attn_fwd_x3_dropout: dropout_p=%g outside [0, 1)", (double)dropout_p);
    const snf::DropoutState st = snf::make_dropout(dropout_p, seed, offset);
    return x3_forward(q, ldq, v, ldv, kp, n, k, h, dk, scale, out, attn, lse, workspace, workspace_bytes, stream, st.thresh ? &st : nullptr);
}

static int x3_forward(const float* q, int64_t ldq, const float* v, int64_t ldv, const float* kp, int64_t n, int k, int h, int dk,
                      float scale, float* out, float* attn, float* lse, void* workspace, size_t workspace_bytes, snf_stream_t stream,
                      const snf::DropoutState* drop) {
    SNF_REQUIRE(q && v && kp && out, "snf_sparse_attn_fwd_x3: null pointer");
    SNF_REQUIRE(n >= 1 && k >= 1 && h >= 1, "snf_sparse_attn_fwd_x3: bad shape");
    X3Plan pl;
    X3Chunks ch;
    if (!x3_chunks(k, dk, &ch) || !x3_plan(n, ch.size, h, dk, &pl)) {
        snf::set_error("snf_sparse_attn_fwd_x3: unsupported shape k=%d dk=%d (dk in {64, 128}, k <= 8 x 256 / 8 x 224)", k, dk);
        return SNF_EUNSUPPORTED;
    }
    const int64_t d = (int64_t)h * dk;
    SNF_REQUIRE(ldq >= d && ldv >= d && (ldq % 4) == 0 && (ldv % 4) == 0, "snf_sparse_attn_fwd_x3: ldq=%lld / ldv=%lld must be >= "
                "h*dk and keep rows 16-byte aligned", (long long)ldq, (long long)ldv);
    SNF_REQUIRE(((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(v) | reinterpret_cast<uintptr_t>(kp)) & 15) == 0,
                "snf_sparse_attn_fwd_x3: q / v / kp must be 16-byte aligned");
    const size_t part_bytes = x3_workspace(pl, dk);
    const size_t need = part_bytes + (ch.count > 1 ? (size_t)ch.count * h * n * sizeof(f32x2) : 0);
    if (!workspace || workspace_bytes < need) {
        snf::set_error("snf_sparse_attn_fwd_x3: workspace %zu < %zu", workspace_bytes, need);
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
    if (drop) {
        if (ch.count != 1) {
            snf::set_error("snf_sparse_attn_fwd_x3_dropout: k=%d needs key chunks; the in-kernel mask covers one launch (k <= %d)", k,
                           dk == 128 ? 224 : 256);
            return SNF_EUNSUPPORTED;
        }
        P.drop = *drop;
        return dk == 128 ? x3_dispatch_dropout<128>(P, pl, out, s) : x3_dispatch_dropout<64>(P, pl, out, s);
    }
    if (ch.count == 1) return dk == 128 ? x3_dispatch<128>(P, pl, out, s, 0) : x3_dispatch<64>(P, pl, out, s, 0);
    // key chunks: statistics of every chunk first, then the chunks' main passes with the softmax exact over all keys
    for (int pass = 1; pass <= 2; ++pass)
        for (int c = 0; c < ch.count; ++c) {
            const int k0 = c * ch.size, kc = k - k0 < ch.size ? k - k0 : ch.size;
            X3Params C = P;
            C.kp = kp + (int64_t)k0 * d;
            C.k = kc, C.chunk = c;
            C.attn = (pass == 2 && attn) ? attn + k0 : nullptr;
            C.lse = (pass == 2 && c == 0) ? lse : nullptr;
            int rc = dk == 128 ? x3_dispatch<128>(C, pl, out + (int64_t)k0 * d, s, pass)
                               : x3_dispatch<64>(C, pl, out + (int64_t)k0 * d, s, pass);
            if (rc) return rc;
        }
    return SNF_OK;
}

// ---- varlen (see snf_sparse_attn_varlen_plan in sparse_attn_mfma.hip for the protocol; this is the fp32-class kernel's plan) ----
int snf_sparse_attn_x3_varlen_plan(const int64_t* offsets, int bags, int k, int h, int dk, int32_t* table, size_t table_ints,
                                   size_t* table_ints_needed, size_t* workspace_bytes) {
    SNF_REQUIRE(offsets && bags >= 1 && k >= 1 && h >= 1, "snf_sparse_attn_x3_varlen_plan: bad arguments");
    X3VarlenPlan vp;
    if (!x3_varlen_plan(offsets, bags, k, h, dk, &vp, nullptr, 0)) {
        snf::set_error("snf_sparse_attn_x3_varlen_plan: unsupported shape (bags=%d k=%d dk=%d: dk in {64, 128}, k <= %d, non-empty "
                       "bags)", bags, k, dk, dk == 128 ? 224 : 256);
        return SNF_EUNSUPPORTED;
    }
    const size_t need = (size_t)VL_DESC * bags + (size_t)vp.total_wg;
    if (table_ints_needed) *table_ints_needed = need;
    if (workspace_bytes) *workspace_bytes = (size_t)vp.partial_slots * (size_t)(vp.nkb * (dk / 32)) * 1024 * sizeof(float);
    if (table) {
        SNF_REQUIRE(table_ints >= need, "snf_sparse_attn_x3_varlen_plan: table %zu < %zu ints", table_ints, need);
        x3_varlen_plan(offsets, bags, k, h, dk, &vp, table, table_ints);
    }
    return SNF_OK;
}

// q, v [T, ld] f32 packed rows, kp [bags * k, h * dk] f32, out [bags * k, h * dk], attn [h, T, k] / lse [h, T] or null
int snf_sparse_attn_fwd_x3_varlen(const float* q, int64_t ldq, const float* v, int64_t ldv, const float* kp, const int64_t* offsets,
                                  int bags, int k, int h, int dk, float scale, float* out, float* attn, float* lse,
                                  const int32_t* table_dev, void* workspace, size_t workspace_bytes, snf_stream_t stream) {
    SNF_REQUIRE(q && v && kp && out && offsets && table_dev, "snf_sparse_attn_fwd_x3_varlen: null pointer");
    X3VarlenPlan vp;
    if (!x3_varlen_plan(offsets, bags, k, h, dk, &vp, nullptr, 0)) {
        snf::set_error("snf_sparse_attn_fwd_x3_varlen: unsupported shape (bags=%d k=%d dk=%d)", bags, k, dk);
        return SNF_EUNSUPPORTED;
    }
    const int64_t d = (int64_t)h * dk, total = offsets[bags];
    SNF_REQUIRE(ldq >= d && ldv >= d && (ldq % 4) == 0 && (ldv % 4) == 0, "snf_sparse_attn_fwd_x3_varlen: ldq=%lld / ldv=%lld must be "
                ">= h*dk and keep rows 16-byte aligned", (long long)ldq, (long long)ldv);
    SNF_REQUIRE(((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(v) | reinterpret_cast<uintptr_t>(kp)) & 15) == 0,
                "snf_sparse_attn_fwd_x3_varlen: q / v / kp must be 16-byte aligned");
    const size_t need = (size_t)vp.partial_slots * (size_t)(vp.nkb * (dk / 32)) * 1024 * sizeof(float);
    if (!workspace || workspace_bytes < need) {
        snf::set_error("snf_sparse_attn_fwd_x3_varlen: workspace %zu < %zu", workspace_bytes, need);
        return SNF_EWORKSPACE;
    }
    X3Params P;
    P.q = q, P.v = v, P.kp = kp;
    P.n = total, P.ldq = ldq, P.ldv = ldv, P.ldkp = d;
    P.k = k, P.h = h, P.scale = scale;
    P.attn = attn, P.attn_ld = k, P.lse = lse;
    P.partial = reinterpret_cast<float*>(workspace);
    P.stats = nullptr, P.nchunks = 1, P.chunk = 0;
    P.tiles_per_head = P.tiles_per_wg = P.total_tiles = P.seg_count = 0;   // per bag, from the table
    P.n_stride = total, P.vl = table_dev, P.vl_bags = bags, P.out_direct = out;
    X3Plan pl;
    pl.num_wg = (int)vp.total_wg, pl.nkb = vp.nkb;
    pl.tiles_per_head = pl.tiles_per_wg = pl.total_tiles = pl.seg_count = 0;
    if (vp.all_direct) pl.tiles_per_head = -1;   // x3_launch: no reduction pass
    hipStream_t s = snf::as_stream(stream);
    return dk == 128 ? x3_dispatch_varlen<128>(P, pl, out, s) : x3_dispatch_varlen<64>(P, pl, out, s);
}

// ---- varlen above one key chunk: the chunks of x3_chunks (the single-bag driver's rule, so a packed bag's P and lse are those of its own
// launch bit for bit), a statistics launch (MODE 1) per chunk over all bags, then the chunks' main launches (MODE 2).  One table serves
// every chunk (a bag's tile geometry depends on n and h only); only the key-block count changes per chunk.
struct X3VarlenChunks {
    X3Chunks ch;
    X3VarlenPlan vp;           // geometry at the LARGEST chunk's key-block count (sizes the partial tiles)
    size_t partial_bytes, stats_bytes;
};
static int x3_chunk_nkb(int kc, int dk) {
    X3Plan one;
    return x3_plan(1, kc, 1, dk, &one, true) ? one.nkb : 0;
}
static bool x3_varlen_chunks(const int64_t* offsets, int bags, int k, int h, int dk, X3VarlenChunks* vc, int32_t* table, size_t table_ints) {
    if (bags < 1 || k < 1 || !x3_chunks(k, dk, &vc->ch)) return false;
    const int size = vc->ch.size;
    if (vc->ch.count > 1)
        for (int c = 0; c < vc->ch.count; ++c) {
            const int kc = k - c * size < size ? k - c * size : size;
            if (kc < 1 || !x3_varlen_chunk_built(dk, x3_chunk_nkb(kc, dk))) return false;
        }
    // descriptor word 3 (first Kp / output row of bag b) stays b * k with the FULL key count: the driver offsets the pointers per chunk
    if (!snf_attn::make_varlen_table(offsets, bags, k, &vc->vp, table, table_ints,
                                     [&](int64_t n, X3Plan* pl) { return x3_plan(n, size, h, dk, pl, true); }))
        return false;
    vc->partial_bytes = (size_t)vc->vp.partial_slots * (size_t)(vc->vp.nkb * (dk / 32)) * 1024 * sizeof(float);
    vc->stats_bytes = vc->ch.count > 1 ? (size_t)vc->ch.count * h * (size_t)offsets[bags] * sizeof(f32x2) : 0;
    return true;
}

int snf_sparse_attn_x3_varlen_chunked_plan(const int64_t* offsets, int bags, int k, int h, int dk, int32_t* table, size_t table_ints,
                                           size_t* table_ints_needed, size_t* workspace_bytes, int* n_chunks, int* chunk_k) {
    SNF_REQUIRE(offsets && bags >= 1 && k >= 1 && h >= 1, "snf_sparse_attn_x3_varlen_chunked_plan: bad arguments");
    X3VarlenChunks vc;
    if (!x3_varlen_chunks(offsets, bags, k, h, dk, &vc, nullptr, 0)) {
        snf::set_error("snf_sparse_attn_x3_varlen_chunked_plan: unsupported shape (bags=%d k=%d dk=%d: dk in {64, 128}, k <= 8 x %d, "
                       "non-empty bags)", bags, k, dk, dk == 64 ? 256 : 224);
        return SNF_EUNSUPPORTED;
    }
    const size_t need = (size_t)VL_DESC * bags + (size_t)vc.vp.total_wg;
    if (table_ints_needed) *table_ints_needed = need;
    if (workspace_bytes) *workspace_bytes = vc.partial_bytes + vc.stats_bytes;
    if (n_chunks) *n_chunks = vc.ch.count;
    if (chunk_k) *chunk_k = vc.ch.size;
    if (table) {
        SNF_REQUIRE(table_ints >= need, "snf_sparse_attn_x3_varlen_chunked_plan: table %zu < %zu ints", table_ints, need);
        x3_varlen_chunks(offsets, bags, k, h, dk, &vc, table, table_ints);
    }
    return SNF_OK;
}

// layouts as snf_sparse_attn_fwd_x3_varlen; table_dev / workspace from snf_sparse_attn_x3_varlen_chunked_plan
int snf_sparse_attn_fwd_x3_varlen_chunked(const float* q, int64_t ldq, const float* v, int64_t ldv, const float* kp,
                                          const int64_t* offsets, int bags, int k, int h, int dk, float scale, float* out, float* attn,
                                          float* lse, const int32_t* table_dev, void* workspace, size_t workspace_bytes,
                                          snf_stream_t stream) {
    SNF_REQUIRE(q && v && kp && out && offsets && table_dev, "snf_sparse_attn_fwd_x3_varlen_chunked: null pointer");
    SNF_REQUIRE(k >= 1 && h >= 1, "snf_sparse_attn_fwd_x3_varlen_chunked: bad shape");
    X3VarlenChunks vc;
    if (!x3_varlen_chunks(offsets, bags, k, h, dk, &vc, nullptr, 0)) {
        snf::set_error("snf_sparse_attn_fwd_x3_varlen_chunked: unsupported shape (bags=%d k=%d dk=%d)", bags, k, dk);
        return SNF_EUNSUPPORTED;
    }
    if (vc.ch.count == 1)   // one chunk: the launch (and the table, integer for integer) of the single-chunk entry point
        return snf_sparse_attn_fwd_x3_varlen(q, ldq, v, ldv, kp, offsets, bags, k, h, dk, scale, out, attn, lse, table_dev, workspace,
                                             workspace_bytes, stream);
    const int64_t d = (int64_t)h * dk, total = offsets[bags];
    SNF_REQUIRE(ldq >= d && ldv >= d && (ldq % 4) == 0 && (ldv % 4) == 0, "snf_sparse_attn_fwd_x3_varlen_chunked: ldq=%lld / ldv=%lld "
                "must be >= h*dk and keep rows 16-byte aligned", (long long)ldq, (long long)ldv);
    SNF_REQUIRE(((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(v) | reinterpret_cast<uintptr_t>(kp)) & 15) == 0,
                "snf_sparse_attn_fwd_x3_varlen_chunked: q / v / kp must be 16-byte aligned");
    const size_t need = vc.partial_bytes + vc.stats_bytes;
    if (!workspace || workspace_bytes < need) {
        snf::set_error("snf_sparse_attn_fwd_x3_varlen_chunked: workspace %zu < %zu", workspace_bytes, need);
        return SNF_EWORKSPACE;
    }
    X3Params P;
    P.q = q, P.v = v;
    P.n = total, P.ldq = ldq, P.ldv = ldv, P.ldkp = d;
    P.h = h, P.scale = scale;
    P.attn_ld = k;
    P.partial = reinterpret_cast<float*>(workspace);
    P.stats = reinterpret_cast<f32x2*>(reinterpret_cast<unsigned char*>(workspace) + vc.partial_bytes);   // [count][h][total]
    P.nchunks = vc.ch.count;
    P.tiles_per_head = P.tiles_per_wg = P.total_tiles = P.seg_count = 0;   // per bag, from the table
    P.n_stride = total, P.vl = table_dev, P.vl_bags = bags;
    X3Plan pl;
    pl.num_wg = (int)vc.vp.total_wg;
    pl.tiles_per_wg = pl.total_tiles = pl.seg_count = 0;
    pl.tiles_per_head = vc.vp.all_direct ? -1 : 0;   // x3_launch: -1 = no reduction pass
    hipStream_t s = snf::as_stream(stream);
    for (int pass = 1; pass <= 2; ++pass)
        for (int c = 0; c < vc.ch.count; ++c) {
            const int k0 = c * vc.ch.size, kc = k - k0 < vc.ch.size ? k - k0 : vc.ch.size;
            pl.nkb = x3_chunk_nkb(kc, dk);
            // bag b's keys of this chunk: rows b k + k0 .. of Kp and of the output (the descriptor adds b k)
            P.kp = kp + (int64_t)k0 * d;
            P.k = kc, P.chunk = c;
            P.attn = (pass == 2 && attn) ? attn + k0 : nullptr;
            P.lse = (pass == 2 && c == 0) ? lse : nullptr;
            float* out_c = out + (int64_t)k0 * d;
            P.out_direct = out_c;
            int rc = snf::x3_launch_varlen_chunk(dk, pass, P, pl, out_c, s);
            if (rc) return rc;
        }
    return SNF_OK;
}

}  // extern "C"
