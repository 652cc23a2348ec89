#pragma once
// (implementation header: compiled by sparse_attn_x3_dk192.hip -- the one-launch forms, single bag and varlen, and the C entry points --
// and by sparse_attn_x3_dk192_chunks.hip, the statistics and main passes of a key-chunked launch)
// K7 (fp32-class form on the matrix cores) at its NATIVE head width of 192 (the MAE recipe: D = 768, h = 4).  The arithmetic, the
// organisation and the launch protocol are those of sparse_attn_x3_kernel (sparse_attn_x3_impl.h, which this header includes for the
// parameter block, the split and the reduction kernel); the kernel has a name of its own so that no existing instantiation is touched.
//
// What DK = 192 changes against the 64 / 128 body:
//   keys     128 per launch (key blocks 1, 2, 4): the Kp fragments of a block are 2 x 12 x 4 = 96 VGPRs, a workgroup keeps one wave per
//            block and the kernel is compiled for ONE workgroup per CU (__launch_bounds__(512, 1): two waves per SIMD, 256 registers per
//            lane, AGPRs included; the 64 / 128 body is compiled for 128)
//   GEMM1    NKS = 12 k-steps; the Q piece index is taken modulo 12, not masked
//   GEMM2    NCB = 6 column blocks.  Wave w works on ONE key block, kb = w / (8 / NKB), and on the column blocks
//            cb = w % (8 / NKB) + (8 / NKB) ti of it (three each at NKB = 4; an uneven share at NKB = 1, 2): one P^T fragment pair per
//            16-row k-step feeds all of the wave's MFMAs of that step, the V fragments change per tile.  Partial tiles keep the order
//            t_idx = kb * NCB + cb that x3_reduce_kernel reads
//   V image  row pitch 384 bytes = one and a half bank rows: chunk c of row r sits at chunk position c ^ 4 ((r >> 1) & 1) (the swizzle
//            of the bf16 kernel at this width, sparse_attn_mfma_impl.h, where the bank argument is written out)
//   LDS      64-row tiles, 4 key blocks: Q hi+lo 48 KiB | P hi+lo 40 KiB | V hi+lo 48 KiB | statistics 4 KiB = 140 KiB of 160.  V is
//            SINGLE-buffered (a second buffer would need 188 KiB): the next tile's V rows are written after GEMM2 behind a fourth
//            workgroup barrier (B4), its Q rows just before it.  Both leave HBM after B2 of the tile before, so they are in flight under
//            the softmax and GEMM2 and out of the registers during GEMM1 (the statistics pass, which has the room, fetches two tiles
//            ahead as the 64 / 128 body does).  Scratch figures of every form: DESIGN.md section 4, tests/test_attn_widths_host.py.
#include "sparse_attn_x3_impl.h"
#include "attn_width.h"

namespace snf {
// sparse_attn_x3_dk192_chunks.hip: one chunk's statistics pass (mode 1) or main pass (mode 2), single bag (P.vl null) or varlen
int x3_dk192_launch_chunk(int mode, const snf_attn::X3Params& P, const snf_attn::TilePlan& pl, float* out, hipStream_t s);
}  // namespace snf

namespace {

constexpr int X3W_DK = 192;          // 128 keys per launch, up to 8 chunks: X3Wide

template <int NKB, bool AUX, int MODE, bool VL = false>
__global__ __launch_bounds__(512, 1) void sparse_attn_x3_dk192_kernel(X3Params PA) {
    constexpr int DK = X3W_DK;
    constexpr int NKS = DK / 16;               // k-steps of GEMM1
    X3Params P = PA;
    int bid = blockIdx.x;
    if constexpr (VL) {
        const int* __restrict__ tb = PA.vl;
        const int* __restrict__ dsc = tb + VL_DESC * tb[VL_DESC * PA.vl_bags + bid];
        const int row0 = dsc[1];
        bid -= dsc[0];
        P.n = dsc[2];
        P.q = PA.q + (int64_t)row0 * PA.ldq;
        P.v = PA.v + (int64_t)row0 * PA.ldv;
        P.kp = PA.kp + (int64_t)dsc[3] * PA.ldkp;
        if (PA.attn) P.attn = PA.attn + (int64_t)row0 * PA.attn_ld;
        if (PA.lse) P.lse = PA.lse + row0;
        if constexpr (MODE != 0) P.stats = PA.stats + row0;   // this bag's rows of every (chunk, head) plane of n_stride rows
        P.tiles_per_head = dsc[4], P.tiles_per_wg = dsc[5], P.total_tiles = dsc[6], P.seg_count = dsc[7];
        P.partial = PA.partial + (int64_t)dsc[8] * (NKB * (DK / 32)) * 1024;
        P.out_direct = (PA.out_direct && dsc[10]) ? PA.out_direct + (int64_t)dsc[3] * ((int64_t)PA.h * DK) : nullptr;
    }
    constexpr int NCB = DK / 32;               // 32-wide column blocks of the output
    constexpr int TILES = NKB * NCB;
    constexpr int WPK = 8 / NKB;               // waves that share a key block in GEMM2
    constexpr int NT = (NCB + WPK - 1) / WPK;  // output tiles owned by one wave (3, 2, 1 at NKB = 4, 2, 1)
    constexpr int RB = TROWS / 32;             // 32-row blocks per tile
    constexpr int RS = p_row_bytes(NKB);       // row pitch of a P image
    constexpr int VRS = 2 * DK, NCH = DK / 8;  // row pitch of a V image, 16-byte chunks per row
    constexpr int Q_BYTES = RB * NKS * 1024, PI_BYTES = TROWS * RS, V_BYTES = TROWS * VRS;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    u32x4* lds_qh = reinterpret_cast<u32x4*>(smem);                        // [RB][NKS][64] B fragments of Q, hi
    u32x4* lds_ql = reinterpret_cast<u32x4*>(smem + Q_BYTES);              // lo
    unsigned char* lds_ph = smem + 2 * Q_BYTES;                            // [64 rows][RS] row-major P, hi
    unsigned char* lds_pl = lds_ph + PI_BYTES;                             // lo
    unsigned char* lds_v = lds_pl + PI_BYTES;                              // [hi | lo][64 rows][VRS], swizzled, one buffer
    f32x2* lds_st = reinterpret_cast<f32x2*>(lds_v + 2 * V_BYTES);         // [8 waves][64 rows] (max * c, sum)

    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, hf = lane >> 5;
    const int n32 = (int)P.n;
    const float c_exp = P.scale * 1.44269504088896340736f;

    const int f_begin = bid * P.tiles_per_wg;
    int f_end = f_begin + P.tiles_per_wg;
    if (f_end > P.total_tiles) f_end = P.total_tiles;
    if (f_begin >= f_end) return;
    const int first_head = f_begin / P.tiles_per_head;
    int a = first_head, t = f_begin - first_head * P.tiles_per_head;
    int cur_head = -1;

    // ---- staging of one tile's Q and V rows: piece p of Q = B fragment (rb, kb, lane': row 32 rb + (lane' & 31), 8 k from
    //      16 kb + 8 (lane' >> 5)); piece p of V = 8 columns (chunk p % NCH) of row p / NCH.  Three pieces of each per thread.
    constexpr int QPT = RB * NKS * 64 / 512, VPT = TROWS * NCH / 512;
    static_assert(QPT * 512 == RB * NKS * 64 && VPT * 512 == TROWS * NCH, "pieces divide over the 512 threads");
    f32x8 qpre[QPT], vpre[VPT];                // the rows of the next tile, in flight from B2 to the end of GEMM2
    int qa = a, qt = t, va = a, vt = t;        // fetch cursors of Q and V
    // (opaque thread index in the fetches: their per-thread piece terms, hoisted out of the tile loop, were spilled and re-read in
    // front of every load -- three 64-bit offsets per piece; recomputed they are a handful of VALU operations)
    auto fetch_q = [&]() __attribute__((always_inline)) {
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
#pragma unroll
        for (int i = 0; i < QPT; ++i) {
            const int p = tid + 512 * i;
            const int rb = p / (NKS * 64), kb = (p >> 6) % NKS, lp = p & 63;
            int row = qt * TROWS + 32 * rb + (lp & 31);
            if (row > n32 - 1) row = n32 - 1;
            qpre[i] = load8(P.q + (int64_t)row * P.ldq + qa * DK + 16 * kb + 8 * (lp >> 5));
        }
        if (++qt == P.tiles_per_head) {
            qt = 0;
            ++qa;
        }
    };
    auto fetch_v = [&]() __attribute__((always_inline)) {
        if constexpr (MODE != 1) {
            int tid = threadIdx.x;
            asm volatile("" : "+v"(tid));
#pragma unroll
            for (int i = 0; i < VPT; ++i) {
                const int p = tid + 512 * i;
                int row = vt * TROWS + p / NCH;
                if (row > n32 - 1) row = n32 - 1;
                vpre[i] = load8(P.v + (int64_t)row * P.ldv + va * DK + 8 * (p % NCH));
            }
            if (++vt == P.tiles_per_head) {
                vt = 0;
                ++va;
            }
        }
    };
    // chunk position of chunk c in row r of a V image
    auto vpos = [](int r, int c) __attribute__((always_inline)) -> int { return c ^ (4 * ((r >> 1) & 1)); };
    auto commit_q = [&]() __attribute__((always_inline)) {
        u32x4 hi, lo;
#pragma unroll
        for (int i = 0; i < QPT; ++i) {
            x3_split8(qpre[i], hi, lo);
            lds_qh[tid + 512 * i] = hi;
            lds_ql[tid + 512 * i] = lo;
        }
    };
    auto commit_v = [&]() __attribute__((always_inline)) {
        if constexpr (MODE != 1) {
            u32x4 hi, lo;
#pragma unroll
            for (int i = 0; i < VPT; ++i) {
                x3_split8(vpre[i], hi, lo);
                const int p = tid + 512 * i;
                const int row = p / NCH, ch = p % NCH;
                const int off = row * VRS + 16 * vpos(row, ch);
                *reinterpret_cast<u32x4*>(lds_v + off) = hi;
                *reinterpret_cast<u32x4*>(lds_v + V_BYTES + off) = lo;
            }
        }
    };
    // this wave's key block (w < NKB) as MFMA A fragments, hi and lo, in registers for the whole head (96 VGPRs); read in three rounds of
    // four k-steps so that the raw fp32 rows in flight stay at 32 registers
    bf16x8 kph[NKS], kpl[NKS];
    auto load_kp = [&](int a_) __attribute__((always_inline)) {
        if (w < NKB) {
            int key = 32 * w + j;
            const bool pad = key >= P.k;
            if (pad) key = P.k - 1;
            const float* src = P.kp + (int64_t)key * P.ldkp + a_ * DK + 8 * hf;
#pragma unroll
            for (int g = 0; g < NKS / 4; ++g) {
                f32x8 raw[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) raw[u] = load8(src + 16 * (4 * g + u));
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    u32x4 hi, lo;
                    x3_split8(raw[u], hi, lo);
                    if (pad) hi = lo = u32x4{0u, 0u, 0u, 0u};
                    kph[4 * g + u] = __builtin_bit_cast(bf16x8, hi);
                    kpl[4 * g + u] = __builtin_bit_cast(bf16x8, lo);
                }
            }
        }
    };

    // ---- GEMM2 addressing: reader lane = group g (16 lanes) x i; tile ti of this wave = (key block kbw, column block cbw + WPK ti)
    const int rg = lane >> 4, ri = lane & 15;
    const int rr0 = 8 * (rg >> 1) + (ri >> 2), rr1 = rr0 + 4;
    const int rch = 4 * (rg & 1) + (ri & 3);
    const int kbw = w / WPK, cbw = w % WPK;
    auto tile_ok = [&](int ti) __attribute__((always_inline)) -> bool { return NCB % WPK == 0 || cbw + WPK * ti < NCB; };
    const int poff0 = rr0 * RS + 8 * (rch ^ ((rr0 >> 1) & 7)) + 64 * kbw;
    const int poff1 = rr1 * RS + 8 * (rch ^ ((rr1 >> 1) & 7)) + 64 * kbw;
    // one V address per output tile (clamped for the tiles that do not exist); the second transpose-read is 4 rows further on
    // (vpos(r + 4, c) == vpos(r, c)), a k-step 16 rows
    int voff[NT];
#pragma unroll
    for (int ti = 0; ti < NT; ++ti) {
        int cbt = cbw + WPK * ti;
        if (cbt > NCB - 1) cbt = NCB - 1;
        voff[ti] = rr0 * VRS + 16 * vpos(rr0, 4 * cbt + 2 * (rg & 1) + ((ri & 3) >> 1)) + 8 * (ri & 1);
    }
    // P image writer (softmax): row 32 rb + j, 4 keys per 8-byte chunk; chunk (2 c4 + hf) of key block w at position ^ ((j >> 1) & 7)
    int waddr[4];
#pragma unroll
    for (int c4 = 0; c4 < 4; ++c4) waddr[c4] = j * RS + 64 * w + 8 * (((2 * c4) | hf) ^ ((j >> 1) & 7));

    f32x16 acc_o[NT];
    auto zero_acc = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int ti = 0; ti < NT; ++ti)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc_o[ti][r] = 0.f;
    };
    auto flush = [&](int head) __attribute__((always_inline)) {
        // (opaque lane terms: the 48 row addresses of the direct store are loop invariants of the tile loop otherwise, and were hoisted
        // and spilled)
        int lane_ = lane;
        asm volatile("" : "+v"(lane_));
        const int j_ = lane_ & 31, hf_ = lane_ >> 5;
        if constexpr (VL) {
            if (P.out_direct) {   // the whole head is in this workgroup: register 4 q4 + i of tile (kb, cb) = O[32 kb + i + 8 q4 + 4 hf, 32 cb + j]
                const int64_t ld = (int64_t)P.h * DK;
#pragma unroll
                for (int ti = 0; ti < NT; ++ti) {
                    if (tile_ok(ti)) {
                        float* dcol = P.out_direct + ((int64_t)(32 * kbw + 4 * hf_) * ld + head * DK + 32 * (cbw + WPK * ti) + j_);
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int key = 32 * kbw + (r & 3) + 8 * (r >> 2) + 4 * hf_;
                            if (key < P.k) dcol[(int64_t)((r & 3) + 8 * (r >> 2)) * ld] = acc_o[ti][r];
                        }
                    }
                }
                return;
            }
        }
        const int seg = head - first_head;
        float* dst = P.partial + ((int64_t)bid * P.seg_count + seg) * (int64_t)TILES * 1024;
#pragma unroll
        for (int ti = 0; ti < NT; ++ti) {
            if (tile_ok(ti)) {
                const int t_idx = kbw * NCB + cbw + WPK * ti;
#pragma unroll
                for (int q4 = 0; q4 < 4; ++q4)
                    if (32 * kbw + 8 * q4 < P.k) {
                        const f32x4 v4 = {acc_o[ti][q4 * 4], acc_o[ti][q4 * 4 + 1], acc_o[ti][q4 * 4 + 2], acc_o[ti][q4 * 4 + 3]};
                        *reinterpret_cast<f32x4*>(dst + ((int64_t)(t_idx * 4 + q4) * 64 + lane_) * 4) = v4;
                    }
            }
        }
    };

    zero_acc();
    fetch_q();                                   // tile f_begin
    fetch_v();
    commit_q();
    commit_v();
    if constexpr (MODE == 1)
        if (f_begin + 1 < f_end) fetch_q();      // statistics pass: tile f_begin + 1 flies under the first tile
    const bool attn_vec = AUX && (P.attn_ld & 3) == 0 && (reinterpret_cast<uintptr_t>(P.attn) & 15) == 0;
    for (int f = f_begin; f < f_end; ++f) {
        int an = a, tn = t + 1;
        if (tn == P.tiles_per_head) {
            tn = 0;
            an = a + 1;
        }
        if (a != cur_head) {
            // new head: this wave's GEMM2 of the previous tile is behind it, so its accumulators can go
            if (MODE != 1 && cur_head >= 0) {
                flush(cur_head);
                zero_acc();
            }
            load_kp(a);
            cur_head = a;
        }
        __syncthreads();                         // B1: Q(f) / V(f) images complete, everybody is past GEMM2(f-1): the P images are free

        // ---- GEMM1 (swapped): S^T[key, row] for key block w, both row blocks; lane = (row j, half hf): keys 32 w + (r&3) + 8 (r>>2) + 4 hf
        f32x16 s[RB];
        float mw[RB], lw[RB];
        if (w < NKB) {
#pragma unroll
            for (int rb = 0; rb < RB; ++rb)
#pragma unroll
                for (int r = 0; r < 16; ++r) s[rb][r] = 0.f;
#pragma unroll
            for (int kb = 0; kb < NKS; ++kb) {
                bf16x8 qh[RB], ql[RB];
#pragma unroll
                for (int rb = 0; rb < RB; ++rb) {
                    qh[rb] = __builtin_bit_cast(bf16x8, lds_qh[(rb * NKS + kb) * 64 + lane]);
                    ql[rb] = __builtin_bit_cast(bf16x8, lds_ql[(rb * NKS + kb) * 64 + lane]);
                }
                // the two row blocks' accumulation chains alternate: a dependent 32x32 MFMA waits 16 passes for its predecessor
#pragma unroll
                for (int rb = 0; rb < RB; ++rb) s[rb] = mfma(kpl[kb], qh[rb], s[rb]);
#pragma unroll
                for (int rb = 0; rb < RB; ++rb) s[rb] = mfma(kph[kb], ql[rb], s[rb]);
#pragma unroll
                for (int rb = 0; rb < RB; ++rb) s[rb] = mfma(kph[kb], qh[rb], s[rb]);
            }
            // block-local softmax statistics (padded keys -> -inf)
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) {
                float mx = -INFINITY;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = 32 * w + (r & 3) + 8 * (r >> 2) + 4 * hf;
                    s[rb][r] = key < P.k ? s[rb][r] * c_exp : -INFINITY;
                    mx = fmaxf(mx, s[rb][r]);
                }
                mw[rb] = xhalf_max(mx);
                const float mref = mw[rb] == -INFINITY ? 0.f : mw[rb];   // a block of padding only: all zeros
                float l = 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    s[rb][r] = __builtin_amdgcn_exp2f(s[rb][r] - mref);
                    l += s[rb][r];
                }
                lw[rb] = xhalf_sum(l);
                if (hf == 0) lds_st[w * TROWS + 32 * rb + j] = f32x2{mw[rb], lw[rb]};
            }
        }
        __syncthreads();                         // B2: statistics published, every wave is done with the Q images
        // the next tile's rows leave HBM here and are written behind GEMM2: in flight under the softmax and GEMM2, and out of the
        // registers while GEMM1 holds the Kp fragments, two score tiles and the output tiles (96 + 32 + 48 VGPRs)
        if constexpr (MODE != 1)
            if (f + 1 < f_end) {
                fetch_q();
                fetch_v();
            }

        if constexpr (MODE == 1) {
            // statistics pass: this chunk's (max, sum) per row, then on to the next tile
            if (w < RB && hf == 0) {
                const int row = t * TROWS + 32 * w + j;
                if (row < n32) {
                    float m = -INFINITY;
#pragma unroll
                    for (int b = 0; b < NKB; ++b) m = fmaxf(m, lds_st[b * TROWS + 32 * w + j][0]);
                    float l = 0.f;
#pragma unroll
                    for (int b = 0; b < NKB; ++b) {
                        const f32x2 st = lds_st[b * TROWS + 32 * w + j];
                        if (st[0] != -INFINITY) l = fmaf(st[1], __builtin_amdgcn_exp2f(st[0] - m), l);
                    }
                    P.stats[((int64_t)P.chunk * P.h + a) * (VL ? P.n_stride : P.n) + row] = f32x2{m, l};
                }
            }
            if (f + 1 < f_end) {
                commit_q();                      // Q images of the next tile
                if (f + 2 < f_end) fetch_q();
            }
            a = an;
            t = tn;
            continue;                            // B1 of the next tile orders the statistics slots
        }
        // ---- exact combination over the key blocks, normalisation, publish P = hi + lo
        if (w < NKB) {
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) {
                const int row = t * TROWS + 32 * rb + j;
                const bool rvalid = row < n32;
                float m = -INFINITY, l = 0.f;
                if constexpr (MODE == 2) {
                    // (a padded row of the last tile reads the BAG's last row: n32 is the bag's own length in a varlen launch)
                    const int64_t so = (int64_t)a * (VL ? P.n_stride : P.n) + (rvalid ? row : n32 - 1);
                    for (int c = 0; c < P.nchunks; ++c) m = fmaxf(m, P.stats[(int64_t)c * P.h * (VL ? P.n_stride : P.n) + so][0]);
                    for (int c = 0; c < P.nchunks; ++c) {
                        const f32x2 st = P.stats[(int64_t)c * P.h * (VL ? P.n_stride : P.n) + so];
                        if (st[0] != -INFINITY) l = fmaf(st[1], __builtin_amdgcn_exp2f(st[0] - m), l);
                    }
                } else {
#pragma unroll
                    for (int b = 0; b < NKB; ++b) m = fmaxf(m, lds_st[b * TROWS + 32 * rb + j][0]);
#pragma unroll
                    for (int b = 0; b < NKB; ++b) {
                        const f32x2 st = lds_st[b * TROWS + 32 * rb + j];
                        l = fmaf(st[1], __builtin_amdgcn_exp2f(st[0] - m), l);
                    }
                }
                const float fscale = rvalid ? __builtin_amdgcn_exp2f(mw[rb] - m) / l : 0.f;
                if constexpr (AUX)
                    if (P.lse && rvalid && hf == 0 && w == 0) P.lse[(int64_t)a * P.n_stride + row] = (m + __log2f(l)) * 0.69314718055994530942f;
                float* arow = nullptr;
                if constexpr (AUX) arow = P.attn ? P.attn + ((int64_t)a * P.n_stride + row) * P.attn_ld + 32 * w + 4 * hf : nullptr;
#pragma unroll
                for (int c4 = 0; c4 < 4; ++c4) {
                    f32x4 p4 = {s[rb][4 * c4] * fscale, s[rb][4 * c4 + 1] * fscale, s[rb][4 * c4 + 2] * fscale, s[rb][4 * c4 + 3] * fscale};
                    // P is ROUNDED to fp32 here in every variant: without this the compiler contracts the product into the
                    // subtraction of the split below (fma) in the variants that do not store A, and their O differs in the last bits
                    asm volatile("" : "+v"(p4));
                    if constexpr (AUX) {
                        if (arow && rvalid) {
                            const int key0 = 32 * w + 8 * c4 + 4 * hf;
                            if (attn_vec && key0 + 4 <= P.k) {
                                *reinterpret_cast<f32x4*>(arow + 8 * c4) = p4;
                            } else {
#pragma unroll
                                for (int e = 0; e < 4; ++e)
                                    if (key0 + e < P.k) arow[8 * c4 + e] = p4[e];
                            }
                        }
                    }
                    const bf16x2 h01 = __builtin_convertvector(f32x2{p4[0], p4[1]}, bf16x2);
                    const bf16x2 h23 = __builtin_convertvector(f32x2{p4[2], p4[3]}, bf16x2);
                    const f32x2 r01 = f32x2{p4[0], p4[1]} - __builtin_convertvector(h01, f32x2);
                    const f32x2 r23 = f32x2{p4[2], p4[3]} - __builtin_convertvector(h23, f32x2);
                    *reinterpret_cast<u32x2*>(lds_ph + 32 * rb * RS + waddr[c4]) =
                        u32x2{__builtin_bit_cast(unsigned, h01), __builtin_bit_cast(unsigned, h23)};
                    *reinterpret_cast<u32x2*>(lds_pl + 32 * rb * RS + waddr[c4]) =
                        u32x2{__builtin_bit_cast(unsigned, __builtin_convertvector(r01, bf16x2)),
                              __builtin_bit_cast(unsigned, __builtin_convertvector(r23, bf16x2))};
                }
            }
        }
        __syncthreads();                         // B3: P images complete

        // ---- GEMM2: O[key, col] += P^T V over the 64 rows of the tile (four 16-row k-steps, 3 MFMAs per tile and step)
#pragma unroll
        for (int sk = 0; sk < TROWS / 16; ++sk) {
            const bf16x8 ph = tr_frag(lds_ph + poff0 + sk * 16 * RS, lds_ph + poff1 + sk * 16 * RS);
            const bf16x8 pl = tr_frag(lds_pl + poff0 + sk * 16 * RS, lds_pl + poff1 + sk * 16 * RS);
#pragma unroll
            for (int ti = 0; ti < NT; ++ti) {
                if (tile_ok(ti)) {
                    const unsigned char* vp = lds_v + voff[ti] + sk * 16 * VRS;
                    const bf16x8 vh = tr_frag(vp, vp + 4 * VRS);
                    const bf16x8 vl = tr_frag(vp + V_BYTES, vp + V_BYTES + 4 * VRS);
                    acc_o[ti] = mfma(pl, vh, acc_o[ti]);
                    acc_o[ti] = mfma(ph, vl, acc_o[ti]);
                    acc_o[ti] = mfma(ph, vh, acc_o[ti]);
                }
            }
        }
        // the next tile's rows: the Q images are free since B2, the one V buffer once every wave is past GEMM2(f)
        if (f + 1 < f_end) {
            commit_q();
            __syncthreads();                     // B4
            commit_v();
        }
        a = an;
        t = tn;
    }
    if constexpr (MODE != 1) flush(cur_head);
}

// The width as attn_width.h sees it.  A bag inside a packed launch takes at least 16 tiles (1024 rows) per workgroup, as in x3_plan
struct X3W : X3Wide {
    static constexpr int DK = X3W_DK, ROWS = TROWS, THREADS = 512;
    static constexpr int PACKED_TILES = 16;
    static constexpr bool PACKED_FORCED = false;
    static constexpr const char *DK_TEXT = "192", *NAME = "sparse_attn_x3_dk192", *KERNEL = "sparse_attn_x3_dk192_kernel";
    // Q hi|lo, P hi|lo, V hi|lo, statistics
    static constexpr int lds_bytes(int nkb) {
        return 2 * (TROWS / 32) * (DK / 16) * 1024 + 2 * TROWS * p_row_bytes(nkb) + 2 * TROWS * 2 * DK + 8 * TROWS * 8;
    }
    template <int NKB, bool AUX, int MODE, bool VL>
    static auto kernel() { return sparse_attn_x3_dk192_kernel<NKB, AUX, MODE, VL>; }
    static int launch_chunk(int mode, const X3Params& P, const X3Plan& pl, float* out, hipStream_t s) {
        return snf::x3_dk192_launch_chunk(mode, P, pl, out, s);
    }
};

}  // namespace
