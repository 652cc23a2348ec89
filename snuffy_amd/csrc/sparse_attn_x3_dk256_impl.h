#pragma once
// (implementation header: compiled by sparse_attn_x3_dk256.hip -- the one-launch forms, single bag and varlen, and the C entry points --
// and by sparse_attn_x3_dk256_chunks.hip, the statistics and main passes of a key-chunked launch)
// K7 (fp32-class form on the matrix cores) at its NATIVE head width of 256 (the SimCLR ResNet-18 recipe: D = 512, h = 2, Lambda = 900).
// The arithmetic and the launch protocol are those of sparse_attn_x3_kernel (sparse_attn_x3_impl.h, which this header includes for the
// parameter block, the split and the reduction kernel); the kernel has a name of its own so that no existing instantiation is touched.
//
// What DK = 256 changes against the 64 / 128 body and the 192 one:
//   waves    a workgroup of FOUR waves, one per SIMD (__launch_bounds__(256, 1)): a lane has the whole 512-entry register file.  The Kp
//            fragments of a key block are 2 x 16 x 4 = 128 VGPRs and a wave keeps them for a whole head; next to them 8 output tiles (128
//            accumulators at 4 key blocks), three score tiles (48) and the rows in flight (64) -- 368 before addressing, which two waves
//            per SIMD (256 registers) cannot hold
//   keys     128 per launch (key blocks 1, 2, 4): wave w < NKB owns key block w in GEMM1
//   tile     32 rows (X3Y_ROWS), one row block: at 64 rows and 128 keys Q 64 + P 40 + V 64 KiB do not fit in 160.  GEMM1 has one row
//            block, so the three products of a k-step go to three accumulators of their own (lo x hi, hi x lo, hi x hi: three independent
//            MFMA chains instead of the two interleaved row blocks), summed small terms first: (lh + hl) + hh
//   GEMM2    NCB = 8 column blocks.  Wave w works on ONE key block, kb = w / (4 / NKB), and on the column blocks
//            cb = w % (4 / NKB) + (4 / NKB) ti of it (8, 4, 2 tiles at NKB = 4, 2, 1: an even share always): one P^T fragment pair per
//            16-row k-step feeds all of the wave's MFMAs of that step.  Partial tiles keep the order t_idx = kb * NCB + cb that
//            x3_reduce_kernel reads
//   V image  row pitch 512 bytes = TWO whole bank rows (64 banks x 4 bytes = 256), so every row starts at bank 0 and the 64-byte block b
//            of every row covers the bank quarter b mod 4.  A transpose-read group is 32 lanes = 4 consecutive rows r0 .. r0 + 3 (r0 a
//            multiple of 4) x the same 64-byte block: unswizzled, four times the same quarter.  Block b of row r is stored at block
//            position (b + (r & 3)) mod 8 (in 16-byte chunks: (c + 4 (r & 3)) mod 32, the rotation of the 64 / 128 body at dk = 128): the
//            four rows of a group use the quarters b, b + 1, b + 2, b + 3 (mod 4), every bank once.  Rows 4, 8 or 16 further on have the
//            same r & 3 and sit a whole number of bank rows away, so one address serves both transpose-reads and both k-steps.  The 16-byte
//            stores (8 lanes per group = 32 banks) write the chunks 8 m .. 8 m + 7 of ONE row; rotated by a multiple of 4 chunks they
//            stay 8 consecutive chunks (mod the row, which is bank-row aligned): 128 contiguous bytes, every bank once
//   LDS      32-row tiles, 4 key blocks: Q hi+lo 32 KiB | P hi+lo 20 KiB | V 2 x (hi+lo) 64 KiB | statistics 1 KiB = 117 KiB of 160.  V is
//            DOUBLE-buffered, so the staging is that of the 64 / 128 body: rows fetched two tiles ahead into registers, split and written
//            one tile ahead while the current tile's P is published; three workgroup barriers per tile.
// Register and scratch figures of every form: DESIGN.md section 4, tests/test_attn_widths_host.py.
#include "sparse_attn_x3_impl.h"
#include "attn_width.h"

namespace snf {
// sparse_attn_x3_dk256_chunks.hip: one chunk's statistics pass (mode 1) or main pass (mode 2), single bag (P.vl null) or varlen
int x3_dk256_launch_chunk(int mode, const snf_attn::X3Params& P, const snf_attn::TilePlan& pl, float* out, hipStream_t s);
}  // namespace snf

namespace {

constexpr int X3Y_DK = 256;          // 128 keys per launch, up to 8 chunks: X3Wide
constexpr int X3Y_ROWS = 32;         // query rows per tile (one 32-row block)
constexpr int X3Y_WAVES = 4, X3Y_THREADS = 64 * X3Y_WAVES;

// LDS of one instantiation: Q hi|lo, P hi|lo, V 2 x (hi|lo), statistics
constexpr int x3y_lds_bytes(int nkb) {
    return 2 * (X3Y_DK / 16) * 1024 + 2 * X3Y_ROWS * p_row_bytes(nkb) + 4 * X3Y_ROWS * 2 * X3Y_DK + X3Y_WAVES * X3Y_ROWS * 8;
}

template <int NKB, bool AUX, int MODE, bool VL = false>
__global__ __launch_bounds__(X3Y_THREADS, 1) void sparse_attn_x3_dk256_kernel(X3Params PA) {
    constexpr int DK = X3Y_DK, ROWS = X3Y_ROWS, NTH = X3Y_THREADS;
    constexpr int NKS = DK / 16;               // k-steps of GEMM1
    static_assert(NKB == 1 || NKB == 2 || NKB == 4, "one wave per key block, an even share of the column blocks");
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
    constexpr int WPK = X3Y_WAVES / NKB;       // waves that share a key block in GEMM2
    constexpr int NT = NCB / WPK;              // output tiles owned by one wave (8, 4, 2 at NKB = 4, 2, 1)
    static_assert(NT * WPK == NCB, "the column blocks divide over the waves of a key block");
    constexpr int RS = p_row_bytes(NKB);       // row pitch of a P image
    constexpr int VRS = 2 * DK, NCH = DK / 8;  // row pitch of a V image, 16-byte chunks per row
    constexpr int Q_BYTES = NKS * 1024, PI_BYTES = ROWS * RS, V_BYTES = ROWS * VRS;
    static_assert(2 * Q_BYTES + 2 * PI_BYTES + 4 * V_BYTES + X3Y_WAVES * ROWS * 8 == x3y_lds_bytes(NKB), "LDS map");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    u32x4* lds_qh = reinterpret_cast<u32x4*>(smem);                        // [NKS][64] B fragments of Q, hi
    u32x4* lds_ql = reinterpret_cast<u32x4*>(smem + Q_BYTES);              // lo
    unsigned char* lds_ph = smem + 2 * Q_BYTES;                            // [32 rows][RS] row-major P, hi
    unsigned char* lds_pl = lds_ph + PI_BYTES;                             // lo
    unsigned char* lds_v = lds_pl + PI_BYTES;                              // [2 buffers][hi | lo][32 rows][VRS], chunk-rotated
    f32x2* lds_st = reinterpret_cast<f32x2*>(lds_v + 4 * V_BYTES);         // [4 waves][32 rows] (max * c, sum)

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

    // ---- staging of one tile's Q and V rows: piece p of Q = B fragment (kb = p / 64, lane' = p % 64: row lane' & 31, 8 k from
    //      16 kb + 8 (lane' >> 5)); piece p of V = 8 columns (chunk p % NCH) of row p / NCH.  Four pieces of each per thread.
    constexpr int QPT = NKS * 64 / NTH, VPT = ROWS * NCH / NTH;
    static_assert(QPT * NTH == NKS * 64 && VPT * NTH == ROWS * NCH, "pieces divide over the 256 threads");
    f32x8 qpre[QPT], vpre[VPT];                // the rows of the tile after next, in flight for a whole tile
    int fa = a, ft = t;                        // fetch cursor
    // (opaque thread index: the per-thread piece terms are loop invariants of the tile loop otherwise and are hoisted; recomputed they are
    // a handful of VALU operations)
    auto fetch = [&]() __attribute__((always_inline)) {
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
#pragma unroll
        for (int i = 0; i < QPT; ++i) {
            const int p = tid + NTH * i;
            const int kb = p >> 6, lp = p & 63;
            int row = ft * ROWS + (lp & 31);
            if (row > n32 - 1) row = n32 - 1;
            qpre[i] = load8(P.q + (int64_t)row * P.ldq + fa * DK + 16 * kb + 8 * (lp >> 5));
        }
        if constexpr (MODE != 1) {
#pragma unroll
            for (int i = 0; i < VPT; ++i) {
                const int p = tid + NTH * i;
                int row = ft * ROWS + p / NCH;
                if (row > n32 - 1) row = n32 - 1;
                vpre[i] = load8(P.v + (int64_t)row * P.ldv + fa * DK + 8 * (p % NCH));
            }
        }
        if (++ft == P.tiles_per_head) {
            ft = 0;
            ++fa;
        }
    };
    // chunk position of chunk c in row r of a V image (the bank argument is at the top of this file)
    auto vpos = [](int r, int c) __attribute__((always_inline)) -> int { return (c + 4 * (r & 3)) & (NCH - 1); };
    auto commit = [&](int vbuf) __attribute__((always_inline)) {
        u32x4 hi, lo;
#pragma unroll
        for (int i = 0; i < QPT; ++i) {
            x3_split8(qpre[i], hi, lo);
            lds_qh[tid + NTH * i] = hi;
            lds_ql[tid + NTH * i] = lo;
        }
        if constexpr (MODE != 1) {
            unsigned char* vh = lds_v + vbuf * 2 * V_BYTES;
#pragma unroll
            for (int i = 0; i < VPT; ++i) {
                x3_split8(vpre[i], hi, lo);
                const int p = tid + NTH * i;
                const int row = p / NCH, ch = p % NCH;
                const int off = row * VRS + 16 * vpos(row, ch);
                *reinterpret_cast<u32x4*>(vh + off) = hi;
                *reinterpret_cast<u32x4*>(vh + V_BYTES + off) = lo;
            }
        }
    };
    // this wave's key block (w < NKB) as MFMA A fragments, hi and lo, in registers for the whole head (128 VGPRs); read in four rounds of
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
    const int poff0 = rr0 * RS + 8 * (rch ^ ((rr0 >> 1) & 7)) + 64 * kbw;
    const int poff1 = rr1 * RS + 8 * (rch ^ ((rr1 >> 1) & 7)) + 64 * kbw;
    // V address of tile 0; tile ti is 4 WPK ti chunks further on, modulo the row.  The second transpose-read is 4 rows further on
    // (vpos(r + 4, c) == vpos(r, c)), a k-step 16 rows
    const int vrow = rr0 * VRS + 8 * (ri & 1);
    const int vch0 = vpos(rr0, 4 * cbw + 2 * (rg & 1) + ((ri & 3) >> 1));
    // P image writer (softmax): row j, 4 keys per 8-byte chunk; chunk (2 c4 + hf) of key block w at position ^ ((j >> 1) & 7)
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
        // (opaque lane terms: the row addresses of the direct store are loop invariants of the tile loop otherwise)
        int lane_ = lane;
        asm volatile("" : "+v"(lane_));
        const int j_ = lane_ & 31, hf_ = lane_ >> 5;
        if constexpr (VL) {
            if (P.out_direct) {   // the whole head is in this workgroup: register 4 q4 + i of tile (kb, cb) = O[32 kb + i + 8 q4 + 4 hf, 32 cb + j]
                const int64_t ld = (int64_t)P.h * DK;
#pragma unroll
                for (int ti = 0; ti < NT; ++ti) {
                    float* dcol = P.out_direct + ((int64_t)(32 * kbw + 4 * hf_) * ld + head * DK + 32 * (cbw + WPK * ti) + j_);
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int key = 32 * kbw + (r & 3) + 8 * (r >> 2) + 4 * hf_;
                        if (key < P.k) dcol[(int64_t)((r & 3) + 8 * (r >> 2)) * ld] = acc_o[ti][r];
                    }
                }
                return;
            }
        }
        const int seg = head - first_head;
        float* dst = P.partial + ((int64_t)bid * P.seg_count + seg) * (int64_t)TILES * 1024;
#pragma unroll
        for (int ti = 0; ti < NT; ++ti) {
            const int t_idx = kbw * NCB + cbw + WPK * ti;
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4)
                if (32 * kbw + 8 * q4 < P.k) {
                    const f32x4 v4 = {acc_o[ti][q4 * 4], acc_o[ti][q4 * 4 + 1], acc_o[ti][q4 * 4 + 2], acc_o[ti][q4 * 4 + 3]};
                    *reinterpret_cast<f32x4*>(dst + ((int64_t)(t_idx * 4 + q4) * 64 + lane_) * 4) = v4;
                }
        }
    };

    zero_acc();
    fetch();                                     // tile f_begin
    commit(0);
    if (f_begin + 1 < f_end) fetch();            // tile f_begin + 1 flies under the first tile
    const bool attn_vec = AUX && (P.attn_ld & 3) == 0 && (reinterpret_cast<uintptr_t>(P.attn) & 15) == 0;
    for (int f = f_begin; f < f_end; ++f) {
        const int vb = (f - f_begin) & 1;
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

        // ---- GEMM1 (swapped): S^T[key, row] for key block w; lane = (row j, half hf): keys 32 w + (r&3) + 8 (r>>2) + 4 hf
        f32x16 s;
        float mw = -INFINITY, lw = 0.f;
        if (w < NKB) {
            f32x16 s_lh, s_hl;
#pragma unroll
            for (int r = 0; r < 16; ++r) s[r] = s_lh[r] = s_hl[r] = 0.f;
#pragma unroll
            for (int kb = 0; kb < NKS; ++kb) {
                const bf16x8 qh = __builtin_bit_cast(bf16x8, lds_qh[kb * 64 + lane]);
                const bf16x8 ql = __builtin_bit_cast(bf16x8, lds_ql[kb * 64 + lane]);
                // three accumulation chains: a dependent 32x32 MFMA waits for its predecessor
                s_lh = mfma(kpl[kb], qh, s_lh);
                s_hl = mfma(kph[kb], ql, s_hl);
                s = mfma(kph[kb], qh, s);
            }
            // block-local softmax statistics (padded keys -> -inf)
            float mx = -INFINITY;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = 32 * w + (r & 3) + 8 * (r >> 2) + 4 * hf;
                const float sc = (s_lh[r] + s_hl[r]) + s[r];
                s[r] = key < P.k ? sc * c_exp : -INFINITY;
                mx = fmaxf(mx, s[r]);
            }
            mw = xhalf_max(mx);
            const float mref = mw == -INFINITY ? 0.f : mw;   // a block of padding only: all zeros
            float l = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                s[r] = __builtin_amdgcn_exp2f(s[r] - mref);
                l += s[r];
            }
            lw = xhalf_sum(l);
            if (hf == 0) lds_st[w * ROWS + j] = f32x2{mw, lw};
        }
        __syncthreads();                         // B2: statistics published, every wave is done with the Q images

        if constexpr (MODE == 1) {
            // statistics pass: this chunk's (max, sum) per row, then on to the next tile
            if (w == 0 && hf == 0) {
                const int row = t * ROWS + j;
                if (row < n32) {
                    float m = -INFINITY;
#pragma unroll
                    for (int b = 0; b < NKB; ++b) m = fmaxf(m, lds_st[b * ROWS + j][0]);
                    float l = 0.f;
#pragma unroll
                    for (int b = 0; b < NKB; ++b) {
                        const f32x2 st = lds_st[b * ROWS + j];
                        if (st[0] != -INFINITY) l = fmaf(st[1], __builtin_amdgcn_exp2f(st[0] - m), l);
                    }
                    P.stats[((int64_t)P.chunk * P.h + a) * (VL ? P.n_stride : P.n) + row] = f32x2{m, l};
                }
            }
            if (f + 1 < f_end) {
                commit(0);                       // Q images of the next tile
                if (f + 2 < f_end) fetch();
            }
            a = an;
            t = tn;
            continue;                            // B1 of the next tile orders the statistics slots
        }
        // ---- exact combination over the key blocks, normalisation, publish P = hi + lo
        if (w < NKB) {
            const int row = t * ROWS + j;
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
                for (int b = 0; b < NKB; ++b) m = fmaxf(m, lds_st[b * ROWS + j][0]);
#pragma unroll
                for (int b = 0; b < NKB; ++b) {
                    const f32x2 st = lds_st[b * ROWS + j];
                    l = fmaf(st[1], __builtin_amdgcn_exp2f(st[0] - m), l);
                }
            }
            const float fscale = rvalid ? __builtin_amdgcn_exp2f(mw - m) / l : 0.f;
            if constexpr (AUX)
                if (P.lse && rvalid && hf == 0 && w == 0) P.lse[(int64_t)a * P.n_stride + row] = (m + __log2f(l)) * 0.69314718055994530942f;
            float* arow = nullptr;
            if constexpr (AUX) arow = P.attn ? P.attn + ((int64_t)a * P.n_stride + row) * P.attn_ld + 32 * w + 4 * hf : nullptr;
#pragma unroll
            for (int c4 = 0; c4 < 4; ++c4) {
                f32x4 p4 = {s[4 * c4] * fscale, s[4 * c4 + 1] * fscale, s[4 * c4 + 2] * fscale, s[4 * c4 + 3] * fscale};
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
                *reinterpret_cast<u32x2*>(lds_ph + waddr[c4]) = u32x2{__builtin_bit_cast(unsigned, h01), __builtin_bit_cast(unsigned, h23)};
                *reinterpret_cast<u32x2*>(lds_pl + waddr[c4]) =
                    u32x2{__builtin_bit_cast(unsigned, __builtin_convertvector(r01, bf16x2)),
                          __builtin_bit_cast(unsigned, __builtin_convertvector(r23, bf16x2))};
            }
        }
        // the next tile's rows (fetched a tile ago): Q images are free since B2, the other V buffer since B1
        if (f + 1 < f_end) {
            commit(vb ^ 1);
            if (f + 2 < f_end) fetch();
        }
        __syncthreads();                         // B3: P images complete

        // ---- GEMM2: O[key, col] += P^T V over the 32 rows of the tile (two 16-row k-steps, 3 MFMAs per tile and step)
        const unsigned char* vh_img = lds_v + vb * 2 * V_BYTES + vrow;
#pragma unroll
        for (int sk = 0; sk < ROWS / 16; ++sk) {
            const bf16x8 ph = tr_frag(lds_ph + poff0 + sk * 16 * RS, lds_ph + poff1 + sk * 16 * RS);
            const bf16x8 pl = tr_frag(lds_pl + poff0 + sk * 16 * RS, lds_pl + poff1 + sk * 16 * RS);
#pragma unroll
            for (int ti = 0; ti < NT; ++ti) {
                const unsigned char* vp = vh_img + 16 * ((vch0 + 4 * WPK * ti) & (NCH - 1)) + sk * 16 * VRS;
                const bf16x8 vh = tr_frag(vp, vp + 4 * VRS);
                const bf16x8 vl = tr_frag(vp + V_BYTES, vp + V_BYTES + 4 * VRS);
                acc_o[ti] = mfma(pl, vh, acc_o[ti]);
                acc_o[ti] = mfma(ph, vl, acc_o[ti]);
                acc_o[ti] = mfma(ph, vh, acc_o[ti]);
            }
        }
        a = an;
        t = tn;
    }
    if constexpr (MODE != 1) flush(cur_head);
}

// The width as attn_width.h sees it: 32-row tiles.  A bag inside a packed launch takes 32 tiles (1024 rows, as in x3_plan) per
// workgroup WHATEVER its length: a workgroup's partial tiles are 128 KiB per head segment and key chunk at this width (4 key blocks),
// written once and read once by the reduction -- as much as the Q and V rows of 32 tiles.  The single-bag plan of make_tile_plan (every
// CU busy: two tiles per workgroup at 8000 rows) moved eight times the bag's own bytes in partial tiles per chunk when 64 such bags
// shared a launch; a bag alone keeps that plan, its tiles have the chip to themselves.
struct X3Y : X3Wide {
    static constexpr int DK = X3Y_DK, ROWS = X3Y_ROWS, THREADS = X3Y_THREADS;
    static constexpr int PACKED_TILES = 1024 / X3Y_ROWS;
    static constexpr bool PACKED_FORCED = true;
    static constexpr const char *DK_TEXT = "256", *NAME = "sparse_attn_x3_dk256", *KERNEL = "sparse_attn_x3_dk256_kernel";
    static constexpr int lds_bytes(int nkb) { return x3y_lds_bytes(nkb); }
    template <int NKB, bool AUX, int MODE, bool VL>
    static auto kernel() { return sparse_attn_x3_dk256_kernel<NKB, AUX, MODE, VL>; }
    static int launch_chunk(int mode, const X3Params& P, const X3Plan& pl, float* out, hipStream_t s) {
        return snf::x3_dk256_launch_chunk(mode, P, pl, out, s);
    }
};

}  // namespace
