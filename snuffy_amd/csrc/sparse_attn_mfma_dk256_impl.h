#pragma once
// (implementation header: compiled by sparse_attn_mfma_dk256.hip -- the one-launch forms, single bag and varlen, and the C entry points --
// and by sparse_attn_mfma_dk256_chunks.hip, the statistics and main passes of a key-chunked launch)
// K7 (fast form, bf16 on the matrix cores) at its NATIVE head width of 256 (the SimCLR ResNet-18 recipe: D = 512, h = 2, Lambda = 900).
// The arithmetic and the launch protocol are those of the bf16 family (sparse_attn_mfma_impl.h, which this header includes for the
// parameter block, the Kp staging, the reduction kernel and the driver description): swapped GEMM1 on v_mfma_f32_32x32x16_bf16, fp32
// softmax, P rounded to bf16 for GEMM2, the fp32 P and lse stored before that rounding, (max * scale * log2 e, sum exp) row statistics per
// key chunk.  The ORGANISATION is that of the fp32-class kernel of this width (sparse_attn_x3_dk256_impl.h) with single bf16 images; the
// kernel has a name of its own, so no existing instantiation is touched.
//
// Why not the 64 / 128 / 192 body at DK = 256: its Kp image is NKB x 16 KiB, and beside 4 key blocks (64 KiB) the P (40 KiB) and V
// (64 KiB) images of a 128-row tile do not fit in 160 KiB; its pooling waves would hold 8 output tiles (128 accumulators) plus 64 registers
// of V rows in flight in the 256 registers of a two-waves-per-SIMD launch.  Here:
//   waves    a workgroup of FOUR waves, one per SIMD (__launch_bounds__(256, 1)): a lane may use the whole 512-entry register file.  The Kp
//            fragments of a key block are 16 k-steps x 4 = 64 VGPRs and a wave keeps them for a whole head; next to them 8 output tiles
//            (128 accumulators at 4 key blocks), the score tile (2 x 16 during GEMM1) and the rows in flight (32)
//   keys     128 per launch (key blocks 1, 2, 4): wave w < NKB owns key block w in GEMM1 and the softmax
//   tile     32 rows (one 32-row block), three workgroup barriers per tile
//   GEMM1    16 k-steps in two accumulation chains (even and odd k-steps; a dependent 32x32 MFMA waits for its predecessor), summed once
//   softmax  block-local (max, sum) per wave, published in LDS, combined exactly over the key blocks (or, in a key-chunked launch, over the
//            chunks' statistics from global memory); the block's exponentials are rescaled by exp2(block max - row max) / row sum
//   GEMM2    NCB = 8 column blocks.  Wave w works on ONE key block, kb = w / (4 / NKB), and on the column blocks
//            cb = w % (4 / NKB) + (4 / NKB) ti of it (8, 4, 2 tiles at NKB = 4, 2, 1): one P^T fragment per 16-row k-step feeds all of the
//            wave's MFMAs of that step.  Partial tiles keep the order t_idx = kb * NCB + cb that reduce_partials_kernel<256, NKB> reads
//   V image  row pitch 512 bytes = TWO whole bank rows (64 banks x 4 bytes = 256), so every row starts at bank 0 and the 64-byte block b
//            of every row covers the bank quarter b mod 4.  A transpose-read group is 32 lanes = 4 consecutive rows r0 .. r0 + 3 (r0 a
//            multiple of 4) x the same 64-byte block: unswizzled, four times the same quarter.  Block b of row r is stored at block
//            position (b + (r & 3)) mod 8 (in 16-byte chunks: (c + 4 (r & 3)) mod 32): the four rows of a group use the quarters b, b + 1,
//            b + 2, b + 3 (mod 4), every bank once.  Rows 4, 8 or 16 further on have the same r & 3 and sit a whole number of bank rows
//            away, so one address serves both transpose-reads and both k-steps.  The 16-byte stores (8 lanes per group = 32 banks) write
//            the chunks 8 m .. 8 m + 7 of ONE row; rotated by a multiple of 4 chunks they stay 8 consecutive chunks (mod the row, which is
//            bank-row aligned): 128 contiguous bytes, every bank once.  (The argument of sparse_attn_x3_dk256_impl.h: the image is the same)
//   LDS      4 key blocks: Q 16 KiB | P 10 KiB | V 2 x 16 KiB | statistics 1 KiB = 59 KiB.  V is DOUBLE-buffered: rows are fetched two
//            tiles ahead into registers and written one tile ahead while the current tile's P is published.
// Register and scratch figures of every form: DESIGN.md section 4, tests/test_attn_widths_host.py.
#include "sparse_attn_mfma_impl.h"
#include "attn_width.h"

namespace snf {
// sparse_attn_mfma_dk256_chunks.hip: one chunk's statistics pass (mode 1) or main pass (mode 2), single bag (P.vl null) or varlen
int attn_dk256_launch_chunk(int mode, const snf_attn::AttnParams& P, const snf_attn::TilePlan& pl, float* out, hipStream_t s);
}  // namespace snf

namespace {

constexpr int A256_DK = 256;          // 128 keys per launch, up to 8 chunks: A256 below
constexpr int A256_ROWS = 32;         // query rows per tile (one 32-row block)
constexpr int A256_WAVES = 4, A256_THREADS = 64 * A256_WAVES;

// LDS of one instantiation: Q, P, V x 2, statistics
constexpr int a256_lds_bytes(int nkb) {
    return (A256_DK / 16) * 1024 + A256_ROWS * p_row_bytes(nkb) + 2 * A256_ROWS * 2 * A256_DK + A256_WAVES * A256_ROWS * 8;
}

// Name of the kernel template below.  sparse_attn_mfma_dk256_drop.hip sets it (and SNF_ATTN_DK256_DROP) before it includes this header to
// get the same text under a symbol of its own, with the attention dropout of training compiled in (the device of
// SNF_ATTN_MFMA_KERNEL in sparse_attn_mfma_impl.h); with the defaults nothing about the existing kernels changes.
#ifndef SNF_ATTN_DK256_KERNEL
#define SNF_ATTN_DK256_KERNEL sparse_attn_mfma_dk256_kernel
#endif
#ifndef SNF_ATTN_DK256_DROP
#define SNF_ATTN_DK256_DROP false
#endif

// MODE 0: one launch holds all keys.  MODE 1: statistics pass of one key chunk (P.stats_out).  MODE 2: main pass of one key chunk,
// normalising with the statistics of all chunks (P.stats).  AUX: the attention matrix and / or lse are stored.
// SNF_ATTN_DK256_DROP (single bag, AUX, MODE 0 | 2): the normalised fp32 P is multiplied by the Philox keep-mask / (1 - p) of its 4 keys
// (philox.h; keyed on the key index among ALL keys, P.key0 + ..., and the total key count P.attn_ld) before it is stored and rounded for
// GEMM2 -- lse and the statistics do not see the mask.  The main passes keep the chunks of the launch without dropout: this kernel forms
// P as exp2(s - block max) * (exp2(block max - row max) / row sum), which depends on WHICH 32 keys share a block, so chunks moved to
// multiples of 4 (the 64 / 128 / 192 family's way, whose P is relative to the row max alone) would change P in its last bit.
template <int NKB, bool AUX, int MODE, bool VL = false>
__global__ __launch_bounds__(A256_THREADS, 1) void SNF_ATTN_DK256_KERNEL(AttnParams PA) {
    constexpr bool DROP = SNF_ATTN_DK256_DROP;
    static_assert(!DROP || (AUX && !VL && MODE != 1), "the dropout form: single bag, one launch or main pass");
    constexpr int DK = A256_DK, ROWS = A256_ROWS, NTH = A256_THREADS;
    constexpr int NKS = DK / 16;               // k-steps of GEMM1
    static_assert(NKB == 1 || NKB == 2 || NKB == 4, "one wave per key block, an even share of the column blocks");
    using QT = unsigned short;                 // bf16 bits
    AttnParams P = PA;
    int bid = blockIdx.x;
    if constexpr (VL) {
        const int* __restrict__ tb = PA.vl;
        const int* __restrict__ dsc = tb + VL_DESC * tb[VL_DESC * PA.vl_bags + bid];
        const int row0 = dsc[1];
        bid -= dsc[0];
        P.n = dsc[2];
        P.q = reinterpret_cast<const QT*>(PA.q) + (int64_t)row0 * PA.ldq;
        P.v = reinterpret_cast<const QT*>(PA.v) + (int64_t)row0 * PA.ldv;
        P.kp = PA.kp + (int64_t)dsc[3] * PA.ldkp;
        if (PA.attn) P.attn = PA.attn + (int64_t)row0 * PA.attn_ld;
        if (PA.lse) P.lse = PA.lse + row0;
        if constexpr (MODE == 2) P.stats = PA.stats + (int64_t)row0 * 2;   // this bag's rows of every (chunk, head) plane of n_stride rows
        if constexpr (MODE == 1) P.stats_out = PA.stats_out + (int64_t)row0 * 2;
        P.tiles_per_head = dsc[4], P.tiles_per_wg = dsc[5], P.total_tiles = dsc[6], P.seg_count = dsc[7];
        P.partial = PA.partial + (int64_t)dsc[8] * (NKB * (DK / 32)) * 1024;
        P.out_direct = (PA.out_direct && dsc[10]) ? PA.out_direct + (int64_t)dsc[3] * ((int64_t)PA.h * DK) : nullptr;
    }
    constexpr int NCB = DK / 32;               // 32-wide column blocks of the output
    constexpr int TILES = NKB * NCB;
    constexpr int WPK = A256_WAVES / NKB;      // waves that share a key block in GEMM2
    constexpr int NT = NCB / WPK;              // output tiles owned by one wave (8, 4, 2 at NKB = 4, 2, 1)
    static_assert(NT * WPK == NCB, "the column blocks divide over the waves of a key block");
    constexpr int RS = p_row_bytes(NKB);       // row pitch of the P image
    constexpr int VRS = 2 * DK, NCH = DK / 8;  // row pitch of a V image, 16-byte chunks per row
    constexpr int Q_BYTES = NKS * 1024, PI_BYTES = ROWS * RS, V_BYTES = ROWS * VRS;
    static_assert(Q_BYTES + PI_BYTES + 2 * V_BYTES + A256_WAVES * ROWS * 8 == a256_lds_bytes(NKB), "LDS map");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    u32x4* lds_q = reinterpret_cast<u32x4*>(smem);                         // [NKS][64] B fragments of Q
    unsigned char* lds_p = smem + Q_BYTES;                                 // [32 rows][RS] row-major P (bf16), swizzled
    unsigned char* lds_v = lds_p + PI_BYTES;                               // [2 buffers][32 rows][VRS], chunk-rotated
    f32x2* lds_st = reinterpret_cast<f32x2*>(lds_v + 2 * V_BYTES);         // [4 waves][32 rows] (max * c, sum)

    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, hf = lane >> 5;
    const int n32 = (int)P.n;
    const float c_exp = P.scale * 1.44269504088896340736f;
    const int64_t sn = VL ? P.n_stride : P.n;  // rows of a statistics plane
    const QT* __restrict__ qg = reinterpret_cast<const QT*>(P.q);
    const QT* __restrict__ vg = reinterpret_cast<const QT*>(P.v);

    const int f_begin = bid * P.tiles_per_wg;
    int f_end = f_begin + P.tiles_per_wg;
    if (f_end > P.total_tiles) f_end = P.total_tiles;
    if (f_begin >= f_end) return;
    const int first_head = f_begin / P.tiles_per_head;
    int a = first_head, t = f_begin - first_head * P.tiles_per_head;
    int cur_head = -1;

    // ---- staging of one tile's Q and V rows: piece p of Q = B fragment (kb = p / 64, lane' = p % 64: row lane' & 31, 8 k from
    //      16 kb + 8 (lane' >> 5)); piece p of V = 8 columns (chunk p % NCH) of row p / NCH.  Four pieces of each per thread.
    //      Rows behind the bag's last are clamped to row n - 1: always in bounds; their probabilities are zero.
    constexpr int QPT = NKS * 64 / NTH, VPT = ROWS * NCH / NTH;
    static_assert(QPT * NTH == NKS * 64 && VPT * NTH == ROWS * NCH, "pieces divide over the 256 threads");
    u32x4 qpre[QPT], vpre[VPT];                // the rows of the tile after next, in flight for a whole tile
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
            qpre[i] = *reinterpret_cast<const u32x4*>(qg + (int64_t)row * P.ldq + fa * DK + 16 * kb + 8 * (lp >> 5));
        }
        if constexpr (MODE != 1) {
#pragma unroll
            for (int i = 0; i < VPT; ++i) {
                const int p = tid + NTH * i;
                int row = ft * ROWS + p / NCH;
                if (row > n32 - 1) row = n32 - 1;
                vpre[i] = *reinterpret_cast<const u32x4*>(vg + (int64_t)row * P.ldv + fa * DK + 8 * (p % NCH));
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
#pragma unroll
        for (int i = 0; i < QPT; ++i) lds_q[tid + NTH * i] = qpre[i];
        if constexpr (MODE != 1) {
            unsigned char* vimg = lds_v + vbuf * V_BYTES;
#pragma unroll
            for (int i = 0; i < VPT; ++i) {
                const int p = tid + NTH * i;
                const int row = p / NCH, ch = p % NCH;
                *reinterpret_cast<u32x4*>(vimg + row * VRS + 16 * vpos(row, ch)) = vpre[i];
            }
        }
    };
    // this wave's key block (w < NKB) as MFMA A fragments, in registers for the whole head (64 VGPRs).  Keys behind the chunk's last
    // re-read key k - 1 (in bounds) and are zeroed; their scores are masked to -inf before the softmax anyway
    bf16x8 kpf[NKS];
    auto load_kp = [&](int a_) __attribute__((always_inline)) {
        if (w < NKB) {
            int key = 32 * w + j;
            const bool pad = key >= P.k;
            if (pad) key = P.k - 1;
            const QT* src = P.kp + (int64_t)key * P.ldkp + a_ * DK + 8 * hf;
#pragma unroll
            for (int kb = 0; kb < NKS; ++kb) {
                u32x4 raw = *reinterpret_cast<const u32x4*>(src + 16 * kb);
                if (pad) raw = u32x4{0u, 0u, 0u, 0u};
                kpf[kb] = __builtin_bit_cast(bf16x8, raw);
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
                if (32 * kbw + 8 * q4 < P.k) {   // quads of padding only are never read by the reduction
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
        __syncthreads();                         // B1: Q(f) / V(f) images complete, everybody is past GEMM2(f-1): the P image is free

        // ---- GEMM1 (swapped): S^T[key, row] for key block w; lane = (row j, half hf): keys 32 w + (r&3) + 8 (r>>2) + 4 hf
        f32x16 s;
        float mw = -INFINITY, lw = 0.f;
        if (w < NKB) {
            f32x16 s1;
#pragma unroll
            for (int r = 0; r < 16; ++r) s[r] = s1[r] = 0.f;
#pragma unroll
            for (int kb = 0; kb < NKS; kb += 2) {
                s = mfma(kpf[kb], __builtin_bit_cast(bf16x8, lds_q[kb * 64 + lane]), s);
                s1 = mfma(kpf[kb + 1], __builtin_bit_cast(bf16x8, lds_q[(kb + 1) * 64 + lane]), s1);
            }
            // block-local softmax statistics (keys behind the chunk's last -> -inf)
            float mx = -INFINITY;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = 32 * w + (r & 3) + 8 * (r >> 2) + 4 * hf;
                const float sc = s[r] + s1[r];
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
        __syncthreads();                         // B2: statistics published, every wave is done with the Q image

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
                    reinterpret_cast<f32x2*>(P.stats_out)[(int64_t)a * sn + row] = f32x2{m, l};
                }
            }
            if (f + 1 < f_end) {
                commit(0);                       // Q image of the next tile
                if (f + 2 < f_end) fetch();
            }
            a = an;
            t = tn;
            continue;                            // B1 of the next tile orders the statistics slots
        }
        // ---- exact combination over the key blocks, normalisation, publish P
        if (w < NKB) {
            const int row = t * ROWS + j;
            const bool rvalid = row < n32;
            float m = -INFINITY, l = 0.f;
            if constexpr (MODE == 2) {
                // (a padded row of the last tile reads the BAG's last row: n32 is the bag's own length in a varlen launch)
                const f32x2* st_all = reinterpret_cast<const f32x2*>(P.stats) + ((int64_t)a * sn + (rvalid ? row : n32 - 1));
                const int64_t cs = (int64_t)P.h * sn;
                for (int c = 0; c < P.n_chunks; ++c) m = fmaxf(m, st_all[c * cs][0]);
                for (int c = 0; c < P.n_chunks; ++c) {
                    const f32x2 st = st_all[c * cs];
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
                // the fp32 P is pinned here in every variant: the variants that store A and those that do not round the same values
                asm volatile("" : "+v"(p4));
                if constexpr (DROP) {
                    // one Philox call covers the 4 keys 4 g .. 4 g + 3 among ALL keys.  A chunk that starts on a multiple of 4 (every
                    // one-launch forward) has this lane's 4 keys in one group; otherwise they straddle two groups by sh = key0 & 3
                    // (wave-uniform) and both are drawn.  (A group past the row's last only meets padded keys, whose P is 0.)
                    const int g0 = P.key0 + 32 * w + 8 * c4 + 4 * hf, sh = MODE == 2 ? (P.key0 & 3) : 0;
                    const int64_t mrow = rvalid ? row : n32 - 1;
                    const snf::philox_f4 lo = snf::dropout_mask4(P.drop, a, P.n, mrow, (int)P.attn_ld, g0);
                    f32x4 mk = {lo[0], lo[1], lo[2], lo[3]};
                    if (sh) {
                        const snf::philox_f4 hi = snf::dropout_mask4(P.drop, a, P.n, mrow, (int)P.attn_ld, g0 + 4);
                        mk = sh == 1 ? f32x4{lo[1], lo[2], lo[3], hi[0]} : sh == 2 ? f32x4{lo[2], lo[3], hi[0], hi[1]}
                                                                                  : f32x4{lo[3], hi[0], hi[1], hi[2]};
                    }
                    p4 *= mk;
                }
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
                *reinterpret_cast<u32x2*>(lds_p + waddr[c4]) =
                    u32x2{__builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{p4[0], p4[1]}, bf16x2)),
                          __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{p4[2], p4[3]}, bf16x2))};
            }
        }
        // the next tile's rows (fetched a tile ago): the Q image is free since B2, the other V buffer since B1
        if (f + 1 < f_end) {
            commit(vb ^ 1);
            if (f + 2 < f_end) fetch();
        }
        __syncthreads();                         // B3: P image complete

        // ---- GEMM2: O[key, col] += P^T V over the 32 rows of the tile (two 16-row k-steps, one MFMA per tile and step)
        const unsigned char* v_img = lds_v + vb * V_BYTES + vrow;
#pragma unroll
        for (int sk = 0; sk < ROWS / 16; ++sk) {
            const bf16x8 pf = tr_frag(lds_p + poff0 + sk * 16 * RS, lds_p + poff1 + sk * 16 * RS);
#pragma unroll
            for (int ti = 0; ti < NT; ++ti) {
                const unsigned char* vp = v_img + 16 * ((vch0 + 4 * WPK * ti) & (NCH - 1)) + sk * 16 * VRS;
                acc_o[ti] = mfma(pf, tr_frag(vp, vp + 4 * VRS), acc_o[ti]);
            }
        }
        a = an;
        t = tn;
    }
    if constexpr (MODE != 1) flush(cur_head);
}

// The width as attn_width.h sees it: 32-row tiles, the family's chunk rule (make_chunks: ceil(k / 128) near-equal chunks, no rounding)
// at 128 keys per launch.  count >= 2: k > 128 (count - 1), so size >= 65 (3 or 4 blocks -> 4) and the last chunk k - (count - 1) size
// holds more than 64 - count keys (2, 3 or 4 blocks -> 2 or 4): chunked launches run at 2 or 4 key blocks.
// A bag inside a packed launch takes 32 tiles (1024 rows) per workgroup WHATEVER its length, as at the fp32-class kernel of this width:
// a workgroup's partial tiles are 128 KiB per head segment and key chunk (4 key blocks, fp32 whatever the operands), written once and
// read once by the reduction, while the bf16 Q and V rows of a tile are 32 KiB -- half the fp32-class figure, so the balance is worse
// here: at 1024 rows the partial traffic is a quarter of the operand traffic, at the single-bag plan (two tiles per workgroup at 8000
// rows) it would be four times the operand traffic.
struct A256 {
    using Drive = MfmaDrive;
    static constexpr int DK = A256_DK, ROWS = A256_ROWS, THREADS = A256_THREADS;
    static constexpr int KMAX = 128, MAX_CHUNKS = 8, CHUNK_MULTIPLE = 1;
    static constexpr int64_t MAX_ROWS = 0xffff00ll;   // the family's row limit (32-bit element offsets)
    static constexpr int PACKED_TILES = 1024 / A256_ROWS;
    static constexpr bool PACKED_FORCED = true;
    static constexpr const char *DK_TEXT = "256", *NAME = "sparse_attn_mfma_dk256", *KERNEL = "sparse_attn_mfma_dk256_kernel";
    static constexpr int lds_bytes(int nkb) { return a256_lds_bytes(nkb); }
    template <int NKB, bool AUX, int MODE, bool VL>
    static auto kernel() { return SNF_ATTN_DK256_KERNEL<NKB, AUX, MODE, VL>; }
    static int launch_chunk(int mode, const AttnParams& P, const Plan& pl, float* out, hipStream_t s) {
        return snf::attn_dk256_launch_chunk(mode, P, pl, out, s);
    }
    // the wording of the entry points: k < 1, h < 1 are an unsupported shape to the varlen plan, which words the refusal of a short
    // table itself
    static constexpr bool SHORT_TABLE_UNSUPPORTED = true;
    static bool plan_args_ok(int bags, int, int) { return bags >= 1; }
    static bool varlen_shape_ok(int bags, int k, int h) { return bags >= 1 && k >= 1 && h >= 1; }
    static void refuse_bag(const char* me, int64_t n, int k) {
        snf::set_error("%s: unsupported shape n=%lld k=%d (k <= %d = %d chunks of %d)", me, (long long)n, k, MAX_CHUNKS * KMAX, MAX_CHUNKS, KMAX);
    }
    static void refuse_plan(const char* me, int bags, int k, int h) {
        snf::set_error("%s: unsupported shape (bags=%d k=%d h=%d: need 1 <= k <= %d = %d chunks of %d, h >= 1, non-empty bags)", me, bags, k, h,
                       MAX_CHUNKS * KMAX, MAX_CHUNKS, KMAX);
    }
};

}  // namespace
