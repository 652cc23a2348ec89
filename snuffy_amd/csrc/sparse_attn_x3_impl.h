#pragma once
// (implementation header: compiled by sparse_attn_x3.hip -- the single-bag and single-chunk varlen variants and the C entry points -- and
// by sparse_attn_x3_varlen_chunks.hip, the key-chunked varlen variants; included by sparse_attn_x3_dk192_impl.h.  The host driver of
// the entry points is attn_drive.h: this header keeps the family's chunk rule, planner and kernel switches)
// K7 (fp32-class form on the matrix cores): Snuffy's sparse attention with SPLIT-bf16 operands.
//
//   per head a:   P_a = softmax_j(Q_a Kp_a^T * scale)  [n, k]      O_a = P_a^T V_a  [k, dk]        (snuffy.py:160-168)
//
// The reference computes this in fp32.  gfx950 has no fast fp32 matrix path (v_mfma_f32_32x32x2_f32 runs at the vector
// rate, 1/16 of bf16), so every fp32 operand x is split into x = hi + lo with hi = bf16(x), lo = bf16(x - hi), and every
// product a b is taken as  ah bh + ah bl + al bh  -- three bf16 MFMAs with fp32 accumulate; the dropped term al bl is
// 2^-17 relative (fp32-class: measured <= 3.5e-6 on P and <= 1e-5 of its scale on O against the fp64 oracle on nine shapes,
// tests/test_gpu_kernels.py; the exact vector-ALU kernel gives 4e-7 / 9e-7, the bf16 kernel 5e-3).
// Softmax, the normalisation and all accumulation are fp32; P is split after the normalisation.
//
// Organisation (round 3): one workgroup (8 waves) per CU walks (head, 64-ROW tile) items and all 8 waves cooperate on a tile:
//   Kp      wave w owns key block w (32 keys) and keeps its hi / lo MFMA fragments in REGISTERS for the whole head (64 VGPRs at
//           dk = 128) -- a 112 KiB LDS image in the first version, which left room for 32-row tiles only
//   stage   Q and V rows: fp32 from HBM two tiles ahead (registers), split and written as MFMA-shaped images one tile ahead
//           (separate Q / P images, V double-buffered), while the current tile's P is being published
//   GEMM1   S^T[key, row] = Kp Q^T for key block w and both 32-row blocks, 3 MFMAs per 16-deep k-step, the two blocks'
//           accumulation chains interleaved (a dependent 32x32 MFMA waits for its predecessor)
//   softmax every lane holds 16 keys of ONE row (C layout of the swapped product) -> block-local max / exp / sum, one
//           (max, sum) pair per wave and row through LDS, combined exactly (as the key-chunked launches of the bf16 kernel)
//   GEMM2   O[key, col] += P^T V over the tile's 64 rows: 28 output tiles of 32 x 32 spread over the 8 waves, both operands
//           by hardware transpose-read (ds_read_b64_tr_b16) out of row-major images, 3 MFMAs per 16-row k-step
// Three workgroup barriers per 64 rows (four per 32 before).  Accumulators stay in registers until the head changes; partial
// tiles are written in fragment order and summed in ascending workgroup order by a second kernel (no float atomics).
// LDS at dk = 128, 224 keys: Q hi+lo 32 KiB | P hi+lo 56 KiB | V 2 x (hi+lo) 64 KiB | row statistics 4 KiB = 156 KiB.
#include <math.h>

#include "attn_drive.h"
#include "mfma.h"
#include "philox.h"

namespace snf_attn {
struct X3Params {
    const float* q;    // [n, ldq]
    const float* v;    // [n, ldv]
    const float* kp;   // [k, ldkp]
    int64_t n, ldq, ldv, ldkp;
    int k, h;
    float scale;
    float* attn;       // [h, n, attn_ld] (already offset to this launch's first key) or null
    int64_t attn_ld;
    float* lse;        // [h, n] or null
    // key-chunked launches (k above one LDS image): stats [nchunks][h][n] of (max * c, sum) pairs.  MODE 1 writes chunk
    // `chunk`'s pair per row; MODE 2 reads all chunks' pairs instead of combining its own (softmax exact over all keys).
    // Varlen launches: [nchunks][h][n_stride] over ALL packed rows, addressed like lse (row0 + the row inside the bag)
    f32x2* stats;
    int nchunks, chunk;
    float* partial;    // [num_wg * seg_count][tiles][4][64][4]
    int tiles_per_head, tiles_per_wg, total_tiles, seg_count;
    int64_t n_stride;  // rows per head of attn / lse (= n; the packed row count of a varlen launch)
    const int* vl;     // varlen launch: [bags][VL_DESC] descriptors, then the bag of every workgroup (attn_plan.h)
    int vl_bags;
    float* out_direct; // varlen: output [rows, h * dk] for bags with one workgroup per head (descriptor flag 10): stored straight from the
                       // accumulators, no partial tile and no reduction pass for that bag; null = always partials
    snf::DropoutState drop = {0u, 0u, 0u, 0u, 0u, 1.f};   // DROP instantiations (training, snuffy.py:166-167): O = (P o M)^T V, attn = P
};
}  // namespace snf_attn

namespace {

using snf_attn::VL_DESC;
using snf_attn::X3Params;
using snf_attn::p_row_bytes;
using X3Plan = snf_attn::TilePlan;
using X3Chunks = snf_attn::Chunks;   // x3_chunks / width_chunks: count chunks of size keys

constexpr int TROWS = 64;   // query rows per step (two 32-row blocks)

// the shared split, with the timing ablation of tools/x3_ablate.sh in front of it
__device__ __forceinline__ void x3_split8(const f32x8 x, u32x4& hi, u32x4& lo) {
#ifdef X3_ABL_NOSPLIT   // two cheap packs instead of the split, wrong numbers
    const u32x4 a = __builtin_bit_cast(u32x4, f32x4{x[0], x[2], x[4], x[6]}), b = __builtin_bit_cast(u32x4, f32x4{x[1], x[3], x[5], x[7]});
    hi = (a >> 16) | (b & 0xffff0000u);
    lo = (a & 0xffffu) | (b << 16);
    return;
#endif
    split8(x, hi, lo);
}

// MODE 0: one launch covers all keys.  MODE 1: statistics pass of one key chunk (GEMM1 + max / sum, nothing else).
// MODE 2: main pass of one key chunk with the row statistics of ALL chunks taken from P.stats.
//
// Round 3 organisation: wave w keeps the hi / lo fragments of ITS key block in registers for a whole head (2 NKS fragments = 64
// VGPRs at dk = 128) instead of re-reading them from a 112 KiB LDS image every tile.  The LDS that frees holds 64-ROW tiles with
// separate Q, P and (double-buffered) V images, so a tile costs three workgroup barriers instead of four per 32 rows, the next
// tile's rows are split and written while this tile's P is published, and their HBM loads have a whole tile of latency cover.
// DROP (round 5, single key chunk): the Philox keep-mask of csrc/philox.h (the one snf_dropout_mask_f32 writes out, bit for bit) is applied to
// P in registers before its split for GEMM2; the probabilities written to `attn` stay the undropped ones the backward wants.
template <int DK, int NKB, bool AUX, int MODE, bool VL = false, bool DROP = false>
__global__ __launch_bounds__(512, 2) void sparse_attn_x3_kernel(X3Params PA) {
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
    constexpr int NT = (TILES + 7) / 8;        // output tiles owned by one wave
    constexpr int RB = TROWS / 32;             // 32-row blocks per tile
    constexpr int RS = p_row_bytes(NKB);       // row pitch of a P image
    constexpr int VRS = 2 * DK, NCH = DK / 8;  // row pitch of a V image, 16-byte chunks per row
    constexpr int Q_BYTES = RB * NKS * 1024, PI_BYTES = TROWS * RS, V_BYTES = TROWS * VRS;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    u32x4* lds_qh = reinterpret_cast<u32x4*>(smem);                        // [RB][NKS][64] B fragments of Q, hi
    u32x4* lds_ql = reinterpret_cast<u32x4*>(smem + Q_BYTES);              // lo
    unsigned char* lds_ph = smem + 2 * Q_BYTES;                            // [64 rows][RS] row-major P, hi
    unsigned char* lds_pl = lds_ph + PI_BYTES;                             // lo
    unsigned char* lds_v = lds_pl + PI_BYTES;                              // [2 buffers][hi | lo][64 rows][VRS], chunk-rotated
    f32x2* lds_st = reinterpret_cast<f32x2*>(lds_v + 4 * V_BYTES);         // [8 waves][64 rows] (max * c, sum)

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
    //      16 kb + 8 (lane' >> 5)); piece p of V = 8 columns (chunk p % NCH) of row p / NCH
    constexpr int QPT = RB * NKS * 64 / 512, VPT = TROWS * NCH / 512;     // pieces per thread: 2 + 2 at dk = 128, 1 + 1 at dk = 64
    f32x8 qpre[QPT], vpre[VPT];                // the rows of the tile after next, in flight for a whole tile
    int fa = a, ft = t;                        // fetch cursor
    auto fetch = [&]() __attribute__((always_inline)) {
        // (opaque thread index in the DROP instantiation: its per-thread row terms, hoisted out of the tile loop, were spilled next to the
        // Philox state and re-read behind vmcnt(0) waits that also drained the PREVIOUS row fetch -- the next tile's loads went out one
        // HBM round trip after the other)
        int tid = threadIdx.x;
        if constexpr (DROP) asm volatile("" : "+v"(tid));
#pragma unroll
        for (int i = 0; i < QPT; ++i) {
            const int p = tid + 512 * i;
            const int rb = p / (NKS * 64), kb = (p >> 6) & (NKS - 1), lp = p & 63;
            int row = ft * TROWS + 32 * rb + (lp & 31);
            if (row > n32 - 1) row = n32 - 1;
            qpre[i] = load8(P.q + (int64_t)row * P.ldq + fa * DK + 16 * kb + 8 * (lp >> 5));
        }
        if constexpr (MODE != 1) {
#pragma unroll
            for (int i = 0; i < VPT; ++i) {
                const int p = tid + 512 * i;
                int row = ft * TROWS + p / NCH;
                if (row > n32 - 1) row = n32 - 1;
                vpre[i] = load8(P.v + (int64_t)row * P.ldv + fa * DK + 8 * (p % NCH));
            }
        }
        if (++ft == P.tiles_per_head) {
            ft = 0;
            ++fa;
        }
    };
    auto vrot = [](int r) __attribute__((always_inline)) -> int { return DK == 128 ? (r & 3) : ((r >> 1) & 1); };
    auto commit = [&](int vbuf) __attribute__((always_inline)) {
        u32x4 hi, lo;
#pragma unroll
        for (int i = 0; i < QPT; ++i) {
            x3_split8(qpre[i], hi, lo);
            lds_qh[tid + 512 * i] = hi;
            lds_ql[tid + 512 * i] = lo;
        }
        if constexpr (MODE != 1) {
            unsigned char* vh = lds_v + vbuf * 2 * V_BYTES;
#pragma unroll
            for (int i = 0; i < VPT; ++i) {
                x3_split8(vpre[i], hi, lo);
                const int p = tid + 512 * i;
                const int row = p / NCH, ch = p % NCH;
                const int off = row * VRS + 16 * ((ch + 4 * vrot(row)) & (NCH - 1));
                *reinterpret_cast<u32x4*>(vh + off) = hi;
                *reinterpret_cast<u32x4*>(vh + V_BYTES + off) = lo;
            }
        }
    };
    // this wave's key block (w < NKB) as MFMA A fragments, hi and lo, in registers for the whole head
    bf16x8 kph[NKS], kpl[NKS];
    auto load_kp = [&](int a_) __attribute__((always_inline)) {
        if (w < NKB) {
            int key = 32 * w + j;
            const bool pad = key >= P.k;
            if (pad) key = P.k - 1;
            f32x8 raw[NKS];
#pragma unroll
            for (int kb = 0; kb < NKS; ++kb) raw[kb] = load8(P.kp + (int64_t)key * P.ldkp + a_ * DK + 16 * kb + 8 * hf);
#pragma unroll
            for (int kb = 0; kb < NKS; ++kb) {
                u32x4 hi, lo;
                x3_split8(raw[kb], hi, lo);
                if (pad) hi = lo = u32x4{0u, 0u, 0u, 0u};
                kph[kb] = __builtin_bit_cast(bf16x8, hi);
                kpl[kb] = __builtin_bit_cast(bf16x8, lo);
            }
        }
    };

    // ---- GEMM2 addressing (as in sparse_attn_mfma_impl.h): reader lane = group g (16 lanes) x i
    const int rg = lane >> 4, ri = lane & 15;
    const int rr0 = 8 * (rg >> 1) + (ri >> 2), rr1 = rr0 + 4;
    const int rch = 4 * (rg & 1) + (ri & 3);
    const int cb = w & (NCB - 1);                                     // column block of every tile of this wave
    const int kb0 = w / NCB;                                          // key block of tile ti: kb0 + ti * (8 / NCB)
    const int poff0 = rr0 * RS + 8 * (rch ^ ((rr0 >> 1) & 7)) + 64 * kb0;
    const int poff1 = rr1 * RS + 8 * (rch ^ ((rr1 >> 1) & 7)) + 64 * kb0;
    const int vrc = 4 * cb + 2 * (rg & 1) + ((ri & 3) >> 1);
    const int voff0 = rr0 * VRS + 16 * ((vrc + 4 * vrot(rr0)) & (NCH - 1)) + 8 * (ri & 1);
    const int voff1 = rr1 * VRS + 16 * ((vrc + 4 * vrot(rr1)) & (NCH - 1)) + 8 * (ri & 1);
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
        if constexpr (VL) {
            if (P.out_direct) {   // the whole head is in this workgroup: register 4 q4 + i of tile (kb, cb) = O[32 kb + i + 8 q4 + 4 hf, 32 cb + j]
                const int64_t ld = (int64_t)P.h * DK;
#pragma unroll
                for (int ti = 0; ti < NT; ++ti) {
                    const int t_idx = w + 8 * ti;
                    if (t_idx < TILES) {
                        const int kb_ = t_idx / NCB, cb_ = t_idx - kb_ * NCB;
                        float* dcol = P.out_direct + head * DK + 32 * cb_ + j;
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int key = 32 * kb_ + (r & 3) + 8 * (r >> 2) + 4 * hf;
                            if (key < P.k) dcol[(int64_t)key * ld] = acc_o[ti][r];
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
            const int t_idx = w + 8 * ti;
            if (t_idx < TILES) {
                const int key0 = 32 * (t_idx / NCB);
#pragma unroll
                for (int q4 = 0; q4 < 4; ++q4)
                    if (key0 + 8 * q4 < P.k) {
                        const f32x4 v4 = {acc_o[ti][q4 * 4], acc_o[ti][q4 * 4 + 1], acc_o[ti][q4 * 4 + 2], acc_o[ti][q4 * 4 + 3]};
                        *reinterpret_cast<f32x4*>(dst + ((int64_t)(t_idx * 4 + q4) * 64 + lane) * 4) = v4;
                    }
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
                commit(0);                       // Q images of the next tile
                if (f + 2 < f_end) fetch();
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
                    // rows of a statistics plane: the bag's own, or all packed rows of a varlen launch
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
                    if constexpr (DROP) {
                        const snf::philox_f4 mk = snf::dropout_mask4(P.drop, a, P.n_stride, rvalid ? row : 0, P.k, 32 * w + 8 * c4 + 4 * hf);
                        p4 = f32x4{p4[0] * mk[0], p4[1] * mk[1], p4[2] * mk[2], p4[3] * mk[3]};
                        asm volatile("" : "+v"(p4));
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
        // the next tile's rows (fetched a tile ago): Q images are free since B2, the other V buffer since B1
        if (f + 1 < f_end) {
            commit(vb ^ 1);
            if (f + 2 < f_end) fetch();
        }
        __syncthreads();                         // B3: P images complete

        // ---- GEMM2: O[key, col] += P^T V over the 64 rows of the tile (four 16-row k-steps, 3 MFMAs each)
        const unsigned char* vh_img = lds_v + vb * 2 * V_BYTES;
#pragma unroll
        for (int sk = 0; sk < TROWS / 16; ++sk) {
            const bf16x8 vh = tr_frag(vh_img + voff0 + sk * 16 * VRS, vh_img + voff1 + sk * 16 * VRS);
            const bf16x8 vl = tr_frag(vh_img + V_BYTES + voff0 + sk * 16 * VRS, vh_img + V_BYTES + voff1 + sk * 16 * VRS);
#pragma unroll
            for (int ti = 0; ti < NT; ++ti) {
                if (TILES % 8 == 0 || w + 8 * ti < TILES) {
                    const int off = sk * 16 * RS + ti * (8 / NCB) * 64;
                    const bf16x8 ph = tr_frag(lds_ph + poff0 + off, lds_ph + poff1 + off);
                    const bf16x8 pl = tr_frag(lds_pl + poff0 + off, lds_pl + poff1 + off);
                    acc_o[ti] = mfma(pl, vh, acc_o[ti]);
                    acc_o[ti] = mfma(ph, vl, acc_o[ti]);
                    acc_o[ti] = mfma(ph, vh, acc_o[ti]);
                }
            }
        }
        a = an;
        t = tn;
    }
    if constexpr (MODE != 1) flush(cur_head);
}

// out[key, a*DK + col] = sum over the (workgroup, segment) partials of head a, ascending workgroup order
template <int DK, int NKB>
__global__ __launch_bounds__(64) void x3_reduce_kernel(const float* __restrict__ partial, int num_wg, int seg_count,
                                                        int tiles_per_head, int tiles_per_wg, int k, int h, float* __restrict__ out,
                                                        const int* __restrict__ vl = nullptr, int direct_bags = 0) {
    constexpr int NCB = DK / 32, TILES = NKB * NCB;
    if (vl) {   // varlen: blockIdx.z = bag
        const int* __restrict__ dsc = vl + VL_DESC * blockIdx.z;
        if (dsc[10] && direct_bags) return;   // the main kernel stored this bag's heads itself
        tiles_per_head = dsc[4], tiles_per_wg = dsc[5], seg_count = dsc[7], num_wg = dsc[9];
        partial += (int64_t)dsc[8] * TILES * 1024;
        out += (int64_t)dsc[3] * (h * DK);
    }
    const int a = blockIdx.y;
    const int unit = blockIdx.x;   // (tile, q4): one wave per workgroup, so that the 4 TILES h units spread over all CUs
    const int lane = threadIdx.x;
    const int t_idx = unit >> 2, q4 = unit & 3;
    if (32 * (t_idx / NCB) + 8 * q4 >= k) return;
    const int f_lo = a * tiles_per_head, f_hi = (a + 1) * tiles_per_head - 1;
    const int b_lo = f_lo / tiles_per_wg;
    int b_hi = f_hi / tiles_per_wg;
    if (b_hi > num_wg - 1) b_hi = num_wg - 1;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    const int64_t off = ((int64_t)(t_idx * 4 + q4) * 64 + lane) * 4;
    for (int b = b_lo; b <= b_hi; b += 16) {
        f32x4 v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            v[u] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (b + u <= b_hi) {
                const int seg = a - ((b + u) * tiles_per_wg) / tiles_per_head;
                v[u] = *reinterpret_cast<const f32x4*>(partial + ((int64_t)(b + u) * seg_count + seg) * (int64_t)TILES * 1024 + off);
            }
        }
#pragma unroll
        for (int u = 0; u < 16; ++u) s += v[u];
    }
    const int kb = t_idx / NCB, cbk = t_idx - kb * NCB;
    const int col = a * DK + 32 * cbk + (lane & 31);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int key = 32 * kb + i + 8 * q4 + 4 * (lane >> 5);
        if (key < k) out[(int64_t)key * (h * DK) + col] = s[i];
    }
}

inline bool x3_plan(int64_t n, int k, int h, int dk, X3Plan* pl, bool packed = false) {
    if (!(dk == 64 || dk == 128) || k < 1 || k > (dk == 128 ? 224 : 256) || n < 1) return false;
    const int need = (k + 31) / 32;
    const int opts[] = {2, 4, 7, 8};
    int sel = 0;
    for (int o : opts)
        if (o >= need && !(o == 8 && dk == 128)) {
            sel = o;
            break;
        }
    if (!sel) return false;
    pl->nkb = sel;
    // a bag inside a packed (varlen) launch: at least 16 tiles (1024 rows) per workgroup
    return snf_attn::make_tile_plan(n, h, TROWS, /*small_bag_tiles=*/16, packed, pl);
}

template <int DK, int NKB, bool AUX, int MODE, bool VL = false, bool DROP = false>
int x3_launch(const X3Params& P, const X3Plan& pl, float* out, hipStream_t s) {
    constexpr int NKS = DK / 16;
    constexpr int q_bytes = (TROWS / 32) * NKS * 1024, p_bytes = TROWS * p_row_bytes(NKB), v_bytes = TROWS * 2 * DK;
    constexpr int lds = 2 * q_bytes + 2 * p_bytes + 4 * v_bytes + 8 * TROWS * 8;   // Q hi|lo, P hi|lo, V 2 x (hi|lo), statistics
    auto kern = sparse_attn_x3_kernel<DK, NKB, AUX, MODE, VL, DROP>;
    static thread_local unsigned long long attr_set_mask = 0;   // devices (bit = device id) that have the opt-in
    if (int rc = snf::lds_opt_in(reinterpret_cast<const void*>(kern), lds, &attr_set_mask, "sparse_attn_x3")) return rc;
    hipLaunchKernelGGL(kern, dim3(pl.num_wg), dim3(512), lds, s, P);
    int rc = snf::check_launch("sparse_attn_x3_kernel");
    if (rc || MODE == 1) return rc;
    constexpr int TILES = NKB * (DK / 32);
    if (VL && P.out_direct && pl.tiles_per_head == -1) return SNF_OK;   // every bag stored its heads itself (varlen_tile_plan)
    hipLaunchKernelGGL((x3_reduce_kernel<DK, NKB>), dim3(TILES * 4, P.h, VL ? P.vl_bags : 1), dim3(64), 0, s, P.partial, pl.num_wg,
                       pl.seg_count, pl.tiles_per_head, pl.tiles_per_wg, P.k, P.h, out, VL ? P.vl : nullptr,
                       (VL && P.out_direct) ? 1 : 0);
    return snf::check_launch("x3_reduce_kernel");
}
template <int DK>
int x3_dispatch_varlen(const X3Params& P, const X3Plan& pl, float* out, hipStream_t s) {
    const bool aux = P.attn != nullptr || P.lse != nullptr;
#define SNF_X3_VL_CASE(NB) \
    case NB: return aux ? x3_launch<DK, NB, true, 0, true>(P, pl, out, s) : x3_launch<DK, NB, false, 0, true>(P, pl, out, s);
    switch (pl.nkb) {
        SNF_X3_VL_CASE(2)
        SNF_X3_VL_CASE(4)
        SNF_X3_VL_CASE(7)
        case 8:
            if constexpr (DK == 64)
                return aux ? x3_launch<DK, 8, true, 0, true>(P, pl, out, s) : x3_launch<DK, 8, false, 0, true>(P, pl, out, s);
            break;
        default: break;
    }
#undef SNF_X3_VL_CASE
    snf::set_error("sparse_attn_x3 (varlen): key-block count %d not built", pl.nkb);
    return SNF_EUNSUPPORTED;
}
// key-block counts the key-chunked varlen launches are built for.  From x3_chunks: count >= 2 chunks of size = ceil(k / count) rounded up
// to a multiple of 4, with k > (count - 1) kmax, so size > kmax / 2 (dk = 128: 116 .. 224, dk = 64: 132 .. 256) and the last chunk
// k - (count - 1) size >= k / count - 4 (count - 1) > kmax (count - 1) / count - 4 (count - 1) >= kmax / 2 - 4 (108 / 124 keys at least):
// every chunk needs 4 .. 7 (dk = 64: 8) key blocks, which x3_plan serves with 4, 7 (and 8).  plan_varlen (attn_drive.h) checks every chunk of a
// launch against this set, and tests/test_varlen_chunks_host.py walks every k.
constexpr bool x3_varlen_chunk_built(int dk, int nkb) { return nkb == 4 || nkb == 7 || (nkb == 8 && dk == 64); }
template <int DK>
int x3_dispatch_varlen_chunk(const X3Params& P, const X3Plan& pl, float* out, hipStream_t s, int mode) {
    const bool aux = P.attn != nullptr || P.lse != nullptr;
#define SNF_X3_VLC_CASE(NB)                                                               \
    case NB:                                                                              \
        if (mode == 1) return x3_launch<DK, NB, false, 1, true>(P, pl, out, s);           \
        return aux ? x3_launch<DK, NB, true, 2, true>(P, pl, out, s) : x3_launch<DK, NB, false, 2, true>(P, pl, out, s);
    switch (pl.nkb) {
        SNF_X3_VLC_CASE(4)
        SNF_X3_VLC_CASE(7)
        case 8:
            if constexpr (DK == 64) {
                if (mode == 1) return x3_launch<DK, 8, false, 1, true>(P, pl, out, s);
                return aux ? x3_launch<DK, 8, true, 2, true>(P, pl, out, s) : x3_launch<DK, 8, false, 2, true>(P, pl, out, s);
            }
            break;
        default: break;
    }
#undef SNF_X3_VLC_CASE
    snf::set_error("sparse_attn_x3 (varlen, key chunks): key-block count %d not built", pl.nkb);
    return SNF_EUNSUPPORTED;
}
template <int DK, int NB>
int x3_modes(const X3Params& P, const X3Plan& pl, float* out, hipStream_t s, int mode) {
    const bool aux = P.attn != nullptr || P.lse != nullptr;
    if (mode == 1) return x3_launch<DK, NB, false, 1>(P, pl, out, s);
    if (mode == 2) return aux ? x3_launch<DK, NB, true, 2>(P, pl, out, s) : x3_launch<DK, NB, false, 2>(P, pl, out, s);
    return aux ? x3_launch<DK, NB, true, 0>(P, pl, out, s) : x3_launch<DK, NB, false, 0>(P, pl, out, s);
}
template <int DK>
int x3_dispatch_dropout(const X3Params& P, const X3Plan& pl, float* out, hipStream_t s) {
    switch (pl.nkb) {
        case 2: return x3_launch<DK, 2, true, 0, false, true>(P, pl, out, s);
        case 4: return x3_launch<DK, 4, true, 0, false, true>(P, pl, out, s);
        case 7: return x3_launch<DK, 7, true, 0, false, true>(P, pl, out, s);
        case 8:
            if constexpr (DK == 64) return x3_launch<DK, 8, true, 0, false, true>(P, pl, out, s);
            break;
        default: break;
    }
    snf::set_error("sparse_attn_x3 (dropout): key-block count %d not built", pl.nkb);
    return SNF_EUNSUPPORTED;
}
template <int DK>
int x3_dispatch(const X3Params& P, const X3Plan& pl, float* out, hipStream_t s, int mode) {
    switch (pl.nkb) {
        case 2: return x3_modes<DK, 2>(P, pl, out, s, mode);
        case 4: return x3_modes<DK, 4>(P, pl, out, s, mode);
        case 7: return x3_modes<DK, 7>(P, pl, out, s, mode);
        case 8:
            if constexpr (DK == 64) return x3_modes<DK, 8>(P, pl, out, s, mode);
            break;
        default: break;
    }
    snf::set_error("sparse_attn_x3: key-block count %d not built", pl.nkb);
    return SNF_EUNSUPPORTED;
}

// keys per launch: one LDS image holds kmax keys; more keys run as up to 8 chunks of equal size (a multiple of 4)
inline bool x3_chunks(int k, int dk, X3Chunks* c) {
    const int kmax = dk == 128 ? 224 : 256;
    if (!(dk == 64 || dk == 128) || k < 1 || k > 8 * kmax) return false;
    c->count = (k + kmax - 1) / kmax;
    c->size = c->count == 1 ? k : ((k + c->count - 1) / c->count + 3) & ~3;
    return c->size <= kmax;
}


// What every fp32-class driver shares of its family description (attn_drive.h lists the members)
struct X3Drive {
    using Params = X3Params;
    using Kp = float;
    static constexpr size_t ROUND = 1;
    static constexpr bool STAGE_KP = false, OFFSETS32 = false;
    static int kp(const float* kp, bool, int64_t, void*, hipStream_t, const float** used) { return *used = kp, SNF_OK; }
    // statistics [count][h][n_stride] of (max, sum) pairs: MODE 1 writes plane `chunk`, MODE 2 reads them all, MODE 0 none
    static void chunk(X3Params& P, bool, int c, int, int count, void* stats_area) {
        P.stats = reinterpret_cast<f32x2*>(stats_area), P.nchunks = count, P.chunk = c;
    }
    // ---- what the native-width shell (attn_width.h) asks of a family ----
    using In = float;                       // Q | V | Kp as the entry points take them
    static constexpr int ROW_ALIGN = 4;     // elements per 16 bytes of a Q | V row
    // the entry points take no Kp dtype: Kp is f32 and read as given
    static int open(const char*, int, X3Params&, bool* kp_f32) { return *kp_f32 = false, SNF_OK; }
    // the reduction pass behind a main launch
    template <int DK, int NKB>
    static int reduce(const X3Params& P, const X3Plan& pl, float* out, bool vl, hipStream_t s) {
        hipLaunchKernelGGL((x3_reduce_kernel<DK, NKB>), dim3(NKB * (DK / 32) * 4, P.h, vl ? P.vl_bags : 1), dim3(64), 0, s, P.partial, pl.num_wg,
                           pl.seg_count, pl.tiles_per_head, pl.tiles_per_wg, P.k, P.h, out, vl ? P.vl : nullptr, (vl && P.out_direct) ? 1 : 0);
        return snf::check_launch("x3_reduce_kernel");
    }
};

// What the native-width kernels of the family (192: sparse_attn_x3_dk192_impl.h, 256: sparse_attn_x3_dk256_impl.h) share of their width
// description: 128 keys per launch in up to 8 chunks of equal size (a multiple of 4), and how their entry points word a refusal.
// count >= 2: k > 128 (count - 1), so size >= 68 (3 or 4 blocks -> 4) and the last chunk k - (count - 1) size holds 61 keys at least
// (2, 3 or 4 blocks -> 2 or 4): chunked launches run at 2 or 4 key blocks
struct X3Wide {
    using Drive = X3Drive;
    static constexpr int KMAX = 128, MAX_CHUNKS = 8, CHUNK_MULTIPLE = 4;
    static constexpr int64_t MAX_ROWS = INT64_MAX;   // no row limit of the family's own
    static constexpr bool SHORT_TABLE_UNSUPPORTED = false;
    static bool plan_args_ok(int bags, int, int h) { return bags >= 1 && h >= 1; }   // k < 1: an unsupported shape there
    static bool varlen_shape_ok(int bags, int, int h) { return bags >= 1 && h >= 1; }
    static void refuse_bag(const char* me, int64_t, int k) {
        snf::set_error("%s: unsupported shape k=%d (k <= %d x %d)", me, k, MAX_CHUNKS, KMAX);
    }
    static void refuse_plan(const char* me, int bags, int k, int) {
        snf::set_error("%s: unsupported shape (bags=%d k=%d: need 1 <= k <= %d = %d chunks of %d, non-empty bags)", me, bags, k,
                       MAX_CHUNKS * KMAX, MAX_CHUNKS, KMAX);
    }
};

}  // namespace

namespace snf {
// sparse_attn_x3_varlen_chunks.hip: one chunk's statistics pass (mode 1) or main pass (mode 2) of a key-chunked varlen launch
int x3_launch_varlen_chunk(int dk, int mode, const snf_attn::X3Params& P, const snf_attn::TilePlan& pl, float* out, hipStream_t s);
}  // namespace snf
