// K7-bwd (fast form): backward of Snuffy's sparse attention on the CDNA4 matrix cores (bf16 operands, fp32 accumulate).
//
//   forward (snuffy.py:160-168), per head a:   P = softmax_j(Q Kp^T * scale) [n, k],  Pd = P o M,  O = Pd^T V [k, dk]
//   backward, with the saved row log-sum-exp (P is recomputed, never read back):
//       dV = Pd dO              [n, dk]          dP = (V dO^T) o M           [n, k]
//       D  = rowsum(P o dP)     [n]              dS = P o (dP - D) * scale   [n, k]
//       dQ = dS Kp              [n, dk]          dKp = dS^T Q                [k, dk]   (not here: dS is written out and the
//                                                                                       forward's P^T V machinery contracts it)
//
// Dataflow of one wave = 32 query rows of one head, all products with v_mfma_f32_32x32x16_bf16 in the "swapped" form of the
// forward kernel (this lane's ONE query row on the lane axis, keys / columns in registers):
//   S^T  = Kp  Q^T     A = Kp fragment  (LDS image, 16-byte row reads),  B = Q fragment (HBM -> registers)
//   dP^T = dO  V^T     A = dO fragment  (LDS image, 16-byte row reads),  B = V fragment (HBM -> registers)
//   P, dP -> bf16 pairs in registers for all key blocks; D = sum_j P dP is register-local + one cross-half exchange
//   dV^T = dO^T Pd^T   A = dO^T fragment (SAME image, hardware transpose-read),  B = Pd^T straight from the registers
//   dQ^T = Kp^T dS^T   A = Kp^T fragment (SAME image, hardware transpose-read),  B = dS^T straight from the registers
// so P, dP and dS never touch LDS, the waves of a workgroup never synchronise inside a head, and dV / dQ rows are owned by
// one wave (no cross-workgroup reduction).  The Kp and dO images are row-major bf16 [key][dk]; the 16-byte chunks of a row
// are permuted by the row index (img_pos below), which makes BOTH access patterns bank-conflict-free: the 16-lane groups of a ds_read_b128 (16 different rows) and the 32-lane groups of a
// ds_read_b64_tr_b16 (4 consecutive rows x 64 bytes).
#include <math.h>
#include <stdlib.h>

#include "mfma.h"
#include "philox.h"

namespace {

constexpr int TILE_ROWS = 128;  // query rows per workgroup step (4 waves x 32)

struct BwdParams {
    const void* q;      // [n, ldq]
    const void* v;      // [n, ldv]
    const float* kp;    // [k, d] f32
    const float* dout;  // [k, d] f32
    const float* lse;   // [h, n]   log-sum-exp of the scaled scores (forward)
    const float* mask;  // [h, n, k] dropout keep-mask / (1 - p), or null
    int64_t n, ldq, ldv, d;
    int k, h;
    float scale;
    void* dq;   // [n, ldd] f32 or bf16 (dqv_bf16)
    void* dv;   // [n, ldd]
    int64_t ldd;
    int dqv_bf16;
    void* ds;   // [h, n, k] f32, or bf16 when ds_bf16 (the caller then contracts it with a bf16 library GEMM)
    int ds_bf16;
    int tiles_per_head, tiles_per_wg, total_tiles;
    snf::DropoutState drop;   // mask regenerated in registers when thresh != 0 (and mask == null): same stream as the forward
};

__device__ __forceinline__ unsigned pack2(float a, float b) {
    return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{a, b}, bf16x2));
}
__device__ __forceinline__ float lo_f(unsigned u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float hi_f(unsigned u) { return __uint_as_float(u & 0xffff0000u); }

// chunk position inside an image row of 2*DK bytes (DK/8 chunks of 16 bytes = DK/32 blocks of 64 bytes): the block index is
// rotated by the row (so the 4 consecutive rows x 64 bytes of a transpose-read group fall into 4 different 64-byte bank
// quarters: r & 3 for 256-byte rows, (r >> 1) & 1 for 128-byte rows, whose rows already alternate halves), the chunk inside
// the block is XOR-ed with (r >> 2) & 3 (so the 16 rows of a ds_read_b128 service group hit 16 different bank quads).
// 384-byte rows (DK = 192, the chunked kernel only) are one and a half bank rows: row r starts at bank 32 r mod 64, so the 64-byte
// block at block position b covers the bank quarter (2 r + b) mod 4.  Block cb goes to position cb ^ ((r >> 1) & 1) (an XOR of the low
// bit stays inside the row's 6 blocks): rows r0 .. r0 + 3 of a transpose-read group then use the quarters cb, cb + 2, cb ^ 1,
// (cb ^ 1) + 2 (mod 4) -- four different ones, each bank once.  For a ds_read_b128 service group the 16-byte slot (of 16 per bank row)
// is 4 * quarter + ((c & 3) ^ ((r >> 2) & 3)): the quarter is a bijection of r & 3, and the rows of a group that agree in r & 3
// ({0, 12, 20, 24}, {4, 8, 16, 28}, ...) have four different (r >> 2) & 3 -- 16 rows, 16 slots.  Everything is periodic in 16 rows
// (16 * 384 bytes = 24 bank rows), which the fragment addresses below rely on.
// 512-byte rows (DK = 256, the chunked kernel only) are TWO whole bank rows: every row starts at bank 0, and the 64-byte block at block
// position b covers the bank quarter b mod 4 whatever the row.  Block cb goes to position (cb + (r & 3)) mod 8, a rotation over the
// row's 8 blocks (the generic branch below would rotate by (r >> 1) & 1, the rule of 128-byte rows: rows r0 and r0 + 1 of a transpose-read
// group would then share a quarter).  Transpose read: rows r0 .. r0 + 3 (r0 a multiple of 4) x the same block cb use the quarters cb,
// cb + 1, cb + 2, cb + 3 (mod 4), and inside a quarter the 8 lanes of a row read its four 16-byte chunks in two 8-byte halves -- every
// bank once.  ds_read_b128: the 16-byte slot (of 16 per bank row) is 4 * quarter + ((c & 3) ^ ((r >> 2) & 3)); all lanes of a service
// group read the same chunk c, the quarter ((c >> 2) + (r & 3)) mod 4 is a bijection of r & 3, and the rows of a group that agree in
// r & 3 ({0, 12, 20, 24}, {4, 8, 16, 28}, ...) have four different (r >> 2) & 3 -- 16 rows, 16 slots.  Periodic in 16 rows as well.
template <int DK>
__device__ __forceinline__ int img_pos(int row, int c) {
    if constexpr (DK == 192) return 4 * ((c >> 2) ^ ((row >> 1) & 1)) + ((c & 3) ^ ((row >> 2) & 3));
    if constexpr (DK == 256) return 4 * (((c >> 2) + (row & 3)) & 7) + ((c & 3) ^ ((row >> 2) & 3));
    const int rot = DK == 128 ? (row & 3) : ((row >> 1) & 1);
    return 4 * (((c >> 2) + rot) & (DK / 32 - 1)) + ((c & 3) ^ ((row >> 2) & 3));
}

// MODE 0: every option at run time (mask tensor, fp32 dS, K not a multiple of 4).  MODE 1 / 2: the training path's shape --
// bf16 dS, K % 4 == 0, no mask tensor -- without (1) / with (2) the in-register Philox mask.  The fast modes drop the per-store
// predicates of full key blocks, compare against K only in the last block, and (2) generate the mask ONCE: a dropped key is
// remembered in the sign bit of its bf16 probability (P >= 0), so the second use costs a max instead of ten Philox rounds.
template <int DK, int NKB, typename QT, int MODE>
__global__ __launch_bounds__(256, 1) void sparse_attn_bwd_mfma_kernel(BwdParams P) {
    constexpr bool FAST = MODE != 0;
    constexpr int NKS = DK / 16, NCB = DK / 32, RP = 2 * DK, NCH = DK / 8;   // k-steps, column blocks, image row pitch, chunks
    constexpr int IMG = 32 * NKB * RP;   // bytes of one image
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* img_kp = smem;
    unsigned char* img_do = smem + IMG;

    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = lane & 31, hf = lane >> 5;
    const QT* __restrict__ q = reinterpret_cast<const QT*>(P.q);
    const QT* __restrict__ vg = reinterpret_cast<const QT*>(P.v);
    const float c_exp = P.scale * 1.44269504088896340736f;
    const int n32 = (int)P.n;
    const int prow = 32 * w + j;

    // A fragments with the KEY on the lane (S^T, dP^T): row 32 jb + j, 16-byte chunk 2 kb + hf
    int ra[NKS];
#pragma unroll
    for (int kb = 0; kb < NKS; ++kb) ra[kb] = j * RP + 16 * img_pos<DK>(j, 2 * kb + hf);
    // A fragments with the COLUMN on the lane (dV^T, dQ^T), by transpose-read: 16-lane group tg, lane ti in it;
    // rows k_base + 4 (tg >> 1) + (ti >> 2) (+8 for the second read), chunk 4 db + 2 (tg & 1) + ((ti & 3) >> 1), half ti & 1
    const int tg = lane >> 4, ti = lane & 15;
    int rt0[NCB], rt1[NCB];
#pragma unroll
    for (int db = 0; db < NCB; ++db) {
        const int r0 = 4 * (tg >> 1) + (ti >> 2), r1 = r0 + 8;
        const int c = 4 * db + 2 * (tg & 1) + ((ti & 3) >> 1);
        rt0[db] = r0 * RP + 16 * img_pos<DK>(r0, c) + 8 * (ti & 1);
        rt1[db] = r1 * RP + 16 * img_pos<DK>(r1, c) + 8 * (ti & 1);
    }

    const int f_begin = blockIdx.x * P.tiles_per_wg;
    int f_end = f_begin + P.tiles_per_wg;
    if (f_end > P.total_tiles) f_end = P.total_tiles;
    int a = f_begin / P.tiles_per_head, t = f_begin - a * P.tiles_per_head;
    int cur_head = -1;

    for (int f = f_begin; f < f_end; ++f) {
        if (a != cur_head) {
            // Kp_a and dO_a -> LDS (bf16, row-major, swizzled): thread -> (row, chunk), a row's 512 bytes are read coalesced
            __syncthreads();
            for (int ci = threadIdx.x; ci < 32 * NKB * NCH; ci += 256) {
                const int row = ci / NCH, c = ci % NCH;
                u32x4 vk = {0u, 0u, 0u, 0u}, vo = {0u, 0u, 0u, 0u};
                if (row < P.k) {
                    vk = __builtin_bit_cast(u32x4, load_frag(P.kp + (int64_t)row * P.d + a * DK + 8 * c));
                    vo = __builtin_bit_cast(u32x4, load_frag(P.dout + (int64_t)row * P.d + a * DK + 8 * c));
                }
                const int off = row * RP + 16 * img_pos<DK>(row, c);
                *reinterpret_cast<u32x4*>(img_kp + off) = vk;
                *reinterpret_cast<u32x4*>(img_do + off) = vo;
            }
            __syncthreads();
            cur_head = a;
        }
        const int row = t * TILE_ROWS + prow;
        const bool rvalid = row < n32;
        const int lrow = rvalid ? row : n32 - 1;
        // B operands: this lane's row of Q and V, 8 consecutive columns per k-step
        bf16x8 qf[NKS], vf[NKS];
        {
            const QT* qp = q + (int64_t)lrow * P.ldq + a * DK + 8 * hf;
            const QT* vp = vg + (int64_t)lrow * P.ldv + a * DK + 8 * hf;
            static_for<0, NKS>([&](auto kb) __attribute__((always_inline)) {
                qf[kb] = load_frag(qp + 16 * kb);
                vf[kb] = load_frag(vp + 16 * kb);
            });
        }
        // rows past the bag end get P = 0 (exp2(-inf))
        const float lse2 = rvalid ? P.lse[(int64_t)a * P.n + row] * 1.44269504088896340736f : INFINITY;
        const float* mrow = P.mask ? P.mask + ((int64_t)a * P.n + lrow) * P.k : nullptr;
        int kk = P.k;
        asm volatile("" : "+s"(kk));

        unsigned ppk[NKB][8], dpk[NKB][8];   // Pd (= P o M) and dP (o M), later dS, as bf16 pairs: [block][pair of registers]
        float dsum = 0.f;
        static_for<0, NKB>([&](auto jb_t) __attribute__((always_inline)) {
            constexpr int jb = decltype(jb_t)::value;
            f32x16 s, dp;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                // padded keys: P = 0.  Only the last block can hold any; kk is opaque so that the compare masks are not hoisted
                // out of the tile loop (16 NKB SGPR pairs: that was 225 spilled SGPRs)
                if (!FAST || jb == NKB - 1)
                    s[r] = (32 * jb + (r & 3) + 8 * (r >> 2) + 4 * hf >= kk) ? -INFINITY : 0.f;
                else
                    s[r] = 0.f;
                dp[r] = 0.f;
            }
            static_for<0, NKS>([&](auto kb_t) __attribute__((always_inline)) {
                constexpr int kb = decltype(kb_t)::value;
                const bf16x8 ak = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(img_kp + ra[kb] + jb * 32 * RP));
                const bf16x8 ao = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(img_do + ra[kb] + jb * 32 * RP));
                s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ak, qf[kb], s, 0, 0, 0);
                dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ao, vf[kb], dp, 0, 0, 0);
            });
#pragma unroll
            for (int c4 = 0; c4 < 4; ++c4) {
                float pv[4], gv[4];
                f32x4 mk = {1.f, 1.f, 1.f, 1.f};
                if constexpr (MODE == 0) {
                    if (mrow) {
                        const int key0 = 32 * jb + 8 * c4 + 4 * hf;
#pragma unroll
                        for (int e = 0; e < 4; ++e) mk[e] = (key0 + e < P.k) ? mrow[key0 + e] : 0.f;
                    } else if (P.drop.thresh) {
                        const snf::philox_f4 m4 = snf::dropout_mask4(P.drop, a, P.n, lrow, P.k, 32 * jb + 8 * c4 + 4 * hf);
                        mk = f32x4{m4[0], m4[1], m4[2], m4[3]};
                    }
                } else if constexpr (MODE == 2) {
                    const snf::philox_f4 m4 = snf::dropout_mask4(P.drop, a, P.n, lrow, P.k, 32 * jb + 8 * c4 + 4 * hf);
                    mk = f32x4{m4[0], m4[1], m4[2], m4[3]};
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    pv[e] = __builtin_amdgcn_exp2f(fmaf(s[4 * c4 + e], c_exp, -lse2));
                    gv[e] = dp[4 * c4 + e] * mk[e];          // dP = dPd o M
                    if constexpr (MODE == 2) pv[e] = mk[e] == 0.f ? -pv[e] : pv[e];   // dropped: remembered in the sign
                }
                // ppk holds P (un-masked: dS = P o (dP - D)); the masked Pd for dV is rebuilt from it below when a mask exists
                const unsigned p01 = pack2(pv[0], pv[1]), p23 = pack2(pv[2], pv[3]);
                const unsigned g01 = pack2(gv[0], gv[1]), g23 = pack2(gv[2], gv[3]);
                ppk[jb][2 * c4] = p01;
                ppk[jb][2 * c4 + 1] = p23;
                dpk[jb][2 * c4] = g01;
                dpk[jb][2 * c4 + 1] = g23;
                // D += P dP on the ROUNDED values, the ones dS is built from below: sum_j dS_j stays 0 to fp32 accuracy
                dsum = fmaf(lo_f(p01), lo_f(g01), dsum);
                dsum = fmaf(hi_f(p01), hi_f(g01), dsum);
                dsum = fmaf(lo_f(p23), lo_f(g23), dsum);
                dsum = fmaf(hi_f(p23), hi_f(g23), dsum);
            }
            // keep the key blocks apart: interleaved, the scheduler holds every block's 32 accumulator registers live at once
            // (512 registers + 190 spilled before this fence, profiles/history/r02_attn_bwd_resources.txt)
            __builtin_amdgcn_sched_barrier(0);
        });
        const float dtot = xhalf_sum(dsum);

        // dS = P o (dP - D) * scale: written out (fp32, for dKp) and kept as bf16 pairs for dQ; Pd = P o M for dV
        float* dsrow = reinterpret_cast<float*>(P.ds) + ((int64_t)a * P.n + lrow) * P.k;
        unsigned short* dsrow16 = reinterpret_cast<unsigned short*>(P.ds) + ((int64_t)a * P.n + lrow) * P.k;
        if constexpr (FAST) {
            // rows past the bag end skip the whole pass (their registers feed accumulators that are never stored)
            if (rvalid) {
                static_for<0, NKB>([&](auto jb_t) __attribute__((always_inline)) {
                    constexpr int jb = decltype(jb_t)::value;
#pragma unroll
                    for (int c4 = 0; c4 < 4; ++c4) {
                        const unsigned p01 = ppk[jb][2 * c4], p23 = ppk[jb][2 * c4 + 1];
                        const unsigned g01 = dpk[jb][2 * c4], g23 = dpk[jb][2 * c4 + 1];
                        const float pv[4] = {lo_f(p01), hi_f(p01), lo_f(p23), hi_f(p23)};
                        const float gv[4] = {lo_f(g01), hi_f(g01), lo_f(g23), hi_f(g23)};
                        f32x4 dsv;
#pragma unroll
                        for (int e = 0; e < 4; ++e) dsv[e] = fabsf(pv[e]) * (gv[e] - dtot) * P.scale;
                        const int key0 = 32 * jb + 8 * c4 + 4 * hf;
                        const unsigned s01 = pack2(dsv[0], dsv[1]), s23 = pack2(dsv[2], dsv[3]);
                        if (jb < NKB - 1 || key0 < kk) *reinterpret_cast<uint2*>(dsrow16 + key0) = uint2{s01, s23};
                        dpk[jb][2 * c4] = s01;
                        dpk[jb][2 * c4 + 1] = s23;
                        if constexpr (MODE == 2) {   // Pd = P o M: kept keys scaled, dropped keys (negative sign) -> 0
                            ppk[jb][2 * c4] = pack2(fmaxf(pv[0], 0.f) * P.drop.scale, fmaxf(pv[1], 0.f) * P.drop.scale);
                            ppk[jb][2 * c4 + 1] = pack2(fmaxf(pv[2], 0.f) * P.drop.scale, fmaxf(pv[3], 0.f) * P.drop.scale);
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);
                });
            }
        } else {
        const bool vec_ok = (P.k & 3) == 0;
        static_for<0, NKB>([&](auto jb_t) __attribute__((always_inline)) {
            constexpr int jb = decltype(jb_t)::value;
#pragma unroll
            for (int c4 = 0; c4 < 4; ++c4) {
                const unsigned p01 = ppk[jb][2 * c4], p23 = ppk[jb][2 * c4 + 1];
                const unsigned g01 = dpk[jb][2 * c4], g23 = dpk[jb][2 * c4 + 1];
                const float pv[4] = {lo_f(p01), hi_f(p01), lo_f(p23), hi_f(p23)};
                const float gv[4] = {lo_f(g01), hi_f(g01), lo_f(g23), hi_f(g23)};
                f32x4 dsv;
#pragma unroll
                for (int e = 0; e < 4; ++e) dsv[e] = pv[e] * (gv[e] - dtot) * P.scale;
                const int key0 = 32 * jb + 8 * c4 + 4 * hf;
                const unsigned s01 = pack2(dsv[0], dsv[1]), s23 = pack2(dsv[2], dsv[3]);
                if (rvalid) {
                    if (P.ds_bf16) {
                        if (vec_ok) {
                            if (key0 < P.k) *reinterpret_cast<uint2*>(dsrow16 + key0) = uint2{s01, s23};
                        } else {
                            const unsigned short hv[4] = {(unsigned short)(s01 & 0xffffu), (unsigned short)(s01 >> 16),
                                                          (unsigned short)(s23 & 0xffffu), (unsigned short)(s23 >> 16)};
#pragma unroll
                            for (int e = 0; e < 4; ++e)
                                if (key0 + e < P.k) dsrow16[key0 + e] = hv[e];
                        }
                    } else if (vec_ok) {
                        if (key0 < P.k) *reinterpret_cast<f32x4*>(dsrow + key0) = dsv;
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (key0 + e < P.k) dsrow[key0 + e] = dsv[e];
                    }
                }
                dpk[jb][2 * c4] = s01;
                dpk[jb][2 * c4 + 1] = s23;
                if (mrow) {
                    float mk[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) mk[e] = (key0 + e < P.k) ? mrow[key0 + e] : 0.f;
                    ppk[jb][2 * c4] = pack2(pv[0] * mk[0], pv[1] * mk[1]);
                    ppk[jb][2 * c4 + 1] = pack2(pv[2] * mk[2], pv[3] * mk[3]);
                } else if (P.drop.thresh) {   // the mask is regenerated (second use): 4 keys per Philox call
                    const snf::philox_f4 m4 = snf::dropout_mask4(P.drop, a, P.n, lrow, P.k, key0);
                    ppk[jb][2 * c4] = pack2(pv[0] * m4[0], pv[1] * m4[1]);
                    ppk[jb][2 * c4 + 1] = pack2(pv[2] * m4[2], pv[3] * m4[3]);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        });
        }

        // dV^T[col, row] += dO^T Pd^T ;  dQ^T[col, row] += Kp^T dS^T : k-step = 16 keys (registers 8u .. 8u+7 of block jb)
        f32x16 acc_v[NCB], acc_q[NCB];
#pragma unroll
        for (int db = 0; db < NCB; ++db)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc_v[db][r] = acc_q[db][r] = 0.f;
        static_for<0, NKB>([&](auto jb_t) __attribute__((always_inline)) {
            constexpr int jb = decltype(jb_t)::value;
            static_for<0, 2>([&](auto u_t) __attribute__((always_inline)) {
                constexpr int u = decltype(u_t)::value;
                const u32x4 pb = {ppk[jb][4 * u], ppk[jb][4 * u + 1], ppk[jb][4 * u + 2], ppk[jb][4 * u + 3]};
                const u32x4 sb = {dpk[jb][4 * u], dpk[jb][4 * u + 1], dpk[jb][4 * u + 2], dpk[jb][4 * u + 3]};
                constexpr int koff = (32 * jb + 16 * u) * RP;
                static_for<0, NCB>([&](auto db_t) __attribute__((always_inline)) {
                    constexpr int db = decltype(db_t)::value;
                    const bf16x8 ao = tr_frag(img_do + rt0[db] + koff, img_do + rt1[db] + koff);
                    const bf16x8 ak = tr_frag(img_kp + rt0[db] + koff, img_kp + rt1[db] + koff);
                    acc_v[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ao, __builtin_bit_cast(bf16x8, pb), acc_v[db], 0, 0, 0);
                    acc_q[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ak, __builtin_bit_cast(bf16x8, sb), acc_q[db], 0, 0, 0);
                });
            });
        });
        // C layout of X^T[col, row]: lane = row, registers = columns 32 db + (r & 3) + 8 (r >> 2) + 4 hf -> 16-byte stores
        if (rvalid && !P.dqv_bf16) {
            float* dvp = reinterpret_cast<float*>(P.dv) + (int64_t)row * P.ldd + a * DK + 4 * hf;
            float* dqp = reinterpret_cast<float*>(P.dq) + (int64_t)row * P.ldd + a * DK + 4 * hf;
#pragma unroll
            for (int db = 0; db < NCB; ++db)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    *reinterpret_cast<f32x4*>(dvp + 32 * db + 8 * g) =
                        f32x4{acc_v[db][4 * g], acc_v[db][4 * g + 1], acc_v[db][4 * g + 2], acc_v[db][4 * g + 3]};
                    *reinterpret_cast<f32x4*>(dqp + 32 * db + 8 * g) =
                        f32x4{acc_q[db][4 * g], acc_q[db][4 * g + 1], acc_q[db][4 * g + 2], acc_q[db][4 * g + 3]};
                }
        }
        if (rvalid && P.dqv_bf16) {   // gradients leave as bf16 (operands of the weight-gradient GEMMs), 8-byte stores
            unsigned short* dvp = reinterpret_cast<unsigned short*>(P.dv) + (int64_t)row * P.ldd + a * DK + 4 * hf;
            unsigned short* dqp = reinterpret_cast<unsigned short*>(P.dq) + (int64_t)row * P.ldd + a * DK + 4 * hf;
#pragma unroll
            for (int db = 0; db < NCB; ++db)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    uint2 pv, pq;
                    pv.x = pack_bf16x2(acc_v[db][4 * g], acc_v[db][4 * g + 1]);
                    pv.y = pack_bf16x2(acc_v[db][4 * g + 2], acc_v[db][4 * g + 3]);
                    pq.x = pack_bf16x2(acc_q[db][4 * g], acc_q[db][4 * g + 1]);
                    pq.y = pack_bf16x2(acc_q[db][4 * g + 2], acc_q[db][4 * g + 3]);
                    *reinterpret_cast<uint2*>(dvp + 32 * db + 8 * g) = pv;
                    *reinterpret_cast<uint2*>(dqp + 32 * db + 8 * g) = pq;
                }
        }
        if (++t == P.tiles_per_head) {
            t = 0;
            ++a;
        }
    }
}

struct BwdPlan {
    int num_wg, tiles_per_head, tiles_per_wg, total_tiles, nkb;
};
inline bool make_bwd_plan(int64_t n, int k, int h, int dk, BwdPlan* pl) {
    if (!((dk == 128 && k <= 224) || (dk == 64 && k <= 256)) || k < 1 || n < 1 || n > 0x7fffff00ll) return false;
    const int nkb = (k + 31) / 32;
    const int64_t tph = (n + TILE_ROWS - 1) / TILE_ROWS, total = tph * h;
    if (total > 0x7fffffff) return false;
    const int cus = snf::cu_count();
    int64_t num_wg = total < cus ? total : cus;
    const int64_t tpw = (total + num_wg - 1) / num_wg;
    num_wg = (total + tpw - 1) / tpw;
    *pl = {(int)num_wg, (int)tph, (int)tpw, (int)total, nkb};
    return true;
}

template <int DK, int NKB, typename QT, int MODE>
int launch_bwd_mode(const BwdParams& P, const BwdPlan& pl, hipStream_t s) {
    const size_t lds = (size_t)2 * 32 * NKB * 2 * DK;
    auto kern = sparse_attn_bwd_mfma_kernel<DK, NKB, QT, MODE>;
    static thread_local unsigned long long attr_set_mask = 0;   // devices (bit = device id) that have the opt-in
    if (int rc = snf::lds_opt_in(reinterpret_cast<const void*>(kern), lds, &attr_set_mask, "sparse_attn_bwd_mfma")) return rc;
    hipLaunchKernelGGL(kern, dim3(pl.num_wg), dim3(256), lds, s, P);
    return snf::check_launch("sparse_attn_bwd_mfma_kernel");
}
template <int DK, int NKB, typename QT>
int launch_bwd(const BwdParams& P, const BwdPlan& pl, hipStream_t s) {
    if constexpr (std::is_same<QT, unsigned short>::value) {   // the training path: bf16 operands, bf16 dS, K % 4 == 0
        if (P.ds_bf16 && !P.mask && (P.k & 3) == 0)
            return P.drop.thresh ? launch_bwd_mode<DK, NKB, QT, 2>(P, pl, s) : launch_bwd_mode<DK, NKB, QT, 1>(P, pl, s);
    }
    return launch_bwd_mode<DK, NKB, QT, 0>(P, pl, s);
}
template <int DK, typename QT>
int launch_bwd_nkb(const BwdParams& P, const BwdPlan& pl, hipStream_t s) {
    switch (pl.nkb) {
        case 1: return launch_bwd<DK, 1, QT>(P, pl, s);
        case 2: return launch_bwd<DK, 2, QT>(P, pl, s);
        case 3: return launch_bwd<DK, 3, QT>(P, pl, s);
        case 4: return launch_bwd<DK, 4, QT>(P, pl, s);
        case 5: return launch_bwd<DK, 5, QT>(P, pl, s);
        case 6: return launch_bwd<DK, 6, QT>(P, pl, s);
        case 7: return launch_bwd<DK, 7, QT>(P, pl, s);
        default:
            if constexpr (DK == 64) return launch_bwd<DK, 8, QT>(P, pl, s);
            snf::set_error("sparse_attn_bwd_mfma: key-block count %d not built", pl.nkb);
            return SNF_EUNSUPPORTED;
    }
}


// ---- more keys than one pair of LDS images holds: the backward over key chunks ------------------------------------------------------
// The forward's lse is GLOBAL (all keys), so P of any chunk is recomputed on its own; what needs all keys is D = rowsum(P o dP) and
// the sums dV, dQ.  Two series of launches, one launch per chunk each (the forward's "statistics pass, then main pass"):
//   series A   S -> P -> Pd = P o M -> dV += dO^T Pd^T                      the last launch also takes D = V . dV per head and row:
//                                                                           D = sum_j Pd_j (V . dO_j) = V . sum_j Pd_j dO_j, mask or not
//   series B   S, dP = (V dO^T) o M, dS = P o (dP - D) * scale -> column k0 of the full-width dS, dQ += Kp^T dS^T
// The running sums live in fp32 between the launches (the caller's dq / dv when those are fp32, else the workspace): a wave owns
// its rows in every launch and the chunks are added in launch order -- no atomics, one summation order.  Nothing is kept per key
// block across blocks (P or dS of a block goes straight into its MFMAs), so the block loop is a run-time loop and one kernel
// serves every chunk length; 8 waves per workgroup (two per SIMD) overlap one wave's exponentials with the other's MFMAs.
// The mask is keyed on the GLOBAL key index and the total key count, in registers (Philox) or from the [h, n, k] tensor; each
// series uses it once, so the single-chunk kernel's sign-bit memory has nothing to save here.
// dk = 192: 4 waves (one per SIMD, 512 registers each).  A row's 6 accumulators (96 registers) next to the Q and V fragments (48 + 48 in
// series B) and s / dp (32) do not fit the 256 registers of two waves per SIMD: series B spilled 63 - 119 registers that way.
// dk = 256: 4 waves for the same reason (8 accumulators = 128 registers, Q and V fragments 64 + 64, s / dp 32).
constexpr int ch_waves(int dk) { return dk == 192 || dk == 256 ? 4 : 8; }
// widths the single-launch kernel above is built for; the others (192, 256) run one chunk on the chunked kernel too
constexpr bool bwd_single_launch(int dk) { return dk == 64 || dk == 128; }

struct ChunkParams {
    BwdParams b;        // kp / dout point at the chunk's first key, b.k = keys of THIS chunk; mask / ds at column 0 of the full rows
    int k0, k_total;    // first key of the chunk, keys of all chunks
    int nkb;            // key blocks of this chunk
    int first, last;    // first / last launch of the series
    float* acc;         // [n, ldacc] f32 running sum of the series (dV in A, dQ in B)
    int64_t ldacc;
    float* dsum;        // [h, n] D: written by the last launch of series A, read by series B
};

__device__ __forceinline__ void load4_bf16(const float* p, float (&o)[4]) {   // rounded as the MFMA operand is (load_frag)
    const f32x4 x = *reinterpret_cast<const f32x4*>(p);
    const unsigned a = pack2(x[0], x[1]), b = pack2(x[2], x[3]);
    o[0] = lo_f(a), o[1] = hi_f(a), o[2] = lo_f(b), o[3] = hi_f(b);
}
__device__ __forceinline__ void load4_bf16(const unsigned short* p, float (&o)[4]) {
    const uint2 x = *reinterpret_cast<const uint2*>(p);
    o[0] = lo_f(x.x), o[1] = hi_f(x.x), o[2] = lo_f(x.y), o[3] = hi_f(x.y);
}

// SERIES 0 = A, 1 = B.  FAST (series B, the training path's shape): bf16 dS, K % 4 == 0, no mask tensor.
template <int DK, typename QT, int SERIES, bool FAST>
__global__ __launch_bounds__(64 * ch_waves(DK), 1) void sparse_attn_bwd_chunk_kernel(ChunkParams C) {
    constexpr int CH_WAVES = ch_waves(DK), CH_ROWS = 32 * CH_WAVES;
    const BwdParams& P = C.b;
    constexpr int NKS = DK / 16, NCB = DK / 32, RP = 2 * DK, NCH = DK / 8;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* img_kp = smem;
    unsigned char* img_do = smem + 32 * C.nkb * RP;
    // A operand of the second product: dO^T (series A, dV) or Kp^T (series B, dQ)
    const unsigned char* img_t = SERIES == 0 ? img_do : img_kp;

    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = lane & 31, hf = lane >> 5;
    const QT* __restrict__ q = reinterpret_cast<const QT*>(P.q);
    const QT* __restrict__ vg = reinterpret_cast<const QT*>(P.v);
    const float c_exp = P.scale * 1.44269504088896340736f;
    const int n32 = (int)P.n;
    const int prow = 32 * w + j;

    int ra[NKS];   // see sparse_attn_bwd_mfma_kernel: the same images, the same fragment addresses
#pragma unroll
    for (int kb = 0; kb < NKS; ++kb) ra[kb] = j * RP + 16 * img_pos<DK>(j, 2 * kb + hf);
    const int tg = lane >> 4, ti = lane & 15;
    int rt0[NCB], rt1[NCB];
#pragma unroll
    for (int db = 0; db < NCB; ++db) {
        const int r0 = 4 * (tg >> 1) + (ti >> 2), r1 = r0 + 8;
        const int c = 4 * db + 2 * (tg & 1) + ((ti & 3) >> 1);
        rt0[db] = r0 * RP + 16 * img_pos<DK>(r0, c) + 8 * (ti & 1);
        rt1[db] = r1 * RP + 16 * img_pos<DK>(r1, c) + 8 * (ti & 1);
    }

    const int f_begin = blockIdx.x * P.tiles_per_wg;
    int f_end = f_begin + P.tiles_per_wg;
    if (f_end > P.total_tiles) f_end = P.total_tiles;
    int a = f_begin / P.tiles_per_head, t = f_begin - a * P.tiles_per_head;
    int cur_head = -1;

    for (int f = f_begin; f < f_end; ++f) {
        if (a != cur_head) {
            __syncthreads();
            for (int ci = threadIdx.x; ci < 32 * C.nkb * NCH; ci += 64 * CH_WAVES) {
                const int row = ci / NCH, c = ci % NCH;
                u32x4 vk = {0u, 0u, 0u, 0u}, vo = {0u, 0u, 0u, 0u};
                if (row < P.k) {
                    vk = __builtin_bit_cast(u32x4, load_frag(P.kp + (int64_t)row * P.d + a * DK + 8 * c));
                    vo = __builtin_bit_cast(u32x4, load_frag(P.dout + (int64_t)row * P.d + a * DK + 8 * c));
                }
                const int off = row * RP + 16 * img_pos<DK>(row, c);
                *reinterpret_cast<u32x4*>(img_kp + off) = vk;
                *reinterpret_cast<u32x4*>(img_do + off) = vo;
            }
            __syncthreads();
            cur_head = a;
        }
        const int row = t * CH_ROWS + prow;
        const bool rvalid = row < n32;
        const int lrow = rvalid ? row : n32 - 1;
        bf16x8 qf[NKS], vf[SERIES == 1 ? NKS : 1];
        {
            const QT* qp = q + (int64_t)lrow * P.ldq + a * DK + 8 * hf;
            const QT* vp = vg + (int64_t)lrow * P.ldv + a * DK + 8 * hf;
            static_for<0, NKS>([&](auto kb) __attribute__((always_inline)) {
                qf[kb] = load_frag(qp + 16 * kb);
                if constexpr (SERIES == 1) vf[kb] = load_frag(vp + 16 * kb);
            });
        }
        const float lse2 = rvalid ? P.lse[(int64_t)a * P.n + row] * 1.44269504088896340736f : INFINITY;   // rows past the end: P = 0
        const float* mrow = P.mask ? P.mask + ((int64_t)a * P.n + lrow) * C.k_total + C.k0 : nullptr;
        float dtot = 0.f;
        if constexpr (SERIES == 1) dtot = C.dsum[(int64_t)a * P.n + lrow];
        float* dsrow = reinterpret_cast<float*>(P.ds) + ((int64_t)a * P.n + lrow) * C.k_total + C.k0;
        unsigned short* dsrow16 = reinterpret_cast<unsigned short*>(P.ds) + ((int64_t)a * P.n + lrow) * C.k_total + C.k0;
        const bool vec_ok = (C.k_total & 3) == 0;   // chunk starts are multiples of 32

        // the running sum of the chunks before this one; C layout of X^T[col, row]: lane = row, registers = columns
        // 32 db + (r & 3) + 8 (r >> 2) + 4 hf
        f32x16 acc[NCB];
        float* accp = C.acc + (int64_t)lrow * C.ldacc + a * DK + 4 * hf;
#pragma unroll
        for (int db = 0; db < NCB; ++db)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                f32x4 x = {0.f, 0.f, 0.f, 0.f};
                if (!C.first && rvalid) x = *reinterpret_cast<const f32x4*>(accp + 32 * db + 8 * g);
                acc[db][4 * g] = x[0], acc[db][4 * g + 1] = x[1], acc[db][4 * g + 2] = x[2], acc[db][4 * g + 3] = x[3];
            }

#pragma unroll 1
        for (int jb = 0; jb < C.nkb; ++jb) {
            const int jo = jb * 32 * RP;
            const bool tail = jb == C.nkb - 1;   // only the last block holds padded keys: P = 0 there
            f32x16 s, dp;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                s[r] = (tail && 32 * jb + (r & 3) + 8 * (r >> 2) + 4 * hf >= P.k) ? -INFINITY : 0.f;
                dp[r] = 0.f;
            }
            static_for<0, NKS>([&](auto kb_t) __attribute__((always_inline)) {
                constexpr int kb = decltype(kb_t)::value;
                const bf16x8 ak = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(img_kp + ra[kb] + jo));
                s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ak, qf[kb], s, 0, 0, 0);
                if constexpr (SERIES == 1) {
                    const bf16x8 ao = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(img_do + ra[kb] + jo));
                    dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ao, vf[kb], dp, 0, 0, 0);
                }
            });
            unsigned bk[8];   // B operand of the second product: Pd (A) or dS (B) of this block as bf16 pairs
#pragma unroll
            for (int c4 = 0; c4 < 4; ++c4) {
                const int key0 = 32 * jb + 8 * c4 + 4 * hf;   // inside the chunk; C.k0 + key0 of all keys
                f32x4 mk = {1.f, 1.f, 1.f, 1.f};
                if (!FAST && mrow) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) mk[e] = (key0 + e < P.k) ? mrow[key0 + e] : 0.f;
                } else if (P.drop.thresh) {
                    const snf::philox_f4 m4 = snf::dropout_mask4(P.drop, a, P.n, lrow, C.k_total, C.k0 + key0);
                    mk = f32x4{m4[0], m4[1], m4[2], m4[3]};
                }
                f32x4 o;
                float pvv[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) pvv[e] = __builtin_amdgcn_exp2f(fmaf(s[4 * c4 + e], c_exp, -lse2));
                if constexpr (SERIES == 1 && !bwd_single_launch(DK)) {   // (64 and 128 keep the bits they always had)
                    // dS_j = (bf16(P_j M_j) dPd_j - P_j D) * scale.  D came out of series A as sum_j bf16(P_j M_j) dPd_j (bf16(P o M) is the
                    // MFMA operand of dV), so the first term carries the SAME rounded factor: sum_j dS_j = D - D sum_j P_j = 0 to fp32
                    // accuracy, and a row whose gradient cancels exactly (one key: P = 1, dS = 0) gives 0 instead of
                    // (M - bf16(M)) dPd -- 2^-9 of a term that the true gradient does not contain.
                    const unsigned r01 = pack2(pvv[0] * mk[0], pvv[1] * mk[1]), r23 = pack2(pvv[2] * mk[2], pvv[3] * mk[3]);
                    const float pd[4] = {lo_f(r01), hi_f(r01), lo_f(r23), hi_f(r23)};
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e] = (pd[e] * dp[4 * c4 + e] - pvv[e] * dtot) * P.scale;
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float pv = pvv[e];
                        if constexpr (SERIES == 0)
                            o[e] = pv * mk[e];                                       // Pd = P o M
                        else
                            o[e] = pv * (dp[4 * c4 + e] * mk[e] - dtot) * P.scale;   // dS = P o (dP - D) * scale, dP = dPd o M
                    }
                }
                const unsigned o01 = pack2(o[0], o[1]), o23 = pack2(o[2], o[3]);
                bk[2 * c4] = o01;
                bk[2 * c4 + 1] = o23;
                if constexpr (SERIES == 1) {
                    if (rvalid) {
                        if constexpr (FAST) {
                            if (!tail || key0 < P.k) *reinterpret_cast<uint2*>(dsrow16 + key0) = uint2{o01, o23};
                        } else if (P.ds_bf16) {
                            if (vec_ok) {
                                if (key0 < P.k) *reinterpret_cast<uint2*>(dsrow16 + key0) = uint2{o01, o23};
                            } else {
                                const unsigned short hv[4] = {(unsigned short)(o01 & 0xffffu), (unsigned short)(o01 >> 16),
                                                              (unsigned short)(o23 & 0xffffu), (unsigned short)(o23 >> 16)};
#pragma unroll
                                for (int e = 0; e < 4; ++e)
                                    if (key0 + e < P.k) dsrow16[key0 + e] = hv[e];
                            }
                        } else if (vec_ok) {
                            if (key0 < P.k) *reinterpret_cast<f32x4*>(dsrow + key0) = o;
                        } else {
#pragma unroll
                            for (int e = 0; e < 4; ++e)
                                if (key0 + e < P.k) dsrow[key0 + e] = o[e];
                        }
                    }
                }
            }
            // X^T[col, row] += T^T B^T: k-step = 16 keys (registers 4u .. 4u + 3 of the block)
            static_for<0, 2>([&](auto u_t) __attribute__((always_inline)) {
                constexpr int u = decltype(u_t)::value;
                const u32x4 bb = {bk[4 * u], bk[4 * u + 1], bk[4 * u + 2], bk[4 * u + 3]};
                const int koff = jo + 16 * u * RP;
                static_for<0, NCB>([&](auto db_t) __attribute__((always_inline)) {
                    constexpr int db = decltype(db_t)::value;
                    const bf16x8 at = tr_frag(img_t + rt0[db] + koff, img_t + rt1[db] + koff);
                    acc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(at, __builtin_bit_cast(bf16x8, bb), acc[db], 0, 0, 0);
                });
            });
            // keep the key blocks apart, as in the single-chunk kernel
            __builtin_amdgcn_sched_barrier(0);
        }

        if constexpr (SERIES == 0) {
            if (C.last) {   // D = V . dV per head: the lane's V row in the accumulators' column layout, one cross-half exchange
                float dpart = 0.f;
                const QT* vp = vg + (int64_t)lrow * P.ldv + a * DK + 4 * hf;
#pragma unroll
                for (int db = 0; db < NCB; ++db)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        float vv[4];
                        load4_bf16(vp + 32 * db + 8 * g, vv);
#pragma unroll
                        for (int e = 0; e < 4; ++e) dpart = fmaf(vv[e], acc[db][4 * g + e], dpart);
                    }
                const float dall = xhalf_sum(dpart);
                if (rvalid && hf == 0) C.dsum[(int64_t)a * P.n + row] = dall;
            }
        }
        if (rvalid) {
            if (C.last && P.dqv_bf16) {   // the sums leave once, in the caller's dtype and pitch
                unsigned short* op = reinterpret_cast<unsigned short*>(SERIES == 0 ? P.dv : P.dq) + (int64_t)row * P.ldd + a * DK + 4 * hf;
#pragma unroll
                for (int db = 0; db < NCB; ++db)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        uint2 pk;
                        pk.x = pack_bf16x2(acc[db][4 * g], acc[db][4 * g + 1]);
                        pk.y = pack_bf16x2(acc[db][4 * g + 2], acc[db][4 * g + 3]);
                        *reinterpret_cast<uint2*>(op + 32 * db + 8 * g) = pk;
                    }
            } else {
#pragma unroll
                for (int db = 0; db < NCB; ++db)
#pragma unroll
                    for (int g = 0; g < 4; ++g)
                        *reinterpret_cast<f32x4*>(accp + 32 * db + 8 * g) =
                            f32x4{acc[db][4 * g], acc[db][4 * g + 1], acc[db][4 * g + 2], acc[db][4 * g + 3]};
            }
        }
        if (++t == P.tiles_per_head) {
            t = 0;
            ++a;
        }
    }
}

// keys per chunk: as few chunks as the forward's make_chunks takes (224 keys at dk = 128, 256 at dk = 64, at most 8 chunks),
// near-equal, every chunk start a multiple of 32.  dk = 192: two images of 32 nkb rows x 384 bytes fit 160 KiB up to nkb = 6
// (144 KiB) = 192 keys per chunk -- fewer chunks than the forward's 128-key ones; the key range stays the forward's, k <= 8 * 128.
// dk = 256: two images of 32 nkb rows x 512 bytes are 128 KiB at nkb = 4 (a fifth block would take all 160 KiB) = 128 keys per chunk,
// the forward's figure: k <= 8 * 128 in at most 8 chunks.
constexpr int CH_MAX_CHUNKS = 8;
constexpr int bwd_chunk_kmax(int dk) { return dk == 64 ? 256 : dk == 128 ? 224 : dk == 192 ? 192 : dk == 256 ? 128 : 0; }
constexpr int bwd_chunk_klimit(int dk) { return dk == 192 ? 8 * 128 : CH_MAX_CHUNKS * bwd_chunk_kmax(dk); }
inline bool make_bwd_chunks(int k, int dk, int* n_chunks, int* chunk_k) {
    const int kmax = bwd_chunk_kmax(dk);
    if (!kmax || k < 1 || k > bwd_chunk_klimit(dk)) return false;
    const int nc = (k + kmax - 1) / kmax;
    if (nc > CH_MAX_CHUNKS) return false;
    const int ck = ((k + nc - 1) / nc + 31) / 32 * 32;
    *chunk_k = ck;
    *n_chunks = (k + ck - 1) / ck;
    return true;
}
inline size_t chunked_acc_bytes(int64_t n, int h, int dk) { return ((size_t)n * h * dk * sizeof(float) + 255) / 256 * 256; }

template <int DK, typename QT, int SERIES, bool FAST>
int launch_chunk(const ChunkParams& C, int num_wg, hipStream_t s) {
    constexpr size_t lds_max = (size_t)2 * (bwd_chunk_kmax(DK)) * 2 * DK;
    const size_t lds = (size_t)2 * 32 * C.nkb * 2 * DK;
    auto kern = sparse_attn_bwd_chunk_kernel<DK, QT, SERIES, FAST>;
    static thread_local unsigned long long attr_set_mask = 0;
    if (int rc = snf::lds_opt_in(reinterpret_cast<const void*>(kern), lds_max, &attr_set_mask, "sparse_attn_bwd_mfma_chunked")) return rc;
    hipLaunchKernelGGL(kern, dim3(num_wg), dim3(64 * ch_waves(DK)), lds, s, C);
    return snf::check_launch("sparse_attn_bwd_chunk_kernel");
}
template <int DK, typename QT>
int launch_chunk_series(const ChunkParams& C, int series, int num_wg, hipStream_t s) {
    if (series == 0) return launch_chunk<DK, QT, 0, false>(C, num_wg, s);
    if constexpr (std::is_same<QT, unsigned short>::value) {   // the training path: bf16 operands, bf16 dS, K % 4 == 0
        if (C.b.ds_bf16 && !C.b.mask && (C.k_total & 3) == 0) return launch_chunk<DK, QT, 1, true>(C, num_wg, s);
    }
    return launch_chunk<DK, QT, 1, false>(C, num_wg, s);
}

}  // namespace

extern "C" {

int snf_sparse_attn_bwd_mfma(const void* q, int64_t ldq, const void* v, int64_t ldv, int qv_dtype, const float* kp,
                             const float* dout, const float* lse, const float* mask, int64_t n, int k, int h, int dk,
                             float scale, float* dq, float* dv, void* ds, int ds_dtype, snf_stream_t stream) {
    return snf_sparse_attn_bwd_mfma_dropout(q, ldq, v, ldv, qv_dtype, kp, dout, lse, mask, 0.f, 0, 0, n, k, h, dk, scale, dq, dv, ds,
                                            ds_dtype, stream);
}

int snf_sparse_attn_bwd_mfma_dropout(const void* q, int64_t ldq, const void* v, int64_t ldv, int qv_dtype, const float* kp,
                                     const float* dout, const float* lse, const float* mask, float dropout_p, uint64_t seed,
                                     uint64_t offset, int64_t n, int k, int h, int dk, float scale, float* dq, float* dv,
                                     void* ds, int ds_dtype, snf_stream_t stream) {
    return snf_sparse_attn_bwd_mfma_ex(q, ldq, v, ldv, qv_dtype, kp, dout, lse, mask, dropout_p, seed, offset, n, k, h, dk, scale,
                                       dq, dv, (int64_t)h * dk, SNF_DT_F32, ds, ds_dtype, stream);
}

int snf_sparse_attn_bwd_mfma_ex(const void* q, int64_t ldq, const void* v, int64_t ldv, int qv_dtype, const float* kp,
                                const float* dout, const float* lse, const float* mask, float dropout_p, uint64_t seed,
                                uint64_t offset, int64_t n, int k, int h, int dk, float scale, void* dq, void* dv, int64_t ldd,
                                int dqv_dtype, void* ds, int ds_dtype, snf_stream_t stream) {
    SNF_REQUIRE(q && v && kp && dout && lse && dq && dv && ds, "snf_sparse_attn_bwd_mfma: null pointer");
    SNF_REQUIRE(dqv_dtype == SNF_DT_F32 || dqv_dtype == SNF_DT_BF16, "snf_sparse_attn_bwd_mfma: bad dq / dv dtype %d", dqv_dtype);
    SNF_REQUIRE(ldd >= (int64_t)h * dk && ldd % (dqv_dtype == SNF_DT_BF16 ? 8 : 4) == 0,
                "snf_sparse_attn_bwd_mfma: ldd=%lld must be >= h*dk and keep rows 16-byte aligned", (long long)ldd);
    SNF_REQUIRE(dropout_p >= 0.f && dropout_p < 1.f, "snf_sparse_attn_bwd_mfma: dropout_p=%f outside [0, 1)", dropout_p);
    SNF_REQUIRE(!(mask && dropout_p > 0.f), "snf_sparse_attn_bwd_mfma: pass a mask tensor OR (dropout_p, seed, offset), not both");
    SNF_REQUIRE(qv_dtype == SNF_DT_F32 || qv_dtype == SNF_DT_BF16, "snf_sparse_attn_bwd_mfma: bad dtype %d", qv_dtype);
    SNF_REQUIRE(ds_dtype == SNF_DT_F32 || ds_dtype == SNF_DT_BF16, "snf_sparse_attn_bwd_mfma: bad ds dtype %d", ds_dtype);
    BwdPlan pl;
    if (!make_bwd_plan(n, k, h, dk, &pl)) {
        snf::set_error("snf_sparse_attn_bwd_mfma: unsupported shape k=%d dk=%d (need dk == 128 with k <= 224 or dk == 64 "
                       "with k <= 256; dk == 192 and dk == 256 run on snf_sparse_attn_bwd_mfma_chunked)", k, dk);
        return SNF_EUNSUPPORTED;
    }
    const int64_t d = (int64_t)h * dk;
    const int align = qv_dtype == SNF_DT_BF16 ? 8 : 4;
    SNF_REQUIRE(ldq >= d && ldv >= d && (ldq % align) == 0 && (ldv % align) == 0,
                "snf_sparse_attn_bwd_mfma: ldq=%lld / ldv=%lld must be >= h*dk and keep rows 16-byte aligned", (long long)ldq,
                (long long)ldv);
    auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    SNF_REQUIRE(al16(q) && al16(v) && al16(kp) && al16(dout) && al16(dq) && al16(dv) && al16(ds),
                "snf_sparse_attn_bwd_mfma: buffers must be 16-byte aligned");
    BwdParams P;
    P.q = q;
    P.v = v;
    P.kp = kp;
    P.dout = dout;
    P.lse = lse;
    P.mask = mask;
    P.drop = snf::make_dropout(dropout_p, seed, offset);
    P.n = n;
    P.ldq = ldq;
    P.ldv = ldv;
    P.d = d;
    P.k = k;
    P.h = h;
    P.scale = scale;
    P.dq = dq;
    P.dv = dv;
    P.ldd = ldd;
    P.dqv_bf16 = dqv_dtype == SNF_DT_BF16;
    P.ds = ds;
    P.ds_bf16 = ds_dtype == SNF_DT_BF16;
    P.tiles_per_head = pl.tiles_per_head;
    P.tiles_per_wg = pl.tiles_per_wg;
    P.total_tiles = pl.total_tiles;
    hipStream_t s = snf::as_stream(stream);
    if (dk == 128)
        return qv_dtype == SNF_DT_F32 ? launch_bwd_nkb<128, float>(P, pl, s) : launch_bwd_nkb<128, unsigned short>(P, pl, s);
    return qv_dtype == SNF_DT_F32 ? launch_bwd_nkb<64, float>(P, pl, s) : launch_bwd_nkb<64, unsigned short>(P, pl, s);
}

size_t snf_sparse_attn_bwd_mfma_chunked_workspace_bytes(int64_t n, int k, int h, int dk, int dqv_dtype) {
    int nc, ck;
    // one chunk is the single-launch kernel's (no workspace) -- except at dk = 192 and 256, which only the chunked kernel is built for
    if (n < 1 || h < 1 || !make_bwd_chunks(k, dk, &nc, &ck) || (nc == 1 && bwd_single_launch(dk))) return 0;
    const size_t dsum = ((size_t)h * n * sizeof(float) + 255) / 256 * 256;
    return dsum + (dqv_dtype == SNF_DT_BF16 ? 2 * chunked_acc_bytes(n, h, dk) : 0);   // D | fp32 dV | fp32 dQ
}

int snf_sparse_attn_bwd_mfma_chunked(const void* q, int64_t ldq, const void* v, int64_t ldv, int qv_dtype, const float* kp,
                                     const float* dout, const float* lse, const float* mask, float dropout_p, uint64_t seed,
                                     uint64_t offset, int64_t n, int k, int h, int dk, float scale, void* dq, void* dv, int64_t ldd,
                                     int dqv_dtype, void* ds, int ds_dtype, void* workspace, size_t workspace_bytes,
                                     snf_stream_t stream) {
    int nc = 0, ck = 0;
    if (!make_bwd_chunks(k, dk, &nc, &ck)) {
        snf::set_error("snf_sparse_attn_bwd_mfma_chunked: unsupported shape k=%d dk=%d (need dk == 128 with k <= %d, dk == 64 with "
                       "k <= %d, dk == 192 with k <= %d or dk == 256 with k <= %d)", k, dk, bwd_chunk_klimit(128), bwd_chunk_klimit(64),
                       bwd_chunk_klimit(192), bwd_chunk_klimit(256));
        return SNF_EUNSUPPORTED;
    }
    if (nc == 1 && bwd_single_launch(dk))   // one chunk: the single-launch kernel, bit for bit (dk = 192 / 256 have none: one launch per series below)
        return snf_sparse_attn_bwd_mfma_ex(q, ldq, v, ldv, qv_dtype, kp, dout, lse, mask, dropout_p, seed, offset, n, k, h, dk, scale, dq,
                                           dv, ldd, dqv_dtype, ds, ds_dtype, stream);
    SNF_REQUIRE(q && v && kp && dout && lse && dq && dv && ds, "snf_sparse_attn_bwd_mfma_chunked: null pointer");
    SNF_REQUIRE(h >= 1 && n >= 1 && n <= 0x7fffff00ll, "snf_sparse_attn_bwd_mfma_chunked: bad shape n=%lld h=%d", (long long)n, h);
    SNF_REQUIRE(dqv_dtype == SNF_DT_F32 || dqv_dtype == SNF_DT_BF16, "snf_sparse_attn_bwd_mfma_chunked: bad dq / dv dtype %d", dqv_dtype);
    SNF_REQUIRE(ldd >= (int64_t)h * dk && ldd % (dqv_dtype == SNF_DT_BF16 ? 8 : 4) == 0,
                "snf_sparse_attn_bwd_mfma_chunked: ldd=%lld must be >= h*dk and keep rows 16-byte aligned", (long long)ldd);
    SNF_REQUIRE(dropout_p >= 0.f && dropout_p < 1.f, "snf_sparse_attn_bwd_mfma_chunked: dropout_p=%f outside [0, 1)", dropout_p);
    SNF_REQUIRE(!(mask && dropout_p > 0.f), "snf_sparse_attn_bwd_mfma_chunked: pass a mask tensor OR (dropout_p, seed, offset), not both");
    SNF_REQUIRE(qv_dtype == SNF_DT_F32 || qv_dtype == SNF_DT_BF16, "snf_sparse_attn_bwd_mfma_chunked: bad dtype %d", qv_dtype);
    SNF_REQUIRE(ds_dtype == SNF_DT_F32 || ds_dtype == SNF_DT_BF16, "snf_sparse_attn_bwd_mfma_chunked: bad ds dtype %d", ds_dtype);
    const int64_t d = (int64_t)h * dk;
    const int align = qv_dtype == SNF_DT_BF16 ? 8 : 4;
    SNF_REQUIRE(ldq >= d && ldv >= d && (ldq % align) == 0 && (ldv % align) == 0,
                "snf_sparse_attn_bwd_mfma_chunked: ldq=%lld / ldv=%lld must be >= h*dk and keep rows 16-byte aligned", (long long)ldq,
                (long long)ldv);
    auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    SNF_REQUIRE(al16(q) && al16(v) && al16(kp) && al16(dout) && al16(dq) && al16(dv) && al16(ds) && al16(workspace),
                "snf_sparse_attn_bwd_mfma_chunked: buffers must be 16-byte aligned");
    const size_t need = snf_sparse_attn_bwd_mfma_chunked_workspace_bytes(n, k, h, dk, dqv_dtype);
    if (!workspace || workspace_bytes < need) {
        snf::set_error("snf_sparse_attn_bwd_mfma_chunked: workspace %zu < %zu", workspace_bytes, need);
        return SNF_EWORKSPACE;
    }
    const int ch_rows = 32 * ch_waves(dk);   // query rows per workgroup step
    const int64_t tph = (n + ch_rows - 1) / ch_rows, total = tph * h;
    if (total > 0x7fffffff) {
        snf::set_error("snf_sparse_attn_bwd_mfma_chunked: too many row tiles (n=%lld h=%d)", (long long)n, h);
        return SNF_EUNSUPPORTED;
    }
    const int cus = snf::cu_count();
    int64_t num_wg = total < cus ? total : cus;
    const int64_t tpw = (total + num_wg - 1) / num_wg;
    num_wg = (total + tpw - 1) / tpw;

    unsigned char* wsb = reinterpret_cast<unsigned char*>(workspace);
    const size_t dsum_bytes = ((size_t)h * n * sizeof(float) + 255) / 256 * 256;
    ChunkParams C;
    BwdParams& P = C.b;
    P.q = q, P.v = v, P.lse = lse, P.mask = mask;
    P.drop = snf::make_dropout(dropout_p, seed, offset);
    P.n = n, P.ldq = ldq, P.ldv = ldv, P.d = d, P.h = h, P.scale = scale;
    P.dq = dq, P.dv = dv, P.ldd = ldd, P.dqv_bf16 = dqv_dtype == SNF_DT_BF16;
    P.ds = ds, P.ds_bf16 = ds_dtype == SNF_DT_BF16;
    P.tiles_per_head = (int)tph, P.tiles_per_wg = (int)tpw, P.total_tiles = (int)total;
    C.k_total = k;
    C.dsum = reinterpret_cast<float*>(wsb);
    hipStream_t s = snf::as_stream(stream);
    for (int series = 0; series < 2; ++series) {
        // fp32 outputs are their own running sums; bf16 outputs are written once, by the last launch, from the workspace's
        if (P.dqv_bf16) {
            C.acc = reinterpret_cast<float*>(wsb + dsum_bytes + (series ? chunked_acc_bytes(n, h, dk) : 0));
            C.ldacc = d;
        } else {
            C.acc = reinterpret_cast<float*>(series ? dq : dv);
            C.ldacc = ldd;
        }
        for (int c = 0; c < nc; ++c) {
            C.k0 = c * ck;
            P.k = k - C.k0 < ck ? k - C.k0 : ck;
            P.kp = kp + (int64_t)C.k0 * d;
            P.dout = dout + (int64_t)C.k0 * d;
            C.nkb = (P.k + 31) / 32;
            C.first = c == 0, C.last = c == nc - 1;
            int rc;
            if (dk == 128)
                rc = qv_dtype == SNF_DT_F32 ? launch_chunk_series<128, float>(C, series, (int)num_wg, s)
                                            : launch_chunk_series<128, unsigned short>(C, series, (int)num_wg, s);
            else if (dk == 192)
                rc = qv_dtype == SNF_DT_F32 ? launch_chunk_series<192, float>(C, series, (int)num_wg, s)
                                            : launch_chunk_series<192, unsigned short>(C, series, (int)num_wg, s);
            else if (dk == 256)
                rc = qv_dtype == SNF_DT_F32 ? launch_chunk_series<256, float>(C, series, (int)num_wg, s)
                                            : launch_chunk_series<256, unsigned short>(C, series, (int)num_wg, s);
            else
                rc = qv_dtype == SNF_DT_F32 ? launch_chunk_series<64, float>(C, series, (int)num_wg, s)
                                            : launch_chunk_series<64, unsigned short>(C, series, (int)num_wg, s);
            if (rc) return rc;
        }
    }
    return SNF_OK;
}

}  // extern "C"
