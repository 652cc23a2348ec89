// The one copy of the device code of the differentiable ViT self-attention (gfx950): the LDS layouts per head width, the tile
// primitives, the two tile bodies of the backward, the whole backward for T <= 256, the T == 1 copy and the host-side argument
// checks.  Shells over it: csrc/vit_attn_bwd.hip (dk = 64, T <= 256), csrc/vit_attn_bwd_long.hip (dk = 64, 256 < T <= 4096) and
// csrc/vit_attn_dk32.hip (dk = 32, forward and backward).  A further head width is a layout below and a launch shell.
//
// What every user of these tiles relies on, stated here once:
//   * Every output element has one owner and one summation order: nothing is reduced across waves, there are no atomics.
//   * Staged rows >= T are zero, and their lse * log2(e) and D are 0: finite values, so that the (zero) Q and dO rows of queries
//     past T give dS = 0 exactly and add nothing to dK and dV.
//   * S is rebuilt, not approximated: the key-side tile forms S from the same three fp32-class terms in the same order as the
//     query-side tile (by operand identity: K_hi Q_lo, then K_lo Q_hi, then K_hi Q_hi; the same for V and dO), so the P of
//     both are the same bits although the operands swap sides of the MFMA.
//   * ds_read_b64_tr_b16 needs EXEC all ones: lanes past T clamp their global addresses and skip stores only; a wave whose tile
//     is past T skips its work by a wave-uniform branch and still reaches every barrier.
#pragma once
#include <initializer_list>

#include "mfma.h"

namespace {

typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;

constexpr int VT_THREADS = 512;   // 8 waves: one staged image of 256 rows is 8 tiles of 32
constexpr float VT_LOG2E = 1.44269504088896340736f;

// ---------------------------------------------------------------------------------------------------------------- layouts
// A staged image is [rows][DK] bf16, row-major, moved in 16-byte parts.  off(r, c) is the byte offset of part c of row r; both
// fragment forms below address through it with r relative to a row that is a multiple of 16.
//
// dk = 64: 144-byte rows (64 + 8 bf16), conflict-free 16-byte fragment reads both ways.
struct VitLayout64 {
    static constexpr int DK = 64, KS = DK / 16, NB = DK / 32, PARTS = DK / 8, ROWB = 144;
    static __device__ __forceinline__ int off(int r, int c) { return r * ROWB + 16 * c; }
};
// dk = 32: LDS rows are 64 bytes with NO padding; the 16-byte part c of row r sits at part position c ^ ((r >> 2) & 3).
//   Why not a padded pitch: one image is read both ways (K in phase A: row fragments for S, transposed for dQ; Q and dO in phase B
//   likewise).  A transpose-read lane group (32 lanes, ds_read_b64_tr_b16) covers 4 consecutive rows x 64 bytes = 256 bytes, which
//   is exactly the 64 banks once if and only if the 4 rows are contiguous: any pitch above 64 bytes makes them overlap (80 bytes:
//   rows 0 and 3 share 12 banks, a 2-way conflict on every transposed read).  Unpadded rows alone would make the row fragments
//   4-way conflicted (ds_read_b128 serves 16 lanes per cycle, rows r and r + 4 land on the same banks), so the parts are XOR-rotated:
//     - row fragment, ds_read_b128, lane = row r0 + j, logical part 2 ks + hf.  The four lane groups hold, per half-wave, the rows
//       {0-3, 12-15, 20-27} or {4-11, 16-19, 28-31}.  The 4-bank span of a lane is 4 (r & 3) + (part ^ ((r >> 2) & 3)); in either
//       set the four rows of equal r & 3 have (r >> 2) & 3 = {0, 3, 1, 2} or {1, 2, 0, 3}: 16 distinct spans, conflict-free.
//     - transposed fragment, lanes 0-31 read rows r0 + {0..3} (r0 % 4 == 0: one rotation for all four rows, a permutation of the
//       parts inside each row), lanes 32-63 rows r0 + 4 + {0..3}: every group reads 4 whole rows = 64 distinct banks.
//     - staging stores (ds_write_b128, 8 consecutive lanes per cycle = 2 rows x 4 parts): 128 contiguous bytes, permuted.
//   The V image of the forward uses the same layout (the 128-byte-row rotation of vit.hip has no meaning at 64-byte rows): it is
//   only read transposed, and the argument above holds for it unchanged.
struct VitLayout32 {
    static constexpr int DK = 32, KS = DK / 16, NB = DK / 32, PARTS = DK / 8, ROWB = 64;
    static __device__ __forceinline__ int off(int r, int c) { return r * ROWB + 16 * (c ^ ((r >> 2) & 3)); }
};

template <bool X3>
using vit_elt_t = typename std::conditional<X3, float, unsigned short>::type;

// 32 rows of a [T, DK] matrix as an MFMA operand (lane & 31 = row): one fragment per k-step, hi and (fp32 class) lo
template <typename L, bool X3>
struct VitRows {
    bf16x8 hi[L::KS], lo[X3 ? L::KS : 1];
};

// -------------------------------------------------------------------------------------------------------------- primitives
__device__ __forceinline__ u32x4 load8(const unsigned short* p) { return *reinterpret_cast<const u32x4*>(p); }

// Rows row0 .. row0 + ROWS - 1 of two [T, DK] matrices of the image whose first row is `base` (row strides ld0, ld1 elements) into
// two LDS images of one or two bf16 planes each (plane stride ROWS * ROWB); rows >= T are zero.  Workgroup-wide: every thread runs
// it.  Every global load of the thread is issued before its first LDS store.
template <typename L, int ROWS, bool X3>
__device__ __forceinline__ void stage(unsigned char* img0, unsigned char* img1, const vit_elt_t<X3>* __restrict__ p0, int64_t ld0,
                                      const vit_elt_t<X3>* __restrict__ p1, int64_t ld1, int64_t base, int row0, int T) {
    constexpr int IMG = ROWS * L::ROWB;
    constexpr int NI = (ROWS * L::PARTS + VT_THREADS - 1) / VT_THREADS;
    constexpr bool WHOLE = ROWS * L::PARTS % VT_THREADS == 0;   // otherwise the last round has threads past the image
    typename std::conditional<X3, f32x8, u32x4>::type s0[NI], s1[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int c = threadIdx.x + VT_THREADS * i;
        const int r = c / L::PARTS, part = c % L::PARTS;
        s0[i] = {};
        s1[i] = {};
        if (row0 + r < T && (WHOLE || r < ROWS)) {
            s0[i] = load8(p0 + (base + row0 + r) * ld0 + part * 8);
            s1[i] = load8(p1 + (base + row0 + r) * ld1 + part * 8);
        }
    }
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int c = threadIdx.x + VT_THREADS * i;
        const int r = c / L::PARTS, part = c % L::PARTS;
        if (WHOLE || r < ROWS) {
            const int off = L::off(r, part);
            if constexpr (X3) {
                u32x4 h0, l0, h1, l1;
                split8(s0[i], h0, l0);
                split8(s1[i], h1, l1);
                *reinterpret_cast<u32x4*>(img0 + off) = h0;
                *reinterpret_cast<u32x4*>(img0 + IMG + off) = l0;
                *reinterpret_cast<u32x4*>(img1 + off) = h1;
                *reinterpret_cast<u32x4*>(img1 + IMG + off) = l1;
            } else {
                *reinterpret_cast<u32x4*>(img0 + off) = s0[i];
                *reinterpret_cast<u32x4*>(img1 + off) = s1[i];
            }
        }
    }
}

// What a lane keeps for the whole kernel: its place in the wave and the addressing of the two fragment forms (byte offsets relative
// to an image row r0, r0 % 16 == 0).
template <typename L>
struct VitLane {
    int lane, j, hf;    // lane = 32 hf + j
    int rf[L::KS];      // row fragment of k-step ks: row j, part 2 ks + hf
    int tr[L::NB][2];   // transposed fragment of column block db: rows 4 hf + (ti >> 2) and the same + 8, 8-byte half ti & 1 of
                        // part 4 db + 2 (tg & 1) + ((ti & 3) >> 1), for lane ti of 16-lane group tg
    __device__ __forceinline__ VitLane() {
        lane = threadIdx.x & 63;
        j = lane & 31, hf = lane >> 5;
        static_for<0, L::KS>([&](auto ks) __attribute__((always_inline)) { rf[ks] = L::off(j, 2 * ks + hf); });
        const int tg = lane >> 4, ti = lane & 15;
        const int row = 4 * (tg >> 1) + (ti >> 2);
        static_for<0, L::NB>([&](auto db) __attribute__((always_inline)) {
            const int part = 4 * db + 2 * (tg & 1) + ((ti & 3) >> 1), half = 8 * (ti & 1);
            tr[db][0] = L::off(row, part) + half;
            tr[db][1] = L::off(row + 8, part) + half;
        });
    }
    // A or B operand with the image's row r0 + j on the lane: columns 16 ks + 8 hf .. + 7
    __device__ __forceinline__ bf16x8 row_frag(const unsigned char* img, int r0, int ks) const {
        return __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(img + r0 * L::ROWB + rf[ks]));
    }
    // A operand with the image's COLUMN 32 db + j on the lane: rows r0 + 4 hf + {0..3} and the same + 8 in the registers -- the order
    // in which a C tile holds its rows, so P^T / dS^T feed the next product without lane movement
    __device__ __forceinline__ bf16x8 col_frag(const unsigned char* img, int r0, int db) const {
        const unsigned char* p = img + r0 * L::ROWB;
        return tr_frag(p + tr[db][0], p + tr[db][1]);
    }
};

// 32 rows of a [T, DK] matrix in HBM as an operand (p: this lane's row), split when X3
template <typename L, bool X3>
__device__ __forceinline__ void load_rows(const VitLane<L>& ln, const vit_elt_t<X3>* __restrict__ p, VitRows<L, X3>& x) {
    const int hf = ln.hf;
    static_for<0, L::KS>([&](auto ks) __attribute__((always_inline)) {
        if constexpr (X3)
            split8(load8(p + 16 * ks + 8 * hf), x.hi[ks], x.lo[ks]);
        else
            x.hi[ks] = load_frag(p + 16 * ks + 8 * hf);
    });
}

// acc[db] += (columns 32 db .. of image rows r0 + 16 u ..)^T x (registers 8 u .. 8 u + 7 of x), db < DK / 32, u = 0, 1
template <typename L, int IMG, bool X3>
__device__ __forceinline__ void tr_product(const VitLane<L>& ln, const unsigned char* img, int r0, const f32x16& x, f32x16 (&acc)[L::NB]) {
    static_for<0, 2>([&](auto u_t) __attribute__((always_inline)) {
        constexpr int u = decltype(u_t)::value;
        f32x8 xv;
#pragma unroll
        for (int e = 0; e < 8; ++e) xv[e] = x[8 * u + e];
        if constexpr (X3) {
            bf16x8 xh, xl;
            split8(xv, xh, xl);
            static_for<0, L::NB>([&](auto db_t) __attribute__((always_inline)) {
                constexpr int db = decltype(db_t)::value;
                const bf16x8 ah = ln.col_frag(img, r0 + 16 * u, db), al = ln.col_frag(img + IMG, r0 + 16 * u, db);
                acc[db] = mfma(ah, xl, acc[db]);
                acc[db] = mfma(al, xh, acc[db]);
                acc[db] = mfma(ah, xh, acc[db]);
            });
        } else {
            static_for<0, L::NB>([&](auto db_t) __attribute__((always_inline)) {
                constexpr int db = decltype(db_t)::value;
                acc[db] = mfma(ln.col_frag(img, r0 + 16 * u, db), __builtin_convertvector(xv, bf16x8), acc[db]);
            });
        }
    });
}

// store a transposed DK x 32 result (p: this lane's row of the output matrix, 4 consecutive columns per register group) times f
template <typename L, bool X3>
__device__ __forceinline__ void store_rows(const VitLane<L>& ln, vit_elt_t<X3>* __restrict__ p, const f32x16 (&acc)[L::NB], float f) {
    const int hf = ln.hf;
    static_for<0, L::NB>([&](auto db) __attribute__((always_inline)) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 o4 = {acc[db][4 * g] * f, acc[db][4 * g + 1] * f, acc[db][4 * g + 2] * f, acc[db][4 * g + 3] * f};
            const int d0 = 32 * db + 8 * g + 4 * hf;
            if constexpr (X3)
                *reinterpret_cast<f32x4*>(p + d0) = o4;
            else
                *reinterpret_cast<u32x2*>(p + d0) = __builtin_bit_cast(u32x2, __builtin_convertvector(o4, bf16x4));
        }
    });
}

// ------------------------------------------------------------------------------------------------------------ tile bodies
// Each side is bound once per wave to what stays put over its walk (images, the wave's operands in registers, scalars) and then
// called per staged tile.  The members are references, like the captures of a lambda written in the kernel: passed by value as
// function arguments the same code schedules differently and leaves the kernels' register budgets.
//
// Query side.  P^T and dP^T of the 32 staged keys at image rows r0 .. (K in img0, V in img1, staged from row row0 on) against the
// wave's queries q and their dO rows g: lane = query, register r = key row0 + r0 + (r & 3) + 8 (r >> 2) + 4 hf.
//   S^T = K Q^T, P = exp2(c_exp S - lse2) (lse2 = lse * log2 e of the lane's query), 0 for keys >= T;  dP^T = V dO^T
template <typename L, int IMG, bool X3>
struct VitQuerySide {
    const VitLane<L>& ln;
    const unsigned char *img0, *img1;
    const int& T;
    const VitRows<L, X3>&q, &g;
    const float &c_exp, &lse2;
    __device__ __forceinline__ void operator()(int r0, int row0, f32x16& p, f32x16& dp) const {
#pragma unroll
        for (int r = 0; r < 16; ++r) p[r] = 0.f, dp[r] = 0.f;
        static_for<0, L::KS>([&](auto ks) __attribute__((always_inline)) {
            const bf16x8 kh = ln.row_frag(img0, r0, ks), vh = ln.row_frag(img1, r0, ks);
            if constexpr (X3) {
                const bf16x8 kl = ln.row_frag(img0 + IMG, r0, ks), vl = ln.row_frag(img1 + IMG, r0, ks);
                p = mfma(kh, q.lo[ks], p);
                p = mfma(kl, q.hi[ks], p);
                dp = mfma(vh, g.lo[ks], dp);
                dp = mfma(vl, g.hi[ks], dp);
            }
            p = mfma(kh, q.hi[ks], p);
            dp = mfma(vh, g.hi[ks], dp);
        });
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key = row0 + r0 + (r & 3) + 8 * (r >> 2) + 4 * ln.hf;
            const float e = __builtin_amdgcn_exp2f(fmaf(p[r], c_exp, -lse2));
            p[r] = key < T ? e : 0.f;
        }
    }
};

// Key side.  Adds the 32 staged queries at image rows r0 .. (Q in img0, dO in img1; their lse * log2 e and D at lse2_l, d_l) into
// dK and dV of the wave's key tile (k, v in registers): lane = key, register r = query r0 + (r & 3) + 8 (r >> 2) + 4 hf.
//   S = Q K^T, P;  dV^T += dO^T P;  dP = dO V^T, dS = P o (dP - D);  dK^T += Q^T dS
// P is consumed by dV before dP is formed, which keeps the live tiles at two.
template <typename L, int IMG, bool X3>
struct VitKeySide {
    const VitLane<L>& ln;
    const unsigned char *img0, *img1;
    const float *lse2_l, *d_l;
    const VitRows<L, X3>&k, &v;
    const float& c_exp;
    __device__ __forceinline__ void operator()(int r0, f32x16 (&dk)[L::NB], f32x16 (&dv)[L::NB]) const {
        const int hf = ln.hf;
        f32x16 p, dp;
#pragma unroll
        for (int r = 0; r < 16; ++r) p[r] = 0.f, dp[r] = 0.f;
        static_for<0, L::KS>([&](auto ks) __attribute__((always_inline)) {
            const bf16x8 qh = ln.row_frag(img0, r0, ks);
            if constexpr (X3) {   // the terms of the query side in its order (K_hi Q_lo, K_lo Q_hi, K_hi Q_hi): S is rebuilt, not approximated
                const bf16x8 ql = ln.row_frag(img0 + IMG, r0, ks);
                p = mfma(ql, k.hi[ks], p);
                p = mfma(qh, k.lo[ks], p);
            }
            p = mfma(qh, k.hi[ks], p);
        });
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 l4 = *reinterpret_cast<const f32x4*>(lse2_l + r0 + 8 * g + 4 * hf);
#pragma unroll
            for (int e = 0; e < 4; ++e) p[4 * g + e] = __builtin_amdgcn_exp2f(fmaf(p[4 * g + e], c_exp, -l4[e]));
        }
        tr_product<L, IMG, X3>(ln, img1, r0, p, dv);    // dV^T += dO^T P
        static_for<0, L::KS>([&](auto ks) __attribute__((always_inline)) {
            const bf16x8 gh = ln.row_frag(img1, r0, ks);
            if constexpr (X3) {
                const bf16x8 gl = ln.row_frag(img1 + IMG, r0, ks);
                dp = mfma(gl, v.hi[ks], dp);
                dp = mfma(gh, v.lo[ks], dp);
            }
            dp = mfma(gh, v.hi[ks], dp);
        });
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 d4 = *reinterpret_cast<const f32x4*>(d_l + r0 + 8 * g + 4 * hf);
#pragma unroll
            for (int e = 0; e < 4; ++e) dp[4 * g + e] = p[4 * g + e] * (dp[4 * g + e] - d4[e]);
        }
        tr_product<L, IMG, X3>(ln, img0, r0, dp, dk);   // dK^T += Q^T dS
    }
};

// ------------------------------------------------------------------------------------------------- backward, T <= 32 NKB <= 256
// One workgroup per (image, head) = (blockIdx.y, blockIdx.x), 8 waves, two phases over the same LDS:
//   phase A  K and V staged.  Wave w owns query tile w (32 queries, one per lane pair): D_i = sum_j P_ij dP_ij (first pass over the
//            key blocks), then dQ^T += K^T dS^T (second pass).  lse * log2(e) and D go to two small fp32 arrays in LDS.
//   phase B  wave w keeps the K and V fragments of key tile w in registers; Q and dO are staged over the images of K and V; every
//            query tile is added into dK and dV.
// S is computed three times (twice in phase A): the price of keeping no T x T state and needing no cross-wave reduction.
template <typename L, int NKB>
constexpr size_t vit_bwd_lds_bytes(bool x3) {
    return (size_t)2 * (x3 ? 2 : 1) * (32 * NKB * L::ROWB) + (size_t)2 * 32 * NKB * sizeof(float);
}

template <typename L, int NKB, bool X3>
__device__ __forceinline__ void vit_bwd_short(const void* qkv_, const void* dout_, const float* lse, int T, int h, float scale, void* dqkv_) {
    constexpr int DK = L::DK;
    constexpr int NP = X3 ? 2 : 1;         // operand planes (hi, lo)
    constexpr int ROWS = 32 * NKB;
    constexpr int IMG = ROWS * L::ROWB;    // bytes of one plane of one staged matrix
    typedef vit_elt_t<X3> elt_t;
    const elt_t* __restrict__ qkv = reinterpret_cast<const elt_t*>(qkv_);
    const elt_t* __restrict__ dout = reinterpret_cast<const elt_t*>(dout_);
    elt_t* __restrict__ dqkv = reinterpret_cast<elt_t*>(dqkv_);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // images [matrix 0 / 1][plane][ROWS][ROWB bytes] (phase A: K, V; phase B: Q, dO), then lse * log2(e) and D per query
    unsigned char* const img0 = smem;
    unsigned char* const img1 = smem + NP * IMG;
    float* const lse2_l = reinterpret_cast<float*>(smem + 2 * NP * IMG);
    float* const d_l = lse2_l + ROWS;

    const int a = blockIdx.x, b = blockIdx.y;
    const int D = h * DK;
    const int64_t base = (int64_t)b * T;
    const VitLane<L> ln;
    const int j = ln.j, hf = ln.hf;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ntile = (T + 31) / 32;
    const bool active = w < ntile;   // wave-uniform: this wave owns query tile w (phase A) and key tile w (phase B)
    const float c_exp = scale * VT_LOG2E;

    // ------------------------------------------------------------ phase A: D and dQ of query tile w
    stage<L, ROWS, X3>(img0, img1, qkv + D + a * DK, 3 * (int64_t)D, qkv + 2 * D + a * DK, 3 * (int64_t)D, base, 0, T);
    __syncthreads();
    if (active) {
        const int q_row = 32 * w + j;
        const int q_ld = q_row < T ? q_row : T - 1;   // lanes past T recompute the last row and store nothing
        VitRows<L, X3> q, g;
        load_rows<L, X3>(ln, qkv + (base + q_ld) * 3 * D + a * DK, q);
        load_rows<L, X3>(ln, dout + (base + q_ld) * D + a * DK, g);
        const float lse2 = lse[((int64_t)b * h + a) * T + q_ld] * VT_LOG2E;
        const VitQuerySide<L, IMG, X3> p_dp{ln, img0, img1, T, q, g, c_exp, lse2};
        float d_lane = 0.f;
#pragma unroll 1
        for (int jb = 0; jb < ntile; ++jb) {
            f32x16 p, dp;
            p_dp(32 * jb, 0, p, dp);
#pragma unroll
            for (int r = 0; r < 16; ++r) d_lane = fmaf(p[r], dp[r], d_lane);
        }
        const float d_row = xhalf_sum(d_lane);   // the two half-waves hold the two halves of the row's keys
        f32x16 dq[L::NB] = {};
#pragma unroll 1
        for (int jb = 0; jb < ntile; ++jb) {
            f32x16 p, dp;
            p_dp(32 * jb, 0, p, dp);
#pragma unroll
            for (int r = 0; r < 16; ++r) p[r] *= dp[r] - d_row;
            tr_product<L, IMG, X3>(ln, img0, 32 * jb, p, dq);   // dQ^T += K^T dS^T
        }
        if (q_row < T) store_rows<L, X3>(ln, dqkv + (base + q_row) * 3 * D + a * DK, dq, scale);
        if (hf == 0) {   // rows past T: lse = D = 0
            lse2_l[q_row] = q_row < T ? lse2 : 0.f;
            d_l[q_row] = q_row < T ? d_row : 0.f;
        }
    }

    // ------------------------------------------------------------ phase B: dK and dV of key tile w
    VitRows<L, X3> k, v;
    if (active) {
        static_for<0, L::KS>([&](auto ks) __attribute__((always_inline)) {
            k.hi[ks] = ln.row_frag(img0, 32 * w, ks);
            v.hi[ks] = ln.row_frag(img1, 32 * w, ks);
            if constexpr (X3) {
                k.lo[ks] = ln.row_frag(img0 + IMG, 32 * w, ks);
                v.lo[ks] = ln.row_frag(img1 + IMG, 32 * w, ks);
            }
        });
    }
    __syncthreads();   // every wave is done with the images of K and V
    stage<L, ROWS, X3>(img0, img1, qkv + a * DK, 3 * (int64_t)D, dout + a * DK, (int64_t)D, base, 0, T);
    __syncthreads();
    if (active) {
        const VitKeySide<L, IMG, X3> add_tile{ln, img0, img1, lse2_l, d_l, k, v, c_exp};
        f32x16 dk[L::NB] = {}, dv[L::NB] = {};
#pragma unroll 1
        for (int qt = 0; qt < ntile; ++qt) add_tile(32 * qt, dk, dv);
        const int key = 32 * w + j;
        if (key < T) {
            store_rows<L, X3>(ln, dqkv + (base + key) * 3 * D + D + a * DK, dk, scale);
            store_rows<L, X3>(ln, dqkv + (base + key) * 3 * D + 2 * D + a * DK, dv, 1.0f);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------ T == 1
// Softmax over one key is the constant 1: dQ = dK = 0, dV = dO, so dqkv row = (0 | 0 | dout row), exact in both arithmetics.  The
// one text of the copy kernel; every file that serves T == 1 gives it the kernel name its entry point is known by.
#define VIT_BWD_T1_KERNEL(name)                                                                                                              \
    template <typename elt_t>                                                                                                                \
    __global__ __launch_bounds__(256) void name(const elt_t* __restrict__ dout, int64_t total, int D, elt_t* __restrict__ dqkv) {            \
        for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {                  \
            const int64_t row = i / (3 * D);                                                                                                 \
            const int col = (int)(i - row * 3 * D);                                                                                          \
            dqkv[i] = col >= 2 * D ? dout[row * D + col - 2 * D] : elt_t(0);                                                                 \
        }                                                                                                                                    \
    }

// launches a file's VIT_BWD_T1_KERNEL in the form of the tensors
inline int vit_launch_bwd_t1(void (*kf)(const float*, int64_t, int, float*), void (*kh)(const unsigned short*, int64_t, int, unsigned short*),
                             const char* what, bool x3, const void* dout, int b, int h, int dk, void* dqkv, hipStream_t s) {
    const int64_t total = (int64_t)b * 3 * h * dk;
    const int grid = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    if (x3)
        hipLaunchKernelGGL(kf, dim3(grid), dim3(256), 0, s, reinterpret_cast<const float*>(dout), total, h * dk, reinterpret_cast<float*>(dqkv));
    else
        hipLaunchKernelGGL(kh, dim3(grid), dim3(256), 0, s, reinterpret_cast<const unsigned short*>(dout), total, h * dk,
                           reinterpret_cast<unsigned short*>(dqkv));
    return snf::check_launch(what);
}

// -------------------------------------------------------------------------------------------------------------- host checks
// The argument checks of an entry point `who`: SNF_EINVAL for a null pointer, a dtype that is neither form or b / t / h < 1;
// SNF_EUNSUPPORTED for a shape outside dk == need_dk, t_above < t <= t_max, b <= 65535 (blockIdx.y) and for operands that the
// vector accesses cannot take: `vec` (named `vec_names` in the message) 16-byte aligned, `f32` (lse, workspace) 4-byte.
inline int vit_check_args(const char* who, std::initializer_list<const void*> vec, const char* vec_names, std::initializer_list<const void*> f32,
                          int dtype, int b, int t, int h, int dk, int need_dk, int t_above, int t_max) {
    uintptr_t vec_bits = 0, f32_bits = 0;
    bool null = false;
    for (const void* p : vec) null |= !p, vec_bits |= reinterpret_cast<uintptr_t>(p);
    for (const void* p : f32) null |= !p, f32_bits |= reinterpret_cast<uintptr_t>(p);
    SNF_REQUIRE(!null, "%s: null pointer", who);
    SNF_REQUIRE(dtype == SNF_DT_F32 || dtype == SNF_DT_BF16, "%s: dtype is f32 (fp32 class) or bf16 (got %d)", who, dtype);
    SNF_REQUIRE(b >= 1 && t >= 1 && h >= 1, "%s: bad shape", who);
    if (dk != need_dk || t <= t_above || t > t_max || b > 65535) {
        if (t_above)
            snf::set_error("%s: unsupported shape dk=%d t=%d b=%d (need dk == %d, %d < t <= %d, b <= 65535; t <= %d is served by "
                           "snf_vit_attention_bwd)", who, dk, t, b, need_dk, t_above, t_max, t_above);
        else
            snf::set_error("%s: unsupported shape dk=%d t=%d b=%d (need dk == %d, t <= %d, b <= 65535)", who, dk, t, b, need_dk, t_max);
        return SNF_EUNSUPPORTED;
    }
    if ((vec_bits & 15) != 0 || (f32_bits & 3) != 0) {
        snf::set_error("%s: unsupported operands: %s must be 16-byte aligned (16-byte vector loads and stores)", who, vec_names);
        return SNF_EUNSUPPORTED;
    }
    return SNF_OK;
}

}  // namespace
