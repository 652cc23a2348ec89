// Differentiable ViT self-attention at head width 32 on the matrix cores (gfx950), 1 <= T <= 256: the MAE decoder of adapter
// pre-training (512 wide, 16 heads, T = 197).  The 64-wide pair is csrc/vit.hip (forward) and csrc/vit_attn_bwd.hip (backward); this
// file is both at dk = 32, with the same operands, arithmetics and ownership of outputs.
//
//   snf_vit_attention_dk32_fwd_lse  qkv [B*T, 3*h*32] (q | k | v) -> out [B*T, h*32], lse [B, h, T] f32 (natural log)
//   snf_vit_attention_dk32_bwd      qkv, dout [B*T, h*32], lse -> dqkv [B*T, 3*h*32] (dQ | dK | dV), fully written
//
//   SNF_DT_F32  : fp32 tensors, fp32-class arithmetic: every operand is hi + lo (hi = bf16(x), lo = bf16(x - hi)), every product
//                 hi hi + hi lo + lo hi on v_mfma_f32_32x32x16_bf16, fp32 accumulation; P and dS are split in registers.
//   SNF_DT_BF16 : bf16 tensors, P and dS rounded to bf16 as operands, fp32 accumulation, bf16 outputs.
//
// Forward (vit_attn32_fwd_kernel<NKB, X3>): one workgroup per (image, head), 8 waves, wave w owns query tile w (T <= 256 is at most 8
// tiles of 32, so one round).  K and V are staged row-major; S^T = K Q^T takes two k-steps (dk = 32 = 2 x 16), the softmax is online
// across the key blocks, O^T = V^T P^T is ONE 32 x 32 accumulator with V^T read back by ds_read_b64_tr_b16.
//
// Backward (vit_attn32_bwd_kernel<NKB, X3>): the two phases of vit_attention_bwd_kernel over the same LDS.
//   phase A  K and V staged; wave w owns query tile w: D_i = sum_j P_ij dP_ij (first pass over the key blocks), then
//            dQ^T += K^T dS^T (second pass).  lse * log2(e) and D go to two small fp32 arrays in LDS.
//   phase B  wave w keeps the K and V fragments of key tile w in registers; Q and dO are staged over the images of K and V; for every
//            query tile dV^T += dO^T P and dK^T += Q^T dS.
// No atomics, no cross-wave reduction: every output element has one owner and one summation order.  T == 1 is a copy kernel
// (vit_attn32_bwd_t1_kernel: dQ = dK = 0, dV = dO), exact in both arithmetics.
//
// Key-block counts built: 2, 4 and 8 (T <= 64, <= 128, <= 256).  NKB sizes the LDS images and the staging loops only; the loops
// over key blocks and query tiles run to ceil(T / 32), so T = 197 under NKB = 8 does 7 blocks of work.  A separate 6 would save
// 64 zero rows of staging and nothing else.
//
// Layout decisions at this width
//   * LDS rows are 64 bytes with NO padding; the 16-byte part c of row r sits at part position c ^ ((r >> 2) & 3).
//     Why not a padded pitch: one image is read both ways (K in phase A: row fragments for S, transposed for dQ; Q and dO in phase B
//     likewise).  A transpose-read lane group (32 lanes, ds_read_b64_tr_b16) covers 4 consecutive rows x 64 bytes = 256 bytes, which
//     is exactly the 64 banks once if and only if the 4 rows are contiguous: any pitch above 64 bytes makes them overlap (80 bytes:
//     rows 0 and 3 share 12 banks, a 2-way conflict on every transposed read).  Unpadded rows alone would make the row fragments
//     4-way conflicted (ds_read_b128 serves 16 lanes per cycle, rows r and r + 4 land on the same banks), so the parts are XOR-rotated:
//       - row fragment, ds_read_b128, lane = row r0 + j, logical part 2 ks + hf.  The four lane groups hold, per half-wave, the rows
//         {0-3, 12-15, 20-27} or {4-11, 16-19, 28-31}.  The 4-bank span of a lane is 4 (r & 3) + (part ^ ((r >> 2) & 3)); in either
//         set the four rows of equal r & 3 have (r >> 2) & 3 = {0, 3, 1, 2} or {1, 2, 0, 3}: 16 distinct spans, conflict-free.
//       - transposed fragment, lanes 0-31 read rows r0 + {0..3} (r0 % 4 == 0: one rotation for all four rows, a permutation of the
//         parts inside each row), lanes 32-63 rows r0 + 4 + {0..3}: every group reads 4 whole rows = 64 distinct banks.
//       - staging stores (ds_write_b128, 8 consecutive lanes per cycle = 2 rows x 4 parts): 128 contiguous bytes, permuted.
//   * The V image of the forward uses the same layout (the 128-byte-row rotation of vit.hip has no meaning at 64-byte rows): it is
//     only read transposed, and the argument above holds for it unchanged.
//   * Staging is 4 sixteen-byte parts per row; every global load of a thread is issued before its first LDS store.
//   * ds_read_b64_tr_b16 needs EXEC all ones: lanes past T clamp their global addresses and skip stores only; a wave whose tile is
//     past T skips its work by a wave-uniform branch and still reaches every barrier.
#include "mfma.h"

namespace {

typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;

constexpr int V32_THREADS = 512;   // 8 waves
constexpr int V32_DK = 32;
constexpr int V32_ROWB = 64;       // bytes of an LDS row: 32 bf16, unpadded
constexpr float V32_LOG2E = 1.44269504088896340736f;
constexpr float V32_LN2 = 0.69314718055994530942f;

// byte offset of the 16-byte part c (0..3) of row r inside an image
__device__ __forceinline__ int v32_off(int r, int c) { return r * V32_ROWB + 16 * (c ^ ((r >> 2) & 3)); }

// Lane-constant addressing of the two fragment forms (byte offsets relative to the first row of a 32-row / 16-row group).
struct V32Lane {
    int lane, j, hf;
    int rf[2];   // row fragment of k-step ks: row j, logical part 2 ks + hf
    int tr[2];   // transposed fragment: rows 4 hf + (ti >> 2) and the same + 8, columns 16 (tg & 1) + 4 (ti & 3) .. + 3
    __device__ __forceinline__ V32Lane() {
        lane = threadIdx.x & 63;
        j = lane & 31, hf = lane >> 5;
        rf[0] = v32_off(j, hf);
        rf[1] = v32_off(j, 2 + hf);
        const int tg = lane >> 4, ti = lane & 15;
        const int row = 4 * (tg >> 1) + (ti >> 2), part = 2 * (tg & 1) + ((ti & 3) >> 1), half = 8 * (ti & 1);
        tr[0] = v32_off(row, part) + half;
        tr[1] = v32_off(row + 8, part) + half;
    }
    // A or B operand with the image's row r0 + j on the lane (r0 % 32 == 0): columns 16 ks + 8 hf .. + 7
    __device__ __forceinline__ bf16x8 row_frag(const unsigned char* img, int r0, int ks) const {
        return __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(img + r0 * V32_ROWB + rf[ks]));
    }
    // A operand with the image's COLUMN j on the lane (r0 % 16 == 0): rows r0 + 4 hf + {0..3} and the same + 8 in the registers,
    // the order in which a C tile holds its rows, so P^T / dS^T feed the next product without lane movement
    __device__ __forceinline__ bf16x8 col_frag(const unsigned char* img, int r0) const {
        const unsigned char* p = img + r0 * V32_ROWB;
        return tr_frag(p + tr[0], p + tr[1]);
    }
};

// Rows 0 .. ROWS-1 of two [T, 32] matrices (row strides ld0, ld1 elements, first row `base`) into two images of NP planes each
// (plane stride IMG bytes); rows >= T are zero.  Every global load of the thread is issued before its first LDS store.
template <int ROWS, bool X3, typename elt_t>
__device__ __forceinline__ void v32_stage(const elt_t* __restrict__ p0, int64_t ld0, const elt_t* __restrict__ p1, int64_t ld1, int64_t base,
                                          int T, unsigned char* img0, unsigned char* img1) {
    constexpr int IMG = ROWS * V32_ROWB;
    constexpr int NI = (ROWS * 4 + V32_THREADS - 1) / V32_THREADS;
    if constexpr (X3) {
        f32x8 s0[NI], s1[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int c = threadIdx.x + V32_THREADS * i;
            const int row = c >> 2, part = c & 3;
            s0[i] = f32x8{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            s1[i] = s0[i];
            if (row < T && row < ROWS) {
                s0[i] = load8(p0 + (base + row) * ld0 + part * 8);
                s1[i] = load8(p1 + (base + row) * ld1 + part * 8);
            }
        }
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int c = threadIdx.x + V32_THREADS * i;
            const int row = c >> 2, part = c & 3;
            if (row < ROWS) {
                u32x4 h0, l0, h1, l1;
                split8(s0[i], h0, l0);
                split8(s1[i], h1, l1);
                const int off = v32_off(row, part);
                *reinterpret_cast<u32x4*>(img0 + off) = h0;
                *reinterpret_cast<u32x4*>(img0 + IMG + off) = l0;
                *reinterpret_cast<u32x4*>(img1 + off) = h1;
                *reinterpret_cast<u32x4*>(img1 + IMG + off) = l1;
            }
        }
    } else {
        u32x4 s0[NI], s1[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int c = threadIdx.x + V32_THREADS * i;
            const int row = c >> 2, part = c & 3;
            s0[i] = u32x4{0u, 0u, 0u, 0u};
            s1[i] = s0[i];
            if (row < T && row < ROWS) {
                s0[i] = *reinterpret_cast<const u32x4*>(p0 + (base + row) * ld0 + part * 8);
                s1[i] = *reinterpret_cast<const u32x4*>(p1 + (base + row) * ld1 + part * 8);
            }
        }
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int c = threadIdx.x + V32_THREADS * i;
            const int row = c >> 2, part = c & 3;
            if (row < ROWS) {
                const int off = v32_off(row, part);
                *reinterpret_cast<u32x4*>(img0 + off) = s0[i];
                *reinterpret_cast<u32x4*>(img1 + off) = s1[i];
            }
        }
    }
}

// a row of a [T, 32] matrix in HBM as a B operand (lane = row), split when X3
template <bool X3, typename elt_t>
__device__ __forceinline__ void v32_load_rows(const elt_t* __restrict__ p, int hf, bf16x8 (&hi)[2], bf16x8 (&lo)[X3 ? 2 : 1]) {
    static_for<0, 2>([&](auto ks) __attribute__((always_inline)) {
        if constexpr (X3)
            split8(load8(p + 16 * ks + 8 * hf), hi[ks], lo[ks]);
        else
            hi[ks] = load_frag(p + 16 * ks + 8 * hf);
    });
}

// acc += (image rows r0 + 16 u ..)^T x (registers 8 u .. 8 u + 7 of x), u = 0, 1: a [32 columns] x [32 lanes] product over 32 rows
template <int IMG, bool X3>
__device__ __forceinline__ void v32_tr_product(const V32Lane& L, const unsigned char* img, int r0, const f32x16& x, f32x16& acc) {
    static_for<0, 2>([&](auto u_t) __attribute__((always_inline)) {
        constexpr int u = decltype(u_t)::value;
        f32x8 xv;
#pragma unroll
        for (int e = 0; e < 8; ++e) xv[e] = x[8 * u + e];
        if constexpr (X3) {
            bf16x8 xh, xl;
            split8(xv, xh, xl);
            const bf16x8 ah = L.col_frag(img, r0 + 16 * u), al = L.col_frag(img + IMG, r0 + 16 * u);
            acc = mfma(ah, xl, acc);
            acc = mfma(al, xh, acc);
            acc = mfma(ah, xh, acc);
        } else {
            acc = mfma(L.col_frag(img, r0 + 16 * u), __builtin_convertvector(xv, bf16x8), acc);
        }
    });
}

// store a transposed 32 x 32 result (lane = row of the output matrix, 4 consecutive columns per register group) times f
template <bool X3, typename elt_t>
__device__ __forceinline__ void v32_store_rows(elt_t* __restrict__ p, int hf, const f32x16& acc, float f) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const f32x4 o4 = {acc[4 * g] * f, acc[4 * g + 1] * f, acc[4 * g + 2] * f, acc[4 * g + 3] * f};
        const int d0 = 8 * g + 4 * hf;
        if constexpr (X3)
            *reinterpret_cast<f32x4*>(p + d0) = o4;
        else
            *reinterpret_cast<u32x2*>(p + d0) = __builtin_bit_cast(u32x2, __builtin_convertvector(o4, bf16x4));
    }
}

template <int NKB, bool X3>
constexpr size_t v32_fwd_lds_bytes() {
    return (size_t)2 * (X3 ? 2 : 1) * (32 * NKB * V32_ROWB);
}
template <int NKB, bool X3>
constexpr size_t v32_bwd_lds_bytes() {
    return (size_t)2 * (X3 ? 2 : 1) * (32 * NKB * V32_ROWB) + (size_t)2 * 32 * NKB * sizeof(float);
}

// ---------------------------------------------------------------------------------------------------------------- forward
template <int NKB, bool X3>
__global__ __launch_bounds__(V32_THREADS, X3 ? 2 : 4) void vit_attn32_fwd_kernel(const void* __restrict__ qkv_, int B, int T, int h, float scale,
                                                                                void* __restrict__ out_, float* __restrict__ lse) {
    constexpr int DK = V32_DK;
    constexpr int NP = X3 ? 2 : 1;
    constexpr int ROWS = 32 * NKB;
    constexpr int IMG = ROWS * V32_ROWB;
    typedef typename std::conditional<X3, float, unsigned short>::type elt_t;
    const elt_t* __restrict__ qkv = reinterpret_cast<const elt_t*>(qkv_);
    elt_t* __restrict__ out = reinterpret_cast<elt_t*>(out_);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* const img_k = smem;              // [NP][ROWS][64 B]
    unsigned char* const img_v = smem + NP * IMG;   // [NP][ROWS][64 B]

    const int a = blockIdx.x, b = blockIdx.y;
    const int D = h * DK;
    const int64_t base = (int64_t)b * T;
    const V32Lane L;
    const int j = L.j, hf = L.hf;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ntile = (T + 31) / 32;
    const bool active = w < ntile;   // wave-uniform: this wave owns query tile w
    const float c_exp = scale * V32_LOG2E;

    // this wave's queries are requested before the staging: B operand of S^T = K Q^T, lane = query (clamped past T)
    const int q_row = 32 * w + j;
    bf16x8 qh[2], ql[X3 ? 2 : 1];
    if (active) v32_load_rows<X3>(qkv + (base + (q_row < T ? q_row : T - 1)) * 3 * D + a * DK, hf, qh, ql);
    v32_stage<ROWS, X3>(qkv + D + a * DK, 3 * (int64_t)D, qkv + 2 * D + a * DK, 3 * (int64_t)D, base, T, img_k, img_v);
    __syncthreads();
    if (!active) return;   // no barrier follows

    f32x16 o_acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) o_acc[r] = 0.f;
    float m_run = -INFINITY, l_lane = 0.f;   // running max (all-reduced over the two half-waves), lane-local sum
#pragma unroll 1
    for (int jb = 0; jb < ntile; ++jb) {
        // S^T block: keys in registers (register r = key 32 jb + (r & 3) + 8 (r >> 2) + 4 hf), this lane's query on the lane
        f32x16 s_acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key = 32 * jb + (r & 3) + 8 * (r >> 2) + 4 * hf;
            s_acc[r] = (key >= T) ? -INFINITY : 0.f;
        }
        static_for<0, 2>([&](auto ks) __attribute__((always_inline)) {
            const bf16x8 kh = L.row_frag(img_k, 32 * jb, ks);
            if constexpr (X3) {
                const bf16x8 kl = L.row_frag(img_k + IMG, 32 * jb, ks);
                s_acc = mfma(kh, ql[ks], s_acc);
                s_acc = mfma(kl, qh[ks], s_acc);
            }
            s_acc = mfma(kh, qh[ks], s_acc);
        });
        float mb0 = fmaxf(s_acc[0], s_acc[1]), mb1 = fmaxf(s_acc[2], s_acc[3]);
#pragma unroll
        for (int r = 4; r < 16; r += 4) {
            mb0 = fmaxf(fmaxf(mb0, s_acc[r]), s_acc[r + 1]);
            mb1 = fmaxf(fmaxf(mb1, s_acc[r + 2]), s_acc[r + 3]);
        }
        // the first block always holds a valid key, so m_new is finite from the first block on
        const float m_new = fmaxf(m_run, xhalf_max(fmaxf(mb0, mb1)));
        const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * c_exp);   // exp2(-inf) = 0 on the first block
        const float mc = m_new * c_exp;
        m_run = m_new;
        float lsum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float e = __builtin_amdgcn_exp2f(fmaf(s_acc[r], c_exp, -mc));
            s_acc[r] = e;
            lsum += e;
        }
        l_lane = fmaf(l_lane, alpha, lsum);
#pragma unroll
        for (int r = 0; r < 16; ++r) o_acc[r] *= alpha;
        v32_tr_product<IMG, X3>(L, img_v, 32 * jb, s_acc, o_acc);   // O^T += V^T P^T
    }
    const float l = xhalf_sum(l_lane);
    if (q_row < T) {
        // the row statistic the backward rebuilds P from: log sum_j exp(scale s_j) = scale max + log l
        if (hf == 0) lse[((int64_t)b * h + a) * T + q_row] = fmaf(m_run, scale, __builtin_amdgcn_logf(l) * V32_LN2);
        v32_store_rows<X3>(out + (base + q_row) * D + a * DK, hf, o_acc, __builtin_amdgcn_rcpf(l));
    }
}

// ---------------------------------------------------------------------------------------------------------------- backward
template <int NKB, bool X3>
__global__ __launch_bounds__(V32_THREADS, 1) void vit_attn32_bwd_kernel(const void* __restrict__ qkv_, const void* __restrict__ dout_,
                                                                       const float* __restrict__ lse, int B, int T, int h, float scale,
                                                                       void* __restrict__ dqkv_) {
    constexpr int DK = V32_DK;
    constexpr int NP = X3 ? 2 : 1;
    constexpr int ROWS = 32 * NKB;
    constexpr int IMG = ROWS * V32_ROWB;
    typedef typename std::conditional<X3, float, unsigned short>::type elt_t;
    const elt_t* __restrict__ qkv = reinterpret_cast<const elt_t*>(qkv_);
    const elt_t* __restrict__ dout = reinterpret_cast<const elt_t*>(dout_);
    elt_t* __restrict__ dqkv = reinterpret_cast<elt_t*>(dqkv_);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // images [matrix 0 / 1][plane][ROWS][64 B] (phase A: K, V; phase B: Q, dO), then lse * log2(e) and D per query
    unsigned char* const img0 = smem;
    unsigned char* const img1 = smem + NP * IMG;
    float* const lse2_l = reinterpret_cast<float*>(smem + 2 * NP * IMG);
    float* const d_l = lse2_l + ROWS;

    const int a = blockIdx.x, b = blockIdx.y;
    const int D = h * DK;
    const int64_t base = (int64_t)b * T;
    const V32Lane L;
    const int j = L.j, hf = L.hf;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ntile = (T + 31) / 32;
    const bool active = w < ntile;   // wave-uniform: this wave owns query tile w (phase A) and key tile w (phase B)
    const float c_exp = scale * V32_LOG2E;

    // ------------------------------------------------------------ phase A: D and dQ of query tile w
    v32_stage<ROWS, X3>(qkv + D + a * DK, 3 * (int64_t)D, qkv + 2 * D + a * DK, 3 * (int64_t)D, base, T, img0, img1);
    __syncthreads();
    if (active) {
        const int q_row = 32 * w + j;
        const int q_ld = q_row < T ? q_row : T - 1;   // lanes past T recompute the last row and store nothing
        bf16x8 qh[2], ql[X3 ? 2 : 1], gh[2], gl[X3 ? 2 : 1];
        v32_load_rows<X3>(qkv + (base + q_ld) * 3 * D + a * DK, hf, qh, ql);
        v32_load_rows<X3>(dout + (base + q_ld) * D + a * DK, hf, gh, gl);
        const float lse2 = lse[((int64_t)b * h + a) * T + q_ld] * V32_LOG2E;
        // P^T and dP^T of key block jb: lane = query, register r = key 32 jb + (r & 3) + 8 (r >> 2) + 4 hf
        auto p_dp = [&](int jb, f32x16& p, f32x16& dp) __attribute__((always_inline)) {
#pragma unroll
            for (int r = 0; r < 16; ++r) p[r] = 0.f, dp[r] = 0.f;
            static_for<0, 2>([&](auto ks) __attribute__((always_inline)) {
                const bf16x8 kh = L.row_frag(img0, 32 * jb, ks), vh = L.row_frag(img1, 32 * jb, ks);
                if constexpr (X3) {
                    const bf16x8 kl = L.row_frag(img0 + IMG, 32 * jb, ks), vl = L.row_frag(img1 + IMG, 32 * jb, ks);
                    p = mfma(kh, ql[ks], p);
                    p = mfma(kl, qh[ks], p);
                    dp = mfma(vh, gl[ks], dp);
                    dp = mfma(vl, gh[ks], dp);
                }
                p = mfma(kh, qh[ks], p);
                dp = mfma(vh, gh[ks], dp);
            });
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = 32 * jb + (r & 3) + 8 * (r >> 2) + 4 * hf;
                const float e = __builtin_amdgcn_exp2f(fmaf(p[r], c_exp, -lse2));
                p[r] = key < T ? e : 0.f;
            }
        };
        float d_lane = 0.f;
#pragma unroll 1
        for (int jb = 0; jb < ntile; ++jb) {
            f32x16 p, dp;
            p_dp(jb, p, dp);
#pragma unroll
            for (int r = 0; r < 16; ++r) d_lane = fmaf(p[r], dp[r], d_lane);
        }
        const float d_row = xhalf_sum(d_lane);   // the two half-waves hold the two halves of the row's keys
        f32x16 dq;
#pragma unroll
        for (int r = 0; r < 16; ++r) dq[r] = 0.f;
#pragma unroll 1
        for (int jb = 0; jb < ntile; ++jb) {
            f32x16 p, dp;
            p_dp(jb, p, dp);
#pragma unroll
            for (int r = 0; r < 16; ++r) p[r] *= dp[r] - d_row;
            v32_tr_product<IMG, X3>(L, img0, 32 * jb, p, dq);   // dQ^T += K^T dS^T
        }
        if (q_row < T) v32_store_rows<X3>(dqkv + (base + q_row) * 3 * D + a * DK, hf, dq, scale);
        if (hf == 0) {   // rows past T: finite values, so that their (zero) Q and dO rows give dS = 0 and add nothing in phase B
            lse2_l[q_row] = q_row < T ? lse2 : 0.f;
            d_l[q_row] = q_row < T ? d_row : 0.f;
        }
    }

    // ------------------------------------------------------------ phase B: dK and dV of key tile w
    bf16x8 kh[2], kl[X3 ? 2 : 1], vh[2], vl[X3 ? 2 : 1];
    if (active) {
        static_for<0, 2>([&](auto ks) __attribute__((always_inline)) {
            kh[ks] = L.row_frag(img0, 32 * w, ks);
            vh[ks] = L.row_frag(img1, 32 * w, ks);
            if constexpr (X3) {
                kl[ks] = L.row_frag(img0 + IMG, 32 * w, ks);
                vl[ks] = L.row_frag(img1 + IMG, 32 * w, ks);
            }
        });
    }
    __syncthreads();   // every wave is done with the images of K and V
    v32_stage<ROWS, X3>(qkv + a * DK, 3 * (int64_t)D, dout + a * DK, (int64_t)D, base, T, img0, img1);
    __syncthreads();
    if (active) {
        f32x16 dk, dv;
#pragma unroll
        for (int r = 0; r < 16; ++r) dk[r] = 0.f, dv[r] = 0.f;
#pragma unroll 1
        for (int qt = 0; qt < ntile; ++qt) {
            // P of query tile qt: lane = key, register r = query 32 qt + (r & 3) + 8 (r >> 2) + 4 hf.  P is consumed by dV before
            // dP is formed, which keeps the live tiles at two
            f32x16 p, dp;
#pragma unroll
            for (int r = 0; r < 16; ++r) p[r] = 0.f, dp[r] = 0.f;
            static_for<0, 2>([&](auto ks) __attribute__((always_inline)) {
                const bf16x8 ah = L.row_frag(img0, 32 * qt, ks);
                if constexpr (X3) {   // the same three terms in the same order as phase A: S is rebuilt, not approximated
                    const bf16x8 al = L.row_frag(img0 + IMG, 32 * qt, ks);
                    p = mfma(al, kh[ks], p);
                    p = mfma(ah, kl[ks], p);
                }
                p = mfma(ah, kh[ks], p);
            });
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 l4 = *reinterpret_cast<const f32x4*>(lse2_l + 32 * qt + 8 * g + 4 * hf);
#pragma unroll
                for (int e = 0; e < 4; ++e) p[4 * g + e] = __builtin_amdgcn_exp2f(fmaf(p[4 * g + e], c_exp, -l4[e]));
            }
            v32_tr_product<IMG, X3>(L, img1, 32 * qt, p, dv);    // dV^T += dO^T P
            static_for<0, 2>([&](auto ks) __attribute__((always_inline)) {
                const bf16x8 gh = L.row_frag(img1, 32 * qt, ks);
                if constexpr (X3) {
                    const bf16x8 gl = L.row_frag(img1 + IMG, 32 * qt, ks);
                    dp = mfma(gl, vh[ks], dp);
                    dp = mfma(gh, vl[ks], dp);
                }
                dp = mfma(gh, vh[ks], dp);
            });
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 d4 = *reinterpret_cast<const f32x4*>(d_l + 32 * qt + 8 * g + 4 * hf);
#pragma unroll
                for (int e = 0; e < 4; ++e) dp[4 * g + e] = p[4 * g + e] * (dp[4 * g + e] - d4[e]);
            }
            v32_tr_product<IMG, X3>(L, img0, 32 * qt, dp, dk);   // dK^T += Q^T dS
        }
        const int key = 32 * w + j;
        if (key < T) {
            v32_store_rows<X3>(dqkv + (base + key) * 3 * D + D + a * DK, hf, dk, scale);
            v32_store_rows<X3>(dqkv + (base + key) * 3 * D + 2 * D + a * DK, hf, dv, 1.0f);
        }
    }
}

// T == 1: dqkv row = (0 | 0 | dout row)
template <typename elt_t>
__global__ __launch_bounds__(256) void vit_attn32_bwd_t1_kernel(const elt_t* __restrict__ dout, int64_t total, int D, elt_t* __restrict__ dqkv) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = i / (3 * D);
        const int col = (int)(i - row * 3 * D);
        dqkv[i] = col >= 2 * D ? dout[row * D + col - 2 * D] : elt_t(0);
    }
}

template <int NKB, bool X3>
int launch_v32_fwd(const void* qkv, int B, int T, int h, float scale, void* out, float* lse, hipStream_t s) {
    constexpr size_t lds = v32_fwd_lds_bytes<NKB, X3>();
    static_assert(lds <= 160 * 1024, "vit_attn32_fwd: LDS budget");
    auto kern = vit_attn32_fwd_kernel<NKB, X3>;
    static thread_local unsigned long long attr_set_mask = 0;   // devices (bit = device id) that have the opt-in
    if (lds > 48 * 1024)
        if (int rc = snf::lds_opt_in(reinterpret_cast<const void*>(kern), lds, &attr_set_mask, "vit_attn32_fwd")) return rc;
    hipLaunchKernelGGL(kern, dim3(h, B), dim3(V32_THREADS), lds, s, qkv, B, T, h, scale, out, lse);
    return snf::check_launch("vit_attn32_fwd_kernel");
}

template <int NKB, bool X3>
int launch_v32_bwd(const void* qkv, const void* dout, const float* lse, int B, int T, int h, float scale, void* dqkv, hipStream_t s) {
    constexpr size_t lds = v32_bwd_lds_bytes<NKB, X3>();
    static_assert(lds <= 160 * 1024, "vit_attn32_bwd: LDS budget");
    auto kern = vit_attn32_bwd_kernel<NKB, X3>;
    static thread_local unsigned long long attr_set_mask = 0;
    if (lds > 48 * 1024)
        if (int rc = snf::lds_opt_in(reinterpret_cast<const void*>(kern), lds, &attr_set_mask, "vit_attn32_bwd")) return rc;
    hipLaunchKernelGGL(kern, dim3(h, B), dim3(V32_THREADS), lds, s, qkv, dout, lse, B, T, h, scale, dqkv);
    return snf::check_launch("vit_attn32_bwd_kernel");
}

template <bool X3>
int dispatch_v32_fwd(const void* qkv, int B, int T, int h, float scale, void* out, float* lse, hipStream_t s) {
    const int nkb = (T + 31) / 32;
    if (nkb <= 2) return launch_v32_fwd<2, X3>(qkv, B, T, h, scale, out, lse, s);
    if (nkb <= 4) return launch_v32_fwd<4, X3>(qkv, B, T, h, scale, out, lse, s);
    return launch_v32_fwd<8, X3>(qkv, B, T, h, scale, out, lse, s);
}

template <bool X3>
int dispatch_v32_bwd(const void* qkv, const void* dout, const float* lse, int B, int T, int h, float scale, void* dqkv, hipStream_t s) {
    const int nkb = (T + 31) / 32;
    if (nkb <= 2) return launch_v32_bwd<2, X3>(qkv, dout, lse, B, T, h, scale, dqkv, s);
    if (nkb <= 4) return launch_v32_bwd<4, X3>(qkv, dout, lse, B, T, h, scale, dqkv, s);
    return launch_v32_bwd<8, X3>(qkv, dout, lse, B, T, h, scale, dqkv, s);
}

inline bool v32_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" {

int snf_vit_attention_dk32_fwd_lse(const void* qkv, int dtype, int b, int t, int h, int dk, float scale, void* out, float* lse,
                                   snf_stream_t stream) {
    SNF_REQUIRE(qkv && out && lse, "snf_vit_attention_dk32_fwd_lse: null pointer");
    SNF_REQUIRE(dtype == SNF_DT_F32 || dtype == SNF_DT_BF16, "snf_vit_attention_dk32_fwd_lse: dtype is f32 (fp32 class) or bf16 (got %d)", dtype);
    SNF_REQUIRE(b >= 1 && t >= 1 && h >= 1, "snf_vit_attention_dk32_fwd_lse: bad shape");
    if (dk != V32_DK || t > SNF_VIT_DK32_MAX_T || b > 65535) {
        snf::set_error("snf_vit_attention_dk32_fwd_lse: unsupported shape dk=%d t=%d b=%d (need dk == 32, t <= %d, b <= 65535)", dk, t, b,
                       SNF_VIT_DK32_MAX_T);
        return SNF_EUNSUPPORTED;
    }
    if (!v32_aligned16(qkv) || !v32_aligned16(out) || (reinterpret_cast<uintptr_t>(lse) & 3) != 0) {
        snf::set_error("snf_vit_attention_dk32_fwd_lse: unsupported operands: qkv and out must be 16-byte aligned (16-byte vector loads and stores)");
        return SNF_EUNSUPPORTED;
    }
    hipStream_t s = snf::as_stream(stream);
    return dtype == SNF_DT_F32 ? dispatch_v32_fwd<true>(qkv, b, t, h, scale, out, lse, s) : dispatch_v32_fwd<false>(qkv, b, t, h, scale, out, lse, s);
}

int snf_vit_attention_dk32_bwd(const void* qkv, const void* dout, const float* lse, int dtype, int b, int t, int h, int dk, float scale,
                               void* dqkv, snf_stream_t stream) {
    SNF_REQUIRE(qkv && dout && lse && dqkv, "snf_vit_attention_dk32_bwd: null pointer");
    SNF_REQUIRE(dtype == SNF_DT_F32 || dtype == SNF_DT_BF16, "snf_vit_attention_dk32_bwd: dtype is f32 (fp32 class) or bf16 (got %d)", dtype);
    SNF_REQUIRE(b >= 1 && t >= 1 && h >= 1, "snf_vit_attention_dk32_bwd: bad shape");
    if (dk != V32_DK || t > SNF_VIT_DK32_MAX_T || b > 65535) {
        snf::set_error("snf_vit_attention_dk32_bwd: unsupported shape dk=%d t=%d b=%d (need dk == 32, t <= %d, b <= 65535)", dk, t, b,
                       SNF_VIT_DK32_MAX_T);
        return SNF_EUNSUPPORTED;
    }
    if (!v32_aligned16(qkv) || !v32_aligned16(dout) || !v32_aligned16(dqkv) || (reinterpret_cast<uintptr_t>(lse) & 3) != 0) {
        snf::set_error("snf_vit_attention_dk32_bwd: unsupported operands: qkv, dout and dqkv must be 16-byte aligned (16-byte vector loads and stores)");
        return SNF_EUNSUPPORTED;
    }
    hipStream_t s = snf::as_stream(stream);
    const bool x3 = dtype == SNF_DT_F32;
    if (t == 1) {
        const int64_t total = (int64_t)b * 3 * h * dk;
        const int grid = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
        if (x3)
            hipLaunchKernelGGL(vit_attn32_bwd_t1_kernel<float>, dim3(grid), dim3(256), 0, s, reinterpret_cast<const float*>(dout), total, h * dk,
                               reinterpret_cast<float*>(dqkv));
        else
            hipLaunchKernelGGL(vit_attn32_bwd_t1_kernel<unsigned short>, dim3(grid), dim3(256), 0, s,
                               reinterpret_cast<const unsigned short*>(dout), total, h * dk, reinterpret_cast<unsigned short*>(dqkv));
        return snf::check_launch("vit_attn32_bwd_t1_kernel");
    }
    return x3 ? dispatch_v32_bwd<true>(qkv, dout, lse, b, t, h, scale, dqkv, s) : dispatch_v32_bwd<false>(qkv, dout, lse, b, t, h, scale, dqkv, s);
}

}  // extern "C"
