// Backward of the ViT self-attention of csrc/vit.hip on the matrix cores (gfx950), dk = 64, 256 < T <= 4096: the two phases of
// csrc/vit_attn_bwd.hip as two launches on one stream, each a loop over 256-row chunks of the side it stages in LDS.
//
//   snf_vit_attention_bwd_long   qkv [B*T, 3*h*64] (q | k | v), dout [B*T, h*64], lse [B, h, T] (natural log, what
//                                snf_vit_attention_fwd_lse wrote), dwork [B, h, T] f32 (scratch) -> dqkv [B*T, 3*h*64], fully written.
//
// The arithmetics are those of vit_attn_bwd.hip: SNF_DT_F32 is the fp32 class (every operand hi + lo, every product
// hi lo + lo hi + hi hi on v_mfma_f32_32x32x16_bf16, fp32 accumulation, P and dS split in registers), SNF_DT_BF16 has bf16 operands.
//
// Both kernels: grid (h, B, ceil(T / 256)), 8 waves.  Wave w of the workgroup at z = c owns tile 8 c + w (32 rows).
//
//   vit_attention_bwd_dq_kernel   the wave holds the Q and dO rows and lse of its query tile in registers; the workgroup walks the key
//                                 chunks (256 rows of K and V staged row-major, one or two bf16 planes) twice:
//                                   first walk   S^T = K Q^T, P = exp(scale S - lse), dP^T = V dO^T, D_i = sum_j P_ij dP_ij
//                                   second walk  dS^T = P o (dP - D), dQ^T += K^T dS^T
//                                 and stores dQ * scale and D (rows < T, [B, h, T] workspace in HBM).
//   vit_attention_bwd_dkv_kernel  the wave holds the K and V fragments of its key tile in registers (straight from HBM); the workgroup
//                                 walks the query chunks (256 rows of Q and dO staged, lse * log2 e and D of the chunk in two small LDS
//                                 arrays; rows >= T: zero Q and dO, lse = D = 0, so that their dS is exactly 0):
//                                   S = Q K^T (the three x3 terms of the dQ kernel in its order: S is rebuilt, not approximated), P,
//                                   dV^T += dO^T P, dP = dO V^T, dS, dK^T += Q^T dS
//                                 and stores dK * scale and dV once.
//
// A wave whose tile is past T does no arithmetic and takes part in every staging loop and every barrier of the chunk walk.  Nothing is
// reduced across waves or workgroups and there are no atomics: every output element has one owner and one summation order.
#include "mfma.h"

namespace {

typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;

constexpr int VL_THREADS = 512;   // 8 waves
constexpr int VL_ROWS = 256;      // rows of one staged chunk: 8 tiles of 32
constexpr int VL_PITCH = 64 + 8;  // bf16 elements per LDS row: 144-byte rows, conflict-free 16-byte fragment reads
constexpr int VL_IMG = VL_ROWS * VL_PITCH * 2;   // bytes of one plane of one staged matrix
constexpr float VL_LOG2E = 1.44269504088896340736f;

template <bool X3>
constexpr size_t vl_lds_bytes() {
    return (size_t)2 * (X3 ? 2 : 1) * VL_IMG + (size_t)2 * VL_ROWS * sizeof(float);
}

template <bool X3>
struct vl_elt {
    typedef typename std::conditional<X3, float, unsigned short>::type type;
};

// rows row0 .. row0 + 255 of two [T, 64] matrices of image `base / T` (row strides ld0, ld1 elements) into the two images; rows >= T
// are zero.  Workgroup-wide: every thread runs it.  Every global load of the thread is issued before its first LDS store.
template <bool X3>
__device__ __forceinline__ void vl_stage(unsigned char* img0, unsigned char* img1, const typename vl_elt<X3>::type* __restrict__ p0,
                                         int64_t ld0, const typename vl_elt<X3>::type* __restrict__ p1, int64_t ld1, int64_t base,
                                         int row0, int T) {
    constexpr int NI = VL_ROWS * 8 / VL_THREADS;
    if constexpr (X3) {
        f32x8 s0[NI], s1[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int c = threadIdx.x + VL_THREADS * i;
            const int row = row0 + (c >> 3), part = c & 7;
            s0[i] = f32x8{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            s1[i] = s0[i];
            if (row < T) {
                s0[i] = load8(p0 + (base + row) * ld0 + part * 8);
                s1[i] = load8(p1 + (base + row) * ld1 + part * 8);
            }
        }
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int c = threadIdx.x + VL_THREADS * i;
            u32x4 h0, l0, h1, l1;
            split8(s0[i], h0, l0);
            split8(s1[i], h1, l1);
            const int off = ((c >> 3) * VL_PITCH + (c & 7) * 8) * 2;
            *reinterpret_cast<u32x4*>(img0 + off) = h0;
            *reinterpret_cast<u32x4*>(img0 + VL_IMG + off) = l0;
            *reinterpret_cast<u32x4*>(img1 + off) = h1;
            *reinterpret_cast<u32x4*>(img1 + VL_IMG + off) = l1;
        }
    } else {
        u32x4 s0[NI], s1[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int c = threadIdx.x + VL_THREADS * i;
            const int row = row0 + (c >> 3), part = c & 7;
            s0[i] = u32x4{0u, 0u, 0u, 0u};
            s1[i] = s0[i];
            if (row < T) {
                s0[i] = *reinterpret_cast<const u32x4*>(p0 + (base + row) * ld0 + part * 8);
                s1[i] = *reinterpret_cast<const u32x4*>(p1 + (base + row) * ld1 + part * 8);
            }
        }
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int c = threadIdx.x + VL_THREADS * i;
            const int off = ((c >> 3) * VL_PITCH + (c & 7) * 8) * 2;
            *reinterpret_cast<u32x4*>(img0 + off) = s0[i];
            *reinterpret_cast<u32x4*>(img1 + off) = s1[i];
        }
    }
}

// row fragment (A or B operand with the image's row on the lane): row r0 + (lane & 31), columns 16 ks + 8 (lane >> 5) .. + 7
__device__ __forceinline__ bf16x8 vl_row_frag(const unsigned char* img, int r0, int ks) {
    const int lane = threadIdx.x & 63;
    return __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(img + ((r0 + (lane & 31)) * VL_PITCH + 16 * ks + 8 * (lane >> 5)) * 2));
}

// transposed fragment (A operand with the image's COLUMN 32 db + j on the lane): rows r0 + 4 hf + {0..3} and the same + 8 in the
// registers -- the order in which a C tile holds its rows, so P^T / dS^T feed the next product without lane movement
__device__ __forceinline__ bf16x8 vl_col_frag(const unsigned char* img, int r0, int db) {
    const int lane = threadIdx.x & 63;
    const int tg = lane >> 4, ti = lane & 15;
    const int tr_off = ((4 * (tg >> 1) + (ti >> 2)) * VL_PITCH) * 2 + 32 * (tg & 1) + 8 * (ti & 3);
    const unsigned char* p = img + r0 * (VL_PITCH * 2) + 64 * db + tr_off;
    return tr_frag(p, p + 8 * VL_PITCH * 2);
}

// a row of a [T, 64] matrix in HBM as a B operand (lane = row), split when X3
template <bool X3>
__device__ __forceinline__ void vl_load_rows(const typename vl_elt<X3>::type* __restrict__ p, bf16x8 (&hi)[4], bf16x8 (&lo)[X3 ? 4 : 1]) {
    const int hf = (threadIdx.x & 63) >> 5;
    static_for<0, 4>([&](auto ks) __attribute__((always_inline)) {
        if constexpr (X3)
            split8(load8(p + 16 * ks + 8 * hf), hi[ks], lo[ks]);
        else
            hi[ks] = load_frag(p + 16 * ks + 8 * hf);
    });
}

// acc[db] += (columns 32 db .. of image rows r0 + 16 u ..)^T x (registers 8 u .. 8 u + 7 of x), db = 0, 1, u = 0, 1
template <bool X3>
__device__ __forceinline__ void vl_tr_product(const unsigned char* img, int r0, const f32x16& x, f32x16 (&acc)[2]) {
    static_for<0, 2>([&](auto u_t) __attribute__((always_inline)) {
        constexpr int u = decltype(u_t)::value;
        f32x8 xv;
#pragma unroll
        for (int e = 0; e < 8; ++e) xv[e] = x[8 * u + e];
        if constexpr (X3) {
            bf16x8 xh, xl;
            split8(xv, xh, xl);
            static_for<0, 2>([&](auto db_t) __attribute__((always_inline)) {
                constexpr int db = decltype(db_t)::value;
                const bf16x8 ah = vl_col_frag(img, r0 + 16 * u, db), al = vl_col_frag(img + VL_IMG, r0 + 16 * u, db);
                acc[db] = mfma(ah, xl, acc[db]);
                acc[db] = mfma(al, xh, acc[db]);
                acc[db] = mfma(ah, xh, acc[db]);
            });
        } else {
            const bf16x8 xb = __builtin_convertvector(xv, bf16x8);
            static_for<0, 2>([&](auto db_t) __attribute__((always_inline)) {
                constexpr int db = decltype(db_t)::value;
                acc[db] = mfma(vl_col_frag(img, r0 + 16 * u, db), xb, acc[db]);
            });
        }
    });
}

// store a transposed 64 x 32 result (lane = row of the output matrix, 4 consecutive columns per register group) times f
template <bool X3>
__device__ __forceinline__ void vl_store_rows(typename vl_elt<X3>::type* __restrict__ p, const f32x16 (&acc)[2], float f) {
    const int hf = (threadIdx.x & 63) >> 5;
    static_for<0, 2>([&](auto db) __attribute__((always_inline)) {
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

__device__ __forceinline__ void vl_zero2(f32x16 (&acc)[2]) {
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[0][r] = 0.f, acc[1][r] = 0.f;
}

// ------------------------------------------------------------------------------------------------ D and dQ of query tile 8 z + w
template <bool X3>
__global__ __launch_bounds__(VL_THREADS, 1) void vit_attention_bwd_dq_kernel(const void* __restrict__ qkv_, const void* __restrict__ dout_,
                                                                             const float* __restrict__ lse, int B, int T, int h, float scale,
                                                                             float* __restrict__ dwork, void* __restrict__ dqkv_) {
    constexpr int DK = 64;
    constexpr int NP = X3 ? 2 : 1;   // operand planes (hi, lo)
    typedef typename vl_elt<X3>::type elt_t;
    const elt_t* __restrict__ qkv = reinterpret_cast<const elt_t*>(qkv_);
    const elt_t* __restrict__ dout = reinterpret_cast<const elt_t*>(dout_);
    elt_t* __restrict__ dqkv = reinterpret_cast<elt_t*>(dqkv_);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* const img0 = smem;               // K [plane][256][VL_PITCH] bf16
    unsigned char* const img1 = smem + NP * VL_IMG;   // V

    const int a = blockIdx.x, b = blockIdx.y;
    const int D = h * DK;
    const int64_t base = (int64_t)b * T;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = lane & 31, hf = lane >> 5;
    const int ntile = (T + 31) / 32;
    const int nchunk = (T + VL_ROWS - 1) / VL_ROWS;
    const int qt = 8 * (int)blockIdx.z + w;
    const bool active = qt < ntile;   // wave-uniform; an idle wave still stages and still reaches every barrier below
    const float c_exp = scale * VL_LOG2E;

    const int q_row = 32 * qt + j;
    const int q_ld = q_row < T ? q_row : T - 1;   // lanes past T (and idle waves) recompute the last row and store nothing
    bf16x8 qh[4], ql[X3 ? 4 : 1], gh[4], gl[X3 ? 4 : 1];
    vl_load_rows<X3>(qkv + (base + q_ld) * 3 * D + a * DK, qh, ql);
    vl_load_rows<X3>(dout + (base + q_ld) * D + a * DK, gh, gl);
    const float lse2 = lse[((int64_t)b * h + a) * T + q_ld] * VL_LOG2E;

    // P^T and dP^T of key block jb of the staged chunk (keys from key0): lane = query, register r = key key0 + 32 jb + (r & 3) + 8 (r >> 2) + 4 hf
    auto p_dp = [&](int key0, int jb, f32x16& p, f32x16& dp) __attribute__((always_inline)) {
#pragma unroll
        for (int r = 0; r < 16; ++r) p[r] = 0.f, dp[r] = 0.f;
        static_for<0, 4>([&](auto ks) __attribute__((always_inline)) {
            const bf16x8 kh = vl_row_frag(img0, 32 * jb, ks), vh = vl_row_frag(img1, 32 * jb, ks);
            if constexpr (X3) {
                const bf16x8 kl = vl_row_frag(img0 + VL_IMG, 32 * jb, ks), vl = vl_row_frag(img1 + VL_IMG, 32 * jb, ks);
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
            const int key = key0 + 32 * jb + (r & 3) + 8 * (r >> 2) + 4 * hf;   // the global key index
            const float e = __builtin_amdgcn_exp2f(fmaf(p[r], c_exp, -lse2));
            p[r] = key < T ? e : 0.f;
        }
    };

    // first walk: D
    float d_lane = 0.f;
#pragma unroll 1
    for (int kc = 0; kc < nchunk; ++kc) {
        if (kc) __syncthreads();   // every wave is done with the previous chunk
        vl_stage<X3>(img0, img1, qkv + D + a * DK, 3 * (int64_t)D, qkv + 2 * D + a * DK, 3 * (int64_t)D, base, VL_ROWS * kc, T);
        __syncthreads();
        if (active) {
            const int nb = ntile - 8 * kc < 8 ? ntile - 8 * kc : 8;
#pragma unroll 1
            for (int jb = 0; jb < nb; ++jb) {
                f32x16 p, dp;
                p_dp(VL_ROWS * kc, jb, p, dp);
#pragma unroll
                for (int r = 0; r < 16; ++r) d_lane = fmaf(p[r], dp[r], d_lane);
            }
        }
    }
    const float d_row = xhalf_sum(d_lane);   // the two half-waves hold the two halves of the row's keys

    // second walk: dQ
    f32x16 dq[2];
    vl_zero2(dq);
#pragma unroll 1
    for (int kc = 0; kc < nchunk; ++kc) {
        __syncthreads();
        vl_stage<X3>(img0, img1, qkv + D + a * DK, 3 * (int64_t)D, qkv + 2 * D + a * DK, 3 * (int64_t)D, base, VL_ROWS * kc, T);
        __syncthreads();
        if (active) {
            const int nb = ntile - 8 * kc < 8 ? ntile - 8 * kc : 8;
#pragma unroll 1
            for (int jb = 0; jb < nb; ++jb) {
                f32x16 p, dp;
                p_dp(VL_ROWS * kc, jb, p, dp);
#pragma unroll
                for (int r = 0; r < 16; ++r) p[r] *= dp[r] - d_row;
                vl_tr_product<X3>(img0, 32 * jb, p, dq);   // dQ^T += K^T dS^T
            }
        }
    }
    if (active && q_row < T) {
        vl_store_rows<X3>(dqkv + (base + q_row) * 3 * D + a * DK, dq, scale);
        if (hf == 0) dwork[((int64_t)b * h + a) * T + q_row] = d_row;
    }
}

// ------------------------------------------------------------------------------------------------ dK and dV of key tile 8 z + w
template <bool X3>
__global__ __launch_bounds__(VL_THREADS, 1) void vit_attention_bwd_dkv_kernel(const void* __restrict__ qkv_, const void* __restrict__ dout_,
                                                                              const float* __restrict__ lse, const float* __restrict__ dwork,
                                                                              int B, int T, int h, float scale, void* __restrict__ dqkv_) {
    constexpr int DK = 64;
    constexpr int NP = X3 ? 2 : 1;
    typedef typename vl_elt<X3>::type elt_t;
    const elt_t* __restrict__ qkv = reinterpret_cast<const elt_t*>(qkv_);
    const elt_t* __restrict__ dout = reinterpret_cast<const elt_t*>(dout_);
    elt_t* __restrict__ dqkv = reinterpret_cast<elt_t*>(dqkv_);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* const img0 = smem;               // Q [plane][256][VL_PITCH] bf16
    unsigned char* const img1 = smem + NP * VL_IMG;   // dO
    float* const lse2_l = reinterpret_cast<float*>(smem + 2 * NP * VL_IMG);   // lse * log2(e) and D of the staged queries
    float* const d_l = lse2_l + VL_ROWS;

    const int a = blockIdx.x, b = blockIdx.y;
    const int D = h * DK;
    const int64_t base = (int64_t)b * T;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = lane & 31, hf = lane >> 5;
    const int ntile = (T + 31) / 32;
    const int nchunk = (T + VL_ROWS - 1) / VL_ROWS;
    const int kt = 8 * (int)blockIdx.z + w;
    const bool active = kt < ntile;   // wave-uniform; an idle wave still stages and still reaches every barrier below
    const float c_exp = scale * VL_LOG2E;

    const int key = 32 * kt + j;
    const int k_ld = key < T ? key : T - 1;   // lanes past T (and idle waves) compute on the last key and store nothing
    bf16x8 kh[4], kl[X3 ? 4 : 1], vh[4], vl[X3 ? 4 : 1];
    vl_load_rows<X3>(qkv + (base + k_ld) * 3 * D + D + a * DK, kh, kl);
    vl_load_rows<X3>(qkv + (base + k_ld) * 3 * D + 2 * D + a * DK, vh, vl);

    f32x16 dk[2], dv[2];
    vl_zero2(dk);
    vl_zero2(dv);
#pragma unroll 1
    for (int qc = 0; qc < nchunk; ++qc) {
        if (qc) __syncthreads();   // every wave is done with the previous chunk
        vl_stage<X3>(img0, img1, qkv + a * DK, 3 * (int64_t)D, dout + a * DK, (int64_t)D, base, VL_ROWS * qc, T);
        if (threadIdx.x < VL_ROWS) {   // rows past T: finite values, so that their (zero) Q and dO rows give dS = 0 and add nothing
            const int row = VL_ROWS * qc + threadIdx.x;
            const int64_t at = ((int64_t)b * h + a) * T + row;
            lse2_l[threadIdx.x] = row < T ? lse[at] * VL_LOG2E : 0.f;
            d_l[threadIdx.x] = row < T ? dwork[at] : 0.f;
        }
        __syncthreads();
        if (active) {
            const int nq = ntile - 8 * qc < 8 ? ntile - 8 * qc : 8;
#pragma unroll 1
            for (int qt = 0; qt < nq; ++qt) {
                // P of query tile qt of the chunk: lane = key, register r = query 32 qt + (r & 3) + 8 (r >> 2) + 4 hf.  P is consumed by dV
                // before dP is formed, which keeps the live tiles at two
                f32x16 p, dp;
#pragma unroll
                for (int r = 0; r < 16; ++r) p[r] = 0.f, dp[r] = 0.f;
                static_for<0, 4>([&](auto ks) __attribute__((always_inline)) {
                    const bf16x8 ah = vl_row_frag(img0, 32 * qt, ks);
                    if constexpr (X3) {   // the same three terms in the same order as the dQ kernel: S is rebuilt, not approximated
                        const bf16x8 al = vl_row_frag(img0 + VL_IMG, 32 * qt, ks);
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
                vl_tr_product<X3>(img1, 32 * qt, p, dv);    // dV^T += dO^T P
                static_for<0, 4>([&](auto ks) __attribute__((always_inline)) {
                    const bf16x8 gh = vl_row_frag(img1, 32 * qt, ks);
                    if constexpr (X3) {
                        const bf16x8 gl = vl_row_frag(img1 + VL_IMG, 32 * qt, ks);
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
                vl_tr_product<X3>(img0, 32 * qt, dp, dk);   // dK^T += Q^T dS
            }
        }
    }
    if (active && key < T) {
        vl_store_rows<X3>(dqkv + (base + key) * 3 * D + D + a * DK, dk, scale);
        vl_store_rows<X3>(dqkv + (base + key) * 3 * D + 2 * D + a * DK, dv, 1.0f);
    }
}

template <bool X3>
int launch_vit_bwd_long(const void* qkv, const void* dout, const float* lse, int B, int T, int h, float scale, float* dwork, void* dqkv,
                        hipStream_t s) {
    constexpr size_t lds = vl_lds_bytes<X3>();
    static_assert(lds <= 160 * 1024, "vit_attention_bwd_long: LDS budget");
    auto dq = vit_attention_bwd_dq_kernel<X3>;
    auto dkv = vit_attention_bwd_dkv_kernel<X3>;
    static thread_local unsigned long long dq_mask = 0, dkv_mask = 0;   // devices (bit = device id) that have the opt-in
    if (int rc = snf::lds_opt_in(reinterpret_cast<const void*>(dq), lds, &dq_mask, "vit_attention_bwd_dq")) return rc;
    if (int rc = snf::lds_opt_in(reinterpret_cast<const void*>(dkv), lds, &dkv_mask, "vit_attention_bwd_dkv")) return rc;
    const dim3 grid(h, B, (T + VL_ROWS - 1) / VL_ROWS);
    hipLaunchKernelGGL(dq, grid, dim3(VL_THREADS), lds, s, qkv, dout, lse, B, T, h, scale, dwork, dqkv);
    if (int rc = snf::check_launch("vit_attention_bwd_dq_kernel")) return rc;
    hipLaunchKernelGGL(dkv, grid, dim3(VL_THREADS), lds, s, qkv, dout, lse, (const float*)dwork, B, T, h, scale, dqkv);
    return snf::check_launch("vit_attention_bwd_dkv_kernel");
}

}  // namespace

extern "C" {

int snf_vit_attention_bwd_long(const void* qkv, const void* dout, const float* lse, int dtype, int b, int t, int h, int dk, float scale,
                               float* dwork, void* dqkv, snf_stream_t stream) {
    SNF_REQUIRE(qkv && dout && lse && dwork && dqkv, "snf_vit_attention_bwd_long: null pointer");
    SNF_REQUIRE(dtype == SNF_DT_F32 || dtype == SNF_DT_BF16, "snf_vit_attention_bwd_long: dtype is f32 (fp32 class) or bf16 (got %d)", dtype);
    SNF_REQUIRE(b >= 1 && t >= 1 && h >= 1, "snf_vit_attention_bwd_long: bad shape");
    if (dk != 64 || t <= SNF_VIT_BWD_MAX_T || t > SNF_VIT_BWD_LONG_MAX_T || b > 65535) {
        snf::set_error("snf_vit_attention_bwd_long: unsupported shape dk=%d t=%d b=%d (need dk == 64, %d < t <= %d, b <= 65535; "
                       "t <= %d is served by snf_vit_attention_bwd)", dk, t, b, SNF_VIT_BWD_MAX_T, SNF_VIT_BWD_LONG_MAX_T, SNF_VIT_BWD_MAX_T);
        return SNF_EUNSUPPORTED;
    }
    if (((reinterpret_cast<uintptr_t>(qkv) | reinterpret_cast<uintptr_t>(dout) | reinterpret_cast<uintptr_t>(dqkv)) & 15) != 0 ||
        ((reinterpret_cast<uintptr_t>(lse) | reinterpret_cast<uintptr_t>(dwork)) & 3) != 0) {
        snf::set_error("snf_vit_attention_bwd_long: unsupported operands: qkv, dout and dqkv must be 16-byte aligned (16-byte vector loads and stores)");
        return SNF_EUNSUPPORTED;
    }
    hipStream_t s = snf::as_stream(stream);
    return dtype == SNF_DT_F32 ? launch_vit_bwd_long<true>(qkv, dout, lse, b, t, h, scale, dwork, dqkv, s)
                               : launch_vit_bwd_long<false>(qkv, dout, lse, b, t, h, scale, dwork, dqkv, s);
}

}  // extern "C"
