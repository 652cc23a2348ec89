// Backward of the ViT self-attention of csrc/vit.hip on the matrix cores (gfx950), dk = 64, T <= 256.
//
//   snf_vit_attention_bwd   qkv [B*T, 3*h*64] (q | k | v), dout [B*T, h*64], lse [B, h, T] (natural log, what
//                           snf_vit_attention_fwd_lse wrote) -> dqkv [B*T, 3*h*64] (dQ | dK | dV), fully written.
//
//   SNF_DT_F32  : fp32 tensors, the fp32-class arithmetic of the forward: every operand is hi + lo (hi = bf16(x),
//                 lo = bf16(x - hi)), every product hi hi + hi lo + lo hi on v_mfma_f32_32x32x16_bf16, fp32 accumulation;
//                 P and dS are split in registers.
//   SNF_DT_BF16 : bf16 tensors, P and dS rounded to bf16 as operands, fp32 accumulation, dqkv stored as bf16.
//
// One workgroup per (image, head), 8 waves, two phases over the same LDS.  Nothing is reduced across waves and there are no
// atomics: every output element has one owner and one summation order, so two runs give the same bits.
//
//   phase A  K and V staged row-major (one or two bf16 planes).  Wave w owns query tile w (32 queries, one per lane pair):
//              S^T = K Q^T, P = exp(scale S - lse);  dP^T = V dO^T;  D_i = sum_j P_ij dP_ij  (first pass over the key blocks)
//              dS^T = P o (dP - D);  dQ^T += K^T dS^T (second pass: K^T by transpose read, dS^T straight from the C layout)
//            D and lse go to two small fp32 arrays in LDS.
//   phase B  wave w keeps the K and V fragments of key tile w in registers; Q and dO are staged over the images of K and V.
//            For every query tile:  S = Q K^T (queries in registers, keys on lanes), P, dP = dO V^T, dS as above,
//              dV^T += dO^T P,  dK^T += Q^T dS  (A operands by transpose read, P / dS straight from the C layout).
//
// S is computed three times (twice in phase A): the price of keeping no T x T state and needing no cross-wave reduction.
// T == 1 has a closed form (softmax over one key is the constant 1: dQ = dK = 0, dV = dO) and is served by a copy kernel, which
// makes that form exact in both arithmetics.
#include "mfma.h"

namespace {

typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;

constexpr int VB_THREADS = 512;   // 8 waves: T <= 256 is at most 8 tiles of 32
constexpr int VB_PITCH = 64 + 8;  // bf16 elements per LDS row: 144-byte rows, conflict-free 16-byte fragment reads
constexpr float VB_LOG2E = 1.44269504088896340736f;

template <int NKB, bool X3>
constexpr size_t vb_lds_bytes() {
    return (size_t)2 * (X3 ? 2 : 1) * (32 * NKB * VB_PITCH * 2) + (size_t)2 * 32 * NKB * sizeof(float);
}

template <int NKB, bool X3>
__global__ __launch_bounds__(VB_THREADS, 1) void vit_attention_bwd_kernel(const void* __restrict__ qkv_, const void* __restrict__ dout_,
                                                                          const float* __restrict__ lse, int B, int T, int h, float scale,
                                                                          void* __restrict__ dqkv_) {
    constexpr int DK = 64;
    constexpr int NP = X3 ? 2 : 1;            // operand planes (hi, lo)
    constexpr int ROWS = 32 * NKB;
    constexpr int IMG = ROWS * VB_PITCH * 2;  // bytes of one plane of one staged matrix
    typedef typename std::conditional<X3, float, unsigned short>::type elt_t;
    const elt_t* __restrict__ qkv = reinterpret_cast<const elt_t*>(qkv_);
    const elt_t* __restrict__ dout = reinterpret_cast<const elt_t*>(dout_);
    elt_t* __restrict__ dqkv = reinterpret_cast<elt_t*>(dqkv_);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // images [matrix 0 / 1][plane][ROWS][VB_PITCH] bf16 (phase A: K, V; phase B: Q, dO), then lse * log2(e) and D per query
    unsigned char* const img0 = smem;
    unsigned char* const img1 = smem + NP * IMG;
    float* const lse2_l = reinterpret_cast<float*>(smem + 2 * NP * IMG);
    float* const d_l = lse2_l + ROWS;

    const int a = blockIdx.x, b = blockIdx.y;
    const int D = h * DK;
    const int64_t base = (int64_t)b * T;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = lane & 31, hf = lane >> 5;
    const int ntile = (T + 31) / 32;
    const bool active = w < ntile;   // wave-uniform: this wave owns query tile w (phase A) and key tile w (phase B)
    const float c_exp = scale * VB_LOG2E;

    // rows 0 .. ROWS-1 of two [T, 64] matrices (row strides ld0, ld1 elements) into the two images; rows >= T are zero.  Every
    // global load of the thread is issued before its first LDS store.
    constexpr int NI = (ROWS * 8 + VB_THREADS - 1) / VB_THREADS;
    auto stage = [&](const elt_t* __restrict__ p0, int64_t ld0, const elt_t* __restrict__ p1, int64_t ld1) __attribute__((always_inline)) {
        if constexpr (X3) {
            f32x8 s0[NI], s1[NI];
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                const int c = threadIdx.x + VB_THREADS * i;
                const int row = c >> 3, part = c & 7;
                s0[i] = f32x8{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                s1[i] = s0[i];
                if (row < T && row < ROWS) {
                    s0[i] = load8(p0 + (base + row) * ld0 + part * 8);
                    s1[i] = load8(p1 + (base + row) * ld1 + part * 8);
                }
            }
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                const int c = threadIdx.x + VB_THREADS * i;
                const int row = c >> 3, part = c & 7;
                if (row < ROWS) {
                    u32x4 h0, l0, h1, l1;
                    split8(s0[i], h0, l0);
                    split8(s1[i], h1, l1);
                    const int off = (row * VB_PITCH + part * 8) * 2;
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
                const int c = threadIdx.x + VB_THREADS * i;
                const int row = c >> 3, part = c & 7;
                s0[i] = u32x4{0u, 0u, 0u, 0u};
                s1[i] = s0[i];
                if (row < T && row < ROWS) {
                    s0[i] = *reinterpret_cast<const u32x4*>(p0 + (base + row) * ld0 + part * 8);
                    s1[i] = *reinterpret_cast<const u32x4*>(p1 + (base + row) * ld1 + part * 8);
                }
            }
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                const int c = threadIdx.x + VB_THREADS * i;
                const int row = c >> 3, part = c & 7;
                if (row < ROWS) {
                    const int off = (row * VB_PITCH + part * 8) * 2;
                    *reinterpret_cast<u32x4*>(img0 + off) = s0[i];
                    *reinterpret_cast<u32x4*>(img1 + off) = s1[i];
                }
            }
        }
    };
    // row fragment (A or B operand with the image's row on the lane): row r0 + j, columns 16 ks + 8 hf .. + 7
    auto row_frag = [&](const unsigned char* img, int r0, int ks) __attribute__((always_inline)) -> bf16x8 {
        return __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(img + ((r0 + j) * VB_PITCH + 16 * ks + 8 * hf) * 2));
    };
    // transposed fragment (A operand with the image's COLUMN 32 db + j on the lane): rows r0 + 4 hf + {0..3} and the same + 8 in
    // the registers -- the order in which a C tile holds its rows, so P^T / dS^T feed the next product without lane movement
    const int tg = lane >> 4, ti = lane & 15;
    const int tr_off = ((4 * (tg >> 1) + (ti >> 2)) * VB_PITCH) * 2 + 32 * (tg & 1) + 8 * (ti & 3);
    auto col_frag = [&](const unsigned char* img, int r0, int db) __attribute__((always_inline)) -> bf16x8 {
        const unsigned char* p = img + r0 * (VB_PITCH * 2) + 64 * db + tr_off;
        return tr_frag(p, p + 8 * VB_PITCH * 2);
    };
    // a row of a [T, 64] matrix in HBM as a B operand (lane = row), split when X3
    auto load_rows = [&](const elt_t* __restrict__ p, bf16x8 (&hi)[4], bf16x8 (&lo)[X3 ? 4 : 1]) __attribute__((always_inline)) {
        static_for<0, 4>([&](auto ks) __attribute__((always_inline)) {
            if constexpr (X3)
                split8(load8(p + 16 * ks + 8 * hf), hi[ks], lo[ks]);
            else
                hi[ks] = load_frag(p + 16 * ks + 8 * hf);
        });
    };
    // acc[db] += (columns 32 db .. of image rows r0 + 16 u ..)^T x (registers 8 u .. 8 u + 7 of x), db = 0, 1, u = 0, 1
    auto tr_product = [&](const unsigned char* img, int r0, const f32x16& x, f32x16 (&acc)[2]) __attribute__((always_inline)) {
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
                    const bf16x8 ah = col_frag(img, r0 + 16 * u, db), al = col_frag(img + IMG, r0 + 16 * u, db);
                    acc[db] = mfma(ah, xl, acc[db]);
                    acc[db] = mfma(al, xh, acc[db]);
                    acc[db] = mfma(ah, xh, acc[db]);
                });
            } else {
                const bf16x8 xb = __builtin_convertvector(xv, bf16x8);
                static_for<0, 2>([&](auto db_t) __attribute__((always_inline)) {
                    constexpr int db = decltype(db_t)::value;
                    acc[db] = mfma(col_frag(img, r0 + 16 * u, db), xb, acc[db]);
                });
            }
        });
    };
    // store a transposed 64 x 32 result (lane = row of the output matrix, 4 consecutive columns per register group) times f
    auto store_rows = [&](elt_t* __restrict__ p, const f32x16 (&acc)[2], float f) __attribute__((always_inline)) {
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
    };
    auto zero2 = [&](f32x16 (&acc)[2]) __attribute__((always_inline)) {
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[0][r] = 0.f, acc[1][r] = 0.f;
    };

    // ------------------------------------------------------------ phase A: D and dQ of query tile w
    stage(qkv + D + a * DK, 3 * (int64_t)D, qkv + 2 * D + a * DK, 3 * (int64_t)D);
    __syncthreads();
    if (active) {
        const int q_row = 32 * w + j;
        const int q_ld = q_row < T ? q_row : T - 1;   // lanes past T recompute the last row and store nothing
        bf16x8 qh[4], ql[X3 ? 4 : 1], gh[4], gl[X3 ? 4 : 1];
        load_rows(qkv + (base + q_ld) * 3 * D + a * DK, qh, ql);
        load_rows(dout + (base + q_ld) * D + a * DK, gh, gl);
        const float lse2 = lse[((int64_t)b * h + a) * T + q_ld] * VB_LOG2E;
        // P^T and dP^T of key block jb: lane = query, register r = key 32 jb + (r & 3) + 8 (r >> 2) + 4 hf
        auto p_dp = [&](int jb, f32x16& p, f32x16& dp) __attribute__((always_inline)) {
#pragma unroll
            for (int r = 0; r < 16; ++r) p[r] = 0.f, dp[r] = 0.f;
            static_for<0, 4>([&](auto ks) __attribute__((always_inline)) {
                const bf16x8 kh = row_frag(img0, 32 * jb, ks), vh = row_frag(img1, 32 * jb, ks);
                if constexpr (X3) {
                    const bf16x8 kl = row_frag(img0 + IMG, 32 * jb, ks), vl = row_frag(img1 + IMG, 32 * jb, ks);
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
        f32x16 dq[2];
        zero2(dq);
#pragma unroll 1
        for (int jb = 0; jb < ntile; ++jb) {
            f32x16 p, dp;
            p_dp(jb, p, dp);
#pragma unroll
            for (int r = 0; r < 16; ++r) p[r] *= dp[r] - d_row;
            tr_product(img0, 32 * jb, p, dq);   // dQ^T += K^T dS^T
        }
        if (q_row < T) store_rows(dqkv + (base + q_row) * 3 * D + a * DK, dq, scale);
        if (hf == 0) {   // rows past T: finite values, so that their (zero) Q and dO rows give dS = 0 and add nothing in phase B
            lse2_l[q_row] = q_row < T ? lse2 : 0.f;
            d_l[q_row] = q_row < T ? d_row : 0.f;
        }
    }

    // ------------------------------------------------------------ phase B: dK and dV of key tile w
    bf16x8 kh[4], kl[X3 ? 4 : 1], vh[4], vl[X3 ? 4 : 1];
    if (active) {
        static_for<0, 4>([&](auto ks) __attribute__((always_inline)) {
            kh[ks] = row_frag(img0, 32 * w, ks);
            vh[ks] = row_frag(img1, 32 * w, ks);
            if constexpr (X3) {
                kl[ks] = row_frag(img0 + IMG, 32 * w, ks);
                vl[ks] = row_frag(img1 + IMG, 32 * w, ks);
            }
        });
    }
    __syncthreads();   // every wave is done with the images of K and V
    stage(qkv + a * DK, 3 * (int64_t)D, dout + a * DK, (int64_t)D);
    __syncthreads();
    if (active) {
        f32x16 dk[2], dv[2];
        zero2(dk);
        zero2(dv);
#pragma unroll 1
        for (int qt = 0; qt < ntile; ++qt) {
            // P of query tile qt: lane = key, register r = query 32 qt + (r & 3) + 8 (r >> 2) + 4 hf.  P is consumed by dV before
            // dP is formed, which keeps the live tiles at two
            f32x16 p, dp;
#pragma unroll
            for (int r = 0; r < 16; ++r) p[r] = 0.f, dp[r] = 0.f;
            static_for<0, 4>([&](auto ks) __attribute__((always_inline)) {
                const bf16x8 ah = row_frag(img0, 32 * qt, ks);
                if constexpr (X3) {   // the same three terms in the same order as phase A: S is rebuilt, not approximated
                    const bf16x8 al = row_frag(img0 + IMG, 32 * qt, ks);
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
            tr_product(img1, 32 * qt, p, dv);    // dV^T += dO^T P
            static_for<0, 4>([&](auto ks) __attribute__((always_inline)) {
                const bf16x8 gh = row_frag(img1, 32 * qt, ks);
                if constexpr (X3) {
                    const bf16x8 gl = row_frag(img1 + IMG, 32 * qt, ks);
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
            tr_product(img0, 32 * qt, dp, dk);   // dK^T += Q^T dS
        }
        const int key = 32 * w + j;
        if (key < T) {
            store_rows(dqkv + (base + key) * 3 * D + D + a * DK, dk, scale);
            store_rows(dqkv + (base + key) * 3 * D + 2 * D + a * DK, dv, 1.0f);
        }
    }
}

// T == 1: dqkv row = (0 | 0 | dout row)
template <typename elt_t>
__global__ __launch_bounds__(256) void vit_attention_bwd_t1_kernel(const elt_t* __restrict__ dout, int64_t total, int D, elt_t* __restrict__ dqkv) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = i / (3 * D);
        const int col = (int)(i - row * 3 * D);
        dqkv[i] = col >= 2 * D ? dout[row * D + col - 2 * D] : elt_t(0);
    }
}

template <int NKB, bool X3>
int launch_vit_bwd(const void* qkv, const void* dout, const float* lse, int B, int T, int h, float scale, void* dqkv, hipStream_t s) {
    constexpr size_t lds = vb_lds_bytes<NKB, X3>();
    static_assert(lds <= 160 * 1024, "vit_attention_bwd: LDS budget");
    auto kern = vit_attention_bwd_kernel<NKB, X3>;
    static thread_local unsigned long long attr_set_mask = 0;   // devices (bit = device id) that have the opt-in
    if (lds > 48 * 1024)
        if (int rc = snf::lds_opt_in(reinterpret_cast<const void*>(kern), lds, &attr_set_mask, "vit_attention_bwd")) return rc;
    hipLaunchKernelGGL(kern, dim3(h, B), dim3(VB_THREADS), lds, s, qkv, dout, lse, B, T, h, scale, dqkv);
    return snf::check_launch("vit_attention_bwd_kernel");
}

template <bool X3>
int dispatch_vit_bwd(const void* qkv, const void* dout, const float* lse, int B, int T, int h, float scale, void* dqkv, hipStream_t s) {
    const int nkb = (T + 31) / 32;
    if (nkb <= 2) return launch_vit_bwd<2, X3>(qkv, dout, lse, B, T, h, scale, dqkv, s);
    if (nkb <= 4) return launch_vit_bwd<4, X3>(qkv, dout, lse, B, T, h, scale, dqkv, s);
    if (nkb <= 6) return launch_vit_bwd<6, X3>(qkv, dout, lse, B, T, h, scale, dqkv, s);
    return launch_vit_bwd<8, X3>(qkv, dout, lse, B, T, h, scale, dqkv, s);
}

}  // namespace

extern "C" {

int snf_vit_attention_bwd(const void* qkv, const void* dout, const float* lse, int dtype, int b, int t, int h, int dk, float scale,
                          void* dqkv, snf_stream_t stream) {
    SNF_REQUIRE(qkv && dout && lse && dqkv, "snf_vit_attention_bwd: null pointer");
    SNF_REQUIRE(dtype == SNF_DT_F32 || dtype == SNF_DT_BF16, "snf_vit_attention_bwd: dtype is f32 (fp32 class) or bf16 (got %d)", dtype);
    SNF_REQUIRE(b >= 1 && t >= 1 && h >= 1, "snf_vit_attention_bwd: bad shape");
    if (dk != 64 || t > SNF_VIT_BWD_MAX_T || b > 65535) {
        snf::set_error("snf_vit_attention_bwd: unsupported shape dk=%d t=%d b=%d (need dk == 64, t <= %d, b <= 65535)", dk, t, b,
                       SNF_VIT_BWD_MAX_T);
        return SNF_EUNSUPPORTED;
    }
    if (((reinterpret_cast<uintptr_t>(qkv) | reinterpret_cast<uintptr_t>(dout) | reinterpret_cast<uintptr_t>(dqkv)) & 15) != 0 ||
        (reinterpret_cast<uintptr_t>(lse) & 3) != 0) {
        snf::set_error("snf_vit_attention_bwd: unsupported operands: qkv, dout and dqkv must be 16-byte aligned (16-byte vector loads and stores)");
        return SNF_EUNSUPPORTED;
    }
    hipStream_t s = snf::as_stream(stream);
    const bool x3 = dtype == SNF_DT_F32;
    if (t == 1) {
        const int64_t total = (int64_t)b * 3 * h * dk;
        const int grid = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
        if (x3)
            hipLaunchKernelGGL(vit_attention_bwd_t1_kernel<float>, dim3(grid), dim3(256), 0, s, reinterpret_cast<const float*>(dout), total,
                               h * dk, reinterpret_cast<float*>(dqkv));
        else
            hipLaunchKernelGGL(vit_attention_bwd_t1_kernel<unsigned short>, dim3(grid), dim3(256), 0, s,
                               reinterpret_cast<const unsigned short*>(dout), total, h * dk, reinterpret_cast<unsigned short*>(dqkv));
        return snf::check_launch("vit_attention_bwd_t1_kernel");
    }
    return x3 ? dispatch_vit_bwd<true>(qkv, dout, lse, b, t, h, scale, dqkv, s) : dispatch_vit_bwd<false>(qkv, dout, lse, b, t, h, scale, dqkv, s);
}

}  // extern "C"
