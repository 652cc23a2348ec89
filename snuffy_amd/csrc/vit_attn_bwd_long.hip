// Backward of the ViT self-attention of csrc/vit.hip on the matrix cores (gfx950), dk = 64, 256 < T <= 4096: the two phases of
// csrc/vit_attn_bwd.hip as two launches on one stream, each a loop over 256-row chunks of the side it stages in LDS.
//
//   snf_vit_attention_bwd_long   qkv [B*T, 3*h*64] (q | k | v), dout [B*T, h*64], lse [B, h, T] (natural log, what
//                                snf_vit_attention_fwd_lse wrote), dwork [B, h, T] f32 (scratch) -> dqkv [B*T, 3*h*64], fully written.
//
// The arithmetics are those of vit_attn_bwd.hip (SNF_DT_F32: the fp32 class; SNF_DT_BF16: bf16 operands), and the tiles, their
// layout and what keeps them deterministic and exact past T are those of csrc/vit_attn_tile.h.
//
// Both kernels: grid (h, B, ceil(T / 256)), 8 waves.  Wave w of the workgroup at z = c owns tile 8 c + w (32 rows).
//
//   vit_attention_bwd_dq_kernel   the wave holds the Q and dO rows and lse of its query tile in registers; the workgroup walks the key
//                                 chunks (256 rows of K and V staged) twice:
//                                   first walk   D_i = sum_j P_ij dP_ij
//                                   second walk  dS^T = P o (dP - D), dQ^T += K^T dS^T
//                                 and stores dQ * scale and D (rows < T, [B, h, T] workspace in HBM).
//   vit_attention_bwd_dkv_kernel  the wave holds the K and V fragments of its key tile in registers (straight from HBM); the workgroup
//                                 walks the query chunks (256 rows of Q and dO staged, lse * log2 e and D of the chunk in two small LDS
//                                 arrays) and stores dK * scale and dV once.
//
// A wave whose tile is past T does no arithmetic and takes part in every staging loop and every barrier of the chunk walk.
#include "vit_attn_tile.h"

namespace {

typedef VitLayout64 VL;
constexpr int VL_ROWS = 256;                 // rows of one staged chunk: 8 tiles of 32
constexpr int VL_IMG = VL_ROWS * VL::ROWB;   // bytes of one plane of one staged matrix

template <bool X3>
constexpr size_t vl_lds_bytes() {
    return (size_t)2 * (X3 ? 2 : 1) * VL_IMG + (size_t)2 * VL_ROWS * sizeof(float);
}

// ------------------------------------------------------------------------------------------------ D and dQ of query tile 8 z + w
template <bool X3>
__global__ __launch_bounds__(VT_THREADS, 1) void vit_attention_bwd_dq_kernel(const void* __restrict__ qkv_, const void* __restrict__ dout_,
                                                                             const float* __restrict__ lse, int B, int T, int h, float scale,
                                                                             float* __restrict__ dwork, void* __restrict__ dqkv_) {
    constexpr int DK = VL::DK;
    constexpr int NP = X3 ? 2 : 1;   // operand planes (hi, lo)
    typedef vit_elt_t<X3> elt_t;
    const elt_t* __restrict__ qkv = reinterpret_cast<const elt_t*>(qkv_);
    const elt_t* __restrict__ dout = reinterpret_cast<const elt_t*>(dout_);
    elt_t* __restrict__ dqkv = reinterpret_cast<elt_t*>(dqkv_);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* const img0 = smem;                 // K [plane][256][144 B]
    unsigned char* const img1 = smem + NP * VL_IMG;   // V

    const int a = blockIdx.x, b = blockIdx.y;
    const int D = h * DK;
    const int64_t base = (int64_t)b * T;
    const VitLane<VL> ln;
    const int j = ln.j, hf = ln.hf;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ntile = (T + 31) / 32;
    const int nchunk = (T + VL_ROWS - 1) / VL_ROWS;
    const int qt = 8 * (int)blockIdx.z + w;
    const bool active = qt < ntile;   // wave-uniform; an idle wave still stages and still reaches every barrier below
    const float c_exp = scale * VT_LOG2E;

    const int q_row = 32 * qt + j;
    const int q_ld = q_row < T ? q_row : T - 1;   // lanes past T (and idle waves) recompute the last row and store nothing
    VitRows<VL, X3> q, g;
    load_rows<VL, X3>(ln, qkv + (base + q_ld) * 3 * D + a * DK, q);
    load_rows<VL, X3>(ln, dout + (base + q_ld) * D + a * DK, g);
    const float lse2 = lse[((int64_t)b * h + a) * T + q_ld] * VT_LOG2E;

    const VitQuerySide<VL, VL_IMG, X3> p_dp{ln, img0, img1, T, q, g, c_exp, lse2};

    // first walk: D
    float d_lane = 0.f;
#pragma unroll 1
    for (int kc = 0; kc < nchunk; ++kc) {
        if (kc) __syncthreads();   // every wave is done with the previous chunk
        stage<VL, VL_ROWS, X3>(img0, img1, qkv + D + a * DK, 3 * (int64_t)D, qkv + 2 * D + a * DK, 3 * (int64_t)D, base, VL_ROWS * kc, T);
        __syncthreads();
        if (active) {
            const int nb = ntile - 8 * kc < 8 ? ntile - 8 * kc : 8;
#pragma unroll 1
            for (int jb = 0; jb < nb; ++jb) {
                f32x16 p, dp;
                p_dp(32 * jb, VL_ROWS * kc, p, dp);
#pragma unroll
                for (int r = 0; r < 16; ++r) d_lane = fmaf(p[r], dp[r], d_lane);
            }
        }
    }
    const float d_row = xhalf_sum(d_lane);   // the two half-waves hold the two halves of the row's keys

    // second walk: dQ
    f32x16 dq[VL::NB] = {};
#pragma unroll 1
    for (int kc = 0; kc < nchunk; ++kc) {
        __syncthreads();
        stage<VL, VL_ROWS, X3>(img0, img1, qkv + D + a * DK, 3 * (int64_t)D, qkv + 2 * D + a * DK, 3 * (int64_t)D, base, VL_ROWS * kc, T);
        __syncthreads();
        if (active) {
            const int nb = ntile - 8 * kc < 8 ? ntile - 8 * kc : 8;
#pragma unroll 1
            for (int jb = 0; jb < nb; ++jb) {
                f32x16 p, dp;
                p_dp(32 * jb, VL_ROWS * kc, p, dp);
#pragma unroll
                for (int r = 0; r < 16; ++r) p[r] *= dp[r] - d_row;
                tr_product<VL, VL_IMG, X3>(ln, img0, 32 * jb, p, dq);   // dQ^T += K^T dS^T
            }
        }
    }
    if (active && q_row < T) {
        store_rows<VL, X3>(ln, dqkv + (base + q_row) * 3 * D + a * DK, dq, scale);
        if (hf == 0) dwork[((int64_t)b * h + a) * T + q_row] = d_row;
    }
}

// ------------------------------------------------------------------------------------------------ dK and dV of key tile 8 z + w
template <bool X3>
__global__ __launch_bounds__(VT_THREADS, 1) void vit_attention_bwd_dkv_kernel(const void* __restrict__ qkv_, const void* __restrict__ dout_,
                                                                              const float* __restrict__ lse, const float* __restrict__ dwork,
                                                                              int B, int T, int h, float scale, void* __restrict__ dqkv_) {
    constexpr int DK = VL::DK;
    constexpr int NP = X3 ? 2 : 1;
    typedef vit_elt_t<X3> elt_t;
    const elt_t* __restrict__ qkv = reinterpret_cast<const elt_t*>(qkv_);
    const elt_t* __restrict__ dout = reinterpret_cast<const elt_t*>(dout_);
    elt_t* __restrict__ dqkv = reinterpret_cast<elt_t*>(dqkv_);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* const img0 = smem;                 // Q [plane][256][144 B]
    unsigned char* const img1 = smem + NP * VL_IMG;   // dO
    float* const lse2_l = reinterpret_cast<float*>(smem + 2 * NP * VL_IMG);   // lse * log2(e) and D of the staged queries
    float* const d_l = lse2_l + VL_ROWS;

    const int a = blockIdx.x, b = blockIdx.y;
    const int D = h * DK;
    const int64_t base = (int64_t)b * T;
    const VitLane<VL> ln;
    const int j = ln.j;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ntile = (T + 31) / 32;
    const int nchunk = (T + VL_ROWS - 1) / VL_ROWS;
    const int kt = 8 * (int)blockIdx.z + w;
    const bool active = kt < ntile;   // wave-uniform; an idle wave still stages and still reaches every barrier below
    const float c_exp = scale * VT_LOG2E;

    const int key = 32 * kt + j;
    const int k_ld = key < T ? key : T - 1;   // lanes past T (and idle waves) compute on the last key and store nothing
    VitRows<VL, X3> k, v;
    load_rows<VL, X3>(ln, qkv + (base + k_ld) * 3 * D + D + a * DK, k);
    load_rows<VL, X3>(ln, qkv + (base + k_ld) * 3 * D + 2 * D + a * DK, v);

    const VitKeySide<VL, VL_IMG, X3> add_tile{ln, img0, img1, lse2_l, d_l, k, v, c_exp};
    f32x16 dk[VL::NB] = {}, dv[VL::NB] = {};
#pragma unroll 1
    for (int qc = 0; qc < nchunk; ++qc) {
        if (qc) __syncthreads();   // every wave is done with the previous chunk
        stage<VL, VL_ROWS, X3>(img0, img1, qkv + a * DK, 3 * (int64_t)D, dout + a * DK, (int64_t)D, base, VL_ROWS * qc, T);
        if (threadIdx.x < VL_ROWS) {   // rows past T: lse = D = 0
            const int row = VL_ROWS * qc + threadIdx.x;
            const int64_t at = ((int64_t)b * h + a) * T + row;
            lse2_l[threadIdx.x] = row < T ? lse[at] * VT_LOG2E : 0.f;
            d_l[threadIdx.x] = row < T ? dwork[at] : 0.f;
        }
        __syncthreads();
        if (active) {
            const int nq = ntile - 8 * qc < 8 ? ntile - 8 * qc : 8;
#pragma unroll 1
            for (int qt = 0; qt < nq; ++qt) add_tile(32 * qt, dk, dv);
        }
    }
    if (active && key < T) {
        store_rows<VL, X3>(ln, dqkv + (base + key) * 3 * D + D + a * DK, dk, scale);
        store_rows<VL, X3>(ln, dqkv + (base + key) * 3 * D + 2 * D + a * DK, dv, 1.0f);
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
    hipLaunchKernelGGL(dq, grid, dim3(VT_THREADS), lds, s, qkv, dout, lse, B, T, h, scale, dwork, dqkv);
    if (int rc = snf::check_launch("vit_attention_bwd_dq_kernel")) return rc;
    hipLaunchKernelGGL(dkv, grid, dim3(VT_THREADS), lds, s, qkv, dout, lse, (const float*)dwork, B, T, h, scale, dqkv);
    return snf::check_launch("vit_attention_bwd_dkv_kernel");
}

}  // namespace

extern "C" {

int snf_vit_attention_bwd_long(const void* qkv, const void* dout, const float* lse, int dtype, int b, int t, int h, int dk, float scale,
                               float* dwork, void* dqkv, snf_stream_t stream) {
    if (int rc = vit_check_args("snf_vit_attention_bwd_long", {qkv, dout, dqkv}, "qkv, dout and dqkv", {lse, dwork}, dtype, b, t, h, dk, 64,
                                SNF_VIT_BWD_MAX_T, SNF_VIT_BWD_LONG_MAX_T))
        return rc;
    hipStream_t s = snf::as_stream(stream);
    return dtype == SNF_DT_F32 ? launch_vit_bwd_long<true>(qkv, dout, lse, b, t, h, scale, dwork, dqkv, s)
                               : launch_vit_bwd_long<false>(qkv, dout, lse, b, t, h, scale, dwork, dqkv, s);
}

}  // extern "C"
