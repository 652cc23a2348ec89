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
// Backward (vit_attn32_bwd_kernel<NKB, X3>): vit_bwd_short of csrc/vit_attn_tile.h, the two phases of vit_attention_bwd_kernel, over
// the unpadded, XOR-rotated 64-byte-row layout (VitLayout32 there says why).  T == 1 is the copy kernel.
//
// Key-block counts built: 2, 4 and 8 (T <= 64, <= 128, <= 256).  NKB sizes the LDS images and the staging loops only; the loops
// over key blocks and query tiles run to ceil(T / 32), so T = 197 under NKB = 8 does 7 blocks of work.  A separate 6 would save
// 64 zero rows of staging and nothing else.
#include "vit_attn_tile.h"

namespace {

typedef VitLayout32 V32;
constexpr float V32_LN2 = 0.69314718055994530942f;

template <int NKB, bool X3>
constexpr size_t v32_fwd_lds_bytes() {
    return (size_t)2 * (X3 ? 2 : 1) * (32 * NKB * V32::ROWB);
}

// ---------------------------------------------------------------------------------------------------------------- forward
template <int NKB, bool X3>
__global__ __launch_bounds__(VT_THREADS, X3 ? 2 : 4) void vit_attn32_fwd_kernel(const void* __restrict__ qkv_, int B, int T, int h, float scale,
                                                                               void* __restrict__ out_, float* __restrict__ lse) {
    constexpr int DK = V32::DK;
    constexpr int NP = X3 ? 2 : 1;
    constexpr int ROWS = 32 * NKB;
    constexpr int IMG = ROWS * V32::ROWB;
    typedef vit_elt_t<X3> elt_t;
    const elt_t* __restrict__ qkv = reinterpret_cast<const elt_t*>(qkv_);
    elt_t* __restrict__ out = reinterpret_cast<elt_t*>(out_);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* const img_k = smem;              // [NP][ROWS][64 B]
    unsigned char* const img_v = smem + NP * IMG;   // [NP][ROWS][64 B]

    const int a = blockIdx.x, b = blockIdx.y;
    const int D = h * DK;
    const int64_t base = (int64_t)b * T;
    const VitLane<V32> ln;
    const int j = ln.j, hf = ln.hf;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ntile = (T + 31) / 32;
    const bool active = w < ntile;   // wave-uniform: this wave owns query tile w
    const float c_exp = scale * VT_LOG2E;

    // this wave's queries are requested before the staging: B operand of S^T = K Q^T, lane = query (clamped past T)
    const int q_row = 32 * w + j;
    VitRows<V32, X3> q;
    if (active) load_rows<V32, X3>(ln, qkv + (base + (q_row < T ? q_row : T - 1)) * 3 * D + a * DK, q);
    stage<V32, ROWS, X3>(img_k, img_v, qkv + D + a * DK, 3 * (int64_t)D, qkv + 2 * D + a * DK, 3 * (int64_t)D, base, 0, T);
    __syncthreads();
    if (!active) return;   // no barrier follows

    f32x16 o_acc[V32::NB];   // one 32 x 32 block
#pragma unroll
    for (int r = 0; r < 16; ++r) o_acc[0][r] = 0.f;
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
        static_for<0, V32::KS>([&](auto ks) __attribute__((always_inline)) {
            const bf16x8 kh = ln.row_frag(img_k, 32 * jb, ks);
            if constexpr (X3) {
                const bf16x8 kl = ln.row_frag(img_k + IMG, 32 * jb, ks);
                s_acc = mfma(kh, q.lo[ks], s_acc);
                s_acc = mfma(kl, q.hi[ks], s_acc);
            }
            s_acc = mfma(kh, q.hi[ks], s_acc);
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
        for (int r = 0; r < 16; ++r) o_acc[0][r] *= alpha;
        tr_product<V32, IMG, X3>(ln, img_v, 32 * jb, s_acc, o_acc);   // O^T += V^T P^T
    }
    const float l = xhalf_sum(l_lane);
    if (q_row < T) {
        // the row statistic the backward rebuilds P from: log sum_j exp(scale s_j) = scale max + log l
        if (hf == 0) lse[((int64_t)b * h + a) * T + q_row] = fmaf(m_run, scale, __builtin_amdgcn_logf(l) * V32_LN2);
        store_rows<V32, X3>(ln, out + (base + q_row) * D + a * DK, o_acc, __builtin_amdgcn_rcpf(l));
    }
}

// ---------------------------------------------------------------------------------------------------------------- backward
template <int NKB, bool X3>
__global__ __launch_bounds__(VT_THREADS, 1) void vit_attn32_bwd_kernel(const void* __restrict__ qkv, const void* __restrict__ dout,
                                                                      const float* __restrict__ lse, int B, int T, int h, float scale,
                                                                      void* __restrict__ dqkv) {
    vit_bwd_short<V32, NKB, X3>(qkv, dout, lse, T, h, scale, dqkv);
}

VIT_BWD_T1_KERNEL(vit_attn32_bwd_t1_kernel)

template <int NKB, bool X3>
int launch_v32_fwd(const void* qkv, int B, int T, int h, float scale, void* out, float* lse, hipStream_t s) {
    constexpr size_t lds = v32_fwd_lds_bytes<NKB, X3>();
    static_assert(lds <= 160 * 1024, "vit_attn32_fwd: LDS budget");
    auto kern = vit_attn32_fwd_kernel<NKB, X3>;
    static thread_local unsigned long long attr_set_mask = 0;   // devices (bit = device id) that have the opt-in
    if (lds > 48 * 1024)
        if (int rc = snf::lds_opt_in(reinterpret_cast<const void*>(kern), lds, &attr_set_mask, "vit_attn32_fwd")) return rc;
    hipLaunchKernelGGL(kern, dim3(h, B), dim3(VT_THREADS), lds, s, qkv, B, T, h, scale, out, lse);
    return snf::check_launch("vit_attn32_fwd_kernel");
}

template <int NKB, bool X3>
int launch_v32_bwd(const void* qkv, const void* dout, const float* lse, int B, int T, int h, float scale, void* dqkv, hipStream_t s) {
    constexpr size_t lds = vit_bwd_lds_bytes<V32, NKB>(X3);
    static_assert(lds <= 160 * 1024, "vit_attn32_bwd: LDS budget");
    auto kern = vit_attn32_bwd_kernel<NKB, X3>;
    static thread_local unsigned long long attr_set_mask = 0;
    if (lds > 48 * 1024)
        if (int rc = snf::lds_opt_in(reinterpret_cast<const void*>(kern), lds, &attr_set_mask, "vit_attn32_bwd")) return rc;
    hipLaunchKernelGGL(kern, dim3(h, B), dim3(VT_THREADS), lds, s, qkv, dout, lse, B, T, h, scale, dqkv);
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

}  // namespace

extern "C" {

int snf_vit_attention_dk32_fwd_lse(const void* qkv, int dtype, int b, int t, int h, int dk, float scale, void* out, float* lse,
                                   snf_stream_t stream) {
    if (int rc = vit_check_args("snf_vit_attention_dk32_fwd_lse", {qkv, out}, "qkv and out", {lse}, dtype, b, t, h, dk, V32::DK, 0,
                                SNF_VIT_DK32_MAX_T))
        return rc;
    hipStream_t s = snf::as_stream(stream);
    return dtype == SNF_DT_F32 ? dispatch_v32_fwd<true>(qkv, b, t, h, scale, out, lse, s) : dispatch_v32_fwd<false>(qkv, b, t, h, scale, out, lse, s);
}

int snf_vit_attention_dk32_bwd(const void* qkv, const void* dout, const float* lse, int dtype, int b, int t, int h, int dk, float scale,
                               void* dqkv, snf_stream_t stream) {
    if (int rc = vit_check_args("snf_vit_attention_dk32_bwd", {qkv, dout, dqkv}, "qkv, dout and dqkv", {lse}, dtype, b, t, h, dk, V32::DK, 0,
                                SNF_VIT_DK32_MAX_T))
        return rc;
    hipStream_t s = snf::as_stream(stream);
    const bool x3 = dtype == SNF_DT_F32;
    if (t == 1)
        return vit_launch_bwd_t1(vit_attn32_bwd_t1_kernel<float>, vit_attn32_bwd_t1_kernel<unsigned short>, "vit_attn32_bwd_t1_kernel", x3, dout,
                                 b, h, dk, dqkv, s);
    return x3 ? dispatch_v32_bwd<true>(qkv, dout, lse, b, t, h, scale, dqkv, s) : dispatch_v32_bwd<false>(qkv, dout, lse, b, t, h, scale, dqkv, s);
}

}  // extern "C"
