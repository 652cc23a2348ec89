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
// One workgroup per (image, head), 8 waves (T <= 256 is at most 8 tiles of 32), two phases over the same LDS: the kernel is
// vit_bwd_short of csrc/vit_attn_tile.h over the 144-byte-row layout, which also states what makes it deterministic and exact
// past T.  T == 1 has a closed form and is served by the copy kernel.
#include "vit_attn_tile.h"

namespace {

template <int NKB, bool X3>
__global__ __launch_bounds__(VT_THREADS, 1) void vit_attention_bwd_kernel(const void* __restrict__ qkv, const void* __restrict__ dout,
                                                                          const float* __restrict__ lse, int B, int T, int h, float scale,
                                                                          void* __restrict__ dqkv) {
    vit_bwd_short<VitLayout64, NKB, X3>(qkv, dout, lse, T, h, scale, dqkv);
}

VIT_BWD_T1_KERNEL(vit_attention_bwd_t1_kernel)

template <int NKB, bool X3>
int launch_vit_bwd(const void* qkv, const void* dout, const float* lse, int B, int T, int h, float scale, void* dqkv, hipStream_t s) {
    constexpr size_t lds = vit_bwd_lds_bytes<VitLayout64, NKB>(X3);
    static_assert(lds <= 160 * 1024, "vit_attention_bwd: LDS budget");
    auto kern = vit_attention_bwd_kernel<NKB, X3>;
    static thread_local unsigned long long attr_set_mask = 0;   // devices (bit = device id) that have the opt-in
    if (lds > 48 * 1024)
        if (int rc = snf::lds_opt_in(reinterpret_cast<const void*>(kern), lds, &attr_set_mask, "vit_attention_bwd")) return rc;
    hipLaunchKernelGGL(kern, dim3(h, B), dim3(VT_THREADS), lds, s, qkv, dout, lse, B, T, h, scale, dqkv);
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
    if (int rc = vit_check_args("snf_vit_attention_bwd", {qkv, dout, dqkv}, "qkv, dout and dqkv", {lse}, dtype, b, t, h, dk, 64, 0,
                                SNF_VIT_BWD_MAX_T))
        return rc;
    hipStream_t s = snf::as_stream(stream);
    const bool x3 = dtype == SNF_DT_F32;
    if (t == 1)
        return vit_launch_bwd_t1(vit_attention_bwd_t1_kernel<float>, vit_attention_bwd_t1_kernel<unsigned short>, "vit_attention_bwd_t1_kernel",
                                 x3, dout, b, h, dk, dqkv, s);
    return x3 ? dispatch_vit_bwd<true>(qkv, dout, lse, b, t, h, scale, dqkv, s) : dispatch_vit_bwd<false>(qkv, dout, lse, b, t, h, scale, dqkv, s);
}

}  // extern "C"
