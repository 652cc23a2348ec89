// Row passes of the frozen-trunk training route of adapter pre-training (snuffy_amd/ssl_pretrain.py, FUSED_TRUNK): the GELU between the
// two GEMMs of a frozen MLP, forward and backward, written straight as the operand image of the next fp32-class GEMM.
//
//   snf_gelu_image_f32      pre [m, n] f32 (row pitch ldp)              -> image of gelu(pre)
//   snf_gelu_bwd_image_f32  da [m, n] f32 (pitch ldda), pre (pitch ldp) -> image of da * gelu'(pre)
//
//   gelu(x)  = x Phi(x) = 0.5 x (1 + erf(x / sqrt 2))          (the erf form of nn.GELU)
//   gelu'(x) = Phi(x) + x phi(x),  phi(x) = exp(-x^2 / 2) / sqrt(2 pi)
//
// The image is one of the two a GEMM of csrc/gemm.hip reads (include/snuffy_hip.h, "fp32-class GEMMs"):
//   SNF_DT_BF16_HL      [m, 2 n], every 32 columns as [hi(32) | lo(32)]   (snf_split_hl_f32 writes the same of an fp32 tensor), n % 32 == 0
//   SNF_DT_BF16_SPLIT3  [m, 3 n] = [hi | hi | lo]                         (snf_split3_f32),                                     n % 8 == 0
// with hi = bf16(v), lo = bf16(v - hi), round to nearest even: the value v exists in registers only.
//
// Memory-bound: 4 (or 8) bytes read and 4 (or 6) written per element against one erff (and one expf).  A lane owns 4 consecutive
// columns: one 16-byte load per operand, so a wave's load instruction reads 1024 contiguous bytes, 8 full lines.  The lane's 4 hi and 4 lo
// values are 8 bytes each; the two lanes of a pair swap one half over DPP (quad_perm [1, 0, 3, 2], no LDS), after which the even lane
// holds the pair's 8 hi values and the odd lane its 8 lo values: 16-byte stores.  hl: the 8 lanes over a 32-column group write its
// 64 hi bytes and its 64 lo bytes, which are one 128-byte line of the image, in one instruction; a wave writes 8 such lines.  cat: one
// instruction writes 512 contiguous bytes of plane 0 (even lanes) and 512 of plane 2 (odd lanes), a second the even lanes' 512 of plane 1.
// The file is built with -ffp-contract=off: both images come from one sequence of individually rounded operations.
#include "common.h"

namespace {

constexpr float VT_SQRT1_2 = 0.70710678118654752440f;
constexpr float VT_INV_SQRT_2PI = 0.39894228040143267794f;

__device__ __forceinline__ float gelu_value(float x) { return 0.5f * x * (1.f + erff(x * VT_SQRT1_2)); }

__device__ __forceinline__ float gelu_slope(float x) {
    const float cdf = 0.5f * (1.f + erff(x * VT_SQRT1_2));
    const float pdf = expf(-0.5f * x * x) * VT_INV_SQRT_2PI;
    return cdf + x * pdf;
}

// the other lane of the pair (lane ^ 1)
__device__ __forceinline__ unsigned pair_swap(unsigned v) {
    return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, true);
}

// total = m * nq items of 4 columns, nq = n / 4 (even: a pair of lanes never straddles two rows, and total is even, so a pair is live
// or idle as one).  Every lane runs every trip of the loop (the swap needs its partner); only the stores are predicated.
template <bool HL, bool BWD>
__global__ __launch_bounds__(256) void gelu_image_kernel(const float* __restrict__ da, int64_t ldda, const float* __restrict__ pre,
                                                         int64_t ldp, unsigned total, unsigned nq, int n, unsigned short* __restrict__ out) {
    const unsigned step = gridDim.x * 256u;
    const bool odd = threadIdx.x & 1;
    for (unsigned base = blockIdx.x * 256u; base < total; base += step) {
        const unsigned i = base + threadIdx.x;
        const bool live = i < total;
        const unsigned item = live ? i : 0u;
        const unsigned row = item / nq;
        const int c = (int)(item - row * nq) * 4;
        const float4 p = *reinterpret_cast<const float4*>(pre + (int64_t)row * ldp + c);
        float v[4];
        if (BWD) {
            const float4 g = *reinterpret_cast<const float4*>(da + (int64_t)row * ldda + c);
            v[0] = g.x * gelu_slope(p.x);
            v[1] = g.y * gelu_slope(p.y);
            v[2] = g.z * gelu_slope(p.z);
            v[3] = g.w * gelu_slope(p.w);
        } else {
            v[0] = gelu_value(p.x);
            v[1] = gelu_value(p.y);
            v[2] = gelu_value(p.z);
            v[3] = gelu_value(p.w);
        }
        unsigned hi[2], lo[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            hi[e] = pack_bf16x2(v[2 * e], v[2 * e + 1]);
            lo[e] = pack_bf16x2(v[2 * e] - __uint_as_float(hi[e] << 16), v[2 * e + 1] - __uint_as_float(hi[e] & 0xffff0000u));
        }
        // the even lane gives its lo half away and takes the odd lane's hi half; the odd lane the other way round
        const unsigned r0 = pair_swap(odd ? hi[0] : lo[0]);
        const unsigned r1 = pair_swap(odd ? hi[1] : lo[1]);
        const uint4 st = odd ? make_uint4(r0, r1, lo[0], lo[1]) : make_uint4(hi[0], hi[1], r0, r1);
        const int pc = c & ~7;                               // first column of the pair
        if (!live) continue;
        if (HL) {
            unsigned short* o = out + (int64_t)row * 2 * n + 64 * (pc >> 5) + (pc & 31) + (odd ? 32 : 0);
            *reinterpret_cast<uint4*>(o) = st;
        } else {
            // one store by every lane (hi into plane 0, lo into plane 2), then the even lanes' second copy of hi into plane 1
            unsigned short* o = out + (int64_t)row * 3 * n + pc;
            *reinterpret_cast<uint4*>(o + (odd ? 2 * n : 0)) = st;
            if (!odd) *reinterpret_cast<uint4*>(o + n) = st;
        }
    }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <bool BWD>
int launch_gelu_image(const char* who, const float* da, int64_t ldda, const float* pre, int64_t ldp, int64_t m, int n, void* out_img,
                      int out_dtype, snf_stream_t stream) {
    SNF_REQUIRE(pre && out_img && (!BWD || da), "%s: null pointer", who);
    SNF_REQUIRE(out_dtype == SNF_DT_BF16_HL || out_dtype == SNF_DT_BF16_SPLIT3, "%s: out_dtype %d is neither the hl nor the split3 image", who,
                out_dtype);
    const int granule = out_dtype == SNF_DT_BF16_HL ? 32 : 8;
    SNF_REQUIRE(m >= 1 && n >= granule && n % granule == 0, "%s: bad shape m=%lld n=%d (n %% %d == 0)", who, (long long)m, n, granule);
    SNF_REQUIRE(ldp >= n && ldp % 4 == 0 && (!BWD || (ldda >= n && ldda % 4 == 0)), "%s: row pitches must cover n and be multiples of 4", who);
    SNF_REQUIRE(aligned16(pre) && aligned16(out_img) && (!BWD || aligned16(da)), "%s: buffers must be 16-byte aligned", who);
    const int64_t total = m * (int64_t)(n >> 2);
    SNF_REQUIRE(total < ((int64_t)1 << 31), "%s: m * n = %lld elements, at most 2^33 - 1", who, (long long)(m * (int64_t)n));
    int64_t blocks = (total + 255) / 256;
    const int64_t cap = (int64_t)snf::cu_count() * 8;
    if (blocks > cap) blocks = cap;
    unsigned short* o = reinterpret_cast<unsigned short*>(out_img);
    hipStream_t s = snf::as_stream(stream);
    if (out_dtype == SNF_DT_BF16_HL)
        hipLaunchKernelGGL((gelu_image_kernel<true, BWD>), dim3((int)blocks), dim3(256), 0, s, da, ldda, pre, ldp, (unsigned)total,
                           (unsigned)(n >> 2), n, o);
    else
        hipLaunchKernelGGL((gelu_image_kernel<false, BWD>), dim3((int)blocks), dim3(256), 0, s, da, ldda, pre, ldp, (unsigned)total,
                           (unsigned)(n >> 2), n, o);
    return snf::check_launch(BWD ? "gelu_image_kernel<bwd>" : "gelu_image_kernel<fwd>");
}

}  // namespace

int snf_gelu_image_f32(const float* pre, int64_t ldp, int64_t m, int n, void* out_img, int out_dtype, snf_stream_t stream) {
    return launch_gelu_image<false>("snf_gelu_image_f32", nullptr, 0, pre, ldp, m, n, out_img, out_dtype, stream);
}

int snf_gelu_bwd_image_f32(const float* da, int64_t ldda, const float* pre, int64_t ldp, int64_t m, int n, void* out_img, int out_dtype,
                           snf_stream_t stream) {
    return launch_gelu_image<true>("snf_gelu_bwd_image_f32", da, ldda, pre, ldp, m, n, out_img, out_dtype, stream);
}
