// ResNet-18 patch extractor (the reference's SimCLR recipe: torchvision resnet18 with InstanceNorm2d, fc = Identity), inference only.
//
//   conv2d_nhwc_kernel     implicit-GEMM convolution on v_mfma_f32_32x32x16_bf16: M = B Ho Wo output pixels, N = Cout, K = KH KW Cin in
//                          tap-major / channel-minor order.  No im2col matrix in memory: a workgroup gathers its 128 x 64 A tile tap
//                          by tap from the NHWC input into LDS (taps outside the image are zero), the 64 x 64 weight tile next to it,
//                          and its 4 waves each own a 32 x 64 block of the output.  The next K step's global loads are in flight while
//                          the MFMAs of the current one run.  X3: fp32 operands split into bf16 hi + lo, hi hi + hi lo + lo hi (the
//                          fp32 class of gemm.hip); otherwise one bf16 product.  Output fp32 [M, Cout]; the last row tile is cut in
//                          the kernel.  The stem (7 x 7 / 2, Cin = 3, K = 147 padded to 192) is the same kernel with a gathering
//                          source: fp32 NCHW or uint8 NHWC (value / 255.0f: the division of to_tensor), three channels per tap.
//   instnorm_stats_kernel  mean and 1 / sqrt(var + eps) per (image, channel) of an fp32 NHWC map, two passes (mean, then the centred
//                          squares), fixed summation order for a given map size: no atomics, bit-reproducible.
//   norm_act_nhwc_kernel   y = (x - mean) rstd gamma + beta (+ identity) (ReLU), statistics per (image, channel) or per channel
//                          (eval-mode BatchNorm), output fp32 or bf16.
//   maxpool3x3s2 / avgpool the stem's max-pool (padding is -inf) and the global average pool.
// Every byte offset is 64-bit.
#include "mfma.h"

namespace {

constexpr int BM = 128, BN = 64, BK = 64;
constexpr int LDT = 72;   // LDS row pitch in bf16 (144 bytes): the 16-byte fragment reads of 16 consecutive rows fall on distinct banks

enum { SRC_F32 = 0, SRC_BF16 = 1, SRC_STEM_NCHW = 2, SRC_STEM_U8 = 3 };

struct ConvParams {
    const void* x;
    const unsigned short* wh;   // [cout, kp] bf16 (hi half under X3)
    const unsigned short* wl;   // [cout, kp] bf16 lo half (X3 only)
    float* out;                 // [m, cout]
    int h, w, cin, ho, wo, cout, kp, tiles_n;
    int64_t m;
};

template <int KH, int STRIDE, bool X3, int SRC>
__global__ __launch_bounds__(256) void conv2d_nhwc_kernel(ConvParams P) {
    constexpr int PAD = KH / 2;
    constexpr bool STEM = SRC >= SRC_STEM_NCHW;
    constexpr int NI = X3 ? 2 : 1;
    __shared__ __attribute__((aligned(16))) unsigned short As[NI][BM * LDT];
    __shared__ __attribute__((aligned(16))) unsigned short Bs[NI][BN * LDT];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int tile_n = blockIdx.x % P.tiles_n;
    const int64_t tile_m = blockIdx.x / P.tiles_n;

    // staging roles: thread (row arow, half ahalf) of the A tile carries 32 K elements of one output pixel per step; thread (row brow,
    // quarter bq) of the weight tile 16
    const int arow = tid >> 1, ahalf = tid & 1;
    const int64_t am = tile_m * BM + arow;
    const bool arow_ok = am < P.m;
    int img = 0, iy0 = 0, ix0 = 0;
    if (arow_ok) {
        const int hw = P.ho * P.wo;
        img = (int)(am / hw);
        const int rem = (int)(am - (int64_t)img * hw);
        const int oy = rem / P.wo, ox = rem - oy * P.wo;
        iy0 = oy * STRIDE - PAD, ix0 = ox * STRIDE - PAD;
    }
    const int brow = tid >> 2, bq = tid & 3;
    const int64_t woff = (int64_t)(tile_n * BN + brow) * P.kp + 16 * bq;
    const int cpt = STEM ? 1 : P.cin / BK;                          // K steps per tap
    const int nsteps = STEM ? (KH * KH * 3 + BK - 1) / BK : KH * KH * cpt;

    f32x8 af[4];     // fp32 / stem sources
    u32x4 ab[4];     // bf16 source
    u32x4 bh[2], bl[2];
    auto load = [&](int step) {
        if constexpr (STEM) {
            const float* xf = reinterpret_cast<const float*>(P.x);
            const unsigned char* xu = reinterpret_cast<const unsigned char*>(P.x);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int k = step * BK + ahalf * 32 + g * 8 + e;
                    const int tap = k / 3, c = k - 3 * tap;
                    const int ky = tap / KH, kx = tap - ky * KH;
                    const int iy = iy0 + ky, ix = ix0 + kx;
                    float v = 0.f;
                    if (arow_ok && k < KH * KH * 3 && iy >= 0 && iy < P.h && ix >= 0 && ix < P.w) {
                        if constexpr (SRC == SRC_STEM_NCHW)
                            v = xf[(((int64_t)img * 3 + c) * P.h + iy) * P.w + ix];
                        else
                            v = (float)xu[(((int64_t)img * P.h + iy) * P.w + ix) * 3 + c] / 255.0f;
                    }
                    af[g][e] = v;
                }
            }
        } else {
            const int tap = step / cpt, c0 = (step - tap * cpt) * BK + ahalf * 32;
            const int ky = tap / KH, kx = tap - ky * KH;
            const int iy = iy0 + ky, ix = ix0 + kx;
            const bool ok = arow_ok && iy >= 0 && iy < P.h && ix >= 0 && ix < P.w;
            const int64_t off = ok ? (((int64_t)img * P.h + iy) * P.w + ix) * P.cin + c0 : 0;
            if constexpr (SRC == SRC_F32) {
                const float* p = reinterpret_cast<const float*>(P.x) + off;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    if (ok) {
                        af[g] = load8(p + 8 * g);
                    } else {
#pragma unroll
                        for (int e = 0; e < 8; ++e) af[g][e] = 0.f;
                    }
                }
            } else {
                const unsigned short* p = reinterpret_cast<const unsigned short*>(P.x) + off;
#pragma unroll
                for (int g = 0; g < 4; ++g) ab[g] = ok ? *reinterpret_cast<const u32x4*>(p + 8 * g) : u32x4{0u, 0u, 0u, 0u};
            }
        }
        const int64_t wo_ = woff + (int64_t)step * BK;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            bh[i] = *reinterpret_cast<const u32x4*>(P.wh + wo_ + 8 * i);
            if constexpr (X3) bl[i] = *reinterpret_cast<const u32x4*>(P.wl + wo_ + 8 * i);
        }
    };
    auto store = [&]() {
        unsigned short* a0 = &As[0][arow * LDT + ahalf * 32];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            if constexpr (SRC == SRC_BF16) {
                *reinterpret_cast<u32x4*>(a0 + 8 * g) = ab[g];
            } else if constexpr (X3) {
                u32x4 hi, lo;
                split8(af[g], hi, lo);
                *reinterpret_cast<u32x4*>(a0 + 8 * g) = hi;
                *reinterpret_cast<u32x4*>(&As[NI - 1][arow * LDT + ahalf * 32 + 8 * g]) = lo;
            } else {
                *reinterpret_cast<u32x4*>(a0 + 8 * g) = __builtin_bit_cast(u32x4, __builtin_convertvector(af[g], bf16x8));
            }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            *reinterpret_cast<u32x4*>(&Bs[0][brow * LDT + 16 * bq + 8 * i]) = bh[i];
            if constexpr (X3) *reinterpret_cast<u32x4*>(&Bs[NI - 1][brow * LDT + 16 * bq + 8 * i]) = bl[i];
        }
    };

    f32x16 acc0, acc1;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc0[i] = 0.f, acc1[i] = 0.f;
    const int r = lane & 31, hf = lane >> 5;
    const int a_off = (32 * wv + r) * LDT + 8 * hf, b_off = r * LDT + 8 * hf;

    load(0);
    for (int step = 0; step < nsteps; ++step) {
        __syncthreads();   // the MFMAs of the previous step have read the tiles
        store();
        __syncthreads();
        if (step + 1 < nsteps) load(step + 1);
#pragma unroll
        for (int ks = 0; ks < BK / 16; ++ks) {
            const bf16x8 ah = load_frag(&As[0][a_off + 16 * ks]);
            const bf16x8 b0h = load_frag(&Bs[0][b_off + 16 * ks]);
            const bf16x8 b1h = load_frag(&Bs[0][b_off + 32 * LDT + 16 * ks]);
            if constexpr (X3) {
                const bf16x8 al = load_frag(&As[NI - 1][a_off + 16 * ks]);
                const bf16x8 b0l = load_frag(&Bs[NI - 1][b_off + 16 * ks]);
                const bf16x8 b1l = load_frag(&Bs[NI - 1][b_off + 32 * LDT + 16 * ks]);
                acc0 = mfma(al, b0h, acc0);
                acc1 = mfma(al, b1h, acc1);
                acc0 = mfma(ah, b0l, acc0);
                acc1 = mfma(ah, b1l, acc1);
            }
            acc0 = mfma(ah, b0h, acc0);
            acc1 = mfma(ah, b1h, acc1);
        }
    }
    // C layout: lane (r, hf) holds output channel r of rows (i & 3) + 8 (i >> 2) + 4 hf: 32 lanes store 128 consecutive bytes of a row
    float* o = P.out + (int64_t)tile_n * BN + r;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int64_t m = tile_m * BM + 32 * wv + (i & 3) + 8 * (i >> 2) + 4 * hf;
        if (m < P.m) {
            o[m * P.cout] = acc0[i];
            o[m * P.cout + 32] = acc1[i];
        }
    }
}

// weight [cout, cin, kh, kw] f32 (torch layout) -> image [cout, kp] in the kernel's K order (tap-major, channel-minor), zero beyond
// kh kw cin; hi = bf16(w), lo (nullable) = bf16(w - hi)
__global__ __launch_bounds__(256) void conv_pack_weight_kernel(const float* __restrict__ w, int cout, int cin, int kh, int kw, int kp,
                                                               unsigned short* __restrict__ hi, unsigned short* __restrict__ lo) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)cout * kp) return;
    const int co = (int)(i / kp), k = (int)(i - (int64_t)co * kp);
    float v = 0.f;
    if (k < kh * kw * cin) {
        const int tap = k / cin, c = k - tap * cin;
        const int ky = tap / kw, kx = tap - ky * kw;
        v = w[(((int64_t)co * cin + c) * kh + ky) * kw + kx];
    }
    const unsigned short h = f32_to_bf16_bits(v);
    hi[i] = h;
    if (lo) lo[i] = f32_to_bf16_bits(v - bf16_bits_to_f32(h));
}

// one workgroup per (32 channels, image): thread (l4, p) walks pixels p, p + SLOTS, ... of channels 4 l4 .. + 3 (8 lanes read the 128
// contiguous bytes of a pixel); the pixel slots are summed in slot order by the first 32 threads.  NT = 1024 threads (128 slots) for the
// large maps, where a (32 channels, image) pair is all the parallelism there is; 256 (32 slots) otherwise.  AVG: only the mean, written
// to `mean` (the global average pool).
constexpr int STAT_CW = 32;
template <bool AVG, int NT>
__global__ __launch_bounds__(NT) void instnorm_stats_kernel(const float* __restrict__ x, int64_t hw, int c, float eps,
                                                            float* __restrict__ mean, float* __restrict__ rstd) {
    constexpr int LP = STAT_CW / 4, SLOTS = NT / LP;
    __shared__ float red[SLOTS][STAT_CW];
    __shared__ float mu[STAT_CW];
    const int tid = threadIdx.x, l4 = tid % LP, p = tid / LP;
    const int cb = blockIdx.x, b = blockIdx.y;
    const float* base = x + (int64_t)b * hw * c + cb * STAT_CW + 4 * l4;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    for (int64_t q = p; q < hw; q += SLOTS) s += *reinterpret_cast<const f32x4*>(base + q * c);
#pragma unroll
    for (int e = 0; e < 4; ++e) red[p][4 * l4 + e] = s[e];
    __syncthreads();
    if (tid < STAT_CW) {
        float t = 0.f;
        for (int q = 0; q < SLOTS; ++q) t += red[q][tid];
        t = t / (float)hw;
        mu[tid] = t;
        if constexpr (AVG) mean[(int64_t)b * c + cb * STAT_CW + tid] = t;
    }
    if constexpr (AVG) return;
    __syncthreads();
    const f32x4 m = {mu[4 * l4], mu[4 * l4 + 1], mu[4 * l4 + 2], mu[4 * l4 + 3]};
    s = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int64_t q = p; q < hw; q += SLOTS) {
        const f32x4 d = *reinterpret_cast<const f32x4*>(base + q * c) - m;
        s += d * d;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) red[p][4 * l4 + e] = s[e];
    __syncthreads();
    if (tid < STAT_CW) {
        float t = 0.f;
        for (int q = 0; q < SLOTS; ++q) t += red[q][tid];
        const int64_t o = (int64_t)b * c + cb * STAT_CW + tid;
        mean[o] = mu[tid];
        rstd[o] = 1.0f / sqrtf(t / (float)hw + eps);
    }
}

// grid (chunks of an image's hw c / 4 float4 groups, image)
template <bool OUT_BF16>
__global__ __launch_bounds__(256) void norm_act_nhwc_kernel(const float* __restrict__ x, int n4, int c, const float* __restrict__ mean,
                                                            const float* __restrict__ rstd, int per_image, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, const float* __restrict__ identity, int relu,
                                                            void* __restrict__ out) {
    const int b = blockIdx.y;
    const int64_t ioff = (int64_t)b * n4 * 4;
    const int64_t soff = per_image ? (int64_t)b * c : 0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n4; i += gridDim.x * 256) {
        const int ch = (int)(((int64_t)i * 4) % c);
        const int64_t e = ioff + (int64_t)i * 4;
        f32x4 v = *reinterpret_cast<const f32x4*>(x + e);
        const f32x4 mu = *reinterpret_cast<const f32x4*>(mean + soff + ch), rs = *reinterpret_cast<const f32x4*>(rstd + soff + ch);
        v = (v - mu) * rs;
        if (gamma) v = v * *reinterpret_cast<const f32x4*>(gamma + ch);
        if (beta) v = v + *reinterpret_cast<const f32x4*>(beta + ch);
        if (identity) v = v + *reinterpret_cast<const f32x4*>(identity + e);
        if (relu) {
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = v[q] > 0.f ? v[q] : 0.f;
        }
        if constexpr (OUT_BF16) {
            u32x2 pk = {pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
            *reinterpret_cast<u32x2*>(reinterpret_cast<unsigned short*>(out) + e) = pk;
        } else {
            *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(out) + e) = v;
        }
    }
}

// 3 x 3 / 2, pad 1 (padding never wins: -inf); grid (chunks of ho wo c / 4, image)
__global__ __launch_bounds__(256) void maxpool3x3s2_nhwc_kernel(const float* __restrict__ x, int h, int w, int c, int ho, int wo,
                                                                float* __restrict__ out) {
    const int b = blockIdx.y, c4 = c >> 2, n4 = ho * wo * c4;
    const float* xb = x + (int64_t)b * h * w * c;
    float* ob = out + (int64_t)b * n4 * 4;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n4; i += gridDim.x * 256) {
        const int pix = i / c4, ch = (i - pix * c4) * 4;
        const int oy = pix / wo, ox = pix - oy * wo;
        const float ninf = -__builtin_inff();
        f32x4 v = {ninf, ninf, ninf, ninf};
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int iy = 2 * oy - 1 + ky, ix = 2 * ox - 1 + kx;
                if (iy >= 0 && iy < h && ix >= 0 && ix < w) {
                    const f32x4 t = *reinterpret_cast<const f32x4*>(xb + ((int64_t)iy * w + ix) * c + ch);
#pragma unroll
                    for (int q = 0; q < 4; ++q) v[q] = t[q] > v[q] ? t[q] : v[q];
                }
            }
        }
        *reinterpret_cast<f32x4*>(ob + (int64_t)i * 4) = v;
    }
}

bool conv_width(int c) { return c == 64 || c == 128 || c == 256 || c == 512; }
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <int KH, int STRIDE, int SRC>
int launch_conv(const ConvParams& P, bool x3, int64_t grid, hipStream_t s) {
    if (x3) {
        if constexpr (SRC == SRC_BF16) {
            return SNF_EINVAL;   // refused by the caller
        } else {
            hipLaunchKernelGGL((conv2d_nhwc_kernel<KH, STRIDE, true, SRC>), dim3((unsigned)grid), dim3(256), 0, s, P);
        }
    } else {
        hipLaunchKernelGGL((conv2d_nhwc_kernel<KH, STRIDE, false, SRC>), dim3((unsigned)grid), dim3(256), 0, s, P);
    }
    return snf::check_launch("conv2d_nhwc_kernel");
}

}  // namespace

extern "C" int snf_conv2d_nhwc_plan(int b, int h, int w, int cin, int cout, int kh, int stride, int* ho, int* wo, int64_t* m, int* tiles_m,
                                    int* tiles_n, size_t* workspace_bytes) {
    SNF_REQUIRE(b >= 1 && h >= 1 && w >= 1, "snf_conv2d_nhwc_plan: bad shape b=%d h=%d w=%d", b, h, w);
    const bool stem = kh == 7 && stride == 2 && cin == 3 && cout == 64;
    const bool body = ((kh == 3 && (stride == 1 || stride == 2)) || (kh == 1 && stride == 2)) && conv_width(cin) && conv_width(cout);
    if (!stem && !body) {
        snf::set_error("snf_conv2d_nhwc_plan: no kernel for a %dx%d / %d convolution %d -> %d (3x3 / 1, 3x3 / 2, 1x1 / 2 over 64, 128, 256, "
                       "512 channels; 7x7 / 2 from 3 to 64)", kh, kh, stride, cin, cout);
        return SNF_EUNSUPPORTED;
    }
    const int pad = kh / 2;
    const int oh = (h + 2 * pad - kh) / stride + 1, ow = (w + 2 * pad - kh) / stride + 1;
    SNF_REQUIRE(h + 2 * pad >= kh && w + 2 * pad >= kh && oh >= 1 && ow >= 1, "snf_conv2d_nhwc_plan: empty output");
    const int64_t rows = (int64_t)b * oh * ow;
    const int64_t tm = (rows + BM - 1) / BM;
    if ((int64_t)oh * ow >= (1ll << 31) || tm * (cout / BN) >= (1ll << 31)) {
        snf::set_error("snf_conv2d_nhwc_plan: %lld output pixels are more than one launch holds: split the batch", (long long)rows);
        return SNF_EUNSUPPORTED;
    }
    if (ho) *ho = oh;
    if (wo) *wo = ow;
    if (m) *m = rows;
    if (tiles_m) *tiles_m = (int)tm;
    if (tiles_n) *tiles_n = cout / BN;
    if (workspace_bytes) *workspace_bytes = 0;   // the statistics are a pass of their own (snf_instnorm_stats_nhwc)
    return SNF_OK;
}

extern "C" int snf_conv_pack_weight_f32(const float* w, int cout, int cin, int kh, int kw, int kp, void* hi_bf16, void* lo_bf16,
                                        snf_stream_t stream) {
    SNF_REQUIRE(w && hi_bf16, "snf_conv_pack_weight_f32: null pointer");
    SNF_REQUIRE(cout >= 1 && cin >= 1 && kh >= 1 && kw >= 1 && (int64_t)kh * kw * cin <= kp && kp % BK == 0 && (int64_t)cout * kp < (1ll << 31),
                "snf_conv_pack_weight_f32: bad shape (cout %d cin %d %dx%d, row length %d must be a multiple of %d and hold the taps)", cout,
                cin, kh, kw, kp, BK);
    const int64_t n = (int64_t)cout * kp;
    hipLaunchKernelGGL(conv_pack_weight_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, snf::as_stream(stream), w, cout, cin, kh, kw,
                       kp, reinterpret_cast<unsigned short*>(hi_bf16), reinterpret_cast<unsigned short*>(lo_bf16));
    return snf::check_launch("conv_pack_weight_kernel");
}

extern "C" int snf_conv2d_nhwc(const void* x, int x_dtype, const void* w_hi, const void* w_lo, int b, int h, int w, int cin, int cout, int kh,
                               int stride, float* out, snf_stream_t stream) {
    SNF_REQUIRE(x && w_hi && out, "snf_conv2d_nhwc: null pointer");
    SNF_REQUIRE(x_dtype == SNF_DT_F32 || x_dtype == SNF_DT_BF16, "snf_conv2d_nhwc: x must be f32 or bf16");
    SNF_REQUIRE(!(w_lo && x_dtype != SNF_DT_F32), "snf_conv2d_nhwc: the hi / lo (fp32-class) product takes fp32 activations");
    SNF_REQUIRE(aligned16(x) && aligned16(w_hi) && aligned16(w_lo) && aligned16(out), "snf_conv2d_nhwc: pointers must be 16-byte aligned");
    SNF_REQUIRE(kh != 7, "snf_conv2d_nhwc: the 7x7 stem is snf_conv_stem");
    ConvParams P;
    int tm = 0;
    if (int rc = snf_conv2d_nhwc_plan(b, h, w, cin, cout, kh, stride, &P.ho, &P.wo, &P.m, &tm, &P.tiles_n, nullptr)) return rc;
    P.x = x, P.wh = reinterpret_cast<const unsigned short*>(w_hi), P.wl = reinterpret_cast<const unsigned short*>(w_lo), P.out = out;
    P.h = h, P.w = w, P.cin = cin, P.cout = cout, P.kp = kh * kh * cin;
    const int64_t grid = (int64_t)tm * P.tiles_n;
    hipStream_t s = snf::as_stream(stream);
    const bool x3 = w_lo != nullptr, bf = x_dtype == SNF_DT_BF16;
    if (kh == 3 && stride == 1) return bf ? launch_conv<3, 1, SRC_BF16>(P, x3, grid, s) : launch_conv<3, 1, SRC_F32>(P, x3, grid, s);
    if (kh == 3 && stride == 2) return bf ? launch_conv<3, 2, SRC_BF16>(P, x3, grid, s) : launch_conv<3, 2, SRC_F32>(P, x3, grid, s);
    return bf ? launch_conv<1, 2, SRC_BF16>(P, x3, grid, s) : launch_conv<1, 2, SRC_F32>(P, x3, grid, s);
}

extern "C" int snf_conv_stem(const void* x, int src_u8_nhwc, const void* w_hi, const void* w_lo, int b, int h, int w, float* out,
                             snf_stream_t stream) {
    SNF_REQUIRE(x && w_hi && out, "snf_conv_stem: null pointer");
    SNF_REQUIRE(aligned16(w_hi) && aligned16(w_lo) && aligned16(out), "snf_conv_stem: weight images and output must be 16-byte aligned");
    ConvParams P;
    int tm = 0;
    if (int rc = snf_conv2d_nhwc_plan(b, h, w, 3, 64, 7, 2, &P.ho, &P.wo, &P.m, &tm, &P.tiles_n, nullptr)) return rc;
    P.x = x, P.wh = reinterpret_cast<const unsigned short*>(w_hi), P.wl = reinterpret_cast<const unsigned short*>(w_lo), P.out = out;
    P.h = h, P.w = w, P.cin = 3, P.cout = 64, P.kp = 3 * BK;   // 147 taps x channels, zero-padded to 192
    const int64_t grid = (int64_t)tm * P.tiles_n;
    hipStream_t s = snf::as_stream(stream);
    return src_u8_nhwc ? launch_conv<7, 2, SRC_STEM_U8>(P, w_lo != nullptr, grid, s)
                       : launch_conv<7, 2, SRC_STEM_NCHW>(P, w_lo != nullptr, grid, s);
}

extern "C" int snf_instnorm_stats_nhwc(const float* x, int b, int64_t hw, int c, float eps, float* mean, float* rstd, snf_stream_t stream) {
    SNF_REQUIRE(x && mean && rstd, "snf_instnorm_stats_nhwc: null pointer");
    SNF_REQUIRE(b >= 1 && b <= 65535 && hw >= 1 && c >= 64 && c % 64 == 0 && aligned16(x),
                "snf_instnorm_stats_nhwc: bad shape (b %d in 1 .. 65535, hw %lld, c %d a multiple of 64, x 16-byte aligned)", b, (long long)hw, c);
    if (hw >= 2048)
        hipLaunchKernelGGL((instnorm_stats_kernel<false, 1024>), dim3(c / STAT_CW, b), dim3(1024), 0, snf::as_stream(stream), x, hw, c, eps,
                           mean, rstd);
    else
        hipLaunchKernelGGL((instnorm_stats_kernel<false, 256>), dim3(c / STAT_CW, b), dim3(256), 0, snf::as_stream(stream), x, hw, c, eps,
                           mean, rstd);
    return snf::check_launch("instnorm_stats_kernel");
}

extern "C" int snf_avgpool_nhwc(const float* x, int b, int64_t hw, int c, float* out, snf_stream_t stream) {
    SNF_REQUIRE(x && out, "snf_avgpool_nhwc: null pointer");
    SNF_REQUIRE(b >= 1 && b <= 65535 && hw >= 1 && c >= 64 && c % 64 == 0 && aligned16(x),
                "snf_avgpool_nhwc: bad shape (b %d in 1 .. 65535, hw %lld, c %d a multiple of 64, x 16-byte aligned)", b, (long long)hw, c);
    hipLaunchKernelGGL((instnorm_stats_kernel<true, 256>), dim3(c / STAT_CW, b), dim3(256), 0, snf::as_stream(stream), x, hw, c, 0.f, out,
                       static_cast<float*>(nullptr));
    return snf::check_launch("instnorm_stats_kernel<avg>");
}

extern "C" int snf_norm_act_nhwc(const float* x, int b, int64_t hw, int c, const float* mean, const float* rstd, int per_image,
                                 const float* gamma, const float* beta, const float* identity, int relu, void* out, int out_dtype,
                                 snf_stream_t stream) {
    SNF_REQUIRE(x && mean && rstd && out, "snf_norm_act_nhwc: null pointer");
    SNF_REQUIRE(out_dtype == SNF_DT_F32 || out_dtype == SNF_DT_BF16, "snf_norm_act_nhwc: output must be f32 or bf16");
    SNF_REQUIRE(b >= 1 && b <= 65535 && hw >= 1 && c >= 4 && c % 4 == 0 && hw * c / 4 < (1ll << 31) - 256 * 4096,
                "snf_norm_act_nhwc: bad shape (b %d in 1 .. 65535, hw %lld, c %d a multiple of 4)", b, (long long)hw, c);
    SNF_REQUIRE(aligned16(x) && aligned16(mean) && aligned16(rstd) && aligned16(gamma) && aligned16(beta) && aligned16(identity) &&
                    (reinterpret_cast<uintptr_t>(out) & 7) == 0,
                "snf_norm_act_nhwc: pointers must be 16-byte aligned");
    const int n4 = (int)(hw * c / 4);
    int gx = (n4 + 255) / 256;
    if (gx > 4096) gx = 4096;
    hipStream_t s = snf::as_stream(stream);
    if (out_dtype == SNF_DT_BF16)
        hipLaunchKernelGGL(norm_act_nhwc_kernel<true>, dim3(gx, b), dim3(256), 0, s, x, n4, c, mean, rstd, per_image, gamma, beta, identity,
                           relu, out);
    else
        hipLaunchKernelGGL(norm_act_nhwc_kernel<false>, dim3(gx, b), dim3(256), 0, s, x, n4, c, mean, rstd, per_image, gamma, beta, identity,
                           relu, out);
    return snf::check_launch("norm_act_nhwc_kernel");
}

extern "C" int snf_maxpool3x3s2_nhwc(const float* x, int b, int h, int w, int c, float* out, snf_stream_t stream) {
    SNF_REQUIRE(x && out, "snf_maxpool3x3s2_nhwc: null pointer");
    SNF_REQUIRE(b >= 1 && b <= 65535 && h >= 1 && w >= 1 && c >= 4 && c % 4 == 0 && (int64_t)h * w * c < (1ll << 31) && aligned16(x) &&
                    aligned16(out),
                "snf_maxpool3x3s2_nhwc: bad shape (b %d in 1 .. 65535, %d x %d x %d, c a multiple of 4, 16-byte aligned)", b, h, w, c);
    const int ho = (h - 1) / 2 + 1, wo = (w - 1) / 2 + 1;
    const int n4 = ho * wo * (c / 4);
    int gx = (n4 + 255) / 256;
    if (gx > 4096) gx = 4096;
    hipLaunchKernelGGL(maxpool3x3s2_nhwc_kernel, dim3(gx, b), dim3(256), 0, snf::as_stream(stream), x, h, w, c, ho, wo, out);
    return snf::check_launch("maxpool3x3s2_nhwc_kernel");
}
