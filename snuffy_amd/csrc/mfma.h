// Device primitives shared by the MFMA kernels (gfx950): vector types, compile-time loop, fragment loads, the fp32 -> bf16 hi + lo
// split, the transposing LDS read and the half-wave all-reduce.  Everything is internal to the including translation unit.
#pragma once
#include <type_traits>

#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(8))) float f32x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
typedef __attribute__((address_space(3))) void lds_void;
typedef const __attribute__((address_space(1))) void glb_void;

// compile-time loop: every index into the register-resident fragment arrays must be a constant, or the arrays go to
// scratch (a "#pragma unroll" is only a hint and gives up on the larger variants)
template <int I, int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"i"(N) : "memory");
}

// 8 consecutive floats as two 16-byte loads
__device__ __forceinline__ f32x8 load8(const float* p) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
    return f32x8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}
// 8 consecutive elements -> bf16x8 (f32 source converted with v_cvt_pk_bf16_f32, round-to-nearest-even)
__device__ __forceinline__ bf16x8 load_frag(const float* p) { return __builtin_convertvector(load8(p), bf16x8); }
__device__ __forceinline__ bf16x8 load_frag(const unsigned short* p) {
    return __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(p));
}

// x (8 fp32) -> hi = bf16(x), lo = bf16(x - hi); the second form hands the halves over as packed dwords
__device__ __forceinline__ void split8(const f32x8 x, bf16x8& hi, bf16x8& lo) {
    hi = __builtin_convertvector(x, bf16x8);
    lo = __builtin_convertvector(x - __builtin_convertvector(hi, f32x8), bf16x8);
}
__device__ __forceinline__ void split8(const f32x8 x, u32x4& hi, u32x4& lo) {
    bf16x8 h, l;
    split8(x, h, l);
    hi = __builtin_bit_cast(u32x4, h), lo = __builtin_bit_cast(u32x4, l);
}

// One transposed MFMA operand (8 consecutive rows of one column in a lane's registers) out of a row-major bf16 image in LDS:
// two hardware transpose-reads.  ds_read_b64_tr_b16 semantics (probed on gfx950, tools/probes/tr16_probe.hip): every lane
// supplies the address of its own 8-byte chunk; inside each group of 16 lanes the 16 chunks form a [4 rows][16 columns]
// bf16 matrix (lane i = row i>>2, columns 4(i&3)..+3) and lane i receives column i.
__device__ __forceinline__ bf16x8 tr_frag(const unsigned char* p0, const unsigned char* p1) {
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)p0);
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)p1);
    return __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

// all-reduce across the two half-waves (lane l <-> lane l^32) on the VALU: v_permlane32_swap(x, x) = {x.lo, x.lo}, {x.hi, x.hi}
__device__ __forceinline__ float xhalf_max(float v) {
    const unsigned u = __float_as_uint(v);
    auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float xhalf_sum(float v) {
    const unsigned u = __float_as_uint(v);
    auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

__device__ __forceinline__ f32x16 mfma(bf16x8 a, bf16x8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }

}  // namespace
