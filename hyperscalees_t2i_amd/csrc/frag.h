// Fragment types, bf16 helpers and lane-group reductions of eggroll_nhwc / _norm / _qk / _linattn / _attn / _image.hip.
#pragma once
#include "common.h"

namespace eggroll {

typedef __attribute__((ext_vector_type(8))) unsigned short u16x8m;
typedef __attribute__((ext_vector_type(4))) unsigned short u16x4m;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2m;
typedef __attribute__((ext_vector_type(8))) __bf16 la_bf16x8;  // MFMA 16x16x32 operand fragment
typedef __attribute__((ext_vector_type(4))) float la_f32x4;     // MFMA 16x16 accumulator fragment
typedef __attribute__((ext_vector_type(4))) short la_s4;        // one ds_read_tr16_b64 result
typedef __attribute__((address_space(3))) la_s4 la_lds_s4;

__device__ __forceinline__ float b2f(unsigned short h) { return __uint_as_float(((uint32_t)h) << 16); }
__device__ __forceinline__ unsigned short f2b(float f) {
    __bf16 b = (__bf16)f;
    return *reinterpret_cast<unsigned short*>(&b);
}

// Reductions over the 4 lane groups of 16 (xor 16, then xor 32) on v_permlane16_swap / v_permlane32_swap
// instead of two ds_bpermute shuffles (LDS round trips): each swap returns the lane's own value and its
// partner's, combined exactly as `v op __shfl_xor(v, 16)` then `op __shfl_xor(v, 32)` (+ and max are
// commutative, so the same bits).
__device__ __forceinline__ float g4_sum(float v) {
    auto r = __builtin_amdgcn_permlane16_swap(__builtin_bit_cast(unsigned, v), __builtin_bit_cast(unsigned, v), false, false);
    v = __builtin_bit_cast(float, (unsigned)r[0]) + __builtin_bit_cast(float, (unsigned)r[1]);
    r = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, v), __builtin_bit_cast(unsigned, v), false, false);
    return __builtin_bit_cast(float, (unsigned)r[0]) + __builtin_bit_cast(float, (unsigned)r[1]);
}
__device__ __forceinline__ float g4_max(float v) {
    auto r = __builtin_amdgcn_permlane16_swap(__builtin_bit_cast(unsigned, v), __builtin_bit_cast(unsigned, v), false, false);
    v = fmaxf(__builtin_bit_cast(float, (unsigned)r[0]), __builtin_bit_cast(float, (unsigned)r[1]));
    r = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, v), __builtin_bit_cast(unsigned, v), false, false);
    return fmaxf(__builtin_bit_cast(float, (unsigned)r[0]), __builtin_bit_cast(float, (unsigned)r[1]));
}

// x * sigmoid(x) with the hardware reciprocal (v_rcp_f32, ~1 ulp) instead of an IEEE division
// (v_div_scale/fmas/fixup): every caller rounds the result to bf16.
__device__ __forceinline__ float silu(float x) { return x * __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }

// Sum over SEG-lane segments (16 / 32 / 64) without LDS round trips, as the xor butterfly
// __shfl_xor(·, SEG/2 ... 1) computes it — the same additions in the same order, so the same bits in every
// lane: xor 32 / xor 16 by v_permlane32_swap / v_permlane16_swap (gfx950; called on one register twice,
// the two results are each lane's own value and its partner's, and their sum is the butterfly step), xor 8
// by DPP row_ror:8; after that every value is symmetric under xor 8, so row_ror:4 reads the xor-4 partner;
// quad_perm does xor 2 and xor 1.
template <int CTRL>
__device__ __forceinline__ float dpp_f(float x) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xf, 0xf, false));
}
template <int SEG>
__device__ __forceinline__ float seg_sum(float v) {
    static_assert(SEG == 16 || SEG == 32 || SEG == 64, "segment of 16, 32 or 64 lanes");
    if constexpr (SEG == 64) {
        const auto r = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, v), __builtin_bit_cast(unsigned, v),
                                                         false, false);
        v = __builtin_bit_cast(float, (unsigned)r[0]) + __builtin_bit_cast(float, (unsigned)r[1]);
    }
    if constexpr (SEG >= 32) {
        const auto r = __builtin_amdgcn_permlane16_swap(__builtin_bit_cast(unsigned, v), __builtin_bit_cast(unsigned, v),
                                                         false, false);
        v = __builtin_bit_cast(float, (unsigned)r[0]) + __builtin_bit_cast(float, (unsigned)r[1]);
    }
    v += dpp_f<0x128>(v);  // row_ror:8 = xor 8
    v += dpp_f<0x124>(v);  // row_ror:4 = xor 4 here
    v += dpp_f<0x4E>(v);   // quad_perm [2,3,0,1] = xor 2
    v += dpp_f<0xB1>(v);   // quad_perm [1,0,3,2] = xor 1
    return v;
}

// 8 consecutive values of a bf16 (f32 = 0) or fp32 (f32 = 1) vector as floats
__device__ __forceinline__ void load8f(const void* p, int f32, int64_t off, float (&o)[8]) {
    if (f32) {
        const float4 a0 = *reinterpret_cast<const float4*>((const float*)p + off);
        const float4 a1 = *reinterpret_cast<const float4*>((const float*)p + off + 4);
        o[0] = a0.x; o[1] = a0.y; o[2] = a0.z; o[3] = a0.w; o[4] = a1.x; o[5] = a1.y; o[6] = a1.z; o[7] = a1.w;
    } else {
        const u16x8m q = *reinterpret_cast<const u16x8m*>((const unsigned short*)p + off);
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] = b2f(q[i]);
    }
}

}  // namespace eggroll
