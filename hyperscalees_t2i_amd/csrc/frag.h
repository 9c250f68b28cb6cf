// Fragment types and lane-group reductions shared by the model-side units (eggroll_model.hip, eggroll_attn.hip).
#pragma once
#include "common.h"

namespace eggroll {

typedef __attribute__((ext_vector_type(8))) unsigned short u16x8m;
typedef __attribute__((ext_vector_type(4))) unsigned short u16x4m;
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

}  // namespace eggroll
