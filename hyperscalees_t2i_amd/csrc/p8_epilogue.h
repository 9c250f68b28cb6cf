// libeggroll — the epilogue pieces of the 8-phase kernels that both eggroll_lora.hip and
// eggroll_conv.hip use: the epilogue ops, the per-wave C-tile store and the MFMA bias / LoRA addend.
#pragma once
#include "p8.h"

namespace eggroll {

// Epilogue ops applied to the bf16-rounded GEMM output y (one rounding per torch op it replaces):
//   EPI_SILU  : out = bf16(silu(y))                        (GLUMBConv: 1x1 conv -> SiLU)
//   EPI_RES   : out = bf16(res + y)                        (x = x + attn2(...))
//   EPI_GATED : out = bf16(res + gate[row / rpg] * y)      (x += gate * attn1(...), k_gated_residual)
// res may alias Y (each element is read and written by the same lane).
// fp32 residual stream (Sana blocks) — res is an fp32 [M, ldr] stream updated in place,
// Y (optional, may be NULL) receives its bf16 shadow copy (the next GEMM's operand):
//   EPI_RES32   : res = res + float(y)                     (x = x + attn2(...))
//   EPI_GATED32 : res = fma(gate32[row / rpg], float(y), res)  (x += gate * attn1(...); gate fp32)
// The same expressions as eggroll_gated_residual_f32, so fused == unfused bit for bit.
//   EPI_GELU  : out = bf16(gelu_tanh(y))                   (Infinity / VAR ffn: fc1 -> GELU(tanh))
//   EPI_MUL   : out = bf16(res * y)                        (Z-Image SwiGLU: silu(w1 x) * w3 x)
//   EPI_GELU_ERF : out = bf16(gelu(y))                     (PickScore CLIP-H/14 mlp: fc1 -> exact GELU)
enum { EPI_NONE = 0, EPI_SILU = 1, EPI_RES = 2, EPI_GATED = 3, EPI_RES32 = 4, EPI_GATED32 = 5, EPI_GELU = 6, EPI_MUL = 7,
       EPI_GELU_ERF = 8 };
struct EpiArgs {
    const unsigned short* res;
    int64_t ldr;
    const unsigned short* gate;
    int64_t gstride;
    int64_t rpg;
};
__device__ __forceinline__ float epi_silu(float v) { return v * __builtin_amdgcn_rcpf(1.0f + __expf(-v)); }
// GELU, approximate = "tanh": 0.5 x (1 + tanh(k)) = x * sigmoid(2k), k = sqrt(2/pi) (x + 0.044715 x^3),
// with the hardware exp2 / rcp as the SiLU epilogue (ocml's tanhf made the fc1 store phase 15 % of the
// GEMM: tools/gelu_epi_probe.py); within 1 bf16 ulp of torch's tanh form
__device__ __forceinline__ float epi_gelu(float x) {
    constexpr float kBeta2L = (float)(M_SQRT2 * M_2_SQRTPI * 0.5 * 2.0 * 1.4426950408889634);
    constexpr float kKappa = 0.044715f;
    const float u = x + kKappa * (x * x * x);
    return x * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-kBeta2L * u));
}
// GELU, approximate = "none": x * 0.5 * (1 + erf(x / sqrt 2)) in fp32, the expression (and the erff) torch's
// GeluCUDAKernelImpl evaluates on a bf16 tensor, so fused == F.gelu(bf16 GEMM output) bit for bit
// (test_lora_linear_pop_gelu_erf_bitexact)
__device__ __forceinline__ float epi_gelu_erf(float x) {
    return x * 0.5f * (1.0f + erff(x * (float)M_SQRT1_2));
}

// x * sigmoid(x) on two values: the multiplies / add as packed fp32 ops (v_pk_mul_f32 / v_pk_add_f32),
// exp2 and rcp per value: the same operations, value by value, as x * rcp(1 + __expf(-x)) (v_mul by
// log2(e), v_exp_f32, v_add, v_rcp_f32, v_mul), so the same bits (test_lora_linear_pop_epilogue_bitexact;
// test_epilogue_layouts stores the same elements through this form and through epi_apply1: equal bits)
__device__ __forceinline__ f32x2 silu2(f32x2 v) {
    f32x2 t = v * (f32x2){-1.4426950408889634f, -1.4426950408889634f};
    t.x = __builtin_amdgcn_exp2f(t.x);
    t.y = __builtin_amdgcn_exp2f(t.y);
    t = t + (f32x2){1.0f, 1.0f};
    t.x = __builtin_amdgcn_rcpf(t.x);
    t.y = __builtin_amdgcn_rcpf(t.y);
    return v * t;
}

template <int EPI>
__device__ __forceinline__ u16x8 epi_apply(u16x8 v, int row, int col, const EpiArgs& ea) {
    if constexpr (EPI == EPI_SILU) {
#pragma unroll
        for (int u = 0; u < 8; u += 2) {
            const f32x2 t = silu2((f32x2){bf16_to_f32(v[u]), bf16_to_f32(v[u + 1])});
            v[u] = f32_to_bf16(t.x);
            v[u + 1] = f32_to_bf16(t.y);
        }
    } else if constexpr (EPI == EPI_GELU) {
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = f32_to_bf16(epi_gelu(bf16_to_f32(v[u])));
    } else if constexpr (EPI == EPI_GELU_ERF) {
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = f32_to_bf16(epi_gelu_erf(bf16_to_f32(v[u])));
    } else if constexpr (EPI == EPI_RES || EPI == EPI_GATED || EPI == EPI_MUL) {
        const u16x8 r = *reinterpret_cast<const u16x8*>(ea.res + (int64_t)row * ea.ldr + col);
        if constexpr (EPI == EPI_MUL) {
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = f32_to_bf16(bf16_to_f32(r[u]) * bf16_to_f32(v[u]));
        } else if constexpr (EPI == EPI_RES) {
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = f32_to_bf16(bf16_to_f32(r[u]) + bf16_to_f32(v[u]));
        } else {
            const u16x8 g = *reinterpret_cast<const u16x8*>(ea.gate + (row / ea.rpg) * ea.gstride + col);
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = f32_to_bf16(bf16_to_f32(r[u]) + bf16_to_f32(g[u]) * bf16_to_f32(v[u]));
        }
    }
    return v;
}
// EPI_RES32 / EPI_GATED32 on one 8-column chunk (vector) or one element (tail)
template <int EPI>
__device__ __forceinline__ void epi_store32(u16x8 v, int row, int col, const EpiArgs& ea, unsigned short* Y, int64_t ldy) {
    float* r = const_cast<float*>(reinterpret_cast<const float*>(ea.res)) + (int64_t)row * ea.ldr + col;
    float4 a0 = *reinterpret_cast<const float4*>(r), a1 = *reinterpret_cast<const float4*>(r + 4);
    float x[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
    if constexpr (EPI == EPI_GATED32) {
        const float* g = reinterpret_cast<const float*>(ea.gate) + (row / ea.rpg) * ea.gstride + col;
        const float4 g0 = *reinterpret_cast<const float4*>(g), g1 = *reinterpret_cast<const float4*>(g + 4);
        const float gv[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
#pragma unroll
        for (int u = 0; u < 8; ++u) x[u] = __builtin_fmaf(gv[u], bf16_to_f32(v[u]), x[u]);
    } else {
#pragma unroll
        for (int u = 0; u < 8; ++u) x[u] = x[u] + bf16_to_f32(v[u]);
    }
    *reinterpret_cast<float4*>(r) = float4{x[0], x[1], x[2], x[3]};
    *reinterpret_cast<float4*>(r + 4) = float4{x[4], x[5], x[6], x[7]};
    if (Y) {
        u16x8 o;
#pragma unroll
        for (int u = 0; u < 8; ++u) o[u] = f32_to_bf16(x[u]);
        *reinterpret_cast<u16x8*>(Y + (int64_t)row * ldy + col) = o;
    }
}
template <int EPI>
__device__ __forceinline__ void epi_store32_1(unsigned short v, int row, int col, const EpiArgs& ea, unsigned short* Y,
                                              int64_t ldy) {
    float* r = const_cast<float*>(reinterpret_cast<const float*>(ea.res)) + (int64_t)row * ea.ldr + col;
    float x = *r;
    if constexpr (EPI == EPI_GATED32)
        x = __builtin_fmaf(reinterpret_cast<const float*>(ea.gate)[(row / ea.rpg) * ea.gstride + col], bf16_to_f32(v), x);
    else
        x = x + bf16_to_f32(v);
    *r = x;
    if (Y) Y[(int64_t)row * ldy + col] = f32_to_bf16(x);
}

template <int EPI>
__device__ __forceinline__ unsigned short epi_apply1(unsigned short v, int row, int col, const EpiArgs& ea) {
    if constexpr (EPI == EPI_SILU) return f32_to_bf16(epi_silu(bf16_to_f32(v)));
    if constexpr (EPI == EPI_GELU) return f32_to_bf16(epi_gelu(bf16_to_f32(v)));
    if constexpr (EPI == EPI_GELU_ERF) return f32_to_bf16(epi_gelu_erf(bf16_to_f32(v)));
    if constexpr (EPI == EPI_RES) return f32_to_bf16(bf16_to_f32(ea.res[(int64_t)row * ea.ldr + col]) + bf16_to_f32(v));
    if constexpr (EPI == EPI_MUL) return f32_to_bf16(bf16_to_f32(ea.res[(int64_t)row * ea.ldr + col]) * bf16_to_f32(v));
    if constexpr (EPI == EPI_GATED)
        return f32_to_bf16(bf16_to_f32(ea.res[(int64_t)row * ea.ldr + col]) +
                           bf16_to_f32(ea.gate[(row / ea.rpg) * ea.gstride + col]) * bf16_to_f32(v));
    return v;
}

// Store of a transposed (TR) 128x64 wave tile: acc[i][j][e] = Y[rbase + 16 i + (l & 15)]
// [cbase + 16 j + 4 (l >> 4) + e]; 4 columns -> one ds_write_b64 into the wave's swizzled LDS
// staging tile, then 16-B global stores of whole 128-B row segments.
template <int EPI = EPI_NONE>
__device__ __forceinline__ void store_tile_t(f32x4 (&acc)[8][4], char* smem, int wave, int lane, int m0, int n0,
                                             int rbase, int cbase, int M, int N, unsigned short* __restrict__ Y,
                                             int64_t ldy, const EpiArgs& ea = EpiArgs{}) {
    constexpr int ROWB = 128, SLOTS = 8;
    char* ctile = smem + wave * (128 * ROWB);
    const int r_l = lane & 15, c_l = (lane >> 4) * 4;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int rr = i * 16 + r_l;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int cc = j * 16 + c_l;
            const int slot = (cc >> 3) ^ (rr & (SLOTS - 1));
            u16x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = f32_to_bf16(acc[i][j][e]);
            *reinterpret_cast<u16x4*>(ctile + rr * ROWB + slot * 16 + (cc & 7) * 2) = o;
        }
    }
    __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): this wave's LDS writes done (wave-private tile)
    constexpr bool E32 = EPI == EPI_RES32 || EPI == EPI_GATED32;
    const bool full = m0 + rbase + 128 <= M && n0 + cbase + 64 <= N && (ldy & 7) == 0 && (((uintptr_t)Y) & 15) == 0;
    const bool epi_vec = EPI == EPI_NONE || EPI == EPI_SILU || EPI == EPI_GELU || EPI == EPI_GELU_ERF ||
                         ((ea.ldr & 7) == 0 && (((uintptr_t)ea.res) & 15) == 0 &&
                          ((EPI != EPI_GATED && EPI != EPI_GATED32) ||
                           ((ea.gstride & 7) == 0 && (((uintptr_t)ea.gate) & 15) == 0)));
    if (full && epi_vec) {  // interior wave tile: all 16 row reads in flight, then 16 unconditional 16-B stores
        u16x8 v[16];
#pragma unroll
        for (int it = 0; it < 16; ++it) {
            const int rr = it * 8 + (lane >> 3), sl = lane & 7;
            v[it] = *reinterpret_cast<const u16x8*>(ctile + rr * ROWB + ((sl ^ (rr & (SLOTS - 1))) << 4));
        }
        const int row0 = m0 + rbase + (lane >> 3), col0 = n0 + cbase + (lane & 7) * 8;
        if constexpr (E32) {
            // the fp32 residual rows (and gates) of 8 row-steps are all loaded before any is stored: one
            // epi_store32 per row-step put every res load behind the previous row-step's stores (the
            // compiler cannot prove they do not alias), i.e. 16 serial HBM round trips per wave
            float* rb = const_cast<float*>(reinterpret_cast<const float*>(ea.res));
            const float* gb = reinterpret_cast<const float*>(ea.gate);
#pragma unroll
            for (int h = 0; h < 16; h += 8) {
                float4 rv[8][2], gv[8][2];
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const int row = row0 + (h + i) * 8;
                    const float* r = rb + (int64_t)row * ea.ldr + col0;
                    rv[i][0] = *reinterpret_cast<const float4*>(r);
                    rv[i][1] = *reinterpret_cast<const float4*>(r + 4);
                    if constexpr (EPI == EPI_GATED32) {
                        const float* g = gb + (int64_t)(row / ea.rpg) * ea.gstride + col0;
                        gv[i][0] = *reinterpret_cast<const float4*>(g);
                        gv[i][1] = *reinterpret_cast<const float4*>(g + 4);
                    }
                }
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const int row = row0 + (h + i) * 8;
                    const u16x8 yv = v[h + i];
                    float x[8] = {rv[i][0].x, rv[i][0].y, rv[i][0].z, rv[i][0].w,
                                  rv[i][1].x, rv[i][1].y, rv[i][1].z, rv[i][1].w};
                    if constexpr (EPI == EPI_GATED32) {
                        const float gg[8] = {gv[i][0].x, gv[i][0].y, gv[i][0].z, gv[i][0].w,
                                             gv[i][1].x, gv[i][1].y, gv[i][1].z, gv[i][1].w};
#pragma unroll
                        for (int u = 0; u < 8; ++u) x[u] = __builtin_fmaf(gg[u], bf16_to_f32(yv[u]), x[u]);
                    } else {
#pragma unroll
                        for (int u = 0; u < 8; ++u) x[u] = x[u] + bf16_to_f32(yv[u]);
                    }
                    float* r = rb + (int64_t)row * ea.ldr + col0;
                    *reinterpret_cast<float4*>(r) = float4{x[0], x[1], x[2], x[3]};
                    *reinterpret_cast<float4*>(r + 4) = float4{x[4], x[5], x[6], x[7]};
                    if (Y) {
                        u16x8 o;
#pragma unroll
                        for (int u = 0; u < 8; ++u) o[u] = f32_to_bf16(x[u]);
                        *reinterpret_cast<u16x8*>(Y + (int64_t)row * ldy + col0) = o;
                    }
                }
            }
            return;
        }
        if constexpr (EPI != EPI_NONE && !E32) {
#pragma unroll
            for (int it = 0; it < 16; ++it) v[it] = epi_apply<EPI>(v[it], row0 + it * 8, col0, ea);
        }
        unsigned short* dst = Y + (int64_t)row0 * ldy + col0;
#pragma unroll
        for (int it = 0; it < 16; ++it) *reinterpret_cast<u16x8*>(dst + (int64_t)it * 8 * ldy) = v[it];
        return;
    }
#pragma unroll
    for (int it = 0; it < 16; ++it) {
        const int rr = it * 8 + (lane >> 3), sl = lane & 7;
        const int row = m0 + rbase + rr;
        const int col = n0 + cbase + sl * 8;
        if (row >= M || col >= N) continue;
        u16x8 v = *reinterpret_cast<const u16x8*>(ctile + rr * ROWB + ((sl ^ (rr & (SLOTS - 1))) << 4));
        if constexpr (E32) {
            if (col + 8 <= N && epi_vec && (ldy & 7) == 0 && (((uintptr_t)Y) & 15) == 0)
                epi_store32<EPI>(v, row, col, ea, Y, ldy);
            else
                for (int u = 0; u < 8 && col + u < N; ++u) epi_store32_1<EPI>(v[u], row, col + u, ea, Y, ldy);
            continue;
        }
        unsigned short* dst = Y + (int64_t)row * ldy + col;
        if (col + 8 <= N && (((uintptr_t)dst) & 15) == 0 && epi_vec) {
            if constexpr (EPI != EPI_NONE) v = epi_apply<EPI>(v, row, col, ea);
            *reinterpret_cast<u16x8*>(dst) = v;
        } else {
            for (int u = 0; u < 8 && col + u < N; ++u) dst[u] = epi_apply1<EPI>(v[u], row, col + u, ea);
        }
    }
}

__device__ __forceinline__ short bf16_bits(float f) { return (short)f32_to_bf16(f); }

// acc[i][j] += L_i . R_j over one 32-deep k-step, which adds bias[n] + scale * T[m,:] . B_k[n,:] to
// every element of the wave's 128x64 tile.  k-slots 0..7 (lanes 0-15 of a fragment) carry the
// tile's first member a = m0 / rows_per_member, slots 8..15 (lanes 16-31) the next member b (a tile
// spans at most two members when rows_per_member >= 256); each row puts its data in its own
// member's block and zeros in the other:
//   L[m] = [Th_q (R) | Tl_q (R) | Th_q (R) | 1 | 0..]      R[n] = [sBh_q | sBh_q | sBl_q | bias | 0..]
// with T = Th + Tl and s*B = sBh + sBl split into bf16 pairs, so the product is
// Th.sBh + Tl.sBh + Th.sBl + bias: fp32-accurate to ~2^-16 relative (the Tl.sBl term is dropped).
template <int R>
__device__ __forceinline__ void lora_mfma_addend(f32x4 (&acc)[8][4], int lane, int m0, int n0, int rbase, int cbase,
                                                 const unsigned short* __restrict__ bias, const float* __restrict__ T,
                                                 const float* __restrict__ theta_pop, int64_t ld_theta, int64_t offB,
                                                 float scale, int rows_per_member, int M, int N) {
    static_assert(3 * R + 1 <= 8, "MFMA epilogue needs 3R+1 <= 8 k-slots per member");
    const int h = lane >> 4, l16 = lane & 15;
    const int ma = m0 / rows_per_member;
    const int last = (m0 + 255 < M ? m0 + 255 : M - 1);
    const bool straddle = last / rows_per_member != ma;
    bf16x8 rf[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        int col = n0 + cbase + j * 16 + l16;
        col = col < N ? col : N - 1;
        short v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (h == 0 || (h == 1 && straddle)) {
            if constexpr (R > 0) {
                const float* Bk = theta_pop + (int64_t)(ma + h) * ld_theta + offB;
#pragma unroll
                for (int q = 0; q < R; ++q) {
                    const float sb = scale * Bk[col * R + q];
                    const short hi = bf16_bits(sb);
                    v[q] = hi;
                    v[R + q] = hi;
                    v[2 * R + q] = bf16_bits(sb - bf16_to_f32((unsigned short)hi));
                }
            }
            v[3 * R] = bias ? (short)bias[col] : (short)0;
        }
        rf[j] = *reinterpret_cast<bf16x8*>(v);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        int row = m0 + rbase + i * 16 + l16;
        row = row < M ? row : M - 1;
        short v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (h == row / rows_per_member - ma) {
            if constexpr (R > 0) {
#pragma unroll
                for (int q = 0; q < R; ++q) {
                    const float t = T[(int64_t)row * R + q];
                    const short th = bf16_bits(t);
                    v[q] = th;
                    v[R + q] = bf16_bits(t - bf16_to_f32((unsigned short)th));
                    v[2 * R + q] = th;
                }
            }
            v[3 * R] = (short)0x3F80;  // 1.0
        }
        const bf16x8 lf = *reinterpret_cast<bf16x8*>(v);
#pragma unroll
        for (int j = 0; j < 4; ++j)  // transposed fragments (TR main loop): D[n][m]
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(rf[j], lf, acc[i][j], 0, 0, 0);
    }
}

}  // namespace eggroll
