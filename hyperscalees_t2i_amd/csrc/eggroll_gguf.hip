// libeggroll — GGUF block dequantisation (gfx950): the load-time path of a GGUF-quantised Z-Image transformer.
//
//   k_gguf_dequant<TYPE, OUT_F32, WIDE> : ggml blocks -> bf16 (RNE) or fp32, one pass, HBM-bound (it writes
//                                         2 or 4 bytes per element and reads 0.26 .. 1.06).
//
// A workgroup of 256 lanes owns 2048 consecutive elements: 64 blocks of the 32-element types, 8 of the
// 256-element K types.  Block strides are 18 .. 210 bytes, so a block is only 2-byte aligned, but a
// workgroup's span starts at a multiple of 8 (or 64) strides = a multiple of 16 bytes from the tensor base:
// the span is staged into LDS with 16-byte loads (2-byte loads for the last < 16 bytes, and for everything
// when the base itself is not 16-byte aligned), never touching a byte past n_blocks * stride, and decoded
// from LDS with byte reads.  Lane t decodes elements 8t .. 8t+7 of the span — always inside one block and one
// scale sub-block, so the fp16 fields and the packed K-type scales are unpacked once per lane — and stores
// them as one 16-byte (bf16) or two 16-byte (fp32) accesses; a wave's stores cover 1 KiB / 2 KiB contiguous.
//
// Arithmetic is the ggml dequantisation expression of each type, every multiply / add / subtract rounded to
// fp32 on its own: floating-point contraction is OFF for this translation unit (hipcc's default would fuse
// d * q - m into one FMA and change the last bit).  fp16 fields widen to fp32 by bit manipulation (exact,
// subnormals included, whatever the denormal mode).
#include "common.h"

#pragma clang fp contract(off)

namespace eggroll {

enum GgmlType {
    GGML_Q4_0 = 2, GGML_Q4_1 = 3, GGML_Q5_0 = 6, GGML_Q5_1 = 7, GGML_Q8_0 = 8,
    GGML_Q2_K = 10, GGML_Q3_K = 11, GGML_Q4_K = 12, GGML_Q5_K = 13, GGML_Q6_K = 14
};

__host__ __device__ constexpr int gguf_block_elems(int t) { return t >= GGML_Q2_K ? 256 : 32; }
__host__ __device__ constexpr int gguf_block_bytes(int t) {
    return t == GGML_Q4_0 ? 18 : t == GGML_Q4_1 ? 20 : t == GGML_Q5_0 ? 22 : t == GGML_Q5_1 ? 24
         : t == GGML_Q8_0 ? 34 : t == GGML_Q2_K ? 84 : t == GGML_Q3_K ? 110 : t == GGML_Q4_K ? 144
         : t == GGML_Q5_K ? 176 : t == GGML_Q6_K ? 210 : 0;
}

constexpr int GQ_THREADS = 256;
constexpr int GQ_SPAN = GQ_THREADS * 8;          // elements per workgroup
constexpr int GQ_LDS = 64 * 34;                  // the largest span: 64 Q8_0 blocks (8 Q6_K blocks: 1680)

__device__ __forceinline__ unsigned short gq_bf16(float f) {
    __bf16 b = (__bf16)f;   // RNE
    return *reinterpret_cast<unsigned short*>(&b);
}

// fp16 bits -> fp32, exact
__device__ __forceinline__ float gq_h2f(uint32_t h) {
    const uint32_t sign = (h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3ffu;
    if (e == 0) return __uint_as_float(sign | __float_as_uint((float)m * 5.9604644775390625e-08f));  // m * 2^-24
    if (e == 31) return __uint_as_float(sign | 0x7f800000u | (m << 13));
    return __uint_as_float(sign | ((e + 112u) << 23) | (m << 13));
}
__device__ __forceinline__ float gq_h2f_at(const uint8_t* p) { return gq_h2f((uint32_t)p[0] | ((uint32_t)p[1] << 8)); }

// the 6-bit (scale, min) pair j of the 12 packed bytes of Q4_K / Q5_K
__device__ __forceinline__ void gq_scale_min_k4(const uint8_t* q, int j, int& sc, int& mn) {
    if (j < 4) {
        sc = q[j] & 63;
        mn = q[j + 4] & 63;
    } else {
        sc = (q[j + 4] & 15) | ((q[j - 4] >> 6) << 4);
        mn = (q[j + 4] >> 4) | ((q[j] >> 6) << 4);
    }
}

// y[0..7] = elements o .. o+7 (o a multiple of 8) of the block at b (LDS)
template <int TYPE>
__device__ __forceinline__ void gq_decode8(const uint8_t* b, int o, float (&y)[8]) {
    if constexpr (TYPE == GGML_Q4_0 || TYPE == GGML_Q4_1) {
        constexpr bool M = TYPE == GGML_Q4_1;
        const float d = gq_h2f_at(b), m = M ? gq_h2f_at(b + 2) : 0.0f;
        const uint8_t* qs = b + (M ? 4 : 2) + (o & 15);
        const int sh = (o >> 4) * 4;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int q = (qs[i] >> sh) & 15;
            y[i] = M ? (float)q * d + m : (float)(q - 8) * d;
        }
    } else if constexpr (TYPE == GGML_Q5_0 || TYPE == GGML_Q5_1) {
        constexpr bool M = TYPE == GGML_Q5_1;
        const float d = gq_h2f_at(b), m = M ? gq_h2f_at(b + 2) : 0.0f;
        const uint8_t* hp = b + (M ? 4 : 2);
        const uint32_t qh = (uint32_t)hp[0] | ((uint32_t)hp[1] << 8) | ((uint32_t)hp[2] << 16) | ((uint32_t)hp[3] << 24);
        const uint8_t* qs = hp + 4 + (o & 15);
        const int sh = (o >> 4) * 4;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int q = ((qs[i] >> sh) & 15) | (int)(((qh >> (o + i)) & 1u) << 4);
            y[i] = M ? (float)q * d + m : (float)(q - 16) * d;
        }
    } else if constexpr (TYPE == GGML_Q8_0) {
        const float d = gq_h2f_at(b);
        const int8_t* qs = reinterpret_cast<const int8_t*>(b + 2 + o);
#pragma unroll
        for (int i = 0; i < 8; ++i) y[i] = (float)qs[i] * d;
    } else if constexpr (TYPE == GGML_Q2_K) {
        const int s = o >> 4, n = s >> 3, k = (s & 7) >> 1, half = s & 1;
        const int sc = b[s];
        const float dl = gq_h2f_at(b + 80) * (float)(sc & 15), ml = gq_h2f_at(b + 82) * (float)(sc >> 4);
        const uint8_t* qs = b + 16 + 32 * n + 16 * half + (o & 15);
#pragma unroll
        for (int i = 0; i < 8; ++i) y[i] = dl * (float)((qs[i] >> (2 * k)) & 3) - ml;
    } else if constexpr (TYPE == GGML_Q3_K) {
        const int s = o >> 4, n = s >> 3, k = (s & 7) >> 1, half = s & 1;
        const uint8_t* scp = b + 96;
        const int low4 = s < 8 ? (scp[s] & 15) : (scp[s - 8] >> 4);
        const int high2 = (scp[8 + (s & 3)] >> (2 * (s >> 2))) & 3;
        const float dl = gq_h2f_at(b + 108) * (float)((low4 | (high2 << 4)) - 32);
        const uint8_t* hm = b + 16 * half + (o & 15);
        const uint8_t* qs = b + 32 + 32 * n + 16 * half + (o & 15);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int q = ((qs[i] >> (2 * k)) & 3) - (((hm[i] >> (s >> 1)) & 1) ? 0 : 4);
            y[i] = dl * (float)q;
        }
    } else if constexpr (TYPE == GGML_Q4_K || TYPE == GGML_Q5_K) {
        constexpr bool H = TYPE == GGML_Q5_K;
        const int j = o >> 5, l = o & 31;
        int sc, mn;
        gq_scale_min_k4(b + 4, j, sc, mn);
        const float dl = gq_h2f_at(b) * (float)sc, ml = gq_h2f_at(b + 2) * (float)mn;
        const uint8_t* qh = b + 16 + l;
        const uint8_t* qs = b + (H ? 48 : 16) + 32 * (j >> 1) + l;
        const int sh = 4 * (j & 1);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            int q = (qs[i] >> sh) & 15;
            if (H) q += ((qh[i] >> j) & 1) << 4;
            y[i] = dl * (float)q - ml;
        }
    } else {  // GGML_Q6_K
        const int n = o >> 7, quarter = (o >> 5) & 3, l = o & 31;
        const int sc = reinterpret_cast<const int8_t*>(b + 192)[o >> 4];
        const float dl = gq_h2f_at(b + 208) * (float)sc;
        const uint8_t* ql = b + 64 * n + 32 * (quarter & 1) + l;
        const uint8_t* qh = b + 128 + 32 * n + l;
        const int sh = 4 * (quarter >> 1);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int q = (((ql[i] >> sh) & 15) | (((qh[i] >> (2 * quarter)) & 3) << 4)) - 32;
            y[i] = dl * (float)q;
        }
    }
}

template <int TYPE, bool OUT_F32, bool WIDE>
__global__ __launch_bounds__(GQ_THREADS) void k_gguf_dequant(const uint8_t* __restrict__ blocks, int64_t n_blocks,
                                                             void* __restrict__ out) {
    constexpr int BE = gguf_block_elems(TYPE), BB = gguf_block_bytes(TYPE), BPW = GQ_SPAN / BE;
    static_assert(BPW * BB <= GQ_LDS && (BPW * BB) % 16 == 0, "span does not fit / is not 16-byte aligned");
    __shared__ __attribute__((aligned(16))) uint8_t lds[GQ_LDS];
    const int t = threadIdx.x;
    const int64_t blk0 = (int64_t)blockIdx.x * BPW;
    const int nb = (int)(n_blocks - blk0 < BPW ? n_blocks - blk0 : BPW);   // >= 1: the grid is ceil(n_blocks / BPW)
    const int bytes = nb * BB;                                              // even; the span is [src, src + bytes)
    const uint8_t* src = blocks + blk0 * BB;
    if constexpr (WIDE) {
        const int full = bytes >> 4;                                        // <= 136 < GQ_THREADS
        if (t < full) reinterpret_cast<uint4*>(lds)[t] = reinterpret_cast<const uint4*>(src)[t];
        const int rest = (bytes & 15) >> 1;                                 // 2-byte pieces after the last full 16
        if (t < rest)
            reinterpret_cast<unsigned short*>(lds)[full * 8 + t] = reinterpret_cast<const unsigned short*>(src)[full * 8 + t];
    } else {
        for (int i = t; i < (bytes >> 1); i += GQ_THREADS)
            reinterpret_cast<unsigned short*>(lds)[i] = reinterpret_cast<const unsigned short*>(src)[i];
    }
    __syncthreads();
    const int e = t * 8;                                                    // first element of this lane in the span
    if (e >= nb * BE) return;
    float y[8];
    gq_decode8<TYPE>(lds + (e / BE) * BB, e % BE, y);
    const int64_t o = blk0 * BE + e;                                        // o + 8 <= n_blocks * BE
    if constexpr (OUT_F32) {
        float4* p = reinterpret_cast<float4*>(reinterpret_cast<float*>(out) + o);
        p[0] = make_float4(y[0], y[1], y[2], y[3]);
        p[1] = make_float4(y[4], y[5], y[6], y[7]);
    } else {
        uint4 v;
        v.x = (uint32_t)gq_bf16(y[0]) | ((uint32_t)gq_bf16(y[1]) << 16);
        v.y = (uint32_t)gq_bf16(y[2]) | ((uint32_t)gq_bf16(y[3]) << 16);
        v.z = (uint32_t)gq_bf16(y[4]) | ((uint32_t)gq_bf16(y[5]) << 16);
        v.w = (uint32_t)gq_bf16(y[6]) | ((uint32_t)gq_bf16(y[7]) << 16);
        *reinterpret_cast<uint4*>(reinterpret_cast<unsigned short*>(out) + o) = v;
    }
}

template <int TYPE>
static void gq_launch(const void* blocks, int64_t n_blocks, void* out, bool f32, bool wide, hipStream_t s) {
    constexpr int BPW = GQ_SPAN / gguf_block_elems(TYPE);
    const dim3 grid((unsigned)((n_blocks + BPW - 1) / BPW)), block(GQ_THREADS);
    const uint8_t* b = static_cast<const uint8_t*>(blocks);
    if (f32) {
        if (wide) hipLaunchKernelGGL((k_gguf_dequant<TYPE, true, true>), grid, block, 0, s, b, n_blocks, out);
        else hipLaunchKernelGGL((k_gguf_dequant<TYPE, true, false>), grid, block, 0, s, b, n_blocks, out);
    } else {
        if (wide) hipLaunchKernelGGL((k_gguf_dequant<TYPE, false, true>), grid, block, 0, s, b, n_blocks, out);
        else hipLaunchKernelGGL((k_gguf_dequant<TYPE, false, false>), grid, block, 0, s, b, n_blocks, out);
    }
}

}  // namespace eggroll

using namespace eggroll;

extern "C" int eggroll_gguf_dequant(int32_t ggml_type, const void* blocks, int64_t n_elems, void* out, int32_t out_fp32,
                                    void* stream) {
    const int bb = gguf_block_bytes(ggml_type);
    EGG_CHECK_ARG(bb != 0, "gguf_dequant: ggml type %d unsupported (Q4_0 2, Q4_1 3, Q5_0 6, Q5_1 7, Q8_0 8, Q2_K 10, "
                  "Q3_K 11, Q4_K 12, Q5_K 13, Q6_K 14)", (int)ggml_type);
    const int be = gguf_block_elems(ggml_type);
    EGG_CHECK_ARG(n_elems >= 0 && n_elems % be == 0, "gguf_dequant: n_elems=%lld is not a non-negative multiple of the "
                  "block size %d", (long long)n_elems, be);
    EGG_CHECK_ARG(n_elems <= (1ll << 31), "gguf_dequant: n_elems=%lld above 2^31", (long long)n_elems);
    EGG_CHECK_ARG(out_fp32 == 0 || out_fp32 == 1, "gguf_dequant: out_fp32 must be 0 or 1");
    if (n_elems == 0) return EGGROLL_OK;
    EGG_CHECK_ARG(blocks && out, "gguf_dequant: NULL pointer");
    EGG_CHECK_ARG(((uintptr_t)blocks & 1) == 0 && ((uintptr_t)out & 15) == 0,
                  "gguf_dequant: blocks must be 2-byte aligned and out 16-byte aligned");
    const int64_t nb = n_elems / be;
    const bool wide = ((uintptr_t)blocks & 15) == 0, f32 = out_fp32 != 0;
    hipStream_t s = as_stream(stream);
    switch (ggml_type) {
        case GGML_Q4_0: gq_launch<GGML_Q4_0>(blocks, nb, out, f32, wide, s); break;
        case GGML_Q4_1: gq_launch<GGML_Q4_1>(blocks, nb, out, f32, wide, s); break;
        case GGML_Q5_0: gq_launch<GGML_Q5_0>(blocks, nb, out, f32, wide, s); break;
        case GGML_Q5_1: gq_launch<GGML_Q5_1>(blocks, nb, out, f32, wide, s); break;
        case GGML_Q8_0: gq_launch<GGML_Q8_0>(blocks, nb, out, f32, wide, s); break;
        case GGML_Q2_K: gq_launch<GGML_Q2_K>(blocks, nb, out, f32, wide, s); break;
        case GGML_Q3_K: gq_launch<GGML_Q3_K>(blocks, nb, out, f32, wide, s); break;
        case GGML_Q4_K: gq_launch<GGML_Q4_K>(blocks, nb, out, f32, wide, s); break;
        case GGML_Q5_K: gq_launch<GGML_Q5_K>(blocks, nb, out, f32, wide, s); break;
        default: gq_launch<GGML_Q6_K>(blocks, nb, out, f32, wide, s); break;
    }
    EGG_CHECK_LAUNCH("gguf_dequant");
    return EGGROLL_OK;
}
