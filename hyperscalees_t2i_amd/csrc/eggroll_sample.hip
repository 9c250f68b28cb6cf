// libeggroll — token sampling (gfx950):
//
//   k_sample_topk_topp : CFG combine, top-k, top-p and the multinomial draw of one row of logits per workgroup
//                        (VAR's sample_with_top_k_top_p_, VAR_models/helpers.py:6-19, restated)
#include "common.h"

using namespace eggroll;

// ------------------------------------------------------------------------------------
// One workgroup of 256 threads per row of V <= 4096 logits; the row lives in registers, 16 values per thread
// (thread t holds the 4-element chunks t, t + 256, t + 512, t + 768), as its order-preserving integer key
// (key(a) < key(b) <=> a < b over every non-NaN float) and its softmax numerator.  Both selections are a
// bitwise search for a threshold key, one workgroup reduction per bit:
//   top-k : the largest T with  #{key >= T} >= k           = the k-th largest value, counted with multiplicity
//   top-p : the largest T with  sum{p_i : key_i <= T} <= p_cut ; everything <= T but the row maximum is masked
// The sum of a fixed reduction tree is monotone in each non-negative term, so the second predicate is monotone
// in T as the first is, and equal logits (one key) are kept or dropped together.  Every reduction is that fixed
// tree (the thread's 16 values in order, the xor butterfly of the wave, the four waves in order): a row's result
// depends on the row alone and is the same in every launch.  No atomics, no cross-workgroup traffic.
// ------------------------------------------------------------------------------------
constexpr int kSampleThreads = 256;
constexpr int kSampleChunks = 4;                       // 4-element chunks per thread: 256 * 4 * 4 = 4096 values
constexpr uint32_t kKeyPosInf = 0xFF800000u;           // key(+inf); anything above is a positive NaN
constexpr uint32_t kKeyNegInf = 0x007FFFFFu;           // key(-inf); anything below is a negative NaN

__device__ __forceinline__ uint32_t f2key(float f) {
    const uint32_t b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key2f(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

// fl(fl(wc c) - fl(wu u)): the products are rounded before the subtraction (contraction into an FMA is off here)
__device__ __forceinline__ float cfg_combine(float wc, float c, float wu, float u) {
#pragma clang fp contract(off)
    const float a = wc * c, b = wu * u;
    return a - b;
}

struct OpAdd {
    template <class T> __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
};
struct OpMax {
    template <class T> __device__ __forceinline__ T operator()(T a, T b) const { return a > b ? a : b; }
};

// The reduction of v over the workgroup, returned to every thread (bitwise the same in each: the butterfly's
// operands commute, the waves' partials are combined in one order).  `red` is 2 x 4 eight-byte slots used in
// turn (`round` counts the calls), so one barrier per call is enough: a slot is rewritten two calls later, past
// the next call's barrier, which every reader of this call has reached by then.
template <class T, class Op>
__device__ __forceinline__ T block_all(T v, Op op, unsigned long long* red, int& round) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
    T* slot = reinterpret_cast<T*>(red + 4 * (round & 1));
    ++round;
    if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
    __syncthreads();
    return op(op(slot[0], slot[1]), op(slot[2], slot[3]));
}

template <bool BF16>
__global__ __launch_bounds__(kSampleThreads) void k_sample_topk_topp(
    const void* __restrict__ cond, const void* __restrict__ uncond, int64_t ld, int64_t rpb, int64_t block_ld,
    float w_cond, float w_uncond, int V, int top_k, float p_cut, const float* __restrict__ q, int64_t ldq,
    int64_t* __restrict__ idx, float* __restrict__ x_out, int64_t ldx) {
    __shared__ unsigned long long red[8];
    int round = 0;
    const int64_t r = blockIdx.x;
    const int64_t off = (r / rpb) * block_ld + (r % rpb) * ld;
    const int tid = threadIdx.x;

    // ---- CFG combine: x = fl(fl(w_cond c) - fl(w_uncond u)), the two products rounded on their own ----
    uint32_t key[4 * kSampleChunks];
    uint32_t kmax = 0;
    bool bad = false;
#pragma unroll
    for (int i = 0; i < kSampleChunks; ++i) {
        const int col = (i * kSampleThreads + tid) * 4;
        float c[4] = {0.f, 0.f, 0.f, 0.f}, u[4] = {0.f, 0.f, 0.f, 0.f};
        const bool live = col < V;
        if (live) {
            if (BF16) {
                const ushort4 cv = *reinterpret_cast<const ushort4*>((const unsigned short*)cond + off + col);
                c[0] = __uint_as_float((uint32_t)cv.x << 16), c[1] = __uint_as_float((uint32_t)cv.y << 16);
                c[2] = __uint_as_float((uint32_t)cv.z << 16), c[3] = __uint_as_float((uint32_t)cv.w << 16);
                if (uncond) {
                    const ushort4 uv = *reinterpret_cast<const ushort4*>((const unsigned short*)uncond + off + col);
                    u[0] = __uint_as_float((uint32_t)uv.x << 16), u[1] = __uint_as_float((uint32_t)uv.y << 16);
                    u[2] = __uint_as_float((uint32_t)uv.z << 16), u[3] = __uint_as_float((uint32_t)uv.w << 16);
                }
            } else {
                const float4 cv = *reinterpret_cast<const float4*>((const float*)cond + off + col);
                c[0] = cv.x, c[1] = cv.y, c[2] = cv.z, c[3] = cv.w;
                if (uncond) {
                    const float4 uv = *reinterpret_cast<const float4*>((const float*)uncond + off + col);
                    u[0] = uv.x, u[1] = uv.y, u[2] = uv.z, u[3] = uv.w;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float x = uncond ? cfg_combine(w_cond, c[j], w_uncond, u[j]) : c[j];
            const uint32_t k = live ? f2key(x) : 0u;   // 0 is below every key of a good row: a dead slot is never chosen
            key[4 * i + j] = k;
            kmax = k > kmax ? k : kmax;
            bad |= live && (k >= kKeyPosInf || k < kKeyNegInf);
        }
    }
    // one reduction for both: the high word says whether any thread saw NaN or +inf, the low word is the row maximum
    const unsigned long long top = block_all(((unsigned long long)bad << 32) | kmax, OpMax{}, red, round);
    kmax = (uint32_t)top;
    if ((top >> 32) != 0 || kmax <= kKeyNegInf) {   // NaN, +inf, or nothing finite: -1 and nothing else
        if (tid == 0) idx[r] = -1;
        return;
    }
    if (x_out) {
#pragma unroll
        for (int i = 0; i < kSampleChunks; ++i) {
            const int col = (i * kSampleThreads + tid) * 4;
            if (col < V)
                *reinterpret_cast<float4*>(x_out + r * ldx + col) =
                    make_float4(key2f(key[4 * i]), key2f(key[4 * i + 1]), key2f(key[4 * i + 2]), key2f(key[4 * i + 3]));
        }
    }

    // ---- top-k: kth = the top_k-th largest key; keys below it are masked, ties at it stay ----
    uint32_t kth = 0;
    if (top_k > 0 && top_k < V) {
#pragma unroll 1
        for (int b = 31; b >= 0; --b) {
            const uint32_t cand = kth | (1u << b);
            int n = 0;
#pragma unroll
            for (int i = 0; i < 4 * kSampleChunks; ++i) n += key[i] >= cand ? 1 : 0;
            if (block_all(n, OpAdd{}, red, round) >= top_k) kth = cand;
        }
    }
    // softmax numerators of what is unmasked (0: masked, a dead slot, or an input of -inf)
    const float xmax = key2f(kmax);
    float e[4 * kSampleChunks], s = 0.f;
#pragma unroll
    for (int i = 0; i < 4 * kSampleChunks; ++i) {
        e[i] = (key[i] >= kth && key[i] != 0u) ? expf(key2f(key[i]) - xmax) : 0.f;
        s += e[i];
    }
    float Z = block_all(s, OpAdd{}, red, round);

    // ---- top-p: mask j when C(x_j) = sum{p_i : x_i <= x_j} <= p_cut and x_j is below the row maximum ----
    if (p_cut >= 0.f) {
        float p[4 * kSampleChunks];
#pragma unroll
        for (int i = 0; i < 4 * kSampleChunks; ++i) p[i] = e[i] / Z;
        uint32_t cut = 0;   // C(0) = 0 <= p_cut: no live key is 0
#pragma unroll 1
        for (int b = 31; b >= 0; --b) {
            const uint32_t cand = cut | (1u << b);
            float c = 0.f;
#pragma unroll
            for (int i = 0; i < 4 * kSampleChunks; ++i) c += key[i] <= cand ? p[i] : 0.f;
            if (block_all(c, OpAdd{}, red, round) <= p_cut) cut = cand;
        }
        s = 0.f;
#pragma unroll
        for (int i = 0; i < 4 * kSampleChunks; ++i) {
            if (key[i] <= cut && key[i] < kmax) e[i] = 0.f;
            s += e[i];
        }
        Z = block_all(s, OpAdd{}, red, round);
    }

    // ---- draw: the lowest index of argmax p'_j / q_j, p' the softmax over what is left ----
    unsigned long long best = 0;
#pragma unroll
    for (int i = 0; i < kSampleChunks; ++i) {
        const int col = (i * kSampleThreads + tid) * 4;
        if (col < V) {
            const float4 qv = *reinterpret_cast<const float4*>(q + r * ldq + col);
            const float qq[4] = {qv.x, qv.y, qv.z, qv.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float w = e[4 * i + j] > 0.f ? (e[4 * i + j] / Z) / qq[j] : 0.f;
                // w >= 0: its bits order as the values do; the complemented index makes the lower one win a tie
                const unsigned long long cnd =
                    ((unsigned long long)__float_as_uint(w) << 32) | (uint32_t)(0xFFFFFFFFu - (uint32_t)(col + j));
                best = cnd > best ? cnd : best;
            }
        }
    }
    best = block_all(best, OpMax{}, red, round);
    if (tid == 0) idx[r] = (int64_t)(0xFFFFFFFFu - (uint32_t)best);
}

extern "C" int eggroll_sample_topk_topp(const void* cond, const void* uncond, int32_t in_bf16, int64_t ld,
                                        int64_t rows_per_block, int64_t block_ld, float w_cond, float w_uncond,
                                        int64_t R, int64_t V, int32_t top_k, float p_cut, const float* q, int64_t ldq,
                                        int64_t* idx, float* x_out, int64_t ldx, void* stream) {
    EGG_CHECK_ARG(in_bf16 == 0 || in_bf16 == 1, "sample_topk_topp: in_bf16 must be 0 or 1 (got %d)", in_bf16);
    EGG_CHECK_ARG(V >= 2 && V <= 4 * kSampleChunks * kSampleThreads && V % 4 == 0,
                  "sample_topk_topp: V=%lld outside the class (a multiple of 4 in [2, 4096])", (long long)V);
    EGG_CHECK_ARG(R >= 0 && R < (1ll << 31) && rows_per_block >= 1 && block_ld >= 0,
                  "sample_topk_topp: bad sizes R=%lld rows_per_block=%lld block_ld=%lld", (long long)R,
                  (long long)rows_per_block, (long long)block_ld);
    EGG_CHECK_ARG(ld >= V && ldq >= V && (!x_out || ldx >= V), "sample_topk_topp: ld / ldq / ldx must be >= V");
    EGG_CHECK_ARG(ld % 4 == 0 && block_ld % 4 == 0 && ldq % 4 == 0 && (!x_out || ldx % 4 == 0),
                  "sample_topk_topp: ld, block_ld, ldq and ldx must be multiples of 4");
    EGG_CHECK_ARG(top_k >= 0 && p_cut == p_cut, "sample_topk_topp: top_k must be >= 0 and p_cut not NaN");
    const uintptr_t in_mask = in_bf16 ? 7 : 15;
    EGG_CHECK_ARG(((uintptr_t)cond & in_mask) == 0 && ((uintptr_t)uncond & in_mask) == 0 && ((uintptr_t)q & 15) == 0 &&
                      ((uintptr_t)x_out & 15) == 0 && ((uintptr_t)idx & 7) == 0,
                  "sample_topk_topp: cond / uncond must be %d-byte aligned, q / x_out 16-byte, idx 8-byte",
                  (int)in_mask + 1);
    if (R == 0) return EGGROLL_OK;
    EGG_CHECK_ARG(cond && q && idx, "sample_topk_topp: NULL pointer");
    const dim3 grid((unsigned)R), block(kSampleThreads);
    if (in_bf16)
        hipLaunchKernelGGL(k_sample_topk_topp<true>, grid, block, 0, as_stream(stream), cond, uncond, ld, rows_per_block,
                           block_ld, w_cond, w_uncond, (int)V, (int)top_k, p_cut, q, ldq, idx, x_out, ldx);
    else
        hipLaunchKernelGGL(k_sample_topk_topp<false>, grid, block, 0, as_stream(stream), cond, uncond, ld, rows_per_block,
                           block_ld, w_cond, w_uncond, (int)V, (int)top_k, p_cut, q, ldq, idx, x_out, ldx);
    EGG_CHECK_LAUNCH("sample_topk_topp");
    return EGGROLL_OK;
}
