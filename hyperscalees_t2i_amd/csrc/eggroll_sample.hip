// libeggroll — token sampling (gfx950):
//
//   k_sample_topk_topp : CFG combine, top-k, top-p and the multinomial draw of one row of logits per workgroup
//                        (VAR's sample_with_top_k_top_p_, VAR_models/helpers.py:6-19, restated)
//   k_sample_bits      : the same chain over two classes per bit, closed forms, plus the BSQ codes of the drawn bits
//                        (Infinity's per-scale tail: CFG, tau, top-k / top-p, multinomial, bits_to_codes)
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

// ------------------------------------------------------------------------------------
// Infinity's bit sampling.  Every bit is a row of two logits, so both selections are closed forms and a bit needs
// nothing but its own two (cond, uncond) pairs and its two draws: one thread per bit, pure streaming.  A workgroup
// takes kBitsTok consecutive tokens of one image and walks their d_tok bits in passes of kBitsChunk; within a pass
// consecutive threads take consecutive bits of a token, then the next token, so the pair loads (4 or 8 bytes per
// lane), the q loads and the int64 bit stores of a wave are contiguous runs.  The codes are the transpose
// [token][bit] -> [channel][pixel]: the pass's +-code_mag values go through LDS (row stride kBitsChunk + 1, odd,
// so the transposed read is conflict free) and leave as runs over the tile's tokens (2 floats per token with
// spatial patchify, where a token's bits 4c + 2dy + dx are channel c of the 2 x 2 pixels of pixel_shuffle).
// No atomics, no cross-workgroup traffic: a bit's result depends on that bit's inputs alone.
// ------------------------------------------------------------------------------------
constexpr int kBitsThreads = 256;
constexpr int kBitsTok = 64;                 // tokens per workgroup
constexpr int kBitsChunk = 64;               // bits of a token per pass
constexpr int kBitsStageLd = kBitsChunk + 1;

// fl(fl(wc fl(c it)) + fl(wu fl(u it))): torch's `lg / tau` (on the GPU a multiplication by it = float(1.0 / tau)) and
// `cfg * lg[:, 0] + (1 - cfg) * lg[:, 1]`, each operation rounded on its own
__device__ __forceinline__ float cfg_tau_combine(float wc, float c, float wu, float u, float it) {
#pragma clang fp contract(off)
    const float a = c * it, b = u * it;
    const float pa = wc * a, pb = wu * b;
    return pa + pb;
}

template <bool BF16>
__device__ __forceinline__ void load_pair(const void* __restrict__ head, int64_t off, float& a, float& b) {
    if (BF16) {
        const uint32_t v = *reinterpret_cast<const uint32_t*>((const unsigned short*)head + off);
        a = __uint_as_float(v << 16), b = __uint_as_float(v & 0xFFFF0000u);
    } else {
        a = ((const float*)head)[off], b = ((const float*)head)[off + 1];
    }
}

template <bool BF16>
__global__ __launch_bounds__(kBitsThreads) void k_sample_bits(
    const void* __restrict__ head, int64_t ld, int B, int L, int w, int d_tok, int tiles, float inv_tau, float w_cond,
    float w_uncond, int top_k, float p_cut, const float* __restrict__ q, int64_t* __restrict__ bits,
    float* __restrict__ codes, int patchify, float code_mag, float* __restrict__ x_out, int32_t* __restrict__ bad) {
    __shared__ float stage[kBitsTok * kBitsStageLd];
    const int tid = threadIdx.x;
    const int64_t img = blockIdx.x / tiles;                      // member * B + image
    const int t0 = (int)(blockIdx.x % tiles) * kBitsTok;
    const int nt = min(kBitsTok, L - t0);
    const int64_t mem = img / B, j = img % B;
    const int64_t row_c = (mem * 2 * B + j) * L + t0;            // the cond row of token t0; uncond is B * L rows on
    const int64_t row_u = row_c + (int64_t)B * L;
    const int64_t qbit0 = (j * L + t0) * d_tok;                  // bit index of (t0, 0) in q
    const int64_t obit0 = (img * L + t0) * d_tok;                // ... in bits and x_out

    for (int i0 = 0; i0 < d_tok; i0 += kBitsChunk) {
        const int dc = min(kBitsChunk, d_tok - i0);
        for (int e = tid; e < nt * dc; e += kBitsThreads) {
            const int tt = e / dc, ii = e - tt * dc, i = i0 + ii;
            float c0, c1, u0, u1;
            load_pair<BF16>(head, (row_c + tt) * ld + 2 * i, c0, c1);
            load_pair<BF16>(head, (row_u + tt) * ld + 2 * i, u0, u1);
            const float x0 = cfg_tau_combine(w_cond, c0, w_uncond, u0, inv_tau);
            const float x1 = cfg_tau_combine(w_cond, c1, w_uncond, u1, inv_tau);
            const int64_t ob = obit0 + (int64_t)tt * d_tok + i;
            const float pinf = __uint_as_float(0x7F800000u);
            // NaN, +inf or nothing finite: -1, a zero code, the flag, and nothing else
            if (x0 != x0 || x1 != x1 || x0 == pinf || x1 == pinf || (x0 == -pinf && x1 == -pinf)) {
                bits[ob] = -1;
                stage[tt * kBitsStageLd + ii] = 0.f;
                *bad = 1;
                continue;
            }
            if (x_out) x_out[2 * ob] = x0, x_out[2 * ob + 1] = x1;
            const float2 qv = *reinterpret_cast<const float2*>(q + 2 * (qbit0 + (int64_t)tt * d_tok + i));
            const bool hi1 = x1 > x0;
            const bool tie = x0 == x1;           // a tie group of two is never masked: drawn by q alone
            const float e_lo = tie ? 1.f : expf(hi1 ? x0 - x1 : x1 - x0), Z = 1.f + e_lo;
            // the smaller of two: top_k == 1 masks it (0 or >= 2 masks nothing), top-p when its share is <= p_cut
            const bool masked = !tie && (top_k == 1 || (p_cut >= 0.f && e_lo / Z <= p_cut));
            int bit = hi1 ? 1 : 0;
            if (!masked) {                       // argmax p'_c / q_c, the lower index on a tie
                const float w0 = ((hi1 ? e_lo : 1.f) / Z) / qv.x, w1 = ((hi1 ? 1.f : e_lo) / Z) / qv.y;
                bit = w1 > w0 ? 1 : 0;
            }
            bits[ob] = bit;
            stage[tt * kBitsStageLd + ii] = bit ? code_mag : -code_mag;
        }
        __syncthreads();
        if (!patchify) {                         // channel i, pixel t: runs of nt floats
            float* dst = codes + (img * d_tok + i0) * L + t0;
            for (int f = tid; f < dc * nt; f += kBitsThreads) {
                const int ii = f / nt, tt = f - ii * nt;
                dst[(int64_t)ii * L + tt] = stage[tt * kBitsStageLd + ii];
            }
        } else {                                 // channel c, pixel (2y + dy, 2x + dx): runs of 2 floats per token
            const int W2 = 2 * w, H2 = 2 * (L / w);
            float* dst = codes + (img * (d_tok / 4) + i0 / 4) * H2 * W2;
            for (int f = tid; f < dc * nt; f += kBitsThreads) {
                const int dx = f & 1, g = f >> 1;
                const int r = g / nt, tt = g - r * nt;           // r = 2 c + dy
                const int t = t0 + tt, y = t / w, x = t - y * w;
                dst[((int64_t)(r >> 1) * H2 + 2 * y + (r & 1)) * W2 + 2 * x + dx] =
                    stage[tt * kBitsStageLd + 2 * r + dx];
            }
        }
        __syncthreads();
    }
}

extern "C" int eggroll_sample_bits(const void* head, int32_t in_bf16, int64_t ld, int64_t n, int64_t B, int64_t h,
                                   int64_t w, int64_t d_tok, float inv_tau, float w_cond, float w_uncond,
                                   int32_t top_k, float p_cut, const float* q, int64_t* bits, float* codes,
                                   int32_t patchify, float code_mag, float* x_out, int32_t* bad, void* stream) {
    EGG_CHECK_ARG(in_bf16 == 0 || in_bf16 == 1, "sample_bits: in_bf16 must be 0 or 1 (got %d)", in_bf16);
    EGG_CHECK_ARG(d_tok >= 1, "sample_bits: d_tok=%lld must be >= 1", (long long)d_tok);
    EGG_CHECK_ARG((patchify == 0 || patchify == 1) && (patchify == 0 || d_tok % 4 == 0),
                  "sample_bits: patchify must be 0 or 1, and d_tok a multiple of 4 with it (got patchify=%d d_tok=%lld)",
                  patchify, (long long)d_tok);
    EGG_CHECK_ARG(ld % 2 == 0 && ld / 2 >= d_tok, "sample_bits: ld=%lld must be even and >= 2 * d_tok = 2 * %lld",
                  (long long)ld, (long long)d_tok);
    EGG_CHECK_ARG(n >= 0 && B >= 0 && h >= 0 && w >= 0, "sample_bits: negative size n=%lld B=%lld h=%lld w=%lld",
                  (long long)n, (long long)B, (long long)h, (long long)w);
    int64_t total = (n == 0 || B == 0 || h == 0 || w == 0) ? 0 : 1;     // the bits of the call
    for (const int64_t f : {n, B, h, w, d_tok}) {
        EGG_CHECK_ARG(total == 0 || total <= ((1ll << 31) - 1) / f,
                      "sample_bits: n * B * h * w * d_tok must be below 2^31 (n=%lld B=%lld h=%lld w=%lld d_tok=%lld)",
                      (long long)n, (long long)B, (long long)h, (long long)w, (long long)d_tok);
        total *= f;
    }
    EGG_CHECK_ARG(top_k >= 0 && p_cut == p_cut, "sample_bits: top_k must be >= 0 and p_cut not NaN");
    EGG_CHECK_ARG(((uintptr_t)head & 3) == 0 && ((uintptr_t)q & 7) == 0 && ((uintptr_t)bits & 7) == 0 &&
                      ((uintptr_t)codes & 3) == 0 && ((uintptr_t)x_out & 3) == 0 && ((uintptr_t)bad & 3) == 0,
                  "sample_bits: head / codes / x_out / bad must be 4-byte aligned, q / bits 8-byte");
    if (total == 0) return EGGROLL_OK;
    EGG_CHECK_ARG(head && q && bits && codes && bad, "sample_bits: NULL pointer");
    const int64_t L = h * w;
    const int tiles = (int)((L + kBitsTok - 1) / kBitsTok);
    const dim3 grid((unsigned)(n * B * tiles)), block(kBitsThreads);
    if (in_bf16)
        hipLaunchKernelGGL(k_sample_bits<true>, grid, block, 0, as_stream(stream), head, ld, (int)B, (int)L, (int)w,
                           (int)d_tok, tiles, inv_tau, w_cond, w_uncond, (int)top_k, p_cut, q, bits, codes,
                           (int)patchify, code_mag, x_out, bad);
    else
        hipLaunchKernelGGL(k_sample_bits<false>, grid, block, 0, as_stream(stream), head, ld, (int)B, (int)L, (int)w,
                           (int)d_tok, tiles, inv_tau, w_cond, w_uncond, (int)top_k, p_cut, q, bits, codes,
                           (int)patchify, code_mag, x_out, bad);
    EGG_CHECK_LAUNCH("sample_bits");
    return EGGROLL_OK;
}
