// libeggroll — softmax attention on MFMA (gfx950).
//
//   k_cross_attn, k_cross_attn_h2 : a short key sequence staged whole in LDS (Sana attn2, the CLIP towers,
//                  Infinity's text cross-attention); two-pass, or online softmax over two key halves
//   k_flash_attn : head dim 128 or 64, any key count, no mask (Z-Image self-attention; Infinity and VAR over
//                  their KV caches)
//   k_seq_attn   : the prompt encoders' self-attention (T5 relative bias, Gemma-2 soft-cap, Qwen3 causal)
#include "frag.h"

using namespace eggroll;

// ------------------------------------------------------------------------------------
// Softmax cross-attention over a short key sequence (Sana attn2: 300 caption tokens, head dim 112),
// diffusers SanaAttnProcessor2_0 / F.scaled_dot_product_attention(q, k, v, attn_mask=bias, scale):
//   o[b, n, h, :] = softmax_j(scale * q[b,n,h,:] . k[u,j,h,:] + bias[u, j]) @ v[u, :, h, :],
//   u = enc_index[b] (the image's caption row: images of one prompt share k / v).
// One workgroup per (image, head): the caption's k and v ([L <= 320][112] bf16 each) are staged in
// LDS once and the 8 waves sweep the image's queries in blocks of 16.  Per block, on MFMA
// 16x16x32 bf16 with fp32 accumulation:
//   S^T = K Q^T   A = k rows (16 keys x 32 dims, 16-B LDS reads), B = q rows (16-B global reads);
//                 the C layout leaves each lane 4 consecutive keys of ONE query, so the softmax max /
//                 sum per query reduce over the lane's registers and the 4 lane groups (xor 16, 32);
//   O^T = V^T P^T B = exp(S^T - max) packed straight from the C registers: lane group g holds keys
//                 4g..4g+3 of each 16-key fragment, so a 32-key k-step uses the key order
//                 {4g..4g+3, 16+4g..16+4g+3} per group — A (V^T) reads exactly that order from the
//                 key-major V tile with ds_read_tr16_b64 (no data movement for P);
//   o = O / rowsum, written as 4 consecutive dims of one query per lane (8-B stores) in the q layout.
// Keys past L are excluded (-inf); the additive bias is the reference's attention mask.
// ------------------------------------------------------------------------------------
#ifndef EGG_XA_PREFETCH
#define EGG_XA_PREFETCH 1
#endif
constexpr int XA_LMAX = 320;          // keys per (caption, head) staged in LDS
constexpr int XA_LMAX_128 = 256;      // the same at head dim 128 (2 x 256 x 136 x 2 B of k / v)

template <int RS>
__device__ __forceinline__ la_bf16x8 xa_tr8_perm(const unsigned short* base, int lane) {
    // rows base + 4g + {0..3} and base + 16 + 4g + {0..3} of the 16-lane group g (lane 4q+p: row q, columns 4p..)
    const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
    const unsigned short* r0 = base + (4 * g + q) * RS + 4 * p;
    const la_s4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((la_lds_s4*)(r0));
    const la_s4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((la_lds_s4*)(r0 + 16 * RS));
    typedef __attribute__((ext_vector_type(8))) short s8;
    const s8 f = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(la_bf16x8, f);
}

// k / v rows of caption u, head h -> LDS (row stride HD + 8), rows >= L zero.  Every load of the thread
// is issued before the first store: the strided loop this replaces waited for each 16-B pair in turn (one
// memory latency per trip, ~9 trips with one workgroup per CU and nothing to overlap them).
template <int HD, int LM, int NT>
__device__ __forceinline__ void xa_stage_kv(const unsigned short* __restrict__ k, const unsigned short* __restrict__ v,
                                            int64_t ldkv, int u, int h, int L, int tid, unsigned short* sk,
                                            unsigned short* sv) {
    constexpr int RS = HD + 8, CH = HD / 8, NCH = LM * CH, IT = (NCH + NT - 1) / NT;
    u16x8m kr[IT], vr[IT];
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int c = tid + it * NT, r = c / CH, cc = c - r * CH;
        kr[it] = vr[it] = u16x8m{0, 0, 0, 0, 0, 0, 0, 0};
        if (c < NCH && r < L) {
            const int64_t off = ((int64_t)u * L + r) * ldkv + (int64_t)h * HD + cc * 8;
            kr[it] = *reinterpret_cast<const u16x8m*>(k + off);
            vr[it] = *reinterpret_cast<const u16x8m*>(v + off);
        }
    }
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int c = tid + it * NT, r = c / CH, cc = c - r * CH;
        if (NCH % NT == 0 || c < NCH) {
            *reinterpret_cast<u16x8m*>(sk + r * RS + cc * 8) = kr[it];
            *reinterpret_cast<u16x8m*>(sv + r * RS + cc * 8) = vr[it];
        }
    }
}

template <int HD, int NWAVE, int QF, int LM = XA_LMAX>
__global__ __launch_bounds__(64 * NWAVE) void k_cross_attn(const unsigned short* __restrict__ q, int64_t ldq,
                                                    const unsigned short* __restrict__ k,
                                                    const unsigned short* __restrict__ v, int64_t ldkv,
                                                    const unsigned short* __restrict__ bias,
                                                    const int* __restrict__ enc_index, int heads, int N, int L,
                                                    int U, float scale, unsigned short* __restrict__ o, int64_t ldo) {
    // NWAVE waves sweep the image's queries in blocks of 16 * QF (QF query fragments share every k / v
    // fragment read from LDS)
    constexpr int RS = HD + 8, KSN = (HD + 31) / 32, DF = HD / 16;  // LDS row stride, Q.K k-steps, PV dim frags
    static_assert(HD % 16 == 0 && HD <= 128 && LM % 32 == 0, "head dim / key capacity");
    __shared__ __attribute__((aligned(16))) unsigned short sk[LM * RS];
    __shared__ __attribute__((aligned(16))) unsigned short sv[LM * RS];
    __shared__ float sb[LM];
    constexpr int NT = 64 * NWAVE;
    const int bh = xcd_remap(blockIdx.x, gridDim.x);
    const int b = bh / heads, h = bh - b * heads;
    const int u_in = enc_index ? enc_index[b] : b;
    const bool u_bad = u_in < 0 || u_in >= U;  // out-of-range caption row: NaN output, no out-of-bounds read
    const int u = u_bad ? 0 : u_in;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r16 = lane & 15, g = lane >> 4;
    // stage k / v rows of caption u, head h: HD / 8 chunks of 16 B per row; rows >= L are zeros
    xa_stage_kv<HD, LM, NT>(k, v, ldkv, u, h, L, tid, sk, sv);
    for (int r = tid; r < LM; r += NT)
        sb[r] = u_bad ? __builtin_nanf("") : r < L ? (bias ? b2f(bias[(int64_t)u * L + r]) : 0.0f) : -INFINITY;
    __syncthreads();
    const int nkf = (L + 15) / 16, nkb = (L + 31) / 32;  // key fragments / 32-key PV steps in use
    const int nqb = (N + 16 * QF - 1) / (16 * QF);
    // B = Q^T fragments for the 4 k-steps (dims 32ks + 8g .. +7; dims >= 112 are zero).  EGG_XA_PREFETCH:
    // the next block's q fragments are loaded right after this block's S^T MFMAs are issued, so their
    // global-load latency runs under the softmax and PV instead of opening the next block.
    auto load_q = [&](int qb_, la_bf16x8 (&dst)[QF][KSN]) {
#pragma unroll
        for (int x = 0; x < QF; ++x) {
            const int qrow = qb_ * 16 * QF + 16 * x + r16;
#pragma unroll
            for (int ks = 0; ks < KSN; ++ks) {
                const int d0 = 32 * ks + 8 * g;
                u16x8m t = u16x8m{0, 0, 0, 0, 0, 0, 0, 0};
                if (d0 < HD && qrow < N)
                    t = *reinterpret_cast<const u16x8m*>(q + ((int64_t)b * N + qrow) * ldq + (int64_t)h * HD + d0);
                dst[x][ks] = __builtin_bit_cast(la_bf16x8, t);
            }
        }
    };
    la_bf16x8 bq[QF][KSN], bqn[QF][KSN];
    if (EGG_XA_PREFETCH && w < nqb) load_q(w, bqn);
    for (int qb = w; qb < nqb; qb += NWAVE) {
        if (EGG_XA_PREFETCH) {
#pragma unroll
            for (int x = 0; x < QF; ++x)
#pragma unroll
                for (int ks = 0; ks < KSN; ++ks) bq[x][ks] = bqn[x][ks];
        } else {
            load_q(qb, bq);
        }
        // S^T[key][query] for every key fragment
        la_f32x4 sf[QF][(LM / 16)];
        float mx[QF];
#pragma unroll
        for (int x = 0; x < QF; ++x) mx[x] = -INFINITY;
#pragma unroll
        for (int f = 0; f < (LM / 16); ++f) {
#pragma unroll
            for (int x = 0; x < QF; ++x) sf[x][f] = la_f32x4{0.f, 0.f, 0.f, 0.f};
            if (f < nkf) {
#pragma unroll
                for (int ks = 0; ks < KSN; ++ks) {
                    const int d0 = 32 * ks + 8 * g;
                    la_bf16x8 a;
                    if (d0 < HD) a = *reinterpret_cast<const la_bf16x8*>(sk + (16 * f + r16) * RS + d0);
                    else a = la_bf16x8{};
#pragma unroll
                    for (int x = 0; x < QF; ++x) sf[x][f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bq[x][ks], sf[x][f], 0, 0, 0);
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float bb = sb[16 * f + 4 * g + e];
#pragma unroll
                    for (int x = 0; x < QF; ++x) {
                        const float sv_ = sf[x][f][e] * scale + bb;
                        sf[x][f][e] = sv_;
                        mx[x] = fmaxf(mx[x], sv_);
                    }
                }
            }
        }
        if (EGG_XA_PREFETCH && qb + NWAVE < nqb) load_q(qb + NWAVE, bqn);
        float sum[QF];
#pragma unroll
        for (int x = 0; x < QF; ++x) {
            mx[x] = g4_max(mx[x]);
            sum[x] = 0.0f;
        }
#pragma unroll
        for (int f = 0; f < (LM / 16); ++f) {
            if (f < nkf) {
#pragma unroll
                for (int x = 0; x < QF; ++x)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float pe = __expf(sf[x][f][e] - mx[x]);
                        sf[x][f][e] = pe;
                        sum[x] += pe;
                    }
            }
        }
#pragma unroll
        for (int x = 0; x < QF; ++x) {
            sum[x] = g4_sum(sum[x]);
        }
        // O^T[dim][query] = sum_keys V^T[dim][key] P^T[key][query]
        la_f32x4 oc[QF][DF];
#pragma unroll
        for (int x = 0; x < QF; ++x)
#pragma unroll
            for (int d = 0; d < DF; ++d) oc[x][d] = la_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < (LM / 16) / 2; ++j) {
            if (j < nkb) {
                la_bf16x8 bp[QF];
#pragma unroll
                for (int x = 0; x < QF; ++x)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        bp[x][e] = (__bf16)sf[x][2 * j][e];
                        bp[x][4 + e] = (__bf16)sf[x][2 * j + 1][e];
                    }
#pragma unroll
                for (int d = 0; d < DF; ++d) {
                    const la_bf16x8 av = xa_tr8_perm<RS>(sv + (32 * j) * RS + 16 * d, lane);
#pragma unroll
                    for (int x = 0; x < QF; ++x) oc[x][d] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, bp[x], oc[x][d], 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int x = 0; x < QF; ++x) {
            const int qrow = qb * 16 * QF + 16 * x + r16;
            if (qrow < N) {
                const float inv = 1.0f / sum[x];
                unsigned short* dst = o + ((int64_t)b * N + qrow) * ldo + (int64_t)h * HD + 4 * g;
#pragma unroll
                for (int d = 0; d < DF; ++d) {
                    u16x4m t;
#pragma unroll
                    for (int e = 0; e < 4; ++e) t[e] = f2b(oc[x][d][e] * inv);
                    *reinterpret_cast<u16x4m*>(dst + 16 * d) = t;
                }
            }
        }
    }
}

// Round 5: 32 queries per wave block (QF = 2 query fragments share every k / v fragment read from LDS:
// half the LDS bytes per query, the bound of the 16-query form), with the softmax taken online over two
// key halves so that only half the scores are live in registers (S for 2 x LM/2 keys: the QF = 2
// two-pass form needed 160 score registers and fell to 1 wave per SIMD).  After the first half
// (max m0, P0 = exp(S0 - m0), O = V0^T P0), the second rescales O and the running row sums by
// exp(m0 - m1) before adding its own keys — exact softmax up to fp32 rounding.
template <int HD, int NWAVE, int LM>
__global__ __launch_bounds__(64 * NWAVE) void k_cross_attn_h2(const unsigned short* __restrict__ q, int64_t ldq,
                                                       const unsigned short* __restrict__ k,
                                                       const unsigned short* __restrict__ v, int64_t ldkv,
                                                       const unsigned short* __restrict__ bias,
                                                       const int* __restrict__ enc_index, int heads, int N, int L,
                                                       int U, float scale, unsigned short* __restrict__ o, int64_t ldo) {
    constexpr int QF = 2;
    constexpr int RS = HD + 8, KSN = (HD + 31) / 32, DF = HD / 16;
    constexpr int FH = LM / 32;  // key fragments (of 16) per half
    static_assert(HD % 16 == 0 && HD <= 128 && LM % 64 == 0, "head dim / key capacity");
    __shared__ __attribute__((aligned(16))) unsigned short sk[LM * RS];
    __shared__ __attribute__((aligned(16))) unsigned short sv[LM * RS];
    __shared__ float sb[LM];
    constexpr int NT = 64 * NWAVE;
    const int bh = xcd_remap(blockIdx.x, gridDim.x);
    const int b = bh / heads, h = bh - b * heads;
    const int u_in = enc_index ? enc_index[b] : b;
    const bool u_bad = u_in < 0 || u_in >= U;  // out-of-range caption row: NaN output, no out-of-bounds read
    const int u = u_bad ? 0 : u_in;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r16 = lane & 15, g = lane >> 4;
    xa_stage_kv<HD, LM, NT>(k, v, ldkv, u, h, L, tid, sk, sv);
    for (int r = tid; r < LM; r += NT)
        sb[r] = u_bad ? __builtin_nanf("") : r < L ? (bias ? b2f(bias[(int64_t)u * L + r]) : 0.0f) : -INFINITY;
    __syncthreads();
    const int nkf = (L + 15) / 16, nkb = (L + 31) / 32;
    const int nqb = (N + 16 * QF - 1) / (16 * QF);
    auto load_q = [&](int qb_, la_bf16x8 (&dst)[QF][KSN]) {
#pragma unroll
        for (int x = 0; x < QF; ++x) {
            const int qrow = qb_ * 16 * QF + 16 * x + r16;
#pragma unroll
            for (int ks = 0; ks < KSN; ++ks) {
                const int d0 = 32 * ks + 8 * g;
                u16x8m t = u16x8m{0, 0, 0, 0, 0, 0, 0, 0};
                if (d0 < HD && qrow < N)
                    t = *reinterpret_cast<const u16x8m*>(q + ((int64_t)b * N + qrow) * ldq + (int64_t)h * HD + d0);
                dst[x][ks] = __builtin_bit_cast(la_bf16x8, t);
            }
        }
    };
    // the next block's q fragments are loaded right after this block's first-half S^T MFMAs are issued
    // (their latency runs under the softmax and PV: EGG_XA_PREFETCH)
    la_bf16x8 bq[QF][KSN], bqn[QF][KSN];
    if (w < nqb) load_q(w, bqn);
#pragma unroll 1
    for (int qb = w; qb < nqb; qb += NWAVE) {
#pragma unroll
        for (int x = 0; x < QF; ++x)
#pragma unroll
            for (int ks = 0; ks < KSN; ++ks) bq[x][ks] = bqn[x][ks];
        float mx[QF], sum[QF];
        la_f32x4 oc[QF][DF];
#pragma unroll
        for (int x = 0; x < QF; ++x) {
            mx[x] = -INFINITY;
            sum[x] = 0.0f;
#pragma unroll
            for (int d = 0; d < DF; ++d) oc[x][d] = la_f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const int f0 = half * FH;
            if (f0 >= nkf) break;  // uniform: L <= LM / 2 keys
            la_f32x4 sf[QF][FH];
            float lm[QF];
#pragma unroll
            for (int x = 0; x < QF; ++x) lm[x] = -INFINITY;
#pragma unroll
            for (int f = 0; f < FH; ++f) {
#pragma unroll
                for (int x = 0; x < QF; ++x) sf[x][f] = la_f32x4{0.f, 0.f, 0.f, 0.f};
                if (f0 + f < nkf) {
#pragma unroll
                    for (int ks = 0; ks < KSN; ++ks) {
                        const int d0 = 32 * ks + 8 * g;
                        la_bf16x8 a;
                        if (d0 < HD) a = *reinterpret_cast<const la_bf16x8*>(sk + (16 * (f0 + f) + r16) * RS + d0);
                        else a = la_bf16x8{};
#pragma unroll
                        for (int x = 0; x < QF; ++x) sf[x][f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bq[x][ks], sf[x][f], 0, 0, 0);
                    }
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float bb = sb[16 * (f0 + f) + 4 * g + e];
#pragma unroll
                        for (int x = 0; x < QF; ++x) {
                            const float sv_ = sf[x][f][e] * scale + bb;
                            sf[x][f][e] = sv_;
                            lm[x] = fmaxf(lm[x], sv_);
                        }
                    }
                }
            }
            if (half == 0 && qb + NWAVE < nqb) load_q(qb + NWAVE, bqn);
            float alpha[QF];
#pragma unroll
            for (int x = 0; x < QF; ++x) {
                lm[x] = g4_max(lm[x]);
                const float mn = fmaxf(mx[x], lm[x]);
                alpha[x] = half == 0 ? 0.0f : __expf(mx[x] - mn);
                mx[x] = mn;
            }
            if (half > 0) {
#pragma unroll
                for (int x = 0; x < QF; ++x) {
                    sum[x] *= alpha[x];
#pragma unroll
                    for (int d = 0; d < DF; ++d)
#pragma unroll
                        for (int e = 0; e < 4; ++e) oc[x][d][e] *= alpha[x];
                }
            }
#pragma unroll
            for (int f = 0; f < FH; ++f) {
                if (f0 + f < nkf) {
#pragma unroll
                    for (int x = 0; x < QF; ++x)
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const float pe = __expf(sf[x][f][e] - mx[x]);
                            sf[x][f][e] = pe;
                            sum[x] += pe;
                        }
                }
            }
#pragma unroll
            for (int j = 0; j < FH / 2; ++j) {
                const int jj = half * (FH / 2) + j;
                if (jj < nkb) {
                    la_bf16x8 bp[QF];
#pragma unroll
                    for (int x = 0; x < QF; ++x)
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            bp[x][e] = (__bf16)sf[x][2 * j][e];
                            bp[x][4 + e] = (__bf16)sf[x][2 * j + 1][e];
                        }
#pragma unroll
                    for (int d = 0; d < DF; ++d) {
                        const la_bf16x8 av = xa_tr8_perm<RS>(sv + (32 * jj) * RS + 16 * d, lane);
#pragma unroll
                        for (int x = 0; x < QF; ++x) oc[x][d] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, bp[x], oc[x][d], 0, 0, 0);
                    }
                }
            }
        }
#pragma unroll
        for (int x = 0; x < QF; ++x) {
            sum[x] = g4_sum(sum[x]);
            const int qrow = qb * 16 * QF + 16 * x + r16;
            if (qrow < N) {
                const float inv = 1.0f / sum[x];
                unsigned short* dst = o + ((int64_t)b * N + qrow) * ldo + (int64_t)h * HD + 4 * g;
#pragma unroll
                for (int d = 0; d < DF; ++d) {
                    u16x4m t;
#pragma unroll
                    for (int e = 0; e < 4; ++e) t[e] = f2b(oc[x][d][e] * inv);
                    *reinterpret_cast<u16x4m*>(dst + 16 * d) = t;
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------
// Flash attention, head dim HD = 128 (Z-Image self-attention; Infinity's cosine attention over the KV cache)
// or 64 (VAR's L2-normalised attention over its KV cache):
//   o[b, n, h, :] = softmax_j(scale * q[b,n,h,:] . k[b,j,h,:]) @ v[b, :, h, :],  j < Lk, no mask.
// q / k / v / o: [B][rows][heads * HD] bf16 views with their own batch and row strides (a KV cache
// [B][ltot][C] is read in place).  Workgroup = (b, h, 64 QF-query block), 4 waves x 16 QF queries; keys in
// blocks of 64 staged in LDS (k and v [64][RS] bf16), the next block held in registers while this one
// computes.  Key rows >= Lk are never read (the last key's row is read in their place and zeroed), so a cache
// slice of uninitialised memory behind Lk is harmless.  Per key block and wave, MFMA 16x16x32 bf16, fp32 accumulation, the k_cross_attn layout:
//   S^T = K Q^T   (Q^T fragments stay in registers for the whole key sweep; each lane: 4 keys of ONE query)
//   online softmax in base 2: m' = max(m, rowmax), O *= 2^(m - m'), P = 2^(S - m'), per-lane partial row
//                 sums rescaled the same way and reduced over the 4 lane groups once at the end
//   O^T += V^T P^T  (P^T packed from the C registers, V^T read with ds_read_tr16_b64 in the matching key order)
// ------------------------------------------------------------------------------------
// LDS row stride 144 bf16 = 288 B = 72 dwords: consecutive rows start 8 banks apart, so the S^T k reads
// (ds_read_b128, lane groups {0-3,12-15,20-27}...: 8 rows x 2 chunks) and the V^T reads (ds_read_b64_tr_b16,
// 32-lane groups: 8 rows x 32 B) both cover 64 distinct banks; the first form's 136 (4 banks apart) left
// 38 % of the LDS cycles to bank conflicts (PMC SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE)
// Head dim 64: row stride 72 bf16 = 36 dwords (k_seq_attn<SA_RELBIAS>'s, measured there), rows 4 banks apart:
// the 4 chunks x 16 rows of a k read and the 8 rows x 32 B of a V^T read each cover 64 distinct banks.  k + v of
// a block are 18 KB and the qf 2 instance holds 32 accumulator registers, so 4 / 3 / 2 workgroups per CU at
// qf 1 / 2 / 4 (128 / 168 / 256 VGPRs) against 3 / 2 / 1 at head dim 128.
constexpr int FA_HD = 128, FA_KB = 64, FA_RS = FA_HD + 16, FA_RS64 = 64 + 8;
typedef float fa_f32x2 __attribute__((ext_vector_type(2)));

template <int HD, int RS, int QF, int MINB>
__global__ __launch_bounds__(256, MINB) void k_flash_attn(const unsigned short* __restrict__ q, int64_t q_bs, int64_t ldq,
                                                    const unsigned short* __restrict__ k, int64_t k_bs, int64_t ldk,
                                                    const unsigned short* __restrict__ v, int64_t v_bs, int64_t ldv,
                                                    int heads, int Nq, int Lk, int nqb, float scale_log2,
                                                    unsigned short* __restrict__ o, int64_t o_bs, int64_t ldo) {
    constexpr int QW = 16 * QF, KSN = HD / 32, DF = HD / 16, KF = FA_KB / 16, CH = HD / 8;
    constexpr int UNITS = 2 * FA_KB * CH / 256;   // 16-B chunks of k + v per thread per key block (8 at head dim 128, 4 at 64)
    __shared__ __attribute__((aligned(16))) unsigned short sk[FA_KB * RS];
    __shared__ __attribute__((aligned(16))) unsigned short sv[FA_KB * RS];
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    const int qb = bid % nqb, bh = bid / nqb;
    const int b = bh / heads, h = bh - b * heads;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r16 = lane & 15, g = lane >> 4;
    const unsigned short* kb_ = k + (int64_t)b * k_bs + (int64_t)h * HD;
    const unsigned short* vb_ = v + (int64_t)b * v_bs + (int64_t)h * HD;
    // Q^T fragments (B operand): dims 32 ks + 8 g .. +7 of query 16 x + r16 of this wave's 32
    la_bf16x8 bq[QF][KSN];
    const int q0 = qb * (4 * QW) + w * QW;
#pragma unroll
    for (int x = 0; x < QF; ++x) {
        const int qr = q0 + 16 * x + r16;
#pragma unroll
        for (int ks = 0; ks < KSN; ++ks) {
            u16x8m t = u16x8m{0, 0, 0, 0, 0, 0, 0, 0};
            if (qr < Nq)
                t = *reinterpret_cast<const u16x8m*>(q + (int64_t)b * q_bs + (int64_t)qr * ldq + (int64_t)h * HD +
                                                     32 * ks + 8 * g);
            bq[x][ks] = __builtin_bit_cast(la_bf16x8, t);
        }
    }
    u16x8m pre[UNITS];
    auto load_blk = [&](int key0) {
#pragma unroll
        for (int i = 0; i < UNITS; ++i) {
            const int c = tid + 256 * i;             // [k | v][row][chunk]
            const int kv = c / (FA_KB * CH), rc = c - kv * (FA_KB * CH);
            const int r = rc / CH, cc = rc - r * CH;
            // branch-free: rows past Lk read the last key (in bounds) and are zeroed by a select
            const int row = min(key0 + r, Lk - 1);
            const unsigned short* src = kv ? vb_ + (int64_t)row * ldv : kb_ + (int64_t)row * ldk;
            const u16x8m t = *reinterpret_cast<const u16x8m*>(src + cc * 8);
            pre[i] = key0 + r < Lk ? t : u16x8m{0, 0, 0, 0, 0, 0, 0, 0};
        }
    };
    auto store_blk = [&]() {
#pragma unroll
        for (int i = 0; i < UNITS; ++i) {
            const int c = tid + 256 * i;
            const int kv = c / (FA_KB * CH), rc = c - kv * (FA_KB * CH);
            const int r = rc / CH, cc = rc - r * CH;
            *reinterpret_cast<u16x8m*>((kv ? sv : sk) + r * RS + cc * 8) = pre[i];
        }
    };
    la_f32x4 oc[QF][DF];
    float m[QF], l[QF];
#pragma unroll
    for (int x = 0; x < QF; ++x) {
        m[x] = -INFINITY;
        l[x] = 0.0f;
#pragma unroll
        for (int d = 0; d < DF; ++d) oc[x][d] = la_f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const int nkb = (Lk + FA_KB - 1) / FA_KB;
    load_blk(0);
    for (int kb = 0; kb < nkb; ++kb) {
        __syncthreads();   // every wave is done reading the previous block
        store_blk();
        __syncthreads();
        if (kb + 1 < nkb) load_blk((kb + 1) * FA_KB);   // in flight under this block's MFMAs
        la_f32x4 sf[QF][KF];
        // k-step outer, key fragment inner: 4 x QF independent accumulations between two dependent MFMAs
        // (f outer put each chain's next MFMA right behind it: PMC issue stalls ~35 % of wave cycles)
#pragma unroll
        for (int ks = 0; ks < KSN; ++ks) {
#pragma unroll
            for (int f = 0; f < KF; ++f) {
                const la_bf16x8 a = *reinterpret_cast<const la_bf16x8*>(sk + (16 * f + r16) * RS + 32 * ks + 8 * g);
                // the first k-step takes a literal zero accumulator (no per-block zeroing of 32 registers)
#pragma unroll
                for (int x = 0; x < QF; ++x)
                    sf[x][f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bq[x][ks], ks ? sf[x][f] : la_f32x4{0.f, 0.f, 0.f, 0.f},
                                                                       0, 0, 0);
            }
        }
        const int key0 = kb * FA_KB;
        // the VALU side is the bound here (PMC: ~6 VALU instructions per MFMA), so the softmax runs on
        // raw scores: max of raw S (scale > 0 commutes with max), then p = 2^(s * scale_log2 - m) as one
        // packed FMA per pair + exp2; O is rescaled only when some lane's running max moved
        if (key0 + FA_KB > Lk) {   // the partial last block: keys >= Lk -> -inf (uniform branch)
#pragma unroll
            for (int f = 0; f < KF; ++f)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const bool ok = key0 + 16 * f + 4 * g + e < Lk;
#pragma unroll
                    for (int x = 0; x < QF; ++x) sf[x][f][e] = ok ? sf[x][f][e] : -INFINITY;
                }
        }
#pragma unroll
        for (int x = 0; x < QF; ++x) {
            float mb = fmaxf(fmaxf(sf[x][0][0], sf[x][0][1]), fmaxf(sf[x][0][2], sf[x][0][3]));
#pragma unroll
            for (int f = 1; f < KF; ++f)
                mb = fmaxf(fmaxf(mb, fmaxf(sf[x][f][0], sf[x][f][1])), fmaxf(sf[x][f][2], sf[x][f][3]));
            mb = g4_max(mb);
            const float mn = fmaxf(m[x], mb * scale_log2);
            if (__builtin_amdgcn_ballot_w64(mn != m[x])) {   // a running max moved: rescale this query set
                const float alpha = __builtin_amdgcn_exp2f(m[x] - mn);   // 0 on the first block (m = -inf)
                l[x] *= alpha;
#pragma unroll
                for (int d = 0; d < DF; ++d)
#pragma unroll
                    for (int e = 0; e < 4; ++e) oc[x][d][e] *= alpha;
                m[x] = mn;
            }
            const fa_f32x2 sc2 = {scale_log2, scale_log2}, nm2 = {-mn, -mn};
            fa_f32x2 acc2 = {0.f, 0.f};
#pragma unroll
            for (int f = 0; f < KF; ++f)
#pragma unroll
                for (int e = 0; e < 4; e += 2) {
                    fa_f32x2 t = (fa_f32x2){sf[x][f][e], sf[x][f][e + 1]} * sc2 + nm2;
                    t.x = __builtin_amdgcn_exp2f(t.x);
                    t.y = __builtin_amdgcn_exp2f(t.y);
                    sf[x][f][e] = t.x;
                    sf[x][f][e + 1] = t.y;
                    acc2 = acc2 + t;
                }
            l[x] += acc2.x + acc2.y;
        }
#pragma unroll
        for (int j = 0; j < KF / 2; ++j) {
            la_bf16x8 bp[QF];
#pragma unroll
            for (int x = 0; x < QF; ++x)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    bp[x][e] = (__bf16)sf[x][2 * j][e];
                    bp[x][4 + e] = (__bf16)sf[x][2 * j + 1][e];
                }
#pragma unroll
            for (int d = 0; d < DF; ++d) {
                const la_bf16x8 av = xa_tr8_perm<RS>(sv + (32 * j) * RS + 16 * d, lane);
#pragma unroll
                for (int x = 0; x < QF; ++x) oc[x][d] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, bp[x], oc[x][d], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int x = 0; x < QF; ++x) {
        float sum = l[x];
        sum = g4_sum(sum);
        const int qr = q0 + 16 * x + r16;
        if (qr < Nq) {
            const float inv = 1.0f / sum;
            unsigned short* dst = o + (int64_t)b * o_bs + (int64_t)qr * ldo + (int64_t)h * HD + 4 * g;
#pragma unroll
            for (int d = 0; d < DF; ++d) {
                u16x4m t;
#pragma unroll
                for (int e = 0; e < 4; ++e) t[e] = f2b(oc[x][d][e] * inv);
                *reinterpret_cast<u16x4m*>(dst + 16 * d) = t;
            }
        }
    }
}

// ------------------------------------------------------------------------------------
// Self-attention of the prompt encoders: per-sequence key lengths, q / k / v read in place from one fused
// qkv GEMM output.  One kernel template, three instances:
//   o[b, i, h, :] = softmax_{j in keys(b, i)}(t(q[b,i,h,:] . k[b,j,hk,:])) @ v[b, j, hk, :]
// q / k / v / o: rows b*N + i of bf16 matrices with their own row strides, head h at columns HD h.
//
// The sweep is k_flash_attn's: workgroup = (b, query head, 64 QF-query block) under xcd_remap, 4 waves x QF
// sets of 16 queries; keys in blocks of KB staged in LDS (k and v [KB][RS] bf16) with the next block held in
// registers while this one computes.  Per key block and wave, MFMA 16x16x32 bf16 with fp32 accumulation:
//   S^T = K Q^T   (Q^T fragments stay in registers for the whole sweep; each lane: 4 keys of ONE query)
//   online softmax in base 2: m' = max(m, rowmax), O *= 2^(m - m') only when some lane's max moved,
//                 P = 2^(t - m'), per-lane partial row sums reduced over the 4 lane groups once at the end
//   O^T += V^T P^T  (P^T packed to bf16 from the C registers, V^T through ds_read_tr16_b64 in that key order)
// Only the blocks holding keys < len[b] are swept; keys >= len[b] inside the last one take -inf, and key rows
// are read clamped to len[b] - 1, so nothing past row N - 1 of a sequence is touched.  Key 0 is visible to
// every query of a swept block and block 0 is swept first, so every running max is finite after block 0:
// a later block with no visible key gives rowmax = -inf, m' = m, and exp2(m - m') never sees -inf - -inf.
// A query block with no query < len[b] writes zeros and leaves before any barrier; every other branch around
// a barrier is block-uniform.  Query rows >= len[b] are written as zeros.
//
// SA_RELBIAS <64, 64, 1, 72> (the T5 encoder): keys(b, i) = {j < len[b]}, hk = h,
//   t = scale * s + rel_bias[h][j - i + R-1].  The head's bias row sits in LDS as sb[d + 511], d = key - query
//   (pre-multiplied by log2 e; zero where |d| >= N, which only padded queries / masked keys reach): one
//   subtraction per score, and no clamp for any key / query of a 64-padded N <= 512 (index in [0, 1022]).
// SA_SOFTCAP <256, 32, 1, 264> (Gemma-2, Sana): keys(b, i) = {j <= i, j < len[b]}, hk = h / G with
//   G = heads_q / heads_kv, t = cap > 0 ? cap * tanh(scale * s / cap) : scale * s.  The soft-cap is evaluated
//   in fp32 before the mask as tanh(x) = 1 - 2 / (exp2(2 x log2 e) + 1), which saturates to +-1 without a NaN.
//   Per lane 32 VGPRs of Q fragments, 64 of output accumulators, 32 of prefetch; k + v of a 32-key block are
//   2 x 32 x 264 x 2 B = 33 KB of LDS.  No table over N lives in LDS, so N has no upper limit.
// SA_CAUSAL <128, 64, 2, 144> (Qwen3, Z-Image): keys and hk as SA_SOFTCAP, t = scale * s; k_flash_attn<2>'s
//   tile and LDS row stride.  The softmax runs on raw scores: max of raw S (scale > 0 commutes with max), then
//   p = 2^(s * scale_log2 - m') as one packed FMA per pair.  The G workgroups of one KV head have adjacent ids
//   under xcd_remap, so their K / V reads meet in one XCD's L2.
// In the two causal modes a query block sweeps the key blocks that hold a key < min(len[b], its last query +
// 1); a wave skips the arithmetic of a block wholly past its 16 QF queries (after the block's barriers); the
// j <= i / j < len selects run only in blocks that reach past the wave's first query or past len[b]
// (wave-uniform branch).
// ------------------------------------------------------------------------------------
enum { SA_RELBIAS = 0, SA_SOFTCAP = 1, SA_CAUSAL = 2 };
constexpr int RB_NMAX = 512;

template <int MODE, int HD, int KB, int QF, int RS, int MINB>
__global__ __launch_bounds__(256, MINB) void k_seq_attn(const unsigned short* __restrict__ q, int64_t ldq,
                                                        const unsigned short* __restrict__ k, int64_t ldk,
                                                        const unsigned short* __restrict__ v, int64_t ldv,
                                                        const float* __restrict__ rel_bias, int R,
                                                        const int* __restrict__ lens, int heads_q, int group, int N,
                                                        int nqb, float scale_log2, float cap_in, float cap_log2,
                                                        unsigned short* __restrict__ o, int64_t ldo) {
    constexpr bool CAUSAL = MODE != SA_RELBIAS;
    constexpr int QW = 16 * QF, QB = 4 * QW, KSN = HD / 32, DF = HD / 16, KF = KB / 16, CH = HD / 8;
    constexpr int UNITS = 2 * KB * CH / 256;   // 16-B chunks of k + v per thread per key block
    __shared__ __attribute__((aligned(16))) unsigned short sk[KB * RS];
    __shared__ __attribute__((aligned(16))) unsigned short sv[KB * RS];
    __shared__ float sb[MODE == SA_RELBIAS ? 2 * RB_NMAX : 1];   // SA_RELBIAS only: unused, so no LDS, elsewhere
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    const int qb = bid % nqb, bh = bid / nqb;
    const int b = bh / heads_q, h = bh - b * heads_q, hk = MODE == SA_RELBIAS ? h : h / group;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r16 = lane & 15, g = lane >> 4;
    const int L = min(max(lens[b], 0), N);
    const int64_t row0 = (int64_t)b * N;
    if (qb * QB >= L) {   // no valid query in this block (block-uniform): zeros, before any barrier
#pragma unroll
        for (int i = 0; i < QB * (HD / 4) / 256; ++i) {
            const int c = tid + 256 * i, r = c / (HD / 4), cc = c - r * (HD / 4);
            if (qb * QB + r < N)
                *reinterpret_cast<u16x4m*>(o + (row0 + qb * QB + r) * ldo + (int64_t)h * HD + 4 * cc) =
                    u16x4m{0, 0, 0, 0};
        }
        return;
    }
    if constexpr (MODE == SA_RELBIAS) {
        for (int t = tid; t < 2 * RB_NMAX; t += 256) {
            const int d = t - (RB_NMAX - 1);
            sb[t] = (d > -N && d < N) ? rel_bias[(int64_t)h * (2 * R - 1) + d + (R - 1)] * 1.4426950408889634f : 0.0f;
        }
    }
    const unsigned short* kb_ = k + row0 * ldk + (int64_t)hk * HD;
    const unsigned short* vb_ = v + row0 * ldv + (int64_t)hk * HD;
    // Q^T fragments (B operand): dims 32 ks + 8 g .. +7 of query 16 x + r16 of this wave's QW
    const int q0 = qb * QB + w * QW;
    la_bf16x8 bq[QF][KSN];
#pragma unroll
    for (int x = 0; x < QF; ++x) {
        const int qr = q0 + 16 * x + r16;
#pragma unroll
        for (int ks = 0; ks < KSN; ++ks) {
            u16x8m t = u16x8m{0, 0, 0, 0, 0, 0, 0, 0};
            if (qr < N) t = *reinterpret_cast<const u16x8m*>(q + (row0 + qr) * ldq + (int64_t)h * HD + 32 * ks + 8 * g);
            bq[x][ks] = __builtin_bit_cast(la_bf16x8, t);
        }
    }
    u16x8m pre[UNITS];
    auto load_blk = [&](int key0) {
#pragma unroll
        for (int i = 0; i < UNITS; ++i) {
            const int c = tid + 256 * i;             // [k | v][row][chunk]
            const int kv = c / (KB * CH), rc = c - kv * (KB * CH);
            const int r = rc / CH, cc = rc - r * CH;
            // branch-free: rows past L read the last valid key (in bounds) and are zeroed by a select
            const int row = min(key0 + r, L - 1);
            const unsigned short* src = kv ? vb_ + (int64_t)row * ldv : kb_ + (int64_t)row * ldk;
            const u16x8m t = *reinterpret_cast<const u16x8m*>(src + cc * 8);
            pre[i] = key0 + r < L ? t : u16x8m{0, 0, 0, 0, 0, 0, 0, 0};
        }
    };
    auto store_blk = [&]() {
#pragma unroll
        for (int i = 0; i < UNITS; ++i) {
            const int c = tid + 256 * i;
            const int kv = c / (KB * CH), rc = c - kv * (KB * CH);
            const int r = rc / CH, cc = rc - r * CH;
            *reinterpret_cast<u16x8m*>((kv ? sv : sk) + r * RS + cc * 8) = pre[i];
        }
    };
    la_f32x4 oc[QF][DF];
    float m[QF], l[QF];
#pragma unroll
    for (int x = 0; x < QF; ++x) {
        m[x] = -INFINITY;
        l[x] = 0.0f;
#pragma unroll
        for (int d = 0; d < DF; ++d) oc[x][d] = la_f32x4{0.f, 0.f, 0.f, 0.f};
    }
    // keys [0, kend): below len, and in the causal modes up to the block's last query
    const int kend = CAUSAL ? min(L, qb * QB + QB) : L;
    const int nkb = (kend + KB - 1) / KB;
    load_blk(0);
    for (int kb = 0; kb < nkb; ++kb) {
        __syncthreads();   // every wave is done reading the previous block (SA_RELBIAS, first trip: sb is being written)
        store_blk();
        __syncthreads();
        if (kb + 1 < nkb) load_blk((kb + 1) * KB);   // in flight under this block's MFMAs
        const int key0 = kb * KB;
        if (CAUSAL && key0 > q0 + QW - 1) continue;   // wholly past this wave's queries (wave-uniform; barriers are above)
        la_f32x4 sf[QF][KF];
#pragma unroll
        for (int ks = 0; ks < KSN; ++ks) {
#pragma unroll
            for (int f = 0; f < KF; ++f) {
                const la_bf16x8 a = *reinterpret_cast<const la_bf16x8*>(sk + (16 * f + r16) * RS + 32 * ks + 8 * g);
#pragma unroll
                for (int x = 0; x < QF; ++x)
                    sf[x][f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bq[x][ks], ks ? sf[x][f] : la_f32x4{0.f, 0.f, 0.f, 0.f},
                                                                       0, 0, 0);
            }
        }
        // the score transform; lane: keys key0 + 16 f + 4 g + e of query q0 + 16 x + r16
        if constexpr (MODE == SA_RELBIAS) {
            // t = log2 e * (scale * s + bias[key - query]); key <= 511 and query <= 511 (64-padded N <= 512), so
            // the index lies in [0, 1022]
#pragma unroll
            for (int x = 0; x < QF; ++x) {
                const float* bl = sb + (key0 + 4 * g - (q0 + 16 * x + r16) + (RB_NMAX - 1));
#pragma unroll
                for (int f = 0; f < KF; ++f)
#pragma unroll
                    for (int e = 0; e < 4; ++e) sf[x][f][e] = fmaf(sf[x][f][e], scale_log2, bl[16 * f + e]);
            }
        } else if constexpr (MODE == SA_SOFTCAP) {
            // t = log2 e * softcap(scale * s)
            if (cap_log2 > 0.0f) {   // cap_in = 2 log2 e * scale / cap, cap_log2 = log2 e * cap
#pragma unroll
                for (int x = 0; x < QF; ++x)
#pragma unroll
                    for (int f = 0; f < KF; ++f)
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const float ex = __builtin_amdgcn_exp2f(sf[x][f][e] * cap_in);   // +inf / 0 at the ends: tanh = +-1
                            sf[x][f][e] = fmaf(-2.0f * cap_log2, __builtin_amdgcn_rcpf(ex + 1.0f), cap_log2);
                        }
            } else {
#pragma unroll
                for (int x = 0; x < QF; ++x)
#pragma unroll
                    for (int f = 0; f < KF; ++f)
#pragma unroll
                        for (int e = 0; e < 4; ++e) sf[x][f][e] *= scale_log2;
            }
        }   // SA_CAUSAL: none, the scale is folded into the exp below
        // the partial last block, and in the causal modes the diagonal (wave-uniform branch)
        if (key0 + KB > L || (CAUSAL && key0 + KB - 1 > q0)) {
#pragma unroll
            for (int f = 0; f < KF; ++f)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int key = key0 + 16 * f + 4 * g + e;
#pragma unroll
                    for (int x = 0; x < QF; ++x)
                        sf[x][f][e] = (key < L && (!CAUSAL || key <= q0 + 16 * x + r16)) ? sf[x][f][e] : -INFINITY;
                }
        }
#pragma unroll
        for (int x = 0; x < QF; ++x) {
            float mb = fmaxf(fmaxf(sf[x][0][0], sf[x][0][1]), fmaxf(sf[x][0][2], sf[x][0][3]));
#pragma unroll
            for (int f = 1; f < KF; ++f)
                mb = fmaxf(fmaxf(mb, fmaxf(sf[x][f][0], sf[x][f][1])), fmaxf(sf[x][f][2], sf[x][f][3]));
            mb = g4_max(mb);   // -inf only in a later block with no visible key: then mn = m, finite since block 0
            const float mn = fmaxf(m[x], MODE == SA_CAUSAL ? mb * scale_log2 : mb);   // scale > 0 commutes with max
            if (__builtin_amdgcn_ballot_w64(mn != m[x])) {   // a running max moved: rescale this query set
                const float alpha = __builtin_amdgcn_exp2f(m[x] - mn);   // 0 on the first block (m = -inf)
                l[x] *= alpha;
#pragma unroll
                for (int d = 0; d < DF; ++d)
#pragma unroll
                    for (int e = 0; e < 4; ++e) oc[x][d][e] *= alpha;
                m[x] = mn;
            }
            if constexpr (MODE == SA_CAUSAL) {   // raw scores: one packed FMA per pair, then exp2
                const fa_f32x2 sc2 = {scale_log2, scale_log2}, nm2 = {-mn, -mn};
                fa_f32x2 acc2 = {0.f, 0.f};
#pragma unroll
                for (int f = 0; f < KF; ++f)
#pragma unroll
                    for (int e = 0; e < 4; e += 2) {
                        fa_f32x2 t = (fa_f32x2){sf[x][f][e], sf[x][f][e + 1]} * sc2 + nm2;
                        t.x = __builtin_amdgcn_exp2f(t.x);
                        t.y = __builtin_amdgcn_exp2f(t.y);
                        sf[x][f][e] = t.x;
                        sf[x][f][e + 1] = t.y;
                        acc2 = acc2 + t;
                    }
                l[x] += acc2.x + acc2.y;
            } else {
                float acc = 0.f;
#pragma unroll
                for (int f = 0; f < KF; ++f)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        sf[x][f][e] = __builtin_amdgcn_exp2f(sf[x][f][e] - mn);
                        acc += sf[x][f][e];
                    }
                l[x] += acc;
            }
        }
#pragma unroll
        for (int j = 0; j < KF / 2; ++j) {
            la_bf16x8 bp[QF];
#pragma unroll
            for (int x = 0; x < QF; ++x)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    bp[x][e] = (__bf16)sf[x][2 * j][e];
                    bp[x][4 + e] = (__bf16)sf[x][2 * j + 1][e];
                }
#pragma unroll
            for (int d = 0; d < DF; ++d) {
                const la_bf16x8 av = xa_tr8_perm<RS>(sv + (32 * j) * RS + 16 * d, lane);
#pragma unroll
                for (int x = 0; x < QF; ++x) oc[x][d] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, bp[x], oc[x][d], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int x = 0; x < QF; ++x) {
        const float sum = g4_sum(l[x]);
        const int qr = q0 + 16 * x + r16;
        if (qr < N) {
            const bool valid = qr < L;
            const float inv = 1.0f / sum;
            unsigned short* dst = o + (row0 + qr) * ldo + (int64_t)h * HD + 4 * g;
#pragma unroll
            for (int d = 0; d < DF; ++d) {
                u16x4m t;
#pragma unroll
                for (int e = 0; e < 4; ++e) t[e] = valid ? f2b(oc[x][d][e] * inv) : (unsigned short)0;
                *reinterpret_cast<u16x4m*>(dst + 16 * d) = t;
            }
        }
    }
}

// ------------------------------------------------------------------------------------
// Host side.  The stride / alignment / NULL / grid checks every entry point makes; `fn` names the entry point in
// every message.  q / o rows hold heads_q heads of hd, k / v rows heads_kv; more_ok: the entry point's further
// stride conditions; `empty`: nothing to launch, accepted (*go = false) once the strides are seen and before any
// pointer is looked at; lens: the per-sequence length vector where the entry point has one.
// ------------------------------------------------------------------------------------
static int attn_args(const char* fn, int64_t hd, int64_t heads_q, int64_t heads_kv, const void* q, int64_t ldq,
                     const void* k, int64_t ldk, const void* v, int64_t ldv, const void* o, int64_t ldo, bool more_ok,
                     bool empty, const int32_t* lens, bool has_lens, int64_t grid, bool* go) {
    *go = false;
    EGG_CHECK_ARG(ldq % 8 == 0 && ldk % 8 == 0 && ldv % 8 == 0 && ldo % 4 == 0 && more_ok && ldq >= heads_q * hd &&
                  ldk >= heads_kv * hd && ldv >= heads_kv * hd && ldo >= heads_q * hd, "%s: bad strides", fn);
    if (empty) return EGGROLL_OK;
    EGG_CHECK_ARG(q && k && v && o && (lens || !has_lens), "%s: NULL pointer", fn);
    EGG_CHECK_ARG(((uintptr_t)q & 15) == 0 && ((uintptr_t)k & 15) == 0 && ((uintptr_t)v & 15) == 0 && ((uintptr_t)o & 7) == 0 &&
                  ((uintptr_t)lens & 3) == 0, "%s: q/k/v must be 16-byte aligned, o 8-byte aligned", fn);
    EGG_CHECK_ARG(grid < (1ll << 31), "%s: grid too large", fn);
    *go = true;
    return EGGROLL_OK;
}

template <int HD, int LM>
static void cross_attn_launch(int variant, const void* q, int64_t ldq, const void* k, const void* v, int64_t ldkv,
                              const void* bias, const int32_t* enc_index, int64_t B, int64_t N, int64_t heads, int64_t L,
                              int64_t U, float scale, void* o, int64_t ldo, void* stream) {
    // 8 waves x 16-query blocks (164 VGPRs, 2 waves per SIMD): measured 0.80 ms at the Sana attn2 shape
    // (B 128, N 1024, 20 heads, L 300) vs 0.94 for 4 waves x 32 queries and 1.27 for 4 x 16 (SDPA on
    // the gathered k / v with the mask: 1.53 ms)
    // default: 32-query blocks with the two-half online softmax (k_cross_attn_h2)
    hipLaunchKernelGGL(variant == 1 ? (k_cross_attn<HD, 8, 1, LM>) : (k_cross_attn_h2<HD, 8, LM>),
                       dim3((unsigned)(B * heads)), dim3(512), 0, as_stream(stream), (const unsigned short*)q, ldq,
                       (const unsigned short*)k, (const unsigned short*)v, ldkv, (const unsigned short*)bias, enc_index,
                       (int)heads, (int)N, (int)L, (int)U, scale, (unsigned short*)o, ldo);
}

// variant: 0 = automatic (the 32-query two-half online-softmax k_cross_attn_h2), 1 = the 16-query two-pass
// k_cross_attn (one max / exp pass over all keys), 2 = k_cross_attn_h2 explicitly.  Both are exact softmax up
// to fp32 rounding; the selector lets the full-size rank test score the same epochs through each form.
extern "C" int eggroll_cross_attention_sel(const void* q, int64_t ldq, const void* k, const void* v, int64_t ldkv,
                                           const void* bias, const int32_t* enc_index, int64_t B, int64_t N,
                                           int64_t heads, int64_t head_dim, int64_t L, int64_t U, float scale, void* o,
                                           int64_t ldo, int32_t variant, void* stream) {
    EGG_CHECK_ARG(variant >= 0 && variant <= 2, "cross_attention: variant must be 0 (auto), 1 (two-pass) or 2 (online)");
    EGG_CHECK_ARG(head_dim == 64 || head_dim == 80 || head_dim == 112 || head_dim == 128, "cross_attention: head_dim "
                  "%lld unsupported (64, 80, 112, 128)", (long long)head_dim);
    // head dim 128 (Infinity's text cross-attention) stages at most 256 keys: k + v at 320 would not fit 160 KiB
    const int64_t lmax = head_dim == 128 ? XA_LMAX_128 : XA_LMAX;
    EGG_CHECK_ARG(B >= 0 && N > 0 && heads > 0 && L > 0 && L <= lmax, "cross_attention: bad sizes (L <= %lld at head "
                  "dim %lld)", (long long)lmax, (long long)head_dim);
    EGG_CHECK_ARG(U > 0 && U * L < (1ll << 31) && (enc_index || U >= B),
                  "cross_attention: U=%lld caption rows (need U >= B without enc_index)", (long long)U);
    bool go;
    if (int rc = attn_args("cross_attention", head_dim, heads, heads, q, ldq, k, ldkv, v, ldkv, o, ldo, true, B == 0,
                           nullptr, false, B * heads, &go))
        return rc;
    if (!go) return EGGROLL_OK;
    auto launch = head_dim == 112 ? cross_attn_launch<112, XA_LMAX>
                : head_dim == 128 ? cross_attn_launch<128, XA_LMAX_128>
                : head_dim == 80  ? cross_attn_launch<80, XA_LMAX> : cross_attn_launch<64, XA_LMAX>;
    launch(variant, q, ldq, k, v, ldkv, bias, enc_index, B, N, heads, L, U, scale, o, ldo, stream);
    EGG_CHECK_LAUNCH("cross_attention");
    return EGGROLL_OK;
}

extern "C" int eggroll_cross_attention(const void* q, int64_t ldq, const void* k, const void* v, int64_t ldkv,
                                       const void* bias, const int32_t* enc_index, int64_t B, int64_t N,
                                       int64_t heads, int64_t head_dim, int64_t L, int64_t U, float scale, void* o,
                                       int64_t ldo, void* stream) {
    return eggroll_cross_attention_sel(q, ldq, k, v, ldkv, bias, enc_index, B, N, heads, head_dim, L, U, scale, o, ldo,
                                       0, stream);
}

extern "C" int eggroll_flash_attention_sel(const void* q, int64_t q_bs, int64_t ldq, const void* k, int64_t k_bs,
                                           int64_t ldk, const void* v, int64_t v_bs, int64_t ldv, int64_t B,
                                           int64_t heads, int64_t Nq, int64_t Lk, int64_t head_dim, float scale, void* o,
                                           int64_t o_bs, int64_t ldo, int32_t qf, void* stream) {
    EGG_CHECK_ARG(qf == 0 || qf == 1 || qf == 2 || qf == 4, "flash_attention: qf must be 0 (auto), 1, 2 or 4");
    EGG_CHECK_ARG(head_dim == 64 || head_dim == FA_HD, "flash_attention: head_dim %lld unsupported (64, 128)",
                  (long long)head_dim);
    EGG_CHECK_ARG(B >= 0 && heads > 0 && Nq >= 0 && Lk >= 1, "flash_attention: bad sizes");
    // automatic: 32 queries per wave; at head dim 64 (VAR: 1 ... 256 queries a scale) 16 where 64-query workgroups
    // pad the queries with fewer dead rows than 128-query ones (measured at B 128, 16 heads: 8.1 vs 11.2 us at
    // Nq <= 9, 25 vs 31 at 64, 109 vs 117 at 169; 48 vs 45 at 100 and 228 vs 193 at 256, where they pad alike)
    if (qf == 0) qf = head_dim == 64 && (Nq + 63) / 64 * 64 < (Nq + 127) / 128 * 128 ? 1 : 2;
    const int64_t qwg = 4 * 16 * qf, nqb = (Nq + qwg - 1) / qwg;
    // a sequence too long for the kernel's int counts is reported as such, after the pointer checks, not as a grid
    const bool fits = Nq < (1ll << 31) && Lk < (1ll << 31);
    bool go;
    if (int rc = attn_args("flash_attention", head_dim, heads, heads, q, ldq, k, ldk, v, ldv, o, ldo,
                           q_bs % 8 == 0 && k_bs % 8 == 0 && v_bs % 8 == 0 && o_bs % 4 == 0, B == 0 || Nq == 0, nullptr,
                           false, fits ? B * heads * nqb : 0, &go))
        return rc;
    if (!go) return EGGROLL_OK;
    EGG_CHECK_ARG(fits, "flash_attention: sequence too long");
    auto* kern = head_dim == 64
        ? (qf == 4 ? k_flash_attn<64, FA_RS64, 4, 2> : (qf == 1 ? k_flash_attn<64, FA_RS64, 1, 4> : k_flash_attn<64, FA_RS64, 2, 3>))
        : (qf == 4 ? k_flash_attn<FA_HD, FA_RS, 4, 1> : (qf == 1 ? k_flash_attn<FA_HD, FA_RS, 1, 3> : k_flash_attn<FA_HD, FA_RS, 2, 2>));
    hipLaunchKernelGGL(kern, dim3((unsigned)(B * heads * nqb)), dim3(256), 0, as_stream(stream),
                       (const unsigned short*)q, q_bs, ldq, (const unsigned short*)k, k_bs, ldk,
                       (const unsigned short*)v, v_bs, ldv, (int)heads, (int)Nq, (int)Lk, (int)nqb,
                       scale * 1.4426950408889634f, (unsigned short*)o, o_bs, ldo);
    EGG_CHECK_LAUNCH("flash_attention");
    return EGGROLL_OK;
}

extern "C" int eggroll_flash_attention(const void* q, int64_t q_bs, int64_t ldq, const void* k, int64_t k_bs,
                                       int64_t ldk, const void* v, int64_t v_bs, int64_t ldv, int64_t B, int64_t heads,
                                       int64_t Nq, int64_t Lk, int64_t head_dim, float scale, void* o, int64_t o_bs,
                                       int64_t ldo, void* stream) {
    return eggroll_flash_attention_sel(q, q_bs, ldq, k, k_bs, ldk, v, v_bs, ldv, B, heads, Nq, Lk, head_dim, scale, o,
                                       o_bs, ldo, 0, stream);
}

// The argument checks the three prompt-encoder entry points share.  nmax: the largest N the instance takes; qblk:
// its query block.  An empty batch (B == 0) is accepted before any pointer is looked at and gives *nqb = 0:
// nothing to launch.
static int seq_attn_args(const char* fn, int hd, int qblk, int64_t nmax, const void* q, int64_t ldq, const void* k,
                         int64_t ldk, const void* v, int64_t ldv, const int32_t* lens, int64_t B, int64_t heads_q,
                         int64_t heads_kv, int64_t N, int64_t head_dim, const void* o, int64_t ldo, int64_t* nqb) {
    *nqb = 0;
    EGG_CHECK_ARG(head_dim == hd, "%s: head_dim %lld unsupported (%d)", fn, (long long)head_dim, hd);
    EGG_CHECK_ARG(B >= 0 && heads_kv >= 1 && heads_q >= heads_kv && heads_q % heads_kv == 0,
                  "%s: bad sizes B=%lld heads_q=%lld heads_kv=%lld (heads_q = G * heads_kv)", fn, (long long)B,
                  (long long)heads_q, (long long)heads_kv);
    if (B == 0) return EGGROLL_OK;
    EGG_CHECK_ARG(N >= 1 && N <= nmax, "%s: N=%lld outside [1, %lld]", fn, (long long)N, (long long)nmax);
    const int64_t n = (N + qblk - 1) / qblk;
    bool go;
    if (int rc = attn_args(fn, hd, heads_q, heads_kv, q, ldq, k, ldk, v, ldv, o, ldo, true, false, lens, true,
                           B * heads_q * n, &go))
        return rc;
    *nqb = n;
    return EGGROLL_OK;
}

template <int MODE, int HD, int KB, int QF, int RS, int MINB>
static int seq_attn_launch(const char* fn, const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v,
                           int64_t ldv, const float* rel_bias, int64_t R, const int32_t* lens, int64_t B,
                           int64_t heads_q, int64_t heads_kv, int64_t N, int64_t nqb, float scale, float cap, void* o,
                           int64_t ldo, void* stream) {
    const float LOG2E = 1.4426950408889634f;
    hipLaunchKernelGGL((k_seq_attn<MODE, HD, KB, QF, RS, MINB>), dim3((unsigned)(B * heads_q * nqb)), dim3(256), 0,
                       as_stream(stream), (const unsigned short*)q, ldq, (const unsigned short*)k, ldk,
                       (const unsigned short*)v, ldv, rel_bias, (int)R, lens, (int)heads_q, (int)(heads_q / heads_kv),
                       (int)N, (int)nqb, scale * LOG2E, cap > 0.0f ? 2.0f * LOG2E * scale / cap : 0.0f, cap * LOG2E,
                       (unsigned short*)o, ldo);
    EGG_CHECK_LAUNCH(fn);
    return EGGROLL_OK;
}

extern "C" int eggroll_relbias_attention(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v,
                                         int64_t ldv, const float* rel_bias, int64_t R, const int32_t* lens, int64_t B,
                                         int64_t heads, int64_t N, int64_t head_dim, float scale, void* o, int64_t ldo,
                                         void* stream) {
    const char* fn = "relbias_attention";
    int64_t nqb;
    if (int rc = seq_attn_args(fn, 64, 64, RB_NMAX, q, ldq, k, ldk, v, ldv, lens, B, heads, heads, N, head_dim, o, ldo, &nqb))
        return rc;
    if (nqb == 0) return EGGROLL_OK;
    EGG_CHECK_ARG(R >= N && R < (1ll << 24), "%s: rel_bias is [heads][2R-1] with R >= N (R=%lld, N=%lld)", fn,
                  (long long)R, (long long)N);
    EGG_CHECK_ARG(rel_bias && ((uintptr_t)rel_bias & 3) == 0, "%s: rel_bias is NULL or not 4-byte aligned", fn);
    return seq_attn_launch<SA_RELBIAS, 64, 64, 1, 72, 1>(fn, q, ldq, k, ldk, v, ldv, rel_bias, R, lens, B, heads, heads, N,
                                                         nqb, scale, 0.0f, o, ldo, stream);
}

extern "C" int eggroll_softcap_attention(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v,
                                         int64_t ldv, const int32_t* lens, int64_t B, int64_t heads_q, int64_t heads_kv,
                                         int64_t N, int64_t head_dim, float scale, float cap, void* o, int64_t ldo,
                                         void* stream) {
    const char* fn = "softcap_attention";
    EGG_CHECK_ARG(cap >= 0.0f && cap < INFINITY, "%s: cap must be finite and >= 0 (0: no soft-cap)", fn);
    int64_t nqb;
    if (int rc = seq_attn_args(fn, 256, 64, (1ll << 31) - 64 - 1, q, ldq, k, ldk, v, ldv, lens, B, heads_q, heads_kv, N,
                               head_dim, o, ldo, &nqb))
        return rc;
    if (nqb == 0) return EGGROLL_OK;
    return seq_attn_launch<SA_SOFTCAP, 256, 32, 1, 264, 1>(fn, q, ldq, k, ldk, v, ldv, nullptr, 0, lens, B, heads_q,
                                                           heads_kv, N, nqb, scale, cap, o, ldo, stream);
}

extern "C" int eggroll_causal_attention(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v,
                                        int64_t ldv, const int32_t* lens, int64_t B, int64_t heads_q, int64_t heads_kv,
                                        int64_t N, int64_t head_dim, float scale, void* o, int64_t ldo, void* stream) {
    const char* fn = "causal_attention";
    EGG_CHECK_ARG(scale > 0.0f && scale < INFINITY, "%s: scale must be finite and > 0", fn);
    int64_t nqb;
    if (int rc = seq_attn_args(fn, FA_HD, 128, (1ll << 31) - 128 - 1, q, ldq, k, ldk, v, ldv, lens, B, heads_q, heads_kv, N,
                               head_dim, o, ldo, &nqb))
        return rc;
    if (nqb == 0) return EGGROLL_OK;
    return seq_attn_launch<SA_CAUSAL, FA_HD, FA_KB, 2, FA_RS, 2>(fn, q, ldq, k, ldk, v, ldv, nullptr, 0, lens, B, heads_q,
                                                                 heads_kv, N, nqb, scale, 0.0f, o, ldo, stream);
}
