// libeggroll — ReLU linear attention at head dim 32 on MFMA (gfx950): Sana attn1 and the DC-AE's multi-scale
// attention.
//
//   k_la_kv      : pass 1, per (image, head, token chunk) partial kv / ksum
//   k_la_reduce, k_la_reduce_e : the chunk partials summed per head in a fixed order
//   k_la_kv_fold : passes 1 and 2 in one launch for few chunks per head (the same bits)
//   k_la_out     : pass 3, out = relu(q) kv / (relu(q) . ksum)
#include "frag.h"

namespace eggroll {

// ------------------------------------------------------------------------------------
// ReLU linear attention, head dim 32 (SanaLinearAttnProcessor2_0 / DC-AE multiscale attention):
//   kv[i][j] = sum_n v[n,i] relu(k[n,j]),  ksum[j] = sum_n relu(k[n,j])     (per image, head)
//   out[n,i] = (sum_j relu(q[n,j]) kv[i][j]) / (sum_j relu(q[n,j]) ksum[j] + 1e-15)
// fp32 accumulation.  Pass 1: per (image*head, token chunk) partial kv/ksum -> workspace;
// pass 2: per (image*head, token chunk) fixed-order sum of the partials in LDS, then one token
// per thread.  q/k/v are strided views (row stride, head stride) of the projection outputs.
// ------------------------------------------------------------------------------------
constexpr int LA_D = 32;
constexpr int LA_PART = LA_D * LA_D + LA_D;   // kv + ksum floats per partial
constexpr int LA_T = 256;                     // tokens per chunk
#ifndef EGG_LA_HEAD_PAIRS
#define EGG_LA_HEAD_PAIRS 1
#endif
#ifndef EGG_LA_FOLD  // k_la_kv_fold for few chunks per head (A/B knob; 0 = k_la_kv + k_la_reduce)
#define EGG_LA_FOLD 1
#endif

// Pass 1 per (image*head, chunk of LA_T tokens) on MFMA: k (ReLU'd) and v staged into LDS token-major
// as bf16 (all 8 loads per thread in flight), then kv^T-free: C[i][j] = sum_n v[n][i] relu(k[n][j]) as
// 16x16x32 bf16 MFMAs with the TOKEN axis as K — both operands need 8 consecutive tokens of one
// feature per lane, which ds_read_b64_tr_b16 (gfx950 transpose read: per 16-lane group a 4-row x
// 16-column block delivered column-major) reads straight from the token-major image.  ksum[j] is one
// more MFMA with a row of ones as A.  Each wave covers 64 tokens (2 K-steps); the 4 waves' partials
// are summed in a fixed order through LDS.  Products of bf16 inputs are exact in fp32, as in the VALU
// form; only the accumulation order differs.
constexpr int LA_RS = LA_D + 8;  // bf16 LDS row stride (80 B: 8-B aligned rows for the transpose reads)

__device__ __forceinline__ la_bf16x8 la_tr8(const unsigned short* base, int lane) {
    // rows base + 8g + {0..3} and {4..7} of the 16-lane group g; lane 4q+p addresses row q, columns 4p..4p+3
    const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
    const unsigned short* r0 = base + (8 * g + q) * LA_RS + 4 * p;
    const la_s4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((la_lds_s4*)(r0));
    const la_s4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((la_lds_s4*)(r0 + 4 * LA_RS));
    typedef __attribute__((ext_vector_type(8))) short s8;
    const s8 f = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(la_bf16x8, f);
}

// HP = 2 (contiguous heads, hstride == 32, even head count): a block stages one token chunk of a head
// PAIR, so every k / v load covers a whole 128-B line (a token's 64 B of two neighbouring heads) instead
// of relying on the neighbouring head's block to read the other half through L2; each head's MFMAs,
// per-wave token split and partial sums are those of HP = 1 (the same bits).
template <int HP>
__global__ __launch_bounds__(256) void k_la_kv(const unsigned short* __restrict__ k, const unsigned short* __restrict__ v,
                                               int64_t ld, int64_t hstride, int heads, int N, int nchunk, int relu,
                                               float* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) unsigned short lds_kv[HP * 2 * LA_T * LA_RS];  // [head] sk | sv, then red
    float(*red)[LA_PART] = reinterpret_cast<float(*)[LA_PART]>(lds_kv);  // [head * 4 + wave], after the MFMAs
    static_assert(HP * 4 * LA_PART * 4 <= HP * 2 * LA_T * LA_RS * 2, "reduction buffer fits in the staging LDS");
    const int lb = xcd_remap(blockIdx.x, gridDim.x);  // adjacent heads share 128-B lines: same L2
    const int bhp = lb / nchunk, c = lb - bhp * nchunk;
    const int hg = heads / HP, b = bhp / hg, h0 = (bhp - b * hg) * HP;
    const int n0 = c * LA_T;
    const int cnt = (N - n0) < LA_T ? (N - n0) : LA_T;
    const int tid = threadIdx.x;
    constexpr int U = 4 * HP;  // 16-B units per token and tensor (HP heads x 64 B)
    u16x8m kr[U], vr[U];
#pragma unroll
    for (int it = 0; it < U; ++it) {  // LA_T tokens x U units per tensor
        const int u = tid + it * 256, t = u / U, q8 = u % U;
        kr[it] = vr[it] = u16x8m{0, 0, 0, 0, 0, 0, 0, 0};
        if (t < cnt) {
            const int64_t off = ((int64_t)b * N + n0 + t) * ld + (int64_t)h0 * hstride + (q8 >> 2) * hstride + (q8 & 3) * 8;
            kr[it] = *reinterpret_cast<const u16x8m*>(k + off);
            vr[it] = *reinterpret_cast<const u16x8m*>(v + off);
        }
    }
#pragma unroll
    for (int it = 0; it < U; ++it) {
        const int u = tid + it * 256, t = u / U, q8 = u % U;
        unsigned short* sk = lds_kv + (q8 >> 2) * (2 * LA_T * LA_RS);
        unsigned short* sv = sk + LA_T * LA_RS;
        if (relu) {
#pragma unroll
            for (int i = 0; i < 8; ++i) kr[it][i] = (kr[it][i] & 0x8000) ? (unsigned short)0 : kr[it][i];  // bf16 ReLU (-0 -> +0)
        }
        *reinterpret_cast<u16x8m*>(sk + t * LA_RS + (q8 & 3) * 8) = kr[it];
        *reinterpret_cast<u16x8m*>(sv + t * LA_RS + (q8 & 3) * 8) = vr[it];
    }
    __syncthreads();
    const int lane = tid & 63, w = tid >> 6, r16 = lane & 15, g = lane >> 4;
    la_bf16x8 ones;
#pragma unroll
    for (int e = 0; e < 8; ++e) ones[e] = (__bf16)(r16 == 0 ? 1.0f : 0.0f);  // A row 0 = ones -> ksum
    la_f32x4 acc[HP][2][2], ks[HP][2];
#pragma unroll
    for (int hh = 0; hh < HP; ++hh)
#pragma unroll
        for (int x = 0; x < 2; ++x) {
            ks[hh][x] = la_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int y = 0; y < 2; ++y) acc[hh][x][y] = la_f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
    for (int hh = 0; hh < HP; ++hh) {
        const unsigned short* sk = lds_kv + hh * (2 * LA_T * LA_RS);
        const unsigned short* sv = sk + LA_T * LA_RS;
#pragma unroll
        for (int s = 0; s < 2; ++s) {  // this wave's 64 tokens as 2 K-steps of 32
            const int t0 = w * 64 + s * 32;
            la_bf16x8 av[2], bk[2];
#pragma unroll
            for (int x = 0; x < 2; ++x) {
                av[x] = la_tr8(sv + t0 * LA_RS + 16 * x, lane);  // A[i = 16x + r16][n]
                bk[x] = la_tr8(sk + t0 * LA_RS + 16 * x, lane);  // B[n][j = 16x + r16]
            }
#pragma unroll
            for (int x = 0; x < 2; ++x) {
#pragma unroll
                for (int y = 0; y < 2; ++y)
                    acc[hh][x][y] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[x], bk[y], acc[hh][x][y], 0, 0, 0);
                ks[hh][x] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, bk[x], ks[hh][x], 0, 0, 0);
            }
        }
    }
    __syncthreads();  // every wave is done reading sk / sv: reuse the staging LDS for the reduction
    // C layout: lane holds C[4g + e][r16]
#pragma unroll
    for (int hh = 0; hh < HP; ++hh) {
        float* rw = red[hh * 4 + w];
#pragma unroll
        for (int x = 0; x < 2; ++x)
#pragma unroll
            for (int y = 0; y < 2; ++y)
#pragma unroll
                for (int e = 0; e < 4; ++e) rw[(16 * x + 4 * g + e) * LA_D + 16 * y + r16] = acc[hh][x][y][e];
        if (g == 0) {
#pragma unroll
            for (int y = 0; y < 2; ++y) rw[LA_D * LA_D + 16 * y + r16] = ks[hh][y][0];
        }
    }
    __syncthreads();
#pragma unroll
    for (int hh = 0; hh < HP; ++hh) {
        // slot bh * nchunk + c (bh = b * heads + h): k_la_reduce sums chunks in order
        float* dst = part + ((int64_t)b * heads + h0 + hh) * nchunk * LA_PART + (int64_t)c * LA_PART;
        const float(*r4)[LA_PART] = red + hh * 4;
        for (int e = tid; e < LA_PART; e += 256) dst[e] = ((r4[0][e] + r4[1][e]) + r4[2][e]) + r4[3][e];
    }
}

// Round 6: the kv pass with the chunk reduction folded in, for few chunks per head
// (N <= LA_FOLD_MAX * LA_T) on grids large enough to fill the chip with one block per head (group): the block
// walks its head's chunks in order, computes each chunk's partial exactly as k_la_kv does (same MFMAs, same
// ((w0 + w1) + w2) + w3 wave sum), and adds it into a per-thread running sum that starts at 0 as
// k_la_reduce's does — the same additions in the same order, so kvsum is bitwise k_la_kv + k_la_reduce's,
// without the partials' round trip through HBM or the reduce launch.  The next chunk's k / v loads are
// issued as soon as this chunk is in LDS, so they land under its MFMAs and reduction.
constexpr int LA_FOLD_MAX = 4;
template <int HP>
__global__ __launch_bounds__(256) void k_la_kv_fold(const unsigned short* __restrict__ k, const unsigned short* __restrict__ v,
                                                    int64_t ld, int64_t hstride, int heads, int N, int nchunk, int relu,
                                                    float* __restrict__ kvsum) {
    __shared__ __attribute__((aligned(16))) unsigned short lds_kv[HP * 2 * LA_T * LA_RS];
    float(*red)[LA_PART] = reinterpret_cast<float(*)[LA_PART]>(lds_kv);
    static_assert(HP * 4 * LA_PART * 4 <= HP * 2 * LA_T * LA_RS * 2, "reduction buffer fits in the staging LDS");
    constexpr int EPT = (LA_PART + 255) / 256;  // kvsum elements per thread per head
    const int bhp = xcd_remap(blockIdx.x, gridDim.x);
    const int hg = heads / HP, b = bhp / hg, h0 = (bhp - b * hg) * HP;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r16 = lane & 15, g = lane >> 4;
    constexpr int U = 4 * HP;
    u16x8m kr[U], vr[U];
    auto load = [&](int c) {
        const int n0 = c * LA_T, cnt = (N - n0) < LA_T ? (N - n0) : LA_T;
#pragma unroll
        for (int it = 0; it < U; ++it) {
            const int u = tid + it * 256, t = u / U, q8 = u % U;
            kr[it] = vr[it] = u16x8m{0, 0, 0, 0, 0, 0, 0, 0};
            if (t < cnt) {
                const int64_t off = ((int64_t)b * N + n0 + t) * ld + (int64_t)h0 * hstride + (q8 >> 2) * hstride + (q8 & 3) * 8;
                kr[it] = *reinterpret_cast<const u16x8m*>(k + off);
                vr[it] = *reinterpret_cast<const u16x8m*>(v + off);
            }
        }
    };
    la_bf16x8 ones;
#pragma unroll
    for (int e = 0; e < 8; ++e) ones[e] = (__bf16)(r16 == 0 ? 1.0f : 0.0f);
    float sum[HP][EPT];
#pragma unroll
    for (int hh = 0; hh < HP; ++hh)
#pragma unroll
        for (int q = 0; q < EPT; ++q) sum[hh][q] = 0.f;
    load(0);
#pragma unroll 1
    for (int c = 0; c < nchunk; ++c) {
        if (c > 0) __syncthreads();  // every thread is done reading the previous chunk's reduction table
#pragma unroll
        for (int it = 0; it < U; ++it) {
            const int u = tid + it * 256, t = u / U, q8 = u % U;
            unsigned short* sk = lds_kv + (q8 >> 2) * (2 * LA_T * LA_RS);
            unsigned short* sv = sk + LA_T * LA_RS;
            if (relu) {
#pragma unroll
                for (int i = 0; i < 8; ++i) kr[it][i] = (kr[it][i] & 0x8000) ? (unsigned short)0 : kr[it][i];
            }
            *reinterpret_cast<u16x8m*>(sk + t * LA_RS + (q8 & 3) * 8) = kr[it];
            *reinterpret_cast<u16x8m*>(sv + t * LA_RS + (q8 & 3) * 8) = vr[it];
        }
        if (c + 1 < nchunk) load(c + 1);  // in flight under this chunk's MFMAs
        __syncthreads();
        la_f32x4 acc[HP][2][2], ks[HP][2];
#pragma unroll
        for (int hh = 0; hh < HP; ++hh)
#pragma unroll
            for (int x = 0; x < 2; ++x) {
                ks[hh][x] = la_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int y = 0; y < 2; ++y) acc[hh][x][y] = la_f32x4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
        for (int hh = 0; hh < HP; ++hh) {
            const unsigned short* sk = lds_kv + hh * (2 * LA_T * LA_RS);
            const unsigned short* sv = sk + LA_T * LA_RS;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int t0 = w * 64 + s * 32;
                la_bf16x8 av[2], bk[2];
#pragma unroll
                for (int x = 0; x < 2; ++x) {
                    av[x] = la_tr8(sv + t0 * LA_RS + 16 * x, lane);
                    bk[x] = la_tr8(sk + t0 * LA_RS + 16 * x, lane);
                }
#pragma unroll
                for (int x = 0; x < 2; ++x) {
#pragma unroll
                    for (int y = 0; y < 2; ++y)
                        acc[hh][x][y] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[x], bk[y], acc[hh][x][y], 0, 0, 0);
                    ks[hh][x] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, bk[x], ks[hh][x], 0, 0, 0);
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int hh = 0; hh < HP; ++hh) {
            float* rw = red[hh * 4 + w];
#pragma unroll
            for (int x = 0; x < 2; ++x)
#pragma unroll
                for (int y = 0; y < 2; ++y)
#pragma unroll
                    for (int e = 0; e < 4; ++e) rw[(16 * x + 4 * g + e) * LA_D + 16 * y + r16] = acc[hh][x][y][e];
            if (g == 0) {
#pragma unroll
                for (int y = 0; y < 2; ++y) rw[LA_D * LA_D + 16 * y + r16] = ks[hh][y][0];
            }
        }
        __syncthreads();
#pragma unroll
        for (int hh = 0; hh < HP; ++hh) {
            const float(*r4)[LA_PART] = red + hh * 4;
#pragma unroll
            for (int q = 0; q < EPT; ++q) {
                const int e = tid + 256 * q;
                if (e < LA_PART) sum[hh][q] += ((r4[0][e] + r4[1][e]) + r4[2][e]) + r4[3][e];
            }
        }
    }
#pragma unroll
    for (int hh = 0; hh < HP; ++hh) {
        float* dst = kvsum + ((int64_t)b * heads + h0 + hh) * LA_PART;
#pragma unroll
        for (int q = 0; q < EPT; ++q) {
            const int e = tid + 256 * q;
            if (e < LA_PART) dst[e] = sum[hh][q];
        }
    }
}

// Fixed-order sum of the nchunk partials of one (image, head) -> kvsum[bh], once per head: the
// k_la_out blocks then read 4 KiB each instead of every block re-summing all nchunk partials
// (O(nchunk) instead of O(nchunk^2) partial reads: 64 chunks per head at DC-AE's 128x128 stage).
__global__ __launch_bounds__(256) void k_la_reduce(const float* __restrict__ part, int nchunk,
                                                   float* __restrict__ kvsum) {
    const int64_t bh = blockIdx.x;
    const float* src = part + bh * nchunk * LA_PART;
    for (int e = threadIdx.x; e < LA_PART; e += 256) {
        float s = 0.f;
        int cc = 0;
        for (; cc + 8 <= nchunk; cc += 8) {  // 8 loads in flight, summed in chunk order
            float p[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) p[u] = src[(int64_t)(cc + u) * LA_PART + e];
#pragma unroll
            for (int u = 0; u < 8; ++u) s += p[u];
        }
        for (; cc < nchunk; ++cc) s += src[(int64_t)cc * LA_PART + e];
        kvsum[bh * LA_PART + e] = s;
    }
}

// Many chunks (>= LA_RED_WIDE, DC-AE's 64^2 and 128^2 maps): one thread per element, one wave per 64
// elements (17 waves per head), a thread's partials loaded 16 at a time and summed in the same chunk
// order (bit-identical to k_la_reduce, which walks ~4 elements per thread one after another: 8 B x
// 16 K x 16 heads 0.226 -> 0.214 ms for the whole attention; at 4 chunks the 17x more workgroups cost
// more than they save)
constexpr int LA_RED_WAVES = (LA_PART + 63) / 64;
constexpr int LA_RED_WIDE = 16;
__global__ __launch_bounds__(64) void k_la_reduce_e(const float* __restrict__ part, int nchunk,
                                                    float* __restrict__ kvsum) {
    const int64_t bh = blockIdx.x / LA_RED_WAVES;
    const int e = (blockIdx.x % LA_RED_WAVES) * 64 + threadIdx.x;
    if (e >= LA_PART) return;
    const float* src = part + bh * nchunk * LA_PART + e;
    float s = 0.f;
    int cc = 0;
    for (; cc + 16 <= nchunk; cc += 16) {  // 16 loads in flight, summed in chunk order
        float p[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) p[u] = src[(int64_t)(cc + u) * LA_PART];
#pragma unroll
        for (int u = 0; u < 16; ++u) s += p[u];
    }
    for (; cc < nchunk; ++cc) s += src[(int64_t)cc * LA_PART];
    kvsum[bh * LA_PART + e] = s;
}

// Pass 3 on MFMA: out^T[i][t] = sum_j kv[i][j] relu(q[t][j]) as 16x16x32 bf16 MFMAs with kv as the A
// operand (row i, 8 consecutive j per lane — the natural [i][j] layout) and 16 tokens' q as the B
// operand (each lane's 16-B load is 8 consecutive features of one token), so the accumulator lane
// holds 4 consecutive output features of one token (one 8-byte store).  kv (fp32) enters as a bf16
// hi + lo pair (two MFMAs: ~2^-16 relative, fp32-class), and the denominator relu(q) . ksum is one
// more hi/lo MFMA pair with ksum as row 0 of a 16-row A tile.  The VALU form spent 1056 FMAs + as many
// LDS broadcast reads per token-head; this one is 6 MFMAs per 16 tokens and memory-bound.

__device__ __forceinline__ void la_split8(const float (&f)[8], la_bf16x8& hi, la_bf16x8& lo) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const __bf16 h = (__bf16)f[e];
        hi[e] = h;
        lo[e] = (__bf16)(f[e] - (float)h);
    }
}

// Round 5: the denominator row ksum is written into A rows 0, 4, 8 and 12 (each lane group g then holds
// den of its own token r16 as C[4g][r16] — the shuffle that broadcast row 0 is gone), a wave covers
// TPW tiles of 16 tokens (the kv hi/lo split amortised over twice the tokens, twice the q loads in
// flight), and q / out go through buffer descriptors (one per image, head offset in the base: 32-bit
// offsets, tokens past N out of range).  Same MFMAs, same operands: the same bits.
// TPW: 16-token tiles per wave (8; 16 at the DC-AE's 128^2 maps: 166 -> 154 us, r10c); HP = 2: a head
// pair per block as in k_la_kv (each q load / output row a whole 128-B line), per-head math unchanged.
template <int HP, int TPW>
__global__ __launch_bounds__(256) void k_la_out(const unsigned short* __restrict__ q, int64_t ld, int64_t hstride,
                                                int heads, int N, int nblk_tok, int relu, const float* __restrict__ kvsum,
                                                unsigned short* __restrict__ out, int64_t ldo) {
    constexpr int T = 4 * TPW * 16;  // tokens per block
    const int lb = xcd_remap(blockIdx.x, gridDim.x);
    const int bhp = lb / nblk_tok, c = lb - bhp * nblk_tok;
    const int hg = heads / HP, b = bhp / hg, h0 = (bhp - b * hg) * HP;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r16 = lane & 15, g = lane >> 4;
    const int n0 = c * T + wave * (T / 4);
    // q tiles first (the longest latency), then kv from L2
    constexpr uint32_t OOR = 0x80000000u;
    const __amdgpu_buffer_rsrc_t rq = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(q + (int64_t)b * N * ld + (int64_t)h0 * hstride), (short)0, (int)((int64_t)N * ld * 2), 0x00020000);
    u16x8m qr[TPW][HP];
#pragma unroll
    for (int tt = 0; tt < TPW; ++tt) {
        const int tok = n0 + tt * 16 + r16;
#pragma unroll
        for (int hh = 0; hh < HP; ++hh) {
            const uint32_t off = tok < N ? ((uint32_t)tok * (uint32_t)ld + (uint32_t)(hh * hstride) + 8 * g) * 2 : OOR;
            qr[tt][hh] = __builtin_bit_cast(u16x8m, __builtin_amdgcn_raw_buffer_load_b128(rq, off, 0, 0));
        }
    }
    la_bf16x8 akv[HP][2][2], aden[HP][2];  // [head][feature block][hi, lo]
#pragma unroll
    for (int hh = 0; hh < HP; ++hh) {
        const float* kvh = kvsum + ((int64_t)b * heads + h0 + hh) * LA_PART;
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) {
            const float4 x0 = *reinterpret_cast<const float4*>(kvh + (16 * cb + r16) * LA_D + 8 * g);
            const float4 x1 = *reinterpret_cast<const float4*>(kvh + (16 * cb + r16) * LA_D + 8 * g + 4);
            const float f[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
            la_split8(f, akv[hh][cb][0], akv[hh][cb][1]);
        }
        float f[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if ((r16 & 3) == 0) {  // A rows 0, 4, 8, 12 = ksum, the rest 0
            const float4 x0 = *reinterpret_cast<const float4*>(kvh + LA_D * LA_D + 8 * g);
            const float4 x1 = *reinterpret_cast<const float4*>(kvh + LA_D * LA_D + 8 * g + 4);
            f[0] = x0.x; f[1] = x0.y; f[2] = x0.z; f[3] = x0.w;
            f[4] = x1.x; f[5] = x1.y; f[6] = x1.z; f[7] = x1.w;
        }
        la_split8(f, aden[hh][0], aden[hh][1]);
    }
    const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(out + (int64_t)b * N * ldo + h0 * LA_D), (short)0, (int)((int64_t)N * ldo * 2), 0x00020000);
#pragma unroll
    for (int tt = 0; tt < TPW; ++tt) {
        const int tok = n0 + tt * 16 + r16;
#pragma unroll
        for (int hh = 0; hh < HP; ++hh) {
            u16x8m qv = qr[tt][hh];
            if (relu) {
#pragma unroll
                for (int e = 0; e < 8; ++e) qv[e] = (qv[e] & 0x8000) ? (unsigned short)0 : qv[e];  // bf16 ReLU
            }
            const la_bf16x8 bq = *reinterpret_cast<const la_bf16x8*>(&qv);
            la_f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0, ad = a0;
            a0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(akv[hh][0][0], bq, a0, 0, 0, 0);
            a0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(akv[hh][0][1], bq, a0, 0, 0, 0);
            a1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(akv[hh][1][0], bq, a1, 0, 0, 0);
            a1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(akv[hh][1][1], bq, a1, 0, 0, 0);
            ad = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aden[hh][0], bq, ad, 0, 0, 0);
            ad = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aden[hh][1], bq, ad, 0, 0, 0);
            const float inv = 1.0f / (ad[0] + 1e-15f);  // C[4g][r16] = den of token r16 in every lane group
            const uint32_t off = tok < N ? ((uint32_t)tok * (uint32_t)ldo + (uint32_t)(hh * LA_D) + 4 * g) * 2 : OOR;
            u16x4m o0, o1;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                o0[e] = f2b(a0[e] * inv);
                o1[e] = f2b(a1[e] * inv);
            }
            __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2m, o0), ro, off, 0, 0);
            __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2m, o1), ro, off + 32, 0, 0);
        }
    }
}

}  // namespace eggroll

using namespace eggroll;

extern "C" int64_t eggroll_linear_attention_workspace_bytes(int64_t B, int64_t N, int64_t heads) {
    const int64_t nchunk = (N + LA_T - 1) / LA_T;
    return B * heads * (nchunk + 1) * LA_PART * (int64_t)sizeof(float);  // partials, then per-head sums
}

extern "C" int eggroll_linear_attention(const void* q, const void* k, const void* v, int64_t ld, int64_t hstride,
                                        int64_t B, int64_t N, int64_t heads, int32_t relu_qk, void* out, int64_t ldo,
                                        void* workspace, void* stream) {
    EGG_CHECK_ARG(B >= 0 && N > 0 && heads > 0 && ld % 8 == 0 && hstride % 8 == 0 && ldo % 8 == 0,
                  "linear_attention: bad sizes/strides");
    EGG_CHECK_ARG(((uintptr_t)q & 15) == 0 && ((uintptr_t)k & 15) == 0 && ((uintptr_t)v & 15) == 0 &&
                  ((uintptr_t)out & 15) == 0, "linear_attention: pointers must be 16-byte aligned");
    if (B == 0) return EGGROLL_OK;
    EGG_CHECK_ARG(q && k && v && out && workspace, "linear_attention: NULL pointer");
    EGG_CHECK_ARG(N * ld < (1ll << 30) && N * ldo < (1ll << 30), "linear_attention: image too large (< 2 GiB per image)");
    const int64_t nchunk = (N + LA_T - 1) / LA_T;
    const int64_t blocks = B * heads * nchunk;
    EGG_CHECK_ARG(blocks < (1ll << 31), "linear_attention: grid too large");
    hipStream_t st = as_stream(stream);
    // head pairs per block when a head's 64 B and its neighbour's are one 128-B line (Sana's q / k / v,
    // the DC-AE's planar [Q | K | V]) and the grid stays large: Sana attn1 637 -> 615 us, the DC-AE's 128^2
    // maps 154 -> 152; at 8 x 64^2 / 32^2 x 32 heads (4096 / 1024 per-head blocks) the halved grid lost
    // 1-4 % (profiles/r10d_linear_attention_head_pairs_ab.log).  The reference-layout interleaved q | k | v
    // (hstride 96) stays per head.
    const int hp = hstride == LA_D && heads % 2 == 0 && blocks >= 8192 && EGG_LA_HEAD_PAIRS ? 2 : 1;
    float* kvsum = (float*)workspace + blocks * LA_PART;
    // few chunks per head on a grid that one block per head (group) still fills (Sana attn1: 128 x 35 head
    // pairs x 4 chunks): the reduction folded into the kv pass (k_la_kv_fold, the same bits)
    const bool fold = EGG_LA_FOLD && nchunk <= LA_FOLD_MAX && B * heads / hp >= 2048;
    using HeadsPerBlock = std::integer_sequence<int, 1, 2>;
    if (fold) {
        dispatch_int(hp, HeadsPerBlock{}, [&](auto HP) {
            hipLaunchKernelGGL(k_la_kv_fold<decltype(HP)::value>, dim3((unsigned)(B * heads / hp)), dim3(256), 0, st,
                               (const unsigned short*)k, (const unsigned short*)v, ld, hstride, (int)heads, (int)N,
                               (int)nchunk, relu_qk, kvsum);
        });
        EGG_CHECK_LAUNCH("linear_attention_kv_fold");
    } else {
        dispatch_int(hp, HeadsPerBlock{}, [&](auto HP) {
            hipLaunchKernelGGL(k_la_kv<decltype(HP)::value>, dim3((unsigned)(blocks / hp)), dim3(256), 0, st,
                               (const unsigned short*)k, (const unsigned short*)v, ld, hstride, (int)heads, (int)N,
                               (int)nchunk, relu_qk, (float*)workspace);
        });
        EGG_CHECK_LAUNCH("linear_attention_kv");
        if (nchunk >= LA_RED_WIDE)
            hipLaunchKernelGGL(k_la_reduce_e, dim3((unsigned)(B * heads * LA_RED_WAVES)), dim3(64), 0, st,
                               (const float*)workspace, (int)nchunk, kvsum);
        else
            hipLaunchKernelGGL(k_la_reduce, dim3((unsigned)(B * heads)), dim3(256), 0, st, (const float*)workspace,
                               (int)nchunk, kvsum);
        EGG_CHECK_LAUNCH("linear_attention_reduce");
    }
    const bool big = N >= 8192;  // 16 tiles per wave at the DC-AE's 128^2 maps
    const int64_t tpb = 4 * 16 * (big ? 16 : 8);
    const int64_t oblk = (N + tpb - 1) / tpb;
    const dim3 og((unsigned)(B * (heads / hp) * oblk));
    dispatch_int(hp, HeadsPerBlock{}, [&](auto HP) {
        dispatch_int(big ? 16 : 8, std::integer_sequence<int, 8, 16>{}, [&](auto TPW) {
            hipLaunchKernelGGL((k_la_out<decltype(HP)::value, decltype(TPW)::value>), og, dim3(256), 0, st,
                               (const unsigned short*)q, ld, hstride, (int)heads, (int)N, (int)oblk, relu_qk,
                               (const float*)kvsum, (unsigned short*)out, ldo);
        });
    });
    EGG_CHECK_LAUNCH("linear_attention_out");
    return EGGROLL_OK;
}
