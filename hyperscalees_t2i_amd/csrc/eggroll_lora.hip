// libeggroll — (2) population-batched perturbed LoRA linear for gfx950 (MI355X).
//
// Replaces, for all members of one rank at once, the reference's per-member
//   unflatten_to_params(theta + sigma*eps[k])  (unifed_es.py:160-161, utills.py:155-162)
//   PEFT lora.Linear: y = x W^T + bias + (alpha/r) * (x A_k^T) B_k^T   (es_backend.py:193-200)
// Rows of X are stacked member-major, so the frozen base weight W streams through LDS once
// per M-tile for every member instead of once per member-forward.
//
//   k_lora_project : T[row, q] = X[row,:] . A_k[q,:]   (fp32; HBM-bound X read)
//   k_lora_gemm    : Y = X W^T (bf16 MFMA 16x16x32, 128x128x64 tiles, global_load_lds staging,
//                    XOR-swizzled LDS, 2-stage pipeline) with the epilogue
//                    + bias[n] + scale * sum_q T[row,q] * B_k[n,q]
//   k_lora_expand  : Y += scale * T B_k^T  (for hosts that run the base GEMM elsewhere)
//   k_lora_gemm8   : the same GEMM on the 8-phase ring (p8.h), 256 x 256 and 256 x 320 tiles
#include <algorithm>
#include <utility>
#include "p8_epilogue.h"

namespace eggroll {

// ------------------------------------------------------------------------------------
// T = X A_k^T : one wave per row, 16-byte X loads, fp32 accumulate, wave reduction.
// ------------------------------------------------------------------------------------
template <int R>
__global__ __launch_bounds__(256) void k_lora_project(const unsigned short* __restrict__ X, int64_t ldx,
                                                      const float* __restrict__ theta_pop, int64_t ld_theta,
                                                      int64_t offA, int64_t rows_per_member, int64_t M, int64_t K,
                                                      float* __restrict__ T) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const int64_t kl = row / rows_per_member;
    const float* A = theta_pop + kl * ld_theta + offA;
    const unsigned short* x = X + row * ldx;
    float acc[R];
#pragma unroll
    for (int q = 0; q < R; ++q) acc[q] = 0.0f;
    for (int64_t c = lane * 8; c < K; c += 64 * 8) {
        const u16x8 xv = *reinterpret_cast<const u16x8*>(x + c);
        float xf[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) xf[t] = bf16_to_f32(xv[t]);
#pragma unroll
        for (int q = 0; q < R; ++q) {
            const float4 a0 = *reinterpret_cast<const float4*>(A + q * K + c);
            const float4 a1 = *reinterpret_cast<const float4*>(A + q * K + c + 4);
            acc[q] += xf[0] * a0.x + xf[1] * a0.y + xf[2] * a0.z + xf[3] * a0.w + xf[4] * a1.x + xf[5] * a1.y +
                      xf[6] * a1.z + xf[7] * a1.w;
        }
    }
#pragma unroll
    for (int q = 0; q < R; ++q) {
        const float v = wave_sum(acc[q]);
        if (lane == 0) T[row * R + q] = v;
    }
}

// Register-resident-A variant (R <= 2, K <= 512 NI): each wave keeps its member's A_k slice
// (NI x 8 columns x R per lane) in VGPRs and sweeps PR_ROWS rows, two rows' X loads in flight at a
// time — the per-row A re-reads of k_lora_project (4 float4 A loads per X load) are gone, so the
// kernel issues almost only the X stream.  Same lane->column map and summation order as
// k_lora_project: bit-identical T.
constexpr int PR_ROWS = 8;  // rows per wave

template <int R, int NI>
__global__ __launch_bounds__(256) void k_lora_project_ra(const unsigned short* __restrict__ X, int64_t ldx,
                                                         const float* __restrict__ theta_pop, int64_t ld_theta,
                                                         int64_t offA, int64_t rows_per_member, int64_t M, int64_t K,
                                                         float* __restrict__ T) {
    const int lane = threadIdx.x & 63;
    const int64_t row0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * PR_ROWS;
    if (row0 >= M) return;
    const int64_t row_end = row0 + PR_ROWS < M ? row0 + PR_ROWS : M;
    int64_t cur = -1;
    float a[NI][R][8];
    auto load_a = [&](int64_t kl) {
        const float* A = theta_pop + kl * ld_theta + offA;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int64_t c = lane * 8 + 512 * i;
#pragma unroll
            for (int q = 0; q < R; ++q) {
                float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f), a1 = a0;
                if (c < K) {
                    a0 = *reinterpret_cast<const float4*>(A + q * K + c);
                    a1 = *reinterpret_cast<const float4*>(A + q * K + c + 4);
                }
                a[i][q][0] = a0.x; a[i][q][1] = a0.y; a[i][q][2] = a0.z; a[i][q][3] = a0.w;
                a[i][q][4] = a1.x; a[i][q][5] = a1.y; a[i][q][6] = a1.z; a[i][q][7] = a1.w;
            }
        }
    };
    for (int64_t row = row0; row < row_end; row += 2) {
        const bool two = row + 1 < row_end;
        u16x8 xv[2][NI];
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                const int64_t c = lane * 8 + 512 * i;
                xv[h][i] = (c < K && (h == 0 || two)) ? *reinterpret_cast<const u16x8*>(X + (row + h) * ldx + c)
                                                      : u16x8{0, 0, 0, 0, 0, 0, 0, 0};
            }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (h == 1 && !two) break;
            const int64_t kl = (row + h) / rows_per_member;
            if (kl != cur) {  // wave-uniform: only at member boundaries
                load_a(kl);
                cur = kl;
            }
            float acc[R];
#pragma unroll
            for (int q = 0; q < R; ++q) acc[q] = 0.0f;
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                if (lane * 8 + 512 * i >= K) break;
                float xf[8];
#pragma unroll
                for (int t = 0; t < 8; ++t) xf[t] = bf16_to_f32(xv[h][i][t]);
#pragma unroll
                for (int q = 0; q < R; ++q)
                    acc[q] += xf[0] * a[i][q][0] + xf[1] * a[i][q][1] + xf[2] * a[i][q][2] + xf[3] * a[i][q][3] +
                              xf[4] * a[i][q][4] + xf[5] * a[i][q][5] + xf[6] * a[i][q][6] + xf[7] * a[i][q][7];
            }
#pragma unroll
            for (int q = 0; q < R; ++q) {
                const float v = wave_sum(acc[q]);
                if (lane == 0) T[(row + h) * R + q] = v;
            }
        }
    }
}

// ------------------------------------------------------------------------------------
// Multi-linear projection on MFMA: T_l[row, q] = X[row,:] . A_{k,l}[q,:] for n_lin LoRA linears that
// read the SAME X (Sana attn1 to_q / to_k / to_v, attn2 to_k / to_v): X streams from HBM once instead
// of once per linear.  As a GEMM it is [M x K] x [K x 16]: the B operand holds the NQ = n_lin * r
// rows of A as bf16 hi / lo pairs (columns q and NQ + q: hi = bf16(a), lo = bf16(a - hi), so
// hi + lo carries a to ~2^-16 relative), X is the A operand straight from global memory, fp32
// accumulation.  The reduction over K is order-free, so K is permuted to make every lane's X read
// contiguous: in each 128-column group lane-group h = lane >> 4 owns columns [h*32, h*32 + 32) as
// four 16-byte pieces, piece j feeding MFMA k-step j; the B image in LDS uses the same permutation
// (a K % 128 tail runs in the plain 8-column layout).  The B image of the block's member is built in
// LDS once (K * 32 bytes); each wave runs two 16-row groups (32 rows, 8 KiB of X in flight) per pass.
//   img[s][lane] = 8 bf16: column n = lane & 15, K-columns col(s, lane >> 4, 0..7).
// ------------------------------------------------------------------------------------
constexpr int PM_ROWS_PER_BLOCK = 256;  // 4 waves x 2 groups x 16 rows x 2 passes

__device__ __forceinline__ int64_t pm_col(int s, int h, int64_t ng) {
    // first of the 8 consecutive K-columns of k-step s held by lane-group h
    return s < 4 * ng ? (int64_t)(s >> 2) * 128 + h * 32 + (s & 3) * 8 : ng * 128 + (int64_t)(s - 4 * ng) * 32 + h * 8;
}

template <int NQ>
__global__ __launch_bounds__(256) void k_lora_project_mfma(const unsigned short* __restrict__ X, int64_t ldx,
                                                           const float* __restrict__ theta_pop, int64_t ld_theta,
                                                           int64_t offA0, int64_t offA1, int64_t offA2,
                                                           int64_t offA3, int r, int64_t rows_per_member,
                                                           int64_t M, int64_t K, float* __restrict__ T) {
    extern __shared__ __attribute__((aligned(16))) char pm_smem[];
    bf16x8* img = reinterpret_cast<bf16x8*>(pm_smem);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int h = lane >> 4, n = lane & 15;
    const int nsteps = (int)(K / 32);
    const int64_t ng = K / 128;
    const int64_t r0 = (int64_t)blockIdx.x * PM_ROWS_PER_BLOCK;
    const int64_t r1 = r0 + PM_ROWS_PER_BLOCK < M ? r0 + PM_ROWS_PER_BLOCK : M;
    const int64_t kl_first = r0 / rows_per_member, kl_last = (r1 - 1) / rows_per_member;
    for (int64_t kl = kl_first; kl <= kl_last; ++kl) {
        // ---- B image of member kl: entry (s, ln) = 8 bf16 of column ln & 15 ----
        if (kl != kl_first) __syncthreads();  // every wave is done with the previous image
        for (int e = threadIdx.x; e < nsteps * 64; e += 256) {
            const int s = e >> 6, ln = e & 63, cn = ln & 15;
            bf16x8 v;
            if (cn < 2 * NQ) {
                const int q = cn < NQ ? cn : cn - NQ, l = q / r, qq = q - l * r;
                const int64_t off = l == 0 ? offA0 : l == 1 ? offA1 : l == 2 ? offA2 : offA3;
                const float* a = theta_pop + kl * ld_theta + off + (int64_t)qq * K + pm_col(s, ln >> 4, ng);
                const float4 a0 = *reinterpret_cast<const float4*>(a);
                const float4 a1 = *reinterpret_cast<const float4*>(a + 4);
                const float av[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
#pragma unroll
                for (int t = 0; t < 8; ++t) {
                    const __bf16 hi = (__bf16)av[t];
                    v[t] = cn < NQ ? hi : (__bf16)(av[t] - (float)hi);
                }
            } else {
#pragma unroll
                for (int t = 0; t < 8; ++t) v[t] = (__bf16)0.0f;
            }
            img[e] = v;
        }
        __syncthreads();
        const int64_t mlo = kl * rows_per_member > r0 ? kl * rows_per_member : r0;
        const int64_t mhi = (kl + 1) * rows_per_member < r1 ? (kl + 1) * rows_per_member : r1;
        for (int64_t g0 = r0 + wave * 32; g0 < r1; g0 += 4 * 32) {
            if (g0 + 32 <= mlo || g0 >= mhi) continue;  // wave-uniform: no row of this pass in member kl
            const int64_t ra = g0 + n, rb = g0 + 16 + n;
            const bool va = ra >= mlo && ra < mhi, vb = rb >= mlo && rb < mhi;
            const unsigned short* xa = X + (va ? ra : mlo) * ldx + h * 32;
            const unsigned short* xb = X + (vb ? rb : mlo) * ldx + h * 32;
            f32x4 acc_a = {0.f, 0.f, 0.f, 0.f}, acc_b = acc_a;
            const u16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
            u16x8 ca[4], cb[4];
            if (ng > 0) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    ca[j] = va ? *reinterpret_cast<const u16x8*>(xa + j * 8) : z;
                    cb[j] = vb ? *reinterpret_cast<const u16x8*>(xb + j * 8) : z;
                }
            }
            for (int64_t G = 0; G < ng; ++G) {
                u16x8 na[4], nb[4];
                const bool more = G + 1 < ng;
#pragma unroll
                for (int j = 0; j < 4; ++j) {  // next group's X in flight under this group's MFMAs
                    na[j] = (more && va) ? *reinterpret_cast<const u16x8*>(xa + (G + 1) * 128 + j * 8) : z;
                    nb[j] = (more && vb) ? *reinterpret_cast<const u16x8*>(xb + (G + 1) * 128 + j * 8) : z;
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const bf16x8 bfr = img[(G * 4 + j) * 64 + lane];
                    acc_a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, ca[j]), bfr, acc_a,
                                                                    0, 0, 0);
                    acc_b = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, cb[j]), bfr, acc_b,
                                                                    0, 0, 0);
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    ca[j] = na[j];
                    cb[j] = nb[j];
                }
            }
            for (int s = (int)(4 * ng); s < nsteps; ++s) {  // K % 128 tail, plain layout
                const int64_t c = pm_col(s, h, ng) - h * 32;
                const u16x8 xa8 = va ? *reinterpret_cast<const u16x8*>(xa + c) : z;
                const u16x8 xb8 = vb ? *reinterpret_cast<const u16x8*>(xb + c) : z;
                const bf16x8 bfr = img[s * 64 + lane];
                acc_a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, xa8), bfr, acc_a, 0, 0, 0);
                acc_b = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, xb8), bfr, acc_b, 0, 0, 0);
            }
            // D[4h + i][n]: T[q] = D[q] (hi) + D[NQ + q] (lo), joined across lanes n and n + NQ
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float ta = acc_a[i] + __shfl(acc_a[i], (lane + NQ) & 63, 64);
                const float tb = acc_b[i] + __shfl(acc_b[i], (lane + NQ) & 63, 64);
                if (n < NQ) {
                    const int l = n / r, qq = n - l * r;
                    float* Tl = T + (int64_t)l * M * r;
                    const int64_t rowa = g0 + 4 * h + i, rowb = g0 + 16 + 4 * h + i;
                    if (rowa >= mlo && rowa < mhi) Tl[rowa * r + qq] = ta;
                    if (rowb >= mlo && rowb < mhi) Tl[rowb * r + qq] = tb;
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------
// Base GEMM + fused LoRA epilogue on the one-barrier tile (kernel 128):
//   BM x BN = 128 x 128 output tile, BK = 64, WM x WN = 2 x 2 waves (wave tile 64 x 64), 2 LDS stages
//   of (BM + BN) rows x 128 B (64 KiB, 2 blocks/CU), one barrier per K-tile: the global_load_lds of
//   K-tile k+1 is issued right after the barrier and lands while the MFMAs of K-tile k run.
// ------------------------------------------------------------------------------------
struct T128 {
    static constexpr int BM = 128, BN = 128, WM = 2, WN = 2;
    static constexpr int WAVES = WM * WN, THREADS = 64 * WAVES;
    static constexpr int WTM = BM / WM, WTN = BN / WN;   // wave tile
    static constexpr int FM = WTM / 16, FN = WTN / 16;   // 16x16 fragments per wave
    static constexpr int A_BYTES = BM * BK * 2, B_BYTES = BN * BK * 2;
    static constexpr int STAGE = A_BYTES + B_BYTES;
    static constexpr int LDS = 2 * STAGE;
    static constexpr int GA = BM / 8 / WAVES, GB = BN / 8 / WAVES;   // glds per wave per K-tile
    static_assert(BM % (8 * WAVES) == 0 && BN % (8 * WAVES) == 0, "staging split");
    static_assert(WTM * WTN * 2 <= LDS / WAVES, "epilogue staging must fit");
};

// Stage `nglds` x 8 rows of a K-contiguous bf16 matrix into an LDS tile.  LDS image: row r at
// byte 128*r; 16-B slot s' of row r holds global chunk s' ^ (r & 7)  (conflict-free b128
// fragment reads).  One global_load_lds_dwordx4 = 1 KiB = 8 rows.
template <int NG>
__device__ __forceinline__ void stage_rows(const unsigned short* __restrict__ G, int64_t ld, int64_t row0,
                                           int64_t row_max, int64_t k0, char* lds_tile, int wave, int lane) {
#pragma unroll
    for (int i = 0; i < NG; ++i) {
        const int R0 = (wave * NG + i) * 8;
        const int r = R0 + (lane >> 3);
        const int chunk = (lane & 7) ^ (r & 7);
        int64_t gr = row0 + r;
        gr = gr < row_max ? gr : row_max;  // clamp: rows past the end are never stored
        const unsigned short* src = G + gr * ld + k0 + chunk * 8;
        __builtin_amdgcn_global_load_lds((gbl_void*)src, (lds_void*)(lds_tile + R0 * 128), 16, 0, 0);
    }
}

__device__ __forceinline__ bf16x8 read_frag(const char* lds_tile, int row, int chunk) {
    return *reinterpret_cast<const bf16x8*>(lds_tile + row * 128 + ((chunk ^ (row & 7)) << 4));
}

// The VALU epilogue of k_lora_gemm and of k_lora_gemm8's MF = false path: + bias[n] + scale *
// T[row,:] . B_k[n,:], bf16 via a per-wave LDS staging tile (WTM rows of WTN*2 bytes, 16-B slots
// XOR-swizzled by row), 16-B stores.  The LoRA term is added row by row so accumulators retire as
// they are written.  BMtile: rows of the workgroup tile (one member's B_k serves it unless it straddles).
template <int R, int WTM, int WTN>
__device__ __forceinline__ void lora_epilogue(f32x4 (&acc)[WTM / 16][WTN / 16], char* smem, int wave, int lane,
                                              int m0, int n0, int rbase, int cbase, const unsigned short* __restrict__ bias,
                                              const float* __restrict__ T, const float* __restrict__ theta_pop,
                                              int64_t ld_theta, int64_t offB, float scale, int rows_per_member,
                                              int BMtile, int M, int N, unsigned short* __restrict__ Y, int64_t ldy) {
    constexpr int FM = WTM / 16, FN = WTN / 16;
    const int col_l = lane & 15, rq = (lane >> 4) * 4;
    float bv[FN];
    int colv[FN];
#pragma unroll
    for (int j = 0; j < FN; ++j) {
        const int col = n0 + cbase + j * 16 + col_l;
        colv[j] = col < N ? col : N - 1;
        bv[j] = bias ? bf16_to_f32(bias[colv[j]]) : 0.0f;
    }
    constexpr int ROWB = WTN * 2, SLOTS = ROWB / 16;
    char* ctile = smem + wave * (WTM * ROWB);
    float bk[FN][R > 0 ? R : 1];
    bool one_member = true;
    if constexpr (R > 0) {
        const int first = m0 / rows_per_member;
        const int last_row = (m0 + BMtile - 1 < M ? m0 + BMtile - 1 : M - 1);
        one_member = (last_row / rows_per_member) == first;
        const float* Bk = theta_pop + (int64_t)first * ld_theta + offB;
#pragma unroll
        for (int j = 0; j < FN; ++j)
#pragma unroll
            for (int qq = 0; qq < R; ++qq) bk[j][qq] = Bk[colv[j] * R + qq];
    }
#pragma unroll
    for (int i = 0; i < FM; ++i) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int rr = i * 16 + rq + e;
            float add[FN];
#pragma unroll
            for (int j = 0; j < FN; ++j) add[j] = bv[j];
            if constexpr (R > 0) {
                int row = m0 + rbase + rr;
                row = row < M ? row : M - 1;
                float t[R];
#pragma unroll
                for (int qq = 0; qq < R; ++qq) t[qq] = T[(int64_t)row * R + qq];
                if (!one_member) {
                    const float* Bk = theta_pop + (int64_t)(row / rows_per_member) * ld_theta + offB;
#pragma unroll
                    for (int j = 0; j < FN; ++j)
#pragma unroll
                        for (int qq = 0; qq < R; ++qq) bk[j][qq] = Bk[colv[j] * R + qq];
                }
#pragma unroll
                for (int j = 0; j < FN; ++j) {
                    float d = 0.0f;
#pragma unroll
                    for (int qq = 0; qq < R; ++qq) d += t[qq] * bk[j][qq];
                    add[j] += scale * d;
                }
            }
#pragma unroll
            for (int j = 0; j < FN; ++j) {
                const int cc = j * 16 + col_l;
                const int slot = (cc >> 3) ^ (rr & (SLOTS - 1));
                *reinterpret_cast<unsigned short*>(ctile + rr * ROWB + slot * 16 + (cc & 7) * 2) =
                    f32_to_bf16(acc[i][j][e] + add[j]);
            }
        }
    }
    __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): this wave's LDS writes done (wave-private tile)
    constexpr int ROWS_PER_IT = 64 / SLOTS;
#pragma unroll
    for (int it = 0; it < WTM / ROWS_PER_IT; ++it) {
        const int rr = it * ROWS_PER_IT + lane / SLOTS, sl = lane % SLOTS;
        const int row = m0 + rbase + rr;
        const int col = n0 + cbase + sl * 8;
        if (row >= M || col >= N) continue;
        const u16x8 v = *reinterpret_cast<const u16x8*>(ctile + rr * ROWB + ((sl ^ (rr & (SLOTS - 1))) << 4));
        unsigned short* dst = Y + (int64_t)row * ldy + col;
        if (col + 8 <= N && (((uintptr_t)dst) & 15) == 0) {
            *reinterpret_cast<u16x8*>(dst) = v;
        } else {
            for (int u = 0; u < 8 && col + u < N; ++u) dst[u] = v[u];
        }
    }
}

template <int R>
__global__ __launch_bounds__(T128::THREADS, 2) void k_lora_gemm(
    const unsigned short* __restrict__ X, int64_t ldx, const unsigned short* __restrict__ W, int64_t ldw,
    const unsigned short* __restrict__ bias, const float* __restrict__ T, const float* __restrict__ theta_pop,
    int64_t ld_theta, int64_t offB, float scale, int rows_per_member, int M, int N, int64_t K, int tiles_n,
    unsigned short* __restrict__ Y, int64_t ldy) {
    using TL = T128;
    constexpr int FM = TL::FM, FN = TL::FN;
    __shared__ __attribute__((aligned(16))) char smem[TL::LDS];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / TL::WN, wn = wave % TL::WN;
    const TileIdx ti = p8_tile_index<TL::BM>(M, tiles_n);
    const int m0 = ti.m * TL::BM, n0 = ti.n * TL::BN;

    f32x4 acc[FM][FN];
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int nk = (int)(K / BK);
    stage_rows<TL::GA>(X, ldx, m0, M - 1, 0, smem, wave, lane);
    stage_rows<TL::GB>(W, ldw, n0, N - 1, 0, smem + TL::A_BYTES, wave, lane);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const char* cur = smem + (kt & 1) * TL::STAGE;
        if (kt + 1 < nk) {
            char* nxt = smem + ((kt + 1) & 1) * TL::STAGE;
            stage_rows<TL::GA>(X, ldx, m0, M - 1, (int64_t)(kt + 1) * BK, nxt, wave, lane);
            stage_rows<TL::GB>(W, ldw, n0, N - 1, (int64_t)(kt + 1) * BK, nxt + TL::A_BYTES, wave, lane);
        }
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const int ch = kk * 4 + (lane >> 4);
            bf16x8 b[FN];
#pragma unroll
            for (int f = 0; f < FN; ++f) b[f] = read_frag(cur + TL::A_BYTES, wn * TL::WTN + f * 16 + (lane & 15), ch);
            bf16x8 a[FM];
#pragma unroll
            for (int f = 0; f < FM; ++f) a[f] = read_frag(cur, wm * TL::WTM + f * 16 + (lane & 15), ch);
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int i = 0; i < FM; ++i)
#pragma unroll
                for (int j = 0; j < FN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
            __builtin_amdgcn_s_setprio(0);
        }
        __syncthreads();
    }
    lora_epilogue<R, TL::WTM, TL::WTN>(acc, smem, wave, lane, m0, n0, wm * TL::WTM, wn * TL::WTN, bias, T, theta_pop,
                                       ld_theta, offB, scale, rows_per_member, TL::BM, M, N, Y, ldy);
}

// Epilogue operands of the MFMA LoRA addend, prefetched into LDS (after the 128 KiB ring) by
// 4-byte LDS-DMAs issued before the GEMM prologue — the prologue's counted vmcnt retires them, so
// the epilogue reads LDS instead of waiting on dependent global loads after the last MFMA:
// T rows [m0, m0 + 256) x R, B_k columns [n0, n0 + 256) x R of the tile's first member (and of the
// next one when the tile straddles two), bias[n0, n0 + 256).  Out-of-range bytes read as 0.
// (256 and n0 + 256 above stand for the tile: BM rows, BN columns.)  Layout of the block, from the
// geometry: T rows, B_k columns of the tile's members a / a + 1, bias; every piece is fetched in
// 256-byte wave-DMAs, so the bias takes BN * 2 / 256 waves, rounded up (2 for 256 columns, 3 for 320).
template <class G>
struct EpiBlock {
    static constexpr int T = 0, B0 = G::BM * 2 * 4, B1 = B0 + G::BN * 2 * 4, BIAS = B1 + G::BN * 2 * 4;
    static constexpr int BIAS_WAVES = (G::BN * 2 + 255) / 256, BYTES = BIAS + BIAS_WAVES * 256;
};

template <class G, int R>
__device__ __forceinline__ void epi_prefetch(char* ep, int wave, int lane, int m0, int n0, int M, int N,
                                             const float* __restrict__ T, const float* __restrict__ theta_pop,
                                             int64_t ld_theta, int64_t offB, const unsigned short* __restrict__ bias,
                                             int rows_per_member) {
    static_assert(R >= 0 && R <= 2, "MFMA addend: r <= 2");
    using E = EpiBlock<G>;
    const uint32_t vo = lane * 4;
    if constexpr (R > 0) {
        constexpr int TB = G::BM * R * 4, BB = G::BN * R * 4;  // bytes of the tile's T rows / B_k columns
        if (wave * 256 < TB) {
            const __amdgpu_buffer_rsrc_t rt = __builtin_amdgcn_make_buffer_rsrc(
                (void*)(T + (int64_t)m0 * R), (short)0, (int)((int64_t)(M - m0) * R * 4), 0x00020000);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rt, (lds_void*)(ep + E::T + wave * 256), 4, vo, wave * 256, 0, 0);
        }
#pragma unroll
        for (int p = 0; p < (BB + 2047) / 2048; ++p) {
            const int pc = wave + 8 * p;
            if (pc * 256 < BB) {
                const int ma = m0 / rows_per_member;
                const int nrec = (N - n0) * R * 4;
                const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc(
                    (void*)(theta_pop + (int64_t)ma * ld_theta + offB + (int64_t)n0 * R), (short)0, nrec, 0x00020000);
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rb, (lds_void*)(ep + E::B0 + pc * 256), 4, vo, pc * 256, 0, 0);
                const int last = m0 + G::BM - 1 < M ? m0 + G::BM - 1 : M - 1;
                if (last / rows_per_member != ma) {
                    const __amdgpu_buffer_rsrc_t rb1 = __builtin_amdgcn_make_buffer_rsrc(
                        (void*)(theta_pop + (int64_t)(ma + 1) * ld_theta + offB + (int64_t)n0 * R), (short)0, nrec,
                        0x00020000);
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(rb1, (lds_void*)(ep + E::B1 + pc * 256), 4, vo, pc * 256, 0,
                                                             0);
                }
            }
        }
    }
    if (bias && wave < E::BIAS_WAVES) {
        // the range check is per 4-byte access: with an odd column count the dword holding the last bias
        // would be cut by a 2-byte-granular limit and read as 0, so the limit covers that whole dword (its
        // upper half, bias[N], belongs to no stored column)
        const __amdgpu_buffer_rsrc_t rz = __builtin_amdgcn_make_buffer_rsrc((void*)(bias + n0), (short)0,
                                                                            ((N - n0) * 2 + 3) & ~3, 0x00020000);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rz, (lds_void*)(ep + E::BIAS + wave * 256), 4, vo, wave * 256, 0, 0);
    }
}

// lora_mfma_addend with every operand read from the prefetched LDS block (same k-slot layout).
// Branch-free: every lane reads its candidate operands (all inside the LDS block) back to back under
// one lgkmcnt wait, and a lane whose k-slot block is not its row's / column's member keeps zeros by
// select — divergent ifs around the reads serialised eight LDS round trips.  A row's member offset is
// one compare against the tile-local start of the next member (the tile spans at most two).
template <class G, int R>
__device__ __forceinline__ void lora_mfma_addend_lds(f32x4 (&acc)[8][G::NF], int lane, int m0, int rbase, int cbase,
                                                     const char* ep, bool has_bias, float scale, int rows_per_member,
                                                     int M) {
    using E = EpiBlock<G>;
    constexpr int NF = G::NF;
    const int h = lane >> 4, l16 = lane & 15;
    const int ma = m0 / rows_per_member;
    const int last = (m0 + G::BM - 1 < M ? m0 + G::BM - 1 : M - 1);
    const bool straddle = last / rows_per_member != ma;
    const int bnd = (ma + 1) * rows_per_member - m0;  // tile-local first row of member a + 1
    const float* Tl = reinterpret_cast<const float*>(ep + E::T);
    const unsigned short* bl = reinterpret_cast<const unsigned short*>(ep + E::BIAS);
    const float* Bk = reinterpret_cast<const float*>(ep + (h == 1 ? E::B1 : E::B0));
    const bool con = h == 0 || (h == 1 && straddle);
    float bv[NF][R > 0 ? R : 1], tv[8][R > 0 ? R : 1];
    unsigned short bb[NF];
#pragma unroll
    for (int j = 0; j < NF; ++j) {
        const int c = cbase + j * 16 + l16;  // tile-local column
#pragma unroll
        for (int q = 0; q < R; ++q) bv[j][q] = Bk[c * R + q];
        bb[j] = bl[c];
    }
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int q = 0; q < R; ++q) tv[i][q] = Tl[(rbase + i * 16 + l16) * R + q];
    bf16x8 rf[NF];
#pragma unroll
    for (int j = 0; j < NF; ++j) {
        short v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int q = 0; q < R; ++q) {
            const float sb = scale * bv[j][q];
            const short hi = bf16_bits(sb);
            v[q] = hi;
            v[R + q] = hi;
            v[2 * R + q] = bf16_bits(sb - bf16_to_f32((unsigned short)hi));
        }
        v[3 * R] = has_bias ? (short)bb[j] : (short)0;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = con ? v[e] : (short)0;
        rf[j] = *reinterpret_cast<bf16x8*>(v);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int rl = rbase + i * 16 + l16;  // tile-local row
        const bool ron = h == (rl >= bnd ? 1 : 0);
        short v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int q = 0; q < R; ++q) {
            const float t = tv[i][q];
            const short th = bf16_bits(t);
            v[q] = th;
            v[R + q] = bf16_bits(t - bf16_to_f32((unsigned short)th));
            v[2 * R + q] = th;
        }
        v[3 * R] = (short)0x3F80;  // 1.0
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = ron ? v[e] : (short)0;
        const bf16x8 lf = *reinterpret_cast<bf16x8*>(v);
#pragma unroll
        for (int j = 0; j < NF; ++j)  // transposed fragments (TR main loop): D[n][m]
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(rf[j], lf, acc[i][j], 0, 0, 0);
    }
}

// ------------------------------------------------------------------------------------
// 256 x 320 variant of the 8-phase kernel (kernel 10): the same schedule, 8 waves (2 M x 4 N), each
// wave a 128 x 80 sub-tile = 8 x 5 fragments of 16 x 16.  The N side of a K-tile is split into two
// LDS regions by fragment column: B0 = n-fragments 0-2 of every wave column (192 rows, 3 DMAs per
// wave), B1 = n-fragments 3-4 (128 rows, 2 DMAs); A0 / A1 as in k_lora_gemm8.  Quadrant order
// (0,0) (0,1) (1,1) (1,0) = 24, 16, 16, 24 MFMAs.  Why: per 64-deep K-tile the ring moves
// (256 + 320) x 128 B = 72 KiB for 2,560 MFMA cycles per SIMD (28.1 B/cycle/CU) instead of 64 KiB for
// 2,048 (32 B/cycle/CU) — the 256 x 256 main loop is bound by the per-CU LDS-DMA fill rate (28-30
// B/cycle/CU measured), so 10 % fewer fill bytes per MFMA; 2240 and 11200 (the Sana
// widths) are multiples of 320, so the 256-wide tiling's 2.8 % of padded columns at N = 2240 go away;
// and the per-tile prologue / addend / C tile amortise over 25 % more MFMAs.  Ring: 2 x 72 KiB.
// vmcnt: the waits retire everything older than the last three half-tiles issued (A0, B1, A1 of
// the next-but-one K-tile = 6 DMAs) exactly as in k_lora_gemm8; the early-first-K-tile waits in
// phases 1 and 2 count 11 (B0 carries 3 DMAs).  Every output element accumulates the same MFMAs in
// the same k order as k_lora_gemm8, so the two kernels are bit-identical.
// ------------------------------------------------------------------------------------

// C tile of the 256 x 320 workgroup tile, staged through ONE shared LDS tile (256 rows x 640 B = all
// 160 KiB; the caller has passed a barrier after the epilogue block's last read) so that the global
// stores write whole 128-B lines: with per-wave staging each wave's 80-column row segment (160 B)
// straddles lines shared with the neighbouring wave and the store phase took 2x the 256 x 256
// kernel's per byte (stamped).  16-B slots are rotated by row ((slot + row) mod 40): the
// 8-B fragment writes are at most 2-way bank-conflicted.  After a barrier, wave w stores rows
// [32w, 32w + 32): 40 lanes per 640-B row, 20 16-B stores per lane.  EPI ops as store_tile_t.
template <int EPI = EPI_NONE>
__device__ __forceinline__ void store_tile_wg(f32x4 (&acc)[8][5], char* smem, int wave, int lane, int m0, int n0,
                                              int wm, int wn, int M, int N, unsigned short* __restrict__ Y,
                                              int64_t ldy, const EpiArgs& ea = EpiArgs{}) {
    constexpr int RB = 640, SL = 40;
    const int r_l = lane & 15, c_l = (lane >> 4) * 4;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int rr = wm * 128 + i * 16 + r_l;
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            u16x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = f32_to_bf16(acc[i][j][e]);
            const int c = wn * 80 + j * 16 + c_l;  // tile column: 16-B slot c >> 3, 8-B half (c >> 2) & 1
            *reinterpret_cast<u16x4*>(smem + rr * RB + ((c >> 3) + rr) % SL * 16 + ((c >> 2) & 1) * 8) = o;
        }
    }
    __syncthreads();
    constexpr bool E32 = EPI == EPI_RES32 || EPI == EPI_GATED32;
    const bool vec = (ldy & 7) == 0 && (((uintptr_t)Y) & 15) == 0 &&
                     (EPI == EPI_NONE || EPI == EPI_SILU || EPI == EPI_GELU || EPI == EPI_GELU_ERF ||
                      ((ea.ldr & 7) == 0 && (((uintptr_t)ea.res) & 15) == 0 &&
                       ((EPI != EPI_GATED && EPI != EPI_GATED32) ||
                        ((ea.gstride & 7) == 0 && (((uintptr_t)ea.gate) & 15) == 0))));
    if constexpr (E32) {
        // fp32 residual stream: per group of 5 chunks, every residual (and gate) load issued before any
        // store (one load -> fma -> store per chunk serialises the loads behind the earlier stores)
        float* rb = const_cast<float*>(reinterpret_cast<const float*>(ea.res));
        const float* gb = reinterpret_cast<const float*>(ea.gate);
#pragma unroll
        for (int h = 0; h < 20; h += 5) {
            u16x8 v[5];
            float4 rv[5][2], gv[5][2];
            int rows[5], cols[5];
            bool ok[5];
#pragma unroll
            for (int it = 0; it < 5; ++it) {
                const int idx = (h + it) * 64 + lane, rr = wave * 32 + idx / SL, ch = idx % SL;
                v[it] = *reinterpret_cast<const u16x8*>(smem + rr * RB + (ch + rr) % SL * 16);
                rows[it] = m0 + rr;
                cols[it] = n0 + ch * 8;
                ok[it] = rows[it] < M && cols[it] + 8 <= N && vec;
                if (ok[it]) {
                    const float* r = rb + (int64_t)rows[it] * ea.ldr + cols[it];
                    rv[it][0] = *reinterpret_cast<const float4*>(r);
                    rv[it][1] = *reinterpret_cast<const float4*>(r + 4);
                    if constexpr (EPI == EPI_GATED32) {
                        const float* g = gb + (int64_t)(rows[it] / ea.rpg) * ea.gstride + cols[it];
                        gv[it][0] = *reinterpret_cast<const float4*>(g);
                        gv[it][1] = *reinterpret_cast<const float4*>(g + 4);
                    }
                }
            }
#pragma unroll
            for (int it = 0; it < 5; ++it) {
                const int row = rows[it], col = cols[it];
                if (row >= M || col >= N) continue;
                if (!ok[it]) {   // ragged tail / unaligned: the element form
                    for (int u = 0; u < 8 && col + u < N; ++u) epi_store32_1<EPI>(v[it][u], row, col + u, ea, Y, ldy);
                    continue;
                }
                float x[8] = {rv[it][0].x, rv[it][0].y, rv[it][0].z, rv[it][0].w,
                              rv[it][1].x, rv[it][1].y, rv[it][1].z, rv[it][1].w};
                if constexpr (EPI == EPI_GATED32) {
                    const float gg[8] = {gv[it][0].x, gv[it][0].y, gv[it][0].z, gv[it][0].w,
                                         gv[it][1].x, gv[it][1].y, gv[it][1].z, gv[it][1].w};
#pragma unroll
                    for (int u = 0; u < 8; ++u) x[u] = __builtin_fmaf(gg[u], bf16_to_f32(v[it][u]), x[u]);
                } else {
#pragma unroll
                    for (int u = 0; u < 8; ++u) x[u] = x[u] + bf16_to_f32(v[it][u]);
                }
                float* r = rb + (int64_t)row * ea.ldr + col;
                *reinterpret_cast<float4*>(r) = float4{x[0], x[1], x[2], x[3]};
                *reinterpret_cast<float4*>(r + 4) = float4{x[4], x[5], x[6], x[7]};
                if (Y) {
                    u16x8 o;
#pragma unroll
                    for (int u = 0; u < 8; ++u) o[u] = f32_to_bf16(x[u]);
                    *reinterpret_cast<u16x8*>(Y + (int64_t)row * ldy + col) = o;
                }
            }
        }
        return;
    }
#pragma unroll
    for (int h = 0; h < 20; h += 10) {
        u16x8 v[10];
#pragma unroll
        for (int it = 0; it < 10; ++it) {
            const int idx = (h + it) * 64 + lane, rr = wave * 32 + idx / SL, ch = idx % SL;
            v[it] = *reinterpret_cast<const u16x8*>(smem + rr * RB + (ch + rr) % SL * 16);
        }
#pragma unroll
        for (int it = 0; it < 10; ++it) {
            const int idx = (h + it) * 64 + lane, rr = wave * 32 + idx / SL, ch = idx % SL;
            const int row = m0 + rr, col = n0 + ch * 8;
            if (row >= M || col >= N) continue;
            unsigned short* dst = Y + (int64_t)row * ldy + col;
            if (vec && col + 8 <= N) {
                u16x8 w = v[it];
                if constexpr (EPI != EPI_NONE) w = epi_apply<EPI>(w, row, col, ea);
                *reinterpret_cast<u16x8*>(dst) = w;
            } else {
                for (int u = 0; u < 8 && col + u < N; ++u) dst[u] = epi_apply1<EPI>(v[it][u], row, col + u, ea);
            }
        }
    }
}

// The 8-phase LoRA GEMM over the geometry G: G8<2> = 256 x 256 (kernels 8 / 9), G8<2, 5> = 256 x 320
// (kernel 10, below).  MF: bias + LoRA term as the MFMA addend from the prefetched LDS block (r <= 2,
// rows_per_member >= 256, or r = 0), the fragments computed transposed; else the VALU lora_epilogue
// (256 x 256 only).  The C tile goes out per wave (store_tile_t) or, for the 320-column tile, through
// one workgroup-wide staging tile (store_tile_wg; DESIGN §5 says why).
template <class G, int R, bool MF, int EPI = EPI_NONE>
__global__ __launch_bounds__(512, 1) void k_lora_gemm8(
    const unsigned short* __restrict__ X, int64_t ldx, const unsigned short* __restrict__ W, int64_t ldw,
    const unsigned short* __restrict__ bias, const float* __restrict__ T, const float* __restrict__ theta_pop,
    int64_t ld_theta, int64_t offB, float scale, int rows_per_member, int M, int N, int64_t K, int tiles_n,
    unsigned short* __restrict__ Y, int64_t ldy, EpiArgs ea = EpiArgs{}) {
    static_assert(EPI == EPI_NONE || MF, "epilogue ops ride the MFMA-addend path");
    static_assert(G::BM == 256 && (MF || G::NF == 4), "VALU epilogue: the 128 x 64 wave tile only");
    constexpr bool WG = G::NF != 4;  // C tile staged by the whole workgroup
    constexpr int RING = G::LDS + (MF ? EpiBlock<G>::BYTES : 0);  // ring + epilogue block
    constexpr int CTILE = WG ? G::BM * G::BN * 2 : G::CSTAGE;
    __shared__ __attribute__((aligned(16))) char smem[RING > CTILE ? RING : CTILE];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;
    const TileIdx ti = p8_tile_index<G::BM>(M, tiles_n);
    const int m0 = ti.m * G::BM, n0 = ti.n * G::BN;
    EGG_STAMP_RT(6);
    EGG_STAMP(0);

    const Stage<G::NA> sA0 = make_stage_a<G, 0>(m0, M - 1, ldx, wave, lane);
    const Stage<G::NA> sA1 = make_stage_a<G, 1>(m0, M - 1, ldx, wave, lane);
    const Stage<G::NB0> sB0 = make_stage_b<G, 0>(n0, N - 1, ldw, wave, lane);
    const Stage<G::NB1> sB1 = make_stage_b<G, 1>(n0, N - 1, ldw, wave, lane);
    char* const e_buf = smem;
    char* const o_buf = smem + G::BUF;
    const __amdgpu_buffer_rsrc_t rX = __builtin_amdgcn_make_buffer_rsrc((void*)X, (short)0, 0x7fffffff, 0x00020000);
    const __amdgpu_buffer_rsrc_t rW = __builtin_amdgcn_make_buffer_rsrc((void*)W, (short)0, 0x7fffffff, 0x00020000);

    f32x4 acc[8][G::NF];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < G::NF; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    bf16x8 a[4][2], b[G::NF0][2];
    int oA[2], oB0[2], oB1[2];
    p8_frag_offsets(oA, wm * 64 + (lane & 15), lane);
    p8_frag_offsets(oB0, wn * G::PER0 + (lane & 15), lane);
    p8_frag_offsets(oB1, wn * G::PER1 + (lane & 15), lane);

    const int nk = (int)(K / BK);
    // K-tile byte offset; tiles past the end re-load the last K-tile (into regions nothing reads
    // again), so every phase issues the same DMAs and the vmcnt counts stay static.
    auto kb = [nk](int t) -> int { return (t < nk ? t : nk - 1) * (BK * 2); };
    if constexpr (MF)  // older than every ring DMA: the prologue's counted vmcnt retires it
        epi_prefetch<G, R>(smem + G::LDS, wave, lane, m0, n0, M, N, T, theta_pop, ld_theta, offB, bias, rows_per_member);
    // prologue: K-tile 0 complete, K-tile 1 minus its B0 region (issued in phase 1)
    issue(rX, sA0, 0, e_buf + G::RA0, wave);
    issue(rW, sB0, 0, e_buf + G::RB0, wave);
    issue(rW, sB1, 0, e_buf + G::RB1, wave);
    issue(rX, sA1, 0, e_buf + G::RA1, wave);
    issue(rX, sA0, kb(1), o_buf + G::RA0, wave);
    issue(rW, sB1, kb(1), o_buf + G::RB1, wave);
    issue(rX, sA1, kb(1), o_buf + G::RA1, wave);
    wait_vm<G::VMC0>();  // K-tile 0's A0 + B0 only (early first K-tile, see G8)
    P8_BAR();
    EGG_STAMP(1);
    if (wm == 1) P8_BAR();  // stagger: group 1 runs one barrier behind

    // Phase p restages the region last read in phase p-1 (quadrant order (0,0) (0,1) (1,1) (1,0)):
    //   1: B0 of t+1 (odd)  2: A0 of t+2  3: B1 of t+2  4: A1 of t+2 + vmcnt(VMC) retires t+1
    //   5: B0 of t+2 (even) 6: A0 of t+3  7: B1 of t+3  8: A1 of t+3 + vmcnt(VMC) retires t+2
    int t0 = 0;
    for (; t0 + 1 < nk; t0 += 2) {
        const int k1 = kb(t0 + 1), k2 = kb(t0 + 2), k3 = kb(t0 + 3);
        p8_phase<G, 0, 0, 0, false, true, MF>(acc, a, b, e_buf, oA, oB0, oB1, [&] { issue(rW, sB0, k1, o_buf + G::RB0, wave); });
        p8_phase<G, 0, 1, 1, false, true, MF>(acc, a, b, e_buf, oA, oB0, oB1, [&] { issue(rX, sA0, k2, e_buf + G::RA0, wave); });
        p8_phase<G, 1, 1, 2, false, false, MF>(acc, a, b, e_buf, oA, oB0, oB1, [&] { issue(rW, sB1, k2, e_buf + G::RB1, wave); });
        p8_phase<G, 1, 0, 1, true, false, MF>(acc, a, b, e_buf, oA, oB0, oB1, [&] { issue(rX, sA1, k2, e_buf + G::RA1, wave); });
        p8_phase<G, 0, 0, 0, false, false, MF>(acc, a, b, o_buf, oA, oB0, oB1, [&] { issue(rW, sB0, k2, e_buf + G::RB0, wave); });
        p8_phase<G, 0, 1, 1, false, false, MF>(acc, a, b, o_buf, oA, oB0, oB1, [&] { issue(rX, sA0, k3, o_buf + G::RA0, wave); });
        p8_phase<G, 1, 1, 2, false, false, MF>(acc, a, b, o_buf, oA, oB0, oB1, [&] { issue(rW, sB1, k3, o_buf + G::RB1, wave); });
        p8_phase<G, 1, 0, 1, true, false, MF>(acc, a, b, o_buf, oA, oB0, oB1, [&] { issue(rX, sA1, k3, o_buf + G::RA1, wave); });
    }
    if (t0 < nk) {  // odd K-tile count: the last tile is in the even buffer (retired by phase 8)
        const int k1 = kb(t0 + 1), k2 = kb(t0 + 2);
        p8_phase<G, 0, 0, 0, false, true, MF>(acc, a, b, e_buf, oA, oB0, oB1, [&] { issue(rW, sB0, k1, o_buf + G::RB0, wave); });
        p8_phase<G, 0, 1, 1, false, true, MF>(acc, a, b, e_buf, oA, oB0, oB1, [&] { issue(rX, sA0, k2, e_buf + G::RA0, wave); });
        p8_phase<G, 1, 1, 2, false, false, MF>(acc, a, b, e_buf, oA, oB0, oB1, [&] { issue(rW, sB1, k2, e_buf + G::RB1, wave); });
        p8_phase<G, 1, 0, 1, false, false, MF>(acc, a, b, e_buf, oA, oB0, oB1, [&] { issue(rX, sA1, k2, e_buf + G::RA1, wave); });
    }
    if (wm == 0) P8_BAR();  // balance the stagger
    EGG_STAMP(2);
    wait_vm<0>();
    __syncthreads();  // every wave is past its last LDS read: the epilogue reuses the ring
    EGG_STAMP(3);

    if constexpr (MF) {  // bias + LoRA term as one extra MFMA k-step, then a plain bf16 store
        lora_mfma_addend_lds<G, R>(acc, lane, m0, wm * 128, wn * G::WTN, smem + G::LDS, bias != nullptr, scale,
                                   rows_per_member, M);
        EGG_STAMP(4);
        if constexpr (WG) {
            __syncthreads();  // the C tile overwrites the epilogue block every wave's addend has just read
            store_tile_wg<EPI>(acc, smem, wave, lane, m0, n0, wm, wn, M, N, Y, ldy, ea);
        } else {
            store_tile_t<EPI>(acc, smem, wave, lane, m0, n0, wm * 128, wn * 64, M, N, Y, ldy, ea);
        }
        EGG_STAMP_DRAIN();
        EGG_STAMP(5);
        EGG_STAMP_RT(7);
    } else {
        lora_epilogue<R, 128, 64>(acc, smem, wave, lane, m0, n0, wm * 128, wn * 64, bias, T, theta_pop, ld_theta,
                                  offB, scale, rows_per_member, 256, M, N, Y, ldy);
    }
}


// ------------------------------------------------------------------------------------
// Y += scale * T B_k^T   (8 bf16 per thread)
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_lora_expand(const float* __restrict__ T, const float* __restrict__ theta_pop,
                                                     int64_t ld_theta, int64_t offB, int r, float scale,
                                                     int64_t rows_per_member, int64_t M, int64_t N,
                                                     unsigned short* __restrict__ Y, int64_t ldy) {
    const int64_t nch = (N + 7) / 8;
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= M * nch) return;
    const int64_t row = idx / nch, c0 = (idx - row * nch) * 8;
    const int64_t kl = row / rows_per_member;
    const float* Bk = theta_pop + kl * ld_theta + offB;
    const float* t = T + row * r;
    unsigned short* y = Y + row * ldy + c0;
    for (int u = 0; u < 8 && c0 + u < N; ++u) {
        float d = 0.0f;
        for (int qq = 0; qq < r; ++qq) d += t[qq] * Bk[(c0 + u) * r + qq];
        y[u] = f32_to_bf16(bf16_to_f32(y[u]) + scale * d);
    }
}

// fp32 population LoRA term of LoRALinear.forward_fp32 (the time / guidance embedders, AdaLN modulation and
// proj_out — the few small linears whose bf16 rounding moved whole members):
//   y[m, :] += scale * (x[m, :] A_k^T) B_k^T,   k = m / rows_per_member,
// A_k = A + k * lda_member as [R][K], B_k = B + k * ldb_member as [N][R] (the PEFT lora_A / lora_B layouts of
// es_backend.py:193-200; member stride 0 = one adapter for every row).  One wave per row, grid-stride: the
// skinny product T = x A_k^T as per-lane fp32 partial sums over k = lane + 64 i, reduced by a fixed xor
// butterfly (a row's bits do not depend on the member count or the grid), then the rank-R expansion
// y[m, n] + (T B_k^T)[n] * scale in PEFT's order (result + lora_B(lora_A(x)) * scaling).
template <int R>
__global__ __launch_bounds__(256) void k_lora_delta_f32(const float* __restrict__ x, int64_t ldx,
                                                        const float* __restrict__ A, int64_t lda_m,
                                                        const float* __restrict__ B, int64_t ldb_m, float scale,
                                                        int64_t rows_per_member, int64_t M, int N, int K,
                                                        float* __restrict__ y, int64_t ldy) {
    const int lane = threadIdx.x & 63;
    const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t m = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); m < M; m += nwaves) {
        const int64_t kl = m / rows_per_member;
        const float* xr = x + m * ldx;
        const float* Ak = A + kl * lda_m;
        float t[R];
#pragma unroll
        for (int q = 0; q < R; ++q) t[q] = 0.0f;
#pragma unroll 4
        for (int k = lane; k < K; k += 64) {
            const float xv = xr[k];
#pragma unroll
            for (int q = 0; q < R; ++q) t[q] = fmaf(xv, Ak[(int64_t)q * K + k], t[q]);
        }
#pragma unroll
        for (int q = 0; q < R; ++q)
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) t[q] += __shfl_xor(t[q], o, 64);
        const float* Bk = B + kl * ldb_m;
        float* yr = y + m * ldy;
        for (int n = lane; n < N; n += 64) {
            float d = 0.0f;
#pragma unroll
            for (int q = 0; q < R; ++q) d = fmaf(t[q], Bk[(int64_t)n * R + q], d);
            yr[n] = yr[n] + d * scale;
        }
    }
}

// The instantiated kernels (dispatch_int, common.h).
using RanksAll = std::integer_sequence<int, 0, 1, 2, 3, 4, 8, 16>;
using RanksMF = std::integer_sequence<int, 0, 1, 2>;  // the MFMA-addend path
using RanksProject = std::integer_sequence<int, 1, 2, 3, 4, 8, 16>;
using ProjectNI = std::integer_sequence<int, 1, 2, 3, 4, 5, 6, 8>;  // k_lora_project_ra: 512-column steps of K
using ProjectNQ = std::integer_sequence<int, 1, 2, 3, 4, 5, 6, 7, 8>;  // k_lora_project_mfma: n_lin * r
using RanksDelta = std::integer_sequence<int, 1, 2, 3, 4, 5, 6, 7, 8>;

// T = X A_k^T: the register-resident-A kernel for r <= 2 where ceil(K / 512) is one of ProjectNI's step
// counts (K <= 4096, 7 steps excepted), else k_lora_project.
static int project(const void* X, int64_t ldx, const float* tp, int64_t ldt, int64_t offA, int32_t r, int64_t rpm,
                   int64_t M, int64_t K, float* T, hipStream_t st) {
    const unsigned short* x = (const unsigned short*)X;
    const bool ok = dispatch_int(r, RanksProject{}, [&](auto Rc) {
        constexpr int R = decltype(Rc)::value;
        if constexpr (R <= 2) {
            const int64_t rows_per_block = 4 * PR_ROWS;
            const int64_t ni = (K + 511) / 512;
            if (ni <= 8 && dispatch_int((int)ni, ProjectNI{}, [&](auto NI) {
                    hipLaunchKernelGGL((k_lora_project_ra<R, decltype(NI)::value>),
                                       dim3((unsigned)((M + rows_per_block - 1) / rows_per_block)), dim3(256), 0, st, x,
                                       ldx, tp, ldt, offA, rpm, M, K, T);
                }))
                return;
        }
        hipLaunchKernelGGL(k_lora_project<R>, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, st, x, ldx, tp, ldt, offA,
                           rpm, M, K, T);
    });
    if (!ok) {
        set_error("lora: r=%d unsupported (1,2,3,4,8,16)", r);
        return EGGROLL_ERR_UNSUPPORTED;
    }
    EGG_CHECK_LAUNCH("lora_project");
    return EGGROLL_OK;
}
using EpiOps = std::integer_sequence<int, EPI_NONE, EPI_SILU, EPI_RES, EPI_GATED, EPI_RES32, EPI_GATED32, EPI_GELU,
                                     EPI_MUL, EPI_GELU_ERF>;

// The arguments every base-GEMM kernel takes, in kernel order.
struct GemmArgs {
    const void *X;  int64_t ldx;
    const void *W;  int64_t ldw;
    const void* bias;
    const float *T, *theta_pop;
    int64_t ld_theta, offB;
    int32_t r;
    float scale;
    int64_t rows_per_member, M, N, K;
    void* Y;  int64_t ldy;
};

// k_lora_gemm / k_lora_gemm8 over grid = tiles_m * tiles_n (BM x BN tiles); `extra`: k_lora_gemm8's EpiArgs
template <class Kern, class... Extra>
static void launch_tiles(Kern kern, int64_t tiles_m, int64_t tiles_n, int threads, const GemmArgs& g, hipStream_t st,
                         const Extra&... extra) {
    hipLaunchKernelGGL(kern, dim3((unsigned)(tiles_m * tiles_n)), dim3(threads), 0, st, (const unsigned short*)g.X, g.ldx,
                       (const unsigned short*)g.W, g.ldw, (const unsigned short*)g.bias, g.T, g.theta_pop, g.ld_theta,
                       g.offB, g.scale, (int)g.rows_per_member, (int)g.M, (int)g.N, g.K, (int)tiles_n,
                       (unsigned short*)g.Y, g.ldy, extra...);
}

static int unsupported_r(int32_t r) {
    set_error("lora_gemm: r=%d unsupported (0,1,2,3,4,8,16)", r);
    return EGGROLL_ERR_UNSUPPORTED;
}

// The one-barrier tile (kernel 128).
static int launch_gemm(const GemmArgs& g, hipStream_t st) {
    const int64_t tiles_m = (g.M + T128::BM - 1) / T128::BM, tiles_n = (g.N + T128::BN - 1) / T128::BN;
    EGG_CHECK_ARG(tiles_m * tiles_n < (1ll << 31), "lora_gemm: grid too large");
    if (!dispatch_int(g.r, RanksAll{}, [&](auto R) {
            launch_tiles(k_lora_gemm<decltype(R)::value>, tiles_m, tiles_n, T128::THREADS, g, st);
        }))
        return unsupported_r(g.r);
    EGG_CHECK_LAUNCH("lora_gemm");
    return EGGROLL_OK;
}

// The 256 x 320 kernel (kernel 10): MFMA-addend path only (r <= 2 with rows_per_member >= 256, or r = 0).
static bool gemm8n_ok(int32_t r, int64_t rows_per_member) { return r == 0 || (r <= 2 && rows_per_member >= 256); }

// Automatic choice between the 8-phase tiles (256 x 256 = 8, 256 x 320 = 10): rounds of one tile per
// CU (256 CUs) times the tile's cost, a 256 x 320 tile measured at 1.22x a 256 x 256 one (25 % more
// MFMAs, ~2.5 % fewer cycles per output element and a slightly higher clock; tools/gemm10_probe.py,
// DESIGN §5).  131072 x 2240: 18 vs 14 x 1.22 rounds -> 10 (+3-6 % measured); 9600 x 2240: 2 vs 2 x 1.22
// -> 8.  The residual / gated-residual epilogues stay on 8 (their loads slow kernel 10's store phase).
static int gemm8_auto(int64_t M, int64_t N, int32_t r, int64_t rows_per_member, int32_t epi) {
    // the bf16 residual epilogues stay on 8 (their per-chunk loads slow kernel 10's store phase); the fp32
    // ones load in batches and run equal (to_out) or 3 % faster (FFN point conv, K 5632) on 10
    // (profiles/r05h_epi32_kernel8_vs_10_ab.log)
    if (!gemm8n_ok(r, rows_per_member) || epi == EPI_RES || epi == EPI_GATED || epi == EPI_MUL) return 8;
    const int64_t tm = (M + 255) / 256;
    const int64_t rounds8 = (tm * ((N + 255) / 256) + 255) / 256, rounds10 = (tm * ((N + 319) / 320) + 255) / 256;
    return 122 * rounds10 < 100 * rounds8 ? 10 : 8;
}

// The 8-phase kernel over geometry G.  mf: the MFMA-addend path (r <= 2; every epilogue op rides it);
// else the VALU epilogue (256 x 256 only, epi = EPI_NONE).
template <class G>
static int launch_gemm8(const GemmArgs& g, bool mf, int32_t epi, const EpiArgs& ea, hipStream_t st) {
    constexpr bool N320 = G::NF == 5;
    const int64_t tiles_m = (g.M + G::BM - 1) / G::BM, tiles_n = (g.N + G::BN - 1) / G::BN;
    EGG_CHECK_ARG(tiles_m * tiles_n < (1ll << 31), "lora_gemm: grid too large");
    if constexpr (N320)
        EGG_CHECK_ARG(gemm8n_ok(g.r, g.rows_per_member), "lora_gemm: kernel 10 needs r <= 2 and rows_per_member >= 256");
    bool ok;
    if (mf || N320) {
        ok = dispatch_int(g.r, RanksMF{}, [&](auto R) {
            dispatch_int(epi, EpiOps{}, [&](auto E) {
                launch_tiles(k_lora_gemm8<G, decltype(R)::value, true, decltype(E)::value>, tiles_m, tiles_n, 512, g, st,
                             ea);
            });
        });
    } else {
        ok = dispatch_int(g.r, RanksAll{}, [&](auto R) {
            if constexpr (!N320)
                launch_tiles(k_lora_gemm8<G, decltype(R)::value, false, EPI_NONE>, tiles_m, tiles_n, 512, g, st, ea);
        });
    }
    if (!ok) return unsupported_r(g.r);
    EGG_CHECK_LAUNCH(N320 ? "lora_gemm8n" : epi != EPI_NONE ? "lora_gemm8_epi" : "lora_gemm8");
    return EGGROLL_OK;
}

// The operand checks every GEMM entry point shares, reported under the caller's name.  dma32: the
// 8-phase kernels address X and W through 32-bit buffer offsets.
static int gemm_args_ok(const char* api, const GemmArgs& g, bool dma32) {
    EGG_CHECK_ARG(g.ldx % 8 == 0 && g.ldw % 8 == 0 && g.ldx >= g.K && g.ldw >= g.K && g.ldy >= g.N, "%s: bad strides",
                  api);
    EGG_CHECK_ARG(g.M < (1ll << 31) && g.N < (1ll << 31) && g.rows_per_member < (1ll << 31), "%s: M/N too large", api);
    EGG_CHECK_ARG(!dma32 || g.M == 0 || (g.M * g.ldx * 2 < (1ll << 31) && g.N * g.ldw * 2 < (1ll << 31)),
                  "%s: operand > 2 GiB", api);
    return EGGROLL_OK;
}

// Kernel choice is a per-call argument (no process-global state: the C-ABI is thread-safe per
// stream).  0 = automatic: an 8-phase kernel (gemm8_auto) when the grid still fills the chip, else the
// 128x128 one-barrier tile.  8 / 9 = 8-phase 256x256 with MFMA / VALU LoRA epilogue, 10 = 8-phase
// 256x320, 128 = the one-barrier tile.
// Every argument check of the plain GEMM entry points, reported under the caller's name, before
// anything is launched; *tsel: the kernel that will run.
static int plain_args_ok(const char* api, const GemmArgs& g, int32_t kernel, int* tsel) {
    EGG_CHECK_ARG(kernel == 0 || kernel == 8 || kernel == 9 || kernel == 10 || kernel == 128,
                  "%s: kernel must be 0 (auto), 8, 9, 10 or 128 (got %d)", api, kernel);
    EGG_CHECK_ARG(g.M >= 0 && g.N > 0 && g.K > 0, "%s: bad sizes M=%lld N=%lld K=%lld", api, (long long)g.M,
                  (long long)g.N, (long long)g.K);
    EGG_CHECK_ARG(g.K % 64 == 0, "%s: K=%lld must be a multiple of 64", api, (long long)g.K);
    EGG_CHECK_ARG(g.r >= 0 && g.r <= 16, "%s: r=%d out of range", api, g.r);
    EGG_CHECK_ARG(g.rows_per_member > 0, "%s: rows_per_member must be > 0", api);
    *tsel = kernel ? kernel
                   : ((g.M / 256) * ((g.N + 255) / 256) >= 512 ? gemm8_auto(g.M, g.N, g.r, g.rows_per_member, EPI_NONE)
                                                               : 128);
    return gemm_args_ok(api, g, *tsel != 128);
}

// The plain GEMM on kernel tsel, arguments checked by plain_args_ok (M > 0).
static int lora_gemm_launch(const char* api, int tsel, const GemmArgs& g, hipStream_t st) {
    EGG_CHECK_ARG(g.X && g.W && g.Y, "%s: NULL pointer", api);
    EGG_CHECK_ARG(g.r == 0 || (g.T && g.theta_pop), "%s: T / theta_pop NULL with r > 0", api);
    if (tsel == 128) return launch_gemm(g, st);
    if (tsel == 10 && gemm8n_ok(g.r, g.rows_per_member))  // else: kernel 8's VALU-epilogue path, as kernel 8 does
        return launch_gemm8<G8<2, 5>>(g, true, EPI_NONE, EpiArgs{}, st);
    return launch_gemm8<G8<2>>(g, tsel != 9 && g.r <= 2 && g.rows_per_member >= 256, EPI_NONE, EpiArgs{}, st);
}

// The epilogue checks of the _epi_ entry points (epi != EPI_NONE), in plain_args_ok's manner.
static int epi_args_ok(const char* api, const GemmArgs& g, int32_t epi, const EpiArgs& ea, int32_t kernel) {
    EGG_CHECK_ARG(kernel == 0 || kernel == 8 || kernel == 10, "%s: kernel must be 0, 8 or 10", api);
    EGG_CHECK_ARG(epi >= EPI_SILU && epi <= EPI_GELU_ERF, "%s: epi=%d unknown", api, epi);
    EGG_CHECK_ARG(g.r >= 0 && g.r <= 2, "%s: r=%d (epilogue ops need r <= 2)", api, g.r);
    EGG_CHECK_ARG(g.r == 0 || g.rows_per_member >= 256, "%s: rows_per_member must be >= 256 with r > 0", api);
    EGG_CHECK_ARG(g.M >= 0 && g.N > 0 && g.K > 0 && g.K % 64 == 0, "%s: need K %% 64 == 0", api);
    if (const int rc = gemm_args_ok(api, g, true)) return rc;
    EGG_CHECK_ARG(epi == EPI_SILU || epi == EPI_GELU || epi == EPI_GELU_ERF || (ea.res && ea.ldr >= g.N),
                  "%s: res NULL or ldr < N", api);
    EGG_CHECK_ARG((epi != EPI_GATED && epi != EPI_GATED32) || (ea.gate && ea.gstride >= g.N && ea.rpg > 0),
                  "%s: bad gate", api);
    if (g.M == 0) return EGGROLL_OK;
    EGG_CHECK_ARG(g.X && g.W && (g.Y || epi == EPI_RES32 || epi == EPI_GATED32), "%s: NULL pointer", api);
    return EGGROLL_OK;
}

// The epilogue GEMM with T = X A_k^T already computed, arguments checked by epi_args_ok (M > 0).
static int gemm_epi_impl(GemmArgs g, int32_t epi, const EpiArgs& ea, int32_t kernel, hipStream_t st) {
    if (g.r == 0) g.rows_per_member = g.M;  // no members without a LoRA term: the addend sees one
    if (kernel == 0) kernel = gemm8_auto(g.M, g.N, g.r, g.rows_per_member, epi);
    return kernel == 10 ? launch_gemm8<G8<2, 5>>(g, true, epi, ea, st) : launch_gemm8<G8<2>>(g, true, epi, ea, st);
}


}  // namespace eggroll

using namespace eggroll;

extern "C" {

#ifdef EGG_STAMPS
// diagnostic build only: copy the first n stamps (n <= 131072 * 8) to host memory
int eggroll_debug_stamps(unsigned long long* host, int64_t n) {
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_egg_stamps), (size_t)n * 8, 0, hipMemcpyDeviceToHost) == hipSuccess
               ? EGGROLL_OK
               : EGGROLL_ERR_LAUNCH;
}
#endif

int eggroll_lora_project(const void* X, int64_t ldx, const float* theta_pop, int64_t ld_theta, int64_t offA, int32_t r,
                         int64_t rows_per_member, int64_t M, int64_t K, float* T, void* stream) {
    EGG_CHECK_ARG(M >= 0 && K > 0 && K % 8 == 0 && ldx % 8 == 0 && ldx >= K, "lora_project: need K%%8==0, ldx%%8==0");
    EGG_CHECK_ARG(ld_theta % 4 == 0 && offA % 4 == 0, "lora_project: theta offsets must be 16-byte aligned");
    EGG_CHECK_ARG(rows_per_member > 0, "lora_project: rows_per_member must be > 0");
    if (M == 0) return EGGROLL_OK;
    EGG_CHECK_ARG(X && theta_pop && T, "lora_project: NULL pointer");
    return project(X, ldx, theta_pop, ld_theta, offA, r, rows_per_member, M, K, T, as_stream(stream));
}

int eggroll_lora_project_multi(const void* X, int64_t ldx, const float* theta_pop, int64_t ld_theta,
                               const int64_t* offA_host, int32_t n_lin, int32_t r, int64_t rows_per_member, int64_t M,
                               int64_t K, float* T, void* stream) {
    EGG_CHECK_ARG(n_lin >= 1 && n_lin <= 4 && r >= 1 && n_lin * r <= 8,
                  "lora_project_multi: need 1 <= n_lin <= 4 and n_lin * r <= 8 (n_lin=%d r=%d)", n_lin, r);
    EGG_CHECK_ARG(M >= 0 && K >= 32 && K % 32 == 0 && K <= 4096, "lora_project_multi: need K %% 32 == 0, K <= 4096");
    EGG_CHECK_ARG(ldx % 8 == 0 && ldx >= K, "lora_project_multi: ldx must be a multiple of 8 and >= K");
    EGG_CHECK_ARG(rows_per_member > 0 && ld_theta % 4 == 0, "lora_project_multi: bad rows_per_member / ld_theta");
    if (M == 0) return EGGROLL_OK;
    EGG_CHECK_ARG(X && theta_pop && T && offA_host, "lora_project_multi: NULL pointer");
    EGG_CHECK_ARG(((uintptr_t)X & 15) == 0 && ((uintptr_t)theta_pop & 15) == 0,
                  "lora_project_multi: X and theta_pop must be 16-byte aligned (16-byte vector loads)");
    int64_t off[4] = {0, 0, 0, 0};
    for (int l = 0; l < n_lin; ++l) {
        off[l] = offA_host[l];
        EGG_CHECK_ARG(off[l] >= 0 && off[l] % 4 == 0 && off[l] + (int64_t)r * K <= ld_theta,
                      "lora_project_multi: offA[%d] must be 16-byte aligned and inside a theta row", l);
    }
    const unsigned grid = (unsigned)((M + PM_ROWS_PER_BLOCK - 1) / PM_ROWS_PER_BLOCK);
    const size_t lds = (size_t)K * 32;
    hipStream_t st = as_stream(stream);
    dispatch_int(n_lin * r, ProjectNQ{}, [&](auto NQ) {  // 1 <= n_lin * r <= 8: checked above
        hipLaunchKernelGGL(k_lora_project_mfma<decltype(NQ)::value>, dim3(grid), dim3(256), lds, st,
                           (const unsigned short*)X, ldx, theta_pop, ld_theta, off[0], off[1], off[2], off[3], (int)r,
                           rows_per_member, M, K, T);
    });
    EGG_CHECK_LAUNCH("lora_project_multi");
    return EGGROLL_OK;
}

int eggroll_lora_expand(const float* T, const float* theta_pop, int64_t ld_theta, int64_t offB, int32_t r, float scale,
                        int64_t rows_per_member, int64_t M, int64_t N, void* Y, int64_t ldy, void* stream) {
    EGG_CHECK_ARG(M >= 0 && N > 0 && r >= 1 && r <= 16 && rows_per_member > 0 && ldy >= N, "lora_expand: bad sizes");
    if (M == 0) return EGGROLL_OK;
    EGG_CHECK_ARG(T && theta_pop && Y, "lora_expand: NULL pointer");
    const int64_t work = M * ((N + 7) / 8);
    hipLaunchKernelGGL(k_lora_expand, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, as_stream(stream), T,
                       theta_pop, ld_theta, offB, r, scale, rows_per_member, M, N, (unsigned short*)Y, ldy);
    EGG_CHECK_LAUNCH("lora_expand");
    return EGGROLL_OK;
}

int eggroll_lora_delta_f32(const float* x, int64_t ldx, const float* A, int64_t lda_member, const float* B,
                           int64_t ldb_member, int32_t r, float scale, int64_t rows_per_member, int64_t M, int64_t N,
                           int64_t K, float* y, int64_t ldy, void* stream) {
    EGG_CHECK_ARG(r >= 1 && r <= 8, "lora_delta_f32: r=%d must be in [1, 8]", r);
    EGG_CHECK_ARG(M >= 0 && N > 0 && K > 0 && N < (1ll << 31) && K < (1ll << 31) && rows_per_member > 0,
                  "lora_delta_f32: bad sizes M=%lld N=%lld K=%lld rows_per_member=%lld", (long long)M, (long long)N,
                  (long long)K, (long long)rows_per_member);
    EGG_CHECK_ARG(ldx >= K && ldy >= N && lda_member >= 0 && ldb_member >= 0, "lora_delta_f32: bad strides");
    if (M == 0) return EGGROLL_OK;
    EGG_CHECK_ARG(x && A && B && y, "lora_delta_f32: NULL pointer");
    const int64_t blocks = std::min<int64_t>((M + 3) / 4, 2048);
    hipStream_t st = as_stream(stream);
    dispatch_int(r, RanksDelta{}, [&](auto R) {  // 1 <= r <= 8: checked above
        hipLaunchKernelGGL(k_lora_delta_f32<decltype(R)::value>, dim3((unsigned)blocks), dim3(256), 0, st, x, ldx, A,
                           lda_member, B, ldb_member, scale, rows_per_member, M, (int)N, (int)K, y, ldy);
    });
    EGG_CHECK_LAUNCH("lora_delta_f32");
    return EGGROLL_OK;
}

int eggroll_lora_gemm_sel(const void* X, int64_t ldx, const void* W, int64_t ldw, const void* bias, const float* T,
                          const float* theta_pop, int64_t ld_theta, int64_t offB, int32_t r, float scale,
                          int64_t rows_per_member, int64_t M, int64_t N, int64_t K, void* Y, int64_t ldy,
                          int32_t kernel, void* stream) {
    const GemmArgs g{X, ldx, W, ldw, bias, T, theta_pop, ld_theta, offB, r, scale, rows_per_member, M, N, K, Y, ldy};
    int tsel;
    if (const int rc = plain_args_ok("lora_gemm", g, kernel, &tsel)) return rc;
    if (M == 0) return EGGROLL_OK;
    return lora_gemm_launch("lora_gemm", tsel, g, as_stream(stream));
}

int eggroll_lora_gemm(const void* X, int64_t ldx, const void* W, int64_t ldw, const void* bias, const float* T,
                      const float* theta_pop, int64_t ld_theta, int64_t offB, int32_t r, float scale,
                      int64_t rows_per_member, int64_t M, int64_t N, int64_t K, void* Y, int64_t ldy, void* stream) {
    return eggroll_lora_gemm_sel(X, ldx, W, ldw, bias, T, theta_pop, ld_theta, offB, r, scale, rows_per_member, M, N, K,
                                 Y, ldy, 0, stream);
}

int64_t eggroll_lora_workspace_bytes(int64_t M, int64_t K, int32_t r, int64_t rows_per_member) {
    if (M <= 0 || r <= 0 || rows_per_member <= 0) return 0;
    (void)K;  // kept in the signature; the workspace is the fp32 T [M, r] alone
    return M * r * 4;
}

int eggroll_lora_linear_pop_sel(const void* X, int64_t ldx, const void* W, int64_t ldw, const void* bias,
                                const float* theta_pop, int64_t ld_theta, int64_t offA, int64_t offB, int32_t r,
                                float scale, int64_t rows_per_member, int64_t M, int64_t N, int64_t K, void* Y,
                                int64_t ldy, float* T_ws, int32_t kernel, void* stream) {
    const GemmArgs g{X, ldx, W, ldw, bias, T_ws, theta_pop, ld_theta, offB, r, scale, rows_per_member, M, N, K, Y, ldy};
    // every check of the GEMM before the projection is launched: a refused call launches nothing
    int tsel;
    if (const int rc = plain_args_ok("lora_linear_pop", g, kernel, &tsel)) return rc;
    if (M == 0) return EGGROLL_OK;
    EGG_CHECK_ARG(X && W && Y, "lora_linear_pop: NULL pointer");
    EGG_CHECK_ARG(r == 0 || (theta_pop && T_ws), "lora_linear_pop: theta_pop / T_ws NULL with r > 0");
    if (r > 0) {
        int rc = eggroll_lora_project(X, ldx, theta_pop, ld_theta, offA, r, rows_per_member, M, K, T_ws, stream);
        if (rc) return rc;
    }
    return lora_gemm_launch("lora_linear_pop", tsel, g, as_stream(stream));
}

int eggroll_lora_linear_pop_epi_sel(const void* X, int64_t ldx, const void* W, int64_t ldw, const void* bias,
                                    const float* theta_pop, int64_t ld_theta, int64_t offA, int64_t offB, int32_t r,
                                    float scale, int64_t rows_per_member, int64_t M, int64_t N, int64_t K, void* Y,
                                    int64_t ldy, float* T_ws, int32_t epi, const void* res, int64_t ldr,
                                    const void* gate, int64_t gstride, int64_t rows_per_group, int32_t kernel,
                                    void* stream) {
    if (epi == EPI_NONE) {
        EGG_CHECK_ARG(kernel == 0 || kernel == 8 || kernel == 10, "lora_linear_pop_epi: kernel must be 0, 8 or 10");
        return eggroll_lora_linear_pop_sel(X, ldx, W, ldw, bias, theta_pop, ld_theta, offA, offB, r, scale,
                                           rows_per_member, M, N, K, Y, ldy, T_ws, kernel, stream);
    }
    const GemmArgs g{X, ldx, W, ldw, bias, T_ws, theta_pop, ld_theta, offB, r, scale, rows_per_member, M, N, K, Y, ldy};
    const EpiArgs ea{(const unsigned short*)res, ldr, (const unsigned short*)gate, gstride, rows_per_group};
    const int rc0 = epi_args_ok("lora_linear_pop_epi", g, epi, ea, kernel);
    if (rc0 || M == 0) return rc0;
    if (r > 0) {
        EGG_CHECK_ARG(theta_pop && T_ws, "lora_linear_pop_epi: theta_pop / T_ws NULL with r > 0");
        int rc = eggroll_lora_project(X, ldx, theta_pop, ld_theta, offA, r, rows_per_member, M, K, T_ws, stream);
        if (rc) return rc;
    }
    return gemm_epi_impl(g, epi, ea, kernel, as_stream(stream));
}

int eggroll_lora_gemm_epi_sel(const void* X, int64_t ldx, const void* W, int64_t ldw, const void* bias, const float* T,
                              const float* theta_pop, int64_t ld_theta, int64_t offB, int32_t r, float scale,
                              int64_t rows_per_member, int64_t M, int64_t N, int64_t K, void* Y, int64_t ldy,
                              int32_t epi, const void* res, int64_t ldr, const void* gate, int64_t gstride,
                              int64_t rows_per_group, int32_t kernel, void* stream) {
    const GemmArgs g{X, ldx, W, ldw, bias, T, theta_pop, ld_theta, offB, r, scale, rows_per_member, M, N, K, Y, ldy};
    const EpiArgs ea{(const unsigned short*)res, ldr, (const unsigned short*)gate, gstride, rows_per_group};
    const int rc0 = epi_args_ok("lora_gemm_epi", g, epi, ea, kernel);
    if (rc0 || M == 0) return rc0;
    EGG_CHECK_ARG(r == 0 || (T && theta_pop), "lora_gemm_epi: T / theta_pop NULL with r > 0");
    return gemm_epi_impl(g, epi, ea, kernel, as_stream(stream));
}

int eggroll_lora_linear_pop_epi(const void* X, int64_t ldx, const void* W, int64_t ldw, const void* bias,
                                const float* theta_pop, int64_t ld_theta, int64_t offA, int64_t offB, int32_t r,
                                float scale, int64_t rows_per_member, int64_t M, int64_t N, int64_t K, void* Y,
                                int64_t ldy, float* T_ws, int32_t epi, const void* res, int64_t ldr, const void* gate,
                                int64_t gstride, int64_t rows_per_group, void* stream) {
    return eggroll_lora_linear_pop_epi_sel(X, ldx, W, ldw, bias, theta_pop, ld_theta, offA, offB, r, scale,
                                           rows_per_member, M, N, K, Y, ldy, T_ws, epi, res, ldr, gate, gstride,
                                           rows_per_group, 0, stream);
}

int eggroll_lora_linear_pop(const void* X, int64_t ldx, const void* W, int64_t ldw, const void* bias,
                            const float* theta_pop, int64_t ld_theta, int64_t offA, int64_t offB, int32_t r,
                            float scale, int64_t rows_per_member, int64_t M, int64_t N, int64_t K, void* Y,
                            int64_t ldy, float* T_ws, void* stream) {
    return eggroll_lora_linear_pop_sel(X, ldx, W, ldw, bias, theta_pop, ld_theta, offA, offB, r, scale,
                                       rows_per_member, M, N, K, Y, ldy, T_ws, 0, stream);
}

}  // extern "C"
