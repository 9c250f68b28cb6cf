// libeggroll — the 8-phase LDS-ring primitives shared by the population LoRA GEMMs (eggroll_lora.hip)
// and the DC-AE convolutions (eggroll_conv.hip), each in a single form.
#pragma once
#include "common.h"

namespace eggroll {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((ext_vector_type(4))) unsigned short u16x4;
typedef __attribute__((ext_vector_type(8))) unsigned short u16x8;
typedef __attribute__((address_space(3))) void lds_void;
typedef const __attribute__((address_space(1))) void gbl_void;

__device__ __forceinline__ float bf16_to_f32(unsigned short h) {
    return __uint_as_float(((uint32_t)h) << 16);
}
__device__ __forceinline__ unsigned short f32_to_bf16(float f) {  // RNE, NaN-preserving cast
    __bf16 b = (__bf16)f;
    return *reinterpret_cast<unsigned short*>(&b);
}

constexpr int BK = 64;
#ifndef EGG_GROUP_M
#define EGG_GROUP_M 8
#endif
constexpr int GROUP_M = EGG_GROUP_M;  // row-tiles per rasterisation group

// Phase stamps for the tools-only diagnostic build (tools/stamp_probe.py compiles the library with
// -DEGG_STAMPS into a separate file; the shipped libeggroll.so has none): wave 0 of every workgroup
// records s_memtime at fixed points of the 8-phase kernels (vector stores from lane 0).  Each
// translation unit has its own stamp array and its own reader (eggroll_debug_stamps /
// eggroll_debug_conv_stamps).
#ifdef EGG_STAMPS
constexpr int EGG_NSTAMP = 8;
static __device__ unsigned long long g_egg_stamps[131072 * EGG_NSTAMP];
#define EGG_STAMP(k)                                                                                         \
    do {                                                                                                     \
        if (threadIdx.x == 0)                                                                                \
            g_egg_stamps[(size_t)blockIdx.x * EGG_NSTAMP + (k)] = __builtin_amdgcn_s_memtime();              \
    } while (0)
#define EGG_STAMP_RT(k)                                                                                      \
    do {                                                                                                     \
        if (threadIdx.x == 0)                                                                                \
            g_egg_stamps[(size_t)blockIdx.x * EGG_NSTAMP + (k)] = __builtin_amdgcn_s_memrealtime();          \
    } while (0)
#define EGG_STAMP_DRAIN() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")
#else
#define EGG_STAMP(k) \
    do {             \
    } while (0)
#define EGG_STAMP_RT(k) \
    do {                \
    } while (0)
#define EGG_STAMP_DRAIN() \
    do {                  \
    } while (0)
#endif

// XCD-aware bijective remap (consecutive tile ids, which share X rows, land on one XCD) + grouped
// rasterisation: consecutive tiles (one XCD's concurrently resident set) walk GROUP_M row-tiles
// before moving to the next column-tile, so X and W panels are both reused in L2.
struct TileIdx {
    int m, n;
};
template <int BM>
__device__ __forceinline__ TileIdx p8_tile_index(int M, int tiles_n) {
    const int tile = xcd_remap(blockIdx.x, gridDim.x);
    const int tiles_m = (M + BM - 1) / BM;
    const int per_group = GROUP_M * tiles_n;
    const int grp = tile / per_group, first_m = grp * GROUP_M;
    const int gsize = (tiles_m - first_m) < GROUP_M ? (tiles_m - first_m) : GROUP_M;
    const int in_grp = tile - grp * per_group;
    return TileIdx{first_m + in_grp % gsize, in_grp / gsize};
}

// ------------------------------------------------------------------------------------
// The 8-phase schedule (BK = 64, 8 waves, one workgroup per CU).  The waves form 2 groups of 4
// (one wave of each per SIMD); each wave owns a 128 x 16 NF output sub-tile = 4 C-quadrants of
// 64 rows x NF0 or NF1 fragment columns.  Every K-tile is split into 4 LDS regions by quadrant:
// A0 / A1 = rows of quadrant-row qa = 0 / 1 of every wave row, B0 / B1 = columns of quadrant-column
// qb = 0 / 1 of every wave column.  One phase = {ds_read the quadrant's fragments, issue one region's
// prefetch, lgkmcnt(0), s_barrier, the quadrant's MFMAs, s_barrier}; group 1 runs one barrier behind
// group 0, so on every SIMD one wave does MFMA while its partner reads LDS / issues DMA.  Quadrant
// order per K-tile (0,0) (0,1) (1,1) (1,0): A0+B0 read in phase 1, B1 in 2, A1 in 3, B0 again in 4,
// and each region is restaged in the phase after its last read (lgkmcnt(0) before the barrier retired
// those reads).  The prefetch of K-tile t+1 therefore spans phases (t,2)..(t,4)+(t+1,1) and the
// counted vmcnt(VMC) that retires a buffer leaves 3 regions in flight across the barrier; nothing
// drains vmcnt to 0 inside the loop (cdna_hip_programming.md §5 "256² 8-phase template", T3/T4).
//
// G8<WMW, NF>: WMW wave rows x 8 / WMW wave columns, wave tile 128 x 16 NF:
//   G8<2>    256 x 256 (2 x 4 waves): the LoRA GEMM and the convs with PX * Cout >= 256
//   G8<4>    512 x 128 (4 x 2 waves): Cout = 128 convs at PX = 1; A region 32 KiB (4 DMAs per wave),
//            B region 8 KiB (1 DMA), the ring is the whole 160 KiB
//   G8<2, 5> 256 x 320: B0 = n-fragments 0-2 of every wave column (192 rows, 3 DMAs per wave),
//            B1 = n-fragments 3-4 (128 rows, 2 DMAs); ring 2 x 72 KiB
// ------------------------------------------------------------------------------------
template <int WMW, int NF_ = 4>
struct G8 {
    static constexpr int NF = NF_, NF0 = (NF + 1) / 2, NF1 = NF - NF0;  // n-fragments per wave / quadrant column
    static constexpr int WNW = 8 / WMW, WTN = 16 * NF, BM = WMW * 128, BN = WNW * WTN;
    static constexpr int PER0 = 16 * NF0, PER1 = 16 * NF1;  // B-region rows per wave column
    static constexpr int HA = BM * 64, HB0 = WNW * PER0 * 128, HB1 = WNW * PER1 * 128;  // region bytes (rows x 128 B)
    static constexpr int RA0 = 0, RA1 = HA, RB0 = 2 * HA, RB1 = 2 * HA + HB0;
    static constexpr int BUF = 2 * HA + HB0 + HB1, LDS = 2 * BUF;
    static constexpr int NA = HA / 8192, NB0 = HB0 / 8192, NB1 = HB1 / 8192;  // DMAs per wave per region (8 waves x 1 KiB)
    // DMAs left in flight when a K-tile retires (the next K-tile's A0, B1, A1 regions; T3/T4 formula)
    static constexpr int VMC = 2 * NA + NB1;
    // Early first K-tile.  The prologue issues K-tile 0 as A0, B0, B1, A1 and waits only for A0 + B0
    // (what phase 1 reads): younger are B1, A1 and the next K-tile's A0, B1, A1 = VMC0.  Phase 1
    // retires B1 (read in phase 2) and phase 2 retires A1 (read in phase 3), each before its first
    // barrier — "wait in phase q, read in phase q+1", which also covers the wave group that runs one
    // barrier behind.  Younger than each of these are 3 A regions, one B1 and one B0 = VMCE; in steady
    // state at most that many are outstanding at those points, so the two in-loop waits are no-ops
    // after K-tile 0.
    static constexpr int VMC0 = 3 * NA + 2 * NB1, VMCE = 3 * NA + NB0 + NB1;
    static constexpr int CSTAGE = 8 * 128 * 64 * 2;  // per-wave C staging (store_tile_t): one 128x64 bf16 tile per wave
    static_assert(LDS <= 160 * 1024, "ring exceeds the 160 KiB LDS");
};

// Per-thread staging descriptor of one region: ND DMAs (buffer_load_dwordx4 ... lds), each 8 rows x
// 128 B.  `off[i]` is the lane's 32-bit BYTE offset (row * ld + swizzled chunk) at k = 0; the
// K-tile's byte offset goes in the wave-uniform soffset.  The host guarantees rows*ld*2 < 2^31.
// LDS image: region row j at byte 128 j; 16-B slot s' of row j holds global chunk s' ^ (j & 7).
template <int ND>
struct Stage {
    uint32_t off[ND];
};

// A region QA: region row j -> tile row (j / 64) * 128 + QA * 64 + j % 64 (wave row wm = j / 64)
template <class G, int QA>
__device__ __forceinline__ Stage<G::NA> make_stage_a(int m0, int row_max, int64_t ld, int wave, int lane) {
    Stage<G::NA> s;
#pragma unroll
    for (int i = 0; i < G::NA; ++i) {
        const int j = (i * 8 + wave) * 8 + (lane >> 3);  // region row
        const int chunk = (lane & 7) ^ (j & 7);
        int gr = m0 + (j >> 6) * 128 + QA * 64 + (j & 63);
        gr = gr < row_max ? gr : row_max;  // clamp: rows past the end are never stored
        s.off[i] = ((uint32_t)gr * (uint32_t)ld + chunk * 8) * 2;
    }
    return s;
}
// B region QB: PER rows per wave column starting at the wave tile's column FIRST, wave-column pitch
// WTN: region row j -> tile column (j / PER) * WTN + FIRST + j % PER.  (j >= 0, which the compiler
// cannot see through the wave id's readfirstlane: shift and mask where PER is a power of two.)
template <class G, int QB>
__device__ __forceinline__ Stage<(QB ? G::NB1 : G::NB0)> make_stage_b(int n0, int row_max, int64_t ld, int wave,
                                                                      int lane) {
    constexpr int ND = QB ? G::NB1 : G::NB0, PER = QB ? G::PER1 : G::PER0, FIRST = QB ? G::PER0 : 0;
    constexpr bool P2 = (PER & (PER - 1)) == 0;
    Stage<ND> s;
#pragma unroll
    for (int i = 0; i < ND; ++i) {
        const int j = (i * 8 + wave) * 8 + (lane >> 3);
        const int chunk = (lane & 7) ^ (j & 7);
        int gr = n0 + (P2 ? j >> __builtin_ctz(PER) : j / PER) * G::WTN + FIRST + (P2 ? j & (PER - 1) : j % PER);
        gr = gr < row_max ? gr : row_max;
        s.off[i] = ((uint32_t)gr * (uint32_t)ld + chunk * 8) * 2;
    }
    return s;
}

template <int ND>
__device__ __forceinline__ void issue(__amdgpu_buffer_rsrc_t rs, const Stage<ND>& s, int kbytes, char* region,
                                      int wave) {
#pragma unroll
    for (int i = 0; i < ND; ++i) {
        const uint32_t v = s.off[i];  // (a local: hipcc rejects the member access inside the builtin here)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void*)(region + (i * 8 + wave) * 1024), 16, v, kbytes, 0, 0);
    }
}

#define P8_LGKM0() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")
// s_barrier as a full compiler fence: the builtin alone is IntrNoMem, so IR passes may move the
// next phase's ds_reads (or this phase's MFMAs) across it.
#define P8_BAR()                              \
    do {                                      \
        asm volatile("" ::: "memory");        \
        __builtin_amdgcn_sched_barrier(0);    \
        __builtin_amdgcn_s_barrier();         \
        __builtin_amdgcn_sched_barrier(0);    \
        asm volatile("" ::: "memory");        \
    } while (0)

// s_waitcnt vmcnt(N) with a compile-time N
template <int N>
__device__ __forceinline__ void wait_vm() {
    static_assert(N >= 0 && N < 64, "vmcnt range");
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// The MFMAs of quadrant (QA, QB): QB = 0 covers n-fragments 0 .. NF0-1, QB = 1 the rest.
// TR: W as the MFMA A-operand, i.e. the fragment is computed transposed: lane l holds Y row (l & 15),
// columns 4 (l >> 4) .. +3 — one 8-byte LDS write in the epilogue instead of four 2-byte ones.
template <int QA, int QB, bool TR, int NF, int NF0>
__device__ __forceinline__ void p8_mma(f32x4 (&acc)[8][NF], const bf16x8 (&a)[4][2], const bf16x8 (&b)[NF0][2]) {
    constexpr int NB = QB ? NF - NF0 : NF0, G0 = QB ? NF0 : 0;
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int f = 0; f < 4; ++f)
#pragma unroll
            for (int g = 0; g < NB; ++g)
                acc[QA * 4 + f][G0 + g] =
                    TR ? __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[g][kk], a[f][kk], acc[QA * 4 + f][G0 + g], 0, 0, 0)
                       : __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[f][kk], b[g][kk], acc[QA * 4 + f][G0 + g], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
}

// Fragment reads with one per-lane base per k-substep: row r = r0 + 16 f keeps (r & 7) fixed, so
// fragment f is base[kk] + 2048 f (an immediate offset) — no per-fragment address registers.
__device__ __forceinline__ void p8_read_a(bf16x8 (&a)[4][2], const char* region, const int (&off)[2]) {
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int f = 0; f < 4; ++f) a[f][kk] = *reinterpret_cast<const bf16x8*>(region + off[kk] + f * 2048);
}
template <int NB, int NF0>
__device__ __forceinline__ void p8_read_b(bf16x8 (&b)[NF0][2], const char* region, const int (&off)[2]) {
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int g = 0; g < NB; ++g) b[g][kk] = *reinterpret_cast<const bf16x8*>(region + off[kk] + g * 2048);
}
__device__ __forceinline__ void p8_frag_offsets(int (&off)[2], int r0, int lane) {
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) off[kk] = r0 * 128 + ((((kk * 4) + (lane >> 4)) ^ (r0 & 7)) << 4);
}
// One phase: read the quadrant's fragments (RD: 0 = A+B, 1 = B only, 2 = A only; oB0 / oB1: the wave's
// fragment bases in B0 / B1, the same array when both regions have PER0 rows), issue one region's
// DMA (supplied by the caller), [early first K-tile wait], [vmcnt(VMC)], retire the reads, barrier,
// the quadrant's MFMAs, barrier.
template <class G, int QA, int QB, int RD, bool VM, bool EW, bool TR, class Issue>
__device__ __forceinline__ void p8_phase(f32x4 (&acc)[8][G::NF], bf16x8 (&a)[4][2], bf16x8 (&b)[G::NF0][2],
                                         const char* buf, const int (&oA)[2], const int (&oB0)[2], const int (&oB1)[2], Issue&& issue_dma) {
    if (RD != 2) p8_read_b<(QB ? G::NF1 : G::NF0)>(b, buf + (QB ? G::RB1 : G::RB0), QB ? oB1 : oB0);
    if (RD != 1) p8_read_a(a, buf + (QA ? G::RA1 : G::RA0), oA);
    issue_dma();
    if constexpr (EW) wait_vm<G::VMCE>();  // early first K-tile (no-op in steady state)
    if (VM) wait_vm<G::VMC>();
    P8_LGKM0();
    P8_BAR();
    p8_mma<QA, QB, TR>(acc, a, b);
    P8_BAR();
}

}  // namespace eggroll
