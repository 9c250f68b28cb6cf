// libeggroll — the DC-AE decoder's 3x3 / 2x2 convolutions for gfx950 (MI355X): the tap-staged
// implicit GEMM on the 8-phase ring (p8.h) and the halo-staged kernels.
#include "p8_epilogue.h"

namespace eggroll {

// ------------------------------------------------------------------------------------
// Implicit-GEMM 3x3 convolution (stride 1, zero pad 1), NHWC bf16, on the 8-phase template.
// The DC-AE decoder's ResBlock convs (models/SanaSprint.py:157-160 -> diffusers AutoencoderDC):
//   GEMM rows    = "super-pixels" of PX horizontally adjacent output pixels (M' = B*H*W/PX)
//   GEMM columns = PX * Cout (the PX pixels' output channels, contiguous in NHWC)
//   GEMM K       = 3 * (PX+2) taps * Cin: tap (ty, tx) reads input pixel (y+ty-1, x0+tx-1) of the
//                  super-pixel whose first pixel is x0; K-tile kt = (tap, 64-channel slice)
// Two tile shapes, the same 8-phase schedule and wave tile (128 x 64, 8 waves, BK = 64):
//   WMW = 2: 256 x 256 (2 x 4 waves) for PX * Cout >= 256.  PX = 2 serves Cout = 128 with a full
//            256-column tile, but the packed weight is zero where a tap does not touch a pixel
//            (25 % of the MACs).
//   WMW = 4: 512 x 128 (4 x 2 waves) for Cout = 128 at PX = 1 — no zero MACs.  The A half-tile is
//            32 KiB (4 DMAs per wave), the B half-tile 8 KiB (1 DMA); the ring is the whole 160 KiB.
// A operand: each lane's DMA rows keep ONE byte offset (its pixel, relative to a per-block buffer
// base) and a tap-validity bit mask; the tap's shift and channel slice go in the wave-uniform
// soffset, and a tap outside the image turns the lane's offset out of range (0x80000000 >
// num_records), which the buffer unit returns as zeros: the zero padding costs one v_cndmask
// per DMA.  B operand: the packed weight [PX*Cout][3][PX+2][Cin] streams like the GEMM's W.
// Epilogue: bias through the MFMA addend (one k-step), optional SiLU in fp32, one bf16 rounding.
// ------------------------------------------------------------------------------------
template <int ND>
struct ConvStage {
    uint32_t off[ND];   // lane byte offset of its pixel's channel chunk, tap (0,0) = pixel - (W+1)
    uint32_t mask[ND];  // bit t set: tap t reads inside the image
};

template <int PX, int KS, int ND>
__device__ __forceinline__ ConvStage<ND> make_conv_stage(int m0, int Mp, int H, int W, int Cin, int h, int wave,
                                                         int lane) {
    constexpr int TW = PX + KS - 1;
    const int Ho = H + 3 - KS, Ws = (W + 3 - KS) / PX;  // output grid (pad 1)
    // input pixel of a super-pixel row's first output pixel (monotone in the row index)
    auto pin = [&](int gr) -> int64_t {
        const int xs = gr % Ws, yrow = gr / Ws;
        return ((int64_t)(yrow / Ho) * H + yrow % Ho) * W + xs * PX;
    };
    const int64_t pin0 = pin(m0);
    ConvStage<ND> s;
#pragma unroll
    for (int i = 0; i < ND; ++i) {
        const int j = (i * 8 + wave) * 8 + (lane >> 3);  // region row (as make_stage_a)
        const int chunk = (lane & 7) ^ (j & 7);
        const int tr = (j >> 6) * 128 + h * 64 + (j & 63);  // wave row wm = j / 64
        const int gr = m0 + tr;
        uint32_t mk = 0;
        int64_t pg = pin0;
        if (gr < Mp) {
            const int xs = gr % Ws, yrow = gr / Ws, y = yrow % Ho;
            pg = pin(gr);
#pragma unroll
            for (int ty = 0; ty < KS; ++ty)
#pragma unroll
                for (int tx = 0; tx < TW; ++tx) {
                    const int yy = y + ty - 1, xx = xs * PX + tx - 1;
                    if (yy >= 0 && yy < H && xx >= 0 && xx < W) mk |= 1u << (ty * TW + tx);
                }
        }
        s.mask[i] = mk;
        s.off[i] = ((uint32_t)(pg - pin0) * (uint32_t)Cin + chunk * 8) * 2;  // from the block base pixel + (W+1)
    }
    return s;
}

template <int ND>
__device__ __forceinline__ void issue_conv_half(__amdgpu_buffer_rsrc_t rs, const ConvStage<ND>& s, int tap, int kbytes,
                                                char* region, int wave) {
#pragma unroll
    for (int i = 0; i < ND; ++i) {
        const uint32_t v = ((s.mask[i] >> tap) & 1u) ? s.off[i] : 0x80000000u;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void*)(region + (i * 8 + wave) * 1024), 16, v, kbytes, 0, 0);
    }
}

// store_tile_t with an optional fp32 SiLU before the bf16 rounding
template <int ACT>
__device__ __forceinline__ void store_tile_t_act(f32x4 (&acc)[8][4], char* smem, int wave, int lane, int m0, int n0,
                                                 int rbase, int cbase, int M, int N, unsigned short* __restrict__ Y,
                                                 int64_t ldy) {
    if constexpr (ACT == 1) {
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int e = 0; e < 4; e += 2) {
                    const f32x2 t = silu2((f32x2){acc[i][j][e], acc[i][j][e + 1]});
                    acc[i][j][e] = t.x;
                    acc[i][j][e + 1] = t.y;
                }
    }
    store_tile_t(acc, smem, wave, lane, m0, n0, rbase, cbase, M, N, Y, ldy);
}

// ResBlock tail fused into conv2's epilogue (NORM): RMSNorm over each pixel's COUT = BN / PX
// channels (a tile holds whole pixels: N = BN), * w[c] + b[c] + res[row, col], on the fp32
// accumulators.  Row sums of squares: 16 values per lane, xor-16/32 shuffles across the wave's 4
// column lanes, then a [BM rows][WNW waves] LDS table for the WPP = COUT / 64 waves that share a
// pixel, summed in a fixed order.
// RowOf(tile row) -> the row of res (and of the output) that tile row holds.
template <int PX, int WMW, int WNW = 8 / WMW, class RowOf>
__device__ __forceinline__ void conv_rmsnorm_epilogue(f32x4 (&acc)[8][4], float* red, int wm, int wn, int lane,
                                                      RowOf row_of, float eps, const unsigned short* __restrict__ nw,
                                                      const unsigned short* __restrict__ nb,
                                                      const unsigned short* __restrict__ res) {
    constexpr int BN = WNW * 64, COUT = BN / PX, WPP = COUT / 64;
    static_assert(WPP == 2 || WPP == 4, "a pixel spans 2 or 4 waves");
    const int rl = lane & 15, cg = lane >> 4;
    // norm weight / bias: 4 consecutive channels per load, issued ahead of the row-sum barrier
    u16x4 wq[4], bq[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c4 = (wn * 64 + 16 * j + 4 * cg) % COUT;
        wq[j] = *reinterpret_cast<const u16x4*>(nw + c4);
        bq[j] = nb ? *reinterpret_cast<const u16x4*>(nb + c4) : u16x4{0, 0, 0, 0};
    }
    float ss[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        float sq = 0.0f;
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) sq += acc[i][j][e] * acc[i][j][e];
        // xor-16 then xor-32 butterfly on v_permlane16_swap / v_permlane32_swap (VALU; the ds_bpermute
        // shuffles were LDS round trips): each returns the lane's own value and its partner's, whose sum
        // is the butterfly step — the same additions, the same bits
        {
            const auto r16 = __builtin_amdgcn_permlane16_swap(__builtin_bit_cast(unsigned, sq),
                                                              __builtin_bit_cast(unsigned, sq), false, false);
            sq = __builtin_bit_cast(float, (unsigned)r16[0]) + __builtin_bit_cast(float, (unsigned)r16[1]);
            const auto r32 = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, sq),
                                                              __builtin_bit_cast(unsigned, sq), false, false);
            sq = __builtin_bit_cast(float, (unsigned)r32[0]) + __builtin_bit_cast(float, (unsigned)r32[1]);
        }
        ss[i] = sq;
    }
    if (cg == 0)
#pragma unroll
        for (int i = 0; i < 8; ++i) red[(wm * 128 + 16 * i + rl) * WNW + wn] = ss[i];
    __syncthreads();
    float wv[4][4], bv[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            wv[j][e] = bf16_to_f32(wq[j][e]);
            bv[j][e] = bf16_to_f32(bq[j][e]);
        }
    const int w0 = (wn / WPP) * WPP;  // first wave of this pixel
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int rr = wm * 128 + 16 * i + rl;
        const float* rp = red + rr * WNW + w0;
        const float tot = WPP == 4 ? (rp[0] + rp[1]) + (rp[2] + rp[3]) : rp[0] + rp[1];
        const float rs = rsqrtf(tot / COUT + eps);
        const int64_t row = row_of(rr);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (res) {
                const u16x4 r4 = *reinterpret_cast<const u16x4*>(res + row * BN + wn * 64 + 16 * j + 4 * cg);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[i][j][e] = acc[i][j][e] * rs * wv[j][e] + bv[j][e] + bf16_to_f32(r4[e]);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[i][j][e] = acc[i][j][e] * rs * wv[j][e] + bv[j][e];
            }
        }
    }
}

// DC-AE up-block epilogue (eggroll_conv2x2_subpixel_nhwc): the phase conv's C tile goes straight to the
// up-sampled output instead of a y4 [B, H+1, W+1, 4*Cout] intermediate read back by
// k_subpixel_shortcut4.  Row = phase-conv position (b, h', w') of the (H+1) x (W+1) grid, column =
// (phase k = 2i + j, output channel): out[b, 2h + i, 2w + j, c] = bf16(y) + bias[c] + src[b, h, w,
// (4c + k) / REP] with (h, w) = (h' - i, w' - j) (positions with h or w outside the input are dropped),
// y rounded to bf16 first and the two adds in that order — the arithmetic of k_subpixel_shortcut4, so the
// output is bitwise the two-kernel path's.  SP 1: bf16 src and out; SP 2: fp32 src (the DC-AE fp32
// residual stream) and fp32 out, plus its bf16 shadow when given.
struct SubpixArgs {
    const unsigned short* bias;  // [Cout] or null
    const void* src;             // shortcut source [B, H, W, Cin]
    void* out;                   // [B, 2H, 2W, Cout]
    unsigned short* shadow;      // SP 2: optional bf16 copy of out
    int H, W, Cin, Cout;
};

#ifndef EGG_SPX_REGS  // VGPRs of shortcut words in flight per batch in the sub-pixel epilogue (A/B knob)
#define EGG_SPX_REGS 64
#endif
// KP: the wave's phase (wave-uniform, dispatched by the caller) — a compile-time shortcut channel index
template <int SP, int REP, int KP>
__device__ __forceinline__ void store_tile_subpix(f32x4 (&acc)[8][4], char* smem, int wave, int lane, int rbase,
                                                  int col0, int Mp, const SubpixArgs& sp) {
    constexpr int ROWB = 128, SLOTS = 8;
    constexpr int XW = 32 / REP;                     // shortcut channels spanned by 8 outputs
    constexpr int WD = SP == 2 ? XW : XW / 2;        // their dwords (raw, converted at use)
    // rows whose shortcut loads are in flight together (<= EGG_SPX_REGS VGPRs of raw shortcut words)
    constexpr int RBAT_ = EGG_SPX_REGS / WD > 16 ? 16 : (EGG_SPX_REGS / WD > 0 ? EGG_SPX_REGS / WD : 1);
    constexpr int RBAT = 16 % RBAT_ == 0 ? RBAT_ : 8;
    char* ctile = smem + wave * (128 * ROWB);
    {
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
    }
    // the wave's 64 columns lie in one phase (Cout % 64 == 0, host-checked)
    constexpr int k = KP, pi = KP >> 1, pj = KP & 1;
    const int c0 = col0 - k * sp.Cout + (lane & 7) * 8;
    float bv[8];
    if (sp.bias) {
        const u16x8 q = *reinterpret_cast<const u16x8*>(sp.bias + c0);
#pragma unroll
        for (int e = 0; e < 8; ++e) bv[e] = bf16_to_f32(q[e]);
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) bv[e] = 0.f;
    }
    const int H = sp.H, W = sp.W, Ho = H + 1, Wo = W + 1;
    int p = rbase + (lane >> 3);
    int bb = p / (Ho * Wo), hp = (p - bb * Ho * Wo) / Wo, wp = p - bb * Ho * Wo - hp * Wo;
    __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): this wave's LDS writes done (wave-private tile)
#pragma unroll
    for (int it0 = 0; it0 < 16; it0 += RBAT) {
        uint32_t raw[RBAT][WD];
        int32_t opix[RBAT];   // B * 4 * H * W * Cout < 2^31 (host check): pixel and element offsets fit 32 bits
        bool ok[RBAT];
#pragma unroll
        for (int u = 0; u < RBAT; ++u) {
            const int h = hp - pi, w = wp - pj;
            ok[u] = p < Mp && h >= 0 && h < H && w >= 0 && w < W;
            const int64_t lp = ok[u] ? ((int64_t)bb * H + h) * W + w : 0;
            opix[u] = (bb * 2 * H + 2 * h + pi) * (2 * W) + 2 * w + pj;
            // window of channels (4c + k) / REP, c = c0 .. c0+7: XW channels from 4 c0 / REP
            const uint32_t* src = reinterpret_cast<const uint32_t*>(
                reinterpret_cast<const char*>(sp.src) + (lp * sp.Cin + 4 * c0 / REP) * (SP == 2 ? 4 : 2));
#pragma unroll
            for (int t = 0; t < WD / 4; ++t) {
                typedef __attribute__((ext_vector_type(4))) unsigned int sp_u32x4;
                const sp_u32x4 q = *reinterpret_cast<const sp_u32x4*>(src + 4 * t);
#pragma unroll
                for (int e = 0; e < 4; ++e) raw[u][4 * t + e] = q[e];
            }
            p += 8;
            wp += 8;
            while (wp >= Wo) {
                wp -= Wo;
                if (++hp == Ho) { hp = 0; ++bb; }
            }
        }
#pragma unroll
        for (int u = 0; u < RBAT; ++u) {
            const int it = it0 + u, rr = it * 8 + (lane >> 3), sl = lane & 7;
            const u16x8 v = *reinterpret_cast<const u16x8*>(ctile + rr * ROWB + ((sl ^ (rr & (SLOTS - 1))) << 4));
            if (!ok[u]) continue;
            float f[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int ch = (4 * q + k) / REP;  // compile-time: q unrolled, k = KP
                const float xsv = SP == 2 ? __uint_as_float(raw[u][ch])
                                          : bf16_to_f32((unsigned short)(raw[u][ch >> 1] >> (16 * (ch & 1))));
                f[q] = bf16_to_f32(v[q]) + bv[q] + xsv;
            }
            const int32_t oo = opix[u] * sp.Cout + c0;
            if constexpr (SP == 2) {
                float* o32 = reinterpret_cast<float*>(sp.out) + oo;
                *reinterpret_cast<f32x4*>(o32) = f32x4{f[0], f[1], f[2], f[3]};
                *reinterpret_cast<f32x4*>(o32 + 4) = f32x4{f[4], f[5], f[6], f[7]};
            }
            if (SP == 1 || sp.shadow) {
                u16x8 o;
#pragma unroll
                for (int q = 0; q < 8; ++q) o[q] = f32_to_bf16(f[q]);
                *reinterpret_cast<u16x8*>((SP == 2 ? sp.shadow : reinterpret_cast<unsigned short*>(sp.out)) + oo) = o;
            }
        }
    }
}

template <int WMW, bool NORM>
constexpr int conv_smem_bytes() {
    using G = G8<WMW>;
    constexpr int need = G::CSTAGE + (NORM ? G::BM * G::WNW * 4 : 0);  // RMSNorm table after the C staging
    return G::LDS > need ? G::LDS : need;
}

template <int PX, int ACT, bool NORM = false, int KS = 3, int WMW = 2, int SP = 0, int REP = 2>
__global__ __launch_bounds__(512, 1) void k_conv3x3_gemm8(const unsigned short* __restrict__ X,
                                                          const unsigned short* __restrict__ Wt,
                                                          const unsigned short* __restrict__ bias, int H, int W,
                                                          int Cin, int lcpt, int Mp, int N, int tiles_n,
                                                          unsigned short* __restrict__ Y, float eps = 0.0f,
                                                          const unsigned short* __restrict__ nw = nullptr,
                                                          const unsigned short* __restrict__ nb = nullptr,
                                                          const unsigned short* __restrict__ res = nullptr,
                                                          SubpixArgs spa = SubpixArgs{}) {
    static_assert(SP == 0 || (KS == 2 && PX == 1 && ACT == 0 && !NORM), "sub-pixel epilogue: the up-block phase conv");
    using G = G8<WMW>;
    constexpr int TW = PX + KS - 1;
    __shared__ __attribute__((aligned(16))) char smem[conv_smem_bytes<WMW, NORM>()];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / G::WNW, wn = wave % G::WNW;
    const int grp8 = wave >> 2;  // the two staggered wave groups (one wave of each per SIMD)
    const TileIdx ti = p8_tile_index<G::BM>(Mp, tiles_n);
    const int m0 = ti.m * G::BM, n0 = ti.n * G::BN;
    const int64_t K = (int64_t)KS * TW * Cin;
    const int nk = (int)(K / BK);
    EGG_STAMP_RT(6);
    EGG_STAMP(0);

    const ConvStage<G::NA> sA0 = make_conv_stage<PX, KS, G::NA>(m0, Mp, H, W, Cin, 0, wave, lane);
    const ConvStage<G::NA> sA1 = make_conv_stage<PX, KS, G::NA>(m0, Mp, H, W, Cin, 1, wave, lane);
    const Stage<G::NB0> sB0 = make_stage_b<G, 0>(n0, N - 1, K, wave, lane);
    const Stage<G::NB1> sB1 = make_stage_b<G, 1>(n0, N - 1, K, wave, lane);
    char* const e_buf = smem;
    char* const o_buf = smem + G::BUF;
    // block base = input pixel of output row m0, minus (W+1); tap (ty, tx) adds (ty*W + tx) pixels in
    // soffset, so every address offset is >= 0
    int64_t pin0;
    {
        const int Ho = H + 3 - KS, Ws = (W + 3 - KS) / PX, xs = m0 % Ws, yrow = m0 / Ws;
        pin0 = ((int64_t)(yrow / Ho) * H + yrow % Ho) * W + xs * PX;
    }
    // (readfirstlane: the divisions above run on the VALU; an SGPR resource keeps every DMA a single
    // instruction instead of a readfirstlane waterfall)
    const uint64_t xbu = (uint64_t)(X + (pin0 - W - 1) * Cin);
    const unsigned short* xb = (const unsigned short*)(
        ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(xbu >> 32)) << 32) |
        (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)xbu));
    const __amdgpu_buffer_rsrc_t rX = __builtin_amdgcn_make_buffer_rsrc((void*)xb, (short)0, 0x7fffffff, 0x00020000);
    const __amdgpu_buffer_rsrc_t rW = __builtin_amdgcn_make_buffer_rsrc((void*)Wt, (short)0, 0x7fffffff, 0x00020000);

    f32x4 acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    bf16x8 a[4][2], b[2][2];
    int oA[2], oB[2];
    p8_frag_offsets(oA, wm * 64 + (lane & 15), lane);
    p8_frag_offsets(oB, wn * G::PER0 + (lane & 15), lane);  // B0 and B1: PER0 == PER1

    const int cmask = (1 << lcpt) - 1;
    // K-tile t (clamped to the last one, as the GEMM): tap = t >> lcpt, channel slice t & cmask
    auto A = [&](const ConvStage<G::NA>& s, int t, char* dst) {
        t = t < nk ? t : nk - 1;
        const int tap = t >> lcpt, ty = tap / TW, tx = tap - ty * TW;
        const int soff = __builtin_amdgcn_readfirstlane(((ty * W + tx) * Cin + (t & cmask) * BK) * 2);
        issue_conv_half(rX, s, tap, soff, dst, wave);
    };
    auto B = [&](const Stage<G::NB0>& s, int t, char* dst) {
        t = t < nk ? t : nk - 1;
        issue(rW, s, t * (BK * 2), dst, wave);
    };
    A(sA0, 0, e_buf + G::RA0);
    B(sB0, 0, e_buf + G::RB0);
    B(sB1, 0, e_buf + G::RB1);
    A(sA1, 0, e_buf + G::RA1);
    A(sA0, 1, o_buf + G::RA0);
    B(sB1, 1, o_buf + G::RB1);
    A(sA1, 1, o_buf + G::RA1);
    wait_vm<G::VMC0>();  // K-tile 0's A0 + B0 only (early first K-tile, see G8)
    P8_BAR();
    EGG_STAMP(1);
    if (grp8 == 1) P8_BAR();

    int t0 = 0;
    for (; t0 + 1 < nk; t0 += 2) {
        p8_phase<G, 0, 0, 0, false, true, true>(acc, a, b, e_buf, oA, oB, oB, [&] { B(sB0, t0 + 1, o_buf + G::RB0); });
        p8_phase<G, 0, 1, 1, false, true, true>(acc, a, b, e_buf, oA, oB, oB, [&] { A(sA0, t0 + 2, e_buf + G::RA0); });
        p8_phase<G, 1, 1, 2, false, false, true>(acc, a, b, e_buf, oA, oB, oB, [&] { B(sB1, t0 + 2, e_buf + G::RB1); });
        p8_phase<G, 1, 0, 1, true, false, true>(acc, a, b, e_buf, oA, oB, oB, [&] { A(sA1, t0 + 2, e_buf + G::RA1); });
        p8_phase<G, 0, 0, 0, false, false, true>(acc, a, b, o_buf, oA, oB, oB, [&] { B(sB0, t0 + 2, e_buf + G::RB0); });
        p8_phase<G, 0, 1, 1, false, false, true>(acc, a, b, o_buf, oA, oB, oB, [&] { A(sA0, t0 + 3, o_buf + G::RA0); });
        p8_phase<G, 1, 1, 2, false, false, true>(acc, a, b, o_buf, oA, oB, oB, [&] { B(sB1, t0 + 3, o_buf + G::RB1); });
        p8_phase<G, 1, 0, 1, true, false, true>(acc, a, b, o_buf, oA, oB, oB, [&] { A(sA1, t0 + 3, o_buf + G::RA1); });
    }
    if (t0 < nk) {
        p8_phase<G, 0, 0, 0, false, true, true>(acc, a, b, e_buf, oA, oB, oB, [&] { B(sB0, t0 + 1, o_buf + G::RB0); });
        p8_phase<G, 0, 1, 1, false, true, true>(acc, a, b, e_buf, oA, oB, oB, [&] { A(sA0, t0 + 2, e_buf + G::RA0); });
        p8_phase<G, 1, 1, 2, false, false, true>(acc, a, b, e_buf, oA, oB, oB, [&] { B(sB1, t0 + 2, e_buf + G::RB1); });
        p8_phase<G, 1, 0, 1, false, false, true>(acc, a, b, e_buf, oA, oB, oB, [&] { A(sA1, t0 + 2, e_buf + G::RA1); });
    }
    if (grp8 == 0) P8_BAR();
    EGG_STAMP(2);
    wait_vm<0>();
    __syncthreads();
    EGG_STAMP(3);
    if (bias)
        lora_mfma_addend<0>(acc, lane, m0, n0, wm * 128, wn * 64, bias, nullptr, nullptr, 0, 0, 0.0f, 1 << 30, Mp, N);
    if constexpr (SP != 0) {
        EGG_STAMP(4);
        const int kp = __builtin_amdgcn_readfirstlane((n0 + wn * 64) / spa.Cout);
        if (kp == 0) store_tile_subpix<SP, REP, 0>(acc, smem, wave, lane, m0 + wm * 128, n0 + wn * 64, Mp, spa);
        else if (kp == 1) store_tile_subpix<SP, REP, 1>(acc, smem, wave, lane, m0 + wm * 128, n0 + wn * 64, Mp, spa);
        else if (kp == 2) store_tile_subpix<SP, REP, 2>(acc, smem, wave, lane, m0 + wm * 128, n0 + wn * 64, Mp, spa);
        else store_tile_subpix<SP, REP, 3>(acc, smem, wave, lane, m0 + wm * 128, n0 + wn * 64, Mp, spa);
    } else if constexpr (NORM) {
        conv_rmsnorm_epilogue<PX, WMW>(
            acc, reinterpret_cast<float*>(smem + G::CSTAGE), wm, wn, lane,
            [&](int rr) -> int64_t { return m0 + rr < Mp ? m0 + rr : Mp - 1; }, eps, nw, nb, res);
        EGG_STAMP(4);
        store_tile_t(acc, smem, wave, lane, m0, n0, wm * 128, wn * 64, Mp, N, Y, N);
    } else {
        EGG_STAMP(4);
        store_tile_t_act<ACT>(acc, smem, wave, lane, m0, n0, wm * 128, wn * 64, Mp, N, Y, N);
    }
    EGG_STAMP_DRAIN();
    EGG_STAMP(5);
    EGG_STAMP_RT(7);
}

// ------------------------------------------------------------------------------------
// Halo-staged 3x3 conv (stride 1, pad 1, px 1): the tile-sliced implicit GEMM above re-stages its
// A operand once per tap (9 x the input bytes through the LDS-DMA path, which is what bounds it:
// DESIGN.md §5).  Here a tile is TH x TWD output pixels (16 x 32 for the 512 x 128 tile, 16 x 16
// for 256 x 256) and its (TH+2) x (TWD+2) input halo is staged ONCE per 32-channel slice; the nine
// taps read their A fragments from it at a pixel shift.  K-step = (slice, tap), K = 32:
//   halo    [halo pixel][32 ch] bf16, 64-B rows, double-buffered by slice: slice s+1 streams in as
//           one 1-KiB piece per wave at taps 0..NPW-1 of slice s
//   weights [BN rows][32 ch] per K-step, a ring of D+1 slots, K-step k+D issued during step k
// 64-B rows read as 16x16x32 fragments (lane: row l&15, chunk l>>4) are bank-conflict-free for any
// run of 16 consecutive rows with slot = chunk ^ 2*((row >> 2) & 1), i.e. byte L -> L ^ ((L>>3)&32);
// the tap shift is added to the logical byte before the swizzle.  Per K-step each wave runs two
// phases of 16 MFMAs (A fragments 0-3, then 4-7, against the same 4 B fragments) with the p8 wave-
// group stagger; all DMA waits are counted vmcnt (compile-time per tap, see hc_wait_n).
// ------------------------------------------------------------------------------------
// Halo rows are padded: HS = HW2 rounded up to 8 pixels (the pad columns are zero-filled, never read).
// The fragment swizzle keys on bit 2 of the halo pixel index; with HS % 8 == 0 a tap's row shift dy (HS
// pixels) leaves that bit alone, so a fragment needs one swizzled address per column shift dx and the
// row shift is the ds_read immediate (3 addresses per fragment instead of 9: 24 VGPRs instead of 72).
template <int WMW, int WNW = 8 / WMW>
struct HC {
    static_assert(WMW * WNW == 8, "one 8-wave workgroup per CU");
    static constexpr int WM_ = WMW, WN_ = WNW;
    static constexpr int NW = WMW * WNW, BM = WMW * 128, BN = WNW * 64;  // waves, tile
    static constexpr int TH = 16, TWD = BM / TH;                 // output pixels of a tile
    static constexpr int HW2 = TWD + 2;                          // halo pixels per row
    static constexpr int HS = (HW2 + 7) / 8 * 8;                 // halo row stride in LDS (pixels)
    static constexpr int HP = (TH + 2) * HS;                     // halo pixel slots
    static constexpr int NPW = (HP + 16 * NW - 1) / (16 * NW);  // halo pieces (16 px x 64 B) per wave
    static constexpr int HALO = NPW * NW * 1024;
    static constexpr int NBW = BN / (16 * NW);                    // weight pieces per wave per K-step
    static constexpr int BSLOT = BN * 64;
    static constexpr int D = 3, NBUF = D + 1;                     // weight prefetch distance / ring slots
    static constexpr int RB = 2 * HALO, LDS = 2 * HALO + NBUF * BSLOT;
    // the halo of slice s+1 (taps 0..NPW-1 of slice s) is older than the weights of K-step (s+1, 0)
    // (issued at tap 9-D of slice s), so the weight wait also retires the halo
    static_assert(NPW <= 9 - D, "halo pieces must precede the next slice's first weight DMA");
    static constexpr int CSTAGE = NW * 128 * 64 * 2;               // epilogue C staging (one 128x64 tile per wave)
    static_assert(NBW >= 1 && BN % (16 * NW) == 0, "weight pieces");
};

__device__ __forceinline__ uint32_t hc_swz(uint32_t L) { return L ^ ((L >> 3) & 32u); }

// DMAs younger than K-step k+1's weights when step k (tap T) retires them in its second phase
template <class G, int T, bool NEXT, bool LAST>
constexpr int hc_wait_n() {
    int n = 0;
    for (int i = 2; i <= G::D; ++i)
        if (!LAST || T + i < 9) n += G::NBW;
    if (NEXT)
        for (int t = T + 1 - G::D; t <= T; ++t)
            if (t >= 0 && t < G::NPW) n += 1;
    return n;
}

template <int I, int N, class F>
__device__ __forceinline__ void hc_static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        hc_static_for<I + 1, N>(f);
    }
}

template <class G, bool NORM>
constexpr int halo_smem_bytes() {
    constexpr int need = G::CSTAGE + (NORM ? G::BM * G::WN_ * 4 : 0);
    return G::LDS > need ? G::LDS : need;
}

// store_tile_t (fast path only: every conv tile is full) with tile row -> output row through row_of
// the residual rows of a wave's 128 x 64 tile as coalesced 16-B loads (store_tile_rows' order)
template <int I0 = 0, int I1 = 16, class RowOf, int NR>
__device__ __forceinline__ void load_res_rows(u16x8 (&rv)[NR], const unsigned short* __restrict__ res, int lane,
                                              int rbase, int col0, int64_t ldy, RowOf row_of) {
#pragma unroll
    for (int it = I0; it < I1; ++it)
        rv[it] = *reinterpret_cast<const u16x8*>(res + row_of(rbase + it * 8 + (lane >> 3)) * ldy + col0 + (lane & 7) * 8);
}

// NT: the tile may reach past the N = ldy output columns; a lane's 16-byte chunk of 8 columns is stored only
// where it starts below N (N % 8 == 0 makes that chunk-exact).  The full-tile form has no such test.
template <int ACT, class RowOf, bool RES = false, bool PRE = false, bool NT = false>
__device__ __forceinline__ void store_tile_rows(f32x4 (&acc)[8][4], char* smem, int wave, int lane, int rbase,
                                                int col0, unsigned short* __restrict__ Y, int64_t ldy, RowOf row_of,
                                                const unsigned short* __restrict__ res = nullptr,
                                                const u16x8* pre = nullptr) {
    static_assert(!(NT && RES), "the column tail has no residual form");
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
            for (int e = 0; e < 4; e += 2) {
                f32x2 v = {acc[i][j][e], acc[i][j][e + 1]};
                if constexpr (ACT == 1) v = silu2(v);
                o[e] = f32_to_bf16(v.x);
                o[e + 1] = f32_to_bf16(v.y);
            }
            *reinterpret_cast<u16x4*>(ctile + rr * ROWB + slot * 16 + (cc & 7) * 2) = o;
        }
    }
    u16x8 rv[RES ? 16 : 1];
    if constexpr (RES) {  // residual rows as coalesced 16-B loads, in flight while the tile goes through LDS
        if constexpr (PRE) {  // the first 8 rows were loaded by the caller
#pragma unroll
            for (int it = 0; it < 8; ++it) rv[it] = pre[it];
            load_res_rows<8, 16>(rv, res, lane, rbase, col0, ldy, row_of);
        } else {
            load_res_rows(rv, res, lane, rbase, col0, ldy, row_of);
        }
    }
    __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): this wave's LDS writes done (wave-private tile)
    u16x8 v[16];
#pragma unroll
    for (int it = 0; it < 16; ++it) {
        const int rr = it * 8 + (lane >> 3), sl = lane & 7;
        v[it] = *reinterpret_cast<const u16x8*>(ctile + rr * ROWB + ((sl ^ (rr & (SLOTS - 1))) << 4));
    }
#pragma unroll
    for (int it = 0; it < 16; ++it) {
        const int rr = it * 8 + (lane >> 3);
        if constexpr (RES) {
#pragma unroll
            for (int u = 0; u < 8; ++u) v[it][u] = f32_to_bf16(bf16_to_f32(v[it][u]) + bf16_to_f32(rv[it][u]));
        }
        if constexpr (NT) {
            if (col0 + (lane & 7) * 8 >= ldy) continue;
        }
        *reinterpret_cast<u16x8*>(Y + row_of(rbase + rr) * ldy + col0 + (lane & 7) * 8) = v[it];
    }
}

// WMW x WNW waves: (4, 2) 512 x 128 and (2, 4) 256 x 256 tiles run one 8-wave workgroup per CU
// with the two wave groups staggered by a barrier (as the p8 kernels).
// NTAIL: the last column tile may be partial (N % BN != 0).  Weight rows at or past N are never addressed: their
// DMA offset is the out-of-range one of the halo's padding, so the rows arrive as zeros while every wave still
// issues NBW DMAs per K-step (hc_wait_n's counts hold); the bias addend clamps its column to N - 1; the store
// drops the 16-byte chunks at or past N.  NTAIL = false is the full-tile kernel, instruction for instruction.
template <int ACT, bool NORM, int WMW, int WNW, bool NTAIL = false>
__global__ __launch_bounds__(512, 1) void k_conv3x3_halo(const unsigned short* __restrict__ X,
                                                         const unsigned short* __restrict__ Wt,
                                                         const unsigned short* __restrict__ bias, int H, int W,
                                                         int Cin, int N, int tiles_n, unsigned short* __restrict__ Y,
                                                         float eps = 0.0f, const unsigned short* __restrict__ nw = nullptr,
                                                         const unsigned short* __restrict__ nb = nullptr,
                                                         const unsigned short* __restrict__ res = nullptr) {
    using G = HC<WMW, WNW>;
    static_assert(halo_smem_bytes<G, NORM>() <= 160 * 1024, "LDS per CU");
    static_assert(!(NTAIL && NORM), "the RMSNorm tail needs whole pixels in one tile");
    __shared__ __attribute__((aligned(16))) char smem[halo_smem_bytes<G, NORM>()];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WNW, wn = wave % WNW;
    const int grp8 = wave >> 2;
    // XCD-contiguous tile ranges (neighbouring tiles share halo rows and all share the weights);
    // the N-tiles of one pixel tile are adjacent
    const int tile = xcd_remap(blockIdx.x, gridDim.x);
    const int tm = tile / tiles_n, tn = tile - tm * tiles_n;
    const int n0 = tn * G::BN;
    const int tpr = W / G::TWD, tpi = (H / G::TH) * tpr;
    const int img = tm / tpi, trm = tm - img * tpi;
    const int y0 = (trm / tpr) * G::TH, x0 = (trm - (trm / tpr) * tpr) * G::TWD;
    const int K = 9 * Cin, S = Cin / 32;
    EGG_STAMP_RT(6);
    EGG_STAMP(0);

    // halo DMA: piece i*8 + wave holds halo pixels 16p .. 16p+15; out-of-image pixels (and the pad
    // past HP) read as zeros through an out-of-range offset
    uint32_t hoff[G::NPW];
#pragma unroll
    for (int i = 0; i < G::NPW; ++i) {
        const int hp = (i * G::NW + wave) * 16 + (lane >> 2);
        const int c = (lane & 3) ^ (((hp >> 2) & 1) << 1);
        const int hy = hp / G::HS, hx = hp - hy * G::HS;
        const int y = y0 - 1 + hy, x = x0 - 1 + hx;
        const bool ok = hp < G::HP && hx < G::HW2 && y >= 0 && y < H && x >= 0 && x < W;
        hoff[i] = ok ? (uint32_t)(((hy * W + hx) * Cin + c * 8) * 2) : 0x80000000u;
    }
    uint32_t boff[G::NBW];
#pragma unroll
    for (int i = 0; i < G::NBW; ++i) {
        const int n = (i * G::NW + wave) * 16 + (lane >> 2);
        const int c = (lane & 3) ^ (((n >> 2) & 1) << 1);
        boff[i] = !NTAIL || n0 + n < N ? (uint32_t)(((n0 + n) * K + c * 8) * 2) : 0x80000000u;
    }
    // fragment reads: A row f of the wave at tap (0,0) as a logical halo byte la, then the swizzled
    // byte of A row f at column shift dx (row shift dy = immediate dy * HS * 64)
    uint32_t ad[8][3];
#pragma unroll
    for (int f = 0; f < 8; ++f) {
        const int m = wm * 128 + 16 * f + (lane & 15);
        const int ty = m / G::TWD, tx = m % G::TWD;
        const uint32_t la = (uint32_t)((ty * G::HS + tx) * 64 + (lane >> 4) * 16);
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) ad[f][dx] = hc_swz(la + dx * 64);
    }
    auto afrag = [&](const char* hb, int f, auto T_) -> bf16x8 {
        constexpr int T = decltype(T_)::value;
        return *reinterpret_cast<const bf16x8*>(hb + ad[f][T % 3] + (T / 3) * G::HS * 64);
    };
    const uint32_t lb = hc_swz((uint32_t)((wn * 64 + (lane & 15)) * 64 + (lane >> 4) * 16));

    const int64_t pb = ((int64_t)img * H + y0 - 1) * W + (x0 - 1);  // halo pixel (0, 0)
    const uint64_t xbu = (uint64_t)(X + pb * Cin);
    const unsigned short* xb = (const unsigned short*)(
        ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(xbu >> 32)) << 32) |
        (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)xbu));
    const __amdgpu_buffer_rsrc_t rX = __builtin_amdgcn_make_buffer_rsrc((void*)xb, (short)0, 0x7fffffff, 0x00020000);
    const __amdgpu_buffer_rsrc_t rW = __builtin_amdgcn_make_buffer_rsrc((void*)Wt, (short)0, 0x7fffffff, 0x00020000);

    auto issue_b = [&](int sl, int tap, int slot) {
        const int so = __builtin_amdgcn_readfirstlane((tap * Cin + sl * 32) * 2);
        char* dst = smem + G::RB + slot * G::BSLOT;
#pragma unroll
        for (int i = 0; i < G::NBW; ++i) {
            const uint32_t v = boff[i];
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rW, (lds_void*)(dst + (i * G::NW + wave) * 1024), 16, v, so, 0, 0);
        }
    };
    auto issue_h = [&](auto I, int sl) {
        constexpr int i = decltype(I)::value;
        const uint32_t v = hoff[i];
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rX, (lds_void*)(smem + (sl & 1) * G::HALO + (i * G::NW + wave) * 1024),
                                                 16, v, sl * 64, 0, 0);
    };

    f32x4 acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    bf16x8 a[4], b[4];

    hc_static_for<0, G::NPW>([&](auto I) { issue_h(I, 0); });
#pragma unroll
    for (int d = 0; d < G::D; ++d) issue_b(0, d, d);
    wait_vm<(G::D - 1) * G::NBW>();  // halo 0 + weights of K-step 0
    P8_BAR();
    EGG_STAMP(1);
    if (grp8 == 1) P8_BAR();

    auto slice = [&](int s, auto NEXT_, auto LAST_) {
        constexpr bool NEXT = decltype(NEXT_)::value, LAST = decltype(LAST_)::value;
        const char* hb = smem + (s & 1) * G::HALO;
        hc_static_for<0, 9>([&](auto T_) {
            constexpr int T = decltype(T_)::value;
            const int k = s * 9 + T;
            const char* bs = smem + G::RB + (k & (G::NBUF - 1)) * G::BSLOT;
            // phase 1: weights + A fragments 0-3, prefetch K-step k+D's weights
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = *reinterpret_cast<const bf16x8*>(bs + lb + j * 1024);
#pragma unroll
            for (int u = 0; u < 4; ++u) a[u] = afrag(hb, u, T_);
            if constexpr (!LAST || T + G::D < 9) {
                if constexpr (T + G::D < 9) issue_b(s, T + G::D, (k + G::D) & (G::NBUF - 1));
                else issue_b(s + 1, T + G::D - 9, (k + G::D) & (G::NBUF - 1));
            }
            P8_LGKM0();
            P8_BAR();
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[u][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[j], a[u], acc[u][j], 0, 0, 0);
            __builtin_amdgcn_s_setprio(0);
            P8_BAR();
            // phase 2: A fragments 4-7, one halo piece of slice s+1, retire K-step k+1's weights
#pragma unroll
            for (int u = 0; u < 4; ++u) a[u] = afrag(hb, 4 + u, T_);
            if constexpr (NEXT && T < G::NPW) issue_h(std::integral_constant<int, T>{}, s + 1);
            if constexpr (!(LAST && T == 8)) wait_vm<hc_wait_n<G, T, NEXT, LAST>()>();
            P8_LGKM0();
            P8_BAR();
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[4 + u][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[j], a[u], acc[4 + u][j], 0, 0, 0);
            __builtin_amdgcn_s_setprio(0);
            P8_BAR();
        });
    };
    for (int s = 0; s < S - 1; ++s) slice(s, std::true_type{}, std::false_type{});
    slice(S - 1, std::false_type{}, std::true_type{});
    if (grp8 == 0) P8_BAR();
    EGG_STAMP(2);
    wait_vm<0>();
    __syncthreads();
    EGG_STAMP(3);
    const int64_t prow = ((int64_t)img * H + y0) * W + x0;  // output pixel of tile row 0
    auto row_of = [&](int r) -> int64_t { return prow + (int64_t)(r / G::TWD) * W + (r % G::TWD); };
    if (bias)
        lora_mfma_addend<0>(acc, lane, 0, n0, wm * 128, wn * 64, bias, nullptr, nullptr, 0, 0, 0.0f, 1 << 30, 1 << 30, N);
    if constexpr (NORM) {
        // the residual joins in the store phase (coalesced 16-B rows, one more bf16 rounding of the
        // normalised value: bf16(bf16(norm) + res), as the eager bf16 graph x + norm(conv(h)) rounds)
        // (half its loads are issued first, so their latency hides behind the row-sum barrier; all 16
        // would spill)
        u16x8 rv[16];
        load_res_rows<0, 8>(rv, res, lane, wm * 128, n0 + wn * 64, N, row_of);
        conv_rmsnorm_epilogue<1, WMW, WNW>(acc, reinterpret_cast<float*>(smem + G::CSTAGE), wm, wn, lane, row_of, eps,
                                           nw, nb, (const unsigned short*)nullptr);
        EGG_STAMP(4);
        store_tile_rows<0, decltype(row_of), true, true>(acc, smem, wave, lane, wm * 128, n0 + wn * 64, Y, N, row_of,
                                                         res, rv);
    } else {
        EGG_STAMP(4);
        store_tile_rows<ACT, decltype(row_of), false, false, NTAIL>(acc, smem, wave, lane, wm * 128, n0 + wn * 64, Y, N,
                                                                    row_of);
    }
    EGG_STAMP_DRAIN();
    EGG_STAMP(5);
    EGG_STAMP_RT(7);
}

}  // namespace eggroll

using namespace eggroll;

#ifdef EGG_STAMPS
// diagnostic build only: copy the first n stamps of the conv kernels (n <= 131072 * 8) to host memory
extern "C" int eggroll_debug_conv_stamps(unsigned long long* host, int64_t n) {
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_egg_stamps), (size_t)n * 8, 0, hipMemcpyDeviceToHost) == hipSuccess
               ? EGGROLL_OK
               : EGGROLL_ERR_LAUNCH;
}
#endif

// The arguments the conv kernels share, as the entry points got them (the RMSNorm tail's stay null without it).
struct ConvArgs {
    const void *x, *w, *bias;
    int64_t B, H, W, Cin, N;
    void* y;
    float eps = 0.0f;
    const void *nw = nullptr, *nb = nullptr, *res = nullptr;
};

// The halo-staged kernel takes 3x3 px-1 convs whose tiles are all full: H % 16 == 0, W % TWD == 0
// (TWD = 32 for the 512 x 128 tile, 16 for 256 x 256), N % BN == 0: 512 x 128 (N == 128) or 256 x 256
// (N % 256 == 0), one 8-wave workgroup per CU.
static bool halo_ok(int64_t ks, int64_t px, int64_t H, int64_t W, int64_t Cin, int64_t N) {
    if (ks != 3 || px != 1 || H % 16 || 18 * (W + 2) * Cin * 2 >= (1ll << 31)) return false;  // 32-bit halo offsets
    if (N == 128) return W % HC<4>::TWD == 0;
    return N % 256 == 0 && W % HC<2>::TWD == 0;
}

// The wide class: 3x3 px-1 convs at channel counts the rules above refuse (the VAR / Infinity VAE widths 160, 320,
// 640): H % 16 == 0, Cin % 32 == 0 in [32, 2048] (the halo kernel walks Cin in 32-channel slices), N % 32 == 0,
// on the halo kernel with a partial last column tile (NTAIL).  The tile: 512 x 128 needs W % 32 == 0, 256 x 256
// W % 16 == 0; of those W allows, the one with the smaller padded width ceil(N / BN) * BN, a tie to 256 x 256.
// Returns the tile's WMW (4: 512 x 128, 2: 256 x 256), 0 where the shape is outside the class.
static int halo_wide_tile(int64_t ks, int64_t px, int64_t B, int64_t H, int64_t W, int64_t Cin, int64_t N) {
    if (ks != 3 || px != 1 || B <= 0 || H <= 0 || W <= 0 || H % 16 || W % 16) return 0;
    if (Cin < 32 || Cin > 2048 || Cin % 32 || N < 32 || N > 8192 || N % 32) return 0;
    // 32-bit halo and weight offsets, a 31-bit grid (ceil(N / 128) <= 64 column tiles)
    if (18 * (W + 2) * Cin * 2 >= (1ll << 31) || N * 9 * Cin * 2 >= (1ll << 31) || B * H * W >= (1ll << 31)) return 0;
    const int64_t pad4 = (N + 127) / 128 * 128, pad2 = (N + 255) / 256 * 256;
    return W % 32 == 0 && pad4 < pad2 ? 4 : 2;
}

// What conv_nhwc took before the wide class, as far as the channel counts go: those shapes keep their kernel.
static bool conv_classic_channels(int64_t Cin, int64_t N) {
    return N >= 64 && N % 64 == 0 && Cin >= 64 && (Cin & (Cin - 1)) == 0;
}

// The kernel selector of the _sel entry points (`fn` names the one called): 0 the halo kernel where halo_ok
// and the tap-staged one elsewhere, 1 tap-staged, 2 halo (refused where it does not apply).
static int conv_kernel_sel(const char* fn, int32_t kernel, int64_t ks, int64_t px, int64_t H, int64_t W, int64_t Cin,
                           int64_t N, bool* halo) {
    EGG_CHECK_ARG(kernel >= 0 && kernel <= 2, "%s: kernel must be 0 (auto), 1 (tap-staged) or 2 (halo) (got %d)", fn,
                  kernel);
    const bool hok = halo_ok(ks, px, H, W, Cin, N);
    EGG_CHECK_ARG(kernel < 2 || hok, "%s: halo kernel 2 needs ks 3, px 1, H %% 16 == 0 and W, N multiples of the tile "
                  "(see include/eggroll.h)", fn);
    *halo = hok && kernel != 1;
    return EGGROLL_OK;
}

// k_conv3x3_halo over a halo_ok shape.  epi: 0 plain, 1 SiLU, 2 RMSNorm + residual; Epis: the ones the caller has.
// wmw: the tile (4: 512 x 128, 2: 256 x 256); ntail: the last column tile is partial (the wide class only).
template <class Epis, bool NTAIL = false>
static void launch_halo(Epis, int epi, const ConvArgs& a, hipStream_t st, int wmw,
                        std::bool_constant<NTAIL> = std::bool_constant<false>{}) {
    dispatch_int(epi, Epis{}, [&](auto E) {
        dispatch_int(wmw, std::integer_sequence<int, 4, 2>{}, [&](auto WM) {
            constexpr int EPI = decltype(E)::value, WMW = decltype(WM)::value;
            using G = HC<WMW>;
            const int64_t tiles = a.B * (a.H / 16) * (a.W / G::TWD), tn = (a.N + G::BN - 1) / G::BN;
            hipLaunchKernelGGL((k_conv3x3_halo<int(EPI == 1), EPI == 2, WMW, 8 / WMW, NTAIL>),
                               dim3((unsigned)(tiles * tn)), dim3(64 * G::NW), 0, st, (const unsigned short*)a.x,
                               (const unsigned short*)a.w, (const unsigned short*)a.bias, (int)a.H, (int)a.W,
                               (int)a.Cin, (int)a.N, (int)tn, (unsigned short*)a.y, a.eps, (const unsigned short*)a.nw,
                               (const unsigned short*)a.nb, (const unsigned short*)a.res);
        });
    });
}

// What every entry point checks for the tap-staged kernel (`fn` names the one called) over Mp GEMM rows of input
// width W, and the launch geometry that follows.  tall: the 512 x 128 tile, else 256 x 256.
struct Gemm8Geom {
    int lcpt;  // log2 of the 64-channel slices per tap
    int64_t Mp, tiles_n;
    unsigned blocks;
};
static int gemm8_geom(const char* fn, int64_t Mp, int64_t W, int64_t Cin, int64_t N, int64_t ks, int64_t px, bool tall,
                      Gemm8Geom* g) {
    EGG_CHECK_ARG(Cin >= 64 && Cin <= 2048 && (Cin & (Cin - 1)) == 0, "%s: Cin=%lld must be a power of two in [64, 2048]",
                  fn, (long long)Cin);
    const int64_t BM = tall ? 512 : 256, BN = tall ? 128 : 256, K = ks * (px + ks - 1) * Cin;
    EGG_CHECK_ARG(Mp < (1ll << 31) && (BM * (px + 1) + 2 * W + 8) * Cin * 2 < (1ll << 30) && N * K * 2 < (1ll << 31),
                  "%s: sizes exceed the kernel's 32-bit offsets", fn);
    const int64_t tiles_m = (Mp + BM - 1) / BM, tiles_n = (N + BN - 1) / BN;
    EGG_CHECK_ARG(tiles_m * tiles_n < (1ll << 31), "%s: grid too large", fn);
    int lcpt = 0;
    while ((64ll << lcpt) < Cin) ++lcpt;
    *g = Gemm8Geom{lcpt, Mp, tiles_n, (unsigned)(tiles_m * tiles_n)};
    return EGGROLL_OK;
}

// A k_conv3x3_gemm8 instance as one integer for dispatch_int: the decimal digits PX ACT NORM KS WMW SP REP
// (SP 0 with REP 2 is the template's default, the forms without the sub-pixel epilogue).
constexpr int gemm8_id(int px, int act, bool norm, int ks, int wmw, int sp = 0, int rep = 2) {
    return (((((px * 10 + act) * 10 + norm) * 10 + ks) * 10 + wmw) * 10 + sp) * 10 + rep;
}
// ks 2; the 512 x 128 tile; 256 x 256 at px 1; 256 x 256 at px 2 — each plain and SiLU
using ConvIds = std::integer_sequence<int, gemm8_id(1, 0, false, 2, 2), gemm8_id(1, 1, false, 2, 2),
                                      gemm8_id(1, 0, false, 3, 4), gemm8_id(1, 1, false, 3, 4),
                                      gemm8_id(1, 0, false, 3, 2), gemm8_id(1, 1, false, 3, 2),
                                      gemm8_id(2, 0, false, 3, 2), gemm8_id(2, 1, false, 3, 2)>;
using NormIds = std::integer_sequence<int, gemm8_id(1, 0, true, 3, 4), gemm8_id(1, 0, true, 3, 2),
                                      gemm8_id(2, 0, true, 3, 2)>;
// bf16 (SP 1) and fp32 (SP 2) shortcut source at REP 1, 2, 4
using SubpixIds = std::integer_sequence<int, gemm8_id(1, 0, false, 2, 2, 1, 1), gemm8_id(1, 0, false, 2, 2, 1, 2),
                                        gemm8_id(1, 0, false, 2, 2, 1, 4), gemm8_id(1, 0, false, 2, 2, 2, 1),
                                        gemm8_id(1, 0, false, 2, 2, 2, 2), gemm8_id(1, 0, false, 2, 2, 2, 4)>;

template <class Ids>
static void launch_gemm8(Ids, int id, const ConvArgs& a, const Gemm8Geom& g, const SubpixArgs& spa, hipStream_t st) {
    dispatch_int(id, Ids{}, [&](auto ID) {
        constexpr int V = decltype(ID)::value;
        hipLaunchKernelGGL((k_conv3x3_gemm8<V / 1000000, V / 100000 % 10, V / 10000 % 10 != 0, V / 1000 % 10,
                                            V / 100 % 10, V / 10 % 10, V % 10>),
                           dim3(g.blocks), dim3(512), 0, st, (const unsigned short*)a.x, (const unsigned short*)a.w,
                           (const unsigned short*)a.bias, (int)a.H, (int)a.W, (int)a.Cin, g.lcpt, (int)g.Mp, (int)a.N,
                           (int)g.tiles_n, (unsigned short*)a.y, a.eps, (const unsigned short*)a.nw,
                           (const unsigned short*)a.nb, (const unsigned short*)a.res, spa);
    });
}

extern "C" {

/* Implicit-GEMM ks x ks conv, pad 1 (k_conv3x3_gemm8 / k_conv3x3_halo): see include/eggroll.h */
int eggroll_conv_nhwc(const void* x, const void* w_packed, const void* bias, int64_t B, int64_t H, int64_t W,
                      int64_t Cin, int64_t N, int32_t ks, int32_t px, int32_t act, void* y, void* stream) {
    return eggroll_conv_nhwc_sel(x, w_packed, bias, B, H, W, Cin, N, ks, px, act, y, 0, stream);
}

int eggroll_conv_nhwc_sel(const void* x, const void* w_packed, const void* bias, int64_t B, int64_t H, int64_t W,
                          int64_t Cin, int64_t N, int32_t ks, int32_t px, int32_t act, void* y, int32_t kernel,
                          void* stream) {
    EGG_CHECK_ARG(ks == 2 || ks == 3, "conv_nhwc: ks must be 2 or 3 (got %d)", ks);
    EGG_CHECK_ARG(px == 1 || px == 2, "conv_nhwc: px must be 1 or 2 (got %d)", px);
    EGG_CHECK_ARG(ks == 3 || px == 1, "conv_nhwc: px 2 needs ks 3");
    EGG_CHECK_ARG(act == 0 || act == 2, "conv_nhwc: act must be 0 (none) or 2 (silu) (got %d)", act);
    const int64_t Ho = H + 3 - ks, Wo = W + 3 - ks;
    EGG_CHECK_ARG(B > 0 && H > 0 && W > 0 && Wo % px == 0, "conv_nhwc: bad B/H/W (output width %% px == 0 required)");
    // the wide class (halo_wide_tile) is decided first: gemm8_geom's power-of-two Cin is the tap-staged kernel's rule
    if (const int wmw = conv_classic_channels(Cin, N) ? 0 : halo_wide_tile(ks, px, B, H, W, Cin, N)) {
        EGG_CHECK_ARG(kernel == 0 || kernel == 2,
                      "conv_nhwc: Cin=%lld, N=%lld run on the halo kernel only: kernel must be 0 or 2 (got %d)",
                      (long long)Cin, (long long)N, kernel);
        EGG_CHECK_ARG(x && w_packed && y, "conv_nhwc: NULL pointer");
        const ConvArgs a{x, w_packed, bias, B, H, W, Cin, N, y};
        using PlainSilu = std::integer_sequence<int, 0, 1>;
        if (N % (wmw == 4 ? 128 : 256) == 0) launch_halo(PlainSilu{}, act != 0, a, as_stream(stream), wmw);
        else launch_halo(PlainSilu{}, act != 0, a, as_stream(stream), wmw, std::true_type{});
        EGG_CHECK_LAUNCH("conv_nhwc");
        return EGGROLL_OK;
    }
    EGG_CHECK_ARG(N >= 64 && N % 64 == 0 && N <= 8192, "conv_nhwc: N=%lld must be a multiple of 64 (<= 8192), or of 32 "
                  "in the wide class (see include/eggroll.h)", (long long)N);
    // Cout = 128 at px 1 (3x3): the 512 x 128 tile (no zero MACs); everything else 256 x 256
    const bool tall = ks == 3 && px == 1 && N == 128;
    Gemm8Geom g;
    if (int rc = gemm8_geom("conv_nhwc", B * Ho * (Wo / px), W, Cin, N, ks, px, tall, &g)) return rc;
    EGG_CHECK_ARG(x && w_packed && y, "conv_nhwc: NULL pointer");
    bool halo;
    if (int rc = conv_kernel_sel("conv_nhwc", kernel, ks, px, H, W, Cin, N, &halo)) return rc;
    const ConvArgs a{x, w_packed, bias, B, H, W, Cin, N, y};
    const int silu = act != 0;
    if (halo) launch_halo(std::integer_sequence<int, 0, 1>{}, silu, a, as_stream(stream), tall ? 4 : 2);
    else launch_gemm8(ConvIds{}, gemm8_id(px, silu, false, ks, tall ? 4 : 2), a, g, SubpixArgs{}, as_stream(stream));
    EGG_CHECK_LAUNCH("conv_nhwc");
    return EGGROLL_OK;
}

int eggroll_conv2x2_subpixel_nhwc(const void* x, const void* w_packed, const void* bias, const void* src,
                                  int32_t src_f32, int64_t B, int64_t H, int64_t W, int64_t Cin, int64_t Cout,
                                  void* out, void* shadow, void* stream) {
    EGG_CHECK_ARG(B > 0 && H > 0 && W > 0, "conv2x2_subpixel: bad B/H/W");
    Gemm8Geom g;  // the ks-2 phase conv over the (H+1) x (W+1) grid, N = 4 * Cout
    if (int rc = gemm8_geom("conv2x2_subpixel", B * (H + 1) * (W + 1), W, Cin, 4 * Cout, 2, 1, false, &g)) return rc;
    EGG_CHECK_ARG(Cout >= 64 && Cout % 64 == 0 && 4 * Cout <= 8192 && (4 * Cout) % Cin == 0,
                  "conv2x2_subpixel: Cout=%lld must be a multiple of 64 with 4*Cout a multiple of Cin", (long long)Cout);
    const int64_t rep = 4 * Cout / Cin;
    EGG_CHECK_ARG(rep == 1 || rep == 2 || rep == 4, "conv2x2_subpixel: 4*Cout/Cin = %lld unsupported (1, 2, 4)",
                  (long long)rep);
    EGG_CHECK_ARG(src_f32 == 0 || src_f32 == 1, "conv2x2_subpixel: src_f32 must be 0 or 1");
    EGG_CHECK_ARG(src_f32 || !shadow, "conv2x2_subpixel: shadow needs the fp32 form");
    EGG_CHECK_ARG(B * 4 * H * W * Cout < (1ll << 31), "conv2x2_subpixel: sizes exceed the kernel's 32-bit offsets");
    EGG_CHECK_ARG(x && w_packed && src && out, "conv2x2_subpixel: NULL pointer");
    EGG_CHECK_ARG(((uintptr_t)x & 15) == 0 && ((uintptr_t)src & 15) == 0 && ((uintptr_t)out & 15) == 0 &&
                      ((uintptr_t)shadow & 15) == 0 && ((uintptr_t)bias & 15) == 0,
                  "conv2x2_subpixel: pointers must be 16-byte aligned");
    const SubpixArgs spa{(const unsigned short*)bias, src, out, (unsigned short*)shadow, (int)H, (int)W, (int)Cin,
                         (int)Cout};
    const ConvArgs a{x, w_packed, nullptr, B, H, W, Cin, 4 * Cout, nullptr};  // bias and output: the epilogue's (spa)
    launch_gemm8(SubpixIds{}, gemm8_id(1, 0, false, 2, 2, src_f32 ? 2 : 1, (int)rep), a, g, spa, as_stream(stream));
    EGG_CHECK_LAUNCH("conv2x2_subpixel_nhwc");
    return EGGROLL_OK;
}

int eggroll_conv3x3_nhwc(const void* x, const void* w_packed, const void* bias, int64_t B, int64_t H, int64_t W,
                         int64_t Cin, int64_t N, int32_t px, int32_t act, void* y, void* stream) {
    return eggroll_conv_nhwc(x, w_packed, bias, B, H, W, Cin, N, 3, px, act, y, stream);
}

/* ResBlock conv2 + RMSNorm + residual in one launch: see include/eggroll.h */
int eggroll_conv3x3_rmsnorm_nhwc(const void* x, const void* w_packed, const void* bias, int64_t B, int64_t H,
                                 int64_t W, int64_t Cin, int64_t N, int32_t px, float eps, const void* norm_w,
                                 const void* norm_b, const void* res, void* y, void* stream) {
    return eggroll_conv3x3_rmsnorm_nhwc_sel(x, w_packed, bias, B, H, W, Cin, N, px, eps, norm_w, norm_b, res, y, 0,
                                            stream);
}

int eggroll_conv3x3_rmsnorm_nhwc_sel(const void* x, const void* w_packed, const void* bias, int64_t B, int64_t H,
                                     int64_t W, int64_t Cin, int64_t N, int32_t px, float eps, const void* norm_w,
                                     const void* norm_b, const void* res, void* y, int32_t kernel, void* stream) {
    EGG_CHECK_ARG(px == 1 || px == 2, "conv3x3_rmsnorm_nhwc: px must be 1 or 2 (got %d)", px);
    EGG_CHECK_ARG(N == 256 || (N == 128 && px == 1),
                  "conv3x3_rmsnorm_nhwc: N = px * Cout must be 256, or 128 at px 1 (got %lld, px %d)", (long long)N, px);
    const bool tall = N == 128;  // 512 x 128 tile
    EGG_CHECK_ARG(B > 0 && H > 0 && W > 0 && W % px == 0, "conv3x3_rmsnorm_nhwc: bad B/H/W (W %% px == 0 required)");
    Gemm8Geom g;
    if (int rc = gemm8_geom("conv3x3_rmsnorm_nhwc", B * H * (W / px), W, Cin, N, 3, px, tall, &g)) return rc;
    EGG_CHECK_ARG(x && w_packed && y && norm_w && res, "conv3x3_rmsnorm_nhwc: NULL pointer");
    EGG_CHECK_ARG(((uintptr_t)res & 7) == 0, "conv3x3_rmsnorm_nhwc: res must be 8-byte aligned");
    EGG_CHECK_ARG(res != y && x != y, "conv3x3_rmsnorm_nhwc: y may not alias x or res");
    bool halo;
    if (int rc = conv_kernel_sel("conv3x3_rmsnorm_nhwc", kernel, 3, px, H, W, Cin, N, &halo)) return rc;
    const ConvArgs a{x, w_packed, bias, B, H, W, Cin, N, y, eps, norm_w, norm_b, res};
    if (halo) launch_halo(std::integer_sequence<int, 2>{}, 2, a, as_stream(stream), tall ? 4 : 2);
    else launch_gemm8(NormIds{}, gemm8_id(px, 0, true, 3, tall ? 4 : 2), a, g, SubpixArgs{}, as_stream(stream));
    EGG_CHECK_LAUNCH("conv3x3_rmsnorm_nhwc");
    return EGGROLL_OK;
}

}  // extern "C"

