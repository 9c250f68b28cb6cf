// libeggroll — channels-last (NHWC) image ops of the Sana FFN and the DC-AE decoder (gfx950).
//
//   k_dwconv_nhwc    : depthwise KSxKS conv (stride 1, zero pad KS/2) with optional SiLU on the input,
//                      per-channel bias and optional GLU gate out[c] = conv[c] * silu(conv[c + C/2]), or the
//                      DC-AE multi-scale branch's grouped 1x1 conv behind it (PW); replaces the GLUMBConv middle
//                      of every Sana FFN and DC-AE EfficientViT block (MIOpen ran it as per-group grouped GEMMs
//                      at ~10% of HBM bandwidth).  LDS-tiled, HBM-bound.
//   k_upshortcut_add, k_subpixel_shortcut, k_subpixel_shortcut4 : the DC-AE up-block's pixel-shuffle shortcut,
//                      fused into the residual add / the sub-pixel conv's interleave
//   k_dcae_head      : the DC-AE decoder head, RMSNorm + ReLU + 3x3 conv to RGB in one kernel
#include "frag.h"

namespace eggroll {

// LDS-tiled depthwise conv, register sliding window.  Block = (image b, band of DW_TH output rows,
// tile of DW_TW output columns, DW_CS channels per plane).  The (TH+KS-1) x (TW+KS-1) input tile of
// each plane (the value plane, and for GLU the gate plane) is staged into LDS once with SiLU applied
// once per element (bf16, as torch's silu output).  Thread = (4-channel group q, column x): it keeps
// its 4 channels' KS*KS fp32 weights in registers and walks the band's rows; for KS = 3 the 3x3 input
// window lives in registers too (one new input row per output row: 3 LDS reads instead of 9).  The
// previous kernel (8-channel threads, weights and every tap re-read from LDS, bf16->fp32 per use)
// ran the Sana FFN shape at 1.4 TB/s, VALU-bound on conversions.
// HBM traffic: input ~(TH+KS-1)/TH (halo rows, mostly L2 hits), output one write.
constexpr int DW_CS = 32;  // channels per plane per block (64 B per pixel: adjacent blocks share lines)
constexpr int DW_TW = 32;  // output columns per block
constexpr int DW_TH = 8;   // output rows per block
constexpr int DW_ORDER_AUTO = 0;  // block order of kernel 0 (eggroll_dwconv_nhwc_sel: 1 = order 0, 2 = order 1)
#ifndef EGG_DW5_DOT2  // 5x5 taps on v_dot2_f32_bf16 (1) or bf16 -> fp32 conversions + fp32 FMAs (0, the default):
// the dot2 form issues 100 instead of ~150 VALU per output row but measured SLOWER — 385 -> 412 us at
// 8 x 128^2 x 1536, 203 -> 222 at 8 x 64^2 x 3072 (profiles/r14b_dw5_dot2_ab.log; numerics within 1 bf16 ulp)
#define EGG_DW5_DOT2 0
#endif

// PW: the DC-AE multi-scale branch's grouped 1x1 conv (groups of DW_CS = 32 channels, the block's
// channel slice) fused behind the depthwise conv: the block's bf16-rounded conv tile [256 px][32 ch]
// goes to LDS and every wave multiplies its 64 pixels by pw[slice] [32 out][32 in] on MFMA (8 x
// 16x16x32), fp32 accumulate, one bf16 rounding — the torch.bmm it replaces rounds the same way.
template <int KS, bool PRE_SILU, bool GLU, bool PW = false>
__global__ __launch_bounds__(256) void k_dwconv_nhwc(const unsigned short* __restrict__ in,
                                                     const unsigned short* __restrict__ wt,   // [KS*KS][Cin]
                                                     const unsigned short* __restrict__ bias, // [Cin] or null
                                                     int H, int W, int Cin, int xtiles, int bands, int cslices,
                                                     unsigned short* __restrict__ out,
                                                     const unsigned short* __restrict__ pw = nullptr, int ord = 0,
                                                     int ldo = 0) {
    static_assert(!PW || (!GLU && DW_CS == 32 && DW_TH * DW_TW == 256), "PW: one 32-channel group per block");
    constexpr int PLANES = GLU ? 2 : 1;
    constexpr int HALO = KS / 2;
    constexpr int TR = DW_TH + KS - 1, TC = DW_TW + KS - 1;
    constexpr int PIXB = DW_CS * 2;  // bytes per staged pixel per plane
    constexpr int IN_BYTES = PLANES * TR * TC * PIXB;
    // PW: the conv tile [256 px][32 ch] bf16 gets its own region, written row by row as the band is
    // computed (no 8 x 4 result registers held to the end: 284 -> ~170 VGPRs, 1 -> 3 waves per SIMD)
    constexpr int PW_BYTES = PW ? DW_TH * DW_TW * 64 : 0;
    __shared__ __attribute__((aligned(16))) char lds[IN_BYTES + PW_BYTES];
    char* const pwt = lds + IN_BYTES;
    auto swz = [](uint32_t L) { return L ^ ((L >> 3) & 32u); };
    const int Cout = GLU ? Cin / 2 : Cin;
    // output row stride: ldo > Cout pads each pixel's row (the last channel slice's blocks zero the
    // <= 32 pad channels), so a following GEMM sees K = ldo, a multiple of its 64-wide k-step
    const int64_t ldo_ = ldo > 0 ? ldo : Cout;
    const int tid = threadIdx.x;
    // Block order on each XCD (xcd_remap: an XCD walks a contiguous range of ids, ~96 blocks in flight).
    // ord 0: channel slice fastest — adjacent slices share 128-B lines, but a band's vertical neighbour
    // (whose rows overlap its halo) is cslices ids away.  ord 1: column sweep — a pair of slices (one
    // 128-B line per pixel), then all bands of the column, then the tile column: both the shared lines
    // and the overlapping halo rows are read within a few neighbouring ids (L2 hits).
    int bid = xcd_remap(blockIdx.x, gridDim.x);
    int cs, xt, band;
    if (ord == 0) {
        cs = bid % cslices;
        bid /= cslices;
        xt = bid % xtiles;
        bid /= xtiles;
        band = bid % bands;
        bid /= bands;
    } else {
        const int cp = (cslices & 1) ? 1 : 2, chi = cslices / cp;
        const int clo = bid % cp;
        bid /= cp;
        band = bid % bands;
        bid /= bands;
        xt = bid % xtiles;
        bid /= xtiles;
        cs = (bid % chi) * cp + clo;
        bid /= chi;
    }
    const int b = bid;
    const int y0 = band * DW_TH, x0 = xt * DW_TW, c0 = cs * DW_CS;
    const char* img = reinterpret_cast<const char*>(in + (int64_t)b * H * W * Cin);
    const uint32_t cin2 = (uint32_t)Cin * 2, rowb = (uint32_t)W * cin2;
    // Stage the 16-byte units [plane][ty][tx][4 chunks] with buffer loads whose addresses cost no VALU
    // work (the address arithmetic of the previous form was ~40% of the kernel's VALU issue, and the
    // kernel is VALU-issue-bound: profiles/r09a_pmc_dwconv.json).  Main columns (tx in [HALO, HALO+32)):
    // thread = (row parity rp, column mc, chunk ch), one image row pair per pass; the row's buffer
    // descriptor (SGPRs: base = the row, size 0 when the row is outside the image) makes the zero padding
    // rows free, and a column past W gets an out-of-range offset (the load returns zeros).  The 2*HALO
    // halo columns: one unit per thread with its own index arithmetic.  Every load of the thread is issued
    // before the first is consumed.
    constexpr uint32_t OOR = 0x80000000u;  // out-of-range buffer offset (images are < 2 GiB: host check)
    const int rp = __builtin_amdgcn_readfirstlane(tid >> 7);  // wave-uniform
    const int mc = (tid >> 2) & 31, ch = tid & 3;
    const uint32_t mvoff = x0 + mc < W ? (uint32_t)(x0 + mc) * cin2 + (uint32_t)(c0 * 2 + ch * 16) : OOR;
    constexpr int MPASS = PLANES * TR / 2;  // TR is even for KS 3 and 5
    static_assert(TR % 2 == 0, "row pairs");
    u16x8m v[MPASS];
#pragma unroll
    for (int p = 0; p < MPASS; ++p) {
        const int pl = (2 * p) / TR, ty = (2 * p) % TR + rp;
        const int gy = y0 + ty - HALO;
        const bool ok = gy >= 0 && gy < H;
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
            (void*)(img + (int64_t)(ok ? gy : 0) * rowb + pl * Cout * 2), (short)0, ok ? (int)rowb : 0, 0x00020000);
        v[p] = __builtin_bit_cast(u16x8m, __builtin_amdgcn_raw_buffer_load_b128(rs, mvoff, 0, 0));
    }
    constexpr int HC = 2 * HALO, HUNITS = PLANES * TR * HC * 4, HPER = (HUNITS + 255) / 256;
    const __amdgpu_buffer_rsrc_t rimg = __builtin_amdgcn_make_buffer_rsrc((void*)img, (short)0, (int)(H * rowb),
                                                                          0x00020000);
    u16x8m hv[HPER];
    uint32_t hlds[HPER];
#pragma unroll
    for (int k = 0; k < HPER; ++k) {
        const int u = tid + k * 256;
        const int hch = u & 3, hcol = (u >> 2) % HC, row = (u >> 2) / HC;
        const int pl = row / TR, ty = row - pl * TR;
        const int tx = hcol < HALO ? hcol : hcol + DW_TW;
        const int gy = y0 + ty - HALO, gx = x0 + tx - HALO;
        const bool ok = u < HUNITS && gy >= 0 && gy < H && gx >= 0 && gx < W;
        const uint32_t off = ok ? (uint32_t)(gy * W + gx) * cin2 + (uint32_t)((pl * Cout + c0) * 2 + hch * 16) : OOR;
        hv[k] = __builtin_bit_cast(u16x8m, __builtin_amdgcn_raw_buffer_load_b128(rimg, off, 0, 0));
        hlds[k] = u < HUNITS ? (uint32_t)(((pl * TR + ty) * TC + tx) * 64 + hch * 16) : 0xffffffffu;
    }
    auto pre = [](u16x8m& x) {
        if (PRE_SILU) {
#pragma unroll
            for (int i = 0; i < 8; ++i) x[i] = f2b(silu(b2f(x[i])));
        }
    };
    const uint32_t mlds = (uint32_t)((rp * TC + HALO + mc) * 64 + ch * 16);
#pragma unroll
    for (int p = 0; p < MPASS; ++p) {
        pre(v[p]);
        *reinterpret_cast<u16x8m*>(lds + mlds + (2 * p) * TC * 64) = v[p];
    }
#pragma unroll
    for (int k = 0; k < HPER; ++k) {
        if (hlds[k] != 0xffffffffu) {
            pre(hv[k]);
            *reinterpret_cast<u16x8m*>(lds + hlds[k]) = hv[k];
        }
    }
    __syncthreads();
    const int q = tid & 7, xs = tid >> 3;  // 4-channel group, column in the tile
    const int x = x0 + xs;
    const int cq = c0 + q * 4;
    auto rd = [&](int pl, int ty, int tx, float (&f)[4]) {
        const u16x4m v = *reinterpret_cast<const u16x4m*>(lds + ((pl * TR + ty) * TC + tx) * PIXB + q * 8);
#pragma unroll
        for (int i = 0; i < 4; ++i) f[i] = b2f(v[i]);
    };
    // output: one buffer descriptor per image (rows past H: offset out of range, store dropped)
    const int64_t obase = (int64_t)b * H * W * ldo_;
    const __amdgpu_buffer_rsrc_t rout = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(out + obase), (short)0, (int)((int64_t)H * W * ldo_ * 2), 0x00020000);
    float res[DW_TH][4];  // value-plane results, gated by the second plane (GLU)
#pragma unroll 1
    for (int pl = 0; pl < PLANES; ++pl) {
        // DOT2 (5x5, EGG_DW5_DOT2): weights kept as bf16 pairs (w, 0) / (0, w) for v_dot2_f32_bf16 against the
        // raw bf16 channel pairs of a tap — no per-tap bf16 -> fp32 conversions (the 5x5 form's VALU bound)
        constexpr bool DOT2 = KS == 5 && EGG_DW5_DOT2;
        float w[DOT2 ? 1 : KS * KS][4], bs[4];
        uint32_t wd[DOT2 ? KS * KS : 1][4];
        const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(
            (void*)(wt + pl * Cout), (short)0, (int)(KS * KS * cin2), 0x00020000);
#pragma unroll
        for (int t = 0; t < KS * KS; ++t) {
            const u16x4m wv = __builtin_bit_cast(u16x4m, __builtin_amdgcn_raw_buffer_load_b64(rw, (uint32_t)cq * 2,
                                                                                            t * (int)cin2, 0));
            if constexpr (DOT2) {
#pragma unroll
                for (int i = 0; i < 4; ++i) wd[t][i] = (i & 1) ? ((uint32_t)wv[i] << 16) : (uint32_t)wv[i];
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) w[t][i] = b2f(wv[i]);
            }
        }
        if (bias) {
            const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc((void*)(bias + pl * Cout), (short)0,
                                                                                (int)cin2, 0x00020000);
            const u16x4m bv = __builtin_bit_cast(u16x4m, __builtin_amdgcn_raw_buffer_load_b64(rb, (uint32_t)cq * 2, 0, 0));
#pragma unroll
            for (int i = 0; i < 4; ++i) bs[i] = b2f(bv[i]);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) bs[i] = 0.0f;
        }
        // one output row's result -> the PW tile in LDS, the GLU value plane, or the output
        auto emit = [&](int oy, const float (&acc)[4]) {
            if constexpr (PW) {
                // conv tile -> LDS [pixel oy*32+x][32 ch], 64-B rows with slot ^= 2*((pixel >> 2) & 1): the
                // 16x16x32 fragment reads (16 consecutive pixels, 4 chunks) are then bank-conflict-free
                u16x4m o;
#pragma unroll
                for (int i = 0; i < 4; ++i) o[i] = f2b(acc[i]);
                *reinterpret_cast<u16x4m*>(pwt + swz((uint32_t)((oy * DW_TW + xs) * 64 + q * 8))) = o;
            } else if (pl == 0 && GLU) {
#pragma unroll
                for (int i = 0; i < 4; ++i) res[oy][i] = acc[i];
            } else {
                const int y = y0 + oy;
                u16x4m o;
#pragma unroll
                for (int i = 0; i < 4; ++i) o[i] = f2b(GLU ? res[oy][i] * silu(acc[i]) : acc[i]);
                const uint32_t px = (uint32_t)(y * W + x) * (uint32_t)ldo_ * 2;
                const bool ok = y < H && x < W;
                __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2m, o), rout,
                                                      ok ? px + (uint32_t)cq * 2 : OOR, 0, 0);
                if (ldo_ > Cout && cs == cslices - 1 && Cout + q * 4 < ldo_)
                    __builtin_amdgcn_raw_buffer_store_b64(u32x2m{0u, 0u}, rout,
                                                          ok ? px + (uint32_t)(Cout + q * 4) * 2 : OOR, 0, 0);
            }
        };
        if constexpr (KS == 3) {
            // the 3x3 input window in registers, sliding down the band: one new input row (3 LDS reads,
            // 12 conversions) per output row instead of 9
            float win[KS][KS][4];
#pragma unroll
            for (int r = 0; r < KS - 1; ++r)
#pragma unroll
                for (int dx = 0; dx < KS; ++dx) rd(pl, r, xs + dx, win[r][dx]);
#pragma unroll
            for (int oy = 0; oy < DW_TH; ++oy) {
#pragma unroll
                for (int dx = 0; dx < KS; ++dx) rd(pl, oy + KS - 1, xs + dx, win[KS - 1][dx]);
                float acc[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i] = bs[i];
#pragma unroll
                for (int dy = 0; dy < KS; ++dy)
#pragma unroll
                    for (int dx = 0; dx < KS; ++dx)
#pragma unroll
                        for (int i = 0; i < 4; ++i) acc[i] += win[dy][dx][i] * w[dy * KS + dx][i];
#pragma unroll
                for (int r = 0; r < KS - 1; ++r)
#pragma unroll
                    for (int dx = 0; dx < KS; ++dx)
#pragma unroll
                        for (int i = 0; i < 4; ++i) win[r][dx][i] = win[r + 1][dx][i];
                emit(oy, acc);
            }
        } else {
            // KS = 5: every tap read from LDS and converted at its use.  A 5x5 fp32 register window
            // measured 11 % slower (2 vs 3 waves per SIMD, profiles/r05e_dw5_register_window_ab.log), and
            // row groups that convert each input row once for 2-4 output rows spill at 3 waves per SIMD
            // next to the 25 taps' fp32 weights (r09 build, 172-500 B of scratch per lane).  Staging the
            // tile as fp32 (one conversion per staged element, 71.7 KB LDS -> 2 blocks per CU) measured
            // 0.90x (366 -> 408 us at 8 x 128^2 x 1536, profiles/r10a_dw5_fp32_tile_ab.log).
#pragma unroll 1
            for (int oy = 0; oy < DW_TH; ++oy) {
                float acc[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i] = bs[i];
#pragma unroll
                for (int dy = 0; dy < KS; ++dy)
#pragma unroll
                    for (int dx = 0; dx < KS; ++dx) {
                        if constexpr (DOT2) {
                            typedef __attribute__((ext_vector_type(2))) __bf16 dw_bf2;
                            const u32x2m v = *reinterpret_cast<const u32x2m*>(
                                lds + ((pl * TR + oy + dy) * TC + xs + dx) * PIXB + q * 8);
                            // (the dwords through a plain array: hipcc miscompiles __builtin_bit_cast of an
                            // ext-vector subscript v[i >> 1] into element 0 for every i)
                            const uint32_t xw[2] = {v.x, v.y};
#pragma unroll
                            for (int i = 0; i < 4; ++i)
                                acc[i] = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(dw_bf2, xw[i >> 1]),
                                                                         __builtin_bit_cast(dw_bf2, wd[dy * KS + dx][i]),
                                                                         acc[i], false);
                        } else {
                            float tap[4];
                            rd(pl, oy + dy, xs + dx, tap);
#pragma unroll
                            for (int i = 0; i < 4; ++i) acc[i] += tap[i] * w[dy * KS + dx][i];
                        }
                    }
                emit(oy, acc);
            }
        }
    }
    if constexpr (PW) {
        __syncthreads();  // the whole conv tile is in pwt
        const int lane = tid & 63, wv = tid >> 6, r16 = lane & 15, g4 = lane >> 4;
        const unsigned short* pg = pw + (int64_t)cs * (DW_CS * DW_CS);  // [o][c] of this channel group
        la_bf16x8 bo[2];
#pragma unroll
        for (int j = 0; j < 2; ++j)
            bo[j] = *reinterpret_cast<const la_bf16x8*>(pg + (16 * j + r16) * DW_CS + 8 * g4);
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            const int p = wv * 64 + 16 * f + r16;  // tile pixel of this lane's fragment row
            const la_bf16x8 a = *reinterpret_cast<const la_bf16x8*>(pwt + swz((uint32_t)(p * 64 + g4 * 16)));
            const int y = y0 + (p >> 5), xx = x0 + (p & 31);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                // transposed product: lane holds pixel p, outputs 16j + 4 g4 .. +3
                const la_f32x4 d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bo[j], a, la_f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
                u16x4m o;
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = f2b(d[e]);
                const uint32_t off = y < H && xx < W ? ((uint32_t)(y * W + xx) * Cout + c0 + 16 * j + 4 * g4) * 2 : OOR;
                __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2m, o), rout, off, 0, 0);
            }
        }
    }
}

// DCUpBlock2d shortcut, NHWC: y[b, 2h+i, 2w+j, c] += x[b, h, w, (4c + 2i + j) / rep]
// (= pixel_shuffle(repeat_interleave(x, rep, channel), 2) without materialising it).
// One thread = one output pixel x 8 channels; 32-bit index math.
__global__ __launch_bounds__(256) void k_upshortcut_add(unsigned short* __restrict__ y, const unsigned short* __restrict__ x,
                                                        int H, int W, int Cin, int Cout, int rep, int pix_total) {
    const int groups = Cout >> 3;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int pix = t / groups;
    if (pix >= pix_total) return;
    const int c0 = (t - pix * groups) << 3;
    const int W2 = 2 * W, HW4 = 4 * H * W;
    const int bb = pix / HW4;
    const int r = pix - bb * HW4;
    const int Y = r / W2, X = r - Y * W2;
    const int k = 2 * (Y & 1) + (X & 1);
    const unsigned short* src = x + ((int64_t)(bb * H + (Y >> 1)) * W + (X >> 1)) * Cin;
    unsigned short* dst = y + (int64_t)pix * Cout + c0;
    u16x8m yv = *reinterpret_cast<const u16x8m*>(dst);
#pragma unroll
    for (int i = 0; i < 8; ++i) yv[i] = f2b(b2f(yv[i]) + b2f(src[(4 * (c0 + i) + k) / rep]));
    *reinterpret_cast<u16x8m*>(dst) = yv;
}

// Sub-pixel up-block output, NHWC: out[b, 2h+i, 2w+j, c] = y4[b, h+i, w+j, (2i+j)*Cout + c]
//                                                      + x[b, h, w, (4c + 2i + j) / rep]
// y4 = conv2d(x, W4, pad 1) with 2x2 phase kernels [B, H+1, W+1, 4*Cout]: equal to
// conv3x3(upsample_nearest_x2(x)) + pixel_shuffle(repeat_interleave(x)) (DCUpBlock2d).
__global__ __launch_bounds__(256) void k_subpixel_shortcut(const unsigned short* __restrict__ y4,
                                                           const unsigned short* __restrict__ x,
                                                           const unsigned short* __restrict__ bias,
                                                           unsigned short* __restrict__ out, int H, int W, int Cin,
                                                           int Cout, int rep, int pix_total) {
    const int groups = Cout >> 3;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int pix = t / groups;
    if (pix >= pix_total) return;
    const int c0 = (t - pix * groups) << 3;
    const int W2 = 2 * W, HW4 = 4 * H * W;
    const int bb = pix / HW4;
    const int r = pix - bb * HW4;
    const int Y = r / W2, X = r - Y * W2;
    const int i = Y & 1, j = X & 1, h = Y >> 1, w = X >> 1;
    const int k = 2 * i + j;
    const unsigned short* src = x + ((int64_t)(bb * H + h) * W + w) * Cin;
    const u16x8m yv = *reinterpret_cast<const u16x8m*>(
        y4 + ((int64_t)(bb * (H + 1) + h + i) * (W + 1) + (w + j)) * (4 * Cout) + k * Cout + c0);
    u16x8m o;
#pragma unroll
    for (int q = 0; q < 8; ++q)
        o[q] = f2b(b2f(yv[q]) + (bias ? b2f(bias[c0 + q]) : 0.f) + b2f(src[(4 * (c0 + q) + k) / rep]));
    *reinterpret_cast<u16x8m*>(out + (int64_t)pix * Cout + c0) = o;
}

// Same output, one thread per LOW-resolution pixel (b, h, w) and 8 output channels c0..c0+7, all four
// phases (i, j): the shortcut source channels (4c + 2i + j) / REP of all phases lie in one
// 32/REP-channel window of x[b, h, w] starting at 4 c0 / REP, loaded as 16-byte vectors and indexed
// with compile-time positions (the per-output kernel above gathers them as 8 scalar 2-byte loads
// per output chunk).  REP = 4 Cout / Cin in {1, 2, 4}.
// F32: the DC-AE fp32 residual stream — x (the shortcut source) and out are fp32, and `shadow`
// (optional) receives bf16(out); the same arithmetic on the fp32 shortcut values.
template <int REP, bool F32 = false>
__global__ __launch_bounds__(256) void k_subpixel_shortcut4(const unsigned short* __restrict__ y4,
                                                            const void* __restrict__ x,
                                                            const unsigned short* __restrict__ bias,
                                                            void* __restrict__ out, int H, int W, int Cin,
                                                            int Cout, int lowpix_total,
                                                            unsigned short* __restrict__ shadow = nullptr) {
    constexpr int XW = 32 / REP;  // source window (channels)
    const int groups = Cout >> 3;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int lp = t / groups;
    if (lp >= lowpix_total) return;
    const int c0 = (t - lp * groups) << 3;
    const int HW = H * W;
    const int bb = lp / HW;
    const int r = lp - bb * HW;
    const int h = r / W, w = r - h * W;
    float xs[XW];
#pragma unroll
    for (int v = 0; v < XW / 8; ++v) {
        float q[8];
        load8f(x, F32, (int64_t)lp * Cin + 4 * c0 / REP + 8 * v, q);
#pragma unroll
        for (int e = 0; e < 8; ++e) xs[8 * v + e] = q[e];
    }
    float bv[8];
    if (bias) {
        const u16x8m q = *reinterpret_cast<const u16x8m*>(bias + c0);
#pragma unroll
        for (int e = 0; e < 8; ++e) bv[e] = b2f(q[e]);
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) bv[e] = 0.f;
    }
    u16x8m yv[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = k >> 1, j = k & 1;
        yv[k] = *reinterpret_cast<const u16x8m*>(
            y4 + ((int64_t)(bb * (H + 1) + h + i) * (W + 1) + (w + j)) * (4 * Cout) + k * Cout + c0);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = k >> 1, j = k & 1;
        const int64_t opix = ((int64_t)(bb * 2 * H + 2 * h + i) * (2 * W) + 2 * w + j) * Cout + c0;
        float f[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) f[q] = b2f(yv[k][q]) + bv[q] + xs[(4 * q + k) / REP];
        if constexpr (F32) {
            float* o32 = reinterpret_cast<float*>(out) + opix;
            *reinterpret_cast<float4*>(o32) = float4{f[0], f[1], f[2], f[3]};
            *reinterpret_cast<float4*>(o32 + 4) = float4{f[4], f[5], f[6], f[7]};
        }
        if (!F32 || shadow) {
            u16x8m o;
#pragma unroll
            for (int q = 0; q < 8; ++q) o[q] = f2b(f[q]);
            *reinterpret_cast<u16x8m*>((F32 ? shadow : reinterpret_cast<unsigned short*>(out)) + opix) = o;
        }
    }
}

// ------------------------------------------------------------------------------------
// DC-AE decoder head, fused: y[p, o] = cb[o] + sum_{tap, c} a[p + tap, c] * Wc[o, tap, c]  (3x3, pad 1)
// with a = bf16(relu(rms_norm(x) * w + b)) (norm_out + ReLU + conv_out of the reference decoder).
// The unfused pair was a rownorm pass over x plus MIOpen's 128 -> 3 channel conv, which ran at 16 TF
// (3.6 ms per 8-image decode, reading 2 GB at 0.6 TB/s).  Block = 8 x 16 output pixels: the
// 10 x 18-pixel halo tile of x is loaded with every 16-B load in flight, RMS-normalised per pixel
// (16-lane shuffle reduction over 128 channels), written to LDS as bf16; then 36 MFMA k-steps
// (9 taps x 4 x 32 channels) of 16 pixels x 16 outputs (3 real) per output row.  HBM: x read once
// (+halo L2 hits), y written once — the conv is ~free on MFMA.  Round 4: a block walks EGG_HEAD_TPB
// bands down its tile column with the next band's loads in flight under the current band's conv:
// 1217 -> 1014 us at 8 x 1024^2 x 128, bitwise equal (profiles/r07i_dcae_head_band_walk_ab.jsonl).
// ------------------------------------------------------------------------------------
constexpr int HD_C = 128;                // input channels (the decoder's widths[0])
#ifndef EGG_HEAD_TPB
#define EGG_HEAD_TPB 8                   // output bands walked per block (A/B knob; 1 = the round-2 form)
#endif
constexpr int HD_TH = 8, HD_TW = 16;     // output tile
constexpr int HD_TR = HD_TH + 2, HD_TC = HD_TW + 2;
constexpr int HD_PSTR = HD_C * 2;        // LDS bytes per staged pixel: 16-B chunk c of pixel p sits at slot
                                         // c ^ (p & 15) (conflict-free b128 reads of 16 pixels, no padding:
                                         // 53 KB per block -> 3 blocks per CU instead of 2)
__device__ __forceinline__ int hd_slot(int pix, int c) { return pix * HD_PSTR + ((c ^ (pix & 15)) << 4); }

typedef __attribute__((ext_vector_type(8))) __bf16 hd_bf16x8;
typedef __attribute__((ext_vector_type(4))) float hd_f32x4;

__global__ __launch_bounds__(256, 3) void k_dcae_head(const unsigned short* __restrict__ x, int H, int W, float eps,
                                                   const unsigned short* __restrict__ nw,
                                                   const unsigned short* __restrict__ nb,
                                                   const unsigned short* __restrict__ wc,   // [3][3][3][C]
                                                   const unsigned short* __restrict__ cb,   // [3] or null
                                                   int xtiles, int bands, int tpb, unsigned short* __restrict__ y) {
    __shared__ __attribute__((aligned(16))) char tile[HD_TR * HD_TC * HD_PSTR];
    __shared__ __attribute__((aligned(16))) unsigned short wl[3 * 9 * HD_C];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // XCD-contiguous tile ranges: horizontally adjacent tiles (sharing 2 halo columns) on one L2.  A block
    // walks tpb bands down its tile column; the next band's halo loads are issued as soon as the current
    // band's raw values have been normalised into LDS, so they are in flight during its conv and stores
    // (the one-band form waited a full memory latency per tile with only 3 blocks per CU to cover it)
    const int bgroups = (bands + tpb - 1) / tpb;
    int bid = xcd_remap(blockIdx.x, gridDim.x);
    const int xt = bid % xtiles;
    bid /= xtiles;
    const int bg = bid % bgroups;
    const int b = bid / bgroups;
    const int band_lo = bg * tpb, band_hi = min(bands, band_lo + tpb);
    const int x0 = xt * HD_TW;
    const char* img = reinterpret_cast<const char*>(x + (int64_t)b * H * W * HD_C);
    const uint32_t rowb = (uint32_t)W * HD_PSTR;
    // conv weights -> LDS (6.75 KiB), once per block
    for (int u = tid; u < 3 * 9 * HD_C / 8; u += 256)
        *reinterpret_cast<u16x8m*>(wl + u * 8) = *reinterpret_cast<const u16x8m*>(wc + u * 8);
    // Halo tile staging with buffer descriptors (round 5; the per-unit pixel division and 64-bit address
    // arithmetic of the previous form made this kernel VALU-issue-bound, profiles/r09d_epoch_census.txt).
    // Thread = (main column mc, 16-B chunk ch): the 16 main columns (tx 1..16) of every halo row, one row
    // descriptor per row (size 0 outside the image: zero rows), a column past W an out-of-range offset;
    // the 2 halo columns (tx 0, 17) x 10 rows x 16 chunks = 320 units take one or two indexed loads.  A
    // pixel's 16 chunks stay 16 consecutive lanes (its sum of squares is a 16-lane shuffle reduction).
    constexpr uint32_t OOR = 0x80000000u;
    const int ch = tid & 15, mc = tid >> 4;
    const bool mcol_ok = x0 + mc < W;
    const uint32_t mvoff = mcol_ok ? (uint32_t)(x0 + mc) * HD_PSTR + ch * 16 : OOR;
    constexpr int HU = HD_TR * 2 * 16, HPER = (HU + 255) / 256;   // 320 halo-column units
    u16x8m v[HD_TR], hv[HPER];
    bool hok[HPER];
    const __amdgpu_buffer_rsrc_t rimg = __builtin_amdgcn_make_buffer_rsrc((void*)img, (short)0, (int)(H * rowb),
                                                                          0x00020000);
    // halo-column unit k of rows rlo..HD_TR-1: row rlo + (hp >> 1), column 0 or 17
    auto hunit = [&](int k, int rlo, int& ty, int& tx) {
        const int u = tid + k * 256, hp = u >> 4;
        ty = rlo + (hp >> 1);
        tx = (hp & 1) ? HD_TC - 1 : 0;
        return u < (HD_TR - rlo) * 32;
    };
    // rows rlo..HD_TR-1 of the halo tile whose first row is image row y0 - 1 (rlo = 0: a block's first
    // band; 2: a later band, whose rows 0, 1 are the previous band's rows 8, 9, already in LDS)
    auto load = [&](int y0, int rlo) {
#pragma unroll
        for (int r = 0; r < HD_TR; ++r) {
            if (r < rlo) continue;
            const int gy = y0 + r - 1;
            const bool ok = gy >= 0 && gy < H;
            const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
                (void*)(img + (int64_t)(ok ? gy : 0) * rowb), (short)0, ok ? (int)rowb : 0, 0x00020000);
            v[r] = __builtin_bit_cast(u16x8m, __builtin_amdgcn_raw_buffer_load_b128(rs, mvoff, 0, 0));
        }
#pragma unroll
        for (int k = 0; k < HPER; ++k) {
            int ty, tx;
            const bool in = hunit(k, rlo, ty, tx);
            const int gy = y0 + ty - 1, gx = x0 + tx - 1;
            hok[k] = in && gy >= 0 && gy < H && gx >= 0 && gx < W;
            const uint32_t off = hok[k] ? (uint32_t)(gy * W + gx) * HD_PSTR + ch * 16 : OOR;
            hv[k] = __builtin_bit_cast(u16x8m, __builtin_amdgcn_raw_buffer_load_b128(rimg, off, 0, 0));
        }
    };
    float wv[8], bv[8];
    {
        const u16x8m qw = *reinterpret_cast<const u16x8m*>(nw + ch * 8);
        const u16x8m qb = *reinterpret_cast<const u16x8m*>(nb + ch * 8);
#pragma unroll
        for (int i = 0; i < 8; ++i) { wv[i] = b2f(qw[i]); bv[i] = b2f(qb[i]); }
    }
    // RMS-normalise one 16-B unit (8 channels of one pixel), affine, ReLU, bf16; zero where the halo pixel
    // is outside the image.  (f * rstd) * w + b per value as before: the packed pairs round each product
    // and sum exactly like the scalar ops, so the tile is bitwise unchanged.
    typedef __attribute__((ext_vector_type(2))) float f2;
    auto norm = [&](const u16x8m& q, bool ok) {
        float f[8], ss = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) { f[i] = b2f(q[i]); ss += f[i] * f[i]; }
        ss = seg_sum<16>(ss);
        const float rstd = __builtin_amdgcn_rsqf(ss / HD_C + eps);  // >= eps: never denormal
        u16x8m o8 = {0, 0, 0, 0, 0, 0, 0, 0};
        if (ok) {
#pragma unroll
            for (int i = 0; i < 8; i += 2) {
                f2 t = f2{f[i], f[i + 1]} * f2{rstd, rstd};
                t = t * f2{wv[i], wv[i + 1]};
                t = t + f2{bv[i], bv[i + 1]};
                o8[i] = f2b(t.x > 0.f ? t.x : 0.f);
                o8[i + 1] = f2b(t.y > 0.f ? t.y : 0.f);
            }
        }
        return o8;
    };
    const int n = lane & 15, g = lane >> 4;
    const float bias = (n < 3 && cb) ? b2f(cb[n]) : 0.f;
    // B operand column n = output channel n; columns 3..15 are computed and never stored, so their lanes
    // read a real channel's weights (no zero row, no branch: 52.9 KB of LDS, 3 blocks per CU)
    const int wrow = (n % 3) * 9 * HD_C + g * 8;
    // Rolling rows: tile row r of the j-th band a block walks sits in LDS row slot (8j + r) mod 10, so the
    // two rows a band shares with the next (its rows 8, 9 = the next band's rows 0, 1) are loaded and
    // normalised once (10 -> 8 rows per band after the first).
    auto slot = [](int j8, int r) { const int q = j8 + r; return q >= HD_TR ? q - HD_TR : q; };
    load(band_lo * HD_TH, 0);
    int j8 = 0;  // 8j mod 10
#pragma unroll 1
    for (int band = band_lo; band < band_hi; ++band) {
        const int y0 = band * HD_TH;
        const int rlo = band > band_lo ? 2 : 0;
        if (band > band_lo) __syncthreads();  // every wave's conv reads of the previous band are done
#pragma unroll
        for (int r = 0; r < HD_TR; ++r) {
            if (r < rlo) continue;
            const int gy = y0 + r - 1;
            const u16x8m o8 = norm(v[r], mcol_ok && gy >= 0 && gy < H);
            *reinterpret_cast<u16x8m*>(tile + hd_slot(slot(j8, r) * HD_TC + 1 + mc, ch)) = o8;
        }
#pragma unroll
        for (int k = 0; k < HPER; ++k) {
            int ty, tx;
            const bool in = hunit(k, rlo, ty, tx);
            const u16x8m o8 = norm(hv[k], hok[k]);
            if (in) *reinterpret_cast<u16x8m*>(tile + hd_slot(slot(j8, ty) * HD_TC + tx, ch)) = o8;
        }
        if (band + 1 < band_hi) load(y0 + HD_TH, 2);
        // conv A-fragment addresses: hd_slot(pix, cq*4 + g) = hd_slot(pix, g) ^ (cq << 6) (the chunk's low
        // two bits are g, cq only flips bits 2..3 of the slot): one base per (output row, tap), a XOR per k-step
        uint32_t abase[2][9];
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int tap = 0; tap < 9; ++tap)
                abase[r][tap] = (uint32_t)hd_slot(slot(j8, wave * 2 + r + tap / 3) * HD_TC + n + tap % 3, g);
        __syncthreads();
        // conv: wave w computes output rows 2w, 2w+1 (one 16-pixel M-tile each)
        hd_f32x4 acc[2] = {hd_f32x4{0.f, 0.f, 0.f, 0.f}, hd_f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int s = 0; s < 36; ++s) {
            const int tap = s >> 2, cq = s & 3;
            const hd_bf16x8 bf = *reinterpret_cast<const hd_bf16x8*>(wl + wrow + tap * HD_C + cq * 32);
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const hd_bf16x8 af = *reinterpret_cast<const hd_bf16x8*>(tile + (abase[r][tap] ^ (uint32_t)(cq << 6)));
                acc[r] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bf, acc[r], 0, 0, 0);
            }
        }
        // C[m = pixel 4g + e][col = output channel n]
        if (n < 3) {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int yy = y0 + wave * 2 + r;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int xx = x0 + 4 * g + e;
                    if (yy < H && xx < W) y[(((int64_t)b * H + yy) * W + xx) * 3 + n] = f2b(acc[r][e] + bias);
                }
            }
        }
        j8 = slot(j8, HD_TH);
    }
}

}  // namespace eggroll

using namespace eggroll;

// block order (kernel argument `ord`, see k_dwconv_nhwc) for the automatic choice
static int dw_order(int kernel) { return kernel == 0 ? DW_ORDER_AUTO : kernel - 1; }

// The launch of both dwconv entry points.  PW (the grouped 1x1 behind the conv: pw given, no SiLU, no GLU)
// instantiates KS 3 / 5 only, the plain form every KS x PRE_SILU x GLU.
template <bool PW>
static void dw_launch(int ks, bool pre_silu, bool glu, int64_t nblk, hipStream_t st, const void* in, const void* w_t,
                      const void* bias, int64_t H, int64_t W, int64_t C, int64_t xtiles, int64_t bands, int64_t cslices,
                      void* out, const void* pw, int kernel, int64_t ldo) {
    dispatch_int(ks, std::integer_sequence<int, 3, 5>{}, [&](auto KS) {
        dispatch_int(pre_silu, Flag01{}, [&](auto PS) {
            dispatch_int(glu, Flag01{}, [&](auto GL) {
                if constexpr (!PW || (!decltype(PS)::value && !decltype(GL)::value))
                    hipLaunchKernelGGL((k_dwconv_nhwc<decltype(KS)::value, decltype(PS)::value, decltype(GL)::value, PW>),
                                       dim3((unsigned)nblk), dim3(256), 0, st, (const unsigned short*)in,
                                       (const unsigned short*)w_t, (const unsigned short*)bias, (int)H, (int)W, (int)C,
                                       (int)xtiles, (int)bands, (int)cslices, (unsigned short*)out,
                                       (const unsigned short*)pw, dw_order(kernel), (int)ldo);
            });
        });
    });
}

extern "C" int eggroll_dwconv_nhwc(const void* in, const void* w_t, const void* bias, int64_t B, int64_t H, int64_t W,
                                   int64_t C, int32_t ks, int32_t pre_silu, int32_t glu, void* out, void* stream) {
    return eggroll_dwconv_nhwc_sel(in, w_t, bias, B, H, W, C, ks, pre_silu, glu, out, 0, stream);
}

extern "C" int eggroll_dwconv_nhwc_sel(const void* in, const void* w_t, const void* bias, int64_t B, int64_t H,
                                       int64_t W, int64_t C, int32_t ks, int32_t pre_silu, int32_t glu, void* out,
                                       int32_t kernel, void* stream) {
    return eggroll_dwconv_nhwc_ex(in, w_t, bias, B, H, W, C, ks, pre_silu, glu, out, glu ? C / 2 : C, kernel, stream);
}

extern "C" int eggroll_dwconv_nhwc_ex(const void* in, const void* w_t, const void* bias, int64_t B, int64_t H,
                                      int64_t W, int64_t C, int32_t ks, int32_t pre_silu, int32_t glu, void* out,
                                      int64_t ldo, int32_t kernel, void* stream) {
    EGG_CHECK_ARG(kernel >= 0 && kernel <= 2, "dwconv: kernel must be 0 (auto), 1 (channel-fastest) or 2 (column "
                  "sweep) (got %d)", kernel);
    EGG_CHECK_ARG(B >= 0 && H > 0 && W > 0 && C > 0, "dwconv: bad sizes");
    const int64_t cout = glu ? C / 2 : C;
    EGG_CHECK_ARG((!glu || C % 2 == 0) && cout % DW_CS == 0, "dwconv: output channels must be a multiple of %d", DW_CS);
    EGG_CHECK_ARG(ldo >= cout && ldo - cout <= DW_CS && ldo % 8 == 0,
                  "dwconv: output row stride %lld must be in [%lld, %lld] and a multiple of 8", (long long)ldo,
                  (long long)cout, (long long)(cout + DW_CS));
    EGG_CHECK_ARG(ks == 3 || ks == 5, "dwconv: ks=%d unsupported (3, 5)", ks);
    EGG_CHECK_ARG(((uintptr_t)in & 15) == 0 && ((uintptr_t)w_t & 15) == 0 && ((uintptr_t)out & 15) == 0,
                  "dwconv: pointers must be 16-byte aligned");
    EGG_CHECK_ARG(H * W * C < (1ll << 30) && H * W * ldo < (1ll << 30), "dwconv: image too large (< 2 GiB per image)");
    if (B == 0) return EGGROLL_OK;
    EGG_CHECK_ARG(in && w_t && out, "dwconv: NULL pointer");
    const int64_t bands = (H + DW_TH - 1) / DW_TH, xtiles = (W + DW_TW - 1) / DW_TW, cslices = cout / DW_CS;
    const int64_t nblk = B * bands * xtiles * cslices;
    EGG_CHECK_ARG(nblk < (1ll << 31), "dwconv: grid too large");
    dw_launch<false>(ks, pre_silu != 0, glu != 0, nblk, as_stream(stream), in, w_t, bias, H, W, C, xtiles, bands, cslices,
                     out, nullptr, kernel, ldo);
    EGG_CHECK_LAUNCH("dwconv_nhwc");
    return EGGROLL_OK;
}

extern "C" int eggroll_dwconv_pw_nhwc(const void* in, const void* w_t, const void* pw, int64_t B, int64_t H, int64_t W,
                                      int64_t C, int32_t ks, void* out, void* stream) {
    return eggroll_dwconv_pw_nhwc_sel(in, w_t, pw, B, H, W, C, ks, out, 0, stream);
}

extern "C" int eggroll_dwconv_pw_nhwc_sel(const void* in, const void* w_t, const void* pw, int64_t B, int64_t H,
                                          int64_t W, int64_t C, int32_t ks, void* out, int32_t kernel, void* stream) {
    EGG_CHECK_ARG(kernel >= 0 && kernel <= 2, "dwconv_pw: kernel must be 0 (auto), 1 or 2 (got %d)", kernel);
    EGG_CHECK_ARG(B >= 0 && H > 0 && W > 0 && C > 0 && C % DW_CS == 0, "dwconv_pw: C must be a multiple of %d", DW_CS);
    EGG_CHECK_ARG(ks == 3 || ks == 5, "dwconv_pw: ks=%d unsupported (3, 5)", ks);
    EGG_CHECK_ARG(((uintptr_t)in & 15) == 0 && ((uintptr_t)w_t & 15) == 0 && ((uintptr_t)out & 15) == 0 &&
                      ((uintptr_t)pw & 15) == 0,
                  "dwconv_pw: pointers must be 16-byte aligned");
    EGG_CHECK_ARG(H * W * C < (1ll << 30), "dwconv_pw: image too large (< 2 GiB per image)");
    if (B == 0) return EGGROLL_OK;
    EGG_CHECK_ARG(in && w_t && pw && out && out != in, "dwconv_pw: NULL or aliased pointer");
    const int64_t bands = (H + DW_TH - 1) / DW_TH, xtiles = (W + DW_TW - 1) / DW_TW, cslices = C / DW_CS;
    const int64_t nblk = B * bands * xtiles * cslices;
    EGG_CHECK_ARG(nblk < (1ll << 31), "dwconv_pw: grid too large");
    dw_launch<true>(ks, false, false, nblk, as_stream(stream), in, w_t, nullptr, H, W, C, xtiles, bands, cslices, out, pw,
                    kernel, 0);  // (ldo 0: rows of C channels)
    EGG_CHECK_LAUNCH("dwconv_pw_nhwc");
    return EGGROLL_OK;
}

extern "C" int eggroll_upshortcut_add(void* y, const void* x, int64_t B, int64_t H, int64_t W, int64_t Cin,
                                      int64_t Cout, void* stream) {
    EGG_CHECK_ARG(B >= 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0 && (4 * Cout) % Cin == 0 && Cout % 8 == 0,
                  "upshortcut: bad sizes");
    EGG_CHECK_ARG(B * 4 * H * W * Cout < (1ll << 31) && B * H * W * Cin < (1ll << 31), "upshortcut: tensor too large");
    if (B == 0) return EGGROLL_OK;
    EGG_CHECK_ARG(x && y, "upshortcut: NULL pointer");
    const int64_t pix = B * 4 * H * W;
    const int64_t threads = pix * (Cout / 8);
    hipLaunchKernelGGL(k_upshortcut_add, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, as_stream(stream),
                       (unsigned short*)y, (const unsigned short*)x, (int)H, (int)W, (int)Cin, (int)Cout,
                       (int)(4 * Cout / Cin), (int)pix);
    EGG_CHECK_LAUNCH("upshortcut_add");
    return EGGROLL_OK;
}

// k_subpixel_shortcut4 for rep = 4 Cout / Cin in {1, 2, 4}: one thread per low-resolution pixel and 8 channels
template <bool F32>
static void sp4_launch(int64_t rep, const void* y4, const void* x, const void* bias, void* out, void* shadow, int64_t B,
                       int64_t H, int64_t W, int64_t Cin, int64_t Cout, void* stream) {
    const int64_t lowpix = B * H * W;
    const dim3 grid((unsigned)((lowpix * (Cout / 8) + 255) / 256));
    dispatch_int((int)rep, std::integer_sequence<int, 1, 2, 4>{}, [&](auto RP) {
        hipLaunchKernelGGL((k_subpixel_shortcut4<decltype(RP)::value, F32>), grid, dim3(256), 0, as_stream(stream),
                           (const unsigned short*)y4, x, (const unsigned short*)bias, out, (int)H, (int)W, (int)Cin,
                           (int)Cout, (int)lowpix, (unsigned short*)shadow);
    });
}

extern "C" int eggroll_subpixel_shortcut(const void* y4, const void* x, const void* bias, void* out, int64_t B,
                                         int64_t H, int64_t W, int64_t Cin, int64_t Cout, void* stream) {
    EGG_CHECK_ARG(B >= 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0 && (4 * Cout) % Cin == 0 && Cout % 8 == 0,
                  "subpixel_shortcut: bad sizes");
    EGG_CHECK_ARG(B * 4 * H * W * Cout < (1ll << 31) && B * (H + 1) * (W + 1) * 4 * Cout < (1ll << 31),
                  "subpixel_shortcut: tensor too large");
    if (B == 0) return EGGROLL_OK;
    EGG_CHECK_ARG(y4 && x && out, "subpixel_shortcut: NULL pointer");
    EGG_CHECK_ARG(((uintptr_t)bias & 15) == 0, "subpixel_shortcut: bias must be 16-byte aligned");
    const int64_t rep = 4 * Cout / Cin;
    if ((rep == 1 || rep == 2 || rep == 4) && Cin % 8 == 0) {
        sp4_launch<false>(rep, y4, x, bias, out, nullptr, B, H, W, Cin, Cout, stream);
        EGG_CHECK_LAUNCH("subpixel_shortcut");
        return EGGROLL_OK;
    }
    const int64_t pix = B * 4 * H * W;
    const int64_t threads = pix * (Cout / 8);
    hipLaunchKernelGGL(k_subpixel_shortcut, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, as_stream(stream),
                       (const unsigned short*)y4, (const unsigned short*)x, (const unsigned short*)bias,
                       (unsigned short*)out, (int)H, (int)W, (int)Cin, (int)Cout, (int)rep, (int)pix);
    EGG_CHECK_LAUNCH("subpixel_shortcut");
    return EGGROLL_OK;
}

extern "C" int eggroll_subpixel_shortcut_f32(const void* y4, const float* x, const void* bias, float* out,
                                             void* shadow, int64_t B, int64_t H, int64_t W, int64_t Cin, int64_t Cout,
                                             void* stream) {
    const int64_t rep = Cin > 0 ? 4 * Cout / Cin : 0;
    EGG_CHECK_ARG(B >= 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0 && (4 * Cout) % Cin == 0 && Cout % 8 == 0 &&
                      (rep == 1 || rep == 2 || rep == 4) && Cin % 8 == 0,
                  "subpixel_shortcut_f32: bad sizes (4 Cout / Cin in {1, 2, 4})");
    EGG_CHECK_ARG(B * 4 * H * W * Cout < (1ll << 31) && B * (H + 1) * (W + 1) * 4 * Cout < (1ll << 31),
                  "subpixel_shortcut_f32: tensor too large");
    if (B == 0) return EGGROLL_OK;
    EGG_CHECK_ARG(y4 && x && out, "subpixel_shortcut_f32: NULL pointer");
    EGG_CHECK_ARG(((uintptr_t)bias & 15) == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)out & 15) == 0 &&
                      ((uintptr_t)shadow & 15) == 0,
                  "subpixel_shortcut_f32: pointers must be 16-byte aligned");
    sp4_launch<true>(rep, y4, x, bias, out, shadow, B, H, W, Cin, Cout, stream);
    EGG_CHECK_LAUNCH("subpixel_shortcut_f32");
    return EGGROLL_OK;
}

extern "C" int eggroll_dcae_head(const void* x, int64_t B, int64_t H, int64_t W, int64_t C, float eps,
                                 const void* norm_w, const void* norm_b, const void* conv_w, const void* conv_b,
                                 void* y, void* stream) {
    EGG_CHECK_ARG(B >= 0 && H > 0 && W > 0, "dcae_head: bad sizes");
    EGG_CHECK_ARG(C == HD_C, "dcae_head: C=%lld unsupported (%d)", (long long)C, HD_C);
    EGG_CHECK_ARG(H * W * C < (1ll << 30), "dcae_head: image too large (< 2 GiB per image: 32-bit buffer offsets)");
    if (B == 0) return EGGROLL_OK;
    EGG_CHECK_ARG(x && norm_w && norm_b && conv_w && y, "dcae_head: NULL pointer");
    EGG_CHECK_ARG(((uintptr_t)x & 15) == 0 && ((uintptr_t)norm_w & 15) == 0 && ((uintptr_t)norm_b & 15) == 0 &&
                  ((uintptr_t)conv_w & 15) == 0, "dcae_head: pointers must be 16-byte aligned");
    const int64_t bands = (H + HD_TH - 1) / HD_TH, xtiles = (W + HD_TW - 1) / HD_TW;
    // bands per block: enough blocks to fill 256 CUs x 3 many times over, the rest walked in-block
    const int64_t tpb = EGG_HEAD_TPB;
    const int64_t nblk = B * ((bands + tpb - 1) / tpb) * xtiles;
    EGG_CHECK_ARG(nblk < (1ll << 31), "dcae_head: grid too large");
    hipLaunchKernelGGL(k_dcae_head, dim3((unsigned)nblk), dim3(256), 0, as_stream(stream), (const unsigned short*)x,
                       (int)H, (int)W, eps, (const unsigned short*)norm_w, (const unsigned short*)norm_b,
                       (const unsigned short*)conv_w, (const unsigned short*)conv_b, (int)xtiles, (int)bands, (int)tpb,
                       (unsigned short*)y);
    EGG_CHECK_LAUNCH("dcae_head");
    return EGGROLL_OK;
}
