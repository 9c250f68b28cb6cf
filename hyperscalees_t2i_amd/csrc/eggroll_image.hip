// libeggroll — 8-bit images (gfx950): the way out of the decoder to a PIL "RGB" buffer, and the way of a decoder
// output or an 8-bit image into the reward towers.
//
//   k_images_to_u8_vec<MODE> / k_images_to_u8_gen<MODE> : bf16 decoder images (any strides) -> uint8 [n][H][W][3],
//       clip_u8_of's conversion.  HBM-bound: 6 bytes read + 3 written per pixel.
//   k_clip_resize_h<SRC>, k_clip_resize_v : the two passes of the CLIP preprocessing, eggroll_clip_preprocess on the
//       bf16 decoder output and eggroll_clip_preprocess_u8 on a uint8 source.
//
// Vector form (rows of contiguous pixels, every row start and the output 16-byte aligned, W % 16 == 0): a lane owns
// 16 consecutive pixels of one row.  It reads them as two 16-byte loads per channel (96 bytes), interleaves the
// three channels in registers and writes the 48 contiguous output bytes as three 16-byte stores; consecutive lanes
// own consecutive 16-pixel groups, so a wave reads 2 KiB runs of each channel and writes one 3 KiB run.  No lane
// touches a pixel outside its row or a byte outside its 48.  Every other layout (a pixel stride, unaligned rows or
// base, W % 16 != 0: 3 W bytes per output row are then no multiple of 16) takes the per-pixel form, one lane per
// output pixel.
#include "frag.h"

namespace eggroll {

// ------------------------------------------------------------------------------------
// CLIP image preprocessing, bit-exact with transformers' CLIPImageProcessor (PIL backend) on the
// PIL image the reference would build from the decoder output (rewards.py:86-90, 133-147):
//   u8 = PixArt postprocess (mode 0: rint((x/2 + 0.5).clamp(0,1) * 255), Sana) or the VAR PIL
//        path (mode 1: fp16 ((x+1)*0.5).clamp(0,1) * 255 truncated, models/VAR.py:190, 245-259) or
//        Infinity's (mode 2: bf16 (x+1)/2*255 truncated);
//   Pillow BICUBIC resize in 8-bit fixed point (Resample.c: int32 taps of 22 fractional bits,
//   horizontal pass first, each pass rounded + clipped to 8 bits), center crop, then
//   (u8 / 255 - mean[c]) / std[c] in fp32 (IEEE division, as torch).
// Tap tables (host-built from Pillow's precompute_coeffs): int32 [out][1 + KT] = {first input
// index, KT weights (zero beyond the filter's support)}.  Pass 1 writes the horizontally resized
// rows of the crop's columns as uint8 [n][3][H][OW]; pass 2 the normalised [n][3][OH][OW] fp32.
// ------------------------------------------------------------------------------------
__device__ __forceinline__ int clip_u8_of(float x, int mode) {
    if (mode == 0) {
        float v = fminf(fmaxf(x * 0.5f + 0.5f, 0.0f), 1.0f);
        return (int)rintf(v * 255.0f);
    }
    if (mode == 2) {
        // Infinity (models/Infinity.py img postprocess under bf16 autocast): (x + 1) / 2 * 255, every op
        // rounded to bf16, clamped (the decoder output is in [-1, 1]), .to(uint8) truncates
        auto r = [](float v) { return b2f(f2b(v)); };
        float v = r(r(r(x + 1.0f) * 0.5f) * 255.0f);
        v = fminf(fmaxf(v, 0.0f), 255.0f);
        return (int)v;
    }
    // fp16 arithmetic of the reference's autocast output: every op rounded to half
    _Float16 h = (_Float16)x;
    h = (_Float16)(h + (_Float16)1.0f);
    h = (_Float16)(h * (_Float16)0.5f);
    h = h < (_Float16)0.0f ? (_Float16)0.0f : (h > (_Float16)1.0f ? (_Float16)1.0f : h);
    h = (_Float16)(h * (_Float16)255.0f);
    return (int)(float)h;  // .to(torch.uint8) truncates toward zero
}

__device__ __forceinline__ int pil_clip8(int ss) {
    ss >>= 22;  // arithmetic shift: floor, as Resample.c's clip8
    return ss < 0 ? 0 : (ss > 255 ? 255 : ss);
}

// Pass 1: one block per input row (image n, row y): the row's 3 x W pixels are brought to uint8
// once into LDS (coalesced loads), then the 3 x OW horizontal taps are summed from LDS.
// SRC unsigned short: bf16 decoder output, converted by clip_u8_of(mode); SRC unsigned char: the
// pixels are 8-bit already (mode unused).  Strides are in elements of SRC.
constexpr int CLIP_MAXW = 4096;
template <typename SRC>
__global__ __launch_bounds__(256) void k_clip_resize_h(const SRC* __restrict__ img, int64_t sn, int64_t sc,
                                                       int64_t sh, int64_t sw, int H, int W, int OW, int left,
                                                       int mode, const int* __restrict__ tab, int KT,
                                                       unsigned char* __restrict__ tmp) {
    __shared__ unsigned char row[3 * CLIP_MAXW];
    const int64_t n = blockIdx.x / H;
    const int y = (int)(blockIdx.x - n * H);
    const SRC* src = img + n * sn + (int64_t)y * sh;
    for (int t = threadIdx.x; t < 3 * W; t += 256) {
        const int x = t / 3, c = t - 3 * x;
        if constexpr (std::is_same<SRC, unsigned char>::value)
            row[c * W + x] = src[c * sc + (int64_t)x * sw];
        else
            row[c * W + x] = (unsigned char)clip_u8_of(b2f(src[c * sc + (int64_t)x * sw]), mode);
    }
    __syncthreads();
    for (int o = threadIdx.x; o < 3 * OW; o += 256) {
        const int c = o / OW, xo = o - c * OW;
        const int* t = tab + (int64_t)(left + xo) * (KT + 1);
        const unsigned char* r = row + c * W + t[0];
        int ss = 1 << 21;
        for (int k = 0; k < KT; ++k) ss += (int)r[k] * t[1 + k];
        tmp[((n * 3 + c) * H + y) * OW + xo] = (unsigned char)pil_clip8(ss);
    }
}

// Pass 2: the vertical taps + crop + normalisation of both entry points.
__global__ __launch_bounds__(256) void k_clip_resize_v(const unsigned char* __restrict__ tmp, int H, int OW, int OH,
                                                       int top, const int* __restrict__ tab, int KT, float m0,
                                                       float m1, float m2, float s0, float s1, float s2,
                                                       int64_t total, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int xo = (int)(i % OW);
    int64_t r = i / OW;                    // (n, c, yo)
    const int yo = (int)(r % OH);
    const int64_t nc = r / OH;
    const int c = (int)(nc % 3);
    const int* t = tab + (int64_t)(top + yo) * (KT + 1);
    const int y0 = t[0];
    const unsigned char* col = tmp + nc * H * OW + xo;
    int ss = 1 << 21;
    for (int k = 0; k < KT; ++k) {
        const int w = t[1 + k];
        if (w != 0) ss += (int)col[(int64_t)(y0 + k) * OW] * w;
    }
    const float v = (float)pil_clip8(ss) / 255.0f;
    const float m = c == 0 ? m0 : (c == 1 ? m1 : m2), sd = c == 0 ? s0 : (c == 1 ? s1 : s2);
    out[i] = (v - m) / sd;
}

// The argument checks and the two launches of eggroll_clip_preprocess / eggroll_clip_preprocess_u8 (`what` names
// the entry point in error messages).
template <typename SRC>
static int clip_preprocess_run(const char* what, const SRC* img, int64_t n, int64_t H, int64_t W, int64_t sn,
                               int64_t sc, int64_t sh, int64_t sw, int32_t mode, const int32_t* tab_w,
                               const int32_t* tab_h, int32_t ktw, int32_t kth, int64_t RW, int64_t RH,
                               int64_t out_size, const float* mean, const float* stdv, void* tmp, void* out,
                               void* stream) {
    EGG_CHECK_ARG(n >= 0 && H > 0 && W > 0 && out_size > 0 && RW >= out_size && RH >= out_size, "%s: bad sizes", what);
    if constexpr (!std::is_same<SRC, unsigned char>::value)
        EGG_CHECK_ARG(mode >= 0 && mode <= 2, "%s: mode %d (0 PixArt round, 1 VAR fp16 trunc, 2 Infinity bf16 trunc)", what,
                      mode);
    EGG_CHECK_ARG(ktw > 0 && kth > 0 && ktw <= 64 && kth <= 64, "%s: tap counts out of range", what);
    if (n == 0) return EGGROLL_OK;
    EGG_CHECK_ARG(img && tab_w && tab_h && mean && stdv && tmp && out, "%s: NULL pointer", what);
    const int left = (int)((RW - out_size) / 2), top = (int)((RH - out_size) / 2);
    const int64_t t2 = n * 3 * out_size * out_size;
    EGG_CHECK_ARG((t2 + 255) / 256 < (1ll << 31), "%s: grid too large", what);
    hipStream_t st = as_stream(stream);
    EGG_CHECK_ARG(W <= CLIP_MAXW && n * H < (1ll << 31), "%s: W=%lld > %d or too many rows", what, (long long)W,
                  CLIP_MAXW);
    hipLaunchKernelGGL((k_clip_resize_h<SRC>), dim3((unsigned)(n * H)), dim3(256), 0, st, img, sn, sc, sh, sw, (int)H,
                       (int)W, (int)out_size, left, (int)mode, tab_w, (int)ktw, (unsigned char*)tmp);
    EGG_CHECK_LAUNCH("clip_resize_h");
    float m[3], sd[3];
    // mean / std are host pointers (3 floats each): passed by value to the kernel
    for (int k = 0; k < 3; ++k) { m[k] = mean[k]; sd[k] = stdv[k]; }
    hipLaunchKernelGGL(k_clip_resize_v, dim3((unsigned)((t2 + 255) / 256)), dim3(256), 0, st, (const unsigned char*)tmp,
                       (int)H, (int)out_size, (int)out_size, top, tab_h, (int)kth, m[0], m[1], m[2], sd[0], sd[1], sd[2],
                       t2, (float*)out);
    EGG_CHECK_LAUNCH("clip_resize_v");
    return EGGROLL_OK;
}

constexpr int IU_THREADS = 256;
constexpr int IU_PX = 16;   // pixels per lane of the vector form

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4m;

template <int MODE>
__global__ __launch_bounds__(IU_THREADS) void k_images_to_u8_vec(const unsigned short* __restrict__ img, int64_t sn,
                                                                 int64_t sc, int64_t sh, int H, int W, int64_t units,
                                                                 unsigned char* __restrict__ out) {
    const int64_t u = (int64_t)blockIdx.x * IU_THREADS + threadIdx.x;   // (image, row, 16-pixel group)
    if (u >= units) return;
    const int gpr = W / IU_PX;
    const int64_t row = u / gpr;                                        // image * H + y
    const int x0 = (int)(u - row * gpr) * IU_PX;
    const int64_t i = row / H;
    const int y = (int)(row - i * H);
    const unsigned short* src = img + i * sn + (int64_t)y * sh + x0;
    unsigned char px[3 * IU_PX];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const u16x8m a = *reinterpret_cast<const u16x8m*>(src + c * sc);
        const u16x8m b = *reinterpret_cast<const u16x8m*>(src + c * sc + 8);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            px[3 * k + c] = (unsigned char)clip_u8_of(b2f(a[k]), MODE);
            px[3 * (k + 8) + c] = (unsigned char)clip_u8_of(b2f(b[k]), MODE);
        }
    }
    u32x4m* dst = reinterpret_cast<u32x4m*>(out + (row * W + x0) * 3);
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        u32x4m v;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const unsigned char* p = px + 16 * q + 4 * w;
            v[w] = (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16) | ((unsigned)p[3] << 24);
        }
        dst[q] = v;
    }
}

template <int MODE>
__global__ __launch_bounds__(IU_THREADS) void k_images_to_u8_gen(const unsigned short* __restrict__ img, int64_t sn,
                                                                 int64_t sc, int64_t sh, int64_t sw, int H, int W,
                                                                 int64_t pixels, unsigned char* __restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * IU_THREADS + threadIdx.x;   // (image, row, x): the output pixel
    if (p >= pixels) return;
    const int64_t row = p / W;
    const int x = (int)(p - row * W);
    const int64_t i = row / H;
    const int y = (int)(row - i * H);
    const unsigned short* src = img + i * sn + (int64_t)y * sh + (int64_t)x * sw;
#pragma unroll
    for (int c = 0; c < 3; ++c) out[p * 3 + c] = (unsigned char)clip_u8_of(b2f(src[c * sc]), MODE);
}

template <int MODE>
static void launch_images_to_u8(bool vec, const unsigned short* img, int64_t n, int64_t H, int64_t W, int64_t sn,
                                int64_t sc, int64_t sh, int64_t sw, unsigned char* out, hipStream_t st) {
    if (vec) {
        const int64_t units = n * H * (W / IU_PX);
        hipLaunchKernelGGL((k_images_to_u8_vec<MODE>), dim3((unsigned)((units + IU_THREADS - 1) / IU_THREADS)),
                           dim3(IU_THREADS), 0, st, img, sn, sc, sh, (int)H, (int)W, units, out);
    } else {
        const int64_t pixels = n * H * W;
        hipLaunchKernelGGL((k_images_to_u8_gen<MODE>), dim3((unsigned)((pixels + IU_THREADS - 1) / IU_THREADS)),
                           dim3(IU_THREADS), 0, st, img, sn, sc, sh, sw, (int)H, (int)W, pixels, out);
    }
}

}  // namespace eggroll

using namespace eggroll;

extern "C" int eggroll_images_to_u8(const void* img, int64_t n, int64_t H, int64_t W, int64_t sn, int64_t sc,
                                    int64_t sh, int64_t sw, int32_t mode, void* out, void* stream) {
    EGG_CHECK_ARG(n >= 0 && H > 0 && W > 0 && H < (1ll << 31) && W < (1ll << 31), "images_to_u8: bad sizes");
    EGG_CHECK_ARG(mode >= 0 && mode <= 2, "images_to_u8: mode %d (0 PixArt round, 1 VAR fp16 trunc, 2 Infinity bf16 trunc)",
                  mode);
    if (n == 0) return EGGROLL_OK;
    EGG_CHECK_ARG(img && out, "images_to_u8: NULL pointer");
    // one lane per pixel at most: n * H * W below 2^31 blocks of 256 (H * W < 2^62 cannot overflow)
    EGG_CHECK_ARG(n <= ((1ll << 31) * IU_THREADS - 1) / (H * W), "images_to_u8: grid too large");
    const bool vec = sw == 1 && W % IU_PX == 0 && (sn & 7) == 0 && (sc & 7) == 0 && (sh & 7) == 0 &&
                     ((uintptr_t)img & 15) == 0 && ((uintptr_t)out & 15) == 0;
    const unsigned short* src = (const unsigned short*)img;
    unsigned char* dst = (unsigned char*)out;
    hipStream_t st = as_stream(stream);
    if (mode == 0) launch_images_to_u8<0>(vec, src, n, H, W, sn, sc, sh, sw, dst, st);
    else if (mode == 1) launch_images_to_u8<1>(vec, src, n, H, W, sn, sc, sh, sw, dst, st);
    else launch_images_to_u8<2>(vec, src, n, H, W, sn, sc, sh, sw, dst, st);
    EGG_CHECK_LAUNCH("images_to_u8");
    return EGGROLL_OK;
}

extern "C" int eggroll_clip_preprocess_u8(const void* img, int64_t n, int64_t H, int64_t W, int64_t sn, int64_t sc,
                                          int64_t sh, int64_t sw, const int32_t* tab_w, const int32_t* tab_h,
                                          int32_t ktw, int32_t kth, int64_t RW, int64_t RH, int64_t out_size,
                                          const float* mean, const float* stdv, void* tmp, void* out, void* stream) {
    return clip_preprocess_run("clip_preprocess_u8", (const unsigned char*)img, n, H, W, sn, sc, sh, sw, 0, tab_w, tab_h,
                               ktw, kth, RW, RH, out_size, mean, stdv, tmp, out, stream);
}

extern "C" int eggroll_clip_preprocess(const void* img, int64_t n, int64_t H, int64_t W, int64_t sn, int64_t sc,
                                       int64_t sh, int64_t sw, int32_t mode, const int32_t* tab_w, const int32_t* tab_h,
                                       int32_t ktw, int32_t kth, int64_t RW, int64_t RH, int64_t out_size,
                                       const float* mean, const float* stdv, void* tmp, void* out, void* stream) {
    return clip_preprocess_run("clip_preprocess", (const unsigned short*)img, n, H, W, sn, sc, sh, sw, mode, tab_w, tab_h,
                               ktw, kth, RW, RH, out_size, mean, stdv, tmp, out, stream);
}
