// libeggroll — 8-bit images (gfx950): the way out of the decoder to a PIL "RGB" buffer, and the way of an 8-bit
// image into the reward towers.
//
//   k_images_to_u8_vec<MODE> / k_images_to_u8_gen<MODE> : bf16 decoder images (any strides) -> uint8 [n][H][W][3],
//       clip_u8_of's conversion (clip_image.h).  HBM-bound: 6 bytes read + 3 written per pixel.
//   eggroll_clip_preprocess_u8 : the two passes of eggroll_clip_preprocess on a uint8 source (clip_image.h).
//
// Vector form (rows of contiguous pixels, every row start and the output 16-byte aligned, W % 16 == 0): a lane owns
// 16 consecutive pixels of one row.  It reads them as two 16-byte loads per channel (96 bytes), interleaves the
// three channels in registers and writes the 48 contiguous output bytes as three 16-byte stores; consecutive lanes
// own consecutive 16-pixel groups, so a wave reads 2 KiB runs of each channel and writes one 3 KiB run.  No lane
// touches a pixel outside its row or a byte outside its 48.  Every other layout (a pixel stride, unaligned rows or
// base, W % 16 != 0: 3 W bytes per output row are then no multiple of 16) takes the per-pixel form, one lane per
// output pixel.
#include "clip_image.h"

namespace eggroll {

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
