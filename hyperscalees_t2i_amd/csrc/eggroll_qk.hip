// libeggroll — q / k preparation between the qkv projection and the attention kernels of eggroll_attn.hip
// (gfx950), one kernel per model family:
//
//   k_qk_norm_rope      : per-head RMS norm + interleaved-pair RoPE at head dim 128, in place or into a KV
//                         cache slice (Z-Image; with the cache and head scale, Infinity)
//   k_qk_l2norm_kv      : q / k L2 norm, q scale and KV-cache append at head dim 64 (VAR)
//   k_rope_half         : rotate-half RoPE at head dim 256 (Gemma-2)
//   k_qk_norm_rope_half : per-head RMS norm + rotate-half RoPE at head dim 128 (Qwen3)
#include "frag.h"

using namespace eggroll;

// The KV-cache slice an entry point writes (`cached`: it was given one): rows row0 .. row0 + rows_per_seq - 1 of
// each sequence's out_bs values, out_ld apart, C values each.  `fn` names the entry point in the message.
static int kv_cache_args(const char* fn, bool cached, int64_t C, int64_t out_bs, int64_t out_ld, int64_t rows_per_seq,
                         int64_t row0) {
    EGG_CHECK_ARG(!cached || (rows_per_seq > 0 && row0 >= 0 && out_ld >= C && out_ld % 8 == 0 && out_bs % 8 == 0 &&
                              out_bs >= (row0 + rows_per_seq) * out_ld),
                  "%s: bad output geometry", fn);
    return EGGROLL_OK;
}

// ------------------------------------------------------------------------------------
// Per-head RMS norm + rotary position embedding, in place (the Z-Image q / k, head dim 128):
//   y = x * rsqrt(mean_head(x^2) + eps) * w;   (y[2p], y[2p+1]) <- (y0 c - y1 s, y0 s + y1 c)
// with c, s = cos / sin[row % tab_rows][p] (fp32 tables, one row per token position of one member; the
// member copies of a population batch repeat them).  16 lanes per (token, head), 8 consecutive values =
// 4 rotation pairs per lane, fp32 throughout and one bf16 rounding.  Replaces the norm pass and torch's
// fp32 rotation (~10 full passes over q and k per attention).
// ------------------------------------------------------------------------------------
// out == NULL: in place on x.  Otherwise the result goes to out at row (row / rps) * out_bs + (row0 +
// row % rps) * out_ld (a KV cache [seq][ltot][C] slice), and vin (when given) is copied to vout at the same
// row (the values of the same tokens); hscale (optional, fp32 [heads]) multiplies head h's output.
__global__ __launch_bounds__(256) void k_qk_norm_rope(unsigned short* __restrict__ x, int64_t ldx, int heads,
                                                      float eps, const unsigned short* __restrict__ w,
                                                      const float* __restrict__ cosb, const float* __restrict__ sinb,
                                                      int64_t tab_rows, int64_t segs, const float* __restrict__ hscale,
                                                      unsigned short* __restrict__ out, int64_t out_bs, int64_t out_ld,
                                                      int64_t rps, int64_t row0, const unsigned short* __restrict__ vin,
                                                      int64_t ldv, unsigned short* __restrict__ vout) {
    const int64_t seg = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const int l = threadIdx.x & 15;
    const bool live = seg < segs;
    const int64_t row = live ? seg / heads : 0;
    const int h = live ? (int)(seg - row * heads) : 0;
    unsigned short* p = x + row * ldx + h * 128 + l * 8;
    u16x8m v = u16x8m{0, 0, 0, 0, 0, 0, 0, 0};
    if (live) v = *reinterpret_cast<const u16x8m*>(p);
    float f[8], ss = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        f[i] = b2f(v[i]);
        ss += f[i] * f[i];
    }
    ss = seg_sum<16>(ss);   // within the 16-lane segment
    const float r = rsqrtf(ss / 128.f + eps);
    if (!live) return;
    const u16x8m wv = *reinterpret_cast<const u16x8m*>(w + l * 8);
    const int64_t tr = row % tab_rows;
    const float4 c4 = *reinterpret_cast<const float4*>(cosb + tr * 64 + l * 4);
    const float4 s4 = *reinterpret_cast<const float4*>(sinb + tr * 64 + l * 4);
    const float cs[4] = {c4.x, c4.y, c4.z, c4.w}, sn[4] = {s4.x, s4.y, s4.z, s4.w};
    const float hs = hscale ? hscale[h] : 1.0f;
    u16x8m o;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float y0 = f[2 * j] * r * b2f(wv[2 * j]), y1 = f[2 * j + 1] * r * b2f(wv[2 * j + 1]);
        if (hscale) {
            o[2 * j] = f2b(b2f(f2b(y0 * cs[j] - y1 * sn[j])) * hs);
            o[2 * j + 1] = f2b(b2f(f2b(y0 * sn[j] + y1 * cs[j])) * hs);
        } else {
            o[2 * j] = f2b(y0 * cs[j] - y1 * sn[j]);
            o[2 * j + 1] = f2b(y0 * sn[j] + y1 * cs[j]);
        }
    }
    if (!out) {
        *reinterpret_cast<u16x8m*>(p) = o;
        return;
    }
    const int64_t orow = (row / rps) * out_bs + (row0 + row % rps) * out_ld + h * 128 + l * 8;
    *reinterpret_cast<u16x8m*>(out + orow) = o;
    if (vin) *reinterpret_cast<u16x8m*>(vout + orow) = *reinterpret_cast<const u16x8m*>(vin + row * ldv + h * 128 + l * 8);
}

// The body of both entry points (`fn` names the one called in every message); the in-place form has no hscale,
// no out and no value copy, so its cache and copy checks pass by themselves.
static int qk_norm_rope_run(const char* fn, void* x, int64_t ldx, int64_t rows, int32_t heads, int32_t head_dim,
                            float eps, const void* w, const float* cos_tab, const float* sin_tab, int64_t tab_rows,
                            const float* hscale, void* out, int64_t out_bs, int64_t out_ld, int64_t rows_per_seq,
                            int64_t row0, const void* vin, int64_t ldv, void* vout, void* stream) {
    EGG_CHECK_ARG(head_dim == 128, "%s: head_dim must be 128 (got %d)", fn, head_dim);
    EGG_CHECK_ARG(rows >= 0 && heads > 0 && ldx >= (int64_t)heads * 128 && ldx % 8 == 0 && tab_rows > 0,
                  "%s: bad sizes / strides", fn);
    if (int rc = kv_cache_args(fn, out != nullptr, (int64_t)heads * 128, out_bs, out_ld, rows_per_seq, row0)) return rc;
    EGG_CHECK_ARG(!vin || (out && vout && ldv >= (int64_t)heads * 128 && ldv % 8 == 0),
                  "%s: the value copy needs out, vout and ldv", fn);
    EGG_CHECK_ARG(((uintptr_t)x & 15) == 0 && ((uintptr_t)w & 15) == 0 && ((uintptr_t)cos_tab & 15) == 0 &&
                      ((uintptr_t)sin_tab & 15) == 0 && ((uintptr_t)out & 15) == 0 && ((uintptr_t)vin & 15) == 0 &&
                      ((uintptr_t)vout & 15) == 0,
                  "%s: pointers must be 16-byte aligned", fn);
    if (rows == 0) return EGGROLL_OK;
    EGG_CHECK_ARG(x && w && cos_tab && sin_tab, "%s: NULL pointer", fn);
    const int64_t segs = rows * heads;
    EGG_CHECK_ARG(segs < (1ll << 31) / 16, "%s: too many rows", fn);
    hipLaunchKernelGGL(k_qk_norm_rope, dim3((unsigned)((segs * 16 + 255) / 256)), dim3(256), 0, as_stream(stream),
                       (unsigned short*)x, ldx, (int)heads, eps, (const unsigned short*)w, cos_tab, sin_tab, tab_rows,
                       segs, hscale, (unsigned short*)out, out_bs, out_ld, out ? rows_per_seq : 1, row0,
                       (const unsigned short*)vin, ldv, (unsigned short*)vout);
    EGG_CHECK_LAUNCH(fn);
    return EGGROLL_OK;
}

extern "C" int eggroll_qk_norm_rope(void* x, int64_t ldx, int64_t rows, int32_t heads, int32_t head_dim, float eps,
                                    const void* w, const float* cos_tab, const float* sin_tab, int64_t tab_rows,
                                    void* stream) {
    return qk_norm_rope_run("qk_norm_rope", x, ldx, rows, heads, head_dim, eps, w, cos_tab, sin_tab, tab_rows, nullptr,
                            nullptr, 0, 0, 0, 0, nullptr, 0, nullptr, stream);
}

extern "C" int eggroll_qk_norm_rope_kv(void* x, int64_t ldx, int64_t rows, int32_t heads, int32_t head_dim, float eps,
                                       const void* w, const float* cos_tab, const float* sin_tab, int64_t tab_rows,
                                       const float* hscale, void* out, int64_t out_bs, int64_t out_ld,
                                       int64_t rows_per_seq, int64_t row0, const void* vin, int64_t ldv, void* vout,
                                       void* stream) {
    return qk_norm_rope_run("qk_norm_rope_kv", x, ldx, rows, heads, head_dim, eps, w, cos_tab, sin_tab, tab_rows,
                            hscale, out, out_bs, out_ld, rows_per_seq, row0, vin, ldv, vout, stream);
}

// ------------------------------------------------------------------------------------
// q / k L2 normalisation, per-head q scale and KV-cache append at head dim 64 (VAR's attn_l2_norm attention,
// basic_var.py:96-110), on the rows of one fused qkv GEMM output, one launch:
//   q: y = x / max(|x|_2, eps) * qscale[h]   in place (F.normalize(x.float(), dim=-1).mul_(scale): fp32, a true
//                                            division, one bf16 rounding)
//   k: y = x / max(|x|_2, eps)               to kout at (row / rps) * out_bs + (row0 + row % rps) * out_ld + 64 h
//                                            (k_qk_norm_rope's cache addressing), or in place without kout
//   v: copied to vout at the same position.
// 8 lanes per (part, row, head) segment of 64 values, one 16-byte load and store per lane; the segments of the
// parts present follow each other in the grid (`parts`: 2 bits per slot, 0 = q, 1 = k, 2 = v), so q, k and v
// never share a 16-byte chunk or a segment and a block diverges at most at the two part boundaries.
// ------------------------------------------------------------------------------------
__device__ __forceinline__ float seg8_sum(float v) {
    v += dpp_f<0x141>(v);  // row_half_mirror: lane i <-> 7 - i; every quad now holds the four pair sums
    v += dpp_f<0x4E>(v);   // quad_perm [2,3,0,1] = xor 2
    v += dpp_f<0xB1>(v);   // quad_perm [1,0,3,2] = xor 1
    return v;
}

__global__ __launch_bounds__(256) void k_qk_l2norm_kv(unsigned short* __restrict__ q, int64_t ldq,
                                                      unsigned short* __restrict__ k, int64_t ldk,
                                                      const unsigned short* __restrict__ v, int64_t ldv, int heads,
                                                      float eps, const float* __restrict__ qscale, int64_t segs,
                                                      int nparts, int parts, unsigned short* __restrict__ kout,
                                                      unsigned short* __restrict__ vout, int64_t out_bs, int64_t out_ld,
                                                      int64_t rps, int64_t row0) {
    const int64_t gseg = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 3;
    const int l = threadIdx.x & 7;
    const bool live = gseg < segs * nparts;
    const int slot = live ? (int)(gseg / segs) : 0;
    const int part = (parts >> (2 * slot)) & 3;
    const int64_t seg = live ? gseg - slot * segs : 0;
    const int64_t row = seg / heads;
    const int col = (int)(seg - row * heads) * 64 + l * 8;
    unsigned short* src = part == 0 ? q + row * ldq : (part == 1 ? k + row * ldk : const_cast<unsigned short*>(v) + row * ldv);
    u16x8m x = u16x8m{0, 0, 0, 0, 0, 0, 0, 0};
    if (live) x = *reinterpret_cast<const u16x8m*>(src + col);
    float f[8], ss = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        f[i] = b2f(x[i]);
        ss += f[i] * f[i];
    }
    ss = seg8_sum(ss);   // within the 8-lane segment (live or dead as a whole)
    if (!live) return;
    const int64_t orow = (row / rps) * out_bs + (row0 + row % rps) * out_ld + col;
    if (part == 2) {
        *reinterpret_cast<u16x8m*>(vout + orow) = x;
        return;
    }
    const float den = fmaxf(sqrtf(ss), eps);
    const float hs = part == 0 && qscale ? qscale[col >> 6] : 1.0f;
    u16x8m o;
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = f2b(f[i] / den * hs);
    *reinterpret_cast<u16x8m*>(part == 1 && kout ? kout + orow : src + col) = o;
}

extern "C" int eggroll_qk_l2norm_kv(void* q, int64_t ldq, void* k, int64_t ldk, const void* v, int64_t ldv,
                                    int64_t rows, int32_t heads, int32_t head_dim, float eps, const float* qscale,
                                    void* kout, void* vout, int64_t out_bs, int64_t out_ld, int64_t rows_per_seq,
                                    int64_t row0, void* stream) {
    EGG_CHECK_ARG(head_dim == 64, "qk_l2norm_kv: head_dim must be 64 (got %d)", head_dim);
    const int64_t C = (int64_t)heads * 64;
    EGG_CHECK_ARG(rows >= 0 && heads > 0 && eps >= 0.0f && eps < INFINITY, "qk_l2norm_kv: bad sizes / eps");
    EGG_CHECK_ARG((!q || (ldq >= C && ldq % 8 == 0)) && (!k || (ldk >= C && ldk % 8 == 0)) &&
                      (!v || (ldv >= C && ldv % 8 == 0)),
                  "qk_l2norm_kv: bad strides (a multiple of 8, >= heads * 64)");
    EGG_CHECK_ARG((!kout || k) && (!qscale || q) && !v == !vout,
                  "qk_l2norm_kv: kout needs k, qscale needs q, v and vout come together");
    if (int rc = kv_cache_args("qk_l2norm_kv", kout || vout, C, out_bs, out_ld, rows_per_seq, row0)) return rc;
    EGG_CHECK_ARG(((uintptr_t)q & 15) == 0 && ((uintptr_t)k & 15) == 0 && ((uintptr_t)v & 15) == 0 &&
                      ((uintptr_t)kout & 15) == 0 && ((uintptr_t)vout & 15) == 0 && ((uintptr_t)qscale & 3) == 0,
                  "qk_l2norm_kv: q / k / v / kout / vout must be 16-byte aligned, qscale 4-byte aligned");
    int nparts = 0, parts = 0;
    const void* present[3] = {q, k, v};
    for (int p = 0; p < 3; ++p)
        if (present[p]) parts |= p << (2 * nparts++);
    if (rows == 0 || nparts == 0) return EGGROLL_OK;
    const int64_t segs = rows * heads;
    EGG_CHECK_ARG(rows < (1ll << 31) && segs * nparts < (1ll << 31) / 8, "qk_l2norm_kv: too many rows");
    hipLaunchKernelGGL(k_qk_l2norm_kv, dim3((unsigned)((segs * nparts * 8 + 255) / 256)), dim3(256), 0, as_stream(stream),
                       (unsigned short*)q, ldq, (unsigned short*)k, ldk, (const unsigned short*)v, ldv, (int)heads, eps,
                       qscale, segs, nparts, parts, (unsigned short*)kout, (unsigned short*)vout, out_bs, out_ld,
                       (kout || vout) ? rows_per_seq : 1, row0);
    EGG_CHECK_LAUNCH("qk_l2norm_kv");
    return EGGROLL_OK;
}

// ------------------------------------------------------------------------------------
// Rotate-half RoPE at head dim 256, in place on the q and k columns of a fused qkv GEMM output (Gemma-2):
//   x[r, 256 h + d]       = x[d] * cos[p, d] - x[d + 128] * sin[p, d]
//   x[r, 256 h + d + 128] = x[d + 128] * cos[p, d] + x[d] * sin[p, d],   d < 128, p = r % N, h < heads
// cos / sin: fp32 [N, 128] computed on the host (the two halves of transformers' table are equal), so no
// angle moves with GPU rounding.  One thread per (row, head, 8 dims of the lower half); fp32 arithmetic.
// Columns >= 256 heads of a row are not touched.
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_rope_half(unsigned short* __restrict__ x, int64_t ldx, int64_t rows, int N,
                                                   int heads, const float* __restrict__ cs,
                                                   const float* __restrict__ sn) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int c = (int)(t & 15);
    const int64_t rh = t >> 4, r = rh / heads;
    const int h = (int)(rh - r * heads);
    if (r >= rows) return;
    const int p = (int)(r % N);
    unsigned short* px = x + r * ldx + (int64_t)h * 256 + 8 * c;
    const u16x8m lo = *reinterpret_cast<const u16x8m*>(px), hi = *reinterpret_cast<const u16x8m*>(px + 128);
    float co[8], si[8];
    load8f(cs, 1, (int64_t)p * 128 + 8 * c, co);
    load8f(sn, 1, (int64_t)p * 128 + 8 * c, si);
    u16x8m ol, oh;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float a = b2f(lo[i]), bb = b2f(hi[i]);
        ol[i] = f2b(a * co[i] - bb * si[i]);
        oh[i] = f2b(bb * co[i] + a * si[i]);
    }
    *reinterpret_cast<u16x8m*>(px) = ol;
    *reinterpret_cast<u16x8m*>(px + 128) = oh;
}

extern "C" int eggroll_rope_half(void* x, int64_t ldx, int64_t B, int64_t N, int64_t heads, int64_t head_dim,
                                 const float* cos_t, const float* sin_t, void* stream) {
    EGG_CHECK_ARG(head_dim == 256, "rope_half: head_dim %lld unsupported (256)", (long long)head_dim);
    EGG_CHECK_ARG(B >= 0 && heads >= 1, "rope_half: bad sizes B=%lld heads=%lld", (long long)B, (long long)heads);
    if (B == 0) return EGGROLL_OK;
    EGG_CHECK_ARG(N >= 1 && N < (1ll << 31), "rope_half: N=%lld outside [1, 2^31)", (long long)N);
    EGG_CHECK_ARG(ldx % 8 == 0 && ldx >= heads * 256, "rope_half: bad stride");
    EGG_CHECK_ARG(x && cos_t && sin_t, "rope_half: NULL pointer");
    EGG_CHECK_ARG(((uintptr_t)x & 15) == 0 && ((uintptr_t)cos_t & 15) == 0 && ((uintptr_t)sin_t & 15) == 0,
                  "rope_half: x / cos / sin must be 16-byte aligned");
    const int64_t nblk = (B * N * heads * 16 + 255) / 256;
    EGG_CHECK_ARG(nblk < (1ll << 31), "rope_half: grid too large");
    hipLaunchKernelGGL(k_rope_half, dim3((unsigned)nblk), dim3(256), 0, as_stream(stream), (unsigned short*)x, ldx, B * N,
                       (int)N, (int)heads, cos_t, sin_t);
    EGG_CHECK_LAUNCH("rope_half");
    return EGGROLL_OK;
}

// ------------------------------------------------------------------------------------
// Per-head RMS norm, then rotate-half RoPE, head dim 128, in place on the q | k columns of a fused qkv GEMM
// output (Qwen3: q_norm / k_norm over head_dim, applied before the rotation):
//   y = x * rsqrt(mean_128(x^2) + eps) * w[d],   w = wq for heads < heads_q, wk for the next heads_kv
//   x[r, 128 h + d]      = y[d] * cos[p, d] - y[d + 64] * sin[p, d]
//   x[r, 128 h + d + 64] = y[d + 64] * cos[p, d] + y[d] * sin[p, d],   d < 64, p = r % N
// wq / wk fp32 [128]; cos / sin fp32 [N, 64] computed on the host (the two halves of transformers' table are
// equal), so no angle moves with GPU rounding.  8 lanes per (row, head): each holds 8 dims of the lower
// half and the 8 dims 64 above them (16-byte loads and stores), the sum of squares goes round the 8 lanes;
// fp32 arithmetic, one bf16 rounding.  Columns >= 128 (heads_q + heads_kv) of a row are not touched.
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_qk_norm_rope_half(unsigned short* __restrict__ x, int64_t ldx, int64_t rows,
                                                           int N, int heads_q, int heads, float eps,
                                                           const float* __restrict__ wq, const float* __restrict__ wk,
                                                           const float* __restrict__ cs, const float* __restrict__ sn) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int c = (int)(t & 7);
    const int64_t rh = t >> 3, r = rh / heads;
    const int h = (int)(rh - r * heads);
    if (r >= rows) return;   // uniform over the 8 lanes of a (row, head)
    const int p = (int)(r % N);
    unsigned short* px = x + r * ldx + (int64_t)h * 128 + 8 * c;
    const u16x8m lo = *reinterpret_cast<const u16x8m*>(px), hi = *reinterpret_cast<const u16x8m*>(px + 64);
    float a[8], bb[8], ss = 0.0f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        a[i] = b2f(lo[i]);
        bb[i] = b2f(hi[i]);
        ss = fmaf(a[i], a[i], fmaf(bb[i], bb[i], ss));
    }
#pragma unroll
    for (int s = 1; s < 8; s <<= 1) ss += __shfl_xor(ss, s);
    const float rs = 1.0f / sqrtf(ss * (1.0f / 128.0f) + eps);
    const float* w = h < heads_q ? wq : wk;
    float wl[8], wh[8], co[8], si[8];
    load8f(w, 1, 8 * c, wl);
    load8f(w, 1, 64 + 8 * c, wh);
    load8f(cs, 1, (int64_t)p * 64 + 8 * c, co);
    load8f(sn, 1, (int64_t)p * 64 + 8 * c, si);
    u16x8m ol, oh;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float ya = a[i] * rs * wl[i], yb = bb[i] * rs * wh[i];
        ol[i] = f2b(ya * co[i] - yb * si[i]);
        oh[i] = f2b(yb * co[i] + ya * si[i]);
    }
    *reinterpret_cast<u16x8m*>(px) = ol;
    *reinterpret_cast<u16x8m*>(px + 64) = oh;
}

extern "C" int eggroll_qk_norm_rope_half(void* x, int64_t ldx, int64_t B, int64_t N, int64_t heads_q, int64_t heads_kv,
                                         int64_t head_dim, float eps, const float* wq, const float* wk,
                                         const float* cos_t, const float* sin_t, void* stream) {
    EGG_CHECK_ARG(head_dim == 128, "qk_norm_rope_half: head_dim %lld unsupported (128)", (long long)head_dim);
    EGG_CHECK_ARG(B >= 0 && heads_q >= 1 && heads_kv >= 1 && heads_q + heads_kv < (1 << 20),
                  "qk_norm_rope_half: bad sizes B=%lld heads_q=%lld heads_kv=%lld", (long long)B, (long long)heads_q,
                  (long long)heads_kv);
    EGG_CHECK_ARG(eps >= 0.0f && eps < INFINITY, "qk_norm_rope_half: eps must be finite and >= 0");
    if (B == 0) return EGGROLL_OK;
    const int64_t heads = heads_q + heads_kv;
    EGG_CHECK_ARG(N >= 1 && N < (1ll << 31), "qk_norm_rope_half: N=%lld outside [1, 2^31)", (long long)N);
    EGG_CHECK_ARG(ldx % 8 == 0 && ldx >= heads * 128, "qk_norm_rope_half: bad stride");
    EGG_CHECK_ARG(x && wq && wk && cos_t && sin_t, "qk_norm_rope_half: NULL pointer");
    EGG_CHECK_ARG(((uintptr_t)x & 15) == 0 && ((uintptr_t)wq & 15) == 0 && ((uintptr_t)wk & 15) == 0 &&
                  ((uintptr_t)cos_t & 15) == 0 && ((uintptr_t)sin_t & 15) == 0,
                  "qk_norm_rope_half: x / wq / wk / cos / sin must be 16-byte aligned");
    EGG_CHECK_ARG(B < (1ll << 31) && B * N < (1ll << 31), "qk_norm_rope_half: too many rows");
    const int64_t nblk = (B * N * heads * 8 + 255) / 256;
    EGG_CHECK_ARG(nblk < (1ll << 31), "qk_norm_rope_half: grid too large");
    hipLaunchKernelGGL(k_qk_norm_rope_half, dim3((unsigned)nblk), dim3(256), 0, as_stream(stream), (unsigned short*)x,
                       ldx, B * N, (int)N, (int)heads_q, (int)heads, eps, wq, wk, cos_t, sin_t);
    EGG_CHECK_LAUNCH("qk_norm_rope_half");
    return EGGROLL_OK;
}
