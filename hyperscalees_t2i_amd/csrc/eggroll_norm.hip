// libeggroll — normalisations and residual-stream updates over [rows, C] / NHWC activations (gfx950).
//
//   k_rownorm           : RMS / Layer norm + affine / AdaLN modulation + act + residual, one pass (Sana blocks,
//                         DC-AE RMSNorm)
//   k_resid_layernorm   : fp32 residual add + LayerNorm of the CLIP reward towers
//   k_gn_stats / _finalize / _apply : GroupNorm (+ SiLU), the FLUX / Infinity VAE decoders
//   k_gated_residual, k_gated_residual_f32 : x += gate[image] * y on the bf16 / fp32 residual stream
//   k_bias_act          : conv bias + activation in place
//   k_scm_step          : the SCM / trigflow sampler step between two Sana forwards
#include "frag.h"

namespace eggroll {

// ------------------------------------------------------------------------------------
// Fused row normalisation over the channel (last) dim of a [rows, C] bf16 tensor:
//   y = norm(x)                      RMS (x / sqrt(mean x^2 + eps)) or LayerNorm (centred)
//   y = y * w[c] (opt) * (1 + mscale[g, c]) (opt) + mshift[g, c] (opt) + b[c] (opt)
//   y = act(y)  (none / relu / silu);   y += res[r, c] (opt)
// g = row / rows_per_group (AdaLN: one modulation vector per image).  SEG lanes per row
// (16/32/64), up to NCH 16-byte chunks per lane, fp32 statistics.
// Covers DC-AE RMSNorm(+bias)(+residual)(+ReLU), Sana q/k/caption RMSNorm, and the Sana AdaLN
// "layer_norm(x) * (1 + scale) + shift" of every block and of norm_out.
// ------------------------------------------------------------------------------------
// XF: x is fp32 (the fp32 residual stream of the Sana blocks); mf32: the modulation
// vectors mscale / mshift are fp32 (the fp32 AdaLN modulation); rf32: res is fp32.  OF: the output
// is fp32 (the DC-AE fp32 residual stream: out = res + norm(x) in place of res) and `shadow` (optional)
// receives its bf16 copy; else the output is bf16 (a GEMM operand).
template <int SEG, int NCH, bool XF, bool OF>
__global__ __launch_bounds__(256) void k_rownorm(const void* __restrict__ x, int64_t rows, int C, float eps,
                                                 int layer, const unsigned short* __restrict__ w,
                                                 const unsigned short* __restrict__ b,
                                                 const void* __restrict__ mscale,
                                                 const void* __restrict__ mshift, int64_t mstride, int mf32,
                                                 int64_t rows_per_group, int act,
                                                 const void* __restrict__ res, int rf32,
                                                 void* __restrict__ out, unsigned short* __restrict__ shadow) {
    const int lane = threadIdx.x & 63;
    const int seg_lane = lane % SEG;
    const int64_t row = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / SEG;
    const bool live = row < rows;
    const int nchunks = C / 8;
    const int64_t xoff = (live ? row : 0) * C;
    float v[NCH][8];
    float s1 = 0.f;
#pragma unroll
    for (int t = 0; t < NCH; ++t) {
        const int ci = seg_lane + t * SEG;
        if (live && ci < nchunks) {
            load8f(x, XF, xoff + ci * 8, v[t]);
#pragma unroll
            for (int i = 0; i < 8; ++i) s1 += v[t][i];
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) v[t][i] = 0.f;
        }
    }
    s1 = seg_sum<SEG>(s1);
    const float mean = layer ? s1 / C : 0.f;
    float s2 = 0.f;
#pragma unroll
    for (int t = 0; t < NCH; ++t) {
        const int ci = seg_lane + t * SEG;
        if (ci < nchunks)
#pragma unroll
            for (int i = 0; i < 8; ++i) { const float d = v[t][i] - mean; s2 += d * d; }
    }
    s2 = seg_sum<SEG>(s2);
    const float rstd = rsqrtf(s2 / C + eps);
    if (!live) return;
    const int64_t g = row / rows_per_group;
#pragma unroll
    for (int t = 0; t < NCH; ++t) {
        const int ci = seg_lane + t * SEG;
        if (ci >= nchunks) continue;
        const int c0 = ci * 8;
        float y[8], q[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) y[i] = (v[t][i] - mean) * rstd;
        if (w) {
            load8f(w, 0, c0, q);
#pragma unroll
            for (int i = 0; i < 8; ++i) y[i] *= q[i];
        }
        if (mscale) {
            load8f(mscale, mf32, g * mstride + c0, q);
#pragma unroll
            for (int i = 0; i < 8; ++i) y[i] *= 1.0f + q[i];
        }
        if (mshift) {
            load8f(mshift, mf32, g * mstride + c0, q);
#pragma unroll
            for (int i = 0; i < 8; ++i) y[i] += q[i];
        }
        if (b) {
            load8f(b, 0, c0, q);
#pragma unroll
            for (int i = 0; i < 8; ++i) y[i] += q[i];
        }
        if (act == 1) {
#pragma unroll
            for (int i = 0; i < 8; ++i) y[i] = y[i] > 0.f ? y[i] : 0.f;
        } else if (act == 2) {
#pragma unroll
            for (int i = 0; i < 8; ++i) y[i] = silu(y[i]);
        }
        if (res) {
            load8f(res, rf32, row * C + c0, q);
#pragma unroll
            for (int i = 0; i < 8; ++i) y[i] += q[i];
        }
        if constexpr (OF) {
            float* o32 = reinterpret_cast<float*>(out) + row * C + c0;
            *reinterpret_cast<float4*>(o32) = float4{y[0], y[1], y[2], y[3]};
            *reinterpret_cast<float4*>(o32 + 4) = float4{y[4], y[5], y[6], y[7]};
        }
        if (!OF || shadow) {
            u16x8m o;
#pragma unroll
            for (int i = 0; i < 8; ++i) o[i] = f2b(y[i]);
            *reinterpret_cast<u16x8m*>((OF ? shadow : reinterpret_cast<unsigned short*>(out)) + row * C + c0) = o;
        }
    }
}

// ------------------------------------------------------------------------------------
// fp32 residual stream + LayerNorm of the CLIP reward towers (clip_tower.py, fp32_residual):
//   h[r] += float(y[r])           (y bf16, optional: the block output just computed by a GEMM)
//   out[r] = bf16(LN(h[r]) * w + b) with fp32 statistics (mean, then the centred second moment)
// One 64-lane wave per row (h held in registers between the passes), 8 channels per lane-chunk.
// Replaces, per residual point, torch's bf16->fp32 copy, fp32 add, fp32 layer_norm and the bf16
// cast of its output (four passes over the row, three of them over the fp32 stream).
// ------------------------------------------------------------------------------------
template <int NCH>
__global__ __launch_bounds__(256) void k_resid_layernorm(float* __restrict__ h, int64_t ldh,
                                                         const unsigned short* __restrict__ y, int64_t ldy,
                                                         int64_t rows, int C, float eps,
                                                         const unsigned short* __restrict__ w,
                                                         const unsigned short* __restrict__ b,
                                                         unsigned short* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t row = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (row >= rows) return;  // whole waves: a row is one wave
    const int nchunks = C >> 3;
    float* hr = h + row * ldh;
    const unsigned short* yr = y ? y + row * ldy : nullptr;
    float v[NCH][8];
    float s1 = 0.f;
#pragma unroll
    for (int t = 0; t < NCH; ++t) {
        const int ci = lane + t * 64;
#pragma unroll
        for (int i = 0; i < 8; ++i) v[t][i] = 0.f;
        if (ci < nchunks) {
            const float4 a0 = *reinterpret_cast<const float4*>(hr + ci * 8);
            const float4 a1 = *reinterpret_cast<const float4*>(hr + ci * 8 + 4);
            v[t][0] = a0.x; v[t][1] = a0.y; v[t][2] = a0.z; v[t][3] = a0.w;
            v[t][4] = a1.x; v[t][5] = a1.y; v[t][6] = a1.z; v[t][7] = a1.w;
            if (yr) {
                const u16x8m q = *reinterpret_cast<const u16x8m*>(yr + ci * 8);
#pragma unroll
                for (int i = 0; i < 8; ++i) v[t][i] += b2f(q[i]);
                *reinterpret_cast<float4*>(hr + ci * 8) = float4{v[t][0], v[t][1], v[t][2], v[t][3]};
                *reinterpret_cast<float4*>(hr + ci * 8 + 4) = float4{v[t][4], v[t][5], v[t][6], v[t][7]};
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) s1 += v[t][i];
        }
    }
    s1 = seg_sum<64>(s1);
    const float mean = s1 / C;
    float s2 = 0.f;
#pragma unroll
    for (int t = 0; t < NCH; ++t) {
        if (lane + t * 64 < nchunks)
#pragma unroll
            for (int i = 0; i < 8; ++i) { const float d = v[t][i] - mean; s2 += d * d; }
    }
    s2 = seg_sum<64>(s2);
    const float rstd = rsqrtf(s2 / C + eps);
#pragma unroll
    for (int t = 0; t < NCH; ++t) {
        const int ci = lane + t * 64;
        if (ci >= nchunks) continue;
        const u16x8m qw = *reinterpret_cast<const u16x8m*>(w + ci * 8);
        const u16x8m qb = *reinterpret_cast<const u16x8m*>(b + ci * 8);
        u16x8m o;
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] = f2b((v[t][i] - mean) * rstd * b2f(qw[i]) + b2f(qb[i]));
        *reinterpret_cast<u16x8m*>(out + row * C + ci * 8) = o;
    }
}

// x[r, c] += gate[g, c] * y[r, c]   (bf16, in place; g = r / rows_per_group)
__global__ __launch_bounds__(256) void k_gated_residual(unsigned short* __restrict__ x, const unsigned short* __restrict__ y,
                                                        const unsigned short* __restrict__ gate, int64_t gstride,
                                                        int64_t rows_per_group, int C, int64_t total_chunks) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total_chunks) return;
    const int nch = C / 8;
    const int64_t row = i / nch;
    const int c0 = (int)(i - row * nch) * 8;
    const u16x8m xv = *reinterpret_cast<const u16x8m*>(x + row * C + c0);
    const u16x8m yv = *reinterpret_cast<const u16x8m*>(y + row * C + c0);
    const u16x8m gv = *reinterpret_cast<const u16x8m*>(gate + (row / rows_per_group) * gstride + c0);
    u16x8m o;
#pragma unroll
    for (int k = 0; k < 8; ++k) o[k] = f2b(b2f(xv[k]) + b2f(gv[k]) * b2f(yv[k]));
    *reinterpret_cast<u16x8m*>(x + row * C + c0) = o;
}

// fp32 residual stream update (Sana blocks):  x[r, c] = fma(gate[g, c], y[r, c], x[r, c])
// (x fp32 in place, y bf16, gate bf16 or fp32 (g32) or NULL = 1: x += y), optionally also writing the
// bf16 shadow copy of x that the next GEMM reads.  The same expression as the fused GEMM epilogues
// EPI_RES32 / EPI_GATED32 of p8_epilogue.h, so fused == unfused bit for bit.
__global__ __launch_bounds__(256) void k_gated_residual_f32(float* __restrict__ x, const unsigned short* __restrict__ y,
                                                            const void* __restrict__ gate, int g32, int64_t gstride,
                                                            int64_t rows_per_group, int C, int64_t total_chunks,
                                                            unsigned short* __restrict__ shadow) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total_chunks) return;
    const int nch = C / 8;
    const int64_t row = i / nch;
    const int c0 = (int)(i - row * nch) * 8;
    float xv[8], yv[8], gv[8];
    load8f(x, 1, row * C + c0, xv);
    load8f(y, 0, row * C + c0, yv);
    if (gate) {
        load8f(gate, g32, (row / rows_per_group) * gstride + c0, gv);
#pragma unroll
        for (int k = 0; k < 8; ++k) xv[k] = __builtin_fmaf(gv[k], yv[k], xv[k]);
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) xv[k] = xv[k] + yv[k];
    }
    *reinterpret_cast<float4*>(x + row * C + c0) = float4{xv[0], xv[1], xv[2], xv[3]};
    *reinterpret_cast<float4*>(x + row * C + c0 + 4) = float4{xv[4], xv[5], xv[6], xv[7]};
    if (shadow) {
        u16x8m o;
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = f2b(xv[k]);
        *reinterpret_cast<u16x8m*>(shadow + row * C + c0) = o;
    }
}

// One SCM / trigflow sampler step between two transformer forwards (or before the decoder), see
// eggroll_scm_step in include/eggroll.h.  Member = blockIdx.y; thread i of a member handles the
// 4-element chunk i (128-bit loads and stores; nvec chunks, 0 when a pointer or the member length
// rules them out) or, past the chunks, one element of the scalar tail.  RD: 0 none, 1 fp16, 2 bf16.
// x_next may alias x: every element is read and written by the same thread.
struct ScmScalars {
    float in_scale, coef_m, coef_eps, cos_t, sin_t, cos_n, sin_n_sd, in_scale_next, out_scale;
};

template <int RD>
__device__ __forceinline__ float scm_rnd(float v) {
    if (RD == 1) return (float)(_Float16)v;
    if (RD == 2) return b2f(f2b(v));
    return v;
}

template <int RD>
__device__ __forceinline__ void scm_elem(const ScmScalars& s, float x, float e, float nz, float& x_next, float& m_next,
                                         float& x0_out) {
    const float m = scm_rnd<RD>(x * s.in_scale);
    const float pred = __builtin_fmaf(s.coef_m, m, s.coef_eps * scm_rnd<RD>(e));
    const float x0 = __builtin_fmaf(s.cos_t, x, -(s.sin_t * pred));
    x_next = __builtin_fmaf(s.cos_n, x0, s.sin_n_sd * nz);
    m_next = scm_rnd<RD>(x_next * s.in_scale_next);
    x0_out = x0 * s.out_scale;
}

template <int RD, int E32>
__global__ __launch_bounds__(256) void k_scm_step(const float* x, int64_t x_member_stride, const void* __restrict__ eps,
                                                  const float* __restrict__ noise, int64_t n, int64_t nvec,
                                                  ScmScalars s, float* x_next, float* __restrict__ m_next,
                                                  float* __restrict__ x0_out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t k = blockIdx.y;
    const float* xm = x + k * x_member_stride;
    const int64_t mo = k * n;  // this member's offset into eps and the outputs
    if (i < nvec) {
        const int64_t o = i * 4;
        const float4 xv = *reinterpret_cast<const float4*>(xm + o);
        float ev[4], nv[4] = {0.f, 0.f, 0.f, 0.f};
        if (E32) {
            const float4 q = *reinterpret_cast<const float4*>((const float*)eps + mo + o);
            ev[0] = q.x, ev[1] = q.y, ev[2] = q.z, ev[3] = q.w;
        } else {
            const u16x4m q = *reinterpret_cast<const u16x4m*>((const unsigned short*)eps + mo + o);
#pragma unroll
            for (int j = 0; j < 4; ++j) ev[j] = b2f(q[j]);
        }
        if (noise) {
            const float4 q = *reinterpret_cast<const float4*>(noise + o);
            nv[0] = q.x, nv[1] = q.y, nv[2] = q.z, nv[3] = q.w;
        }
        const float xs[4] = {xv.x, xv.y, xv.z, xv.w};
        float xn[4], mn[4], xo[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) scm_elem<RD>(s, xs[j], ev[j], nv[j], xn[j], mn[j], xo[j]);
        if (x_next) *reinterpret_cast<float4*>(x_next + mo + o) = float4{xn[0], xn[1], xn[2], xn[3]};
        if (m_next) *reinterpret_cast<float4*>(m_next + mo + o) = float4{mn[0], mn[1], mn[2], mn[3]};
        if (x0_out) *reinterpret_cast<float4*>(x0_out + mo + o) = float4{xo[0], xo[1], xo[2], xo[3]};
        return;
    }
    const int64_t o = nvec * 4 + (i - nvec);
    if (o >= n) return;
    const float e = E32 ? ((const float*)eps)[mo + o] : b2f(((const unsigned short*)eps)[mo + o]);
    float xn, mn, xo;
    scm_elem<RD>(s, xm[o], e, noise ? noise[o] : 0.f, xn, mn, xo);
    if (x_next) x_next[mo + o] = xn;
    if (m_next) m_next[mo + o] = mn;
    if (x0_out) x0_out[mo + o] = xo;
}

// y = act(bf16(y + bias[c])) in place (conv bias folded into the activation pass; torch's conv2d
// with bias on MIOpen runs the bias as its own add_ pass).  act: 0 none, 1 relu, 2 silu.
__global__ __launch_bounds__(256) void k_bias_act(unsigned short* __restrict__ y, const unsigned short* __restrict__ bias,
                                                  unsigned nch, int act, unsigned total_chunks) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total_chunks) return;
    const unsigned c0 = (i % nch) * 8;
    u16x8m yv = *reinterpret_cast<const u16x8m*>(y + (size_t)i * 8);
    const u16x8m bv = *reinterpret_cast<const u16x8m*>(bias + c0);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        float v = b2f(f2b(b2f(yv[k]) + b2f(bv[k])));
        if (act == 1) v = v > 0.f ? v : 0.f;
        else if (act == 2) v = v / (1.0f + __expf(-v));
        yv[k] = f2b(v);
    }
    *reinterpret_cast<u16x8m*>(y + (size_t)i * 8) = yv;
}

}  // namespace eggroll

using namespace eggroll;

template <int SEG, int NCH>
static void launch_rownorm(const void* x, int xf32, int64_t rows, int C, float eps, int layer, const void* w,
                           const void* b, const void* ms, const void* mh, int64_t mstride, int mf32, int64_t rpg,
                           int act, const void* res, int rf32, void* out, int of32, void* shadow, hipStream_t st) {
    const int64_t threads = rows * SEG;
    const dim3 grid((unsigned)((threads + 255) / 256));
    // instances: fp32 x (1), else fp32 out (2), else bf16 both (0)
    dispatch_int(xf32 ? 1 : of32 ? 2 : 0, std::integer_sequence<int, 0, 1, 2>{}, [&](auto V) {
        constexpr int v = decltype(V)::value;
        hipLaunchKernelGGL((k_rownorm<SEG, NCH, v == 1, v == 2>), grid, dim3(256), 0, st, x, rows, C, eps, layer,
                           (const unsigned short*)w, (const unsigned short*)b, ms, mh, mstride, mf32, rpg, act, res,
                           rf32, out, (unsigned short*)shadow);
    });
}

extern "C" int eggroll_rownorm_ex(const void* x, int32_t x_f32, int64_t rows, int64_t C, float eps, int32_t layer,
                                  const void* w, const void* b, const void* mscale, const void* mshift,
                                  int64_t mstride, int32_t mod_f32, int64_t rows_per_group, int32_t act,
                                  const void* res, int32_t res_f32, void* out, int32_t out_f32, void* shadow,
                                  void* stream) {
    EGG_CHECK_ARG(rows >= 0 && C > 0 && C % 8 == 0 && C <= 8 * 64 * 8, "rownorm: need C %% 8 == 0, C <= 4096");
    EGG_CHECK_ARG(act >= 0 && act <= 2 && rows_per_group > 0, "rownorm: bad act / rows_per_group");
    EGG_CHECK_ARG(((uintptr_t)x & 15) == 0 && ((uintptr_t)out & 15) == 0 && (!res || ((uintptr_t)res & 15) == 0) &&
                      (!mscale || ((uintptr_t)mscale & 15) == 0) && (!mshift || ((uintptr_t)mshift & 15) == 0) &&
                      ((uintptr_t)shadow & 15) == 0,
                  "rownorm: pointers must be 16-byte aligned");
    EGG_CHECK_ARG(mstride % 8 == 0, "rownorm: modulation stride must be a multiple of 8");
    EGG_CHECK_ARG((x_f32 == 0 || x_f32 == 1) && (mod_f32 == 0 || mod_f32 == 1) && (res_f32 == 0 || res_f32 == 1) &&
                      (out_f32 == 0 || out_f32 == 1) && !(x_f32 && out_f32) && (out_f32 || !shadow),
                  "rownorm: dtype flags are 0 / 1; fp32 x with fp32 out, or a shadow without fp32 out, unsupported");
    if (rows == 0) return EGGROLL_OK;
    EGG_CHECK_ARG(x && out, "rownorm: NULL pointer");
    hipStream_t st = as_stream(stream);
    const int nch = (int)(C / 8);
    int slots;  // chunk slots per row: SEG lanes (16 / 32 / 64) x NCH chunks per lane
    if (nch <= 16) slots = 16;
    else if (nch <= 32) slots = 32;
    else if (nch <= 64) slots = 64;
    else if (nch <= 128) slots = 64 * 2;
    else if (nch <= 256) slots = 64 * 4;
    // Sana's C = 2240 (280 chunks): 5 chunks per lane use 88 % of the slots (8: 55 %, 64 dead value
    // registers); a lane sums the same chunks in the same order either way, so the bits do not change
    else if (nch <= 320) slots = 64 * 5;
    else slots = 64 * 8;
    dispatch_int(slots, std::integer_sequence<int, 16, 32, 64, 128, 256, 320, 512>{}, [&](auto S) {
        constexpr int SEG = decltype(S)::value < 64 ? decltype(S)::value : 64;
        launch_rownorm<SEG, decltype(S)::value / SEG>(x, x_f32, rows, (int)C, eps, layer, w, b, mscale, mshift, mstride,
                                                      mod_f32, rows_per_group, act, res, res_f32, out, out_f32, shadow, st);
    });
    EGG_CHECK_LAUNCH("rownorm");
    return EGGROLL_OK;
}

extern "C" int eggroll_rownorm(const void* x, int64_t rows, int64_t C, float eps, int32_t layer, const void* w,
                               const void* b, const void* mscale, const void* mshift, int64_t mstride,
                               int64_t rows_per_group, int32_t act, const void* res, void* out, void* stream) {
    return eggroll_rownorm_ex(x, 0, rows, C, eps, layer, w, b, mscale, mshift, mstride, 0, rows_per_group, act, res,
                              0, out, 0, nullptr, stream);
}

extern "C" int eggroll_resid_layernorm(float* h, int64_t ldh, const void* y, int64_t ldy, int64_t rows, int64_t C,
                                       float eps, const void* w, const void* b, void* out, void* stream) {
    EGG_CHECK_ARG(rows >= 0 && C > 0 && C % 8 == 0 && C <= 4096, "resid_layernorm: need C %% 8 == 0, C <= 4096");
    EGG_CHECK_ARG(ldh >= C && ldh % 4 == 0 && (!y || (ldy >= C && ldy % 8 == 0)),
                  "resid_layernorm: row strides must cover C and keep 16-byte rows");
    EGG_CHECK_ARG(((uintptr_t)h & 15) == 0 && ((uintptr_t)y & 15) == 0 && ((uintptr_t)out & 15) == 0 &&
                      ((uintptr_t)w & 15) == 0 && ((uintptr_t)b & 15) == 0,
                  "resid_layernorm: pointers must be 16-byte aligned");
    if (rows == 0) return EGGROLL_OK;
    EGG_CHECK_ARG(h && w && b && out, "resid_layernorm: NULL pointer");
    EGG_CHECK_ARG(rows < (1ll << 31) / 4, "resid_layernorm: too many rows");
    hipStream_t st = as_stream(stream);
    const dim3 grid((unsigned)((rows + 3) / 4));
    const int nch = (int)(C / 8);
    auto* yy = (const unsigned short*)y;
    auto* ww = (const unsigned short*)w;
    auto* bb = (const unsigned short*)b;
    auto* oo = (unsigned short*)out;
    int per;  // chunks per lane
    if (nch <= 64) per = 1;
    else if (nch <= 128) per = 2;
    else if (nch <= 192) per = 3;   // CLIP-H: C = 1280 (160 chunks)
    else if (nch <= 256) per = 4;
    else per = 8;
    dispatch_int(per, std::integer_sequence<int, 1, 2, 3, 4, 8>{}, [&](auto P) {
        hipLaunchKernelGGL(k_resid_layernorm<decltype(P)::value>, grid, dim3(256), 0, st, h, ldh, yy, ldy, rows, (int)C,
                           eps, ww, bb, oo);
    });
    EGG_CHECK_LAUNCH("resid_layernorm");
    return EGGROLL_OK;
}

extern "C" int eggroll_gated_residual(void* x, const void* y, const void* gate, int64_t gstride, int64_t rows,
                                      int64_t C, int64_t rows_per_group, void* stream) {
    EGG_CHECK_ARG(rows >= 0 && C > 0 && C % 8 == 0 && gstride % 8 == 0 && rows_per_group > 0, "gated_residual: bad sizes");
    if (rows == 0) return EGGROLL_OK;
    EGG_CHECK_ARG(x && y && gate, "gated_residual: NULL pointer");
    const int64_t total = rows * (C / 8);
    hipLaunchKernelGGL(k_gated_residual, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, as_stream(stream),
                       (unsigned short*)x, (const unsigned short*)y, (const unsigned short*)gate, gstride,
                       rows_per_group, (int)C, total);
    EGG_CHECK_LAUNCH("gated_residual");
    return EGGROLL_OK;
}

extern "C" int eggroll_gated_residual_f32(float* x, const void* y, const void* gate, int32_t gate_f32, int64_t gstride,
                                          int64_t rows, int64_t C, int64_t rows_per_group, void* shadow, void* stream) {
    EGG_CHECK_ARG(rows >= 0 && C > 0 && C % 8 == 0 && gstride % 8 == 0 && rows_per_group > 0 &&
                      (gate_f32 == 0 || gate_f32 == 1),
                  "gated_residual_f32: bad sizes");
    EGG_CHECK_ARG(((uintptr_t)x & 15) == 0 && ((uintptr_t)y & 15) == 0 && ((uintptr_t)gate & 15) == 0 &&
                      ((uintptr_t)shadow & 15) == 0,
                  "gated_residual_f32: pointers must be 16-byte aligned");
    if (rows == 0) return EGGROLL_OK;
    EGG_CHECK_ARG(x && y, "gated_residual_f32: NULL pointer");
    const int64_t total = rows * (C / 8);
    hipLaunchKernelGGL(k_gated_residual_f32, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, as_stream(stream), x,
                       (const unsigned short*)y, gate, gate_f32, gstride, rows_per_group, (int)C, total,
                       (unsigned short*)shadow);
    EGG_CHECK_LAUNCH("gated_residual_f32");
    return EGGROLL_OK;
}

extern "C" int eggroll_scm_step(const float* x, int64_t x_member_stride, const void* eps, int32_t eps_f32,
                                const float* noise, int64_t members, int64_t n, float in_scale, float coef_m,
                                float coef_eps, float cos_t, float sin_t, float cos_n, float sin_n_sd,
                                float in_scale_next, float out_scale, int32_t round_dtype, float* x_next,
                                float* m_next, float* x0_out, void* stream) {
    EGG_CHECK_ARG(members > 0 && members <= 65535 && n > 0 && x_member_stride >= 0,
                  "scm_step: bad sizes (members %lld in 1..65535, n %lld > 0, x_member_stride %lld >= 0)",
                  (long long)members, (long long)n, (long long)x_member_stride);
    EGG_CHECK_ARG(round_dtype >= 0 && round_dtype <= 2, "scm_step: round_dtype %d is not 0 (none), 1 (fp16) or 2 (bf16)",
                  (int)round_dtype);
    EGG_CHECK_ARG(eps_f32 == 0 || eps_f32 == 1, "scm_step: eps_f32 must be 0 or 1");
    EGG_CHECK_ARG(x && eps, "scm_step: NULL x or eps");
    EGG_CHECK_ARG(noise || !x_next, "scm_step: x_next needs noise (noise is NULL)");
    EGG_CHECK_ARG(!(x_next == x && x_member_stride != n),
                  "scm_step: x_next may alias x only when every member has its own x (x_member_stride == n)");
    auto al = [](const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; };
    const bool vec = al(x, 16) && al(eps, eps_f32 ? 16 : 8) && al(noise, 16) && al(x_next, 16) && al(m_next, 16) &&
                     al(x0_out, 16) && (members == 1 || (n % 4 == 0 && x_member_stride % 4 == 0));
    const int64_t nvec = vec ? n / 4 : 0;
    const int64_t threads = nvec + (n - 4 * nvec);
    const dim3 grid((unsigned)((threads + 255) / 256), (unsigned)members);
    const ScmScalars s{in_scale, coef_m, coef_eps, cos_t, sin_t, cos_n, sin_n_sd, in_scale_next, out_scale};
    dispatch_int(round_dtype, std::integer_sequence<int, 0, 1, 2>{}, [&](auto RD) {
        dispatch_int(eps_f32, Flag01{}, [&](auto E32) {
            hipLaunchKernelGGL((k_scm_step<decltype(RD)::value, decltype(E32)::value>), grid, dim3(256), 0,
                               as_stream(stream), x, x_member_stride, eps, noise, n, nvec, s, x_next, m_next, x0_out);
        });
    });
    EGG_CHECK_LAUNCH("scm_step");
    return EGGROLL_OK;
}

extern "C" int eggroll_bias_act(void* y, const void* bias, int64_t rows, int64_t C, int32_t act, void* stream) {
    EGG_CHECK_ARG(rows >= 0 && C > 0 && C % 8 == 0 && act >= 0 && act <= 2, "bias_act: bad sizes/act");
    if (rows == 0) return EGGROLL_OK;
    EGG_CHECK_ARG(y && bias, "bias_act: NULL pointer");
    const int64_t total = rows * (C / 8);
    EGG_CHECK_ARG(total < (1ll << 32) - 256, "bias_act: tensor too large for 32-bit chunk index");
    hipLaunchKernelGGL(k_bias_act, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, as_stream(stream),
                       (unsigned short*)y, (const unsigned short*)bias, (unsigned)(C / 8), act, (unsigned)total);
    EGG_CHECK_LAUNCH("bias_act");
    return EGGROLL_OK;
}

// ------------------------------------------------------------------------------------
// GroupNorm (+ SiLU) on NHWC bf16 activations (the FLUX / Infinity VAE decoders' GroupNorm(32)):
//   y[b, p, c] = act((x - mean[b, g]) * rstd[b, g] * w[c] + bias[c]),  g = c / (C / G),
// statistics over the H*W pixels and C/G channels of (b, g), biased variance, fp32 data path.
// Three launches: (1) per (image, pixel chunk) partial per-group sums / sums of squares (fp32 over at most
// 256 x C/G values, reduced in a fixed order), (2) per (image, group) the chunks combined in fp64 ->
// mean, rstd, (3) normalise + affine + act, 16-B loads / stores.  The torch form (an fp32 copy,
// Welford statistics, four elementwise passes) moved ~10x the bytes.
// ------------------------------------------------------------------------------------
constexpr int GN_PASSES = 16;   // pixel passes per block: pixels per chunk = (256 / (C / 8)) * GN_PASSES

__global__ __launch_bounds__(256) void k_gn_stats(const unsigned short* __restrict__ x, int64_t HW, int C, int G,
                                                  int ppc, int nch, float2* __restrict__ part) {
    __shared__ float red[256][17];
    __shared__ float chs[2048][2];
    const int tid = threadIdx.x, tpp = C / 8, pps = 256 / tpp;   // threads per pixel, pixels per pass
    const int b = blockIdx.x / nch, ch = blockIdx.x - b * nch;
    const int slot = tid % tpp, pl = tid / tpp;
    float s[8], q[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) s[i] = q[i] = 0.f;
    if (pl < pps) {
        const int64_t p0 = (int64_t)ch * ppc;
#pragma unroll 4
        for (int k = 0; k < GN_PASSES; ++k) {
            const int64_t p = p0 + (int64_t)k * pps + pl;
            if (p < HW) {
                const u16x8m v = *reinterpret_cast<const u16x8m*>(x + ((int64_t)b * HW + p) * C + slot * 8);
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const float f = b2f(v[i]);
                    s[i] += f;
                    q[i] += f * f;
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        red[tid][i] = s[i];
        red[tid][8 + i] = q[i];
    }
    __syncthreads();
    // channel c = 8 slot + i: sum over the pixel lanes pl (fixed order)
    for (int c = tid; c < C; c += 256) {
        const int sl = c >> 3, i = c & 7;
        float a = 0.f, a2 = 0.f;
        for (int l = 0; l < pps; ++l) {
            a += red[l * tpp + sl][i];
            a2 += red[l * tpp + sl][8 + i];
        }
        chs[c][0] = a;
        chs[c][1] = a2;
    }
    __syncthreads();
    const int cpg = C / G;
    for (int g = tid; g < G; g += 256) {
        float a = 0.f, a2 = 0.f;
        for (int c = g * cpg; c < (g + 1) * cpg; ++c) {
            a += chs[c][0];
            a2 += chs[c][1];
        }
        part[((int64_t)b * nch + ch) * G + g] = float2{a, a2};
    }
}

__global__ __launch_bounds__(256) void k_gn_finalize(const float2* __restrict__ part, int G, int nch, double count,
                                                     float eps, float2* __restrict__ stats) {
    // one workgroup per (image, group): the chunk partials strided over the threads, then a fixed tree
    __shared__ double sa[256], sq[256];
    const int i = blockIdx.x, b = i / G, g = i - b * G, tid = threadIdx.x;
    double a = 0.0, a2 = 0.0;
    for (int c = tid; c < nch; c += 256) {
        const float2 v = part[((int64_t)b * nch + c) * G + g];
        a += v.x;
        a2 += v.y;
    }
    sa[tid] = a;
    sq[tid] = a2;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) {
            sa[tid] += sa[tid + h];
            sq[tid] += sq[tid + h];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const double mean = sa[0] / count;
        double var = sq[0] / count - mean * mean;
        var = var > 0.0 ? var : 0.0;
        stats[i] = float2{(float)mean, (float)(1.0 / sqrt(var + (double)eps))};
    }
}

template <int ACT>
__global__ __launch_bounds__(256) void k_gn_apply(const unsigned short* __restrict__ x, int64_t HW, int C, int G,
                                                  const float2* __restrict__ stats,
                                                  const unsigned short* __restrict__ w,
                                                  const unsigned short* __restrict__ bias, int64_t total8,
                                                  unsigned short* __restrict__ y) {
    const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;   // 8-channel unit
    if (u >= total8) return;
    const int tpp = C / 8, cpg = C / G;
    const int64_t pix = u / tpp;
    const int slot = (int)(u - pix * tpp);
    const int b = (int)(pix / HW);
    const u16x8m v = *reinterpret_cast<const u16x8m*>(x + u * 8);
    const u16x8m wv = *reinterpret_cast<const u16x8m*>(w + slot * 8);
    const u16x8m bv = *reinterpret_cast<const u16x8m*>(bias + slot * 8);
    u16x8m o;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int c = slot * 8 + i;
        const float2 st = stats[(int64_t)b * G + c / cpg];
        float t = (b2f(v[i]) - st.x) * st.y;
        t = t * b2f(wv[i]) + b2f(bv[i]);
        if (ACT == 1) t = silu(t);
        o[i] = f2b(t);
    }
    *reinterpret_cast<u16x8m*>(y + u * 8) = o;
}

static int64_t gn_chunks(int64_t HW, int C, int* ppc_out) {
    const int ppc = (256 / (C / 8)) * GN_PASSES;
    if (ppc_out) *ppc_out = ppc;
    return (HW + ppc - 1) / ppc;
}

extern "C" int64_t eggroll_group_norm_workspace_bytes(int64_t B, int64_t HW, int32_t C, int32_t G) {
    if (B < 0 || HW < 0 || C < 8 || C % 8 || G < 1 || C % G) return 0;
    return (B * gn_chunks(HW, C, nullptr) * G + B * G) * (int64_t)sizeof(float2);
}

extern "C" int eggroll_group_norm_nhwc(const void* x, int64_t B, int64_t HW, int32_t C, int32_t G, float eps,
                                       const void* w, const void* bias, int32_t act, void* y, void* workspace,
                                       void* stream) {
    EGG_CHECK_ARG(C >= 8 && C <= 2048 && C % 8 == 0 && G >= 1 && C % G == 0, "group_norm: need C %% 8 == 0, C <= 2048, "
                  "C %% G == 0 (C=%d G=%d)", C, G);
    EGG_CHECK_ARG(B >= 0 && HW >= 0 && act >= 0 && act <= 1, "group_norm: bad sizes / act");
    if (B == 0 || HW == 0) return EGGROLL_OK;
    EGG_CHECK_ARG(x && w && bias && y && workspace, "group_norm: NULL pointer");
    EGG_CHECK_ARG(((uintptr_t)x & 15) == 0 && ((uintptr_t)y & 15) == 0 && ((uintptr_t)w & 15) == 0 &&
                  ((uintptr_t)bias & 15) == 0 && ((uintptr_t)workspace & 7) == 0, "group_norm: misaligned pointer");
    int ppc = 0;
    const int64_t nch = gn_chunks(HW, C, &ppc);
    EGG_CHECK_ARG(B * nch < (1ll << 31) && B * G < (1ll << 31) && B * HW * C / 8 / 256 < (1ll << 31),
                  "group_norm: grid too large");
    float2* part = reinterpret_cast<float2*>(workspace);
    float2* stats = part + B * nch * G;
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(k_gn_stats, dim3((unsigned)(B * nch)), dim3(256), 0, st, (const unsigned short*)x, HW, C, G, ppc,
                       (int)nch, part);
    hipLaunchKernelGGL(k_gn_finalize, dim3((unsigned)(B * G)), dim3(256), 0, st, part, G, (int)nch,
                       (double)HW * (double)(C / G), eps, stats);
    const int64_t total8 = B * HW * C / 8;
    auto* k = act ? k_gn_apply<1> : k_gn_apply<0>;
    hipLaunchKernelGGL(k, dim3((unsigned)((total8 + 255) / 256)), dim3(256), 0, st, (const unsigned short*)x, HW, C, G,
                       stats, (const unsigned short*)w, (const unsigned short*)bias, total8, (unsigned short*)y);
    EGG_CHECK_LAUNCH("group_norm");
    return EGGROLL_OK;
}
