"""Depthwise conv test cases shared by tests/test_dwconv_host.py and tests/test_gpu_dwconv.py: the fp64
reference of k_dwconv_nhwc (plain torch on the CPU, no kernel call), the input generators, and the bound the
kernel is held to against the reference.

The bound (`tol`), derived from the kernel's arithmetic, not measured
---------------------------------------------------------------------
u32 = 2^-24 and u16 = 2^-8 are the unit roundoffs of fp32 and bf16 (8 significand bits: half an ulp is up to
2^-8 of the value).

Plain forms.  The kernel forms acc = b + sum_i x_i w_i in fp32 over KS*KS <= 25 taps and rounds acc to bf16
once.  x_i and w_i are bf16, so every product is exact in fp32 (16 significand bits) whether or not the
compiler contracts it into an FMA; only the <= 25 additions round.  Each rounds a partial sum that is at
most M = |b| + sum_i |x_i w_i| (1 + 25 u32), so in any order

    |acc - ref| <= 25 u32 (1 + 25 u32) M = 2^-19.36 M.

The bf16 rounding adds at most u16 |acc| <= u16 (|ref| + |acc - ref|):

    |out - ref| <= 2^-8 |ref| + (1 + 2^-8) 2^-19.36 M  <=  2^-8 |ref| + 2^-18 M.

With PRE_SILU the kernel stages silu(x) as bf16 and the reference rounds its fp64 SiLU to bf16 likewise; the
two staged values are the same bits as long as the fp64 SiLU is not next to a rounding tie, which
`unambiguous_silu_inputs` guarantees, so the x_i of both sides are equal and the bound is unchanged.

GLU forms.  out = bf16(A' * silu'(G')) with A' = A + eA, G' = G + eG the fp32 sums of the two planes,
|eA| <= 2^-19.36 M_a and |eG| <= 2^-19.36 M_g as above.  The device SiLU is x * rcp(1 + __expf(-x)).
v_exp_f32, the add, v_rcp_f32 and the product cost about 3 u32 = 2^-22.4 relative (about 2^-21 with the term
below at |x| <= 2).  __expf is exp2(x * log2(e)), whose argument rounding and constant give e^-x a relative
error d of about |x| 2^-23.4, which reaches the SiLU scaled by e^-x / (1 + e^-x): for x >= 0 that is at most
x e^-x 2^-23.4 < 2^-24.8, and for x < 0, where |silu(x)| <= 0.2785, an absolute 0.2785 |x| 2^-23.4 < 2^-25 |x|
<= 2^-25 M_g.  |d silu / dx| <= 1.0998 < 1.1, so

    |silu'(G') - silu(G)| <= 1.1 |eG| + 2^-25 M_g + 2^-22 |silu(G)|,

and the fp32 product A' * silu' adds u32 |A silu(G)|.  To first order

    |A' silu'(G') - A silu(G)| <= (2^-22 + 2^-24) |ref| + 2^-19.36 M_a |silu(G)| + (1.1 2^-19.36 + 2^-25) |A| M_g,

the bf16 rounding adds u16 (|ref| + that), and (1 + 2^-8) of each coefficient is still below the power of two
it is rounded up to:

    |out - ref| <= (2^-8 + 2^-18) |ref| + 2^-18 (M_a |silu(G)| + 1.1 |A| M_g).

What the bound catches: rounding the value plane to bf16 before gating costs up to another 2^-8 |ref|, and
adding the bias after the bf16 rounding costs up to 2^-8 |acc - b| plus a second rounding; the first term
has no room for either (tests/test_dwconv_host.py checks both on a CPU emulation of the kernel).

Rounding fp64 to bf16 here goes through fp32 (torch's conversion).  The double rounding cannot change a
result these tests use: the grid values are exact in fp32, and a SiLU value near enough to a bf16 tie for
it to matter (2^-24 relative) is far inside the 2^-16 margin that marks it ambiguous.
"""
from typing import NamedTuple, Optional

import torch
import torch.nn.functional as F

SILU_TIE_MARGIN = 2.0 ** -8  # in bf16 ulps: 2^-16..2^-15 relative; the device SiLU's error is ~2^-21 at |x| <= 2
#                              and 3 * 2^-24 + |x| 2^-23.4 < 2^-16.9 at the sweep's x = -80 (module docstring)
SILU_SWEEP_MAX = 80.0        # exp(80) is finite in fp32 and silu(-80) ~ -1.4e-33 is a normal fp32 and bf16


class DwRef(NamedTuple):
    ref: torch.Tensor                 # fp64 result [B, H, W, cout]
    M: torch.Tensor                   # |b| + sum |x w|: [B, H, W, C] (GLU: [2, B, H, W, C/2], value / gate plane)
    planes: Optional[torch.Tensor]    # GLU: the fp64 planes [2, B, H, W, C/2] (A, G); else None


def silu64(x):
    x = x.double()
    return x / (1.0 + torch.exp(-x))


def to_bf16(t64):
    """fp64 -> bf16, round to nearest even (through fp32: see the module docstring)."""
    return t64.float().to(torch.bfloat16)


def _conv64(x64, w_t, bias, ks):
    """x64 [B,H,W,C] fp64, w_t [ks*ks, C], bias [C] or None -> fp64 [B,H,W,C], stride 1, zero pad ks/2."""
    C = x64.shape[-1]
    wc = w_t.double().t().reshape(C, 1, ks, ks)
    b = None if bias is None else bias.double()
    return F.conv2d(x64.permute(0, 3, 1, 2), wc, b, padding=ks // 2, groups=C).permute(0, 2, 3, 1).contiguous()


def ref_dwconv(x, w_t, bias, ks, pre_silu, glu) -> DwRef:
    """fp64 reference of k_dwconv_nhwc on bf16 CPU tensors x [B,H,W,C], w_t [ks*ks, C], bias [C] or None."""
    assert x.dtype == w_t.dtype == torch.bfloat16 and x.device.type == "cpu" and (bias is None or bias.dtype == x.dtype)
    xin = to_bf16(silu64(x)).double() if pre_silu else x.double()   # the kernel stages the tile as bf16
    y = _conv64(xin, w_t, bias, ks)
    M = _conv64(xin.abs(), w_t.abs(), None if bias is None else bias.abs(), ks)
    if not glu:
        return DwRef(y, M, None)
    planes = torch.stack(y.chunk(2, dim=-1))
    return DwRef(planes[0] * silu64(planes[1]), torch.stack(M.chunk(2, dim=-1)), planes)


def ref_dwconv_pw(x, w_t, pw, ks):
    """fp64 reference of the fused depthwise + grouped 1x1 form: the conv in fp64 rounded to bf16 (the tile the
    kernel hands to the MFMA), then the 32x32 product of every channel group in fp64.  pw [C/32, 32 out, 32 in]."""
    B, H, W, C = x.shape
    d = to_bf16(_conv64(x.double(), w_t, None, ks)).double()
    return torch.einsum("ngc,goc->ngo", d.reshape(-1, C // 32, 32), pw.double()).reshape(B, H, W, C)


def tol(r: DwRef):
    """Allowed |kernel - r.ref| per element (module docstring)."""
    if r.planes is None:
        return 2.0 ** -8 * r.ref.abs() + 2.0 ** -18 * r.M
    A, G = r.planes
    return (2.0 ** -8 + 2.0 ** -18) * r.ref.abs() + 2.0 ** -18 * (r.M[0] * silu64(G).abs() + 1.1 * A.abs() * r.M[1])


def silu_ambiguous(x):
    """Mask of the elements of x whose fp64 SiLU lies within SILU_TIE_MARGIN bf16 ulps of a bf16 rounding tie:
    there the device SiLU (fp32, relative error below the margin) may round to the other neighbour."""
    s = silu64(x).abs()
    _, e = torch.frexp(s)                                  # s = m * 2^e, m in [0.5, 1): bf16 ulp = 2^(e - 8)
    frac = torch.ldexp(s, 8 - e) % 1.0                     # position inside the ulp; a tie is at 0.5
    return ((frac - 0.5).abs() < SILU_TIE_MARGIN) & (s > 0)


def unambiguous_silu_inputs(x):
    """x with every element whose SiLU is ambiguous (silu_ambiguous) set to 0, and the replaced share."""
    amb = silu_ambiguous(x)
    return torch.where(amb, torch.zeros_like(x), x), float(amb.double().mean())


def silu_sweep_values():
    """Every finite bf16 value with 2^-60 <= |x| <= SILU_SWEEP_MAX, plus 0."""
    bits = torch.arange(0, 1 << 16, dtype=torch.int32).to(torch.int16)
    v = bits.view(torch.bfloat16)
    a = v.double().abs()
    keep = torch.isfinite(a) & (((a >= 2.0 ** -60) & (a <= SILU_SWEEP_MAX)) | (bits == 0))
    return v[keep]


def normal_bf16_values():
    """Every normal finite bf16 value, plus 0."""
    bits = torch.arange(0, 1 << 16, dtype=torch.int32).to(torch.int16)
    v = bits.view(torch.bfloat16)
    a = v.double().abs()
    return v[(torch.isfinite(a) & (a >= 2.0 ** -126)) | (bits == 0)]


def real_inputs(B, H, W, C, ks, seed, pre_silu=False):
    """randn x, w ~ randn / ks, bias ~ randn (bf16, CPU), and for pre_silu the share of x that
    unambiguous_silu_inputs replaced (else 0)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, H, W, C, generator=g).to(torch.bfloat16)
    w = (torch.randn(ks * ks, C, generator=g) / ks).to(torch.bfloat16)
    b = torch.randn(C, generator=g).to(torch.bfloat16)
    share = 0.0
    if pre_silu:
        x, share = unambiguous_silu_inputs(x)
    return x, w, b, share


def grid_inputs(B, H, W, C, ks, seed):
    """x: integers in [-15, 15]; w: k/8, |k| <= 15; bias: k/8, |k| <= 64; pw [C/32, 32, 32]: k/8, |k| <= 8 (bf16,
    CPU).  Every partial sum of the depthwise conv is a multiple of 1/8 below 2^10 and so exact in fp32; the
    bf16-rounded conv (no bias) has 8 significant bits, its products with pw are multiples of 2^-6 and every
    partial sum of 32 of them stays below 2^15: exact in fp32 too.  So the fp64 reference rounded to bf16 is the
    only correct output, bit for bit, in any accumulation order."""
    g = torch.Generator().manual_seed(seed)

    def ints(shape, k):
        return torch.randint(-k, k + 1, shape, generator=g).double()
    x = ints((B, H, W, C), 15).to(torch.bfloat16)
    w = (ints((ks * ks, C), 15) / 8).to(torch.bfloat16)
    b = (ints((C,), 64) / 8).to(torch.bfloat16)
    pw = (ints((C // 32, 32, 32), 8) / 8).to(torch.bfloat16)
    return x, w, b, pw


def bf16_ulps_apart(a, b):
    """Distance in bf16 ulps between two finite bf16 tensors (0 and -0 coincide)."""
    def key(t):
        i = t.contiguous().view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7fff), i)
    return (key(a) - key(b)).abs()
