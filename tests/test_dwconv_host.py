"""Depthwise conv checks that need no GPU: the bound of tests/dwconv_cases.py discriminates (a CPU emulation of
the kernel's arithmetic passes it, two plausible rewrite mistakes do not), its input generators do what they
promise, and eggroll_dwconv_nhwc_ex / eggroll_dwconv_pw_nhwc_sel reject bad arguments before any launch."""
import functools

import pytest
import torch
import torch.nn.functional as F

from hyperscalees_t2i_amd import _lib
from tests import dwconv_cases as D

FORMS = [(ks, pre, glu) for ks in (3, 5) for pre in (False, True) for glu in (False, True)]


# ------------------------------------------------------------------ the bound, on an emulation of the kernel
def _silu32(x):
    """The device formula in fp32: x * rcp(1 + exp(-x))."""
    return x * (1.0 / (1.0 + torch.exp(-x)))


def _bf(x):
    return x.to(torch.bfloat16).float()


def _emulate(x, w, b, ks, pre, glu, mutation=None):
    """k_dwconv_nhwc in fp32 torch: bf16 SiLU staging, fp32 accumulation, one bf16 rounding.  mutation "glu_value":
    the value plane rounded to bf16 before gating; "bias_late": the bias added after the bf16 rounding."""
    C = x.shape[-1]
    xin = _bf(_silu32(x.float())) if pre else x.float()
    wc = w.float().t().reshape(C, 1, ks, ks)
    late = mutation == "bias_late"
    b32 = None if b is None or late else b.float()
    y = F.conv2d(xin.permute(0, 3, 1, 2), wc, b32, padding=ks // 2, groups=C).permute(0, 2, 3, 1)
    if late:
        y = _bf(y) + b.float()
    if glu:
        a, g = y.chunk(2, dim=-1)
        y = (_bf(a) if mutation == "glu_value" else a) * _silu32(g)
    return y.to(torch.bfloat16)


def _form_id(f):
    return "ks%d-pre%d-glu%d" % f


@functools.lru_cache(maxsize=None)
def _emu_case(form):
    """Inputs and fp64 reference of one form, computed once and shared by the tests below (never modified)."""
    ks, pre, glu = form
    x, w, b, share = D.real_inputs(2, 17, 40, 128, ks, seed=100 + ks + 2 * pre + glu, pre_silu=pre)
    assert share < 0.02
    return (ks, pre, glu), (x, w, b), D.ref_dwconv(x, w, b, ks, pre, glu)


def _ratio(got, r):
    return (got.double() - r.ref).abs() / D.tol(r)


@pytest.mark.parametrize("form", FORMS, ids=_form_id)
def test_emulated_kernel_is_within_the_bound(form):
    _, (x, w, b), r = _emu_case(form)
    q = _ratio(_emulate(x, w, b, *form), r)
    print(f"dwconv emulation ks{form[0]} pre{int(form[1])} glu{int(form[2])}: max err/tol {float(q.max()):.3f}")
    assert bool((q <= 1).all()), float(q.max())
    q0 = _ratio(_emulate(x, w, None, *form), D.ref_dwconv(x, w, None, *form))
    assert bool((q0 <= 1).all()), float(q0.max())


@pytest.mark.parametrize("form", FORMS, ids=_form_id)
def test_bias_after_rounding_exceeds_the_bound(form):
    _, (x, w, b), r = _emu_case(form)
    q = _ratio(_emulate(x, w, b, *form, mutation="bias_late"), r)
    share = float((q > 1).double().mean())
    print(f"dwconv bias-after-rounding ks{form[0]} pre{int(form[1])} glu{int(form[2])}: {100 * share:.1f}% outside, "
          f"max err/tol {float(q.max()):.1f}")
    assert share >= 0.01


@pytest.mark.parametrize("form", [f for f in FORMS if f[2]], ids=_form_id)
def test_rounded_glu_value_plane_exceeds_the_bound(form):
    _, (x, w, b), r = _emu_case(form)
    q = _ratio(_emulate(x, w, b, *form, mutation="glu_value"), r)
    share = float((q > 1).double().mean())
    print(f"dwconv rounded GLU value plane ks{form[0]} pre{int(form[1])}: {100 * share:.1f}% outside, "
          f"max err/tol {float(q.max()):.2f}")
    assert share >= 0.01


# ------------------------------------------------------------------------------------------ the generators
@pytest.mark.parametrize("ks", [3, 5])
def test_grid_inputs_are_exact_in_fp32(ks):
    """On grid_inputs fp32 and fp64 agree exactly, for the depthwise conv and the grouped 1x1 behind it, in the
    natural and in the reversed accumulation order."""
    x, w, b, pw = D.grid_inputs(2, 9, 33, 64, ks, seed=ks)
    assert all(bool((t.double() * 8 == (t.double() * 8).round()).all()) for t in (x, w, b, pw))
    assert float(x.double().abs().max()) <= 15 and float(w.double().abs().max()) <= 15 / 8
    assert float(b.double().abs().max()) <= 8 and float(pw.double().abs().max()) <= 1
    C = x.shape[-1]
    r = D.ref_dwconv(x, w, b, ks, False, False)
    for flip in (False, True):       # the taps in reverse: another order of the same fp32 sum
        xf, wf = (x.flip(1, 2), w.flip(0)) if flip else (x, w)
        wc = wf.float().t().reshape(C, 1, ks, ks)
        y32 = F.conv2d(xf.float().permute(0, 3, 1, 2), wc, b.float(), padding=ks // 2, groups=C).permute(0, 2, 3, 1)
        assert torch.equal((y32.flip(1, 2) if flip else y32).double(), r.ref)
    d32 = F.conv2d(x.float().permute(0, 3, 1, 2), w.float().t().reshape(C, 1, ks, ks), padding=ks // 2, groups=C)
    d32 = _bf(d32.permute(0, 2, 3, 1)).reshape(-1, C // 32, 32)
    ref = D.ref_dwconv_pw(x, w, pw, ks)
    for perm in (torch.arange(32), torch.arange(31, -1, -1)):
        z32 = torch.einsum("ngc,goc->ngo", d32[..., perm], pw.float()[..., perm]).reshape(ref.shape)
        assert torch.equal(z32.double(), ref)
    assert float(ref.abs().max()) > 100          # not a degenerate case


def test_unambiguous_silu_inputs_replace_few():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(1 << 18, generator=g).to(torch.bfloat16)
    y, share = D.unambiguous_silu_inputs(x)
    print(f"unambiguous_silu_inputs on randn: replaced {100 * share:.2f}%")
    assert 0 < share < 0.02
    assert not bool(D.silu_ambiguous(y).any())
    keep = y == x
    assert float((~keep).double().mean()) <= share and bool((y[~keep] == 0).all())
    # away from the ties the fp32 device formula stages the same bf16 value as the fp64 reference
    assert torch.equal(_bf(_silu32(y.float())), D.to_bf16(D.silu64(y)).float())


def test_silu_sweep_has_few_ambiguous_values():
    v = D.silu_sweep_values()
    amb = int(D.silu_ambiguous(v).sum())
    print(f"SiLU sweep: {amb} of {v.numel()} bf16 values ambiguous")
    a = v.double().abs()
    assert bool(((a == 0) | ((a >= 2.0 ** -60) & (a <= D.SILU_SWEEP_MAX))).all()) and int((a == 0).sum()) == 1
    assert v.numel() == 2 * (66 * 128 + 33) + 1   # binades 2^-60 .. 2^5, 64 .. 80, both signs, and 0
    assert amb / v.numel() < 0.005
    n = D.normal_bf16_values()
    assert n.numel() == 2 * 254 * 128 + 1 and bool(torch.isfinite(n.float()).all())


# ---------------------------------------------------------------------------------------- C-ABI argument errors
P = 0x10000     # a 16-byte aligned address that is never dereferenced: every call below fails its argument check


def _dw(lib, in_=P, w=P + 0x1000, bias=P + 0x2000, B=1, H=4, W=4, C=64, ks=3, pre=0, glu=0, out=P + 0x3000, ldo=None,
        kernel=0):
    ldo = (C // 2 if glu else C) if ldo is None else ldo
    rc = lib.eggroll_dwconv_nhwc_ex(in_, w, bias, B, H, W, C, ks, pre, glu, out, ldo, kernel, None)
    return rc, lib.eggroll_last_error()


def _pw(lib, in_=P, w=P + 0x1000, pw=P + 0x2000, B=1, H=4, W=4, C=64, ks=3, out=P + 0x3000, kernel=0):
    rc = lib.eggroll_dwconv_pw_nhwc_sel(in_, w, pw, B, H, W, C, ks, out, kernel, None)
    return rc, lib.eggroll_last_error()


DW_ERRORS = [
    ("kernel 3", dict(kernel=3), b"kernel must be"),
    ("kernel -1", dict(kernel=-1), b"kernel must be"),
    ("ks 7", dict(ks=7), b"ks=7"),
    ("C 48", dict(C=48), b"multiple of 32"),
    ("GLU C 96 (cout 48)", dict(C=96, glu=1), b"multiple of 32"),
    ("ldo below cout", dict(ldo=56), b"row stride 56 must be in [64, 96]"),
    ("ldo more than 32 above cout", dict(ldo=104), b"row stride 104"),
    ("GLU ldo more than 32 above cout", dict(C=64, glu=1, ldo=72), b"row stride 72 must be in [32, 64]"),
    ("ldo not a multiple of 8", dict(ldo=68), b"multiple of 8"),
    ("misaligned in", dict(in_=P + 8), b"16-byte aligned"),
    ("misaligned w_t", dict(w=P + 0x1002), b"16-byte aligned"),
    ("misaligned out", dict(out=P + 0x3004), b"16-byte aligned"),
    ("H*W*C = 2^30", dict(H=4096, W=4096), b"too large"),
    ("H*W*ldo >= 2^30", dict(H=4096, W=3000, ldo=96), b"too large"),
    ("2^31 blocks", dict(B=1 << 31, H=1, W=1, C=32), b"grid too large"),
    ("B < 0", dict(B=-1), b"bad sizes"),
    ("H = 0", dict(H=0), b"bad sizes"),
    ("NULL in", dict(in_=None), b"NULL"),
    ("NULL out", dict(out=None), b"NULL"),
]

PW_ERRORS = [
    ("C 48", dict(C=48), b"multiple of 32"),
    ("ks 7", dict(ks=7), b"ks=7"),
    ("kernel 3", dict(kernel=3), b"kernel must be"),
    ("out == in", dict(out=P), b"aliased"),
    ("NULL pw", dict(pw=None), b"NULL"),
    ("misaligned pw", dict(pw=P + 0x2008), b"16-byte aligned"),
    ("H*W*C = 2^30", dict(H=4096, W=4096), b"too large"),
    ("2^31 blocks", dict(B=1 << 31, H=1, W=1, C=32), b"grid too large"),
]


@pytest.mark.parametrize("what,args,msg", DW_ERRORS, ids=[e[0] for e in DW_ERRORS])
def test_dwconv_argument_errors(what, args, msg):
    rc, err = _dw(_lib.load(), **args)
    assert rc == -1 and err.startswith(b"dwconv: ") and msg in err, (rc, err)


@pytest.mark.parametrize("what,args,msg", PW_ERRORS, ids=[e[0] for e in PW_ERRORS])
def test_dwconv_pw_argument_errors(what, args, msg):
    rc, err = _pw(_lib.load(), **args)
    assert rc == -1 and err.startswith(b"dwconv_pw: ") and msg in err, (rc, err)


def test_dwconv_empty_batch_is_a_noop():
    """B == 0 returns 0 with NULL pointers, after the size checks: an image one element short of the limit
    passes them, the limit itself does not."""
    lib = _lib.load()
    none = dict(in_=None, w=None, out=None, B=0)
    assert _dw(lib, bias=None, **none)[0] == 0
    assert _dw(lib, bias=None, glu=1, C=320, ldo=192, **none)[0] == 0
    assert _dw(lib, bias=None, H=4096, W=4095, **none)[0] == 0
    assert _dw(lib, bias=None, H=4096, W=4096, **none)[0] == -1
    assert _pw(lib, pw=None, **none)[0] == 0
    assert _pw(lib, pw=None, H=4096, W=4095, **none)[0] == 0
    assert _pw(lib, pw=None, ks=7, **none)[0] == -1
