"""k_dwconv_nhwc on the GPU against the fp64 reference of tests/dwconv_cases.py: all 8 plain forms (KS 3/5 x
PRE_SILU x GLU) and the fused-1x1 (PW) forms, at every block order, with and without bias, on geometries that
meet every edge of the 8 x 32 x 32 tile.  Real data is held to the derived bound `tol` (dwconv_cases docstring),
integer-grid data to bitwise equality; padded output strides, guard bands around every buffer and a sweep of
the SiLU over all bf16 values complete it.  Every test prints its largest err/tol."""
import functools

import pytest
import torch

from hyperscalees_t2i_amd import kernels as K
from tests import dwconv_cases as D

pytestmark = pytest.mark.gpu

FORMS = [(ks, pre, glu) for ks in (3, 5) for pre in (False, True) for glu in (False, True)]
ORDERS = (0, 1, 2)      # auto, channel slice fastest, column sweep
# (B, H, W, C): one pixel; one ragged tile; exactly one tile; one row / column past the tile (3 images: 12 or 24
# blocks, 12 is no multiple of the 8 XCDs); two rows / columns past two tiles with an odd slice count (27 blocks);
# a ragged second tile column.  C is the input width: GLU forms take 320 for 96 (cout 160, 5 slices, odd) and
# write cout = C/2 = 32, 96 (3 slices) or 160.
GEOMS = [(1, 1, 1, 64), (2, 7, 31, 64), (1, 8, 32, 64), (3, 9, 33, 64), (1, 17, 65, 96), (2, 16, 40, 192)]


def _form_id(f):
    return "ks%d-pre%d-glu%d" % f


def _geom_id(g):
    return "x".join(map(str, g))


def _shape(geom, glu):
    B, H, W, C = geom
    return B, H, W, (320 if glu and C == 96 else C)


@functools.lru_cache(maxsize=None)
def _real_case(form, geom):
    """CPU inputs of one (form, geometry) and the fp64 references with and without bias; shared, never modified."""
    ks, pre, glu = form
    B, H, W, C = _shape(geom, glu)
    x, w, b, share = D.real_inputs(B, H, W, C, ks, seed=1000 * ks + 100 * pre + 10 * glu + H + W, pre_silu=pre)
    assert share < 0.02
    return x, w, b, share, {True: D.ref_dwconv(x, w, b, *form), False: D.ref_dwconv(x, w, None, *form)}


def _err_over_tol(got, r):
    """max err/tol of a device output against a DwRef, after asserting every element is inside the bound."""
    err = (got.cpu().double() - r.ref).abs()
    t = D.tol(r)
    inside = err <= t                                       # (NaN fails; err = tol = 0 passes)
    q = float((err / t.clamp_min(1e-300)).max())
    assert bool(inside.all()), f"{int((~inside).sum())} of {err.numel()} outside the bound, max err/tol {q:.3f}"
    return q


# ------------------------------------------------------------------------------- real data, all 8 plain forms
@pytest.mark.parametrize("geom", GEOMS, ids=_geom_id)
@pytest.mark.parametrize("form", FORMS, ids=_form_id)
def test_dwconv_vs_fp64(dev, form, geom):
    x, w, b, share, refs = _real_case(form, geom)
    xd, wd, bd = x.to(dev), w.to(dev), b.to(dev)
    q = max(_err_over_tol(K.dwconv_nhwc(xd, wd, bd if bias else None, *form, kernel=k), refs[bias])
            for bias in (True, False) for k in ORDERS)
    print(f"dwconv {_form_id(form)} {_geom_id(x.shape)}: max err/tol {q:.3f}, SiLU inputs replaced {100 * share:.2f}%")


# ------------------------------------------------------------------------------------ grid data, bit for bit
@pytest.mark.parametrize("geom", GEOMS, ids=_geom_id)
@pytest.mark.parametrize("ks", [3, 5])
def test_dwconv_grid_bitexact(dev, ks, geom):
    """On grid_inputs every fp32 partial sum is exact: the bf16-rounded fp64 reference is the only right answer,
    for the plain conv (with and without bias) and for the fused depthwise + grouped 1x1."""
    x, w, b, pw = D.grid_inputs(*geom, ks, seed=ks + sum(geom))
    xd, wd, bd, pwd = x.to(dev), w.to(dev), b.to(dev), pw.to(dev)
    want = {True: D.to_bf16(D.ref_dwconv(x, w, b, ks, False, False).ref),
            False: D.to_bf16(D.ref_dwconv(x, w, None, ks, False, False).ref)}
    want_pw = D.to_bf16(D.ref_dwconv_pw(x, w, pw, ks))
    for k in ORDERS:
        for bias in (True, False):
            got = K.dwconv_nhwc(xd, wd, bd if bias else None, ks, False, False, kernel=k).cpu()
            assert torch.equal(got, want[bias]), (k, bias, int((got != want[bias]).sum()))
        got = K.dwconv_pw_nhwc(xd, wd, pwd, ks, kernel=k).cpu()
        assert torch.equal(got, want_pw), (k, int((got != want_pw).sum()))


# --------------------------------------------------------------------------------------- PW on real data
@pytest.mark.parametrize("geom", GEOMS, ids=_geom_id)
@pytest.mark.parametrize("ks", [3, 5])
def test_dwconv_pw_vs_fp64(dev, ks, geom):
    """The fused depthwise + grouped 1x1 on real data, at the bound of test_dwconv_pw_vs_torch: the bf16 rounding
    of the intermediate can flip one ulp between two orders of the fp32 sum, so no tighter bound is derivable."""
    B, H, W, C = geom
    g = torch.Generator().manual_seed(C + ks + W)
    x = torch.randn(B, H, W, C, generator=g).to(torch.bfloat16)
    w = (torch.randn(ks * ks, C, generator=g) * 0.2).to(torch.bfloat16)
    pw = (torch.randn(C // 32, 32, 32, generator=g) / 32 ** 0.5).to(torch.bfloat16)
    ref = D.ref_dwconv_pw(x, w, pw, ks)
    t = 2.0 ** -7 * ref.abs() + 2e-3 * ref.abs().max()
    xd, wd, pwd = x.to(dev), w.to(dev), pw.to(dev)
    q = 0.0
    for k in ORDERS:
        err = (K.dwconv_pw_nhwc(xd, wd, pwd, ks, kernel=k).cpu().double() - ref).abs()
        q = max(q, float((err / t).max()))
        assert bool((err <= t).all()), f"order {k}: max err/tol {q:.3f}"
    print(f"dwconv_pw ks{ks} {_geom_id(geom)}: max err/tol {q:.3f}")


# ------------------------------------------------------------------------------------ padded output stride
@pytest.mark.parametrize("pad", [8, 32])
@pytest.mark.parametrize("form,geom", [((3, False, True), (3, 9, 33, 64)),     # cout 32: pad 32 doubles the row
                                       ((3, False, True), (1, 17, 65, 96)),    # C 320 -> ldo 192: the Sana FFN form
                                       ((5, True, True), (2, 16, 40, 192)),
                                       ((3, False, False), (1, 17, 65, 96)),
                                       ((5, True, False), (2, 7, 31, 64))],
                         ids=lambda v: _form_id(v) if len(v) == 3 else _geom_id(v))
def test_dwconv_padded_stride_vs_fp64(dev, form, geom, pad):
    """eggroll_dwconv_nhwc_ex with ldo = cout + 8 / cout + 32 into a buffer that starts as NaN: the first cout
    channels are within the bound of the fp64 reference, the pad channels come back as +0 bits."""
    x, w, b, _, refs = _real_case(form, geom)
    B, H, W, C = x.shape
    co = C // 2 if form[2] else C
    xd, wd, bd = x.to(dev), w.to(dev), b.to(dev)
    q = 0.0
    for k in ORDERS:
        out = torch.full((B, H, W, co + pad), float("nan"), dtype=torch.bfloat16, device=dev)
        got = K.dwconv_nhwc(xd, wd, bd, *form, out=out, kernel=k, ldo=co + pad)
        assert got.data_ptr() == out.data_ptr()
        q = max(q, _err_over_tol(got[..., :co], refs[True]))
        assert int(got[..., co:].contiguous().view(torch.int16).count_nonzero()) == 0
    print(f"dwconv {_form_id(form)} {_geom_id(x.shape)} ldo {co + pad}: max err/tol {q:.3f}")


# ------------------------------------------------------------------------------------------- guard bands
SENTINEL = 0x5A5B       # bf16 bits of the guard elements around `out` (a finite value the kernel never produces here)


def _guarded(t, dev, guard, fill=float("nan")):
    """t on the device as a 16-byte (not 32-byte) aligned slice of a larger allocation whose other elements are
    `fill`; returns the slice and the allocation."""
    assert guard % 16 == 8
    whole = torch.full((t.numel() + 2 * guard,), fill, dtype=torch.bfloat16, device=dev)
    view = whole[guard:guard + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 32 == 16 and view.is_contiguous()
    return view, whole


def _guarded_out(shape, dev, guard):
    n = 1
    for s in shape:
        n *= s
    whole = torch.full((n + 2 * guard,), SENTINEL, dtype=torch.int16, device=dev).view(torch.bfloat16)
    return whole[guard:guard + n].view(shape), whole


def _guards_intact(whole, guard):
    bits = whole.view(torch.int16)
    return bool((bits[:guard] == SENTINEL).all()) and bool((bits[-guard:] == SENTINEL).all())


@pytest.mark.parametrize("ks", [3, 5])
def test_dwconv_stays_inside_its_buffers(dev, ks):
    """Every operand is a slice of a larger allocation filled with NaN (the output: with a sentinel), and the two
    images differ by 2^12 in magnitude.  The zero padding comes from buffer-descriptor range checks: a descriptor
    that is too long reads a NaN or the other image's rows, one that is misplaced writes over a sentinel."""
    B, H, W, C = 2, 9, 33, 128
    x, w, b, _ = D.real_inputs(B, H, W, C, ks, seed=40 + ks)
    x = x * torch.tensor([1.0, 4096.0], dtype=torch.bfloat16).view(2, 1, 1, 1)      # exact in bf16
    g = torch.Generator().manual_seed(50 + ks)
    pw = (torch.randn(C // 32, 32, 32, generator=g) / 32 ** 0.5).to(torch.bfloat16)
    img = H * W * C + 8                                        # a whole image of guard on either side
    xd, _x = _guarded(x, dev, img)
    wd, _w = _guarded(w, dev, 1032)
    bd, _b = _guarded(b, dev, 1032)
    pwd, _p = _guarded(pw, dev, 1032)
    r = D.ref_dwconv(x, w, b, ks, False, True)
    ref_pw = D.ref_dwconv_pw(x, w, pw, ks)
    t_pw = 2.0 ** -7 * ref_pw.abs() + 2e-3 * ref_pw.abs().amax(dim=(1, 2, 3), keepdim=True)   # per image
    q = 0.0
    for k in ORDERS:
        out, whole = _guarded_out((B, H, W, C // 2), dev, img)
        K.dwconv_nhwc(xd, wd, bd, ks, False, True, out=out, kernel=k)
        q = max(q, _err_over_tol(out, r))
        assert _guards_intact(whole, img), f"dwconv order {k} wrote outside its output"
        out, whole = _guarded_out((B, H, W, C), dev, img)
        K.dwconv_pw_nhwc(xd, wd, pwd, ks, out=out, kernel=k)
        err = (out.cpu().double() - ref_pw).abs()
        assert bool((err <= t_pw).all()), f"dwconv_pw order {k}: max err/tol {float((err / t_pw).max()):.3f}"
        assert _guards_intact(whole, img), f"dwconv_pw order {k} wrote outside its output"
    print(f"dwconv guarded ks{ks}: max err/tol {q:.3f}")


# ---------------------------------------------------------------------------------------- SiLU value sweep
def _as_pixels(v, C):
    """The values of v as the pixels of one [1, H, 32, C] image (zero filled), and their count."""
    n = v.numel()
    H = -(-n // (32 * C))
    x = torch.zeros(H * 32 * C, dtype=torch.bfloat16)
    x[:n] = v
    return x.view(1, H, 32, C), n


def _centre_tap(ks, C, lo, hi):
    w = torch.zeros(ks * ks, C, dtype=torch.bfloat16)
    w[ks * ks // 2, lo:hi] = 1.0
    return w


def _check_silu_sweep(got, v, what):
    want = D.to_bf16(D.silu64(v))
    amb = D.silu_ambiguous(v)
    ulps = D.bf16_ulps_apart(got, want)
    assert bool(torch.isfinite(got.float()).all())
    print(f"{what}: {int((ulps > 0).sum())} of {v.numel()} values differ from the rounded fp64 SiLU, "
          f"{int(amb.sum())} are ambiguous, largest difference {int(ulps.max())} ulp")
    bad = (ulps > amb.to(ulps.dtype))
    assert not bool(bad.any()), [(float(a), float(g), float(e)) for a, g, e in zip(v[bad][:8], got[bad][:8], want[bad][:8])]


@pytest.mark.parametrize("ks", [3, 5])
def test_dwconv_silu_value_sweep(dev, ks):
    """Every finite bf16 value with 2^-60 <= |x| <= 80 (and 0) through the staged SiLU (pre_silu, centre weight 1,
    no bias) and through the GLU gate (value plane: weights 0, bias 1): the output is the bf16-rounded fp64 SiLU,
    at the values next to a rounding tie at most one ulp off."""
    v = D.silu_sweep_values()
    x, n = _as_pixels(v, 32)
    got = K.dwconv_nhwc(x.to(dev), _centre_tap(ks, 32, 0, 32).to(dev), None, ks, True, False).cpu()
    _check_silu_sweep(got.reshape(-1)[:n], v, f"staged SiLU ks{ks}")
    xg = torch.cat([torch.ones_like(x), x], dim=-1)                  # [value plane | gate plane]
    bias = torch.cat([torch.ones(32), torch.zeros(32)]).to(torch.bfloat16)
    got = K.dwconv_nhwc(xg.to(dev), _centre_tap(ks, 64, 32, 64).to(dev), bias.to(dev), ks, False, True).cpu()
    _check_silu_sweep(got.reshape(-1)[:n], v, f"GLU gate SiLU ks{ks}")


@pytest.mark.parametrize("ks", [3, 5])
def test_dwconv_identity_returns_every_bf16_value(dev, ks):
    """pre_silu off, centre weight 1, no bias: every normal finite bf16 value (and 0) comes back as the same bits,
    whatever its neighbours (their products with the zero weights are zeros)."""
    v = D.normal_bf16_values()
    x, n = _as_pixels(v, 32)
    got = K.dwconv_nhwc(x.to(dev), _centre_tap(ks, 32, 0, 32).to(dev), None, ks, False, False).cpu()
    assert torch.equal(got.view(torch.int16), x.view(torch.int16))
