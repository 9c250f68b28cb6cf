"""The layout contract of the LoRA GEMM family's C interface (include/eggroll.h): ldx / ldw any multiple of
8 >= K, ldy / ldr / gstride anything >= N, 16-byte alignment of Y / res / gate an optimisation and never a
requirement, and no byte outside the [M, N] a call owns ever read into a result or written.

Every operand is a view into a larger, poisoned allocation (`_Buf`): inputs sit in NaN (padding columns
and trailing rows), outputs in a fixed bit pattern no result can equal.  After each call the pattern must
still be there, bit for bit, everywhere but in the owned [M, N], and the owned region must hold no NaN.

Layouts:  L0 packed (strides = sizes, allocator bases: what the rest of the suite runs);
          L1 padded and 16-byte aligned (the vector paths with ld != size);
          L2 padded and unaligned (every element-form fallback).
Shapes:   S1 = 600 x 203 x 128, 260 rows per member: three 256-row tiles (the last ragged), members changing
          inside tiles, two K-tiles, N = 25 * 8 + 3 (a 3-column element tail; odd, so packed rows alternate
          between aligned and unaligned);  S2 = 300 x 331 x 192, 100 rows per member: three K-tiles, two
          column tiles for 256- and 320-wide tiles, members shorter than a tile (r 3 / 4, tiles 128 / 9 and the
          automatic choice, tile 0)."""
import functools
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from hyperscalees_t2i_amd import _lib, kernels as K
from tests.lora_cases import lora_case, lora_ref, lora_tol

pytestmark = pytest.mark.gpu

BF16_SENTINEL = 0x7FC1        # a bf16 NaN with a payload: no kernel result has these bits
F32_SENTINEL = 0x7FC00001     # the same for the fp32 residual stream
GUARD_ROWS = 2

S1 = dict(M=600, N=203, Kd=128, rpm=260)
S2 = dict(M=300, N=331, Kd=192, rpm=100)
RPG = 150                     # gate groups change inside a tile and are not aligned with members
LAYOUTS = ("L0", "L1", "L2")


def _ld8(n):
    return -(-(n + 8) // 8) * 8   # the next multiple of 8 that is >= n + 8


def _geometry(layout, N, Kd):
    """operand -> (leading dimension, offset of the view's first element in its 16-byte aligned buffer), in
    elements of the operand's type."""
    if layout == "L0":
        return dict(x=(Kd, 0), w=(Kd, 0), y=(N, 0), res16=(N, 0), res32=(N, 0), gate16=(N, 0), gate32=(N, 0))
    if layout == "L1":
        ld = _ld8(N)
        return dict(x=(Kd + 8, 8), w=(Kd + 16, 8), y=(ld, 8), res16=(ld, 8), res32=(ld, 4), gate16=(ld + 8, 8),
                    gate32=(ld + 8, 4))
    return dict(x=(Kd + 8, 8), w=(Kd + 16, 8), y=(N + 5, 3), res16=(N + 3, 1), res32=(N + 1, 1), gate16=(N + 5, 1),
                gate32=(N + 5, 1))


class _Buf:
    """A [rows, cols] view, rows `ld` apart, `off` elements into a poisoned allocation with GUARD_ROWS rows
    after the last one.  poison "nan": an input; "bits": an output, pre-filled with the sentinel pattern."""

    def __init__(self, dev, dtype, rows, cols, ld, off, data=None, poison="bits"):
        self.dtype, self.shape, self.ld, self.off = dtype, (rows, cols), ld, off
        n = off + (rows + GUARD_ROWS) * ld + 8
        self.itype, self.sentinel = (torch.int16, BF16_SENTINEL) if dtype == torch.bfloat16 else (torch.int32, F32_SENTINEL)
        if poison == "nan":
            self.buf = torch.full((n,), float("nan"), dtype=dtype, device=dev)
        else:
            self.buf = torch.full((n,), self.sentinel, dtype=self.itype, device=dev).view(dtype)
        assert self.buf.data_ptr() % 16 == 0
        self.view = self.buf.as_strided((rows, cols), (ld, 1), off)
        if data is not None:
            self.view.copy_(data)

    @property
    def ptr(self):
        return self.view.data_ptr()

    def bits(self):
        return self.view.contiguous().view(self.itype)

    def check(self, what, written=True):
        """Everything outside the view (padding columns, guard rows, the elements before the view) still holds
        the pattern; the view holds no NaN (written) or still the pattern everywhere (not written)."""
        b = self.buf.view(self.itype).clone()
        if written:
            b.as_strided(self.shape, (self.ld, 1), self.off).fill_(self.sentinel)
        bad = (b != self.sentinel).nonzero().flatten()
        assert bad.numel() == 0, (f"{what}: {bad.numel()} elements outside the owned region were written, the first at "
                                  f"buffer offset {int(bad[0])} (view offset {self.off}, ld {self.ld}, shape {self.shape})")
        if written:
            assert not torch.isnan(self.view).any(), f"{what}: NaN in the owned region (unwritten, or padding read)"


@functools.lru_cache(maxsize=None)
def _case(shape, r):
    """Operands, projection and fp64 oracle of one (shape, r), built once and never modified."""
    s = dict(S1=S1, S2=S2)[shape]
    dev = torch.device("cuda:0")
    M, N, Kd, rpm = s["M"], s["N"], s["Kd"], s["rpm"]
    x, W, b, tp, offA, offB = lora_case(dev, M, N, Kd, r, rpm, seed=11)
    scale = 8.0 / r if r else 0.0
    c = dict(s, r=r, x=x, W=W, b=b, tp=tp, offA=offA, offB=offB, scale=scale)
    c["T"] = K.lora_project(x, tp, offA, r, rpm) if r else None
    c["ref"] = lora_ref(x, W, b, tp, offA, offB, r, scale, rpm)
    g = torch.Generator().manual_seed(12)
    c["res16"] = torch.randn(M, N, generator=g).to(torch.bfloat16).to(dev)
    c["res32"] = torch.randn(M, N, generator=g).to(dev)
    c["gate32"] = torch.randn(-(-M // RPG), N, generator=g).to(dev)
    c["gate16"] = c["gate32"].to(torch.bfloat16)
    torch.cuda.synchronize()
    return c


def _run(c, layout, api, kernel, epi=None, inplace=False, y_null=False):
    """One call of a C entry point on case c under `layout`, every operand in a poisoned allocation.
    api: "linear_pop" (the projection runs inside the call) or "gemm" (T given).  epi: a kernels.EPI name.
    inplace: the bf16 residual aliases Y (Y's layout).  y_null: fp32 stream without the bf16 shadow.
    Returns the bits of the owned output regions, packed: dict(y=..., res=...) (res: the fp32 stream)."""
    dev = c["x"].device
    M, N, Kd, r, rpm = c["M"], c["N"], c["Kd"], c["r"], c["rpm"]
    geo = _geometry(layout, N, Kd)
    X = _Buf(dev, torch.bfloat16, M, Kd, *geo["x"], data=c["x"], poison="nan")
    Wb = _Buf(dev, torch.bfloat16, N, Kd, *geo["w"], data=c["W"], poison="nan")
    code = K.EPI[epi]
    f32 = code in (4, 5)
    bufs = {}
    Y = None
    if not y_null:
        Y = bufs["y"] = _Buf(dev, torch.bfloat16, M, N, *geo["y"])
    res_ptr, ldr = None, 0
    if code in (2, 3, 7):
        if inplace:      # res aliases Y: read and written through the same pointer and stride
            Y.view.copy_(c["res16"])
            res_ptr, ldr = Y.ptr, Y.ld
        else:
            R = _Buf(dev, torch.bfloat16, M, N, *geo["res16"], data=c["res16"], poison="nan")
            res_ptr, ldr = R.ptr, R.ld
    elif f32:            # the fp32 stream is updated in place: an output, so it sits in the bit pattern
        R = bufs["res"] = _Buf(dev, torch.float32, M, N, *geo["res32"], data=c["res32"])
        res_ptr, ldr = R.ptr, R.ld
    gate_ptr, gstride = None, 0
    if code in (3, 5):
        gk = "gate32" if f32 else "gate16"
        G = _Buf(dev, c[gk].dtype, c[gk].shape[0], N, *geo[gk], data=c[gk], poison="nan")
        gate_ptr, gstride = G.ptr, G.ld
    tp_ptr, ld_t = (c["tp"].data_ptr(), c["tp"].stride(0)) if r else (None, 0)
    st = K._stream(dev)
    y_ptr, ldy = (Y.ptr, Y.ld) if Y is not None else (None, N)
    head = (X.ptr, X.ld, Wb.ptr, Wb.ld, c["b"].data_ptr())
    dims = (r, c["scale"], rpm, M, N, Kd, y_ptr, ldy)
    tail = (code, res_ptr, ldr, gate_ptr, gstride, RPG, kernel, st) if epi else (kernel, st)
    if api == "linear_pop":
        ws = torch.empty(K.lora_workspace_numel(M, Kd, r, rpm), dtype=torch.float32, device=dev) if r else None
        name = "eggroll_lora_linear_pop_epi_sel" if epi else "eggroll_lora_linear_pop_sel"
        args = head + (tp_ptr, ld_t, c["offA"], c["offB"]) + dims + (K._p(ws),) + tail
    else:
        name = "eggroll_lora_gemm_epi_sel" if epi else "eggroll_lora_gemm_sel"
        args = head + (K._p(c["T"]), tp_ptr, ld_t, c["offB"]) + dims + tail
    _lib.call(name, *args)
    torch.cuda.synchronize()
    what = f"{name} kernel={kernel} epi={epi} r={r} {layout}"
    for k, b in bufs.items():
        b.check(f"{what} [{k}]")
    return {k: b.bits() for k, b in bufs.items()}


# ---------------------------------------------------------------------------------- 1. plain GEMM, every tile kind
PLAIN = ([(t, "S1", r) for t in (8, 10) for r in (0, 1, 2)] +
         [(t, "S1", r) for t in (128, 0, 9) for r in (0, 2)] +
         [(t, "S2", r) for t in (128, 0, 9) for r in (3, 4)] +
         [(t, "S2", 0) for t in (128, 0, 8, 9, 10)])
PLAIN = [(t, s, r, api) for t, s, r in PLAIN for api in ("linear_pop", "gemm")]


@pytest.mark.parametrize("tile,shape,r,api", PLAIN, ids=[f"tile{t}-{s}-r{r}-{a}" for t, s, r, a in PLAIN])
def test_plain_gemm_layouts(dev, tile, shape, r, api):
    """Every tile kind, through eggroll_lora_linear_pop_sel and eggroll_lora_gemm_sel: the packed call is
    within the suite's bf16 bound of the fp64 oracle; the padded-aligned and padded-unaligned calls equal it
    bit for bit (no arithmetic depends on a stride); nothing outside [M, N] is written or read.  Tile 0 is the
    library's automatic choice: its packed output equals, bit for bit, that of the kernel kernels.gemm_tile_for
    names (the Python mirror agrees with the library)."""
    c = _case(shape, r)
    y = {L: _run(c, L, api, tile)["y"] for L in LAYOUTS}
    got = y["L0"].view(torch.bfloat16).float().cpu().numpy()
    err = np.abs(got - c["ref"])
    assert (err <= lora_tol(c["ref"], c["Kd"])).all(), float(err.max())
    for L in ("L1", "L2"):
        assert torch.equal(y[L], y["L0"]), f"{L} differs from L0 in {int((y[L] != y['L0']).sum())} elements"
    if tile == 0:
        named = K.gemm_tile_for(c["M"], c["N"], r, c["rpm"])
        assert torch.equal(y["L0"], _run(c, "L0", api, named)["y"]), f"automatic choice differs from kernel {named}"


# ---------------------------------------------------------------------------------- 2. every epilogue op
def _pad8(t):
    """[.., N] -> [.., N padded to a multiple of 8] with zeros: the separate elementwise kernels need C % 8 == 0."""
    return F.pad(t, (0, -t.shape[-1] % 8)).contiguous()


def _unfused(c, epi):
    """Kernel 8's plain packed output followed by the separate op the epilogue fuses: (y bf16, stream fp32)."""
    N = c["N"]
    y = _run(c, "L0", "gemm", 8)["y"].view(torch.bfloat16)
    if epi == "silu":
        return (y.float() * torch.reciprocal(1.0 + torch.exp(-y.float()))).to(torch.bfloat16), None
    if epi == "gelu":
        return F.gelu(y, approximate="tanh"), None
    if epi == "gelu_erf":
        return F.gelu(y), None
    if epi == "res":
        return (c["res16"].float() + y.float()).to(torch.bfloat16), None
    if epi == "mul":
        return c["res16"] * y, None
    if epi == "gated":
        out = K.gated_residual_(_pad8(c["res16"]), _pad8(y), _pad8(c["gate16"]), rows_per_group=RPG)
        return out[:, :N].contiguous(), None
    stream, sh = _pad8(c["res32"]), torch.empty_like(_pad8(y))
    K.gated_residual_f32_(stream, _pad8(y), _pad8(c["gate32"]) if epi == "gated32" else None, RPG, shadow=sh)
    return sh[:, :N].contiguous(), stream[:, :N].contiguous()


EPI_CASES = ([(e, False) for e in ("silu", "gelu", "gelu_erf", "res", "gated", "mul", "res32", "gated32")] +
             [(e, True) for e in ("res", "gated", "mul")])


@pytest.mark.parametrize("api", ["linear_pop", "gemm"])
@pytest.mark.parametrize("r", [0, 2])
@pytest.mark.parametrize("epi,inplace", EPI_CASES, ids=[e + ("-inplace" if i else "") for e, i in EPI_CASES])
def test_epilogue_layouts(dev, epi, inplace, r, api):
    """Every epilogue op on both 8-phase tiles (kernels 8 and 10), through eggroll_lora_linear_pop_epi_sel and
    eggroll_lora_gemm_epi_sel.  Packed == kernel 8's plain output followed by the separate op (bitwise, or
    the suite's bound against torch for silu / gelu); padded-aligned and padded-unaligned == packed bit for bit
    for every op, silu and gelu included (an element's bits do not depend on whether the vector or the
    element form stored it); kernel 10 == kernel 8 in every layout; poison intact, the in-place res included."""
    c = _case("S1", r)
    f32 = epi in ("res32", "gated32")
    out = {(k, L): _run(c, L, api, k, epi=epi, inplace=inplace) for k in (8, 10) for L in LAYOUTS}
    ref_y, ref_stream = _unfused(c, epi)
    got = out[8, "L0"]["y"].view(torch.bfloat16)
    if epi == "silu":
        assert float((got.float() - ref_y.float()).abs().max()) <= float(ref_y.float().abs().max()) * 2 ** -7
    elif epi == "gelu":
        diff = (got.float() - ref_y.float()).abs()
        assert (diff <= ref_y.float().abs() * 2 ** -7 + 1e-5).all(), float(diff.max())
        assert (diff == 0).float().mean().item() > 0.99
    else:
        assert torch.equal(got.view(torch.int16), ref_y.view(torch.int16)), int((got != ref_y).sum())
    if f32:
        assert torch.equal(out[8, "L0"]["res"], ref_stream.view(torch.int32))
    for k in (8, 10):
        for L in LAYOUTS:
            for name, bits in out[k, L].items():
                base = out[8, "L0"][name]
                assert torch.equal(bits, base), (f"kernel {k} {L} [{name}] differs from kernel 8 L0 in "
                                                 f"{int((bits != base).sum())} elements")
    if f32:   # Y = NULL: the stream alone, same bits
        for k in (8, 10):
            for L in LAYOUTS:
                o = _run(c, L, api, k, epi=epi, y_null=True)
                assert list(o) == ["res"] and torch.equal(o["res"], out[8, "L0"]["res"]), (k, L)


# ---------------------------------------------------------------------------------- 3. the pieces
@pytest.mark.parametrize("r", [1, 2, 4])
def test_project_padded_x(dev, r):
    """eggroll_lora_project over X with ldx = K + 8 in NaN padding == the packed call, bit for bit."""
    c = _case("S1", 2)
    M, Kd, rpm = c["M"], c["Kd"], c["rpm"]
    tp = (torch.randn(-(-M // rpm), r * Kd + 4, generator=torch.Generator().manual_seed(r)) * 0.1).to(dev)
    out = []
    for ld, off in ((Kd, 0), (Kd + 8, 8)):
        X = _Buf(dev, torch.bfloat16, M, Kd, ld, off, data=c["x"], poison="nan")
        T = _Buf(dev, torch.float32, M, r, r, 4)
        _lib.call("eggroll_lora_project", X.ptr, X.ld, tp.data_ptr(), tp.stride(0), 4, r, rpm, M, Kd, T.ptr,
                  K._stream(dev))
        torch.cuda.synchronize()
        T.check(f"eggroll_lora_project r={r} ldx={ld}")
        out.append(T.bits())
    assert torch.equal(out[0], out[1])
    xs, A = c["x"].double().cpu().numpy(), tp[:, 4:4 + r * Kd].view(-1, r, Kd).double().cpu().numpy()
    ref = np.concatenate([xs[k * rpm:(k + 1) * rpm] @ A[k].T for k in range(A.shape[0])])
    np.testing.assert_allclose(out[0].view(torch.float32).cpu().numpy(), ref, rtol=1e-4, atol=1e-3)


def test_project_multi_padded_x(dev):
    """eggroll_lora_project_multi (3 linears, r = 2) over X with ldx = K + 8 in NaN padding == the packed call."""
    c = _case("S1", 2)
    M, Kd, rpm, r, n_lin = c["M"], c["Kd"], c["rpm"], 2, 3
    tp = (torch.randn(-(-M // rpm), n_lin * r * Kd + 4, generator=torch.Generator().manual_seed(5)) * 0.1).to(dev)
    offs = np.asarray([4 + l * r * Kd for l in range(n_lin)], dtype=np.int64)
    out = []
    for ld, off in ((Kd, 0), (Kd + 8, 8)):
        X = _Buf(dev, torch.bfloat16, M, Kd, ld, off, data=c["x"], poison="nan")
        T = _Buf(dev, torch.float32, n_lin * M, r, r, 4)
        _lib.call("eggroll_lora_project_multi", X.ptr, X.ld, tp.data_ptr(), tp.stride(0), offs.ctypes.data, n_lin, r,
                  rpm, M, Kd, T.ptr, K._stream(dev))
        torch.cuda.synchronize()
        T.check(f"eggroll_lora_project_multi ldx={ld}")
        out.append(T.bits())
    assert torch.equal(out[0], out[1])
    single = torch.stack([K.lora_project(c["x"], tp, int(o), r, rpm) for o in offs]).view(n_lin * M, r)
    np.testing.assert_allclose(out[0].view(torch.float32).cpu().numpy(), single.cpu().numpy(), rtol=1e-4, atol=1e-3)


def test_expand_unaligned_y(dev):
    """eggroll_lora_expand into a Y with ldy = N + 5, 3 elements into its buffer == the packed call; the padding
    is left alone."""
    c = _case("S1", 2)
    M, N, r, rpm = c["M"], c["N"], c["r"], c["rpm"]
    base = _run(c, "L0", "gemm", 8)["y"].view(torch.bfloat16)
    out = []
    for ld, off in ((N, 0), (N + 5, 3)):
        Y = _Buf(dev, torch.bfloat16, M, N, ld, off, data=base)
        _lib.call("eggroll_lora_expand", c["T"].data_ptr(), c["tp"].data_ptr(), c["tp"].stride(0), c["offB"], r, 4.0,
                  rpm, M, N, Y.ptr, Y.ld, K._stream(dev))
        torch.cuda.synchronize()
        Y.check(f"eggroll_lora_expand ldy={ld}")
        out.append(Y.bits())
    assert torch.equal(out[0], out[1])
    assert not torch.equal(out[0], base.view(torch.int16))


# ---------------------------------------------------------------------------------- 4. refusals
def _good_args(c, api, epi, bufs):
    """Keyword arguments of a call that would be accepted (S1, r = 2, kernel 8), on packed operands."""
    M, N, Kd = c["M"], c["N"], c["Kd"]
    a = dict(X=c["x"].data_ptr(), ldx=Kd, W=c["W"].data_ptr(), ldw=Kd, bias=c["b"].data_ptr(), T=c["T"].data_ptr(),
             theta_pop=c["tp"].data_ptr(), ld_theta=c["tp"].stride(0), offA=c["offA"], offB=c["offB"], r=c["r"],
             scale=c["scale"], rpm=c["rpm"], M=M, N=N, K=Kd, Y=bufs["y"].ptr, ldy=N, T_ws=bufs["ws"].ptr, kernel=8,
             stream=K._stream(c["x"].device))
    if epi:
        f32 = epi in ("res32", "gated32")
        a.update(epi=K.EPI[epi], res=bufs["res32" if f32 else "y"].ptr if epi not in ("silu", "gelu", "gelu_erf") else None,
                 ldr=N, gate=c["gate32" if f32 else "gate16"].data_ptr() if "gated" in epi else None, gstride=N,
                 rpg=RPG)
    return a


ORDER = {
    "eggroll_lora_linear_pop_sel": "X ldx W ldw bias theta_pop ld_theta offA offB r scale rpm M N K Y ldy T_ws kernel stream",
    "eggroll_lora_gemm_sel": "X ldx W ldw bias T theta_pop ld_theta offB r scale rpm M N K Y ldy kernel stream",
    "eggroll_lora_linear_pop_epi_sel": "X ldx W ldw bias theta_pop ld_theta offA offB r scale rpm M N K Y ldy T_ws epi res "
                                       "ldr gate gstride rpg kernel stream",
    "eggroll_lora_gemm_epi_sel": "X ldx W ldw bias T theta_pop ld_theta offB r scale rpm M N K Y ldy epi res ldr gate "
                                 "gstride rpg kernel stream",
}
PLAIN_EP = ("eggroll_lora_linear_pop_sel", "eggroll_lora_gemm_sel")
EPI_EP = ("eggroll_lora_linear_pop_epi_sel", "eggroll_lora_gemm_epi_sel")
# (id, entry points, epilogue op of the _epi_ entry points, overrides of the accepted call)
REFUSED = [
    ("ldx%8", PLAIN_EP + EPI_EP, "silu", dict(ldx=S1["Kd"] + 4)),
    ("ldw%8", PLAIN_EP + EPI_EP, "silu", dict(ldw=S1["Kd"] + 4)),
    ("ldx<K", PLAIN_EP + EPI_EP, "silu", dict(ldx=S1["Kd"] - 8)),
    ("ldw<K", PLAIN_EP + EPI_EP, "silu", dict(ldw=S1["Kd"] - 8)),
    ("ldy<N", PLAIN_EP + EPI_EP, "silu", dict(ldy=S1["N"] - 1)),
    ("ldr<N-res", EPI_EP, "res", dict(ldr=S1["N"] - 1)),
    ("ldr<N-res32", EPI_EP, "res32", dict(ldr=S1["N"] - 1)),
    ("gstride<N-gated", EPI_EP, "gated", dict(gstride=S1["N"] - 1)),
    ("gstride<N-gated32", EPI_EP, "gated32", dict(gstride=S1["N"] - 1)),
    ("rpg=0-gated", EPI_EP, "gated", dict(rpg=0)),
    ("rpg=0-gated32", EPI_EP, "gated32", dict(rpg=0)),
    ("K=96", PLAIN_EP + EPI_EP, "silu", dict(K=96, ldx=96, ldw=96)),
    ("kernel=7", PLAIN_EP + EPI_EP, "silu", dict(kernel=7)),
    ("kernel=12", PLAIN_EP + EPI_EP, "silu", dict(kernel=12)),     # the removed fused-projection kernel
    ("kernel=256", PLAIN_EP + EPI_EP, "silu", dict(kernel=256)),   # the removed 256x256 one-barrier tile
    ("kernel=9-epi", EPI_EP, "silu", dict(kernel=9)),
    ("r=3-epi", EPI_EP, "silu", dict(r=3)),
    ("r=2-rpm=255-epi", EPI_EP, "silu", dict(rpm=255)),
    ("kernel=10-r=4-epi", EPI_EP, "silu", dict(kernel=10, r=4)),
    ("r=17", PLAIN_EP + EPI_EP, "silu", dict(r=17)),
    ("res=NULL-res", EPI_EP, "res", dict(res=None)),
]
REFUSED_FLAT = [(i, ep, e, o) for i, eps, e, o in REFUSED for ep in eps]


def _refusal_bufs(c, dev):
    M, N, r = c["M"], c["N"], c["r"]
    return dict(y=_Buf(dev, torch.bfloat16, M, N, N, 0), res32=_Buf(dev, torch.float32, M, N, N, 0),
                ws=_Buf(dev, torch.float32, M, r, r, 0))   # the projection workspace T_ws


@pytest.mark.parametrize("case,entry,epi,over", REFUSED_FLAT, ids=[f"{i}-{ep[8:]}" for i, ep, _, _ in REFUSED_FLAT])
def test_refusals(dev, case, entry, epi, over):
    """A call the header forbids returns an error naming its entry point and launches nothing: Y, the fp32
    stream and the projection workspace still hold the poison, all of it, after a device synchronize."""
    c = _case("S1", 2)
    bufs = _refusal_bufs(c, dev)
    a = _good_args(c, entry, epi if "_epi_" in entry else None, bufs)
    a.update(over)
    rc = getattr(_lib.load(), entry)(*[a[k] for k in ORDER[entry].split()])
    msg = _lib.load().eggroll_last_error().decode()
    torch.cuda.synchronize()
    assert rc != 0, f"{entry} accepted {over}"
    short = entry[len("eggroll_"):-len("_sel")]
    assert re.match(rf"{short}(_sel)?: ", msg), f"{entry} refused {over} with {msg!r}: the entry point is not named"
    for k, b in bufs.items():
        b.check(f"{entry} {case} [{k}]", written=False)


@pytest.mark.parametrize("entry", PLAIN_EP + EPI_EP, ids=[e[8:] for e in PLAIN_EP + EPI_EP])
def test_empty_m_is_ok_and_writes_nothing(dev, entry):
    c = _case("S1", 2)
    bufs = _refusal_bufs(c, dev)
    a = _good_args(c, entry, "gated32" if "_epi_" in entry else None, bufs)
    a.update(M=0)
    _lib.call(entry, *[a[k] for k in ORDER[entry].split()])
    torch.cuda.synchronize()
    for k, b in bufs.items():
        b.check(f"{entry} M=0 [{k}]", written=False)


def test_accepted_call_of_the_refusal_template(dev):
    """The call every refusal case perturbs is itself accepted and correct (so each refusal is due to its one
    override), through all four entry points."""
    c = _case("S1", 2)
    want = _run(c, "L0", "gemm", 8)["y"]
    for entry in PLAIN_EP + EPI_EP:
        bufs = _refusal_bufs(c, c["x"].device)
        epi = "res32" if "_epi_" in entry else None
        a = _good_args(c, entry, epi, bufs)
        if epi:
            bufs["res32"].view.zero_()
        _lib.call(entry, *[a[k] for k in ORDER[entry].split()])
        torch.cuda.synchronize()
        bufs["y"].check(entry)
        assert torch.equal(bufs["y"].bits(), want), entry   # 0 + y, rounded to bf16, is y


# ---------------------------------------------------------------------------------- 5. the Python wrappers
def _wrapper_calls(c):
    x, W, b, tp, T = c["x"], c["W"], c["b"], c["tp"], c["T"]
    common = (c["r"], c["scale"], c["rpm"])
    return {
        "lora_linear_pop": lambda out: K.lora_linear_pop(x, W, b, tp, c["offA"], c["offB"], *common, out=out, kernel=8),
        "lora_gemm": lambda out: K.lora_gemm(x, W, b, T, tp, c["offB"], *common, out=out, kernel=8),
        "lora_linear_pop_epi": lambda out: K.lora_linear_pop_epi(x, W, b, tp, c["offA"], c["offB"], *common, "silu",
                                                                 out=out, kernel=8),
        "lora_gemm_epi": lambda out: K.lora_gemm_epi(x, W, b, T, tp, c["offB"], *common, "silu", out=out, kernel=8),
    }


@pytest.mark.parametrize("wrapper", ["lora_linear_pop", "lora_gemm", "lora_linear_pop_epi", "lora_gemm_epi"])
def test_wrappers_honour_out_stride(dev, wrapper):
    """A caller's `out` that is a column slice of a wider bf16 buffer is written through its row stride: the
    result equals the packed call and the rest of the buffer is untouched.  A wrong dtype or a non-unit inner
    stride raises EggrollError (nothing is reinterpreted)."""
    c = _case("S1", 2)
    M, N = c["M"], c["N"]
    call = _wrapper_calls(c)[wrapper]
    packed = call(None)
    wide = _Buf(dev, torch.bfloat16, M, N, N + 24, 5)      # rows of N + 24, the slice starts at column 5
    got = call(wide.view)
    torch.cuda.synchronize()
    assert got is wide.view
    wide.check(wrapper)
    assert torch.equal(wide.bits(), packed.view(torch.int16))
    for bad in (torch.empty((M, N), dtype=torch.float16, device=dev), torch.empty((M, N), dtype=torch.float32, device=dev),
                torch.empty((N, M), dtype=torch.bfloat16, device=dev).t(),
                torch.empty((M, 2 * N), dtype=torch.bfloat16, device=dev)[:, ::2][:, :N],
                torch.empty((M, N + 8), dtype=torch.bfloat16, device=dev)):
        with pytest.raises(_lib.EggrollError):
            call(bad)


def test_epi_wrapper_fp32_stream_shadow_stride(dev):
    """The fp32-stream ops' bf16 shadow `out` is honoured the same way."""
    c = _case("S1", 2)
    M, N = c["M"], c["N"]
    args = (c["x"], c["W"], c["b"], c["tp"], c["offA"], c["offB"], c["r"], c["scale"], c["rpm"], "res32")
    s0, sh0 = c["res32"].clone(), torch.empty((M, N), dtype=torch.bfloat16, device=dev)
    K.lora_linear_pop_epi(*args, res=s0, out=sh0, kernel=8)
    s1, wide = c["res32"].clone(), _Buf(dev, torch.bfloat16, M, N, N + 24, 5)
    K.lora_linear_pop_epi(*args, res=s1, out=wide.view, kernel=8)
    torch.cuda.synchronize()
    wide.check("lora_linear_pop_epi(res32, out=slice)")
    assert torch.equal(s0, s1) and torch.equal(wide.bits(), sh0.view(torch.int16))
