"""The halo conv's wide class (include/eggroll.h): 3x3 px-1 convs at the VAR / Infinity VAE widths 160, 320, 640,
whose last column tile is partial.  Parity against torch fp32 on the same bf16 operands, no write outside the
output, bitwise repeatability, and the refusals of everything outside the old and the new class.

The tile of a case follows the header's rule: 512 x 128 (BN 128) needs W % 32 == 0, 256 x 256 (BN 256)
W % 16 == 0; the smaller padded width ceil(N / BN) * BN wins, a tie goes to 256 x 256.
"""
import math

import pytest
import torch

from hyperscalees_t2i_amd import _lib
from hyperscalees_t2i_amd import kernels as K

pytestmark = pytest.mark.gpu

# B, H, W, Cin, N, bias, act, BN of the tile the header's rule gives (checked against the Python mirror of the rule)
CASES = {
    # N 160 pads to 256 under either tile, the tie goes to 256 x 256: one column tile whose third wave column
    # (128..191) ends at 160 and whose fourth is empty; two images, 2 x 2 pixel tiles each (interior borders)
    "160_32x32_b2_bias_silu": (2, 32, 32, 160, 160, True, "silu", 256),
    # VAR's 16 x 16 map: W % 32 != 0 leaves 256 x 256 only; 640 = 2.5 tiles, the last half empty; 20 slices
    "640_16x16": (1, 16, 16, 640, 640, False, None, 256),
    # W % 32 == 0 and 640 = 5 x 128 < 768: five exact 512 x 128 column tiles (the full-tile kernel)
    "640_32x64": (1, 32, 64, 640, 640, False, None, 128),
    # 320 pads to 384 on 512 x 128 (83 %) against 512: three column tiles, the last with its second wave empty
    "320_32x64": (1, 32, 64, 320, 320, False, None, 128),
    # ResnetBlock conv1 at a width change.  W = 48: 256 x 256 only, 320 in two tiles
    "160to320_48x48_bias": (1, 48, 48, 160, 320, True, None, 256),
    # 160 out: the 256-wide tie again, ten slices in
    "320to160_16x32_bias": (1, 16, 32, 320, 160, True, None, 256),
    # three slices (odd); N 32 pads to 128 on 512 x 128: half of wave column 0, wave column 1 wholly empty
    "96to32_16x32_b2": (2, 16, 32, 96, 32, False, None, 128),
    # one slice: the sweep is its LAST form alone
    "32to160_16x32": (1, 16, 32, 32, 160, False, None, 256),
}


def _operands(dev, B, H, W, Cin, N, bias):
    g = torch.Generator().manual_seed(B * 100 + H + Cin + N)
    x = torch.randn(B, H, W, Cin, generator=g).to(dev, torch.bfloat16)
    w = (torch.randn(N, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin)).to(dev, torch.bfloat16)
    b = (torch.randn(N, generator=g) * 0.5).to(dev, torch.bfloat16) if bias else None
    return x, w, b


def _reference(x, w, b, act):
    ref = torch.nn.functional.conv2d(x.permute(0, 3, 1, 2).float(), w.float(), None if b is None else b.float(),
                                     padding=1)
    if act == "silu":
        ref = torch.nn.functional.silu(ref)
    return ref.permute(0, 2, 3, 1)


@pytest.mark.parametrize("case", list(CASES))
def test_conv_wide_vs_torch(dev, case):
    """Every case of the table above, under auto dispatch, within the project's conv bound
    |d| <= 2^-8 |y| + 1e-3 max|y| of torch fp32 on the same bf16 operands (test_conv3x3_halo_vs_torch's); the
    explicit halo selector (kernel 2) gives the same bits."""
    B, H, W, Cin, N, bias, act, bn = CASES[case]
    assert K.conv_halo_wide_tile(Cin, N, H, W, B) == bn
    x, w, b = _operands(dev, B, H, W, Cin, N, bias)
    wp = K.pack_conv3x3_weight(w, 1)
    y = K.conv3x3_nhwc(x, wp, b, 1, act)
    ref = _reference(x, w, b, act)
    err = (y.float() - ref).abs()
    tol = 2.0 ** -8 * ref.abs() + 1e-3 * ref.abs().max()
    print(f"[conv wide {case}] max err {err.max().item():.3e}  ref max {ref.abs().max().item():.3e}")
    assert bool((err <= tol).all()), f"max err {err.max().item():.3e} (ref max {ref.abs().max().item():.3e})"
    assert torch.equal(y, K.conv3x3_nhwc(x, wp, b, 1, act, kernel=2))


@pytest.mark.parametrize("case", ["160_32x32_b2_bias_silu", "96to32_16x32_b2"])
def test_conv_wide_writes_inside_output_only(dev, case):
    """A tail case on each tile (256 x 256 at N 160, 512 x 128 at N 32) into a view of a larger buffer: the 96
    sentinel elements ahead of the output and the 96 behind it keep their value, and the view holds the result."""
    B, H, W, Cin, N, bias, act, _ = CASES[case]
    x, w, b = _operands(dev, B, H, W, Cin, N, bias)
    wp = K.pack_conv3x3_weight(w, 1)
    n, guard = B * H * W * N, 96
    buf = torch.full((n + 2 * guard,), 7.0, device=dev, dtype=torch.bfloat16)
    out = buf[guard:guard + n].view(B, H, W, N)
    K.conv3x3_nhwc(x, wp, b, 1, act, out=out)
    torch.cuda.synchronize()
    assert bool((buf[:guard] == 7.0).all()) and bool((buf[guard + n:] == 7.0).all())
    assert torch.equal(out, K.conv3x3_nhwc(x, wp, b, 1, act))


@pytest.mark.parametrize("case", ["640_16x16", "320_32x64"])
def test_conv_wide_bitwise_run_to_run(dev, case):
    B, H, W, Cin, N, bias, act, _ = CASES[case]
    x, w, b = _operands(dev, B, H, W, Cin, N, bias)
    wp = K.pack_conv3x3_weight(w, 1)
    y0 = K.conv3x3_nhwc(x, wp, b, 1, act)
    for _ in range(3):
        assert torch.equal(y0, K.conv3x3_nhwc(x, wp, b, 1, act))


@pytest.mark.parametrize("H,W,Cin,N,kernel", [
    (16, 16, 160, 24, 0),     # N % 32 != 0
    (16, 16, 80, 160, 0),     # Cin % 32 != 0
    (24, 16, 160, 160, 0),    # H % 16 != 0
    (16, 16, 160, 160, 1),    # the tap-staged kernel has no form for the class
    (16, 16, 160, 160, 3),    # removed selector values stay refused
    (16, 16, 160, 160, 4),
], ids=["N24", "Cin80", "H24", "kernel1", "kernel3", "kernel4"])
def test_conv_wide_refusals_launch_nothing(dev, H, W, Cin, N, kernel):
    x = torch.ones(1, H, W, Cin, device=dev, dtype=torch.bfloat16)
    wp = K.pack_conv3x3_weight(torch.ones(N, Cin, 3, 3, device=dev, dtype=torch.bfloat16), 1)
    buf = torch.full((1, H, W, N), 7.0, device=dev, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):
        K.conv3x3_nhwc(x, wp, None, 1, out=buf, kernel=kernel)
    torch.cuda.synchronize()
    assert bool((buf == 7.0).all())


def test_conv_wide_rmsnorm_entry_keeps_its_rule(dev):
    """conv3x3_rmsnorm_nhwc at N = 160 is refused as before (whole pixels per tile: N 128 or 256): by the wrapper,
    and by the library's own entry point with the output's sentinel intact, under auto and the halo selector."""
    x = torch.ones(1, 16, 16, 160, device=dev, dtype=torch.bfloat16)
    wp = K.pack_conv3x3_weight(torch.ones(160, 160, 3, 3, device=dev, dtype=torch.bfloat16), 1)
    nw = torch.ones(160, device=dev, dtype=torch.bfloat16)
    res = torch.zeros(1, 16, 16, 160, device=dev, dtype=torch.bfloat16)
    buf = torch.full((1, 16, 16, 160), 7.0, device=dev, dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        K.conv3x3_rmsnorm_nhwc(x, wp, None, 1, 1e-5, nw, None, res)
    for k in (0, 2):
        with pytest.raises(RuntimeError):
            _lib.call("eggroll_conv3x3_rmsnorm_nhwc_sel", x.data_ptr(), wp.data_ptr(), None, 1, 16, 16, 160, 160, 1,
                      1e-5, nw.data_ptr(), None, res.data_ptr(), buf.data_ptr(), k, None)
    torch.cuda.synchronize()
    assert bool((buf == 7.0).all())
