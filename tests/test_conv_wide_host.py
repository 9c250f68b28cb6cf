"""Host side of the halo conv's wide class: the Python eligibility helpers against the rule stated in
include/eggroll.h, and conv_nhwc's own argument checks, which still come before any library call."""
import pytest
import torch

from hyperscalees_t2i_amd import _lib
from hyperscalees_t2i_amd import kernels as K
from hyperscalees_t2i_amd.dcae import CONV_HALO_WIDE_KEEP_PARENT, conv_gemm_px, conv_halo_wide_ok


def _rule(cin, n, H, W):
    """The header's words, restated independently: the class, then the tile with the least padded width."""
    classic = cin >= 64 and cin & (cin - 1) == 0 and cin <= 2048 and n % 64 == 0 and 64 <= n <= 8192
    in_class = (not classic and H % 16 == 0 and 32 <= cin <= 2048 and cin % 32 == 0 and 32 <= n <= 8192 and n % 32 == 0)
    tiles = [bn for bn, tw in ((256, 16), (128, 32)) if W % tw == 0]     # 256 first: it wins a tie
    if not in_class or not tiles:
        return 0
    return min(tiles, key=lambda bn: -(-n // bn) * bn)


# cin, n, H, W -> BN of the tile (0: outside the class)
TABLE = [
    ((640, 640, 16, 16), 256),    # W % 32 != 0: 256 x 256 only (768 columns)
    ((640, 640, 32, 32), 128),    # five exact 128-wide tiles
    ((320, 320, 64, 64), 128),    # 384 < 512
    ((160, 160, 128, 128), 256),  # 256 either way: the tie goes to 256 x 256
    ((160, 160, 256, 256), 256),
    ((320, 160, 128, 128), 256),
    ((640, 320, 32, 32), 128),
    ((160, 320, 48, 48), 256),
    ((96, 32, 16, 32), 128),
    ((32, 160, 16, 32), 256),
    ((32, 640, 16, 16), 256),
    ((2048, 8192, 16, 16), 0),    # classic channel counts stay where they were
    ((128, 128, 16, 32), 0),
    ((512, 512, 16, 16), 0),
    ((256, 320, 16, 16), 0),      # classic: the tap-staged kernel's own N tail
    ((64, 32, 16, 16), 256),      # N below 64 is not classic
    ((160, 24, 16, 16), 0),       # N % 32
    ((80, 160, 16, 16), 0),       # Cin % 32
    ((160, 160, 24, 16), 0),      # H % 16
    ((160, 160, 16, 24), 0),      # W % 16
    ((160, 160, 16, 8), 0),
    ((2080, 160, 16, 16), 0),     # Cin above 2048
    ((160, 8224, 16, 16), 0),     # N above 8192
    ((0, 160, 16, 16), 0),
]


@pytest.mark.parametrize("shape,bn", TABLE)
def test_conv_halo_wide_tile_follows_the_header_rule(shape, bn):
    assert _rule(*shape) == bn                       # the table agrees with the rule as the header words it
    assert K.conv_halo_wide_tile(*shape) == bn
    want = bn != 0 and shape not in CONV_HALO_WIDE_KEEP_PARENT
    assert conv_halo_wide_ok(*shape) is want
    if conv_gemm_px(shape[0]) and shape[1] % 64 == 0 and shape[1] <= 8192:
        assert bn == 0                               # a width the hosts already route never changes route


def test_conv_halo_wide_tile_sweep_matches_rule():
    for cin in (32, 64, 96, 128, 160, 320, 640, 1024, 2048, 2080):
        for n in (24, 32, 64, 96, 128, 160, 256, 320, 384, 640):
            for H, W in ((16, 16), (16, 32), (32, 48), (8, 32), (16, 40)):
                assert K.conv_halo_wide_tile(cin, n, H, W) == _rule(cin, n, H, W), (cin, n, H, W)


def test_conv_nhwc_wrapper_argument_checks(monkeypatch):
    """Mismatched packed weights / bias raise ValueError, host tensors RuntimeError, before any library call."""
    x = torch.zeros(1, 16, 16, 160, dtype=torch.bfloat16)
    w = torch.zeros(160, 9 * 160, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        K.conv_nhwc(x, w, None, 3)
    monkeypatch.setattr(K, "_dev", lambda t, *a, **k: t)
    monkeypatch.setattr(_lib, "call", lambda *a, **k: pytest.fail("the library was called"))
    with pytest.raises(ValueError, match="packed weight"):
        K.conv_nhwc(x, torch.zeros(160, 9 * 128, dtype=torch.bfloat16), None, 3)     # packed for another Cin
    with pytest.raises(ValueError, match="packed weight"):
        K.conv_nhwc(x, w, None, 2)                                                   # packed for another ks
    with pytest.raises(ValueError, match="bias"):
        K.conv_nhwc(x, w, torch.zeros(128, dtype=torch.bfloat16), 3)
    with pytest.raises(RuntimeError, match="halo kernel only"):
        K.conv_nhwc(x, w, None, 3, kernel=1)                                         # the wide class has no kernel 1
