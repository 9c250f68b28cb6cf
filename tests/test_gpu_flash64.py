"""eggroll_flash_attention at head dim 64 (VAR's attention over its KV cache): accuracy against fp32 SDPA on the
same bf16 inputs, bitwise independence of batch entries and of the cache rows behind Lk, and the host checks.

Bars: the project's for this algorithm (test_flash_attention_vs_sdpa): relative Frobenius error < 1e-2 and
max |d| < 0.05.  A CPU emulation of the algorithm alone (64-key blocks, online softmax, P rounded to bf16, fp32
accumulation, bf16 output) on these inputs gives <= 2.4e-3 and <= 9e-3.
"""
import pytest
import torch
import torch.nn.functional as F

from hyperscalees_t2i_amd import _lib
from hyperscalees_t2i_amd import kernels as K

pytestmark = pytest.mark.gpu

HD = 64
# (B, Nq, Lk, H, cache slice, qf)
CASES = [(3, 1, 1, 2, False, 0),        # VAR's first scale: one query, one key
         (2, 4, 5, 3, True, 0),         # second scale: fewer keys than one MFMA fragment, odd head count
         (4, 64, 64, 2, False, 0),      # exactly one block
         (1, 257, 130, 1, True, 1),     # ragged query block at each qf
         (1, 257, 130, 1, True, 4),
         (2, 100, 200, 2, False, 0),    # each qf
         (2, 100, 200, 2, False, 1),
         (2, 100, 200, 2, False, 4),
         (2, 100, 2521, 2, True, 0),    # many key blocks, partial last
         (2, 256, 680, 16, True, 0)]    # VAR-d16's last scale: cache [2, B, 680 + 37, 1024]
RECIPES = ("randn", "unit4", "unit100")


def _inputs(dev, B, Nq, Lk, H, cache_slice, recipe, pad=37):
    """randn: the recipe of test_flash_attention_vs_sdpa (q, k ~ 0.3 N(0,1), v ~ N(0,1), scale 64^-0.5 * 3).
    unit4 / unit100: VAR's own distribution, q and k unit-norm per head, q times the initial scale_mul 4 or its
    clamp 100 (a near-one-hot softmax), scale 1."""
    g = torch.Generator(device=dev).manual_seed(Nq * 7 + Lk)
    q = torch.randn(B, Nq, H, HD, generator=g, device=dev)
    k = torch.randn(B, Lk + pad, H, HD, generator=g, device=dev)
    v = torch.randn(B, Lk + pad, H, HD, generator=g, device=dev)
    if recipe == "randn":
        q, k, scale = q * 0.3, k * 0.3, HD ** -0.5 * 3
    else:
        q = F.normalize(q, dim=-1) * float(recipe[4:])
        k, scale = F.normalize(k, dim=-1), 1.0
    q = q.bfloat16()
    if cache_slice:
        cache = torch.stack((k, v)).bfloat16().view(2, B, Lk + pad, H * HD)
        k, v = (cache[i, :, :Lk].view(B, Lk, H, HD) for i in (0, 1))
    else:
        k, v = k[:, :Lk].bfloat16().contiguous(), v[:, :Lk].bfloat16().contiguous()
    return q, k, v, scale


def _sdpa32(q, k, v, scale):
    return F.scaled_dot_product_attention(q.float().transpose(1, 2), k.float().transpose(1, 2),
                                          v.float().transpose(1, 2), scale=scale).transpose(1, 2)


@pytest.mark.parametrize("recipe", RECIPES)
@pytest.mark.parametrize("B,Nq,Lk,H,cache_slice,qf", CASES, ids=["-".join(str(x) for x in c) for c in CASES])
def test_flash64_vs_sdpa(dev, B, Nq, Lk, H, cache_slice, qf, recipe):
    q, k, v, scale = _inputs(dev, B, Nq, Lk, H, cache_slice, recipe)
    got = K.flash_attention(q, k, v, scale, qf=qf)
    assert got.shape == (B, Nq, H, HD) and got.dtype == torch.bfloat16
    got = got.float()
    ref = _sdpa32(q, k, v, scale)
    err = ((got - ref).norm() / ref.norm()).item()
    mx = (got - ref).abs().max().item()
    print(f"flash64 {(B, Nq, Lk, H, cache_slice, qf)} {recipe}: rel {err:.3e} max {mx:.3e}")
    assert err < 1e-2, err
    assert mx < 0.05, mx


@pytest.mark.parametrize("qf", (0, 1, 4))
def test_flash64_batch_entries_independent(dev, qf):
    """A B = 5 call equals five B = 1 calls on the slices, bitwise."""
    q, k, v, scale = _inputs(dev, 5, 100, 200, 2, True, "unit4")
    whole = K.flash_attention(q, k, v, scale, qf=qf)
    for b in range(5):
        one = K.flash_attention(q[b:b + 1], k[b:b + 1], v[b:b + 1], scale, qf=qf)
        assert torch.equal(whole[b:b + 1], one), b


@pytest.mark.parametrize("Nq,Lk", [(1, 1), (4, 5), (64, 64), (100, 130)])
def test_flash64_cache_rows_past_lk_are_not_used(dev, Nq, Lk):
    """The product's cache is torch.empty: with every row behind Lk holding NaN bit patterns the output is finite
    and bitwise the clean run's."""
    B, H = 2, 3
    q, k, v, scale = _inputs(dev, B, Nq, Lk, H, True, "unit4")
    clean = K.flash_attention(q, k, v, scale)
    for bits in (0x7FC0, -1):   # a quiet NaN; 0xFFFF as int16
        cache = torch.full((2, B, Lk + 37, H * HD), bits, dtype=torch.int16, device=dev).view(torch.bfloat16)
        assert torch.isnan(cache).all()
        cache[0, :, :Lk] = k.reshape(B, Lk, H * HD)
        cache[1, :, :Lk] = v.reshape(B, Lk, H * HD)
        got = K.flash_attention(q, cache[0, :, :Lk].view(B, Lk, H, HD), cache[1, :, :Lk].view(B, Lk, H, HD), scale)
        assert torch.isfinite(got).all()
        assert torch.equal(got, clean)


def test_flash64_refuses_other_head_dims_and_strides(dev):
    """Head dim 96 is refused with a message naming 64 and 128, a row stride that is no multiple of 8 is refused,
    and in both cases a poisoned output is untouched."""
    B, N, H = 2, 20, 2
    g = torch.Generator(device=dev).manual_seed(0)
    q96, k96, v96 = (torch.randn(B, N, H, 96, generator=g, device=dev).bfloat16() for _ in range(3))
    out = torch.full((B, N, H, 96), 7.0, dtype=torch.bfloat16, device=dev)
    with pytest.raises(_lib.EggrollError, match=r"head_dim 96 unsupported \(64, 128\)"):
        K.flash_attention(q96, k96, v96, 1.0, out=out)
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    buf = torch.randn(B, N, H * HD + 4, generator=g, device=dev).bfloat16()
    q = buf[:, :, :H * HD].unflatten(2, (H, HD))
    assert q.stride(1) == H * HD + 4 and q.stride(2) == HD
    k, v = (torch.randn(B, N, H, HD, generator=g, device=dev).bfloat16() for _ in range(2))
    out = torch.full((B, N, H, HD), 7.0, dtype=torch.bfloat16, device=dev)
    with pytest.raises(_lib.EggrollError, match="bad strides"):
        K.flash_attention(q, k, v, 1.0, out=out)
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    assert torch.isfinite(K.flash_attention(q.contiguous(), k, v, 1.0)).all()   # the same data, strides in order
