"""The core the prompt encoders share (text_encoder.py), the parts that need no GPU: the F.linear path of
`linear` with every epilogue, and the RoPE tables behind gemma2.rope_tables / qwen3.rope_tables."""
import pytest
import torch
import torch.nn.functional as F

from hyperscalees_t2i_amd import gemma2, qwen3
from hyperscalees_t2i_amd import text_encoder as TE


def test_linear_fallback_epilogues():
    """W [8, 40]: K = 40 is outside the GEMM's shape rule, so every call takes the F.linear path; each epilogue
    against its literal formula (the same torch ops on the CPU: exact)."""
    g = torch.Generator().manual_seed(0)
    x = torch.randn(3, 40, generator=g).to(torch.bfloat16)
    W = torch.randn(8, 40, generator=g).to(torch.bfloat16)
    assert not TE.gemm_ok(W) and TE.gemm_ok(torch.zeros(8, 64))
    y = F.linear(x, W)
    assert torch.equal(TE.linear(x, W), y)
    assert torch.equal(TE.linear(x, W, "silu"), F.silu(y))
    assert torch.equal(TE.linear(x, W, "gelu"), F.gelu(y, approximate="tanh"))
    gate = torch.randn(3, 8, generator=g).to(torch.bfloat16)
    res = gate.clone()
    out = TE.linear(x, W, "mul", res=res)
    assert out is res and torch.equal(res, gate * y)                       # in place, bf16
    stream = torch.randn(3, 8, generator=g)
    res = stream.clone()
    out = TE.linear(x, W, "res32", res=res)
    assert out is res and res.dtype == torch.float32 and torch.equal(res, stream + y.float())   # in place, fp32
    with pytest.raises(ValueError):
        TE.linear(x, W, "relu")


def test_rope_tables_are_the_shared_ones():
    for mod, hd, theta in ((gemma2, 256, 10000.0), (qwen3, 128, 1e6)):
        cos, sin = mod.rope_tables(5)
        ref_cos, ref_sin = TE.rope_tables(5, hd, theta)
        assert cos.shape == sin.shape == (5, hd // 2) and cos.dtype == sin.dtype == torch.float32
        assert torch.equal(cos, ref_cos) and torch.equal(sin, ref_sin)
