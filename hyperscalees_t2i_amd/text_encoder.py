"""What the prompt encoders (t5.py, gemma2.py, qwen3.py) share: parameter constructors, the r = 0 GEMM with its
epilogues, the rotate-half RoPE tables, the random fill of init_weights and the batch trimming that opens
every forward.  The architectures, blocks and forward bodies stay in their own modules."""
from __future__ import annotations

from typing import Optional, Tuple

import torch
import torch.nn.functional as F
from torch import nn

from . import kernels as K


def _w(*shape) -> nn.Parameter:
    return nn.Parameter(torch.zeros(*shape, dtype=torch.bfloat16), requires_grad=False)


def _nw(C: int) -> nn.Parameter:
    return nn.Parameter(torch.zeros(1, C, dtype=torch.float32), requires_grad=False)


def gemm_ok(W: torch.Tensor) -> bool:
    """The r = 0 MFMA GEMM's shape rule (eggroll_lora_gemm: K % 64 == 0; 16-byte output rows)."""
    return W.shape[1] % 64 == 0 and W.shape[0] % 8 == 0


def linear(x: torch.Tensor, W: torch.Tensor, epi: Optional[str] = None, res: Optional[torch.Tensor] = None):
    """x [M, K] bf16 @ W^T with the op that follows it: None, "silu", "gelu" (tanh), "mul" (res *= y, bf16),
    "res32" (res += y, the fp32 stream).  On the library's GEMM where its shape rule admits W, else F.linear
    and the same op."""
    M = x.shape[0]
    if gemm_ok(W):
        if epi is None:
            return K.lora_linear_pop(x, W, None, None, 0, 0, 0, 0.0, M)
        return K.lora_linear_pop_epi(x, W, None, None, 0, 0, 0, 0.0, M, epi, res=res)
    y = F.linear(x, W)
    if epi is None:
        return y
    if epi == "silu":
        return F.silu(y)
    if epi == "gelu":
        return F.gelu(y, approximate="tanh")
    if epi == "mul":
        return res.mul_(y)
    if epi == "res32":
        return res.add_(y)
    raise ValueError(f"text_encoder.linear: epi {epi!r} unsupported")


def rope_tables(N: int, head_dim: int, theta: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """transformers' rotary embedding (Gemma2RotaryEmbedding, Qwen3RotaryEmbedding: default rope type, attention
    scaling 1) restated for positions 0..N-1: fp32 CPU cos, sin [N, head_dim / 2] — transformers' [N, head_dim]
    table is this one twice, side by side."""
    inv_freq = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.int64).float() / head_dim))
    freqs = torch.arange(N, dtype=torch.int64).float()[:, None] * inv_freq[None, :]
    return freqs.cos().contiguous(), freqs.sin().contiguous()


def fill(p: torch.Tensor, std: float, generator: torch.Generator) -> None:
    """p <- N(0, std^2), drawn on the generator's device in chunks of 65536 rows: no fp32 copy of a whole matrix."""
    for r in range(0, p.shape[0], 65536):
        q = p[r:r + 65536]
        q.copy_((torch.randn(q.shape, generator=generator, device=generator.device) * std).to(p.dtype))


def trim_batch(name: str, input_ids: torch.Tensor, lens: torch.Tensor, device) -> Tuple[int, int, torch.Tensor, torch.Tensor]:
    """input_ids [B, S] (right-padded), lens [B] valid tokens per prompt -> (B, N, ids, ln): N = max(lens, 1) <= S
    the trimmed length, ids [B*N] on `device` (empty when B == 0), ln the int32 device copy of lens.  `name`
    (the encoder's) opens the messages."""
    B, S = input_ids.shape
    lens = lens.to(torch.int64).reshape(-1)
    if lens.numel() != B:
        raise ValueError(f"{name}: lens has {lens.numel()} entries for {B} prompts")
    lo, hi = (int(lens.min()), int(lens.max())) if B else (0, 0)
    if lo < 0 or hi > S:
        raise ValueError(f"{name}: lens outside [0, {S}]")
    N = max(hi, 1)
    return B, N, input_ids[:, :N].to(device).reshape(-1), lens.to(device=device, dtype=torch.int32)
