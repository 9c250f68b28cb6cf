"""T5 encoder (transformers T5EncoderModel / T5Stack, restated) on libeggroll: the flan-t5-xl prompt
encoder behind InfinityES.encode_prompts (models/Infinity.py:121-129, 257-335).

Per layer: T5 RMSNorm (no mean, no bias) on eggroll_rownorm reading the fp32 residual stream; bias-free
q / k / v as one r = 0 GEMM; eggroll_relbias_attention (unscaled scores + the bucketed relative-position
bias + the key-padding mask) reading the fused qkv output in place; `o` added into the fp32 stream in
the GEMM epilogue (res32); gated GELU (tanh, "gelu_new") feed-forward: wi_0 with the gelu epilogue,
wi_1 with mul, wo with res32; a final RMSNorm.  Weights are bf16, the residual stream fp32 (flan-t5-xl's
residual grows past what 16 bits hold; transformers keeps `wo` in fp32 for the same reason).

The relative-position bucket of every key - query distance is computed on the host (the same fp32 torch
expressions as T5Attention._relative_position_bucket), so a bucket edge cannot move with GPU rounding:
the kernel only reads the gathered [heads, 2R-1] table.  Block 0's table serves every layer, as in T5.

Sequences run trimmed to the batch's longest prompt, not padded to 512: with right padding and masked
keys the valid rows are the same as the padded run's.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from functools import partial

import torch
import torch.nn.functional as F
from torch import nn

from . import kernels as K
from . import text_encoder as TE
from .text_encoder import _w, linear as _linear

MAX_TOKENS = K.RELBIAS_MAX_N   # the reference's max_length (models/Infinity.py:304)


@dataclass(frozen=True)
class T5Arch:
    """Defaults: google/flan-t5-xl's encoder.  heads * d_kv need not equal d_model."""

    d_model: int = 2048
    d_kv: int = 64
    num_heads: int = 32
    d_ff: int = 5120
    num_layers: int = 24
    num_buckets: int = 32
    max_distance: int = 128
    eps: float = 1e-6
    vocab_size: int = 32128

    @property
    def inner(self) -> int:
        return self.num_heads * self.d_kv


def relative_position_bucket(rel: torch.Tensor, num_buckets: int = 32, max_distance: int = 128) -> torch.Tensor:
    """T5Attention._relative_position_bucket(bidirectional=True) restated: rel = key - query (int64).  Half the
    buckets per sign; exact below num_buckets / 4; logarithmic up to max_distance; clamped."""
    rel = rel.to(torch.int64)
    nb = num_buckets // 2
    ret = (rel > 0).to(torch.int64) * nb
    rel = rel.abs()
    max_exact = nb // 2
    is_small = rel < max_exact
    large = max_exact + (torch.log(rel.float() / max_exact) / math.log(max_distance / max_exact)
                         * (nb - max_exact)).to(torch.int64)
    large = torch.min(large, torch.full_like(large, nb - 1))
    return ret + torch.where(is_small, rel, large)


def rel_bias_table(weight: torch.Tensor, R: int, num_buckets: int = 32, max_distance: int = 128) -> torch.Tensor:
    """weight [num_buckets, heads] (relative_attention_bias.weight) -> fp32 [heads, 2R-1]: entry d + R-1 is the
    bias of key - query = d (the operand of kernels.relbias_attention).  Buckets on the host, gather on
    weight's device."""
    if weight.dim() != 2 or weight.shape[0] != num_buckets:
        raise ValueError(f"rel_bias_table: weight {tuple(weight.shape)} is not [num_buckets={num_buckets}, heads]")
    bucket = relative_position_bucket(torch.arange(-(R - 1), R), num_buckets, max_distance)
    return weight.detach().float()[bucket.to(weight.device)].t().contiguous()


class T5Block(nn.Module):
    def __init__(self, a: T5Arch):
        super().__init__()
        self.ln1 = _w(a.d_model)
        self.wqkv = _w(3 * a.inner, a.d_model)
        self.wo = _w(a.d_model, a.inner)
        self.ln2 = _w(a.d_model)
        self.wi0 = _w(a.d_ff, a.d_model)
        self.wi1 = _w(a.d_ff, a.d_model)
        self.wo_ff = _w(a.d_model, a.d_ff)


class T5Encoder(nn.Module):
    def __init__(self, a: T5Arch = T5Arch()):
        super().__init__()
        if a.d_kv != 64:
            raise NotImplementedError(f"T5Encoder: d_kv={a.d_kv} (eggroll_relbias_attention is head dim 64 only)")
        self.arch = a
        self.embed = _w(a.vocab_size, a.d_model)
        self.rel_bias = _w(a.num_buckets, a.num_heads)
        self.blocks = nn.ModuleList([T5Block(a) for _ in range(a.num_layers)])
        self.final_ln = _w(a.d_model)

    @torch.no_grad()
    def init_weights(self, seed: int = 0):
        """Random weights at T5's initialisation scales (timing runs; no checkpoint needed)."""
        a = self.arch
        fill = partial(TE.fill, generator=torch.Generator().manual_seed(seed))   # drawn on the CPU
        fill(self.embed, 1.0)
        fill(self.rel_bias, a.d_model ** -0.5)
        for b in self.blocks:
            b.ln1.fill_(1.0)
            b.ln2.fill_(1.0)
            fill(b.wqkv[: a.inner], (a.d_model * a.d_kv) ** -0.5)
            fill(b.wqkv[a.inner:], a.d_model ** -0.5)
            fill(b.wo, a.inner ** -0.5)
            fill(b.wi0, a.d_model ** -0.5)
            fill(b.wi1, a.d_model ** -0.5)
            fill(b.wo_ff, a.d_ff ** -0.5)
        self.final_ln.fill_(1.0)
        return self

    @torch.no_grad()
    def forward(self, input_ids: torch.Tensor, lens: torch.Tensor) -> torch.Tensor:
        """input_ids [B, S] (right-padded), lens [B] valid tokens per prompt -> last_hidden_state
        [B, N, d_model] bf16 with N = max(lens) <= S: rows < lens[b] are the encoder's output for prompt b, the
        rest padding (finite, not meaningful)."""
        a = self.arch
        dev = self.embed.device
        B, N, ids, ln = TE.trim_batch("T5Encoder", input_ids, lens, dev)
        if N > MAX_TOKENS:
            raise ValueError(f"T5Encoder: {N} tokens in a prompt (at most {MAX_TOKENS})")
        if B == 0:
            return torch.empty((0, N, a.d_model), dtype=torch.bfloat16, device=dev)
        table = rel_bias_table(self.rel_bias, N, a.num_buckets, a.max_distance)
        x = F.embedding(ids, self.embed).float()               # the fp32 residual stream [B*N, d_model]
        inner = a.inner
        for blk in self.blocks:
            h = K.rownorm(x, a.eps, w=blk.ln1)
            qkv = _linear(h, blk.wqkv)
            o = K.relbias_attention(qkv[:, :inner], qkv[:, inner:2 * inner], qkv[:, 2 * inner:], table, ln, B, N,
                                    a.num_heads, 1.0)
            _linear(o, blk.wo, "res32", res=x)
            h = K.rownorm(x, a.eps, w=blk.ln2)
            g = _linear(h, blk.wi0, "gelu")
            _linear(h, blk.wi1, "mul", res=g)
            _linear(g, blk.wo_ff, "res32", res=x)
        return K.rownorm(x, a.eps, w=self.final_ln).view(B, N, a.d_model)
