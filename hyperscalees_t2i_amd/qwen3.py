"""Qwen3 text model (transformers Qwen3Model, restated) on libeggroll: the Qwen3-4B prompt encoder behind
ZImageTurboES.encode_prompts (models/zImageTurbo.py:247-309).

ZImagePipeline.encode_prompt takes `hidden_states[-2]`: the residual stream after layer L - 2.  So only
L - 1 blocks are built and run; the last decoder layer and the final norm never reach the GPU.

The stream is the embedding (not scaled), fp32.  Per layer: RMSNorm (x / rms * w, NOT 1 + w) on
eggroll_rownorm reading the fp32 stream; bias-free q | k | v as one r = 0 GEMM; per-head RMSNorm over head_dim
on q and on k, each with its own weight, then rotate-half RoPE, in place on the q | k columns in one launch
(eggroll_qk_norm_rope_half); eggroll_causal_attention (grouped KV heads, causal + key lengths, scale =
head_dim ** -0.5) reading the fused qkv output in place; o_proj with the res32 epilogue into the stream;
pre-norm; gate with the silu epilogue, up with mul, down with res32.  Weights are bf16; the norm weights are
kept in fp32: the hidden-size ones as rownorm's fp32 `1 + mscale` operand (mscale = w - 1, so w is not
rounded to bf16 on top of the GEMM operand's rounding), the q / k ones as the kernel's fp32 [128] operands.

The cos / sin tables are computed on the host with Qwen3RotaryEmbedding's expressions, so no angle moves
with GPU rounding.  Sequences run trimmed to the batch's longest prompt: with right padding and a causal
mask the valid rows are the same as the padded run's.  PARITY WITH DIFFUSERS' ZImagePipeline.encode_prompt IS
UNPINNED (diffusers is not importable here); the oracle of the tests is transformers' Qwen3Model.
"""
from __future__ import annotations

from dataclasses import dataclass
from functools import partial
from typing import Tuple

import torch
import torch.nn.functional as F
from torch import nn

from . import kernels as K
from . import text_encoder as TE
from .text_encoder import _nw, _w, linear as _linear

HEAD_DIM = 128   # eggroll_causal_attention / eggroll_qk_norm_rope_half


@dataclass(frozen=True)
class Qwen3Arch:
    """Defaults: Qwen3-4B (the text encoder of Tongyi-MAI/Z-Image-Turbo)."""

    hidden_size: int = 2560
    num_layers: int = 36
    num_heads: int = 32
    num_kv_heads: int = 8
    head_dim: int = 128
    intermediate_size: int = 9728
    rope_theta: float = 1e6
    eps: float = 1e-6
    vocab_size: int = 151936

    @property
    def q_width(self) -> int:
        return self.num_heads * self.head_dim

    @property
    def kv_width(self) -> int:
        return self.num_kv_heads * self.head_dim

    @property
    def run_layers(self) -> int:
        """Blocks that run for hidden_states[-2]: all but the last."""
        return max(self.num_layers - 1, 0)


def rope_tables(N: int, head_dim: int = HEAD_DIM, theta: float = 1e6) -> Tuple[torch.Tensor, torch.Tensor]:
    """Qwen3RotaryEmbedding restated: text_encoder.rope_tables at this model's defaults."""
    return TE.rope_tables(N, head_dim, theta)


def _norm(x: torch.Tensor, mscale: torch.Tensor, eps: float) -> torch.Tensor:
    """x / rms(x) * (1 + mscale), mscale = w - 1 fp32 [1, C]; x the fp32 stream; bf16 out."""
    return K.rownorm(x, eps, mscale=mscale, rows_per_group=max(x.shape[0], 1))


class Qwen3Block(nn.Module):
    """ln_in / ln_post_attn hold w - 1 (rownorm's mscale operand); q_norm / k_norm hold w."""

    def __init__(self, a: Qwen3Arch):
        super().__init__()
        C = a.hidden_size
        self.ln_in = _nw(C)
        self.wqkv = _w(a.q_width + 2 * a.kv_width, C)
        self.q_norm = nn.Parameter(torch.zeros(a.head_dim, dtype=torch.float32), requires_grad=False)
        self.k_norm = nn.Parameter(torch.zeros(a.head_dim, dtype=torch.float32), requires_grad=False)
        self.wo = _w(C, a.q_width)
        self.ln_post_attn = _nw(C)
        self.w_gate = _w(a.intermediate_size, C)
        self.w_up = _w(a.intermediate_size, C)
        self.w_down = _w(C, a.intermediate_size)


class Qwen3Encoder(nn.Module):
    def __init__(self, a: Qwen3Arch = Qwen3Arch()):
        super().__init__()
        if a.head_dim != HEAD_DIM:
            raise NotImplementedError(f"Qwen3Encoder: head_dim={a.head_dim} (eggroll_causal_attention is head dim "
                                      f"{HEAD_DIM} only)")
        if a.num_kv_heads < 1 or a.num_heads % a.num_kv_heads:
            raise ValueError(f"Qwen3Encoder: {a.num_heads} query heads on {a.num_kv_heads} KV heads")
        if a.hidden_size % 8 or a.hidden_size > 4096:
            raise NotImplementedError(f"Qwen3Encoder: hidden_size={a.hidden_size} (eggroll_rownorm: a multiple of 8, "
                                      f"at most 4096)")
        if a.num_layers < 1:
            raise ValueError(f"Qwen3Encoder: num_layers={a.num_layers}")
        self.arch = a
        self.embed = _w(a.vocab_size, a.hidden_size)
        self.blocks = nn.ModuleList([Qwen3Block(a) for _ in range(a.run_layers)])   # hidden_states[-2]: L - 1 blocks

    @torch.no_grad()
    def init_weights(self, seed: int = 0):
        """Random weights, fan-in scaled so activations stay O(1) (timing runs; no checkpoint needed).  Drawn on
        the device the parameters live on."""
        a = self.arch
        fill = partial(TE.fill, generator=torch.Generator(device=self.embed.device).manual_seed(seed))
        fill(self.embed, 0.02)
        for b in self.blocks:
            b.ln_in.zero_()
            b.ln_post_attn.zero_()
            b.q_norm.fill_(1.0)
            b.k_norm.fill_(1.0)
            fill(b.wqkv, a.hidden_size ** -0.5)
            fill(b.wo, a.q_width ** -0.5)
            fill(b.w_gate, a.hidden_size ** -0.5)
            fill(b.w_up, a.hidden_size ** -0.5)
            fill(b.w_down, a.intermediate_size ** -0.5)
        return self

    @torch.no_grad()
    def forward(self, input_ids: torch.Tensor, lens: torch.Tensor) -> torch.Tensor:
        """input_ids [B, S] (right-padded), lens [B] valid tokens per prompt -> hidden_states[-2] [B, N, hidden]
        bf16 with N = max(lens) <= S: rows < lens[b] are the model's stream after layer L - 2 for prompt b, the
        rest padding (finite, not meaningful)."""
        a = self.arch
        dev = self.embed.device
        B, N, ids, ln = TE.trim_batch("Qwen3Encoder", input_ids, lens, dev)
        if B == 0:
            return torch.empty((0, N, a.hidden_size), dtype=torch.bfloat16, device=dev)
        cos, sin = (t.to(dev) for t in rope_tables(N, a.head_dim, a.rope_theta))
        x = F.embedding(ids, self.embed).float()   # the fp32 residual stream [B*N, hidden]
        qw, kw = a.q_width, a.kv_width
        scale = float(a.head_dim) ** -0.5
        for blk in self.blocks:
            qkv = _linear(_norm(x, blk.ln_in, a.eps), blk.wqkv)
            K.qk_norm_rope_half_(qkv, blk.q_norm, blk.k_norm, a.eps, cos, sin, B, N, a.num_heads, a.num_kv_heads)
            o = K.causal_attention(qkv[:, :qw], qkv[:, qw:qw + kw], qkv[:, qw + kw:], ln, B, N, a.num_heads,
                                   a.num_kv_heads, scale)
            _linear(o, blk.wo, "res32", res=x)
            h = _norm(x, blk.ln_post_attn, a.eps)
            g = _linear(h, blk.w_gate, "silu")
            _linear(h, blk.w_up, "mul", res=g)
            _linear(g, blk.w_down, "res32", res=x)
        return x.to(torch.bfloat16).view(B, N, a.hidden_size)
