"""Gemma-2 text model (transformers Gemma2Model, restated) on libeggroll: the gemma-2-2b prompt encoder
behind SanaOneStep.encode_prompts (models/SanaSprint.py:171-277).

The stream is embed * sqrt(hidden), fp32.  Per layer: Gemma RMSNorm (x / rms * (1 + w)) on eggroll_rownorm
reading the fp32 stream; bias-free q | k | v as one r = 0 GEMM; rotate-half RoPE at head dim 256 in place
on the q and k columns (eggroll_rope_half); eggroll_softcap_attention (grouped KV heads, causal + key
lengths, cap * tanh(scale * q.k / cap) with scale = query_pre_attn_scalar ** -0.5, NOT head_dim ** -0.5)
reading the fused qkv output in place; o_proj; the post-attention norm and the residual add in one rownorm
(norm, THEN add: Gemma-2's sandwich norms); pre-FFN norm; gate with the gelu (tanh) epilogue, up with mul,
down; the post-FFN norm + add; a final norm.  Weights are bf16; the norm weights are kept in fp32 and enter
rownorm as its fp32 `1 + mscale` operand, because bf16(1 + w) rounds coarser than 1 + bf16(w).

The cos / sin tables are computed on the host with Gemma2RotaryEmbedding's expressions, so no angle moves
with GPU rounding.  Sequences run trimmed to the batch's longest prompt: with right padding and a causal
mask the valid rows are the same as the padded run's.  Gemma-2 alternates sliding-window and global layers;
a window >= N is the causal mask, and longer sequences are refused.
"""
from __future__ import annotations

from dataclasses import dataclass
from functools import partial
from typing import Optional, Tuple

import torch
import torch.nn.functional as F
from torch import nn

from . import kernels as K
from . import text_encoder as TE
from .text_encoder import _nw, _w, linear as _linear

HEAD_DIM = 256   # eggroll_softcap_attention / eggroll_rope_half


@dataclass(frozen=True)
class Gemma2Arch:
    """Defaults: google/gemma-2-2b (the text encoder of Sana_Sprint_1.6B_1024px_diffusers)."""

    hidden_size: int = 2304
    num_layers: int = 26
    num_heads: int = 8
    num_kv_heads: int = 4
    head_dim: int = 256
    intermediate_size: int = 9216
    softcap: float = 50.0
    query_pre_attn_scalar: float = 256.0
    rope_theta: float = 10000.0
    eps: float = 1e-6
    vocab_size: int = 256000
    sliding_window: int = 4096

    @property
    def q_width(self) -> int:
        return self.num_heads * self.head_dim

    @property
    def kv_width(self) -> int:
        return self.num_kv_heads * self.head_dim


def rope_tables(N: int, head_dim: int = HEAD_DIM, theta: float = 10000.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """Gemma2RotaryEmbedding restated: text_encoder.rope_tables at this model's defaults."""
    return TE.rope_tables(N, head_dim, theta)


def _norm(x: torch.Tensor, w: torch.Tensor, eps: float, res: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x / rms(x) * (1 + w), w fp32 [1, C]; with res (the fp32 stream): res += that, in place."""
    return K.rownorm(x, eps, mscale=w, rows_per_group=max(x.shape[0], 1), res=res)


class Gemma2Block(nn.Module):
    def __init__(self, a: Gemma2Arch):
        super().__init__()
        C = a.hidden_size
        self.ln_in = _nw(C)
        self.wqkv = _w(a.q_width + 2 * a.kv_width, C)
        self.wo = _w(C, a.q_width)
        self.ln_post_attn = _nw(C)
        self.ln_pre_ff = _nw(C)
        self.w_gate = _w(a.intermediate_size, C)
        self.w_up = _w(a.intermediate_size, C)
        self.w_down = _w(C, a.intermediate_size)
        self.ln_post_ff = _nw(C)


class Gemma2Encoder(nn.Module):
    def __init__(self, a: Gemma2Arch = Gemma2Arch()):
        super().__init__()
        if a.head_dim != HEAD_DIM:
            raise NotImplementedError(f"Gemma2Encoder: head_dim={a.head_dim} (eggroll_softcap_attention is head dim "
                                      f"{HEAD_DIM} only)")
        if a.num_kv_heads < 1 or a.num_heads % a.num_kv_heads:
            raise ValueError(f"Gemma2Encoder: {a.num_heads} query heads on {a.num_kv_heads} KV heads")
        if a.hidden_size % 8 or a.hidden_size > 4096:
            raise NotImplementedError(f"Gemma2Encoder: hidden_size={a.hidden_size} (eggroll_rownorm: a multiple of 8, "
                                      f"at most 4096)")
        self.arch = a
        self.embed = _w(a.vocab_size, a.hidden_size)
        self.blocks = nn.ModuleList([Gemma2Block(a) for _ in range(a.num_layers)])
        self.final_ln = _nw(a.hidden_size)

    @torch.no_grad()
    def init_weights(self, seed: int = 0):
        """Random weights, fan-in scaled so activations stay O(1) (timing runs; no checkpoint needed).  Drawn on
        the device the parameters live on: the 2.6 B values of the default architecture take seconds there."""
        a = self.arch
        fill = partial(TE.fill, generator=torch.Generator(device=self.embed.device).manual_seed(seed))
        fill(self.embed, 0.02)
        for b in self.blocks:
            for ln in (b.ln_in, b.ln_post_attn, b.ln_pre_ff, b.ln_post_ff):
                ln.zero_()
            fill(b.wqkv, a.hidden_size ** -0.5)
            fill(b.wo, a.q_width ** -0.5)
            fill(b.w_gate, a.hidden_size ** -0.5)
            fill(b.w_up, a.hidden_size ** -0.5)
            fill(b.w_down, a.intermediate_size ** -0.5)
        self.final_ln.zero_()
        return self

    @torch.no_grad()
    def forward(self, input_ids: torch.Tensor, lens: torch.Tensor) -> torch.Tensor:
        """input_ids [B, S] (right-padded), lens [B] valid tokens per prompt -> last_hidden_state
        [B, N, hidden] bf16 with N = max(lens) <= S: rows < lens[b] are the model's output for prompt b, the
        rest padding (finite, not meaningful)."""
        a = self.arch
        dev = self.embed.device
        B, N, ids, ln = TE.trim_batch("Gemma2Encoder", input_ids, lens, dev)
        if N > a.sliding_window:
            raise NotImplementedError(f"Gemma2Encoder: {N} tokens exceed sliding_window={a.sliding_window} (the "
                                      f"sliding-window layers are run as causal layers)")
        if B == 0:
            return torch.empty((0, N, a.hidden_size), dtype=torch.bfloat16, device=dev)
        cos, sin = (t.to(dev) for t in rope_tables(N, a.head_dim, a.rope_theta))
        x = F.embedding(ids, self.embed).float() * (a.hidden_size ** 0.5)   # the fp32 residual stream [B*N, hidden]
        qw, kw = a.q_width, a.kv_width
        scale = float(a.query_pre_attn_scalar) ** -0.5
        for blk in self.blocks:
            h = _norm(x, blk.ln_in, a.eps)
            qkv = _linear(h, blk.wqkv)
            K.rope_half_(qkv, cos, sin, B, N, a.num_heads + a.num_kv_heads)
            o = K.softcap_attention(qkv[:, :qw], qkv[:, qw:qw + kw], qkv[:, qw + kw:], ln, B, N, a.num_heads,
                                    a.num_kv_heads, scale, a.softcap)
            _norm(_linear(o, blk.wo), blk.ln_post_attn, a.eps, res=x)
            h = _norm(x, blk.ln_pre_ff, a.eps)
            g = _linear(h, blk.w_gate, "gelu")
            _linear(h, blk.w_up, "mul", res=g)
            _norm(_linear(g, blk.w_down), blk.ln_post_ff, a.eps, res=x)
        return _norm(x, self.final_ln, a.eps).view(B, N, a.hidden_size)
