"""float64 restatement, in torch on the CPU, of the row arithmetic of eggroll_sample_topk_topp (include/eggroll.h),
and the admissibility rule the sampler tests judge a token by.

Given the fp32 CFG logits x [R, V], the Exponential(1) draws q [R, V], top_k and p_cut = float32(1 - top_p):
  top-k   entries below the top_k-th largest x (with multiplicity) are masked; exact, the values are fp32
  top-p   p = softmax over the unmasked, C(v) = sum of p_i over unmasked i with x_i <= v (a tie group shares one C);
          entry j is kept when C(x_j) > p_cut or x_j is the row maximum
  draw    the lowest index of argmax_j w_j over the kept, w_j = exp(x_j - max) / q_j

The kernel evaluates C in fp32, so an entry whose C lies within D of p_cut may fall either way:
  K_lo (sure keep)  C > p_cut + D        K_hi (may keep)  C > p_cut - D
D = 5e-4 is twice V * 2^-24 at V = 4096, the worst-case error of an fp32 sum of at most 4096 non-negative terms that
total at most 1: one share for the cumulative sum, one for the softmax normaliser.

A token t is admissible when t is in K_hi, w_t >= (1 - SLACK) w_j for every j in K_lo, and w_t >= (1 - SLACK) w_j for
every j in K_hi with x_j >= x_t (the kept set is a threshold set: one that holds t holds those too).  Where
K_lo == K_hi this is the exact argmax up to SLACK.
"""
from functools import lru_cache

import numpy as np
import torch

D = 5e-4
SLACK = 1e-5
# the recipe of the sampler tests (the issue's): 2048 rows of 4096 bf16-valued logits at three scales
ROWS, VOCAB, SCALES, T_CFG, TOP_K, TOP_P, GEN_SEED = 2048, 4096, (0.5, 2.0, 6.0), 2.0, 900, 0.95, 5


def p_cut_of(top_p: float) -> float:
    """What the caller hands the kernel, and what torch compares its fp32 cumsum against: float32(1 - top_p)."""
    return float(np.float32(1 - top_p)) if top_p > 0 else -1.0


def oracle(x: torch.Tensor, q: torch.Tensor, top_k: int, p_cut: float, d: float = D):
    """x, q fp32 [R, V] on the CPU -> dict(K_lo, K_hi bool [R, V]; w float64 [R, V]; exact int64 [R], the token at
    d = 0)."""
    assert x.dtype == torch.float32 and x.device.type == "cpu" and x.dim() == 2
    R, V = x.shape
    xd = x.double()
    mx = xd.amax(dim=-1, keepdim=True)
    live = torch.ones_like(x, dtype=torch.bool)
    if 0 < top_k < V:
        kth = x.topk(top_k, dim=-1)[0][:, -1:]
        live = x >= kth
    e = torch.where(live, (xd - mx).exp(), torch.zeros_like(xd))
    is_max = xd == mx
    if p_cut >= 0:
        p = e / e.sum(dim=-1, keepdim=True)
        xs, order = xd.sort(dim=-1, stable=True)
        cs = p.gather(1, order).cumsum(dim=-1)
        last = torch.searchsorted(xs, xd.contiguous(), right=True) - 1      # the tie group's last member
        C = cs.gather(1, last)
        keep = [live & ((C > p_cut + dd) | is_max) for dd in (d, -d, 0.0)]
    else:
        keep = [live, live, live]
    w = (xd - mx).exp() / q.double()
    exact = torch.where(keep[2], w, torch.full_like(w, -1.0)).argmax(dim=-1)
    return {"K_lo": keep[0], "K_hi": keep[1], "w": w, "exact": exact}


def admissible(o, x: torch.Tensor, tok: torch.Tensor) -> torch.Tensor:
    """bool [R]: is tok[r] an admissible token of row r under oracle `o` of x."""
    tok = tok.reshape(-1).cpu()
    ok = (tok >= 0) & (tok < x.shape[1])
    t = tok.clamp(0, x.shape[1] - 1)[:, None]
    w, none = o["w"], torch.full_like(o["w"], -1.0)
    wt, xt = w.gather(1, t), x.gather(1, t)
    best_lo = torch.where(o["K_lo"], w, none).amax(dim=-1, keepdim=True)
    best_above = torch.where(o["K_hi"] & (x >= xt), w, none).amax(dim=-1, keepdim=True)
    ok &= o["K_hi"].gather(1, t)[:, 0]
    ok &= (wt >= (1 - SLACK) * best_lo)[:, 0] & (wt >= (1 - SLACK) * best_above)[:, 0]
    return ok


@lru_cache(maxsize=None)
def recipe(s: float, rows: int = ROWS, V: int = VOCAB):
    """(c, u, x) of the recipe at scale s: bf16-valued fp32 cond / uncond logits and their CFG combine at T_CFG, as
    torch computes it in fp32 (two rounded products, one subtraction).  Shared by the tests; do not write to them."""
    torch.manual_seed(0)
    c = (torch.randn(rows, V) * s).bfloat16().float()
    u = (torch.randn(rows, V) * s).bfloat16().float()
    return c, u, (1 + T_CFG) * c - T_CFG * u


def draws(shape, seed: int = GEN_SEED, device="cpu") -> torch.Tensor:
    """What torch.multinomial(p, 1, True, generator=g) draws for itself with g seeded `seed`."""
    g = torch.Generator(device=device).manual_seed(seed)
    return torch.empty(shape, dtype=torch.float32, device=device).exponential_(1, generator=g)
