"""float64 restatement, in torch on the CPU, of steps 2-4 of eggroll_sample_bits (include/eggroll.h), and the
admissibility rule the bit sampler tests judge a bit by.

Given the fp32 CFG logits x [..., 2], the Exponential(1) draws q [..., 2], top_k and p_cut = float32(1 - top_p), with
lo <= hi the two logits of a bit:
  top-k   top_k == 1 masks lo when lo < hi; 0 or >= 2 masks nothing
  top-p   p_lo = e^(lo - hi) / (1 + e^(lo - hi)); lo is masked when lo < hi and p_lo <= p_cut (p_cut < 0: off)
  draw    the lowest index of argmax_c p'_c / q_c, p' the softmax over what is left (0 for a masked entry)
Equal logits are never masked.

With neither entry masked, r = (p'_1 / q_1) / (p'_0 / q_0).  A bit is DECIDED when
  |p_lo - p_cut| > D_CUT   (the kernel's fp32 two-term softmax is a few 2^-24 off p_lo), and
  it is masked to one class, or |r - 1| > D_TIE.
A kernel bit is admissible when it equals the oracle's bit wherever the bit is decided; at an undecided bit it must
be 0 or 1 and not a masked-out class: within D_CUT of the cut either the masked or the unmasked draw's bit, within
D_TIE of a tie either class unless the lower is surely masked.  At most CAP of a case's bits may be undecided, else
the case fails: the cap keeps the tolerance from hiding a wrong kernel.
"""
from functools import lru_cache

import numpy as np
import torch

D_CUT = 1e-6
D_TIE = 1e-5
CAP = 1e-3
# the recipe of the bit sampler tests (the issue's)
SCALES, TAU_CFG, TOP_K, TOP_P, GEN_SEED = (0.5, 2.0, 6.0), ((1.0, 3.0), (0.7, 1.5)), 900, 0.97, 5
CASES = tuple((s, tau, cfg) for s in SCALES for tau, cfg in TAU_CFG)


def p_cut_of(top_p: float) -> float:
    """What the caller hands the kernel, and what torch compares its fp32 cumsum against: float32(1 - top_p)."""
    return float(np.float32(1 - top_p)) if top_p > 0 else -1.0


def oracle(x: torch.Tensor, q: torch.Tensor, top_k: int, p_cut: float):
    """x, q fp32 [..., 2] on the CPU (no NaN, no +inf, no pair of -inf) -> dict of [...] tensors:
    bit (int64, the float64 bit), decided (bool), allowed0 / allowed1 (bool: may a kernel bit be 0 / 1)."""
    assert x.dtype == torch.float32 and q.dtype == torch.float32 and x.device.type == "cpu" and x.shape == q.shape
    x0, x1 = x[..., 0].double(), x[..., 1].double()
    q0, q1 = q[..., 0].double(), q[..., 1].double()
    tie = x0 == x1
    hi1 = x1 > x0
    e_lo = (-(x1 - x0).abs()).exp()                        # e^(lo - hi); 1 at a tie, 0 for lo = -inf
    e_lo = torch.where(tie, torch.ones_like(e_lo), e_lo)
    p_lo = e_lo / (1 + e_lo)
    by_k = ~tie & (top_k == 1)
    if p_cut >= 0:
        by_p, near_cut = ~tie & (p_lo <= p_cut), ~tie & ~by_k & ((p_lo - p_cut).abs() <= D_CUT)
    else:
        by_p, near_cut = torch.zeros_like(tie), torch.zeros_like(tie)
    masked = by_k | by_p
    w0 = torch.where(hi1, e_lo, torch.ones_like(e_lo)) / (1 + e_lo) / q0
    w1 = torch.where(hi1, torch.ones_like(e_lo), e_lo) / (1 + e_lo) / q1
    drawn = (w1 > w0).long()                               # neither masked; the lower index on a tie
    near_tie = ((w1 / w0) - 1).abs() <= D_TIE
    hi_bit = hi1.long()
    bit = torch.where(masked, hi_bit, drawn)
    sure_masked = masked & ~near_cut
    decided = ~near_cut & (masked | ~near_tie)
    # what a kernel bit may be: the oracle's bit; the other outcome of an undecided cut; either class of a near tie
    # that may be drawn (the lower entry not surely masked)
    allowed = [bit == c for c in (0, 1)]
    for c in (0, 1):
        allowed[c] = allowed[c] | (near_cut & ((hi_bit == c) | (drawn == c))) | (near_tie & ~sure_masked)
    return {"bit": bit, "decided": decided, "allowed0": allowed[0], "allowed1": allowed[1], "masked": masked}


def admissible(o, bits: torch.Tensor) -> torch.Tensor:
    """bool [...]: is bits[...] an admissible bit under oracle `o`."""
    b = bits.cpu().reshape(o["bit"].shape)
    ok = torch.where(b == 0, o["allowed0"], torch.where(b == 1, o["allowed1"], torch.zeros_like(o["decided"])))
    return ok & (~o["decided"] | (b == o["bit"]))


def check(o, bits: torch.Tensor, what: str = ""):
    """The whole judgement of one case: prints the counts, asserts every bit admissible and the undecided share
    under the cap.  Returns the number of undecided bits."""
    adm = admissible(o, bits)
    und = int((~o["decided"]).sum())
    total = o["bit"].numel()
    differ = int((bits.cpu().reshape(o["bit"].shape) != o["bit"]).sum())
    print(f"[bit oracle{what}] bits {total}; undecided {und}; masked {int(o['masked'].sum())}; off the float64 bit "
          f"{differ}; inadmissible {int((~adm).sum())}")
    assert und <= CAP * total, (und, total)
    assert bool(adm.all())
    return und


def combine(c: torch.Tensor, u: torch.Tensor, tau: float, cfg: float, reciprocal: bool) -> torch.Tensor:
    """torch's `lg / tau; cfg * lg_cond + (1.0 - cfg) * lg_uncond` in fp32 on the CPU, every operation rounded on its
    own; reciprocal: the division as torch evaluates it on the GPU, a multiplication by kernels.inv_tau_of(tau)."""
    if reciprocal:
        from hyperscalees_t2i_amd.kernels import inv_tau_of
        c, u = c * inv_tau_of(tau), u * inv_tau_of(tau)
    else:
        c, u = c / float(tau), u / float(tau)
    return float(cfg) * c + (1.0 - float(cfg)) * u


@lru_cache(maxsize=None)
def recipe(s: float, n: int = 2, B: int = 3, bits_per_image: int = 128):
    """(cond, uncond) of the recipe at scale s: bf16-valued fp32 [n, B, bits_per_image, 2] logits ~ s N(0, 1).
    Shared by the tests; do not write to them."""
    g = torch.Generator().manual_seed(0)
    c = (torch.randn(n, B, bits_per_image, 2, generator=g) * s).bfloat16().float()
    u = (torch.randn(n, B, bits_per_image, 2, generator=g) * s).bfloat16().float()
    return c, u


def draws(shape, seed: int = GEN_SEED, device="cpu") -> torch.Tensor:
    """What torch.multinomial(p, 1, True, generator=g) draws for itself with g seeded `seed`."""
    g = torch.Generator(device=device).manual_seed(seed)
    return torch.empty(shape, dtype=torch.float32, device=device).exponential_(1, generator=g)
