"""The bit sampler's host side (no GPU): eggroll_sample_bits is declared in all the places that bind it, refuses what
is outside its class before anything touches a device, InfinityConfig turns it on by default, and the float64
oracle of tests/bit_sampler_oracle.py agrees with the torch sampler it restates (infinity.sample_bits on the CPU) on
the recipe the GPU tests use."""
import re

import pytest
import torch

from hyperscalees_t2i_amd import _lib
from tests import bit_sampler_oracle as BO

NAME = "eggroll_sample_bits"


def test_signature_is_declared_everywhere():
    assert NAME in _lib.SIGNATURES and NAME in _lib.header_symbols()
    res, args = _lib.SIGNATURES[NAME]
    assert len(args) == 21
    md = (_lib.HEADER.parent.parent / "INTEGRATION.md").read_text()
    stub = re.findall(r"```python\n(.*?)```", md, flags=re.S)[0]
    assert f"lib.{NAME}.restype, lib.{NAME}.argtypes = i32, [" in stub
    assert f"| `{NAME}` |" in md.split("## 3.")[1]     # a row of the §3 table


def _call(lib, head=None, ld=8, n=1, B=1, h=1, w=1, d_tok=4, p_cut=-1.0, patchify=0, top_k=0):
    return lib.eggroll_sample_bits(head, 1, ld, n, B, h, w, d_tok, 1.0, 3.0, -2.0, top_k, p_cut, None, None, None,
                                   patchify, 0.5, None, None, None)


@pytest.mark.parametrize("kw,needle", [(dict(d_tok=0), b"d_tok=0"), (dict(ld=9, d_tok=4), b"ld=9"),
                                       (dict(ld=6, d_tok=4), b"ld=6"), (dict(patchify=1, d_tok=6, ld=12), b"patchify"),
                                       (dict(n=-1), b"negative size n=-1"), (dict(p_cut=float("nan")), b"NaN"),
                                       (dict(head=None), b"NULL pointer")],
                         ids=["d_tok=0", "odd ld", "ld < 2 d_tok", "patchify with d_tok=6", "negative n", "NaN p_cut",
                              "null head with work"])
def test_refused_on_the_host_without_a_device(kw, needle):
    """The class is checked before anything touches the device: the refusals of the issue, by message."""
    lib = _lib.load()
    assert _call(lib, **kw) == -1, kw
    msg = lib.eggroll_last_error()
    assert msg.startswith(b"sample_bits: ") and needle in msg, msg


def test_zero_work_is_a_noop():
    lib = _lib.load()
    for kw in (dict(n=0), dict(B=0), dict(h=0), dict(w=0)):
        assert _call(lib, **kw) == 0, kw
    assert _call(lib, n=1 << 20, B=1 << 20, h=0) == 0                       # zero work, however large the rest
    assert _call(lib, n=1 << 16, B=1 << 15, d_tok=4) == -1                  # 2^33 bits
    assert b"2^31" in lib.eggroll_last_error()


def test_infinity_config_turns_the_native_sampler_on():
    from hyperscalees_t2i_amd.backend import InfinityConfig
    assert InfinityConfig().native_sampler is True
    assert InfinityConfig(native_sampler=False).native_sampler is False


@pytest.mark.parametrize("s,tau,cfg", BO.CASES)
def test_oracle_agrees_with_the_torch_sampler(s, tau, cfg):
    """infinity.sample_bits on the CPU (generator seed 5) against the oracle fed the draws of a generator in the same
    state: every torch bit is admissible, the undecided share is under the cap."""
    from hyperscalees_t2i_amd.infinity import sample_bits
    c, u = BO.recipe(s)
    x = BO.combine(c, u, tau, cfg, reciprocal=False).reshape(-1, c.shape[2], 2)          # [n * B, bits, 2]
    g = torch.Generator().manual_seed(BO.GEN_SEED)
    bits = sample_bits(x.clone(), g, BO.TOP_K, BO.TOP_P)
    o = BO.oracle(x, BO.draws(x.shape), BO.TOP_K, BO.p_cut_of(BO.TOP_P))
    BO.check(o, bits, f", s={s} tau={tau} cfg={cfg}")


def test_oracle_closed_forms_and_edges():
    """The definition's corners on hand-made bits: a tie is never masked and is drawn by q, top_k == 1 keeps the
    larger, the top-p cut masks the smaller exactly when its share is at most p_cut, a single -inf is masked."""
    inf = float("inf")
    x = torch.tensor([[0.0, 0.0], [0.0, 0.0], [1.0, 3.0], [3.0, 1.0], [-inf, 2.0], [0.0, 0.1]])
    q = torch.tensor([[1.0, 2.0], [2.0, 1.0], [1e-6, 1.0], [1.0, 1e-6], [1e-9, 1.0], [1.0, 3.0]])
    o = BO.oracle(x, q, 0, -1.0)                        # nothing masked: the draw alone
    assert o["bit"].tolist() == [0, 1, 0, 1, 1, 0] and bool(o["decided"].all()) and not bool(o["masked"].any())
    o = BO.oracle(x, q, 1, -1.0)                        # top_k 1: the larger, ties by q
    assert o["bit"].tolist() == [0, 1, 1, 0, 1, 1] and o["masked"].tolist() == [False, False, True, True, True, True]
    o = BO.oracle(x, q, 2, 0.2)                         # p_lo = 0.119 (masked), 0, and 0.475 (kept)
    assert o["bit"].tolist() == [0, 1, 1, 0, 1, 0] and o["masked"].tolist() == [False, False, True, True, True, False]
    assert not bool(BO.admissible(o, torch.tensor([1, 0, 0, 1, 0, 1])).any())
    near = BO.oracle(torch.tensor([[0.0, 1.0]]), torch.tensor([[1.0, 2.718281828459045]]), 0, -1.0)   # r = 1
    assert not bool(near["decided"].any()) and bool(BO.admissible(near, torch.tensor([0])).all())
    assert bool(BO.admissible(near, torch.tensor([1])).all()) and not bool(BO.admissible(near, torch.tensor([2])).any())
