"""The token sampler's host side (no GPU): eggroll_sample_topk_topp is declared in all three places that bind it,
VarConfig turns it on by default, and the float64 oracle of tests/sampler_oracle.py agrees with the torch sampler it
restates (sample_population on the CPU) on the recipe the GPU tests use."""
import re

import pytest
import torch

from hyperscalees_t2i_amd import _lib
from hyperscalees_t2i_amd.var import sample_population
from tests import sampler_oracle as SO

NAME = "eggroll_sample_topk_topp"


def test_signature_is_declared_everywhere():
    assert NAME in _lib.SIGNATURES and NAME in _lib.header_symbols()
    res, args = _lib.SIGNATURES[NAME]
    assert len(args) == 18
    md = (_lib.HEADER.parent.parent / "INTEGRATION.md").read_text()
    stub = re.findall(r"```python\n(.*?)```", md, flags=re.S)[0]
    assert f"lib.{NAME}.restype, lib.{NAME}.argtypes = i32, [" in stub
    assert f"| `{NAME}` |" in md.split("## 3.")[1]     # a row of the §3 table
    from hyperscalees_t2i_amd.build_ext import SOURCES
    assert "eggroll_sample.hip" in SOURCES


def test_refused_on_the_host_without_a_device():
    """The class is checked before anything touches the device: the three refusals of the issue, by message."""
    lib = _lib.load()

    def call(V, ld, ldq=4096):
        return lib.eggroll_sample_topk_topp(None, None, 1, ld, 1, 0, 1.0, 0.0, 4, V, 0, -1.0, None, ldq, None, None, 0,
                                            None)
    for V, ld in ((4100, 4100), (4098, 4100), (1002, 1004), (0, 8), (4096, 4092)):
        assert call(V, ld, max(V, 4)) == -1, (V, ld)
        assert b"sample_topk_topp" in lib.eggroll_last_error()
    assert lib.eggroll_sample_topk_topp(None, None, 1, 8, 0, 0, 1.0, 0.0, 4, 8, 0, -1.0, None, 8, None, None, 0, None) == -1
    assert lib.eggroll_sample_topk_topp(None, None, 1, 8, 1, 0, 1.0, 0.0, 0, 8, 0, -1.0, None, 8, None, None, 0, None) == 0


def test_var_config_turns_the_native_sampler_on():
    from hyperscalees_t2i_amd.backend import VarConfig
    assert VarConfig().native_sampler is True
    assert VarConfig(native_sampler=False).native_sampler is False


@pytest.mark.parametrize("s", SO.SCALES)
def test_oracle_agrees_with_the_torch_sampler(s):
    """sample_population on the CPU (generator seed 5) against the oracle fed the draws of a generator in the same
    state: every torch token is admissible and equals the oracle's exact-argmax token.  (The kept SETS differ in
    boundary ties, where torch's sort order decides: that is why tokens are compared, not masks.)"""
    _, _, x = SO.recipe(s)
    g = torch.Generator().manual_seed(SO.GEN_SEED)
    tok = sample_population(x.clone()[None, None], [g], SO.TOP_K, SO.TOP_P).reshape(-1)
    o = SO.oracle(x, SO.draws(x.shape), SO.TOP_K, SO.p_cut_of(SO.TOP_P))
    adm = SO.admissible(o, x, tok)
    differ = int((tok != o["exact"]).sum())
    print(f"[sampler oracle, s={s}] torch tokens off the exact argmax: {differ} of {tok.numel()}; inadmissible: "
          f"{int((~adm).sum())}; rows with K_lo != K_hi: {int((o['K_lo'] != o['K_hi']).any(dim=-1).sum())}")
    assert bool(adm.all())
    assert differ == 0


def test_oracle_tie_groups_and_edges():
    """The definition's corners on hand-made rows: a tie group shares its fate, the maximum always survives, top_k
    counts with multiplicity and keeps ties at the k-th value."""
    x = torch.tensor([[0.0, 0.0, 0.0, 0.0], [1.0, 1.0, 5.0, -1.0], [2.0, 2.0, 2.0, 9.0]])
    q = torch.ones_like(x)
    o = SO.oracle(x, q, 0, 0.6, d=0.0)
    assert o["K_lo"][0].tolist() == [True] * 4            # C = 1 for the whole tie group
    assert o["K_lo"][1].tolist() == [False, False, True, False]
    o = SO.oracle(x, q, 0, 2.0, d=0.0)                     # nothing passes: the maximum alone
    assert o["K_lo"].sum(dim=-1).tolist() == [4, 1, 1]
    o = SO.oracle(x, q, 2, -1.0)
    assert o["K_lo"][1].tolist() == [True, True, True, False] and o["K_lo"][2].tolist() == [True] * 4
    assert o["exact"].tolist() == [0, 2, 3]
