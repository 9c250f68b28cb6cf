"""eggroll_sample_topk_topp on the device: the CFG combine bit for bit against torch, the exact corners of the
definition, admissibility of every token under the float64 oracle (tests/sampler_oracle.py), parity with the torch
sampler it replaces (sample_population), determinism, refused calls, and the wiring into VARPopulationInfer."""
from functools import lru_cache

import pytest
import torch

from hyperscalees_t2i_amd import _lib
from hyperscalees_t2i_amd import kernels as K
from hyperscalees_t2i_amd.var import BAD_PROBS, sample_population, sample_population_native
from tests import sampler_oracle as SO

pytestmark = pytest.mark.gpu

T = SO.T_CFG


def _logits(dev, shape, dtype, seed, scale=3.0):
    g = torch.Generator(device=dev).manual_seed(seed)
    return (torch.randn(shape, generator=g, device=dev) * scale).to(dtype)


def _raw(cond, uncond, bf16, ld, rpb, block_ld, wc, wu, R, V, top_k, p_cut, q, ldq, idx, x_out, ldx):
    _lib.call("eggroll_sample_topk_topp", cond.data_ptr(), None if uncond is None else uncond.data_ptr(), bf16, ld, rpb,
              block_ld, wc, wu, R, V, top_k, p_cut, q.data_ptr(), ldq, idx.data_ptr(),
              None if x_out is None else x_out.data_ptr(), ldx, torch.cuda.current_stream(cond.device).cuda_stream)


# ---------------------------------------------------------------------------------------------------
# the combine, bit for bit
# ---------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("V", (4096, 1000))
@pytest.mark.parametrize("R", (1, 5, 257))
@pytest.mark.parametrize("dtype", (torch.bfloat16, torch.float32), ids=("bf16", "fp32"))
def test_x_out_is_torchs_combine_bitwise(dev, dtype, R, V):
    c, u = _logits(dev, (R, V), dtype, 1), _logits(dev, (R, V), dtype, 2)
    q = SO.draws((R, V), device=dev)
    x = torch.full((R, V), 7.0, device=dev)
    idx = K.sample_topk_topp(c, q, SO.TOP_K, SO.TOP_P, uncond=u, w_cond=1 + T, w_uncond=T, x_out=x)
    assert torch.equal(x, (1 + T) * c.float() - T * u.float())
    assert idx.shape == (R,) and idx.dtype == torch.int64 and bool(((idx >= 0) & (idx < V)).all())
    x1 = torch.full((R, V), 7.0, device=dev)
    K.sample_topk_topp(c, q, SO.TOP_K, SO.TOP_P, x_out=x1)              # uncond=None: x is cond itself
    assert torch.equal(x1, c.float())


@pytest.mark.parametrize("dtype", (torch.bfloat16, torch.float32), ids=("bf16", "fp32"))
def test_blocked_rows_with_padded_stride(dev, dtype):
    """n = 2 blocks of rows_per_block = 3 in a [n, 2, rows, ld] head output whose rows are padded (ld = V + 8): the
    same x and tokens as the packed copy of the same values."""
    n, rows, V, ld = 2, 3, 1000, 1008
    buf = _logits(dev, (n, 2, rows, ld), dtype, 3)
    cond, uncond = buf[:, 0, :, :V], buf[:, 1, :, :V]
    q = SO.draws((n * rows, V), device=dev)
    x = torch.empty((n, rows, V), device=dev)
    idx = K.sample_topk_topp(cond, q, 300, SO.TOP_P, uncond=uncond, w_cond=1 + T, w_uncond=T, x_out=x)
    assert idx.shape == (n, rows)
    assert torch.equal(x, (1 + T) * cond.float() - T * uncond.float())
    packed = K.sample_topk_topp(cond.reshape(-1, V).contiguous(), q, 300, SO.TOP_P,
                                uncond=uncond.reshape(-1, V).contiguous(), w_cond=1 + T, w_uncond=T)
    assert torch.equal(idx.reshape(-1), packed)


# ---------------------------------------------------------------------------------------------------
# exact cases
# ---------------------------------------------------------------------------------------------------


def test_top_k_one_is_the_row_argmax(dev):
    x = _logits(dev, (257, 1000), torch.float32, 4)
    q = SO.draws(x.shape, device=dev)
    assert bool(((x == x.amax(-1, keepdim=True)).sum(-1) == 1).all())
    assert torch.equal(K.sample_topk_topp(x, q, 1, 0.0), x.argmax(-1))
    assert torch.equal(K.sample_topk_topp(x, q, 1, SO.TOP_P), x.argmax(-1))


@pytest.mark.parametrize("top_k", (0, 1000, 5000))
def test_no_masking_is_the_oracles_argmax(dev, top_k):
    """top_k >= V (or 0) with top-p off: argmax(softmax(x) / q) of the oracle, nothing masked."""
    x = _logits(dev, (257, 1000), torch.float32, 5)
    q = SO.draws(x.shape, device=dev)
    o = SO.oracle(x.cpu(), q.cpu(), 0, -1.0)
    assert bool(o["K_lo"].all())
    assert torch.equal(K.sample_topk_topp(x, q, top_k, 0.0).cpu(), o["exact"])


def test_an_all_equal_row_keeps_every_entry(dev):
    x = _logits(dev, (5, 1000), torch.bfloat16, 6)
    x[2] = 1.25
    q = SO.draws(x.shape, device=dev)
    idx = K.sample_topk_topp(x, q, 300, SO.TOP_P)
    assert int(idx[2]) == int(q[2].argmin())            # every p equal: the smallest draw wins, wherever it sits
    x[2, 17] = 1.5                                       # one maximum above a tie group of 999: C(group) is far
    idx = K.sample_topk_topp(x, q, 0, 0.5)               # above 0.5, so the whole group stays with it
    w = x[2].float().exp() / q[2]
    assert int(idx[2]) == int(w.argmax())


def test_a_large_p_cut_leaves_the_maximum_alone(dev):
    x = _logits(dev, (5, 1000), torch.float32, 7)
    q = SO.draws(x.shape, device=dev)
    q[:, :] = 1e3
    q[torch.arange(5, device=dev), x.argmin(-1)] = 1e-6      # the draws favour the smallest logit
    idx = torch.full((5,), -7, dtype=torch.int64, device=dev)
    _raw(x, None, 0, 1000, 5, 0, 1.0, 0.0, 5, 1000, 0, 2.0, q, 1000, idx, None, 0)    # p_cut = 2: every C is below it
    assert torch.equal(idx, x.argmax(-1))
    assert torch.equal(K.sample_topk_topp(x, q, 0, 1e-9), x.argmax(-1))     # float32(1 - 1e-9) = 1 >= every C


@pytest.mark.parametrize("dtype", (torch.bfloat16, torch.float32), ids=("bf16", "fp32"))
def test_bad_rows_give_minus_one_and_touch_nothing_else(dev, dtype):
    V = 1000
    c, u = _logits(dev, (7, V), dtype, 8), _logits(dev, (7, V), dtype, 9)
    q = SO.draws(c.shape, device=dev)
    x0 = torch.full((7, V), 7.0, device=dev)
    good = K.sample_topk_topp(c, q, 300, SO.TOP_P, uncond=u, w_cond=1 + T, w_uncond=T, x_out=x0)
    c[1, 999] = float("nan")
    c[3, 0] = float("inf")
    c[5] = float("-inf")
    u[5] = 0.0
    c[6, 5:900] = float("-inf")                          # -inf entries among finite ones: ordinary masked entries
    x = torch.full((7, V), 7.0, device=dev)
    idx = K.sample_topk_topp(c, q, 300, SO.TOP_P, uncond=u, w_cond=1 + T, w_uncond=T, x_out=x)
    assert idx[[1, 3, 5]].tolist() == [-1, -1, -1]
    assert torch.equal(idx[[0, 2, 4]], good[[0, 2, 4]]) and torch.equal(x[[0, 2, 4]], x0[[0, 2, 4]])
    assert bool((x[[1, 3, 5]] == 7.0).all())             # nothing else written for a bad row
    assert 0 <= int(idx[6]) < V and not (5 <= int(idx[6]) < 900)
    o = SO.oracle(x[6:7].cpu(), q[6:7].cpu(), 300, SO.p_cut_of(SO.TOP_P))
    assert bool(SO.admissible(o, x[6:7].cpu(), idx[6:7]).all())


# ---------------------------------------------------------------------------------------------------
# the recipe: admissibility, parity with the torch sampler, generator streams
# ---------------------------------------------------------------------------------------------------

CASES = [(s, SO.VOCAB, SO.TOP_K) for s in SO.SCALES] + [(s, 1000, 300) for s in SO.SCALES]


@lru_cache(maxsize=None)
def _case(s, V, top_k):
    """The recipe at scale s as a head output of n = 2 members ([2, 2, 1, 1024, V] bf16), through the kernel and
    through sample_population, each on its own pair of generators seeded alike; the oracle on the kernel's own q."""
    dev = torch.device("cuda:0")
    n, rows = 2, SO.ROWS // 2
    c, u, x = SO.recipe(s, SO.ROWS, V)
    head = torch.stack((c.view(n, rows, V), u.view(n, rows, V)), dim=1).to(dev).bfloat16().view(n, 2, 1, rows, V)
    gens = [torch.Generator(device=dev).manual_seed(SO.GEN_SEED) for _ in range(n)]
    tok, x_out = sample_population_native(head, T, gens, top_k, SO.TOP_P, keep_logits=True)
    ref_gens = [torch.Generator(device=dev).manual_seed(SO.GEN_SEED) for _ in range(n)]
    ref = sample_population(x_out.clone(), ref_gens, top_k, SO.TOP_P)
    q = SO.draws((rows, V), device=dev).cpu().repeat(n, 1)            # members seeded alike draw alike
    o = SO.oracle(x, q, top_k, SO.p_cut_of(SO.TOP_P))
    return {"x": x, "x_out": x_out.cpu().view(-1, V), "tok": tok.cpu().view(-1), "ref": ref.cpu().view(-1), "o": o,
            "states": [g.get_state() for g in gens], "ref_states": [g.get_state() for g in ref_gens], "head": head}


@pytest.mark.parametrize("s,V,top_k", CASES)
def test_every_token_is_admissible(dev, s, V, top_k):
    d = _case(s, V, top_k)
    assert torch.equal(d["x_out"], d["x"])               # the oracle judges the logits the kernel sampled
    adm = SO.admissible(d["o"], d["x"], d["tok"])
    print(f"[sampler s={s} V={V} k={top_k}] inadmissible {int((~adm).sum())} of {adm.numel()}; off the exact argmax "
          f"{int((d['tok'] != d['o']['exact']).sum())}; rows with K_lo != K_hi "
          f"{int((d['o']['K_lo'] != d['o']['K_hi']).any(-1).sum())}")
    assert bool(adm.all())


@pytest.mark.parametrize("s,V,top_k", CASES)
def test_parity_with_the_torch_sampler(dev, s, V, top_k):
    """Against sample_population on the same logits and generators seeded alike: at most 1 row in 500 differs, every
    differing row is admissible, and every generator ends in the state the torch path leaves it in."""
    d = _case(s, V, top_k)
    diff = d["tok"] != d["ref"]
    print(f"[sampler parity s={s} V={V} k={top_k}] rows that differ from torch: {int(diff.sum())} of {diff.numel()}")
    assert int(diff.sum()) * 500 <= diff.numel()
    assert bool(SO.admissible(d["o"], d["x"], d["tok"])[diff].all())
    for a, b in zip(d["states"], d["ref_states"]):
        assert torch.equal(a, b)


def test_deterministic_and_batch_invariant(dev):
    d = _case(2.0, SO.VOCAB, SO.TOP_K)
    head = d["head"]
    n, _, _, rows, V = head.shape
    gens = [torch.Generator(device=dev).manual_seed(SO.GEN_SEED) for _ in range(n)]
    again, _ = sample_population_native(head, T, gens, SO.TOP_K, SO.TOP_P)
    assert torch.equal(again.cpu().view(-1), d["tok"])
    q = SO.draws((rows, V), device=dev)
    ho = head.view(n, 2, rows, V)
    for k, r in ((0, 0), (0, 513), (1, 7), (1, rows - 1)):              # rows sampled alone
        one = K.sample_topk_topp(ho[k, 0, r:r + 1], q[r:r + 1], SO.TOP_K, SO.TOP_P, uncond=ho[k, 1, r:r + 1],
                                 w_cond=1 + T, w_uncond=T)
        assert int(one) == int(d["tok"][k * rows + r]), (k, r)


# ---------------------------------------------------------------------------------------------------
# refused calls
# ---------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("V,ld,what", ((4100, 4100, "V > 4096"), (1002, 1004, "V % 4"), (1000, 996, "ld < V")))
def test_refused_calls_write_nothing(dev, V, ld, what):
    R = 4
    c = _logits(dev, (R, 4104), torch.float32, 10)
    q = SO.draws((R, 4104), device=dev)
    idx = torch.full((R,), -7, dtype=torch.int64, device=dev)
    x = torch.full((R, 4104), 7.0, device=dev)
    with pytest.raises(_lib.EggrollError, match="sample_topk_topp"):
        _raw(c, None, 0, ld, R, 0, 1.0, 0.0, R, V, 0, -1.0, q, 4104, idx, x, 4104)
    torch.cuda.synchronize()
    assert bool((idx == -7).all()) and bool((x == 7.0).all()), what
    with pytest.raises(ValueError):
        K.sample_topk_topp(c[:, :1000], q[:, :999], 0, 0.0)              # the wrapper: q does not match cond


# ---------------------------------------------------------------------------------------------------
# wiring: VARPopulationInfer.native_sampler
# ---------------------------------------------------------------------------------------------------


def test_var_native_sampler_wiring(golden, dev, monkeypatch):
    """Free generation on the tiny VAR with native_sampler on: one kernel launch per scale, deterministic, and per
    scale its tokens pass the parity rule against sample_population (what native_sampler=False runs) on the same
    kept logits with generators in the same state; with it off the kernel is never called."""
    from hyperscalees_t2i_amd.lora import set_population
    from tests.test_var_model import ARCH, _build
    d = golden("g11_var_model.npz")
    cfg, top_k, top_p, g_seed = (float(d["meta"][0]), int(d["meta"][1]), float(d["meta"][2]), int(d["meta"][3]))
    gen, theta = _build(dev, d["theta"])
    assert gen.infer.native_sampler is True
    g = torch.Generator(device=dev).manual_seed(3)
    pop = torch.stack([theta, theta + 0.02 * torch.randn(theta.shape, generator=g, device=dev)])
    gen.ctx.theta_pop, gen.ctx.n_members = pop, 2
    set_population(gen.var, gen.ctx)                                    # what generate_population does around run()
    calls = []
    real = K.sample_topk_topp
    monkeypatch.setattr(K, "sample_topk_topp", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    labels = torch.tensor([3, 980], device=dev)
    n, B, V = 2, 2, ARCH.vocab_size
    f1, idx1, lg1 = gen.infer.run(labels, n, g_seed, cfg, top_k, top_p, keep_logits=True)
    assert len(calls) == len(ARCH.patch_nums)
    f2, idx2, _ = gen.infer.run(labels, n, g_seed, cfg, top_k, top_p)
    assert all(torch.equal(a, b) for a, b in zip(idx1, idx2)) and torch.equal(f1, f2)
    ref_gens = [torch.Generator(device=dev).manual_seed(g_seed) for _ in range(n)]
    q_gens = [torch.Generator(device=dev).manual_seed(g_seed) for _ in range(n)]
    rows = differ = 0
    for si, pn in enumerate(ARCH.patch_nums):
        l = pn * pn
        assert lg1[si].shape == (n, B, l, V) and idx1[si].shape == (n * B, l)
        ref = sample_population(lg1[si].clone(), ref_gens, top_k, top_p).reshape(-1).cpu()
        q = torch.stack([torch.empty(B * l, V, device=dev).exponential_(1, generator=g) for g in q_gens]).view(-1, V)
        tok, x = idx1[si].reshape(-1).cpu(), lg1[si].view(-1, V).cpu()
        diff = tok != ref
        if bool(diff.any()):
            o = SO.oracle(x[diff], q.cpu()[diff], top_k, SO.p_cut_of(top_p))
            assert bool(SO.admissible(o, x[diff], tok[diff]).all()), si
        rows, differ = rows + tok.numel(), differ + int(diff.sum())
    print(f"[var native sampler] rows that differ from sample_population: {differ} of {rows}")
    assert differ * 500 <= rows
    calls.clear()
    gen.infer.native_sampler = False
    _, idx3, _ = gen.infer.run(labels, n, g_seed, cfg, top_k, top_p)
    assert not calls and idx3[0].shape == idx1[0].shape


def test_var_nan_logits_raise_once_after_the_last_scale(golden, dev, monkeypatch):
    from tests.test_var_model import ARCH, _build
    d = golden("g11_var_model.npz")
    gen, _ = _build(dev, d["theta"])
    with torch.no_grad():
        gen.var.head.weight[5, 3] = float("nan")                        # logit 5 of every row is NaN
    gen.var.refresh()
    calls = []
    real = K.sample_topk_topp
    monkeypatch.setattr(K, "sample_topk_topp", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    with pytest.raises(RuntimeError) as e:
        gen.infer.run(torch.tensor([3, 980], device=dev), 1, 7, 4.0, 900, 0.95)
    assert str(e.value) == BAD_PROBS == "probability tensor contains either inf, nan or element < 0"
    assert len(calls) == len(ARCH.patch_nums)                            # raised after the last scale, not at the first
