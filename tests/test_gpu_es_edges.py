"""ES kernels (noise -> perturb -> fitness -> update) past the corner the rest of the suite stays in: more
than 64 base samples / members per workgroup (the second pass of the lane-group loops), every tile kind
against an independent reference at every egg rank, caller buffers and factor offsets that are not 16-byte
aligned, the fitness kernel at its size limits and on ties / non-finite scores.

Bars: perturb bit for bit against the kernel-order oracle (O.dev_eps_rows / O.ref_perturb); the fitness
kernel bit for bit against O.dev_fitness (loop form) or O.dev_fitness_fast (pinned equal to it in
tests/test_es_edges.py); the update against an fp64 evaluation of the same fp32 factors and fitness within
O.update_bound, a bound derived from sequential fp32 summation (tests/test_es_edges.py shows an fp32
emulation uses at most ~40 % of it with a random theta and ~7 % with theta = 0, and that one dropped base
sample exceeds it more than tenfold).  Layouts and populations: tests/es_edge_layouts.py."""
import functools

import numpy as np
import pytest
import torch

from hyperscalees_t2i_amd import kernels as K
from oracle import eggroll_oracle as O
from tests import es_edge_layouts as L

pytestmark = pytest.mark.gpu

SEED = 2 ** 40 + 77           # both Philox key words non-zero
SIGMA, LR = 0.01, 1e-3
SENTINEL = -1234.5
FILL = 4096               # one-tile parameters that lift a layout past the perturb split (n_tiles >= 4096)


def _np(t):
    return t.detach().cpu().numpy()


def _build_case(shapes_name, pop, anti, rank, dev):
    """Layout, stored factors (device + reference order on the host), a theta and reward rows."""
    shapes = {"kinds": L.KINDS, "mid": L.MANY_MID, "big": L.MANY_BIG}[shapes_name]
    lay = K.ThetaLayout(shapes, rank)
    nb = K.n_base_samples(pop, anti)
    fac = K.noise_factors(SEED, nb, lay, dev)
    g = torch.Generator().manual_seed(1000 * pop + rank)
    theta = (torch.randn(lay.D, generator=g) * 0.02).to(dev)
    S = (torch.randn(pop, 4, generator=g) + 20).to(dev)
    return dict(shapes=shapes, lay=lay, nb=nb, fac=fac, fac_np=lay.unpack_factors(_np(fac)), theta=theta, S=S)


_case = functools.lru_cache(maxsize=None)(_build_case)     # the KINDS cases are small and shared by the tests


def _singles(c, pop, anti, seeded, dev):
    """Every member's row from a call of its own, stacked."""
    lay = c["lay"]
    out = torch.empty((pop, -(-lay.D // 4) * 4), dtype=torch.float32, device=dev)[:, :lay.D]
    for k in range(pop):
        if seeded:
            K.perturb_seeded(c["theta"], SEED, lay, pop, anti, k, k + 1, SIGMA, dev, out=out[k:k + 1])
        else:
            K.perturb(c["theta"], c["fac"], lay, pop, anti, k, k + 1, SIGMA, out=out[k:k + 1])
    return out


# ---------------------------------------------------------------------------------------------- 1. perturb
@pytest.mark.parametrize("rank", L.RANKS)
@pytest.mark.parametrize("pop,anti", L.POPS)
def test_perturb_every_kind_bit_exact(dev, pop, anti, rank):
    c = _case("kinds", pop, anti, rank, dev)
    lay, fac, theta = c["lay"], c["fac"], c["theta"]
    eps_ref = O.dev_eps_rows(c["fac_np"], L.KINDS, pop, rank, anti, 0, pop)
    eps = K.perturb(None, fac, lay, pop, anti, 0, pop, 1.0)
    np.testing.assert_array_equal(_np(eps), eps_ref)
    # the whole population in one call: split over grid.y into groups of 16 or 17 members, the last one ragged
    full = K.perturb(theta, fac, lay, pop, anti, 0, pop, SIGMA)
    np.testing.assert_array_equal(_np(full), O.ref_perturb(_np(theta)[None, :], eps_ref, SIGMA))
    assert torch.equal(K.perturb_seeded(None, SEED, lay, pop, anti, 0, pop, 1.0, dev), eps)
    assert torch.equal(K.perturb_seeded(theta, SEED, lay, pop, anti, 0, pop, SIGMA, dev), full)
    assert torch.equal(K.perturb_seeded(theta, SEED, lay, pop, anti, 1, pop - 2, SIGMA, dev), full[1:pop - 2])
    assert torch.equal(K.perturb(theta, fac, lay, pop, anti, pop - 31, pop, SIGMA), full[pop - 31:])  # 31: one group
    assert torch.equal(_singles(c, pop, anti, False, dev), full)
    # The same factors behind FILL four-float parameters: with n_tiles >= 4096 the call is not split, so each
    # workgroup walks all `pop` members, 64 per pass of its lane loop (3 to 10 passes).  Offsets move by a
    # multiple of 4, so every parameter keeps its tile kind and must reproduce the rows checked above.
    layb = K.ThetaLayout([(4,)] * FILL + L.KINDS, rank)
    assert layb.n_tiles >= 4096 and L.layout_kinds(layb)[FILL:] == L.layout_kinds(lay)
    assert layb.factor_ld == 4 * FILL + fac.shape[1] and np.array_equal(layb.mats[FILL:, 3], lay.mats[:, 3] + 4 * FILL)
    g = torch.Generator().manual_seed(pop + rank)
    ff, tf = torch.randn(c["nb"], 4 * FILL, generator=g), torch.randn(4 * FILL, generator=g) * 0.02
    facb, thetab = torch.cat([ff.to(dev), fac], 1), torch.cat([tf.to(dev), theta])
    big = K.perturb(thetab, facb, layb, pop, anti, 0, pop, SIGMA)
    assert torch.equal(big[:, 4 * FILL:], full)
    jb, sg = zip(*(O.member_to_base(k, pop, anti) for k in range(pop)))
    eps_f = ff.numpy()[list(jb)] * np.array(sg, np.float32)[:, None]
    np.testing.assert_array_equal(_np(big[:, :4 * FILL]), O.ref_perturb(tf.numpy()[None, :], eps_f, SIGMA))
    own = K.noise_factors(SEED, c["nb"], layb, dev)
    assert torch.equal(K.perturb_seeded(thetab, SEED, layb, pop, anti, 0, pop, SIGMA, dev),
                       K.perturb(thetab, own, layb, pop, anti, 0, pop, SIGMA))


# ---------------------------------------------------------------------------------------------- 2. lane groups
@pytest.mark.parametrize("rank", [1, 2, 4])
@pytest.mark.parametrize("pop,anti", [(131, True), (70, False)])
@pytest.mark.parametrize("size", ["mid", "big"])
def test_perturb_lane_groups(dev, size, pop, anti, rank):
    """More than 64 members in one workgroup (see the split arithmetic at MANY_MID / MANY_BIG): the one-call
    result equals the single-member calls for every member, and the oracle on a sample of members (the numpy
    oracle walks ~4000 matrices per member)."""
    c = _build_case(size, pop, anti, rank, dev)     # not cached: these factor buffers are a few hundred MB
    lay, fac, theta = c["lay"], c["fac"], c["theta"]
    assert (2048 < lay.n_tiles < 4096) if size == "mid" else lay.n_tiles >= 4096
    full = K.perturb(theta, fac, lay, pop, anti, 0, pop, SIGMA)
    assert torch.equal(K.perturb_seeded(theta, SEED, lay, pop, anti, 0, pop, SIGMA, dev), full)
    if pop == 131:   # 130 members: mid runs groups of 65 (64 + 1 lanes), big 64 + 64 + 2
        assert torch.equal(K.perturb(theta, fac, lay, pop, anti, 1, pop, SIGMA), full[1:])
        assert torch.equal(K.perturb_seeded(theta, SEED, lay, pop, anti, 1, pop, SIGMA, dev), full[1:])
    for seeded in (False, True):
        assert torch.equal(_singles(c, pop, anti, seeded, dev), full), seeded
    th = _np(theta)
    for k in sorted({0, 63, 64, 65, pop // 2, pop - 1}):
        ref = O.ref_perturb(th, O.dev_eps_rows(c["fac_np"], c["shapes"], pop, rank, anti, k, k + 1)[0], SIGMA)
        np.testing.assert_array_equal(_np(full[k]), ref, err_msg=f"member {k}")


# ---------------------------------------------------------------------------------------------- 3. update
def _fitness_checked(S, promptnorm):
    fit = K.fitness(S, promptnorm)
    L.assert_fitness_equal({k: _np(v) for k, v in fit.items()}, O.dev_fitness(_np(S), promptnorm), "fitness")
    return fit, _np(fit["fitness"]), int(fit["stats"][1].item())


def _f32(x):
    return float(np.float32(x))


def _check_update(c, fit, f_np, nf, pop, anti, rank, theta, dev, tag):
    """Uncapped, capped (both caps derived from the REFERENCE so that both trigger) and with caps that do not
    trigger; stored and seeded.  Returns the largest |error| / bound of the uncapped update."""
    lay, fac = c["lay"], c["fac"]
    th = _np(theta).astype(np.float64)
    ref, A = O.ref_update_f64(_np(theta), c["fac_np"], c["shapes"], f_np, nf, pop, rank, anti, LR)
    bound = O.update_bound(ref, A, c["nb"], rank, LR, nf)
    out = K.update(theta, fac, fit, lay, pop, anti, LR, 0.0, 0.0)
    ratio = float((np.abs(_np(out).astype(np.float64) - ref) / bound).max())
    print(f"update err/bound {tag}: {ratio:.4f}")
    assert ratio <= 1.0, tag
    assert torch.equal(K.update_seeded(theta, SEED, fit, lay, pop, anti, LR, 0.0, 0.0), out), tag
    # caps that trigger: half the reference's step norm, then half the norm of what the step cap leaves
    ms = _f32(0.5 * np.linalg.norm(ref - th))
    mt = _f32(0.5 * np.linalg.norm(O.ref_caps_f64(th, ref, ms, 0.0)[0]))
    refc, ss, ts = O.ref_caps_f64(th, ref, ms, mt)
    assert ss < 0.51 and ts < 0.51
    outc = K.update(theta, fac, fit, lay, pop, anti, LR, ms, mt)
    tol = bound * ss * ts + 2.0 ** -21 * (np.abs(th) + np.abs(refc))
    rc = float((np.abs(_np(outc).astype(np.float64) - refc) / tol).max())
    print(f"update err/bound {tag} capped: {rc:.4f}")
    assert rc <= 1.0, tag
    assert torch.equal(K.update_seeded(theta, SEED, fit, lay, pop, anti, LR, ms, mt), outc), tag
    # caps at twice the reference's norms: neither triggers, and the capped kernels change no bit
    ms2, mt2 = _f32(2 * np.linalg.norm(ref - th)), _f32(2 * np.linalg.norm(ref))
    refn, ss, ts = O.ref_caps_f64(th, ref, ms2, mt2)
    assert ss == 1.0 and ts == 1.0
    outn = K.update(theta, fac, fit, lay, pop, anti, LR, ms2, mt2)
    assert float((np.abs(_np(outn).astype(np.float64) - refn) / (bound + 2.0 ** -21 * (np.abs(th) + np.abs(refn)))).max()) <= 1.0
    assert torch.equal(outn, out), tag
    assert torch.equal(K.update_seeded(theta, SEED, fit, lay, pop, anti, LR, ms2, mt2), out), tag
    return ratio


@pytest.mark.parametrize("rank", L.RANKS)
@pytest.mark.parametrize("pop,anti", L.POPS)
def test_update_vs_fp64(dev, pop, anti, rank):
    c = _case("kinds", pop, anti, rank, dev)
    fit, f_np, nf = _fitness_checked(c["S"], True)
    assert nf == pop
    for name, theta in (("zero", torch.zeros_like(c["theta"])), ("randn", c["theta"])):   # zero: the step itself
        _check_update(c, fit, f_np, nf, pop, anti, rank, theta, dev, f"rank {rank} pop {pop} theta {name}")


def test_update_vs_fp64_big_layout(dev):
    pop, anti, rank = 131, True, 4
    c = _build_case("big", pop, anti, rank, dev)
    fit, f_np, nf = _fitness_checked(c["S"], True)
    _check_update(c, fit, f_np, nf, pop, anti, rank, c["theta"], dev, "big layout rank 4 pop 131")


# ---------------------------------------------------------------------------------------------- 4. non-finite
@pytest.mark.parametrize("rank", L.RANKS)
def test_update_nonfinite_members_large_population(dev, rank):
    pop, anti = 131, True
    h = pop // 2
    c = _case("kinds", pop, anti, rank, dev)
    lay, fac, theta = c["lay"], c["fac"], c["theta"]
    S = c["S"].clone()
    S[[3, h + 3, h + 10, 2 * h], [0, 1, 2, 3]] = float("nan")   # a whole pair, half a pair, the unpaired member
    fit, f_np, nf = _fitness_checked(S, False)
    assert fit["stats"][1].item() == 127 and nf == 127
    assert not f_np[[3, h + 3, h + 10, 2 * h]].any()
    ref, A = O.ref_update_f64(_np(theta), c["fac_np"], L.KINDS, f_np, nf, pop, rank, anti, LR)
    for out in (K.update(theta, fac, fit, lay, pop, anti, LR, 0.0, 0.0),
                K.update_seeded(theta, SEED, fit, lay, pop, anti, LR, 0.0, 0.0)):
        assert (np.abs(_np(out).astype(np.float64) - ref) <= O.update_bound(ref, A, c["nb"], rank, LR, nf)).all()
    # promptnorm: one NaN poisons every score -> no finite member -> theta comes back untouched, caps or not
    fit, _, nf = _fitness_checked(S, True)
    assert nf == 0
    tn = float(theta.norm())
    for ms, mt in ((0.0, 0.0), (1e-6, 0.5 * tn)):
        assert torch.equal(K.update(theta, fac, fit, lay, pop, anti, LR, ms, mt), theta)
        assert torch.equal(K.update_seeded(theta, SEED, fit, lay, pop, anti, LR, ms, mt), theta)


# ---------------------------------------------------------------------------------------------- 5. unaligned buffers
def _sentinel_buf(n, dev):
    return torch.full((n,), SENTINEL, dtype=torch.float32, device=dev)


def _untouched_outside(buf, view):
    """Every float of buf outside `view` (a strided window into it) still holds the sentinel."""
    mask = torch.ones(buf.shape, dtype=torch.bool, device=buf.device)
    torch.as_strided(mask, view.shape, view.stride(), view.storage_offset() - buf.storage_offset()).fill_(False)
    assert int(mask.sum()) == buf.numel() - view.numel()
    return bool((buf[mask] == SENTINEL).all())


@pytest.mark.parametrize("seeded", [False, True], ids=["stored", "seeded"])
@pytest.mark.parametrize("rank", L.RANKS)
def test_unaligned_caller_buffers(dev, rank, seeded):
    """theta / out / theta_out off 16-byte alignment, or an out row stride that is no multiple of 4, select the
    scalar-access instantiations: same bits as the aligned call, and not one float written outside the rows."""
    pop, anti = 131, True
    c = _case("kinds", pop, anti, rank, dev)
    lay, fac, theta, D = c["lay"], c["fac"], c["theta"], c["lay"].D

    def perturb(th, sigma, out=None):
        if seeded:
            return K.perturb_seeded(th, SEED, lay, pop, anti, 0, pop, sigma, dev, out=out)
        return K.perturb(th, fac, lay, pop, anti, 0, pop, sigma, out=out)

    def update(th, ms, mt, out=None):
        if seeded:
            return K.update_seeded(th, SEED, fit, lay, pop, anti, LR, ms, mt, out=out)
        return K.update(th, fac, fit, lay, pop, anti, LR, ms, mt, out=out)

    full, eps = perturb(theta, SIGMA), perturb(None, 1.0)
    tbuf = _sentinel_buf(D + 8, dev)
    tbuf[1:1 + D] = theta
    tbuf0 = tbuf.clone()
    theta_u = tbuf[1:1 + D]
    assert theta_u.data_ptr() % 16 == 4 and theta.data_ptr() % 16 == 0
    for ld, off, th, want in ((D + 1, 1, theta_u, full), (D + 3, 1, theta_u, full), (D + 3, 1, theta, full),
                              (D + 1, 1, None, eps), (D + 1, 0, theta, full),        # aligned base, odd stride
                              (-(-D // 4) * 4 + 8, 0, theta_u, full),                # only theta unaligned
                              (-(-D // 4) * 4 + 8, 0, theta, full)):                 # all aligned: the vector path
        obuf = _sentinel_buf(off + pop * ld + 8, dev)
        out = torch.as_strided(obuf, (pop, D), (ld, 1), off)
        perturb(th, SIGMA if th is not None else 1.0, out=out)
        assert torch.equal(out, want), (ld, off)
        assert _untouched_outside(obuf, out), (ld, off)
    assert torch.equal(tbuf, tbuf0)

    fit = K.fitness(c["S"], True)
    tn = float(theta.norm())
    for ms, mt in ((0.0, 0.0), (2e-4, 0.5 * tn)):
        want = update(theta, ms, mt)
        for th, off in ((theta_u, 1), (theta, 1), (theta_u, 0)):
            obuf = _sentinel_buf(D + 8, dev)
            out = obuf[off:off + D]
            update(th, ms, mt, out=out)
            assert torch.equal(out, want), (ms, mt, off)
            assert _untouched_outside(obuf, out), (ms, mt, off)
    assert torch.equal(tbuf, tbuf0)


# ---------------------------------------------------------------------------------------------- 6. factor offsets
@pytest.mark.parametrize("rank", L.RANKS)
def test_unaligned_factor_offsets(dev, rank):
    """include/eggroll.h: factor offsets that are no multiples of 4 "are accepted and run the per-element
    path".  eps does not depend on the tile kind, so perturb must reproduce the aligned layout's bits from
    the same factor values at shifted offsets; the update sums in another order and is held to the fp64 bound."""
    pop, anti = 131, True
    c = _case("kinds", pop, anti, rank, dev)
    theta, nb = c["theta"], c["nb"]
    al, sh, copy = L.shifted_layout(L.KINDS, rank)
    fac_sh = torch.from_numpy(copy(_np(c["fac"]))).to(dev)
    assert torch.equal(K.perturb(theta, fac_sh, sh, pop, anti, 0, pop, SIGMA),
                       K.perturb(theta, c["fac"], al, pop, anti, 0, pop, SIGMA))
    assert torch.equal(K.perturb(None, fac_sh, sh, pop, anti, 0, pop, 1.0),
                       K.perturb(None, c["fac"], al, pop, anti, 0, pop, 1.0))
    fit, f_np, nf = _fitness_checked(c["S"], True)
    ref, A = O.ref_update_f64(_np(theta), c["fac_np"], L.KINDS, f_np, nf, pop, rank, anti, LR)
    out = K.update(theta, fac_sh, fit, sh, pop, anti, LR, 0.0, 0.0)
    assert (np.abs(_np(out).astype(np.float64) - ref) <= O.update_bound(ref, A, nb, rank, LR, nf)).all()
    # regenerated factors: element g of the factor vector is the same Philox draw wherever a block starts
    own = K.noise_factors(SEED, nb, sh, dev)
    assert torch.equal(K.perturb_seeded(theta, SEED, sh, pop, anti, 0, pop, SIGMA, dev),
                       K.perturb(theta, own, sh, pop, anti, 0, pop, SIGMA))
    tn = float(theta.norm())
    for ms, mt in ((0.0, 0.0), (2e-4, 0.5 * tn)):
        assert torch.equal(K.update_seeded(theta, SEED, fit, sh, pop, anti, LR, ms, mt),
                           K.update(theta, own, fit, sh, pop, anti, LR, ms, mt))


# ---------------------------------------------------------------------------------------------- 7. fitness
def _check_fitness(dev, S, promptnorm, ref, tag):
    got = {k: _np(v) for k, v in K.fitness(torch.from_numpy(S).to(dev), promptnorm).items()}
    n = S.shape[0]
    assert sorted(got["order"].tolist()) == list(range(n)), f"{tag}: order is no permutation"
    L.assert_fitness_equal(got, ref, tag)
    if np.isfinite(got["scores"]).all():
        assert np.array_equal(got["order"], np.argsort(got["scores"], kind="stable")), tag


@pytest.mark.parametrize("promptnorm", [True, False], ids=["pn", "mean"])
@pytest.mark.parametrize("n,m", L.FIT_SHAPES_LOOP + L.FIT_SHAPES_FAST)
def test_fitness_at_its_limits(dev, n, m, promptnorm):
    S = L.fitness_input(n, m)
    oracle = O.dev_fitness if (n, m) in L.FIT_SHAPES_LOOP else O.dev_fitness_fast
    _check_fitness(dev, S, promptnorm, oracle(S, promptnorm), f"{n}x{m}")


@pytest.mark.parametrize("case", L.PLANTED)
def test_fitness_planted_ties_and_nonfinite(dev, case):
    S = L.planted_input(case)
    with np.errstate(invalid="ignore"):
        ref = O.dev_fitness(S, False)
    _check_fitness(dev, S, False, ref, case)
