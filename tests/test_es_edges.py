"""CPU side of the ES-engine edge tests (tests/test_gpu_es_edges.py runs the kernels):
  * the KINDS layout really holds every tile kind it is meant to hold, at every egg rank;
  * the vectorised fitness oracle is bit-identical to the loop form it stands in for at the large shapes;
  * the fp32 error bound of the update test holds for an fp32 emulation of the update (so a kernel that
    misses it is wrong, not unlucky), and a dropped base sample exceeds it more than tenfold;
  * every ES entry point rejects bad arguments with -1 and a message, before any launch."""
import numpy as np
import pytest

from hyperscalees_t2i_amd import _lib
from hyperscalees_t2i_amd.kernels import ThetaLayout
from oracle import eggroll_oracle as O
from tests import es_edge_layouts as L


same_bits, assert_fitness_equal = L.same_bits, L.assert_fitness_equal


# ------------------------------------------------------------------------------------------------ layouts
@pytest.mark.parametrize("rank", L.RANKS)
def test_kinds_layout_holds_every_tile_kind(rank):
    lay = ThetaLayout(L.KINDS, rank)
    want = L.KINDS_RANK3 if rank == 3 else L.KINDS_FAST
    assert L.layout_kinds(lay) == want
    tiles = lay.tile_table()                                    # the library's own table agrees
    assert [int((tiles[:, 0] == i).sum()) for i in range(lay.n_mats)] == [k[2] for k in want]
    toff = lay.mats[:, 2]
    assert all(t % 4 == 0 for t in toff[:14]) and all(t % 4 != 0 for t in toff[14:])
    assert lay.D == 6631


@pytest.mark.parametrize("rank", [1, 2, 4])
def test_many_layouts_sit_on_both_sides_of_the_perturb_split(rank):
    mid, big = ThetaLayout(L.MANY_MID, rank), ThetaLayout(L.MANY_BIG, rank)
    assert 2048 < mid.n_tiles < 4096 and big.n_tiles >= 4096
    n = len(L.KINDS)
    assert all(k[0] in ("wide", "tall", "vec4") for k in L.layout_kinds(mid)[:-n])
    assert L.layout_kinds(mid)[-n:] == L.KINDS_FAST and L.layout_kinds(big)[-n:] == L.KINDS_FAST


@pytest.mark.parametrize("rank", L.RANKS)
def test_shifted_layout_moves_every_factor_block_off_alignment(rank):
    al, sh, copy = L.shifted_layout(L.KINDS, rank)
    assert all(k[0] in ("vec", "gen") for k in L.layout_kinds(sh))
    assert sh.n_tiles == sum(k[2] for k in L.layout_kinds(sh))
    fac = np.arange(2 * al.factor_ld, dtype=np.float32).reshape(2, -1)
    moved = copy(fac)
    for i in range(al.n_mats):
        m, n = al.mats[i, 0], al.mats[i, 1]
        ln = (m + n) * rank if n else m
        a, s = al.mats[i, 3], sh.mats[i, 3]
        assert np.array_equal(moved[:, s:s + ln], fac[:, a:a + ln])
        if n:   # b starts pad4(rows * r) after a in both layouts
            p = -(-m * rank // 4) * 4
            assert np.array_equal(moved[:, s + p:s + p + n * rank], fac[:, a + p:a + p + n * rank])


# ------------------------------------------------------------------------------------------------ fitness
def test_fast_fitness_oracle_equals_loop_form_on_golden(golden):
    npz = golden("g2_fitness.npz")
    names = sorted({k.split("/", 1)[0] for k in npz.files if k.endswith("/S")})
    assert names
    for name in names:
        for pn in (True, False):
            assert_fitness_equal(O.dev_fitness_fast(npz[name + "/S"], pn), O.dev_fitness(npz[name + "/S"], pn),
                                 f"{name}/{pn}")


@pytest.mark.parametrize("n,m", L.FIT_SHAPES_LOOP)
def test_fast_fitness_oracle_equals_loop_form(n, m):
    S = L.fitness_input(n, m)
    for pn in (True, False):
        assert_fitness_equal(O.dev_fitness_fast(S, pn), O.dev_fitness(S, pn), f"{n}x{m}/{pn}")


@pytest.mark.parametrize("case", L.PLANTED)
def test_fast_fitness_oracle_equals_loop_form_planted(case):
    S = L.planted_input(case)
    with np.errstate(invalid="ignore"):         # inf - inf in the column means
        ref = O.dev_fitness(S, False)
    assert_fitness_equal(O.dev_fitness_fast(S, False), ref, case)
    assert sorted(ref["order"].tolist()) == list(range(L.PLANTED_N))
    nf = {"nan3": L.PLANTED_N - 3, "infs": L.PLANTED_N - 4, "one_finite": 1, "none_finite": 0}.get(case, L.PLANTED_N)
    assert ref["stats"][1] == nf
    if case == "zeros":
        assert (np.signbit(ref["scores"]) & (ref["scores"] == 0)).sum() == 2        # the two underflowed rows
        assert ((ref["scores"] == 0) & ~np.signbit(ref["scores"])).sum() == 6
    if case == "one_finite":
        assert np.isnan(ref["stats"][3]) and np.isnan(ref["fitness"][1234])


# ------------------------------------------------------------------------------------------------ update bound
def _update_case(pop, anti, rank, seed):
    rng = np.random.default_rng(seed)
    lay = ThetaLayout(L.KINDS, rank)
    nb = O.n_base_samples(pop, anti)
    fac = rng.standard_normal((nb, lay.factor_len_packed)).astype(np.float32)
    theta = (rng.standard_normal(lay.D) * 0.02).astype(np.float32)
    fit = O.dev_fitness_fast((rng.standard_normal((pop, 4)) + 20).astype(np.float32), True)
    return lay, nb, fac, theta, fit["fitness"], int(fit["stats"][1])


@pytest.mark.parametrize("pop,anti,rank", [(129, True, 1), (131, True, 2), (70, False, 4), (600, True, 3),
                                           (600, True, 4)])
def test_update_bound_holds_for_an_fp32_emulation(pop, anti, rank):
    """The bound of test_gpu_es_edges' update test is derived, not measured; here the derivation is checked
    on the reference alone: a sequential fp32 emulation of the update stays inside it, with room."""
    lr = 1e-3
    lay, nb, fac, theta, f, nf = _update_case(pop, anti, rank, pop + rank)
    for th in (theta, np.zeros_like(theta)):
        ref, A = O.ref_update_f64(th, fac, L.KINDS, f, nf, pop, rank, anti, lr)
        emu = O.dev_update_generic(th, fac, L.KINDS, f, nf, pop, rank, anti, lr)
        bound = O.update_bound(ref, A, nb, rank, lr, nf)
        ratio = np.abs(emu.astype(np.float64) - ref) / bound
        print(f"pop {pop} rank {rank} theta {'0' if not th.any() else 'randn'}: max err / bound = {ratio.max():.4f}")
        assert ratio.max() <= 1.0
    # detection power: one base sample left out of the sum moves the step far outside the bound
    ref, A = O.ref_update_f64(np.zeros_like(theta), fac, L.KINDS, f, nf, pop, rank, anti, lr)
    g = f.copy()
    j = nb // 2
    g[j] = 0
    if anti and j < pop // 2:
        g[j + pop // 2] = 0
    ref2, _ = O.ref_update_f64(np.zeros_like(theta), fac, L.KINDS, g, nf, pop, rank, anti, lr)
    miss = np.abs(ref2 - ref) / O.update_bound(ref, A, nb, rank, lr, nf)
    assert np.median(miss) > 10


def test_caps_reference_scales():
    rng = np.random.default_rng(0)
    th, step = rng.standard_normal(1000) * 0.02, rng.standard_normal(1000) * 3e-4
    out, ss, ts = O.ref_caps_f64(th, th + step, 0.0, 0.0)
    assert ss == ts == 1.0 and np.array_equal(out, th + step)
    dn = np.linalg.norm(step)
    out, ss, ts = O.ref_caps_f64(th, th + step, 0.5 * dn, 0.0)
    assert abs(ss - 0.5) < 1e-5 and ts == 1.0 and abs(np.linalg.norm(out - th) - 0.5 * dn) < 1e-7
    out, ss, ts = O.ref_caps_f64(th, th + step, 2 * dn, 0.5 * np.linalg.norm(th + step))
    assert ss == 1.0 and abs(ts - 0.5) < 1e-5 and abs(np.linalg.norm(out) - 0.5 * np.linalg.norm(th + step)) < 1e-7


# ------------------------------------------------------------------------------------------------ rejections
P = 4096            # a well-aligned dummy pointer: every call below must return before it is dereferenced


def _perturb(lib, seeded=False, **kw):
    a = dict(theta=P, factors=P, ld_f=64, n_base=4, mats=P, tiles=P, n_tiles=1, D=16, rank=1, pop=8, anti=1, lo=0,
             hi=8, sigma=0.01, out=P, ld_out=16)
    a.update(kw)
    if seeded:
        return lib.eggroll_perturb_seeded(7, a["theta"], a["mats"], a["tiles"], a["n_tiles"], a["D"], a["rank"],
                                          a["pop"], a["anti"], a["lo"], a["hi"], a["sigma"], a["out"], a["ld_out"],
                                          None)
    return lib.eggroll_perturb(a["theta"], a["factors"], a["ld_f"], a["n_base"], a["mats"], a["tiles"], a["n_tiles"],
                               a["D"], a["rank"], a["pop"], a["anti"], a["lo"], a["hi"], a["sigma"], a["out"],
                               a["ld_out"], None)


def _update(lib, seeded=False, **kw):
    a = dict(theta=P, factors=P, ld_f=64, n_base=4, fit=P, stats=P, pop=8, anti=1, mats=P, tiles=P, n_tiles=1, D=16,
             rank=1, lr=1e-3, ms=0.0, mt=0.0, ws=P, out=2 * P)
    a.update(kw)
    if seeded:
        return lib.eggroll_update_seeded(7, a["theta"], a["fit"], a["stats"], a["pop"], a["anti"], a["mats"],
                                         a["tiles"], a["n_tiles"], a["D"], a["rank"], a["lr"], a["ms"], a["mt"],
                                         a["ws"], a["out"], None)
    return lib.eggroll_update(a["theta"], a["factors"], a["ld_f"], a["n_base"], a["fit"], a["stats"], a["pop"],
                              a["anti"], a["mats"], a["tiles"], a["n_tiles"], a["D"], a["rank"], a["lr"], a["ms"],
                              a["mt"], a["ws"], a["out"], None)


PERTURB_BAD = [dict(hi=9),                                          # member_hi > pop
               dict(lo=5, hi=4),                                    # member_lo > member_hi
               dict(lo=-1),
               dict(ld_out=15),                                     # ld_out < D
               dict(out=None), dict(mats=None), dict(tiles=None),
               dict(pop=200000, n_base=100000, hi=65536),           # more than 65535 members in one call
               dict(rank=0),
               dict(n_tiles=0)]
PERTURB_STORED_BAD = [dict(factors=P + 4),                          # factors not 16-byte aligned
                      dict(ld_f=62),                                # ld_f % 4 != 0
                      dict(factors=None),
                      dict(n_base=3),                               # pop 8 antithetic needs 4 base samples
                      dict(anti=0, n_base=7)]


@pytest.mark.parametrize("kw", PERTURB_BAD + PERTURB_STORED_BAD, ids=str)
def test_perturb_rejects(kw):
    lib = _lib.load()
    assert _perturb(lib, **kw) == -1, kw
    assert b"perturb:" in lib.eggroll_last_error(), kw


@pytest.mark.parametrize("kw", PERTURB_BAD, ids=str)
def test_perturb_seeded_rejects(kw):
    lib = _lib.load()
    assert _perturb(lib, seeded=True, **kw) == -1, kw
    assert b"perturb" in lib.eggroll_last_error(), kw


UPDATE_BAD = [dict(out=P),                                          # theta_out == theta
              dict(ws=P + 8),                                       # workspace not 16-byte aligned
              dict(pop=40000, n_base=20000),                        # n_base > 16384
              dict(rank=0), dict(pop=0), dict(ws=None), dict(stats=None), dict(n_tiles=0)]
UPDATE_STORED_BAD = [dict(n_base=5), dict(n_base=3),                # n_base != need_base
                     dict(factors=P + 4), dict(ld_f=62), dict(factors=None)]


@pytest.mark.parametrize("kw", UPDATE_BAD + UPDATE_STORED_BAD, ids=str)
def test_update_rejects(kw):
    lib = _lib.load()
    assert _update(lib, **kw) == -1, kw
    assert b"update:" in lib.eggroll_last_error(), kw


@pytest.mark.parametrize("kw", UPDATE_BAD, ids=str)
def test_update_seeded_rejects(kw):
    lib = _lib.load()
    assert _update(lib, seeded=True, **kw) == -1, kw
    assert b"update" in lib.eggroll_last_error(), kw


def test_fitness_noise_tile_table_reject():
    lib = _lib.load()
    for n, m, eps in ((4097, 4, 1e-8), (64, 1025, 1e-8), (64, 4, -1.0), (0, 4, 1e-8), (64, 0, 1e-8)):
        assert lib.eggroll_fitness(P, n, m, 1, eps, P, P, P, P, P, P, None) == -1, (n, m, eps)
        assert b"fitness:" in lib.eggroll_last_error()
    assert lib.eggroll_fitness(P, 64, 4, 1, 1e-8, P, P, P, P, P, None, None) == -1     # order is NULL
    assert b"fitness:" in lib.eggroll_last_error()
    assert lib.eggroll_noise_factors(0, 0, 65536, 16, 16, P, None) == -1            # more than 65535 base samples
    assert b"noise_factors:" in lib.eggroll_last_error()
    assert lib.eggroll_noise_factors(0, 3, 2, 16, 16, P, None) == -1
    assert lib.eggroll_noise_factors(0, 0, 2, 16, 16, None, None) == -1
    for rows, cols in ((0, 4), (-3, 0), (4, -1)):
        mats = np.array([[2, 8, 0, 0, 0, 0], [rows, cols, 16, 16, 1, 0]], dtype=np.int64)
        assert lib.eggroll_tile_table(mats.ctypes.data, 2, 1, None, 0) == -1, (rows, cols)
        assert b"tile_table:" in lib.eggroll_last_error()
    assert lib.eggroll_tile_table(None, 1, 1, None, 0) == -1
