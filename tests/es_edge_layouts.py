"""Theta layouts and populations shared by tests/test_es_edges.py (CPU) and tests/test_gpu_es_edges.py.

ThetaLayout does not pad theta_off, so the ORDER of KINDS is deliberate: the aligned shapes come first
and the first odd-sized parameter, (5, 7), misaligns every theta_off after it."""
import numpy as np

from hyperscalees_t2i_amd.kernels import ThetaLayout

KINDS = [(1, 8), (2, 1028), (4, 12), (4, 4), (8, 1), (1032, 2), (12, 4), (8,), (1028,), (3, 8), (8, 3), (2, 6),
         (6, 2), (5, 7), (40, 30), (7,), (2, 8), (16,), (1, 1)]

# (kind, NU, tiles) of every KINDS entry at egg rank 1, 2 and 4; at rank 3 every matrix is generic.
#   wide / tall at NU 1, 2, 4 ((4, 4) is wide by the rows <= cols tie-break), two of them with a second
#   tile that holds a single active thread (1028 = 1024 + 4); vec4 with one and with two tiles;
#   gen because a short dimension is 3 / the long dimension is no multiple of 4 / theta_off is
#   misaligned ((2, 8) and (1, 1)), once with two chunks ((40, 30)); vec because the length is no
#   multiple of 4 ((7,)) and because theta_off is misaligned ((16,)).
KINDS_FAST = [("wide", 1, 1), ("wide", 2, 2), ("wide", 4, 1), ("wide", 4, 1), ("tall", 1, 1), ("tall", 2, 2),
              ("tall", 4, 1), ("vec4", 1, 1), ("vec4", 1, 2), ("gen", 0, 1), ("gen", 0, 1), ("gen", 0, 1),
              ("gen", 0, 1), ("gen", 0, 1), ("gen", 0, 2), ("vec", 0, 1), ("gen", 0, 1), ("vec", 0, 1),
              ("gen", 0, 1)]
KINDS_RANK3 = [k if k[0] in ("vec4", "vec") else ("gen", 0, -(-(s[0] * s[1]) // 1024))   # 1024-element chunks
               for k, s in zip(KINDS_FAST, KINDS)]

# The aligned shapes of KINDS with the two 2-tile matrices shortened: 10 tiles and 1196 floats per copy.
MANY = [(1, 8), (2, 8), (4, 12), (4, 4), (8, 1), (8, 2), (12, 4), (8,), (1028,)]
# perturb splits the members of one call over grid.y while n_tiles < 4096, in groups of >= 16 members:
#   MANY_MID (2400 + 23 tiles): 130 members in one call run as two groups of 65, so every workgroup's lane loop
#     (64 members per pass) runs twice, with a single member in pass two; 131 members: groups of 66 and 65.
#   MANY_BIG (4600 + 23 tiles): no split, every workgroup walks all 130 (131) members in three passes.
# Both end with KINDS (still aligned there: 1196 % 4 == 0), so every tile kind also runs with more than 64
# members in one workgroup -- on its own the 23-tile KINDS layout is always split into groups of < 32 members.
MANY_MID = MANY * 240 + KINDS
MANY_BIG = MANY * 460 + KINDS

# (pop, antithetic): n_base 64 (the lane-group boundary); 65 with the unpaired member as base 64 = lane 0 of
# group 1; 66; 70 without antithetic pairs; 300 (past the 256 threads that fill k_update's s_c).
POPS = [(128, True), (129, True), (131, True), (70, False), (600, True)]
RANKS = [1, 2, 3, 4]


def same_bits(a, b):
    """Equal bit for bit, the sign of a zero included; any NaN equals any NaN (payload and sign of a NaN
    differ between instruction sets)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.int32), b[~nb].view(np.int32)))


FIT_KEYS = ("scores", "mu", "stats", "fitness", "finite", "order")


def assert_fitness_equal(got, ref, tag):
    for k in FIT_KEYS:
        assert same_bits(got[k], ref[k]), f"{tag}/{k}"


def tile_kind(m, n, toff, foff, r):
    """(kind, NU, tiles): include/eggroll.h's tile rule restated (common.h egg_tile_kind / egg_tile_count)."""
    al = toff % 4 == 0 and foff % 4 == 0
    if n == 0:
        return ("vec4", 1, -(-m // 1024)) if (al and m % 4 == 0) else ("vec", 0, -(-m // 1024))
    rok = r in (1, 2, 4)
    if rok and al and m <= n and m in (1, 2, 4) and n % 4 == 0:
        return ("wide", m, -(-n // 1024))
    if rok and al and n < m and n in (1, 2, 4) and m % 4 == 0:
        return ("tall", n, -(-m // 1024))
    return ("gen", 0, -(-(m * n) // 1024))


def layout_kinds(lay):
    return [tile_kind(m, n, toff, foff, lay.rank) for m, n, toff, foff, _, _ in lay.mats.tolist()]


def shifted_layout(shapes, rank):
    """(aligned layout, layout whose factor_off % 4 runs through 1, 2, 3 over the parameters, copy function).

    include/eggroll.h accepts factor offsets that are no multiples of 4 (they run the per-element path);
    ThetaLayout never produces one, so parameter i's factor block is moved up by 4 i + 1 + i % 3 floats here,
    before the layout has cached its tile table or a device copy of its records.  copy(fac) moves the factor
    values of an aligned-layout buffer [p, >= factor_len] to their shifted positions."""
    al = ThetaLayout(shapes, rank)
    sh = ThetaLayout(shapes, rank)
    shift = np.array([4 * i + 1 + i % 3 for i in range(sh.n_mats)], dtype=np.int64)
    sh.mats[:, 3] += shift
    lens = np.diff(np.append(al.mats[:, 3], al.factor_len))        # padded block length per parameter
    assert all(sh.mats[i, 3] + lens[i] <= sh.mats[i + 1, 3] for i in range(sh.n_mats - 1))
    sh.factor_len = int(sh.mats[-1, 3] + lens[-1])
    sh.factor_ld = -(-sh.factor_len // 4) * 4
    sh._segments = None                                            # pack / unpack do not apply to this layout
    assert sorted(set((sh.mats[:, 3] % 4).tolist())) == [1, 2, 3]

    def copy(fac):
        out = np.zeros((fac.shape[0], sh.factor_ld), np.float32)
        for i in range(al.n_mats):
            a, s = int(al.mats[i, 3]), int(sh.mats[i, 3])
            out[:, s:s + lens[i]] = fac[:, a:a + lens[i]]
        return out
    return al, sh, copy


# ------------------------------------------------------------------------------------------- fitness inputs
# (n, m): n m = 4096 is the last size k_fitness stages in LDS, (1025, 4) the first it reads from global
# memory; n > 1024 runs the thread-strided loops more than once; m up to the 1024-prompt limit.
FIT_SHAPES_LOOP = [(1024, 4), (1025, 4), (4096, 1), (4096, 3), (3, 1024)]       # checked against O.dev_fitness
FIT_SHAPES_FAST = [(1500, 1024), (4096, 1024)]                                  # against O.dev_fitness_fast
PLANTED = ["dups_far", "block50", "zeros", "infs", "nan3", "one_finite", "none_finite"]
PLANTED_N = 2100


def fitness_input(n, m):
    rng = np.random.default_rng(1000 * n + m)
    return (rng.standard_normal((n, m)) + 20).astype(np.float32)


def planted_input(case):
    """S [2100, 2] for mean scoring with one planted hazard of the rank sort / the finite mask."""
    n = PLANTED_N
    S = fitness_input(n, 2)
    if case == "dups_far":            # equal scores 1100 rows apart: different threads AND different passes
        for k in (3, 500, 999):
            S[k + 1100] = S[k]
    elif case == "block50":
        S[1000:1050] = S[1000]
    elif case == "zeros":             # scores +0.0 and -0.0 (the latter by underflow of -2^-149 / 2) compare equal
        S[::2] -= 20                  # half of the other scores below zero, half above
        S[[5, 1029, 2050]] = 0.0
        S[[7, 1031, 2051]] = -0.0
        S[[9, 1500]] = np.array([-1e-45, 0.0], np.float32)
    elif case == "infs":
        S[[4, 1200]] = np.inf
        S[[6, 2099]] = -np.inf
    elif case == "nan3":
        S[[0, 1024, 2099], [0, 1, 0]] = np.nan
    elif case == "one_finite":        # N_f = 1: the unbiased std is NaN
        S[:] = np.nan
        S[1234] = (1.5, 2.5)
    elif case == "none_finite":
        S[:, 0] = np.nan
        S[::3, 1] = np.inf
    else:
        raise KeyError(case)
    return S
