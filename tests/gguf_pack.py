"""The oracle of tests/test_gguf.py and tests/test_gpu_gguf.py.  NOT a second dequantiser: a PACKER that lays
per-element integer fields (quants, sub-block scales and mins) and fp16 fields out as ggml block bytes, element
by element from the block layouts, and the closed-form VALUE of every element computed from those same fields
in numpy float32, one rounded operation at a time in ggml's order.  Nothing here unpacks a byte.

Fields are uniform over their full ranges; where a case has at least 64 slots of a 6-bit scale the first 64
take every value once.  fp16 fields come from a fixed list of finite values (zero, a subnormal, small, one,
large, both signs) — never a random bit pattern, so no NaN or inf occurs.
"""
import numpy as np

from hyperscalees_t2i_amd import gguf as G

f32 = np.float32
HALF_VALUES = np.array([0.0, 2.0 ** -24, -2.0 ** -24, 6.1e-5, -6.1e-5, 0.0123, -0.0123, 1.0, -1.0, 37.5, -37.5],
                       dtype=np.float16)
QUANT_TYPES = [G.Q4_0, G.Q4_1, G.Q5_0, G.Q5_1, G.Q8_0, G.Q2_K, G.Q3_K, G.Q4_K, G.Q5_K, G.Q6_K]
ALL_TYPES = [G.F32, G.F16, G.BF16] + QUANT_TYPES


def _halves(rng, nb, values):
    """One fp16 per block: the list in order first (so every value occurs once nb allows), then random picks."""
    values = np.asarray(values, dtype=np.float16)
    idx = rng.integers(0, len(values), nb)
    n = min(nb, len(values))
    idx[:n] = rng.permutation(len(values))[:n]
    return values[idx]


def _ints(rng, lo, hi, shape, exhaust=False):
    a = rng.integers(lo, hi + 1, shape)
    if exhaust and a.size >= hi - lo + 1:
        a.reshape(-1)[:hi - lo + 1] = np.arange(lo, hi + 1)
    return a.astype(np.int64)


def random_fields(t, nb, rng, half_values=HALF_VALUES):
    h = lambda: _halves(rng, nb, half_values)  # noqa: E731
    if t == G.F32:
        return {"v": rng.standard_normal(nb).astype(f32)}
    if t == G.F16:
        return {"v": np.concatenate([HALF_VALUES, rng.standard_normal(nb).astype(np.float16)])[:nb] if nb >= 11
                else rng.standard_normal(nb).astype(np.float16)}
    if t == G.BF16:
        bits = rng.integers(0, 1 << 16, nb).astype(np.uint16)
        bits[(bits & 0x7F80) == 0x7F80] &= 0xBFFF                     # no inf / NaN: clear one exponent bit
        return {"bits": bits}
    if t in (G.Q4_0, G.Q4_1, G.Q5_0, G.Q5_1):
        f = {"d": h(), "q": _ints(rng, 0, 31 if t in (G.Q5_0, G.Q5_1) else 15, (nb, 32))}
        if t in (G.Q4_1, G.Q5_1):
            f["m"] = h()
        return f
    if t == G.Q8_0:
        return {"d": h(), "q": _ints(rng, -128, 127, (nb, 32), exhaust=True)}
    if t == G.Q2_K:
        return {"d": h(), "dmin": h(), "sc": _ints(rng, 0, 15, (nb, 16), True), "mn": _ints(rng, 0, 15, (nb, 16), True),
                "q": _ints(rng, 0, 3, (nb, 256))}
    if t == G.Q3_K:
        return {"d": h(), "sc": _ints(rng, 0, 63, (nb, 16), True), "q": _ints(rng, 0, 3, (nb, 256)),
                "h": _ints(rng, 0, 1, (nb, 256))}
    if t in (G.Q4_K, G.Q5_K):
        return {"d": h(), "dmin": h(), "sc": _ints(rng, 0, 63, (nb, 8), True), "mn": _ints(rng, 0, 63, (nb, 8), True),
                "q": _ints(rng, 0, 31 if t == G.Q5_K else 15, (nb, 256), t == G.Q5_K)}
    if t == G.Q6_K:
        return {"d": h(), "sc": _ints(rng, -128, 127, (nb, 16), True), "q": _ints(rng, 0, 63, (nb, 256), True)}
    raise ValueError(t)


def _put_half(blk, off, v):
    blk[:, off:off + 2] = np.asarray(v, dtype="<f2").view(np.uint8).reshape(-1, 2)


def _scatter(blk, base, byte_of, shift_of, vals):
    """blk[:, base + byte_of[e]] |= vals[:, e] << shift_of[e] for every element e."""
    for e in range(vals.shape[1]):
        blk[:, base + byte_of[e]] |= (vals[:, e] << shift_of[e]).astype(np.uint8)


def _k23_pos():
    """Q2_K / Q3_K: element e of sub-block s = e // 16 lives in byte 32 n + 16 half + l at bit 2 k."""
    e = np.arange(256)
    s, l = e // 16, e % 16
    n, k, half = s // 8, (s % 8) // 2, s % 2
    return 32 * n + 16 * half + l, 2 * k


def _k45_pos():
    """Q4_K / Q5_K: element e of sub-block j = e // 32 lives in byte 32 (j // 2) + l, nibble j % 2."""
    e = np.arange(256)
    j, l = e // 32, e % 32
    return 32 * (j // 2) + l, 4 * (j % 2)


def _pack_k4_scales(blk, base, sc, mn):
    for j in range(8):
        if j < 4:
            blk[:, base + j] |= sc[:, j].astype(np.uint8)
            blk[:, base + j + 4] |= mn[:, j].astype(np.uint8)
        else:
            blk[:, base + j + 4] |= ((sc[:, j] & 15) | ((mn[:, j] & 15) << 4)).astype(np.uint8)
            blk[:, base + j - 4] |= ((sc[:, j] >> 4) << 6).astype(np.uint8)
            blk[:, base + j] |= ((mn[:, j] >> 4) << 6).astype(np.uint8)


def pack(t, f):
    """Fields -> raw block bytes (uint8 [n_blocks * type_size])."""
    if t == G.F32:
        return np.asarray(f["v"], dtype="<f4").view(np.uint8).copy()
    if t == G.F16:
        return np.asarray(f["v"], dtype="<f2").view(np.uint8).copy()
    if t == G.BF16:
        return np.asarray(f["bits"], dtype="<u2").view(np.uint8).copy()
    nb = f["q"].shape[0]
    blk = np.zeros((nb, G.GGML_TYPES[t][2]), dtype=np.uint8)
    q = f["q"]
    if t in (G.Q4_0, G.Q4_1, G.Q5_0, G.Q5_1):
        _put_half(blk, 0, f["d"])
        p = 2
        if t in (G.Q4_1, G.Q5_1):
            _put_half(blk, 2, f["m"])
            p = 4
        if t in (G.Q5_0, G.Q5_1):
            qh = np.zeros(nb, dtype=np.uint32)
            for e in range(32):                                        # bit e of the little-endian u32
                qh |= ((q[:, e] >> 4) << e).astype(np.uint32)
            blk[:, p:p + 4] = qh.astype("<u4").view(np.uint8).reshape(nb, 4)
            p += 4
        e = np.arange(32)
        _scatter(blk, p, e % 16, 4 * (e // 16), q & 15)
    elif t == G.Q8_0:
        _put_half(blk, 0, f["d"])
        blk[:, 2:] = q.astype(np.int8).view(np.uint8)
    elif t == G.Q2_K:
        blk[:, 0:16] = (f["sc"] | (f["mn"] << 4)).astype(np.uint8)
        _scatter(blk, 16, *_k23_pos(), q)
        _put_half(blk, 80, f["d"])
        _put_half(blk, 82, f["dmin"])
    elif t == G.Q3_K:
        e = np.arange(256)
        s = e // 16
        _scatter(blk, 0, 16 * (s % 2) + e % 16, s // 2, f["h"])         # hmask: bit s // 2 of byte 16 half + l
        _scatter(blk, 32, *_k23_pos(), q)
        sc = f["sc"]
        for j in range(16):                                             # the per-element form of the 12 scale bytes
            low, high = sc[:, j] & 15, sc[:, j] >> 4
            if j < 8:
                blk[:, 96 + j] |= low.astype(np.uint8)
            else:
                blk[:, 96 + j - 8] |= (low << 4).astype(np.uint8)
            blk[:, 96 + 8 + j % 4] |= (high << (2 * (j // 4))).astype(np.uint8)
        _put_half(blk, 108, f["d"])
    elif t in (G.Q4_K, G.Q5_K):
        _put_half(blk, 0, f["d"])
        _put_half(blk, 2, f["dmin"])
        _pack_k4_scales(blk, 4, f["sc"], f["mn"])
        if t == G.Q5_K:
            e = np.arange(256)
            _scatter(blk, 16, e % 32, e // 32, q >> 4)                  # qh: bit j of byte l
        _scatter(blk, 48 if t == G.Q5_K else 16, *_k45_pos(), q & 15)
    elif t == G.Q6_K:
        e = np.arange(256)
        n, quarter, l = e // 128, (e % 128) // 32, e % 32
        _scatter(blk, 0, 64 * n + 32 * (quarter % 2) + l, 4 * (quarter // 2), q & 15)
        _scatter(blk, 128, 32 * n + l, 2 * quarter, q >> 4)
        blk[:, 192:208] = f["sc"].astype(np.int8).view(np.uint8)
        _put_half(blk, 208, f["d"])
    else:
        raise ValueError(t)
    return blk.reshape(-1)


def _h(f, k):
    return np.asarray(f[k], dtype=np.float16).astype(f32)[:, None]


def formula(t, f):
    """Fields -> the value of every element, float32 [n_elems], each operation rounded to fp32 in order."""
    if t == G.F32:
        return np.asarray(f["v"], dtype=f32).copy()
    if t == G.F16:
        return np.asarray(f["v"], dtype=np.float16).astype(f32)
    if t == G.BF16:
        return (np.asarray(f["bits"], dtype=np.uint16).astype(np.uint32) << 16).view(f32)
    q = f["q"]
    nb = q.shape[0]
    if t == G.Q4_0:
        y = (q - 8).astype(f32) * _h(f, "d")
    elif t == G.Q5_0:
        y = (q - 16).astype(f32) * _h(f, "d")
    elif t in (G.Q4_1, G.Q5_1):
        y = q.astype(f32) * _h(f, "d") + _h(f, "m")
    elif t == G.Q8_0:
        y = q.astype(f32) * _h(f, "d")
    elif t == G.Q2_K:
        dl = _h(f, "d") * f["sc"].astype(f32)
        ml = _h(f, "dmin") * f["mn"].astype(f32)
        y = dl[:, :, None] * q.reshape(nb, 16, 16).astype(f32) - ml[:, :, None]
    elif t == G.Q3_K:
        dl = _h(f, "d") * (f["sc"] - 32).astype(f32)
        y = dl[:, :, None] * (q - 4 * (1 - f["h"])).reshape(nb, 16, 16).astype(f32)
    elif t in (G.Q4_K, G.Q5_K):
        dl = _h(f, "d") * f["sc"].astype(f32)
        ml = _h(f, "dmin") * f["mn"].astype(f32)
        y = dl[:, :, None] * q.reshape(nb, 8, 32).astype(f32) - ml[:, :, None]
    elif t == G.Q6_K:
        dl = _h(f, "d") * f["sc"].astype(f32)
        y = dl[:, :, None] * (q - 32).reshape(nb, 16, 16).astype(f32)
    else:
        raise ValueError(t)
    assert y.dtype == f32
    return y.reshape(-1)


def n_elems(t, nb):
    return nb * G.GGML_TYPES[t][1]


def case(t, nb, seed, half_values=HALF_VALUES):
    """(raw bytes, expected float32 values) of nb random blocks."""
    f = random_fields(t, nb, np.random.default_rng(seed), half_values)
    return pack(t, f), formula(t, f)
