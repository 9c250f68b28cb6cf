"""A/B of two or more builds of libeggroll on the five softmax-attention entry points (eggroll_cross_attention,
eggroll_flash_attention, eggroll_relbias_attention, eggroll_softcap_attention, eggroll_causal_attention) through
the package's own wrappers: the global library handle is swapped between the bound builds.

Bitwise: every output must equal the first build's on the seeded inputs of the kernel tests (test_gpu_kernels.py
flash / cross, test_gpu_t5.py, test_gpu_gemma2.py, test_gpu_qwen3.py, their lens-edge cases included), for flash
qf 1, 2 and 4 and for cross variants 1 and 2, and on the epoch's shapes below.
Timing: the epoch's shapes on the default variant / qf, the builds interleaved in one process, HIP events on the
launch stream around `it` launches, median of rounds.  Give the parent library twice (the file and a byte copy)
ahead of the branch: the largest per-round deviation of A against A per shape is the noise the branch's median is
judged by.

Build A first: `python tools/lib_ab.py build-a <rev>`.
usage: python tools/attn_lib_ab.py <libA.so> [<copy of libA.so>] <libB.so> [--out FILE.json] [--rounds N]"""
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from hyperscalees_t2i_amd import _lib  # noqa: E402
from hyperscalees_t2i_amd import kernels as K  # noqa: E402
from es_lib_ab import bind, timed  # noqa: E402

FLASH_TEST = [(2, 676, 676, 3, False), (3, 1, 1, 2, False), (2, 100, 2521, 2, True), (1, 257, 130, 1, True),
              (4, 64, 64, 2, False), (2, 100, 200, 2, False)]
CROSS_TEST = [(4, 64, 2, 37, 2, 112), (3, 100, 3, 300, 3, 112), (6, 17, 1, 320, 2, 112), (16, 1024, 20, 300, 4, 112),
              (2, 33, 2, 160, 2, 112), (2, 33, 2, 161, 2, 112), (2, 65, 2, 129, 2, 128), (2, 257, 16, 257, 2, 80),
              (8, 36, 4, 77, 4, 128), (6, 145, 2, 256, 3, 128), (5, 1, 3, 20, 2, 128)]
CROSS_EPOCH = [(128, 1024, 20, 112, 300, 4), (128, 257, 16, 80, 257, 128), (128, 50, 12, 64, 50, 128)]  # B N heads hd L U
RELBIAS_TEST = [(3, 37, 3, [37, 1, 20], 37, False, 1.0), (2, 64, 1, [64, 16], 70, False, 1.0),
                (2, 65, 2, [65, 33], 65, True, 1.0), (1, 512, 2, [512], 512, False, 1.0),
                (2, 512, 1, [129, 511], 512, True, 0.125)]
SOFTCAP_TEST = [(3, 37, 4, 2, [37, 1, 20], 5.0, False), (2, 64, 2, 2, [64, 16], 5.0, False),
                (2, 65, 8, 4, [65, 33], 50.0, True), (1, 1, 2, 1, [1], 5.0, False), (1, 300, 8, 4, [300], 50.0, False),
                (2, 300, 4, 1, [129, 299], 0.0, False)]
CAUSAL_TEST = [(3, 37, 4, 2, [37, 1, 20], False), (2, 64, 2, 2, [64, 16], False), (2, 65, 8, 2, [65, 33], True),
               (1, 1, 2, 1, [1], False), (1, 129, 4, 4, [129], False), (2, 300, 8, 2, [129, 299], True),
               (1, 130, 3, 1, [130], False)]
LENS_EDGES = ([0, 20, 3], [-4, 99, 3])   # B 3, N 20; the second one device-resident (clamped in the kernel)


def flash_case(dev, B, Nq, Lk, H, strided, qf):
    g = torch.Generator(device=dev).manual_seed(Nq * 7 + Lk)
    q = (torch.randn(B, Nq, H, 128, generator=g, device=dev) * 0.3).bfloat16()
    if strided:
        cache = (torch.randn(2, B, Lk + 37, H * 128, generator=g, device=dev) * 0.3).bfloat16()
        k, v = cache[0, :, :Lk].view(B, Lk, H, 128), cache[1, :, :Lk].view(B, Lk, H, 128)
    else:
        k = (torch.randn(B, Lk, H, 128, generator=g, device=dev) * 0.3).bfloat16()
        v = torch.randn(B, Lk, H, 128, generator=g, device=dev).bfloat16()
    return lambda: K.flash_attention(q, k, v, 128 ** -0.5 * 3, qf=qf)


def flash_epoch(dev, g, B, N, H, qf):
    q, k, v = ((torch.randn(B, N, H, 128, device=dev, generator=g) * 0.5).bfloat16() for _ in range(3))
    return lambda: K.flash_attention(q, k, v, 128 ** -0.5, qf=qf)


def with_variant(variant, fn):
    def run():
        old, K.XATTN_VARIANT = K.XATTN_VARIANT, variant
        try:
            return fn()
        finally:
            K.XATTN_VARIANT = old
    return run


def cross_test(dev, B, N, H, L, U, hd):
    g = torch.Generator(device=dev).manual_seed(B * 131 + L)
    q = torch.randn((B * N, H * hd), generator=g, device=dev).to(torch.bfloat16)
    if hd == 128:
        kv = torch.randn((U * L, 2 * H * hd), generator=g, device=dev).to(torch.bfloat16)
        k, v = kv[:, :H * hd], kv[:, H * hd:]
    else:
        k = torch.randn((U * L, H * hd), generator=g, device=dev).to(torch.bfloat16)
        v = torch.randn((U * L, H * hd), generator=g, device=dev).to(torch.bfloat16)
    lens = [L] + [int(x) for x in torch.randint(1, L + 1, (U - 1,), generator=g, device=dev).tolist()]
    bias = torch.zeros((U, L), device=dev, dtype=torch.bfloat16)
    for u, n_valid in enumerate(lens):
        bias[u, n_valid:] = float("-inf") if hd == 128 else -10000.0
    enc = torch.arange(B, device=dev) % U if hd != 128 else torch.randint(0, U, (B,), generator=g, device=dev)
    return lambda: K.cross_attention(q, k, v, B, N, H, hd, L, hd ** -0.5, bias=bias, enc_index=enc)


def cross_epoch(dev, g, B, N, heads, hd, L, U):
    q = torch.randn(B * N, heads * hd, device=dev, generator=g).bfloat16()
    k = torch.randn(U * L, heads * hd, device=dev, generator=g).bfloat16()
    v = torch.randn(U * L, heads * hd, device=dev, generator=g).bfloat16()
    cross = U != B   # Sana attn2: masked captions shared through enc_index; the CLIP towers: self-attention
    bias = torch.where(torch.rand(U, L, device=dev, generator=g) < 0.2, -1e4, 0.0).bfloat16() if cross else None
    enc = (torch.arange(B, device=dev, dtype=torch.int32) // (B // U)).contiguous() if cross else None
    return lambda: K.cross_attention(q, k, v, B, N, heads, hd, L, hd ** -0.5, bias=bias, enc_index=enc)


def qkv(dev, B, N, Hq, Hkv, hd, sliced, seed, std=1.0):
    """q / k / v as the encoder tests build them; also returns the generator (the T5 table is drawn next)."""
    g = torch.Generator(device=dev).manual_seed(seed)
    if sliced:   # column slices of one fused qkv GEMM output
        t = (torch.randn((B * N, (Hq + 2 * Hkv) * hd), generator=g, device=dev) * std).to(torch.bfloat16)
        return t[:, :Hq * hd], t[:, Hq * hd:(Hq + Hkv) * hd], t[:, (Hq + Hkv) * hd:], g
    q, k, v = [(torch.randn((B * N, h * hd), generator=g, device=dev) * std).to(torch.bfloat16) for h in (Hq, Hkv, Hkv)]
    return q, k, v, g


def relbias_case(dev, B, N, H, lens, R, sliced, scale, seed):
    q, k, v, g = qkv(dev, B, N, H, H, 64, sliced, seed, 0.5)
    table = torch.randn((H, 2 * R - 1), generator=g, device=dev)
    return lambda: K.relbias_attention(q, k, v, table, lens, B, N, H, scale)


def softcap_case(dev, B, N, Hq, Hkv, lens, cap, sliced, seed):
    q, k, v, _ = qkv(dev, B, N, Hq, Hkv, 256, sliced, seed)
    return lambda: K.softcap_attention(q, k, v, lens, B, N, Hq, Hkv, 0.6 * cap / 16.0 if cap > 0 else 1.0 / 16.0, cap)


def causal_case(dev, B, N, Hq, Hkv, lens, sliced, seed):
    q, k, v, _ = qkv(dev, B, N, Hq, Hkv, 128, sliced, seed)
    return lambda: K.causal_attention(q, k, v, lens, B, N, Hq, Hkv, 128 ** -0.5)


def cases(dev):
    """name -> (fn, timed)."""
    out = {}
    for c in FLASH_TEST:
        for qf in (1, 2, 4):
            out[f"flash test {c} qf{qf}"] = (flash_case(dev, *c, qf), False)
    for c in CROSS_TEST:
        for var in (1, 2):
            out[f"cross test {c} variant{var}"] = (with_variant(var, cross_test(dev, *c)), False)
    for name, table, make in (("relbias", RELBIAS_TEST, relbias_case), ("softcap", SOFTCAP_TEST, softcap_case),
                              ("causal", CAUSAL_TEST, causal_case)):
        for c in table:
            c = list(c)
            li = 3 if name == "relbias" else 4
            lens, c[li] = c[li], torch.tensor(c[li])
            out[f"{name} test B{c[0]} N{c[1]} lens{lens}"] = (make(dev, *c, seed=c[1] * 7 + c[0]), False)
    for i, lens in enumerate(LENS_EDGES):
        lt = torch.tensor(lens, device=dev if i else "cpu")
        out[f"relbias lens {lens}"] = (relbias_case(dev, 3, 20, 2, lt, 20, False, 1.0, seed=9), False)
        out[f"softcap lens {lens}"] = (softcap_case(dev, 3, 20, 2, 1, lt, 5.0, False, seed=9), False)
        out[f"causal lens {lens}"] = (causal_case(dev, 3, 20, 2, 1, lt, False, seed=9), False)
    # the epoch's shapes: bitwise on every variant / qf, timed on the default one
    g = torch.Generator(device=dev).manual_seed(2)
    for c in CROSS_EPOCH:
        fn = cross_epoch(dev, g, *c)
        key = "B{} N{} h{}x{} L{}".format(*c[:5])
        out[f"cross {key}"] = (fn, c[0] * c[1] > 10000)   # Sana attn2 and CLIP-H (CLIP-B/32: bitwise only)
        for var in (1, 2):
            out[f"cross {key} variant{var}"] = (with_variant(var, fn), False)
    g = torch.Generator(device=dev).manual_seed(0)
    for Bf, Nf, Hf in ((4, 4608, 30), (2, 1000, 8)):   # Z-Image's joint sequence; a ragged one
        for qf in (0, 1, 4):
            out[f"flash {Bf}x{Nf} h{Hf} qf{qf}"] = (flash_epoch(dev, g, Bf, Nf, Hf, qf), qf == 0 and Nf == 4608)
    full = lambda B, N: torch.full((B,), N, dtype=torch.int32, device=dev)  # noqa: E731
    out["causal 8x128 h32/8"] = (causal_case(dev, 8, 128, 32, 8, full(8, 128), True, seed=1), True)    # Qwen3-4B heads
    out["causal 8x512 h32/8"] = (causal_case(dev, 8, 512, 32, 8, full(8, 512), True, seed=2), True)
    out["softcap 8x300 h8/4"] = (softcap_case(dev, 8, 300, 8, 4, full(8, 300), 50.0, True, seed=3), True)  # Gemma-2-2B
    out["relbias B16 N80 h32"] = (relbias_case(dev, 16, 80, 32, full(16, 80), 128, True, 1.0, seed=4), True)
    return out


def main(paths, rounds=9, out_file=None):
    libs = [bind(p) for p in paths]
    dev = torch.device("cuda:0")
    res = {"libraries": [str(p) for p in paths], "rounds": rounds, "bitwise": {}, "timing_us": {}}
    for name, (fn, is_timed) in cases(dev).items():
        outs = []
        for lib in libs:
            _lib._lib = lib
            outs.append(fn().clone())
        torch.cuda.synchronize()
        same = all(torch.equal(outs[0], o) for o in outs[1:])
        res["bitwise"][name] = same
        print(json.dumps({name: same}), flush=True)
        assert same, name
        if not is_timed:
            continue
        us = [[] for _ in libs]
        for _ in range(rounds):
            for i, lib in enumerate(libs):
                _lib._lib = lib
                us[i].append(timed(fn, it=20))
        med = [statistics.median(u) for u in us]
        row = {"median": [round(m, 2) for m in med], "min": [round(min(u), 2) for u in us],
               "max": [round(max(u), 2) for u in us]}
        if len(libs) == 3:   # A, a copy of A, B.  The noise: how far one round's A2 / A strays from 1 (the ratio of
            # the two medians alone can be exactly 0); B is judged by its median against A's
            spread = max(abs(a2 / a - 1.0) for a, a2 in zip(us[0], us[1]))
            row.update(A_vs_A_medians=round(med[1] / med[0] - 1.0, 4), A_vs_A_spread=round(spread, 4),
                       B_vs_A=round(med[2] / med[0] - 1.0, 4), within_spread=bool(abs(med[2] / med[0] - 1.0) <= spread))
        res["timing_us"][name] = row
        print(json.dumps({name: row}), flush=True)
    res["all_bitwise_equal"] = all(res["bitwise"].values())
    res["n_bitwise_cases"] = len(res["bitwise"])
    if out_file:
        Path(out_file).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps({"all_bitwise_equal": res["all_bitwise_equal"], "cases": res["n_bitwise_cases"]}))


if __name__ == "__main__":
    args = sys.argv[1:]
    opt = {}
    for flag in ("--out", "--rounds"):
        if flag in args:
            i = args.index(flag)
            opt[flag] = args[i + 1]
            del args[i:i + 2]
    main(args, rounds=int(opt.get("--rounds", 9)), out_file=opt.get("--out"))
