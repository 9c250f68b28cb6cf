"""Per-scale A/B of Infinity's sampling tail, from the head GEMM's bf16 output to (bits, codes), at the bench shape
(Infinity-8B, pn 0.25M: 4 members x 16 images, d_tok 56 with spatial patchify, micro_batch 2, ten scales) and at the
reference's default preset (Infinity-2B, pn 1M: d_tok 32, no patchify, thirteen scales, micro_batch 0 and 2): the torch
op chain of InfinityPopulationInfer.run with native_sampler off (`.float()`, `/ tau`, the CFG combine,
ChunkedBitSampler.sample with one sample_bits call per chunk and member, bits_to_codes) against the native path (one
ChunkedBitDraws fill plus the one eggroll_sample_bits launch) and against that launch alone on ready draws.  HIP
events around `--iters` calls after one warm-up call, median of `--rounds` rounds.  Also counts the bits that differ
between the two paths on generators seeded alike.

usage: python tools/infinity_sampler_ab.py [--out FILE.json] [--rounds N] [--iters N]"""
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from hyperscalees_t2i_amd import kernels as K  # noqa: E402
from hyperscalees_t2i_amd.infinity import (SCALE_SIDES, ChunkedBitDraws, ChunkedBitSampler, InfinityArch,  # noqa: E402
                                           bits_to_codes)

N, B = 4, 16
TAU, CFG, TOP_K, TOP_P = 1.0, 3.0, 900, 0.97
# (name, pn, codebook_dim, spatial_patchify, micro_batch)
PRESETS = [("8b_0.25M_mb2", "0.25M", 14, 1, 2), ("2b_1M_mb0", "1M", 32, 0, 0), ("2b_1M_mb2", "1M", 32, 0, 2)]


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3      # us per call


def main(out_file=None, rounds=3, iters=3):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    res = {"shape": {"members": N, "images_per_member": B, "tau": TAU, "cfg": CFG, "top_k": TOP_K, "top_p": TOP_P},
           "rounds": rounds, "calls_per_round": iters, "presets": {}}
    for name, pn, cd, patchify, micro_batch in PRESETS:
        a = InfinityArch(codebook_dim=cd, spatial_patchify=patchify)
        d = a.d_tok
        mb = B if micro_batch <= 0 or micro_batch >= B else micro_batch
        rows = []

        def gen(seed=5):
            return torch.Generator(device=dev).manual_seed(seed)

        for si, side in enumerate(SCALE_SIDES[pn]):
            h = w = side
            l = h * w
            head = (torch.randn(N * 2 * B * l, 2 * d, generator=g, device=dev) * 2.0).bfloat16()
            bad = torch.zeros(1, dtype=torch.int32, device=dev)

            def torch_chain(sampler):
                lg = head.float().view(N, 2, B, l * d, 2) / TAU
                lg = CFG * lg[:, 0] + (1.0 - CFG) * lg[:, 1]
                bits = sampler.sample(lg, TOP_K, TOP_P).view(N * B, l, d)
                return bits, bits_to_codes(bits, a, h, w)

            def native_chain(draws):
                q = draws.fill(torch.empty((B, l * d, 2), dtype=torch.float32, device=dev))
                return K.sample_bits(head, q, N, B, h, w, d, TAU, CFG, TOP_K, TOP_P, bool(patchify), bad)

            st, sn = ChunkedBitSampler(gen(), B, mb), ChunkedBitDraws(gen(), B, mb)
            q = torch.empty((B, l * d, 2), device=dev).exponential_(1, generator=g)
            bt, ct = torch_chain(ChunkedBitSampler(gen(), B, mb))
            bn, cn = native_chain(ChunkedBitDraws(gen(), B, mb))
            row = {"scale": si, "side": side, "bits": N * B * l * d,
                   "torch_tail_us": round(statistics.median(timed(lambda: torch_chain(st), iters)
                                                            for _ in range(rounds)), 1),
                   "native_tail_us": round(statistics.median(timed(lambda: native_chain(sn), iters)
                                                             for _ in range(rounds)), 1),
                   "launch_alone_us": round(statistics.median(
                       timed(lambda: K.sample_bits(head, q, N, B, h, w, d, TAU, CFG, TOP_K, TOP_P, bool(patchify), bad),
                             iters) for _ in range(rounds)), 1),
                   "bits_differing": int((bt != bn).sum()), "codes_differing": int((ct != cn).sum()),
                   "bad": int(bad.item()), "bytes_moved": N * B * l * d * (2 * 2 * 2 + 8 + 4) + B * l * d * 8}
            rows.append(row)
            print(name, json.dumps(row), flush=True)
            del head, q, bt, ct, bn, cn
        sums = {k: round(sum(r[k] for r in rows), 1) for k in rows[0] if k.endswith("_us")}
        sums["bits_differing"] = sum(r["bits_differing"] for r in rows)
        res["presets"][name] = {"pn": pn, "d_tok": d, "spatial_patchify": patchify, "micro_batch": micro_batch,
                                "scales": rows, "sum_over_scales": sums}
        print(name, json.dumps(sums), flush=True)
    if out_file:
        Path(out_file).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    args = sys.argv[1:]
    opt = {}
    for flag in ("--out", "--rounds", "--iters"):
        if flag in args:
            i = args.index(flag)
            opt[flag] = args[i + 1]
            del args[i:i + 2]
    main(out_file=opt.get("--out"), rounds=int(opt.get("--rounds", 3)), iters=int(opt.get("--iters", 3)))
