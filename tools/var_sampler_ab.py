"""Per-scale A/B of VAR's sampling tail at the VAR-d16 bench shape (pop 4 x 16 images: n * B = 64, rows 64 * pn^2 of
V = 4096 at the ten scales): the torch op chain of VARPopulationInfer.run with native_sampler off, from the `.float()`
of the head GEMM's bf16 output through the CFG combine, top-k / top-p masking, softmax and one torch.multinomial per
member, against sample_population_native (the n exponential fills plus the one eggroll_sample_topk_topp launch) and
against that launch alone on ready draws.  HIP events around `--iters` calls after one warm-up call, median of
`--rounds` rounds; the torch path's host syncs (one `.item()` per multinomial) are inside its window, as they are
inside an epoch's.  Also counts the rows whose token differs between the two paths on generators seeded alike.

usage: python tools/var_sampler_ab.py [--out FILE.json] [--rounds N] [--iters N]"""
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from hyperscalees_t2i_amd import kernels as K  # noqa: E402
from hyperscalees_t2i_amd.var import VAR_D16, sample_population, sample_population_native  # noqa: E402

N, B, V = 4, 16, VAR_D16.vocab_size
CFG, TOP_K, TOP_P = 4.0, 900, 0.95


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


def main(out_file=None, rounds=3, iters=5):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    SN = len(VAR_D16.patch_nums)
    res = {"shape": {"members": N, "images_per_member": B, "vocab": V, "cfg": CFG, "top_k": TOP_K, "top_p": TOP_P},
           "rounds": rounds, "calls_per_round": iters, "scales": []}

    def gens(seed=5):
        return [torch.Generator(device=dev).manual_seed(seed) for _ in range(N)]

    for si, pn in enumerate(VAR_D16.patch_nums):
        l = pn * pn
        t = CFG * si / (SN - 1)
        head = (torch.randn(N, 2, B, l, V, generator=g, device=dev) * 2.0).bfloat16()
        gt, gn = gens(), gens()

        def torch_tail():
            lg = head.float()
            lg = (1 + t) * lg[:, 0] - t * lg[:, 1]
            return sample_population(lg, gt, TOP_K, TOP_P)

        def native_tail():
            return sample_population_native(head, t, gn, TOP_K, TOP_P)[0]

        q = torch.empty(N * B * l, V, device=dev).exponential_(1, generator=g)
        ho = head.view(N, 2, B * l, V)

        def launch_alone():
            return K.sample_topk_topp(ho[:, 0], q, TOP_K, TOP_P, uncond=ho[:, 1], w_cond=1 + t, w_uncond=t)

        a = sample_population_native(head, t, gens(), TOP_K, TOP_P)[0]
        lg = head.float()
        b = sample_population((1 + t) * lg[:, 0] - t * lg[:, 1], gens(), TOP_K, TOP_P)
        del lg
        row = {"scale": si, "pn": pn, "rows": N * B * l,
               "torch_tail_us": round(statistics.median(timed(torch_tail, iters) for _ in range(rounds)), 1),
               "native_tail_us": round(statistics.median(timed(native_tail, iters) for _ in range(rounds)), 1),
               "launch_alone_us": round(statistics.median(timed(launch_alone, iters) for _ in range(rounds)), 1),
               "rows_differing": int((a != b).sum()), "bytes_read": N * B * l * V * (2 * 2 + 4)}
        res["scales"].append(row)
        print(json.dumps(row), flush=True)
    res["sum_over_scales_us"] = {k: round(sum(r[k] for r in res["scales"]), 1) for k in res["scales"][0] if k.endswith("_us")}
    print(json.dumps(res["sum_over_scales_us"]), flush=True)
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
    main(out_file=opt.get("--out"), rounds=int(opt.get("--rounds", 3)), iters=int(opt.get("--iters", 5)))
