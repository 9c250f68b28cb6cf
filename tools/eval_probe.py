"""What the evaluation path costs on the GPU (writes profiles/eval_u8_kernels.json, or --out).

    python tools/eval_probe.py [--sections kernels,clip,e2e] [--out FILE] [--rounds 20]

HIP-event times in one process, warmed up, the two sides of every comparison alternating round by round
(the spread of the rounds is reported next to each median):

  kernels  eggroll_images_to_u8 at 16 x 3 x 1024^2 in each mode against the torch form inside to_pil /
           to_pil_var / to_pil_infinity up to its device-side contiguous uint8 [n, H, W, 3] tensor, on the same
           inputs: ms, TB/s on the kernel's 9 bytes per pixel, share of the 8 TB/s HBM figure, and whether the
           kernel is at least as fast as the torch form (the outputs are compared bitwise first).
  clip     eggroll_clip_preprocess_u8 on 128 uint8 images of 1024^2 against eggroll_clip_preprocess (clip_pixels)
           on the bf16 images they came from: the same taps, so parity within the spread is the expectation.
  e2e      the full Sana-Sprint size with synthetic weights and synthetic reward towers, 64 prompts: images/s of
           generate_and_score with 1, 2 and 4 candidates in one call, the same candidates in separate calls, and
           one bitwise folder-against-direct check on 8 written 1024 px images.
"""
import argparse
import json
import statistics
import sys
import tempfile
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
HBM_TBS = 8.0


def interleaved(fns: dict, rounds: int, inner: int, warmup: int = 2) -> dict:
    """ms per call of every fn(i): per round one timed window of `inner` calls of each, the fns alternating;
    i counts the calls so that a fn can walk over several input buffers.  {name: {median, min, max}}."""
    for _ in range(warmup):
        for f in fns.values():
            for i in range(inner):
                f(i)
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(inner):
                f(i)
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) / inner)
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in times.items()}


def section_kernels(dev, rounds):
    from hyperscalees_t2i_amd import kernels as K
    from hyperscalees_t2i_amd.infinity_pipeline import images_to_uint8
    from hyperscalees_t2i_amd.rewards import postprocess_uint8
    from hyperscalees_t2i_amd.var import quantize_uint8_var
    n, H, W = 16, 1024, 1024
    g = torch.Generator(device=dev).manual_seed(0)
    # four input sets (4 x 144 MiB in + out): consecutive calls do not find their data in the 256 MiB last-level cache
    xs = [(torch.rand((n, 3, H, W), generator=g, device=dev) * 2.2 - 1.1).to(torch.bfloat16) for _ in range(4)]
    forms = {0: postprocess_uint8, 1: quantize_uint8_var, 2: images_to_uint8}
    out = {"shape": [n, 3, H, W], "bytes_per_pixel": 9, "hbm_tbs": HBM_TBS, "calls_per_window": 20, "modes": {}}
    for mode, form in forms.items():
        torch_form = lambda i: form(xs[i % 4]).to(torch.uint8).permute(0, 2, 3, 1).contiguous()   # noqa: E731
        kernel = lambda i: K.images_to_u8(xs[i % 4], mode)                                          # noqa: E731
        same = all(bool(torch.equal(kernel(i), torch_form(i))) for i in range(4))
        t = interleaved({"kernel": kernel, "torch": torch_form}, rounds, inner=20)
        tbs = 9.0 * n * H * W / (t["kernel"]["median_ms"] * 1e-3) / 1e12
        out["modes"][str(mode)] = {**t, "bitwise_equal": same, "kernel_tb_per_s": tbs,
                                   "kernel_share_of_hbm": tbs / HBM_TBS,
                                   "kernel_not_slower": t["kernel"]["median_ms"] <= t["torch"]["median_ms"],
                                   "torch_over_kernel": t["torch"]["median_ms"] / t["kernel"]["median_ms"]}
    return out


def section_clip(dev, rounds):
    from hyperscalees_t2i_amd import kernels as K
    from hyperscalees_t2i_amd.rewards import clip_pixels, clip_pixels_u8
    n = 128
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.cat([(torch.rand((16, 3, 1024, 1024), generator=g, device=dev) * 2.2 - 1.1).to(torch.bfloat16)
                   for _ in range(n // 16)])
    u8 = K.images_to_u8(x, 0)
    same = bool(torch.equal(clip_pixels(x, 0), clip_pixels_u8(u8)))
    t = interleaved({"clip_pixels_bf16": lambda i: clip_pixels(x, 0), "clip_pixels_u8": lambda i: clip_pixels_u8(u8)},
                    rounds, inner=3)
    return {"images": n, "bitwise_equal": same, **t,
            "u8_over_bf16": t["clip_pixels_u8"]["median_ms"] / t["clip_pixels_bf16"]["median_ms"]}


def section_e2e(dev, prompts):
    from hyperscalees_t2i_amd import evaluate as EV
    from hyperscalees_t2i_amd.backend import SanaBackend, SanaConfig
    from hyperscalees_t2i_amd.es import flatten_params
    from hyperscalees_t2i_amd.rewards import RewardModels
    be = SanaBackend(str(dev), SanaConfig(synthetic_weights=True, synthetic_prompts=prompts))
    be.init_and_attach_lora()
    rewards = RewardModels.build(dev, synthetic=True)
    theta = flatten_params(be.collect_lora_params()[0]).float()
    base = EV.load_candidates(be, ["base"])[1][0]
    g = torch.Generator(device=dev).manual_seed(2)
    rows = [base, theta] + [theta + 0.01 * torch.randn(theta.shape, generator=g, device=dev) for _ in range(2)]
    names = ["base", "adapter_0", "adapter_1", "adapter_2"]

    def run(idx, **kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = EV.generate_and_score(be, rewards, ([names[i] for i in idx], torch.stack([rows[i] for i in idx])), **kw)
        torch.cuda.synchronize()
        return r, time.perf_counter() - t0

    run([0, 1], max_prompts=8)                                      # warm-up: every kernel, the text graphs
    out = {"prompts": prompts, "image_px": 1024, "together": {}, "separate": {}}
    for k in (1, 2, 4):
        _, dt = run(list(range(k)))
        out["together"][str(k)] = {"seconds": dt, "images_per_s": k * prompts / dt}
        dts = [run([i])[1] for i in range(k)]
        out["separate"][str(k)] = {"seconds": sum(dts), "images_per_s": k * prompts / sum(dts)}
    with tempfile.TemporaryDirectory() as tmp:
        r, dt = run([1], max_prompts=8, out_root=tmp)
        table = EV.PromptTable(list(be.prompts_list), ["c"] * prompts, ["h"] * prompts, ("Prompt", "Category", "Challenge"))
        out["folder_check"] = {"images": 8, "seconds_with_png": dt,
                               "bitwise_equal": all(EV.score_folder(Path(tmp) / nm, table, rewards) == r.entries(nm)
                                                    for nm in r.names)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sections", default="kernels,clip,e2e")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--prompts", type=int, default=64)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "eval_u8_kernels.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_probe: no ROCm device (this probe measures; it has no CPU form)")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0)}
    for s in a.sections.split(","):
        if s == "kernels":
            res[s] = section_kernels(dev, a.rounds)
        elif s == "clip":
            res[s] = section_clip(dev, a.rounds)
        elif s == "e2e":
            res[s] = section_e2e(dev, a.prompts)
        else:
            raise SystemExit(f"unknown section {s!r}")
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")     # after every section: a late failure keeps the rest
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
