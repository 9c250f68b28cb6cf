"""The multi-step Sana-Sprint backend (SanaConfig(backend_mode="pipeline")) on the GPU, HIP-event timings at
pop 8, 1024 px, synthetic weights, one record:
  a. an ES epoch (ESEngine.step, the benchmark's configuration) with backend_mode "pipeline" next to "one_step",
     alternating, `--steps` timed epochs each after `--warmup`;
  b. per sampler step, eggroll_scm_step next to the torch form of the same step (pipeline._step_torch) on the
     shapes the epoch uses: the mid step (x shared by the members, x_next + m_next written) and the last step
     (x0_out written), alternating, `--kreps` launches per timed window, queued behind a spin kernel so the GPU
     runs them back to back; bytes per launch from the shapes.
A record, not a gate, except for one statement it checks itself: the kernel form is not slower than the torch
form in this run.
usage: python tools/sana_pipeline_profile.py [--pop 8] [--latent 32] [--steps 3] [--warmup 1] [--small] [--out FILE]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from hyperscalees_t2i_amd import kernels as K  # noqa: E402
from hyperscalees_t2i_amd import pipeline as P  # noqa: E402
from hyperscalees_t2i_amd.backend import SanaBackend, SanaConfig  # noqa: E402
from hyperscalees_t2i_amd.es import EggRollNoiser, flatten_params  # noqa: E402
from hyperscalees_t2i_amd.es_step import ESConfig, ESEngine  # noqa: E402
from hyperscalees_t2i_amd.rewards import RewardModels  # noqa: E402
from hyperscalees_t2i_amd.sana import SanaArch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--pop", type=int, default=8)
ap.add_argument("--latent", type=int, default=32, help="32 -> 1024 px")
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--kreps", type=int, default=200)
ap.add_argument("--small", action="store_true", help="tiny architecture (a rehearsal of the script, not a measurement)")
ap.add_argument("--out", default="")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("sana_pipeline_profile: no ROCm device visible (timings are GPU-only)")
dev = torch.device("cuda:0")


def build(mode):
    cfg = SanaConfig(backend_mode=mode, synthetic_weights=True, width_latent=args.latent, height_latent=args.latent)
    if args.small:
        cfg.arch = SanaArch(num_attention_heads=4, attention_head_dim=32, num_layers=2, num_cross_attention_heads=2,
                            cross_attention_head_dim=64, caption_channels=2304)
        cfg.vae_widths, cfg.vae_layers = (16, 32, 32, 64, 64, 64), (1, 1, 1, 1, 1, 1)
    be = SanaBackend(str(dev), cfg)
    be.init_and_attach_lora()
    params, shapes = be.collect_lora_params()
    noiser = EggRollNoiser(shapes, sigma=1e-2, lr_scale=1e-1, rank=1, use_antithetic=True)
    eng = ESEngine(be, rewards, noiser, ESConfig(pop_size=args.pop, sigma=1e-2, lr_scale=1e-1, egg_rank=1,
                                                 use_antithetic=True, promptnorm=True, theta_max_norm=40.0), dev)
    return be, eng, flatten_params(params).to(dev)


def epoch_ms(eng, theta, seed):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    new, st = eng.step(theta, seed=seed, guidance_scale=4.5)
    e.record()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(st["_S"]).all()) and bool(torch.isfinite(new).all())
    return s.elapsed_time(e)


# ---- a. the epoch ------------------------------------------------------------------------------
rewards = RewardModels.build(dev, tiny=args.small, synthetic=True)
modes = {m: build(m) for m in ("one_step", "pipeline")}
ep = {m: [] for m in modes}
for i in range(args.warmup + args.steps):
    for m, (_, eng, theta) in modes.items():
        t = epoch_ms(eng, theta, i)
        if i >= args.warmup:
            ep[m].append(t)
P.FUSE_SCM_STEP = False
ep_torch_step = [epoch_ms(modes["pipeline"][1], modes["pipeline"][2], args.warmup + i) for i in range(args.steps)]
P.FUSE_SCM_STEP = True

# ---- b. the step, kernel next to torch ---------------------------------------------------------
be = modes["pipeline"][0]
es = be.es_model
b = len(be.step_sampling_info(0)["flat_ids"])
R, HW, C = min(args.pop, be.cfg.members_per_pass or args.pop), args.latent * args.latent, es.transformer_config.in_channels
n = b * HW * C
rd = P._ROUND_DTYPES[es.DTYPE]
g = torch.Generator(device=dev).manual_seed(0)
x_shared = torch.randn((b, HW, C), device=dev, generator=g) * 0.5
x_own = torch.randn((R * b, HW, C), device=dev, generator=g) * 0.5
eps = torch.randn((R * b, HW, C), device=dev, generator=g)
noise = torch.randn((b, HW, C), device=dev, generator=g)
o1, o2 = torch.empty_like(eps), torch.empty_like(eps)
ts = es.timesteps
sc_mid = P.scm_step_scalars(ts[0], ts[1], es.sigma_data)
sc_last = P.scm_step_scalars(ts[-2], ts[-1], es.sigma_data, 1.0 / (es.sigma_data * es.vae.scaling_factor))


def timed(fn, it):
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(5_000_000)
    s.record()
    for _ in range(it):
        fn()
    e.record()
    torch.cuda.synchronize()
    return 1e3 * s.elapsed_time(e) / it     # us per launch


cases = {
    "mid_step_shared_x": (lambda: K.scm_step(x_shared, eps, noise, sc_mid, rd, R, x_next=o1, m_next=o2),
                          lambda: P._step_torch(x_shared, eps, noise, sc_mid, rd, R),
                          4 * n + 4 * R * n + 4 * n + 2 * 4 * R * n),
    "last_step": (lambda: K.scm_step(x_own, eps, None, sc_last, rd, R, x0_out=o1),
                  lambda: P._step_torch(x_own, eps, None, sc_last, rd, R, last=True),
                  4 * R * n + 4 * R * n + 4 * R * n),
}
steps_rec = {}
for name, (kern, torch_form, nbytes) in cases.items():
    tk, tt = [], []
    for _ in range(args.reps):
        tk.append(timed(kern, args.kreps))
        tt.append(timed(torch_form, args.kreps))
    mk, mt = statistics.median(tk), statistics.median(tt)
    steps_rec[name] = {"bytes_per_launch": nbytes, "scm_step_us": [round(v, 2) for v in tk],
                       "step_torch_us": [round(v, 2) for v in tt], "scm_step_median_us": round(mk, 2),
                       "step_torch_median_us": round(mt, 2), "scm_step_GBps": round(nbytes / mk / 1e3, 1),
                       "kernel_not_slower": bool(mk <= mt)}

med = lambda v: round(statistics.median(v), 1)  # noqa: E731
rec = {"what": "tools/sana_pipeline_profile.py on an MI355X" + (" (--small: a rehearsal, not a measurement)" if args.small else ""),
       "config": {"pop": args.pop, "members_per_pass": R, "images_per_member": b, "latent": args.latent,
                  "px": 32 * args.latent, "num_inference_steps": es.num_inference_steps, "dtype": str(es.DTYPE),
                  "weights": "synthetic", "warmup": args.warmup, "steps": args.steps},
       "epoch_ms": {"one_step": [round(v, 1) for v in ep["one_step"]], "pipeline": [round(v, 1) for v in ep["pipeline"]],
                    "pipeline_torch_step": [round(v, 1) for v in ep_torch_step],
                    "one_step_median": med(ep["one_step"]), "pipeline_median": med(ep["pipeline"]),
                    "pipeline_torch_step_median": med(ep_torch_step),
                    "pipeline_over_one_step": round(statistics.median(ep["pipeline"]) / statistics.median(ep["one_step"]), 3)},
       "step": {"members": R, "n_per_member": n, "round_dtype": rd, "launches_per_window": args.kreps, **steps_rec}}
line = json.dumps(rec, indent=1)
print(line, flush=True)
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")
if not all(v["kernel_not_slower"] for v in steps_rec.values()):
    sys.exit("sana_pipeline_profile: eggroll_scm_step is slower than the torch form in this run")
