"""Prompt encoding A/B at the flan-t5-xl architecture, random weights: the T5 encoder on libeggroll
(hyperscalees_t2i_amd.t5, sequences trimmed to each batch's longest prompt) vs transformers' T5EncoderModel
in bf16 on ids padded to 512 (the reference's form, models/Infinity.py:302-313).  Both hold the same weights.
Synthetic prompts of 10-80 tokens; warm-up, then alternating timed passes between HIP events; the attention
kernel's OpTimer line at that shape.  A record, not a gate: encoding happens once per run.
usage: python tools/t5_encode_ab.py [--prompts 64] [--batch 16] [--reps 5] [--layers 24] [--out FILE]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from hyperscalees_t2i_amd import checkpoints as ck  # noqa: E402
from hyperscalees_t2i_amd import kernels as K  # noqa: E402
from hyperscalees_t2i_amd.t5 import T5Arch, T5Encoder  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--prompts", type=int, default=64)
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--layers", type=int, default=24)
ap.add_argument("--out", default="")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("t5_encode_ab: no ROCm device visible (timings are GPU-only)")
dev = torch.device("cuda:0")

a = T5Arch(num_layers=args.layers)
ours = T5Encoder(a).init_weights(0).to(dev)
from transformers import T5Config, T5EncoderModel  # noqa: E402
with torch.device(dev):
    hf = T5EncoderModel(T5Config(**{k: v for k, v in ck.t5_config_from_arch(a).items()
                                    if k not in ("model_type", "architectures")})).to(torch.bfloat16).eval()
state = {k: v.to(dev) for k, v in ck.state_from_build(ours, ck.t5_rules(ours)).items()}
missing, unexpected = hf.load_state_dict(state, strict=False)
assert not unexpected and set(missing) <= {"encoder.embed_tokens.weight"}, (missing, unexpected)

g = torch.Generator().manual_seed(0)
lens = torch.randint(10, 81, (args.prompts,), generator=g)
ids = torch.zeros(args.prompts, 512, dtype=torch.long)
for i, L in enumerate(lens.tolist()):
    ids[i, :L] = torch.randint(3, a.vocab_size, (L,), generator=g)
    ids[i, L - 1] = 1
mask = (torch.arange(512)[None, :] < lens[:, None]).long()
ids_d, mask_d = ids.to(dev), mask.to(dev)
batches = [slice(s, min(s + args.batch, args.prompts)) for s in range(0, args.prompts, args.batch)]


@torch.no_grad()
def run_ours():
    return [ours(ids_d[s], lens[s]) for s in batches]


@torch.no_grad()
def run_hf():
    return [hf(input_ids=ids_d[s], attention_mask=mask_d[s]).last_hidden_state for s in batches]


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


for fn in (run_ours, run_hf):   # warm-up: every shape of the timed passes
    fn()
torch.cuda.synchronize()
t = {"ours": [], "hf": []}
for _ in range(args.reps):
    t["ours"].append(timed(run_ours))
    t["hf"].append(timed(run_hf))
o, h = run_ours(), run_hf()
num = den = 0.0
for s, yo, yh in zip(batches, o, h):
    for i, L in enumerate(lens[s].tolist()):
        num += float((yo[i, :L].float() - yh[i, :L].float()).norm() ** 2)
        den += float(yh[i, :L].float().norm() ** 2)
K.OpTimer.reset(True)
run_ours()
attn = K.OpTimer.summary().get("relbias_attention", {})
K.OpTimer.reset(False)
rec = {"arch": "flan-t5-xl (random weights)", "layers": args.layers, "prompts": args.prompts, "batch": args.batch,
       "tokens_min_max_total": [int(lens.min()), int(lens.max()), int(lens.sum())],
       "ours_trimmed_ms": [round(x, 2) for x in t["ours"]], "hf_bf16_padded512_ms": [round(x, 2) for x in t["hf"]],
       "ours_median_ms": round(statistics.median(t["ours"]), 2), "hf_median_ms": round(statistics.median(t["hf"]), 2),
       "rel_diff_ours_vs_hf_bf16_valid_rows": (num / den) ** 0.5,
       "relbias_attention_optimer": {k: (round(v, 3) if isinstance(v, float) else v) for k, v in attn.items()}}
line = json.dumps(rec)
print(line, flush=True)
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")
