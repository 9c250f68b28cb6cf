"""The Gemma-2 prompt encoder on libeggroll (hyperscalees_t2i_amd.gemma2) against transformers, one record:
  1. errors: the tiny random model of tests/gemma2_tiny.py at lengths 5 / 40 / 300 — ours, the same model in
     bf16 and ours with the soft-cap off, each as a relative Frobenius error against the fp32 eager oracle over
     the valid rows;
  2. time: the gemma-2-2b architecture with random weights, B prompts of N tokens — the encoder's wall time
     between HIP events (warm-up, then `reps` timed windows of `epasses` passes), and eggroll_softcap_attention
     next to a torch eager restatement of the same attention (bf16 matmuls, fp32 softmax, as transformers' eager
     path) on the same q / k / v, alternating, `kreps` launches per timed window.
A record, not a gate: encoding happens once per prompt set, outside the epoch.
usage: python tools/gemma2_encode_profile.py [--batch 8] [--tokens 300] [--reps 5] [--layers 26] [--out FILE]"""
import argparse
import copy
import dataclasses
import json
import statistics
import sys
import tempfile
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from hyperscalees_t2i_amd import checkpoints as ck  # noqa: E402
from hyperscalees_t2i_amd import kernels as K  # noqa: E402
from hyperscalees_t2i_amd.gemma2 import Gemma2Arch, Gemma2Encoder  # noqa: E402
from tests.gemma2_tiny import LENS, export_dir, hf_config, hf_state, padded_ids, rel_err, tiny_hf_model  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--tokens", type=int, default=300)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--kreps", type=int, default=1000)
ap.add_argument("--epasses", type=int, default=10)
ap.add_argument("--layers", type=int, default=26)
ap.add_argument("--out", default="")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("gemma2_encode_profile: no ROCm device visible (timings are GPU-only)")
dev = torch.device("cuda:0")


def timed(fn, n=1):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / n


# ---- 1. errors ---------------------------------------------------------------------------------
hf = tiny_hf_model(0)
with tempfile.TemporaryDirectory() as td, torch.no_grad():
    enc = ck.load_gemma2_encoder(export_dir(Path(td) / "tiny", hf_state(hf), hf_config(hf)), dev)
    ids, mask = padded_ids(LENS, 512, 0)
    hf = hf.to(dev)
    ref = hf(input_ids=ids.to(dev), attention_mask=mask.to(dev)).last_hidden_state
    b16 = copy.deepcopy(hf).to(torch.bfloat16)(input_ids=ids.to(dev), attention_mask=mask.to(dev)).last_hidden_state
    ours = enc(ids, torch.tensor(LENS))
    enc.arch = dataclasses.replace(enc.arch, softcap=0.0)
    nocap = enc(ids, torch.tensor(LENS))
errors = {f"len_{L}": {"ours": rel_err(ours[b, :L], ref[b, :L]), "bf16_reference": rel_err(b16[b, :L].float(), ref[b, :L]),
                       "ours_soft_cap_off": rel_err(nocap[b, :L], ref[b, :L])} for b, L in enumerate(LENS)}
del enc, hf

# ---- 2. time at the gemma-2-2b architecture ----------------------------------------------------
a = Gemma2Arch(num_layers=args.layers)
with torch.device(dev):
    full = Gemma2Encoder(a)
full.init_weights(0)
B, N = args.batch, args.tokens
g = torch.Generator().manual_seed(0)
ids = torch.randint(4, a.vocab_size, (B, N), generator=g).to(dev)
lens = torch.full((B,), N)
run = lambda: full(ids, lens)  # noqa: E731
for _ in range(2):
    out = run()
torch.cuda.synchronize()
assert bool(torch.isfinite(out.float()).all())
enc_ms = [timed(run, args.epasses) for _ in range(args.reps)]

gd = torch.Generator(device=dev).manual_seed(1)
qkv = torch.randn((B * N, a.q_width + 2 * a.kv_width), generator=gd, device=dev).to(torch.bfloat16)
q, k, v = qkv[:, :a.q_width], qkv[:, a.q_width:a.q_width + a.kv_width], qkv[:, a.q_width + a.kv_width:]
ln = lens.to(device=dev, dtype=torch.int32)
scale, cap, G = a.query_pre_attn_scalar ** -0.5, a.softcap, a.num_heads // a.num_kv_heads
causal = torch.full((N, N), float("-inf"), device=dev, dtype=torch.bfloat16).triu(1)


def kern():
    return K.softcap_attention(q, k, v, ln, B, N, a.num_heads, a.num_kv_heads, scale, cap)


@torch.no_grad()
def eager():
    """transformers' eager_attention_forward on bf16 tensors: repeat_kv, matmul, soft-cap, mask, fp32 softmax."""
    t = lambda x, h: x.reshape(B, N, h, 256).transpose(1, 2)  # noqa: E731
    qq, kk, vv = t(q, a.num_heads), t(k, a.num_kv_heads).repeat_interleave(G, 1), t(v, a.num_kv_heads).repeat_interleave(G, 1)
    w = torch.matmul(qq, kk.transpose(2, 3)) * scale
    w = torch.tanh(w / cap) * cap + causal
    w = torch.softmax(w, dim=-1, dtype=torch.float32).to(qq.dtype)
    return torch.matmul(w, vv).transpose(1, 2).reshape(B * N, a.q_width)


for fn in (kern, eager):
    fn()
torch.cuda.synchronize()
diff = rel_err(kern().float(), eager().float())
tk, te = [], []
for _ in range(args.reps):
    tk.append(timed(kern, args.kreps))
    te.append(timed(eager, args.kreps))
flops = 2.0 * 2 * B * a.num_heads * N * N * 256 / 2     # causal: half of the dense QK^T + PV work
rec = {"what": "tools/gemma2_encode_profile.py on an MI355X",
       "errors_vs_fp32_eager_oracle_tiny_model": errors,
       "bar": "ours <= 1.5 x the error of the same model in bf16 on the same GPU and inputs",
       "timing": {"arch": "gemma-2-2b (random weights)", "layers": args.layers, "B": B, "N": N,
                  "encoder_passes_per_window": args.epasses, "encoder_ms": [round(x, 2) for x in enc_ms],
                  "encoder_median_ms": round(statistics.median(enc_ms), 2),
                  "softcap_attention_us": [round(1e3 * x, 1) for x in tk],
                  "softcap_attention_median_us": round(1e3 * statistics.median(tk), 1),
                  "torch_eager_attention_us": [round(1e3 * x, 1) for x in te],
                  "torch_eager_attention_median_us": round(1e3 * statistics.median(te), 1),
                  "launches_per_window": args.kreps, "kernel_vs_eager_rel_diff": diff,
                  "softcap_attention_tflops_causal": round(flops / (1e-3 * statistics.median(tk)) / 1e12, 2)}}
line = json.dumps(rec, indent=1)
print(line, flush=True)
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")
