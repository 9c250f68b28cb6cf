"""The Qwen3 prompt encoder on libeggroll (hyperscalees_t2i_amd.qwen3) against transformers and torch, one record:
  1. errors: the tiny random model of tests/qwen3_tiny.py at lengths 5 / 40 / 130 — ours, the same model in
     bf16, ours run through every layer and ours with the q / k norm weights forced to 1, each as a relative
     Frobenius error of hidden_states[-2] against the fp32 eager oracle over the valid rows;
  2. encoder time: the Qwen3-4B architecture with random weights, B prompts of N tokens for each N — wall time
     between HIP events (warm-up, then `reps` timed windows of `epasses` passes);
  3. kernel time at B, 32 query heads on 8 KV heads, each N: eggroll_causal_attention next to torch on the same
     bf16 q / k / v with the same causal + key-length mask — F.scaled_dot_product_attention(enable_gqa=True)
     with the boolean mask (and with is_causal=True, which the full-length rows of this run allow) and the eager
     restatement (repeat_kv, bf16 matmuls, fp32 softmax) — alternating, `kreps` launches per timed window.
A record, not a gate: encoding happens once per prompt set, outside the epoch.  Written to
profiles/qwen3_encoder_vs_transformers.json unless --out names another file.
usage: python tools/qwen3_encode_profile.py [--batch 8] [--tokens 128,512] [--reps 5] [--layers 36] [--out FILE]"""
import argparse
import copy
import json
import statistics
import sys
import tempfile
from pathlib import Path

import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from hyperscalees_t2i_amd import checkpoints as ck  # noqa: E402
from hyperscalees_t2i_amd import kernels as K  # noqa: E402
from hyperscalees_t2i_amd.qwen3 import Qwen3Arch, Qwen3Encoder  # noqa: E402
from tests.qwen3_tiny import LENS, export_dir, hf_config, hf_state, padded_ids, rel_err, tiny_hf_model  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--tokens", default="128,512")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--kreps", type=int, default=500)
ap.add_argument("--epasses", type=int, default=5)
ap.add_argument("--layers", type=int, default=36)
ap.add_argument("--out", default=str(Path(__file__).resolve().parent.parent / "profiles" / "qwen3_encoder_vs_transformers.json"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("qwen3_encode_profile: no ROCm device visible (timings are GPU-only)")
dev = torch.device("cuda:0")
TOKENS = [int(t) for t in args.tokens.split(",")]


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
    st, cfg = hf_state(hf), hf_config(hf)
    enc = ck.load_qwen3_encoder(export_dir(Path(td) / "tiny", st, cfg), dev)
    deep_enc = ck.load_qwen3_encoder(export_dir(Path(td) / "all", st, {**cfg, "num_hidden_layers": cfg["num_hidden_layers"] + 1}), dev)
    ids, mask = padded_ids(LENS, 512, 0)
    hf = hf.to(dev)
    kw = dict(input_ids=ids.to(dev), attention_mask=mask.to(dev), output_hidden_states=True)
    ref = hf(**kw).hidden_states[-2]
    b16 = copy.deepcopy(hf).to(torch.bfloat16)(**kw).hidden_states[-2]
    ours = enc(ids, torch.tensor(LENS))
    deep = deep_enc(ids, torch.tensor(LENS))
    for b in enc.blocks:
        b.q_norm.fill_(1.0)
        b.k_norm.fill_(1.0)
    unit = enc(ids, torch.tensor(LENS))
errors = {f"len_{L}": {"ours": rel_err(ours[b, :L], ref[b, :L]), "bf16_reference": rel_err(b16[b, :L].float(), ref[b, :L]),
                       "ours_all_layers": rel_err(deep[b, :L], ref[b, :L]),
                       "ours_qk_norm_weights_1": rel_err(unit[b, :L], ref[b, :L])} for b, L in enumerate(LENS)}
del enc, deep_enc, hf

# ---- 2. encoder time at the Qwen3-4B architecture ----------------------------------------------
a = Qwen3Arch(num_layers=args.layers)
with torch.device(dev):
    full = Qwen3Encoder(a)
full.init_weights(0)
B = args.batch
encoder = {}
for N in TOKENS:
    g = torch.Generator().manual_seed(N)
    ids = torch.randint(8, a.vocab_size, (B, N), generator=g).to(dev)
    lens = torch.full((B,), N)
    run = lambda: full(ids, lens)  # noqa: E731
    for _ in range(2):
        out = run()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out.float()).all())
    ms = [timed(run, args.epasses) for _ in range(args.reps)]
    encoder[f"N_{N}"] = {"ms": [round(x, 2) for x in ms], "median_ms": round(statistics.median(ms), 2)}
del full
torch.cuda.empty_cache()

# ---- 3. kernel time ----------------------------------------------------------------------------
Hq, Hkv, HD = a.num_heads, a.num_kv_heads, a.head_dim
G, scale = Hq // Hkv, a.head_dim ** -0.5
kernel = {}
for N in TOKENS:
    gd = torch.Generator(device=dev).manual_seed(N + 1)
    qkv = torch.randn((B * N, a.q_width + 2 * a.kv_width), generator=gd, device=dev).to(torch.bfloat16)
    q, k, v = qkv[:, :a.q_width], qkv[:, a.q_width:a.q_width + a.kv_width], qkv[:, a.q_width + a.kv_width:]
    lens = torch.full((B,), N)
    ln = lens.to(device=dev, dtype=torch.int32)
    i, j = torch.arange(N, device=dev)[:, None], torch.arange(N, device=dev)[None, :]
    keep = (j <= i)[None, None] & (j[None, None] < ln.view(B, 1, 1, 1))          # [B, 1, N, N] bool
    bias = torch.zeros(keep.shape, dtype=torch.bfloat16, device=dev).masked_fill(~keep, float("-inf"))
    t = lambda x, h: x.reshape(B, N, h, HD).transpose(1, 2)  # noqa: E731

    def kern():
        return K.causal_attention(q, k, v, ln, B, N, Hq, Hkv, scale)

    @torch.no_grad()
    def sdpa_mask():
        o = F.scaled_dot_product_attention(t(q, Hq), t(k, Hkv), t(v, Hkv), attn_mask=keep, scale=scale, enable_gqa=True)
        return o.transpose(1, 2).reshape(B * N, Hq * HD)

    @torch.no_grad()
    def sdpa_causal():
        o = F.scaled_dot_product_attention(t(q, Hq), t(k, Hkv), t(v, Hkv), is_causal=True, scale=scale, enable_gqa=True)
        return o.transpose(1, 2).reshape(B * N, Hq * HD)

    @torch.no_grad()
    def eager():
        """transformers' eager_attention_forward on bf16 tensors: repeat_kv, matmul, mask, fp32 softmax."""
        qq, kk, vv = t(q, Hq), t(k, Hkv).repeat_interleave(G, 1), t(v, Hkv).repeat_interleave(G, 1)
        w = torch.matmul(qq, kk.transpose(2, 3)) * scale + bias
        w = torch.softmax(w, dim=-1, dtype=torch.float32).to(qq.dtype)
        return torch.matmul(w, vv).transpose(1, 2).reshape(B * N, Hq * HD)

    fns = {"causal_attention": kern, "torch_sdpa_bool_mask": sdpa_mask, "torch_sdpa_is_causal": sdpa_causal,
           "torch_eager": eager}
    rec, live = {}, {}
    for name, fn in fns.items():
        try:
            for _ in range(3):
                o = fn()
            torch.cuda.synchronize()
            live[name] = fn
            rec[name + "_rel_diff_vs_kernel"] = rel_err(o.float(), kern().float())
        except Exception as ex:  # a torch path this build does not offer: recorded, not timed
            rec[name + "_unavailable"] = f"{type(ex).__name__}: {str(ex)[:200]}"
    times = {name: [] for name in live}
    for _ in range(args.reps):
        for name, fn in live.items():
            times[name].append(timed(fn, args.kreps))
    for name, ts in times.items():
        rec[name + "_us"] = [round(1e3 * x, 1) for x in ts]
        rec[name + "_median_us"] = round(1e3 * statistics.median(ts), 1)
    flops = 2.0 * 2 * B * Hq * N * N * HD / 2     # causal: half of the dense QK^T + PV work
    rec["causal_attention_tflops_causal"] = round(flops / (1e-3 * statistics.median(times["causal_attention"])) / 1e12, 2)
    kernel[f"N_{N}"] = rec
    del qkv, keep, bias

rec = {"what": "tools/qwen3_encode_profile.py on an MI355X",
       "errors_vs_fp32_eager_oracle_tiny_model_hidden_states_-2": errors,
       "bar": "ours <= 1.5 x the error of the same model in bf16 on the same GPU and inputs",
       "encoder_timing": {"arch": "Qwen3-4B (random weights)", "layers": args.layers, "blocks_run": a.run_layers, "B": B,
                          "passes_per_window": args.epasses, **encoder},
       "kernel_timing": {"B": B, "heads_q": Hq, "heads_kv": Hkv, "head_dim": HD, "launches_per_window": args.kreps,
                         **kernel}}
line = json.dumps(rec, indent=1)
print(line, flush=True)
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")
