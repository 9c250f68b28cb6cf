"""Kernel A/B at VAR-d16's attention shapes (pop 4: B = 128 sequences, 16 heads of 64, the ten (Nq, Lk) pairs of
the scale schedule): eggroll_flash_attention at head dim 64 (every qf) against F.scaled_dot_product_attention on
the same values in the layout each path keeps them in (token-major cache slice / head-major cache slice), and
eggroll_qk_l2norm_kv against the torch sequence it replaces (F.normalize of q and k in fp32, the per-head scale,
the two strided cache writes).  HIP events around launches queued behind a spin kernel (measure._time), median of
`--rounds` rounds of 20 launches.

usage: python tools/var_attn_ab.py [--out FILE.json] [--rounds N]"""
import json
import statistics
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from hyperscalees_t2i_amd import kernels as K  # noqa: E402
from hyperscalees_t2i_amd.measure import _time  # noqa: E402
from hyperscalees_t2i_amd.var import VAR_D16  # noqa: E402

B, H, HD = 128, 16, 64
C = H * HD


def med(fn, rounds):
    return statistics.median(_time(fn, 20) for _ in range(rounds)) * 1e6


def main(out_file=None, rounds=5):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    L = VAR_D16.L
    tok = torch.empty(2, B, L, C, dtype=torch.bfloat16, device=dev)              # the native path's cache
    tok[0] = F.normalize(torch.randn(B, L, H, HD, generator=g, device=dev), dim=-1).view(B, L, C)
    tok[1] = torch.randn(B, L, C, generator=g, device=dev)
    hm = tok.view(2, B, L, H, HD).transpose(2, 3).contiguous()                    # the torch path's [2, B, H, L, 64]
    qscale = torch.full((H,), 4.0, device=dev)
    res = {"shape": {"B": B, "heads": H, "head_dim": HD}, "rounds": rounds, "launches_per_round": 20, "scales": []}
    cur = 0
    for pn in VAR_D16.patch_nums:
        l = pn * pn
        Lk = cur + l
        qkv = torch.randn(B * l, 3 * C, generator=g, device=dev).bfloat16()
        q_tok = (F.normalize(qkv[:, :C].float().view(B, l, H, HD), dim=-1) * 4).bfloat16()
        q_hm = q_tok.transpose(1, 2).contiguous()
        ks, vs = (tok[i, :, :Lk].view(B, Lk, H, HD) for i in (0, 1))
        row = {"Nq": l, "Lk": Lk}
        for qf in (0, 1, 2, 4):
            row[f"flash64_qf{qf}_us"] = round(med(lambda: K.flash_attention(q_tok, ks, vs, 1.0, qf=qf), rounds), 2)
        row["sdpa_us"] = round(med(lambda: F.scaled_dot_product_attention(q_hm, hm[0, :, :, :Lk], hm[1, :, :, :Lk], scale=1.0),
                                   rounds), 2)
        o = torch.empty(B, H, l, HD, dtype=torch.bfloat16, device=dev)
        row["sdpa_out_transpose_us"] = round(med(lambda: o.transpose(1, 2).reshape(B * l, C).contiguous(), rounds), 2)
        got = K.flash_attention(q_tok, ks, vs, 1.0).float()
        ref = F.scaled_dot_product_attention(q_hm.float(), hm[0, :, :, :Lk].float(), hm[1, :, :, :Lk].float(),
                                             scale=1.0).transpose(1, 2)
        row["flash64_rel_err_vs_fp32"] = float((got - ref).norm() / ref.norm())

        def l2_native():
            K.qk_l2norm_kv(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], H, 1e-12, qscale=qscale, kout=tok[0], vout=tok[1],
                           rows_per_seq=l, row0=cur)

        q_mul = qscale.view(1, H, 1, 1)

        def l2_torch():   # var.py's torch path, line for line
            x5 = qkv.view(B, l, 3, H, HD)
            q = F.normalize(x5[:, :, 0].transpose(1, 2).float(), dim=-1).mul_(q_mul).to(torch.bfloat16)
            hm[0, :, :, cur:Lk] = F.normalize(x5[:, :, 1].transpose(1, 2).float(), dim=-1).to(torch.bfloat16)
            hm[1, :, :, cur:Lk] = x5[:, :, 2].transpose(1, 2)
            return q

        row["qk_l2norm_kv_us"] = round(med(l2_native, rounds), 2)
        row["torch_normalize_scale_append_us"] = round(med(l2_torch, rounds), 2)
        row["qk_l2norm_kv_bytes"] = 6 * 2 * B * l * C     # q, k, v read and written once each
        row["flash64_bytes"] = 2 * B * C * (2 * l + 2 * Lk)
        res["scales"].append(row)
        print(json.dumps(row), flush=True)
        cur += l
    tot = lambda key: round(sum(r[key] for r in res["scales"]), 1)  # noqa: E731
    res["sum_over_scales_us"] = {k: tot(k) for k in res["scales"][0] if k.endswith("_us")}
    print(json.dumps(res["sum_over_scales_us"]))
    if out_file:
        Path(out_file).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    args = sys.argv[1:]
    opt = {}
    for flag in ("--out", "--rounds"):
        if flag in args:
            i = args.index(flag)
            opt[flag] = args[i + 1]
            del args[i:i + 2]
    main(out_file=opt.get("--out"), rounds=int(opt.get("--rounds", 5)))
