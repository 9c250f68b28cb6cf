"""Per-shape A/B of the halo conv's wide class against the route each host took before it: MIOpen through
F.conv2d on channels-last bf16, or var.DConv2d's im2col GEMM for maps of <= 32 x 32 pixels.

    python tools/conv_wide_ab.py --out profiles/conv_wide_vs_parent_ab.jsonl [--batch 16] [--launches 20]

Both routes run through the hosts' own modules (var.DConv2d, flux_vae.Conv) with the native flag on and off, in
one process, interleaved, timed with HIP events: per round, LAUNCHES launches of one route behind a warm-up, then
the other.  One JSON line per shape: the rounds' ms per launch, and `native_faster`, true only where the slowest
native round beats the fastest parent round (a gain beyond the rounds' own spread).
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from hyperscalees_t2i_amd import kernels as K  # noqa: E402
from hyperscalees_t2i_amd.flux_vae import Conv  # noqa: E402
from hyperscalees_t2i_amd.var import DConv2d  # noqa: E402

# (cin, cout, H, W): the VQVAE decoder's 3x3 convs (ch 160, mult 1,1,2,2,4, 16 x 16 latent), the last three its
# width changes (conv_in and the first ResnetBlock conv1 of two levels)
VAR_SHAPES = [(640, 640, 16, 16), (320, 320, 32, 32), (320, 320, 64, 64), (160, 160, 128, 128), (160, 160, 256, 256),
              (32, 640, 16, 16), (640, 320, 32, 32), (320, 160, 128, 128)]
# the BSQ-VAE decoder at bench.py --workload infinity (512 px, f8: 64 x 64 latent, widths 160/320/640/640)
INFINITY_SHAPES = [(640, 640, 64, 64), (640, 640, 128, 128), (640, 640, 256, 256), (640, 320, 256, 256),
                   (320, 320, 256, 256), (320, 320, 512, 512), (320, 160, 512, 512), (160, 160, 512, 512)]


def _time(fn, launches: int) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / launches


def ab(host: str, B: int, cin: int, cout: int, H: int, W: int, launches: int, rounds: int, dev) -> dict:
    g = torch.Generator(device=dev).manual_seed(cin + cout + H)
    if host == "var":
        m = DConv2d(cin, cout, 3, 1, 1).to(dev).to(torch.bfloat16).to(memory_format=torch.channels_last)
        x = torch.randn(B, cin, H, W, generator=g, device=dev).bfloat16().contiguous(memory_format=torch.channels_last)

        def route(native):
            m.native = native
            return lambda: m(x)
        parent = "im2col" if H * W <= 1024 else "miopen"
    else:
        m = Conv(cin, cout).to(dev)
        x = torch.randn(B, H, W, cin, generator=g, device=dev).bfloat16()

        def route(native):
            m.native_wide_conv = native
            return lambda: m(x)
        parent = "miopen"
    with torch.no_grad():
        m.weight.copy_(torch.randn(m.weight.shape, generator=g, device=dev) / (9 * cin) ** 0.5)
        m.bias.copy_(torch.randn(m.bias.shape, generator=g, device=dev) * 0.1)
        ms = {"parent": [], "native": []}
        for name, native in (("parent", False), ("native", True)):   # warm-up: solver choice, weight packing
            fn = route(native)
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        for _ in range(rounds):
            for name, native in (("parent", False), ("native", True)):
                fn = route(native)
                fn()
                ms[name].append(round(_time(fn, launches), 4))
    flops = 2.0 * B * H * W * cout * 9 * cin
    return {"host": host, "B": B, "H": H, "W": W, "cin": cin, "cout": cout, "parent_route": parent,
            "tile_bn": K.conv_halo_wide_tile(cin, cout, H, W, B), "parent_ms": ms["parent"], "native_ms": ms["native"],
            "native_tflops": round(flops / (min(ms["native"]) * 1e9), 1),
            "native_faster": max(ms["native"]) < min(ms["parent"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=Path, required=True)
    ap.add_argument("--batch", type=int, default=16, help="images per decode chunk (vae_chunk)")
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--hosts", default="var,infinity")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    a.out.parent.mkdir(parents=True, exist_ok=True)
    with a.out.open("w") as f:
        for host, shapes in (("var", VAR_SHAPES), ("infinity", INFINITY_SHAPES)):
            if host not in a.hosts.split(","):
                continue
            for cin, cout, H, W in shapes:
                row = ab(host, a.batch, cin, cout, H, W, a.launches, a.rounds, dev)
                f.write(json.dumps(row) + "\n")
                f.flush()
                print(json.dumps(row), flush=True)
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
