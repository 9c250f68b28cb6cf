"""Time eggroll_gguf_dequant on one Z-Image FFN weight (3840 x 10240) per ggml type against the HBM rate of the
project's rooflines (measure.HBM_PEAK_GBPS), next to dequantize_numpy on the same bytes on the same host, and
check that both produce the same bf16 tensor.  Random quants, every fp16 field 0.0123.  Two timings per type: the
same input and output buffers every launch (about 100 MB, which the 256 MiB Infinity Cache can hold), and four
buffer sets in rotation (about 400 MB, more than the cache: the HBM figure).

    python tools/gguf_dequant_probe.py [--out profiles/gguf_dequant.json] [--types Q3_K,Q4_K,Q6_K,Q8_0]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from hyperscalees_t2i_amd import gguf as G  # noqa: E402
from hyperscalees_t2i_amd import kernels as K  # noqa: E402
from hyperscalees_t2i_amd.measure import HBM_PEAK_GBPS, _time  # noqa: E402

ROTATE = 4
HALF_FIELDS = {G.Q4_0: (0,), G.Q4_1: (0, 2), G.Q5_0: (0,), G.Q5_1: (0, 2), G.Q8_0: (0,), G.Q2_K: (80, 82),
               G.Q3_K: (108,), G.Q4_K: (0, 2), G.Q5_K: (0, 2), G.Q6_K: (208,)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/gguf_dequant.json")
    ap.add_argument("--types", default="Q3_K,Q4_K,Q6_K,Q8_0")
    ap.add_argument("--shape", default="3840x10240")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    shape = tuple(int(x) for x in a.shape.split("x"))
    n = int(np.prod(shape))
    by_name = {v[0]: k for k, v in G.GGML_TYPES.items()}
    res = {"shape": list(shape), "hbm_peak_GBps": HBM_PEAK_GBPS, "device": torch.cuda.get_device_name(0),
           "timing": "average of 20 back-to-back launches between HIP events after a warm-up (measure._time); us / GBps / "
                     f"frac_of_hbm_peak: {ROTATE} input + output buffer sets in rotation (working set above the 256 MiB "
                     "Infinity Cache); *_same_buffers: one set reused (cache-assisted); numpy: one call, host wall clock", "types": {}}
    for name in a.types.split(","):
        t = by_name[name]
        _, be, ts = G.GGML_TYPES[t]
        raw = np.random.default_rng(t).integers(0, 256, (n // be, ts), dtype=np.uint8)
        for off in HALF_FIELDS[t]:
            raw[:, off:off + 2] = np.array([0.0123], dtype="<f2").view(np.uint8)
        raw = raw.reshape(-1)
        raw_dev = torch.from_numpy(raw).to(dev)
        sec_same = _time(lambda: K.gguf_dequant(raw_dev, t, n))
        raws, outs, turn = [raw_dev.clone() for _ in range(ROTATE)], [None] * ROTATE, [0]

        def rotating():
            i = turn[0] % ROTATE
            outs[i] = K.gguf_dequant(raws[i], t, n)
            turn[0] += 1
        sec = _time(rotating)
        del raws, outs
        byt = float(raw.size + 2 * n)
        t0 = time.perf_counter()
        ref = G.dequantize_numpy(raw, t, n)
        cpu_s = time.perf_counter() - t0
        same = torch.equal(K.gguf_dequant(raw_dev, t, n).cpu(), torch.from_numpy(ref).to(torch.bfloat16))
        res["types"][name] = {"us": sec * 1e6, "bytes_read": raw.size, "bytes_written": 2 * n,
                              "GBps": byt / sec / 1e9, "frac_of_hbm_peak": byt / sec / 1e9 / HBM_PEAK_GBPS,
                              "us_same_buffers": sec_same * 1e6,
                              "frac_of_hbm_peak_same_buffers": byt / sec_same / 1e9 / HBM_PEAK_GBPS,
                              "numpy_s": cpu_s, "gpu_equals_numpy_bf16": bool(same)}
        print(name, json.dumps(res["types"][name]), flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
