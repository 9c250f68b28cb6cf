"""bench.py's stdout contract on the CPU: the headline line a driver parses from the tail of stdout is
compact (≤ 4 KB), valid JSON, and carries the headline keys, `roofline` and `cpu_baseline`, with the
per-kernel tables moved to the aux record (a 22.6-KB line went unparsed)."""
import importlib.util
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", ROOT / "bench.py")
    m = importlib.util.module_from_spec(spec)
    argv = sys.argv
    try:
        sys.argv = ["bench.py"]
        spec.loader.exec_module(m)
    finally:
        sys.argv = argv
    return m


def test_compact_line_from_full_record():
    b = _bench()
    full = json.loads((ROOT / "profiles" / "r12d_bench_line.json").read_text())   # a full round-5 record
    assert len(json.dumps(full)) > 16000
    full["roofline"]["algorithmic_bytes"] = b.algo_bytes("131072x2240x2240")
    s = json.dumps(b.compact_line(full, "gpurun_out/bench_aux.json"), separators=(",", ":"))
    assert len(s.encode()) <= b.LINE_MAX_BYTES
    c = json.loads(s)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config"):
        assert k in c, k
    r = c["roofline"]
    assert r["kernel"] == "k_lora_gemm8n<2,0>" and r["bound"] == "mfma" and r["unit"] == "TFLOP/s"
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    assert r["algorithmic_bytes"] == 2.0 * (131072 * 2240 * 2 + 2240 * 2240)
    assert r["mfma_busy"] is not None and r["traffic"] > r["algorithmic_bytes"]
    cpu = c["cpu_baseline"]
    assert set(cpu) == {"value", "unit", "cores", "kind", "sample"} and cpu["kind"] in ("port", "reference")
    assert "\n" not in cpu["sample"]
    assert "model_kernels" not in c and "aux_kernels" not in c


def test_emit_writes_aux_and_prints_last(tmp_path, capsys):
    b = _bench()
    full = json.loads((ROOT / "profiles" / "r12d_bench_line.json").read_text())

    class A:
        aux_out = str(tmp_path / "aux.json")
    b.emit(full, {"all": {}}, A)
    out = capsys.readouterr().out.strip().splitlines()
    c = json.loads(out[-1])
    assert c["value"] == full["value"]
    rec = json.loads((tmp_path / "aux.json").read_text())
    assert rec["line"]["model_kernels"] == full["model_kernels"]


def _head():
    full = json.loads((ROOT / "profiles" / "r12d_bench_line.json").read_text())
    return {k: full[k] for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
                                 "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config")}


def test_plain_line_is_the_headline_only(tmp_path, capsys):
    """Without --full the one stdout line carries the headline keys as measured, `roofline` and
    `cpu_baseline` null, and no record is written unless --aux-out names one."""
    b = _bench()
    head = _head()

    class A:
        aux_out = ""
    b.emit_plain(head, A)
    out = capsys.readouterr().out.strip().splitlines()
    assert len(out) == 1 and len(out[0].encode()) <= b.LINE_MAX_BYTES
    c = json.loads(out[0])
    for k, v in head.items():
        assert c[k] == v, k
    assert c["roofline"] is None and c["cpu_baseline"] is None and c["details"] is None
    assert abs(c["ms_per_step"] * c["value"] - 1e3 * c["config"]["pop_total"]) < 1e-6 * 1e3 * c["config"]["pop_total"]
    A.aux_out = str(tmp_path / "sub" / "aux.json")
    b.emit_plain(head, A)
    assert json.loads(capsys.readouterr().out.strip())["details"] == A.aux_out
    assert json.loads((tmp_path / "sub" / "aux.json").read_text())["line"]["value"] == head["value"]


def test_full_and_dump_options_parse():
    b = _bench()
    argv = sys.argv
    try:
        sys.argv = ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"]
        a = b.parse()
        assert a.steps == 7 and a.warmup == 2 and a.full is False and a.dump_outputs == ""
        sys.argv = ["bench.py", "--full", "--dump-outputs", "d"]
        a = b.parse()
        assert a.full is True and a.dump_outputs == "d"
    finally:
        sys.argv = argv


def test_dump_outputs_files(tmp_path):
    """--dump-outputs: one float32 / float64 .npy per array ESEngine.step returned, values unchanged; an
    array over its share of the 64 MB is cut to the same seeded sample every time."""
    import numpy as np
    import torch
    b = _bench()
    g = torch.Generator().manual_seed(0)
    theta = torch.randn(1001, generator=g)
    stats = {"_S": torch.randn(8, 4, generator=g), "_raw": torch.randn(8, 5, generator=g),
             "_fitness": {"fitness": torch.randn(8, generator=g), "order": torch.arange(8, dtype=torch.int32),
                          "finite": torch.ones(8, dtype=torch.bool), "mu": torch.randn(4, generator=g).double()},
             "summary/mean_reward": 0.5}
    b.dump_outputs(str(tmp_path / "o"), theta, stats)
    got = {p.stem: np.load(p) for p in (tmp_path / "o").glob("*.npy")}
    assert set(got) == {"theta", "S", "raw", "fitness_fitness", "fitness_order", "fitness_finite", "fitness_mu"}
    assert got["theta"].dtype == np.float32 and np.array_equal(got["theta"], theta.numpy())
    assert got["S"].shape == (8, 4) and np.array_equal(got["raw"], stats["_raw"].numpy())
    assert got["fitness_order"].dtype == np.float64 and np.array_equal(got["fitness_order"], np.arange(8.0))
    assert got["fitness_finite"].dtype == np.float64 and got["fitness_mu"].dtype == np.float64
    old = b.DUMP_MAX_BYTES
    try:
        b.DUMP_MAX_BYTES = 7 * 400                      # 7 arrays: 400 bytes each = 100 float32 of theta's 1001
        b.dump_outputs(str(tmp_path / "s1"), theta, stats)
        b.dump_outputs(str(tmp_path / "s2"), theta, stats)
    finally:
        b.DUMP_MAX_BYTES = old
    s1, s2 = np.load(tmp_path / "s1" / "theta.npy"), np.load(tmp_path / "s2" / "theta.npy")
    assert s1.shape == (100,) and np.array_equal(s1, s2) and np.isin(s1, theta.numpy()).all()
    assert sum(p.stat().st_size for p in (tmp_path / "s1").glob("*.npy")) <= 7 * 400 + 7 * 128   # + .npy headers
    assert np.array_equal(np.load(tmp_path / "s1" / "S.npy"), stats["_S"].numpy())
