"""A/B of builds of libeggroll on the population LoRA GEMM (eggroll_lora_gemm_sel and eggroll_lora_linear_pop_sel),
every library bound by ctypes in one process, seeded inputs, HIP events on the launch stream.

    python tools/lib_ab.py build-a [REV]               build a committed revision's library into
                                                       tools/_stamps/libeggroll_a.so
    python tools/lib_ab.py A.so B.so [KERNEL]          bitwise equality on ragged / member-straddling / bias / no-bias
                                                       cases, then interleaved timing at the Sana-1.6B shapes (r 2) and
                                                       at 8192 x 2240 x 2240, which the automatic choice gives to
                                                       kernel 128 (r 0 / 2 / 16); "spread" = the largest |1 - A/B|
    python tools/lib_ab.py bits A.so B.so              bitwise equality at the shapes of tests/test_gpu_gemm_layouts.py,
                                                       kernels 0 / 8 / 9 / 10 / 128, r 0 / 1 / 2 / 4, both entry points
"""
import ctypes
import json
import statistics
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
vp, i64, i32, f32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_float


def build_a(rev):
    out = ROOT / "tools" / "_stamps" / "libeggroll_a.so"
    out.parent.mkdir(parents=True, exist_ok=True)
    with tempfile.TemporaryDirectory() as td:
        arc = subprocess.run(["git", "archive", rev, "hyperscalees_t2i_amd/csrc", "include"], cwd=ROOT, check=True,
                             capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", td], input=arc, check=True)
        objs = []
        for src in sorted((Path(td) / "hyperscalees_t2i_amd" / "csrc").glob("*.hip")):  # the revision's own file set
            o = Path(td) / (src.stem + ".o")
            subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c",
                            f"-I{Path(td) / 'include'}", str(src), "-o", str(o)], check=True)
            objs.append(str(o))
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-shared", "-fPIC", *objs, "-o", str(out)],
                       check=True)
    print(out)


class Case:
    """One seeded problem and, per library, its own Y and projection workspace."""

    def __init__(self, libs, M, N, K, rpm, r, bias, seed=3):
        import torch
        self.libs, self.dims, self.r = libs, (M, N, K, rpm), r
        dev = torch.device("cuda:0")
        self.st = vp(torch.cuda.current_stream().cuda_stream)
        g = torch.Generator(device=dev).manual_seed(seed)
        self.x = ((torch.rand(M, K, device=dev, generator=g) * 2 - 1)).bfloat16()
        self.W = ((torch.rand(N, K, device=dev, generator=g) * 2 - 1) * 0.05).bfloat16()
        self.b = torch.randn(N, device=dev, generator=g).bfloat16() if bias else None
        members = (M + rpm - 1) // rpm
        self.tp = torch.randn(members, -(-(r * (K + N) + 8) // 4) * 4, device=dev, generator=g) * 0.1  # [A | B | pad]
        self.T = torch.randn(M, max(r, 1), device=dev, generator=g)
        self.ys = [torch.empty(M, N, device=dev, dtype=torch.bfloat16) for _ in libs]
        self.ws = [torch.empty(M, max(r, 1), device=dev) for _ in libs]

    def run(self, i, kern, api="gemm"):
        M, N, K, rpm = self.dims
        r, tp = self.r, self.tp
        head = (vp(self.x.data_ptr()), i64(K), vp(self.W.data_ptr()), i64(K), vp(self.b.data_ptr() if self.b is not None else 0))
        dims = (i32(r), f32(4.0), i64(rpm), i64(M), i64(N), i64(K), vp(self.ys[i].data_ptr()), i64(N))
        if api == "gemm":
            rc = self.libs[i].eggroll_lora_gemm_sel(*head, vp(self.T.data_ptr()), vp(tp.data_ptr()), i64(tp.stride(0)),
                                                    i64(r * K), *dims, i32(kern), self.st)
        else:
            rc = self.libs[i].eggroll_lora_linear_pop_sel(*head, vp(tp.data_ptr()), i64(tp.stride(0)), i64(0), i64(r * K),
                                                          *dims, vp(self.ws[i].data_ptr()), i32(kern), self.st)
        assert rc == 0, (rc, self.libs[i].eggroll_last_error())

    def equal(self, kern, api):
        import torch
        for y, w in zip(self.ys, self.ws):
            y.fill_(float("nan"))
            w.fill_(float("nan"))
        for i in range(len(self.libs)):
            self.run(i, kern, api)
        torch.cuda.synchronize()
        # torch.equal is False on NaN: an element a library left unwritten fails the comparison too
        same = all(torch.equal(self.ys[0], y) for y in self.ys[1:])
        if api == "linear_pop" and self.r:
            same = same and all(torch.equal(self.ws[0], w) for w in self.ws[1:])
        return same

    def time(self, order, kern, rounds=5, reps=5, api="gemm"):
        """Median over rounds of the per-launch ms of each library, the libraries interleaved in `order`."""
        import torch
        ms = {i: [] for i in order}
        for _ in range(rounds):
            for i in order:
                self.run(i, kern, api)
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                for _ in range(reps):
                    self.run(i, kern, api)
                e.record()
                torch.cuda.synchronize()
                ms[i].append(s.elapsed_time(e) / reps)
        return {i: statistics.median(v) for i, v in ms.items()}


def load(paths):
    import torch  # noqa: F401  (first, as the package does: the libraries then bind the HIP runtime torch has loaded)
    libs = [ctypes.CDLL(str(Path(p).resolve())) for p in paths]
    for lib in libs:
        lib.eggroll_last_error.restype = ctypes.c_char_p
    return libs


def main(pa, pb, kern=8):
    import torch
    libs = load((pa, pb))
    for M, N, K, rpm, r, bias in ((1000, 300, 256, 300, 2, True), (1000, 300, 256, 300, 1, False),
                                  (4096, 512, 512, 256, 2, True), (2560, 1120, 1152, 640, 1, True),
                                  (3000, 700, 320, 1000, 2, False), (8192, 2240, 2240, 2048, 2, True)):
        same = Case(libs, M, N, K, rpm, r, bias).equal(kern, "gemm")
        print(json.dumps({"case": [M, N, K, rpm, r, bias], "bitwise_equal": same}), flush=True)
        assert same

    res = {}
    timed = [(131072, 2240, 2240, 16384, 2), (131072, 11200, 2240, 16384, 2), (131072, 2240, 5632, 16384, 2)]
    timed += [(8192, 2240, 2240, 2048, r) for r in (0, 2, 16)]
    for M, N, K, rpm, r in timed:
        c = Case(libs, M, N, K, rpm, r, True)
        med = c.time((0, 1), kern, reps=5 if M > 8192 else 50)   # a timed window of several ms either way
        a, b = med[0], med[1]
        tf = 2 * M * N * K / 1e9
        key = f"{M}x{N}x{K}-r{r}"
        res[key] = {"A_ms": round(a, 4), "B_ms": round(b, 4), "A_TF": round(tf / a, 1), "B_TF": round(tf / b, 1),
                    "B_vs_A": round(a / b, 4), "bitwise_equal": torch.equal(c.ys[0], c.ys[1])}
        print(json.dumps({key: res[key]}), flush=True)
        del c
    res["spread"] = round(max(abs(1 - v["A_ms"] / v["B_ms"]) for v in res.values()), 4)
    print(json.dumps(res))


def bits(pa, pb):
    libs = load((pa, pb))
    n = 0
    for M, N, K, rpm in ((600, 203, 128, 260), (300, 331, 192, 100)):   # S1, S2 of tests/test_gpu_gemm_layouts.py
        for r in (0, 1, 2, 4):
            c = Case(libs, M, N, K, rpm, r, True)
            for kern in (0, 8, 9, 10, 128):
                for api in ("gemm", "linear_pop"):
                    same = c.equal(kern, api)
                    n += 1
                    if not same:
                        print(json.dumps({"case": [M, N, K, rpm, r], "kernel": kern, "api": api, "bitwise_equal": False}))
                    assert same
    print(json.dumps({"cases": n, "bitwise_equal": True}))


if __name__ == "__main__":
    if sys.argv[1] == "build-a":
        build_a(sys.argv[2] if len(sys.argv) > 2 else "HEAD")
    elif sys.argv[1] == "bits":
        bits(sys.argv[2], sys.argv[3])
    else:
        main(sys.argv[1], sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 8)
