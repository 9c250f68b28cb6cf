"""LoRA GEMM test cases shared by tests/test_gpu_kernels.py and tests/test_gpu_gemm_layouts.py: the random
operands, the fp64 oracle and the bound a bf16 LoRA linear is held to against it."""
import math

import numpy as np
import torch

from oracle import eggroll_oracle as O


def lora_case(dev, M, N, Kd, r, rpm, bias=True, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, Kd, generator=g).to(torch.bfloat16).to(dev)
    W = (torch.randn(N, Kd, generator=g) * 0.05).to(torch.bfloat16).to(dev)
    b = torch.randn(N, generator=g).to(torch.bfloat16).to(dev) if bias else None
    nm = -(-M // rpm)
    D = r * Kd + N * r + 5
    ld = -(-D // 4) * 4
    tp = (torch.randn(nm, ld, generator=g) * 0.1).to(dev)
    offA, offB = 4, 4 + r * Kd
    return x, W, b, tp, offA, offB


def lora_ref(x, W, b, tp, offA, offB, r, scale, rpm):
    return O.ref_lora_linear_pop(x.float().cpu().numpy(), W.float().cpu().numpy(),
                                 None if b is None else b.float().cpu().numpy(), tp.cpu().numpy(), offA, offB, r,
                                 scale, rpm)


def lora_tol(ref, Kd):
    """Allowed |kernel - fp64 oracle| per element: bf16 output rounding (2^-9 relative) + fp32 accumulation
    over K, plus an absolute floor."""
    return 2 ** -8 * np.abs(ref) + 2e-4 * math.sqrt(Kd) * np.abs(ref).std() + 1e-3
