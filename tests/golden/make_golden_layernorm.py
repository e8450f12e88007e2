#!/usr/bin/env python3
"""Generates tests/golden/reference_layernorm.npz by EXECUTING the reference's ExLlamaV2LayerNorm.forward_torch (layernorm.py:128-145):
the nn.LayerNorm its load() builds (layernorm.py:50-59: elementwise affine, bias only when the checkpoint has one, torch's default
eps -- load() does not hand norm_eps to it).

forward_torch reads nothing but `layernorm` from the module, so a SimpleNamespace stands in for it.  Inputs and weights are fp16
values; the module runs on fp32 copies of them (torch's CPU layer_norm wants one dtype), which is exact.  Recorded: x, w, b (where the
case has a bias), the fp32 output and the eps of the nn.LayerNorm; dims 128 and 3072, with and without bias, 3 rows.

Run from the repo root, where the reference tree is present:  python tests/golden/make_golden_layernorm.py
"""
import os
import sys
from types import SimpleNamespace as NS

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

CASES = [(128, False), (128, True), (3072, False), (3072, True)]
ROWS = 3


def inputs(i: int):
    dim, bias = CASES[i]
    rng = np.random.default_rng(1300 + i)
    x = (rng.standard_normal((ROWS, dim)) * rng.uniform(0.5, 20.0, size=(ROWS, 1)) + rng.uniform(-4.0, 4.0, size=(ROWS, 1))).astype(np.float16)
    w = (1 + 0.2 * rng.standard_normal(dim)).astype(np.float16)
    b = (0.5 * rng.standard_normal(dim)).astype(np.float16) if bias else None
    return x, w, b


def main():
    from make_golden import import_reference
    import_reference()
    import torch
    from torch import nn
    from exllamav2.layernorm import ExLlamaV2LayerNorm
    fx = {"n_cases": np.int32(len(CASES))}
    for i, (dim, bias) in enumerate(CASES):
        x, w, b = inputs(i)
        ln = nn.LayerNorm(dim, elementwise_affine=True, bias=bias)                  # layernorm.py:50-52
        ln.weight = nn.Parameter(torch.from_numpy(w.copy()).float(), requires_grad=False)
        if bias:
            ln.bias = nn.Parameter(torch.from_numpy(b.copy()).float(), requires_grad=False)
        with torch.inference_mode():
            y = ExLlamaV2LayerNorm.forward_torch(NS(layernorm=ln), torch.from_numpy(x.copy()).float())
        assert y.dtype == torch.float32
        fx[f"x_{i}"], fx[f"w_{i}"], fx[f"y_{i}"], fx[f"eps_{i}"] = x, w, y.numpy(), np.float64(ln.eps)
        if bias:
            fx[f"b_{i}"] = b
    path = os.path.join(ROOT, "tests", "golden", "reference_layernorm.npz")
    np.savez_compressed(path, **fx)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    sys.exit(main())
