#!/usr/bin/env python3
"""Generates tests/golden/reference_head_norm.npz by EXECUTING the reference's ExLlamaV2HeadNorm.forward_torch (headnorm.py:145-177).

The reference's host layer is importable Python: import_reference() of make_golden.py puts a stub in place of its compiled extension,
and forward_torch reads nothing but `weight`, `variance_epsilon` and `archparams.headnorm` from the module -- a SimpleNamespace stands
in for it.  Recorded: inputs and outputs for the RMS and the LayerNorm form, head_dim 64 / 128 / 256, 3 rows x 4 heads, eps 1e-5 and
1e-6; finite inputs only (forward_torch has no clamp).

Run from the repo root, where the reference tree is present:  python tests/golden/make_golden_headnorm.py
"""
import os
import sys
from types import SimpleNamespace as NS

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

CASES = [(form, hd, eps) for form in ("rmsnorm", "layernorm") for hd in (64, 128, 256) for eps in (1e-5, 1e-6)]
ROWS, HEADS = 3, 4


def inputs(i: int):
    form, hd, eps = CASES[i]
    rng = np.random.default_rng(900 + i)
    x = (rng.standard_normal((ROWS, HEADS, hd)) * rng.uniform(0.3, 4.0, size=(ROWS, HEADS, 1)) + 0.25).astype(np.float16)
    w = (1 + 0.1 * rng.standard_normal((HEADS, hd))).astype(np.float16)
    return x, w


def main():
    from make_golden import import_reference
    import_reference()
    import torch
    from exllamav2.headnorm import ExLlamaV2HeadNorm
    fx = {"n_cases": np.int32(len(CASES))}
    for i, (form, hd, eps) in enumerate(CASES):
        x, w = inputs(i)
        mod = NS(weight=torch.from_numpy(w), variance_epsilon=eps, archparams=NS(headnorm=form))
        y = ExLlamaV2HeadNorm.forward_torch(mod, torch.from_numpy(x.copy()))
        fx[f"x_{i}"], fx[f"w_{i}"], fx[f"y_{i}"] = x, w, y.numpy().astype(np.float16)
        fx[f"eps_{i}"], fx[f"rms_{i}"] = np.float64(eps), np.bool_(form == "rmsnorm")
    path = os.path.join(ROOT, "tests", "golden", "reference_head_norm.npz")
    np.savez_compressed(path, **fx)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    sys.exit(main())
