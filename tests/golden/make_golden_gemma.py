#!/usr/bin/env python3
"""Generates tests/golden/reference_gemma_norm.npz by EXECUTING the reference's ExLlamaV2RMSNorm.forward_torch (rmsnorm.py:183-208) the
way a Gemma-2 / Gemma-3 block uses it: fp32 input (the fp32 residual stream, architecture.py:576, :601), fp32 output, and a weight that
had the architecture's constant bias 1 added in fp16 at load (rmsnorm.py:57-59).

The reference's host layer is importable Python: import_reference() of make_golden.py puts a stub in place of its compiled extension,
and forward_torch reads nothing but `weight` and `variance_epsilon` from the module -- a SimpleNamespace stands in for it.  Recorded:
the raw weight (before the bias), the input and the output, hidden 128 and 2304, 3 rows, eps 1e-6.  The embedding scaling
(embedding.py:184-187) and the logit cap (model.py:1043-1044 -> ext_c.softcap_) run only inside a loaded model resp. the compiled
extension and are not recorded.

Run from the repo root, where the reference tree is present:  python tests/golden/make_golden_gemma.py
"""
import os
import sys
from types import SimpleNamespace as NS

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

CASES = [(128, 1e-6), (2304, 1e-6)]
ROWS = 3
BIAS = 1.0


def inputs(i: int):
    dim, _ = CASES[i]
    rng = np.random.default_rng(1200 + i)
    x = (rng.standard_normal((ROWS, dim)) * rng.uniform(0.5, 40.0, size=(ROWS, 1))).astype(np.float32)
    w_raw = (0.1 * rng.standard_normal(dim)).astype(np.float16)
    return x, w_raw


def main():
    from make_golden import import_reference
    import_reference()
    import torch
    from exllamav2.rmsnorm import ExLlamaV2RMSNorm
    fx = {"n_cases": np.int32(len(CASES)), "bias": np.float64(BIAS)}
    for i, (dim, eps) in enumerate(CASES):
        x, w_raw = inputs(i)
        weight = torch.from_numpy(w_raw.copy())
        weight += BIAS                                           # rmsnorm.py:58-59, in the weight's own dtype
        mod = NS(weight=weight, variance_epsilon=eps)
        y = ExLlamaV2RMSNorm.forward_torch(mod, torch.from_numpy(x.copy()), output_fp32=True)
        assert y.dtype == torch.float32
        fx[f"x_{i}"], fx[f"w_raw_{i}"], fx[f"y_{i}"], fx[f"eps_{i}"] = x, w_raw, y.numpy(), np.float64(eps)
    path = os.path.join(ROOT, "tests", "golden", "reference_gemma_norm.npz")
    np.savez_compressed(path, **fx)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    sys.exit(main())
