"""tests/gemma_oracle.py's norm pinned on the reference: tests/golden/reference_gemma_norm.npz holds what the reference's
ExLlamaV2RMSNorm.forward_torch (rmsnorm.py:183-208) returns for fp32 input / fp32 output and a weight with the constant bias 1 added in
fp16 at load (tests/golden/make_golden_gemma.py).  Bar, in units of 2^-24 relative: the restatement rounds the scale and two products
(3); forward_torch forms the mean in fp32 (1 after the square root halves it), takes an fp32 rsqrt (2: one ulp) and rounds (x * r) and
its product with w (2) -- 8 in all, 2^-21.  The fp16 form: one fp16 ulp."""
import os

import numpy as np

from tests import gemma_oracle as GO
from tests.conftest import ROOT

F16, F64 = np.float16, np.float64


def test_oracle_norm_matches_the_reference_forward_torch():
    fx = np.load(os.path.join(ROOT, "tests", "golden", "reference_gemma_norm.npz"))
    assert int(fx["n_cases"]) == 2 and {fx["x_0"].shape[1], fx["x_1"].shape[1]} == {128, 2304}
    for i in range(int(fx["n_cases"])):
        x, w_raw, y, eps = fx[f"x_{i}"], fx[f"w_raw_{i}"], fx[f"y_{i}"], float(fx[f"eps_{i}"])
        assert x.dtype == np.float32 and y.dtype == np.float32 and w_raw.dtype == F16
        w = (w_raw + F16(float(fx["bias"]))).astype(F16)                                  # the load-time bias, in fp16
        got = GO.rms_norm_any(x, w, eps, out_f32=True)
        assert np.all(np.abs(got.astype(F64) - y.astype(F64)) <= 2.0 ** -21 * np.abs(y.astype(F64)) + 1e-30)
        got16 = GO.rms_norm_any(x, w, eps)
        assert np.all(np.abs(got16.astype(F64) - y.astype(F64)) <= 2.0 ** -10 * np.abs(y.astype(F64)) + 2.0 ** -24)
        # added to a stream: x + norm(t) with t the fp16 rounding of the same rows (clamped input path)
        t = x.astype(F16)
        s = GO.post_norm_add(t, w, x, eps)
        assert s.dtype == np.float32 and np.all(np.abs(s.astype(F64) - (x.astype(F64) + GO.rms_norm_any(t, w, eps, out_f32=True))) <= 2.0 ** -23 * np.abs(s) + 1e-30)
