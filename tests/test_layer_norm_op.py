"""exl2_layer_norm (csrc/layer_norm.hip) against the float64 restatement of layer_norm.cu (tests/layernorm_oracle.py).

Bar: one fp16 ulp of the largest magnitude among the pre-bias value, the bias, the residual and the result: a flip of the normed value to
the neighbouring fp16 value is the only admissible difference, and the fp16 adds of the bias and the residual behind that rounding point
can cancel, which is why the ulp is taken at the largest operand and not at the result.  The kernel accumulates its two row sums in fp64
(csrc/layer_norm.h), so such a flip needs the restatement's own last float64 bit to decide an fp32 rounding; with fp32 sums an element
next to the mean differs by many ulps between two summation orders and the bar is out of reach.  Every case prints how many elements
differ at all.  The restatement itself is pinned on values the reference's own nn.LayerNorm produced (tests/golden/reference_layernorm.npz)."""
import os

import numpy as np
import pytest
import torch

from exllamav2_amd.ext import none_tensor
from tests import layernorm_oracle as LO

F16, F32, F64 = np.float16, np.float32, np.float64
EPS = 1e-5
DIMS = [128, 136, 3072, 4608, 8192, 16384]     # 136: does not fill a wave; 4608: 2.25 vectors per thread; 16384: the widest covered row
ROWS = [1, 3, 17]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_layernorm.npz")


def _inputs(rows, dim, seed=0):
    rng = np.random.default_rng(7000 + 31 * rows + dim + seed)
    x = (rng.standard_normal((rows, dim)) * rng.uniform(0.5, 8.0, size=(rows, 1)) + rng.uniform(-3.0, 3.0, size=(rows, 1))).astype(F16)
    w = (1 + 0.2 * rng.standard_normal(dim)).astype(F16)
    b = (0.5 * rng.standard_normal(dim)).astype(F16)
    res = (rng.standard_normal((rows, dim)) * 2.0).astype(F16)
    return x, w, b, res


def _check(got, want, tol, what):
    err = np.abs(got.astype(F64) - want.astype(F64))
    bad = err > tol
    print(f"{what}: max err / tol = {float((err / tol).max()):.3f}, {int((got.view(np.uint16) != want.view(np.uint16)).sum())} of {got.size} differ")
    assert not bad.any(), (what, int(bad.sum()), float((err / tol).max()))


def _run(be, x, w, b, res=None, in_place=False):
    """y (with a guard row behind it that must stay untouched), through the public binding"""
    rows, dim = x.shape
    wt = be.t(w)
    bt = none_tensor if b is None else be.t(b)
    if in_place:
        buf = torch.full((rows + 1, dim), 3.0, dtype=torch.float16, device=be.device)
        buf[:rows] = be.t(x)
        be.ext.layer_norm_(buf[:rows], wt, bt, EPS)
    else:
        buf = torch.full((rows + 1, dim), 3.0, dtype=torch.float16, device=be.device)
        xt = be.t(x)
        if res is not None:
            buf[:rows] = be.t(res)
            be.ext.layer_norm_add(xt, wt, bt, buf[:rows], EPS)
        else:
            be.ext.layer_norm(xt, wt, bt, buf[:rows], EPS)
        assert np.array_equal(be.n(xt).view(np.uint16), x.view(np.uint16)), "x was written"
    out = be.n(buf)
    assert np.all(out[rows] == 3.0), "the row behind y was written"
    return out[:rows].copy()


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("rows", ROWS)
def test_layer_norm(be, rows, dim):
    x, w, b, res = _inputs(rows, dim)
    for bias in (None, b):
        want, tol = LO.layer_norm_tol(x, w, bias, EPS)
        got = _run(be, x, w, bias)
        _check(got, want, tol, f"rows={rows} dim={dim} bias={bias is not None}")
        got_ip = _run(be, x, w, bias, in_place=True)
        assert np.array_equal(got_ip.view(np.uint16), got.view(np.uint16)), "in place differs from out of place"
        want_r, tol_r = LO.layer_norm_tol(x, w, bias, EPS, res)
        _check(_run(be, x, w, bias, res=res), want_r, tol_r, f"rows={rows} dim={dim} bias={bias is not None} add_residual")


@pytest.mark.parametrize("dim", [136, 4608])
def test_layer_norm_large_mean_small_variance(be, dim):
    """mean 200, sigma 0.5: E[x^2] - mean^2 in fp32 has no bit of the variance left (40000 +- 2^-8 against 0.25)"""
    rng = np.random.default_rng(11 + dim)
    x = (200.0 + 0.5 * rng.standard_normal((3, dim))).astype(F16)
    w = (1 + 0.2 * rng.standard_normal(dim)).astype(F16)
    b = (0.5 * rng.standard_normal(dim)).astype(F16)
    want, tol = LO.layer_norm_tol(x, w, b, EPS)
    assert float(np.abs(want.astype(F64)).max()) > 1.0           # a normalised row, not a flat one
    # what a one-pass variance gives is outside the bar: the case can tell the two apart
    xf = x.astype(F32)
    var1 = np.maximum((xf * xf).mean(axis=-1, dtype=F32) - xf.mean(axis=-1, dtype=F32) ** 2, 0)
    one_pass = (((xf - xf.mean(axis=-1, keepdims=True)) * w.astype(F32)) / np.sqrt(var1 + F32(EPS))[:, None]).astype(F16)
    assert (np.abs(LO.hadd(one_pass, np.broadcast_to(b, one_pass.shape)).astype(F64) - want.astype(F64)) > tol).any()
    _check(_run(be, x, w, b), want, tol, f"mean 200 dim={dim}")


@pytest.mark.parametrize("dim", [128, 3072])
def test_layer_norm_extreme_values(be, dim):
    """rows holding +-65504 (the clamp's edge): finite results, the bar holds"""
    rng = np.random.default_rng(13 + dim)
    x = rng.standard_normal((3, dim)).astype(F16)
    x[0, :4] = [65504.0, -65504.0, 0.0, 1.0]
    x[1, 5] = 65504.0
    x[2, -1] = -65504.0
    w = (1 + 0.2 * rng.standard_normal(dim)).astype(F16)
    want, tol = LO.layer_norm_tol(x, w, None, EPS)
    assert np.all(np.isfinite(want.astype(F32)))
    _check(_run(be, x, w, None), want, tol, f"+-65504 dim={dim}")


@pytest.mark.parametrize("dim", [132, 16392])
def test_layer_norm_shape_not_covered(be, dim):
    """dim no multiple of 8, dim above 16384: reported, nothing written"""
    x = torch.ones((2, dim), dtype=torch.float16, device=be.device)
    w = torch.ones((dim,), dtype=torch.float16, device=be.device)
    y = torch.full((2, dim), 3.0, dtype=torch.float16, device=be.device)
    with pytest.raises(RuntimeError, match="shape not covered"):
        be.ext.layer_norm(x, w, none_tensor, y, EPS)
    with pytest.raises(RuntimeError, match="shape not covered"):
        be.ext.layer_norm_(x, w, w, EPS)
    assert np.all(be.n(y) == 3.0) and np.all(be.n(x) == 1.0)


def test_layer_norm_refuses_bad_arguments(be):
    x = torch.zeros((2, 64), dtype=torch.float16, device=be.device)
    w = torch.ones((64,), dtype=torch.float16, device=be.device)
    with pytest.raises(RuntimeError, match="must be half"):
        be.ext.layer_norm(x.float(), w, none_tensor, x, EPS)
    with pytest.raises(RuntimeError, match="incompatible"):
        be.ext.layer_norm(x, w[:32], none_tensor, x, EPS)
    with pytest.raises(RuntimeError, match="shaped like w"):
        be.ext.layer_norm(x, w, w[:32], x, EPS)


def test_restatement_against_reference_layernorm():
    """tests/golden/make_golden_layernorm.py: the reference's ExLlamaV2LayerNorm.forward_torch (its nn.LayerNorm) on an fp32 copy of fp16
    inputs.  The restatement rounds the normed value to fp16 (half an ulp) and adds the bias in fp16 (half an ulp of the result): one fp16
    ulp of the larger of the two, plus the fp32 arithmetic of nn.LayerNorm (2^-20 relative, far below)."""
    fx = np.load(GOLDEN)
    assert int(fx["n_cases"]) == 4
    for i in range(int(fx["n_cases"])):
        x, w, y, eps = fx[f"x_{i}"], fx[f"w_{i}"], fx[f"y_{i}"], float(fx[f"eps_{i}"])
        b = fx[f"b_{i}"] if f"b_{i}" in fx.files else None
        assert x.dtype == F16 and w.dtype == F16 and y.dtype == F32
        got, pre = LO.layer_norm(x, w, b, eps, parts=True)
        mag = np.maximum(np.abs(pre.astype(F64)), np.abs(y.astype(F64)))
        err = np.abs(got.astype(F64) - y.astype(F64))
        print(f"case {i}: dim {x.shape[1]} bias {b is not None}: max err / ulp = {float((err / LO.ulp16(mag)).max()):.3f}")
        assert np.all(err <= LO.ulp16(mag) * (1.0 + 2.0 ** -8))
