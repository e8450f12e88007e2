"""exl2_parallel_bridge (csrc/layer_norm.hip): the two fp16 adds that end a parallel decoder block (parallel_decoder.py:141-142) and the
LayerNorm that opens the next one, in one launch -- checked BIT FOR BIT against the launches it replaces (add_f16_, add_f16_, layer_norm):
both go through the row routine of csrc/layer_norm.h.  The separate launches are pinned on the float64 restatement by
tests/test_layer_norm_op.py; the adds are pinned here."""
import numpy as np
import pytest
import torch

from exllamav2_amd.ext import none_tensor
from tests import layernorm_oracle as LO

F16 = np.float16
EPS = 1e-5
ROWS = [1, 3, 17]
DIMS = [128, 136, 4608, 16384]


def _inputs(rows, dim):
    rng = np.random.default_rng(9000 + 13 * rows + dim)
    x = (rng.standard_normal((rows, dim)) * 4.0 + 1.0).astype(F16)
    a = (rng.standard_normal((rows, dim)) * 2.0).astype(F16)
    b = (rng.standard_normal((rows, dim)) * 2.0).astype(F16)
    x[0, :2] = [65504.0, -65504.0]; a[0, :2] = [65504.0, -65504.0]                 # an fp16 add that overflows rides along
    w = (1 + 0.2 * rng.standard_normal(dim)).astype(F16)
    bias = (0.5 * rng.standard_normal(dim)).astype(F16)
    return x, a, b, w, bias


def _guarded(be, arr):
    """the rows of arr with a guard row behind them"""
    buf = torch.full((arr.shape[0] + 1, arr.shape[1]), 3.0, dtype=torch.float16, device=be.device)
    buf[:arr.shape[0]] = be.t(arr)
    return buf


def _bits(be, t):
    return be.n(t).copy().view(np.uint16)


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("rows", ROWS)
def test_bridge_against_separate_launches(be, rows, dim):
    x, a, b, w, bias = _inputs(rows, dim)
    ext = be.ext
    wt = be.t(w)
    for bt in (none_tensor, be.t(bias)):
        # the separate launches
        x2, a2, b2 = be.t(x), be.t(a), be.t(b)
        ext.add_f16_(x2, a2)
        ext.add_f16_(x2, b2)
        n2 = torch.zeros((rows, dim), dtype=torch.float16, device=be.device)
        ext.layer_norm(x2, wt, bt, n2, EPS)
        want_x, want_n = _bits(be, x2), _bits(be, n2)
        assert np.array_equal(want_x, LO.hadd(LO.hadd(x, a), b).view(np.uint16)), "the adds are not two fp16 adds in order"
        # the bridge, two copies
        xg, ag, bg = _guarded(be, x), be.t(a), be.t(b)
        n0g, n1g = _guarded(be, np.zeros_like(x)), _guarded(be, np.zeros_like(x))
        assert ext.parallel_bridge(xg[:rows], ag, bg, wt, bt, n0g[:rows], n1g[:rows], EPS) is True
        assert np.array_equal(_bits(be, xg[:rows]), want_x), "x differs from the separate launches"
        assert np.array_equal(_bits(be, n0g[:rows]), want_n) and np.array_equal(_bits(be, n1g[:rows]), want_n), "n differs"
        assert np.array_equal(_bits(be, ag), a.view(np.uint16)) and np.array_equal(_bits(be, bg), b.view(np.uint16)), "a / b were written"
        for g in (xg, n0g, n1g):
            assert np.all(be.n(g)[rows] == 3.0), "a guard row was written"
        # n0 over a and n1 over b: what a decode step does (the attention and the MLP ran in place on the two normed copies)
        x1, a1, b1 = be.t(x), be.t(a), be.t(b)
        assert ext.parallel_bridge(x1, a1, b1, wt, bt, a1, b1, EPS) is True
        assert np.array_equal(_bits(be, x1), want_x) and np.array_equal(_bits(be, a1), want_n) and np.array_equal(_bits(be, b1), want_n)


@pytest.mark.parametrize("dim", [136, 4608])
def test_bridge_null_forms(be, dim):
    rows = 3
    x, a, b, w, bias = _inputs(rows, dim)
    ext = be.ext
    wt, bt = be.t(w), be.t(bias)
    # norm only (the head of layer 0): x is read, never written
    xt = be.t(x)
    n_want = torch.zeros((rows, dim), dtype=torch.float16, device=be.device)
    ext.layer_norm(xt, wt, bt, n_want, EPS)
    n0g, n1g = _guarded(be, np.zeros_like(x)), _guarded(be, np.zeros_like(x))
    assert ext.parallel_bridge(xt, none_tensor, none_tensor, wt, bt, n0g[:rows], n1g[:rows], EPS) is True
    assert np.array_equal(_bits(be, xt), x.view(np.uint16))
    assert np.array_equal(_bits(be, n0g[:rows]), _bits(be, n_want)) and np.array_equal(_bits(be, n1g[:rows]), _bits(be, n_want))
    assert np.all(be.n(n0g)[rows] == 3.0) and np.all(be.n(n1g)[rows] == 3.0)
    # one copy
    n0g = _guarded(be, np.zeros_like(x))
    assert ext.parallel_bridge(xt, none_tensor, none_tensor, wt, bt, n0g[:rows], none_tensor, EPS) is True
    assert np.array_equal(_bits(be, n0g[:rows]), _bits(be, n_want)) and np.all(be.n(n0g)[rows] == 3.0)
    # adds only: n0 / n1 are not touched
    xg = _guarded(be, x)
    n0 = torch.full((rows, dim), 3.0, dtype=torch.float16, device=be.device)
    assert ext.parallel_bridge(xg[:rows], be.t(a), be.t(b), none_tensor, none_tensor, n0, n0, EPS) is True
    assert np.array_equal(_bits(be, xg[:rows]), LO.hadd(LO.hadd(x, a), b).view(np.uint16))
    assert np.all(be.n(xg)[rows] == 3.0) and np.all(be.n(n0) == 3.0)


@pytest.mark.parametrize("dim", [132, 16392])
def test_bridge_declines(be, dim):
    """a shape layer_norm does not cover: False, every buffer untouched"""
    rows = 2
    rng = np.random.default_rng(5)
    x, a, b = (rng.standard_normal((rows, dim)).astype(F16) for _ in range(3))
    w = np.ones(dim, dtype=F16)
    xt, at, bt = be.t(x), be.t(a), be.t(b)
    n0 = torch.full((rows, dim), 3.0, dtype=torch.float16, device=be.device)
    n1 = torch.full((rows, dim), 3.0, dtype=torch.float16, device=be.device)
    assert be.ext.parallel_bridge(xt, at, bt, be.t(w), none_tensor, n0, n1, EPS) is False
    assert np.array_equal(be.n(xt), x) and np.array_equal(be.n(at), a) and np.array_equal(be.n(bt), b)
    assert np.all(be.n(n0) == 3.0) and np.all(be.n(n1) == 3.0)


def test_bridge_refuses_bad_arguments(be):
    x = torch.zeros((2, 64), dtype=torch.float16, device=be.device)
    w = torch.ones((64,), dtype=torch.float16, device=be.device)
    with pytest.raises(RuntimeError, match="come together"):
        be.ext.parallel_bridge(x, x.clone(), none_tensor, w, none_tensor, x.clone(), none_tensor, EPS)
    with pytest.raises(RuntimeError, match="incompatible"):
        be.ext.parallel_bridge(x, none_tensor, none_tensor, w[:32], none_tensor, x.clone(), none_tensor, EPS)
    with pytest.raises(RuntimeError, match="nothing to do"):
        be.ext.parallel_bridge(x, none_tensor, none_tensor, none_tensor, none_tensor, none_tensor, none_tensor, EPS)
