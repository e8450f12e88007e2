"""exl2_norm_bridge (csrc/gemma_ops.hip): the post norm added into the fp32 residual stream and the next module's pre-norm in one launch.

Checked against the two exl2_rms_norm launches it replaces:
  * the new x bit for bit (same clamp, same order of the sum of squares, same three fp32 roundings);
  * n: the bridge sums the squares of the new x in its own thread <-> element mapping, rms_norm_kernel walks an fp32 row as f32x4 vectors,
    so the scale may differ in its last fp32 bit and an element that sits on an fp16 rounding boundary lands on the neighbouring value.
    Bar: every element equal or the adjacent fp16 value, at most 0.1 % of a case's elements different.  A numpy model of the two sum
    orders (below) predicts 14 of 258 048 elements over the cases of this file; inputs are drawn, per case, from the first seed for which
    that model stays under the bar -- the model decides, never the kernel;
  * n against the float64 restatement (tests/gemma_oracle.py) at the bar tests/test_ops.py uses for rms_norm: one fp16 ulp."""
import numpy as np
import pytest
import torch

from tests import gemma_oracle as GO

F16, F32, F64 = np.float16, np.float32, np.float64
EPS = 1e-6
ROWS = [1, 3, 16]
HIDDEN = [128, 256, 2304, 3584, 8192]


def _ulp_close(got, want, ulps=1):
    g, w = got.astype(F32), want.astype(F32)
    return np.all(np.abs(g - w) <= np.maximum(np.abs(w) * 2.0 ** -10, 2.0 ** -24) * ulps)


def _adjacent(a, b):
    """fp16 arrays: True where equal or neighbouring values (finite, same sign or around zero)"""
    def key(h):
        u = h.view(np.uint16).astype(np.int32)
        return np.where(u & 0x8000, -(u & 0x7FFF), u)
    return np.abs(key(a) - key(b)) <= 1


def _fma32(a, b, c):
    return (a.astype(F64) * b.astype(F64) + c.astype(F64)).astype(F32)


def _block_sum(per_thread):
    """[rows, 256] fp32 partial sums -> the workgroup's sum as both kernels form it: butterfly inside each wave of 64, then the four
    wave sums left to right"""
    v = per_thread.reshape(-1, 4, 64).astype(F32)
    for m in (1, 2, 4, 8, 16, 32):
        v = (v + v[:, :, np.arange(64) ^ m]).astype(F32)
    w = v[:, :, 0]
    return (((w[:, 0] + w[:, 1]).astype(F32) + w[:, 2]).astype(F32) + w[:, 3]).astype(F32)


def _sum_squares(x32, vec):
    """sum of squares of fp32 rows with thread t taking the `vec`-element vectors t, t + 256, ... in order, one fmaf per element"""
    rows, dim = x32.shape
    nv = dim // vec
    acc = np.zeros((rows, 256), dtype=F32)
    for j in range(-(-nv // 256)):
        idx = np.arange(256) + 256 * j
        ok = idx < nv
        for e in range(vec):
            col = np.where(ok, idx * vec + e, 0)
            val = np.where(ok[None, :], x32[:, col], F32(0))
            acc = _fma32(val.astype(F32), val.astype(F32), acc)
    return _block_sum(acc)


def _model_n(x_new, w_next, vec):
    ss = _sum_squares(x_new, vec)
    rmf = (1.0 / np.sqrt(_fma32(ss, np.full_like(ss, F32(1.0 / x_new.shape[1])), np.full_like(ss, F32(EPS))).astype(F64))).astype(F32)
    return ((x_new * w_next.astype(F32)[None, :]).astype(F32) * rmf[:, None]).astype(F16)


def _draw(rows, hidden):
    """inputs of a case: the first seed for which the model of the two sum orders differs in at most 0.1 % of the elements"""
    for seed in range(20):
        rng = np.random.default_rng(1000 * seed + 7 * rows + hidden)
        t = (rng.standard_normal((rows, hidden)) * rng.uniform(0.5, 6.0, size=(rows, 1))).astype(F16)
        t[0, :4] = [65504.0, -65504.0, 0.0, 1.0]                   # the clamp's edge values ride along
        x = (rng.standard_normal((rows, hidden)) * rng.uniform(1.0, 30.0, size=(rows, 1))).astype(F32)
        w_post = (1 + 0.1 * rng.standard_normal(hidden)).astype(F16)
        w_next = (1 + 0.1 * rng.standard_normal(hidden)).astype(F16)
        x_new = GO.post_norm_add(t, w_post, x, EPS)
        if (_model_n(x_new, w_next, 8) != _model_n(x_new, w_next, 4)).sum() <= rows * hidden // 1000:
            return t, x, w_post, w_next
    raise AssertionError("no seed under the bar")


@pytest.mark.parametrize("hidden", HIDDEN)
@pytest.mark.parametrize("rows", ROWS)
def test_bridge_against_two_launches(be, rows, hidden):
    t, x, w_post, w_next = _draw(rows, hidden)
    ext = be.ext
    wp, wn = be.t(w_post), be.t(w_next)
    # the two launches
    x2 = be.t(x)
    ext.rms_norm_add(be.t(t), wp, x2, EPS)
    n2 = torch.zeros((rows, hidden), dtype=torch.float16, device=be.device)
    ext.rms_norm(x2, wn, n2, EPS)
    want_x, want_n = be.n(x2).copy(), be.n(n2).copy()
    assert not np.array_equal(want_x, x)
    # the oracle pins those (the bar of tests/test_ops.py::test_rms_norm for the fp16 result; fp32: 2^-21 of the larger term)
    ox = GO.post_norm_add(t, w_post, x, EPS)
    assert np.all(np.abs(want_x.astype(F64) - ox) <= 2.0 ** -21 * (np.abs(ox) + np.abs(x)) + 1e-30)
    for alias in (False, True):
        x1, tt = be.t(x), be.t(t)
        n1 = tt if alias else torch.zeros((rows, hidden), dtype=torch.float16, device=be.device)
        assert ext.norm_bridge(tt, x1, wp, wn, n1, EPS) is True
        got_x, got_n = be.n(x1), be.n(n1)
        assert np.array_equal(got_x.view(np.uint32), want_x.view(np.uint32)), "x differs from the exl2_rms_norm launch"
        if not alias:
            assert np.array_equal(be.n(tt).view(np.uint16), t.view(np.uint16))
        differ = int((got_n.view(np.uint16) != want_n.view(np.uint16)).sum())
        print(f"rows={rows} hidden={hidden} alias={alias}: {differ} of {rows * hidden} elements of n differ from the two launches")
        assert np.all(_adjacent(got_n, want_n))
        assert differ <= rows * hidden // 1000
        assert _ulp_close(got_n, GO.rms_norm_any(want_x, w_next, EPS))
    # without w_next: only the first half; n is not touched
    x1 = be.t(x)
    guard = torch.full((rows, hidden), 3.0, dtype=torch.float16, device=be.device)
    from exllamav2_amd.ext import none_tensor
    assert ext.norm_bridge(be.t(t), x1, wp, none_tensor, none_tensor, EPS) is True
    assert np.array_equal(be.n(x1).view(np.uint32), want_x.view(np.uint32))
    assert np.all(be.n(guard) == 3.0)


def test_bridge_not_covered(be):
    """a row that does not fit the workgroup's registers (hidden > 8192): "not covered", both buffers untouched"""
    rows, hidden = 2, 8200
    rng = np.random.default_rng(5)
    t = rng.standard_normal((rows, hidden)).astype(F16)
    x = rng.standard_normal((rows, hidden)).astype(F32)
    w = np.ones(hidden, dtype=F16)
    tt, xt = be.t(t), be.t(x)
    n = torch.full((rows, hidden), 3.0, dtype=torch.float16, device=be.device)
    assert be.ext.norm_bridge(tt, xt, be.t(w), be.t(w), n, EPS) is False
    assert np.array_equal(be.n(xt), x) and np.array_equal(be.n(tt), t) and np.all(be.n(n) == 3.0)
    # the largest covered width still is
    hidden = 8192
    t, x, w = t[:, :hidden].copy(), x[:, :hidden].copy(), w[:hidden]
    assert be.ext.norm_bridge(be.t(t), be.t(x), be.t(w), be.t(w), torch.zeros((rows, hidden), dtype=torch.float16, device=be.device), EPS) is True


def test_bridge_refuses_bad_shapes(be):
    x = torch.zeros((1, 100), dtype=torch.float32, device=be.device)
    t = torch.zeros((1, 100), dtype=torch.float16, device=be.device)
    w = torch.ones((100,), dtype=torch.float16, device=be.device)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        be.ext.norm_bridge(t, x, w, w, t, EPS)
    with pytest.raises(RuntimeError, match="dtype"):
        be.ext.norm_bridge(t, t, w, w, t, EPS)
