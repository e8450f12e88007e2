"""exl2_softcap / ext.softcap_ (csrc/gemma_ops.hip): x = cap * tanh(x / cap) in place (ext_element.cpp:28-50 -> softcap.cu:8-64).

Bars (derived): fp32 -- the kernel is a division, tanhf and a product, each within 2 ulp of fp32, so 2^-20 relative to the float64 value;
fp16 -- that fp32 value rounded to nearest: equal to the rounded float64 value or the neighbouring fp16 value.  Every one of `numel`
elements is processed for any numel (the reference's fp16 launch mishandles an odd one) and the 8 elements behind the buffer stay."""
import numpy as np
import pytest
import torch

from tests import gemma_oracle as GO

F16, F32, F64 = np.float16, np.float32, np.float64
GUARD = 8


def _values(numel, cap, dtype, seed):
    rng = np.random.default_rng(seed)
    v = (rng.standard_normal(numel) * rng.choice([0.5, 10.0, 80.0, 3000.0], size=numel)).astype(F64)
    edge = [0.0, 65504.0, -65504.0, cap, -cap]
    pos = rng.permutation(numel)[:len(edge)]
    for p, e in zip(pos, edge[:numel] if numel < len(edge) else edge):
        v[p] = e
    return v.astype(dtype)


def _adjacent16(a, b):
    def key(h):
        u = h.view(np.uint16).astype(np.int32)
        return np.where(u & 0x8000, -(u & 0x7FFF), u)
    return np.abs(key(a) - key(b)) <= 1


@pytest.mark.parametrize("dtype", [F16, F32], ids=["fp16", "fp32"])
@pytest.mark.parametrize("cap", [30.0, 50.0])
@pytest.mark.parametrize("numel", [1, 2, 7, 320, 2049])
def test_softcap(be, numel, cap, dtype):
    x = _values(numel, cap, dtype, numel + int(cap))
    buf = np.concatenate([x, np.full(GUARD, 7.0, dtype=dtype)])
    bt = be.t(buf)
    be.ext.softcap_(bt[:numel], cap)
    got = be.n(bt)
    assert np.all(got[numel:] == 7.0), "elements behind the buffer were touched"
    want = GO.softcap(x, cap)
    if dtype == F32:
        err = np.abs(got[:numel].astype(F64) - want)
        assert np.all(err <= 2.0 ** -20 * np.abs(want) + 1e-38)
    else:
        assert np.all(_adjacent16(got[:numel], want.astype(F16)))
    # the cap holds and zero stays zero
    assert np.all(np.abs(got[:numel].astype(F64)) <= cap) and np.all(got[:numel][x == 0] == 0)


def test_softcap_unaligned_start(be):
    """a view that starts inside a 16-byte line: the elements ahead of the first aligned address are handled one by one"""
    for dtype, off in ((F16, 3), (F32, 1)):
        numel = 45
        x = _values(numel, 30.0, dtype, 99)
        buf = np.concatenate([np.full(off, 7.0, dtype=dtype), x, np.full(GUARD, 7.0, dtype=dtype)])
        bt = be.t(buf)
        be.ext.softcap_(bt[off:off + numel], 30.0)
        got = be.n(bt)
        assert np.all(got[:off] == 7.0) and np.all(got[off + numel:] == 7.0)
        want = GO.softcap(x, 30.0)
        if dtype == F32:
            assert np.all(np.abs(got[off:off + numel].astype(F64) - want) <= 2.0 ** -20 * np.abs(want) + 1e-38)
        else:
            assert np.all(_adjacent16(got[off:off + numel], want.astype(F16)))


def test_softcap_wrong_dtype(be):
    """ext_element.cpp:28-50: float or half, anything else is refused"""
    x = torch.zeros((8,), dtype=torch.bfloat16, device=be.device)
    with pytest.raises(RuntimeError, match="wrong dtype"):
        be.ext.softcap_(x, 30.0)
