"""The NORM form of the one-launch FP16 decode attention (csrc/attn_fused_body.h: q / k head norm folded in ahead of the rotation)
against the two launches it replaces: head_norm_qk on (q, k_new), then attn_decode_fused.

Both normalise with the one device function of csrc/head_norm.h, so everything must agree bit for bit: the attention output, the
rows appended to the cache; q and k_new stay as they were (un-normalised, un-rotated), the split tickets end at zero.
The two-launch side is pinned against the oracle by tests/test_head_norm.py (the norm) and tests/test_ops.py (the attention).
"""
import numpy as np
import pytest
import torch

from oracle import modules as OM
from tests.qk_norm_oracle import head_norm as oracle_head_norm

F16 = np.float16


def _u16(a):
    return np.ascontiguousarray(a).view(np.uint16)


@pytest.mark.parametrize("rms", [True, False], ids=["rms", "layernorm"])
@pytest.mark.parametrize("paged", [True, False], ids=["paged", "contiguous"])
@pytest.mark.parametrize("s", [1, 2])
@pytest.mark.parametrize("nh,kvh", [(4, 2), (8, 1)])
@pytest.mark.parametrize("hd", [64, 128, 256])
def test_norm_launch_equals_head_norm_then_attention(be, hd, nh, kvh, s, paged, rms):
    rng = np.random.default_rng(hd + 10 * nh + s)
    ps, b = 256, 3
    past = np.array([700, 3, 255], dtype=np.int32)
    pages_per_seq = 4
    T = ps * pages_per_seq
    table = rng.permutation(b * pages_per_seq).astype(np.int32).reshape(b, pages_per_seq)
    shape = (b * pages_per_seq, ps) if paged else (b, T)
    kc = (rng.standard_normal(shape + (kvh, hd)) * 0.5).astype(F16); vc = rng.standard_normal(shape + (kvh, hd)).astype(F16)
    q = (rng.standard_normal((b, s, nh, hd)) * 2.0).astype(F16)
    kn = (rng.standard_normal((b, s, kvh, hd)) * 0.3 + 0.1).astype(F16); vn = rng.standard_normal((b, s, kvh, hd)).astype(F16)
    qn = (1 + 0.1 * rng.standard_normal((nh, hd))).astype(F16); knw = (1 + 0.1 * rng.standard_normal((kvh, hd))).astype(F16)
    sin, cos = OM.rope_tables(2048, hd, neox=True)
    sint, cost = be.t(sin), be.t(cos)
    scratch = torch.zeros((be.ext.paged_attn_scratch_bytes(b * s * nh, hd, 16) // 4 + 1,), dtype=torch.float32, device=be.device)
    counters = torch.zeros((256,), dtype=torch.int32, device=be.device)
    sl, bt = be.t(past), (be.t(table) if paged else None)
    qnt, knt = be.t(qn), be.t(knw)
    invperm = be.t(rng.permutation(nh * hd).astype(np.uint16).view(np.int16))
    eps = 1e-6
    for nsplit in (1, 4):
        for inv in (None, invperm.data_ptr()):
            # two launches
            q2, k2 = be.t(q), be.t(kn)
            kc2, vc2 = be.t(kc), be.t(vc)
            be.ext.head_norm_qk(q2, k2, qnt, knt, eps, rms)
            out2 = torch.zeros((b, s, nh, hd), dtype=torch.float16, device=be.device)
            assert be.ext.attn_decode_fused(q2, k2, be.t(vn), kc2, vc2, out2, sint, cost, sl, bt, 0, 2, scratch, counters,
                                            nsplit=nsplit, out_invperm=inv)
            # one launch
            q1, k1 = be.t(q), be.t(kn)
            kc1, vc1 = be.t(kc), be.t(vc)
            out1 = torch.zeros((b, s, nh, hd), dtype=torch.float16, device=be.device)
            assert be.ext.attn_decode_fused(q1, k1, be.t(vn), kc1, vc1, out1, sint, cost, sl, bt, 0, 2, scratch, counters,
                                            nsplit=nsplit, out_invperm=inv, head_norm=(qnt, knt, eps, rms))
            what = (nsplit, inv is not None)
            assert np.array_equal(_u16(be.n(q1)), _u16(q)) and np.array_equal(_u16(be.n(k1)), _u16(kn)), what
            assert np.array_equal(_u16(be.n(out1)), _u16(be.n(out2))), what
            assert np.array_equal(_u16(be.n(kc1)), _u16(be.n(kc2))) and np.array_equal(_u16(be.n(vc1)), _u16(be.n(vc2))), what
            assert int(be.n(counters).astype(np.int64).sum()) == 0
    # the appended rows are the normalised, rotated new keys (and the norm is not a no-op)
    k_norm = oracle_head_norm(kn, knw, None, eps, rms)[1]
    k_rot = OM.rope_(k_norm, sin, cos, past, neox=True)
    got = be.n(kc1)
    for i in range(b):
        for j in range(s):
            pos = int(past[i]) + j
            row = got[table[i, pos // ps], pos % ps] if paged else got[i, pos]
            # (a sanity bound, not the parity check: the fp32 norm may round one fp16 ulp away from the float64 oracle, the rotation
            # combines two such values of magnitude <= |result| + 1 with factors <= 1 -- four ulps of that magnitude)
            assert np.all(np.abs(row.astype(np.float64) - k_rot[i, j].astype(np.float64)) <= 4 * 2.0 ** -10 * (np.abs(k_rot[i, j]).astype(np.float64) + 1.0))
    assert not np.array_equal(_u16(k_norm), _u16(kn))


def test_norm_launch_wants_both_weights(be):
    hd, nh, kvh = 64, 4, 2
    z = lambda *shape: torch.zeros(shape, dtype=torch.float16, device=be.device)
    counters = torch.zeros((64,), dtype=torch.int32, device=be.device)
    sin, cos = OM.rope_tables(512, hd, neox=True)
    with pytest.raises(RuntimeError, match="weight shapes"):
        be.ext.attn_decode_fused(z(1, 1, nh, hd), z(1, 1, kvh, hd), z(1, 1, kvh, hd), z(1, 256, kvh, hd), z(1, 256, kvh, hd), z(1, 1, nh, hd),
                                 be.t(sin), be.t(cos), None, None, 3, 2, None, counters, head_norm=(z(nh, hd), z(nh, hd), 1e-6, True))
