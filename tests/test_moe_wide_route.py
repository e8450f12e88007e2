"""Router for wide expert counts (64 / 128 experts, Qwen3-MoE: 128 experts, top 8; csrc/moe.hip: moe_wide_logits_kernel +
moe_wide_select_kernel) against oracle.modules.moe_route.  Reference arithmetic: cuda/q_mlp_softmax.cuh:272- (softmax128_topk_norm_kernel);
the reference then leaves the device (q_mlp.cu:403-435), this router does not."""
import numpy as np
import pytest
import torch

from oracle import modules as OM

F16 = np.float16


@pytest.mark.parametrize("experts,topk", [(128, 8), (64, 4)])
def test_moe_wide_route(be, experts, topk):
    """test_moe_route's inputs at 128 / 64 experts.  The smallest gap between the k-th and the (k + 1)-th logit of these rows is 2.4 / 3.6
    times the 4-ulp rule tests/test_moe.py leaves rows out by: every row is compared."""
    rng = np.random.default_rng(30)
    rows, hidden = 5, 128
    x = rng.standard_normal((rows, hidden)).astype(F16)
    gate = (rng.standard_normal((experts, hidden)) * 0.2).astype(F16)
    logits = torch.zeros((rows, experts), dtype=torch.float16, device=be.device)
    be.ext.moe_route(be.t(x), be.t(gate), logits, topk)
    raw = (x.astype(np.float32) @ gate.astype(np.float32).T).astype(F16)
    srt = np.sort(raw.astype(np.float32), axis=-1)[:, ::-1]
    assert np.all((srt[:, topk - 1] - srt[:, topk]) > 4 * np.maximum(np.abs(srt[:, topk - 1]), 1.0) * 2.0 ** -10)    # (no row is unclear)
    want, mask = OM.moe_route(raw, topk)
    got = be.n(logits)
    assert np.array_equal(got != 0, mask)                                    # same experts selected
    assert np.all(np.abs(got.astype(np.float32) - want.astype(np.float32)) <= 2e-3)
    assert np.allclose(got.astype(np.float32).sum(-1), 1.0, atol=2e-3)
    assert np.all((got != 0).sum(-1) == topk)                                # exact zeros outside the top-k


@pytest.mark.parametrize("experts,topk", [(128, 8), (64, 4)])
def test_moe_wide_route_tie_keeps_the_higher_index(be, experts, topk):
    """Two EQUAL logits at the boundary: the reference's drop loop scans ascending with a strict `<`, so the lower index is dropped
    first and the higher one survives.  One-hot rows pick router entries exactly: logits = topk - 1 large values, two equal ones,
    the rest small; the equal pair sits once inside one lane's two values (e, e + 64) and once across lanes."""
    hidden = 128
    for lo, hi in ((5, 5 + 64) if experts == 128 else (5, 40), (17, 30), (2, experts - 1)):
        col = np.full((experts,), -1.0, dtype=np.float32)
        big = [e for e in range(experts) if e not in (lo, hi)][3:3 + topk - 1]
        col[big] = 2.0 + 0.25 * np.arange(topk - 1)
        col[lo] = col[hi] = 1.0
        gate = np.zeros((experts, hidden), dtype=F16); gate[:, 7] = col.astype(F16)
        x = np.zeros((1, hidden), dtype=F16); x[0, 7] = 1.0
        logits = torch.zeros((1, experts), dtype=torch.float16, device=be.device)
        be.ext.moe_route(be.t(x), be.t(gate), logits, topk)
        got = be.n(logits)[0]
        assert sorted(np.nonzero(got)[0].tolist()) == sorted(big + [hi]), (lo, hi, np.nonzero(got)[0])
        assert got[lo] == 0 and got[hi] != 0
        # (oracle.modules.moe_route sorts stably and would keep `lo`: exact ties are the one place where it is not the reference)
        assert np.allclose(got.astype(np.float32).sum(), 1.0, atol=2e-3)
