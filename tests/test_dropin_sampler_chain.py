"""ext_c.sample_basic through the drop-in with the rest of the sampler chain, called with the reference's argument list
(sampler.py:540-568: fp32 logits [bsz, 1, vocab] on the host, int64 / fp32 outputs on the host, `none_tensor` on the meta device
for the unused ones), against tests/golden/reference_sampler_chain.npz -- what the reference's own stage functions gave -- on the
rows tests/sampler_chain_oracle.py calls decided."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import make_golden_sampler_chain as gold        # noqa: E402
import sampler_chain_oracle as chain            # noqa: E402

MARGIN = 2e-5


def _dropin():
    sys.path.insert(0, os.path.join(ROOT, "dropin"))
    try:
        import exllamav2_ext as dropin
    except (OSError, RuntimeError) as e:                      # the drop-in binds libexl2_hip.so at import
        pytest.skip(f"drop-in not importable here: {e}")
    return dropin


def p_close(got, want):
    return abs(float(got) - float(want)) <= 2e-5 * max(1.0, float(want)) + 1e-6


def call(dropin, lg, st, c, mu, rnd, xtc=0.0):
    """sample_basic as ExLlamaV2Sampler.sample calls it"""
    rows, K = lg.shape[0], int(c["num_probs"])
    none = torch.empty((1, 1), device="meta")
    logits = torch.from_numpy(np.ascontiguousarray(lg, dtype=np.float32)).view(rows, 1, -1)
    out_t = torch.empty((rows, 1), dtype=torch.long)
    out_p = torch.empty((rows, 1), dtype=torch.float)
    kt = torch.empty((rows, 1, K), dtype=torch.long) if K else none
    kp = torch.empty((rows, 1, K), dtype=torch.float) if K else none
    m = dropin.sample_basic(logits, st[0], st[1], st[2], c["top_a"], st[3], c["tfs"], c["typical"], rnd, out_t, out_p, kp, kt, none,
                            c["mirostat"], list(mu) if c["mirostat"] else [], c["mirostat_tau"], c["mirostat_eta"],
                            c["post_temperature"], none, xtc, 0.1, c["min_temp"], c["max_temp"], c["temp_exponent"],
                            c["smoothing_factor"], c["skew"])
    return out_t[:, 0].numpy(), out_p[:, 0].numpy(), m, (kt[:, 0].numpy() if K else None), (kp[:, 0].numpy() if K else None)


def fixture_case(pred):
    z = np.load(gold.OUT)
    for i, case in enumerate(gold.cases()):
        if pred(case[2], case[3]):
            return i, case, z
    raise AssertionError("no such fixture case")


@pytest.mark.gpu
def test_mirostat_settings_across_three_calls_with_mu_carried_by_the_returned_list():
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    dropin = _dropin()
    i, (lg, st, c, mu, rnd), z = fixture_case(lambda c, mu: c["mirostat"] and mu == [0.0, 0.0] and not c["num_probs"] and c["top_a"] == 0)
    rows = lg.shape[0]
    compared = 0
    for step in range(3):
        r = rnd if step == 0 else (rnd + 0.31 * step) % 1.0
        want = chain.sample_chain(lg, st[0], st[1], st[2], st[3], r, c, mu)
        tok, pr, m, _, _ = call(dropin, lg, st, c, mu, r)
        assert isinstance(m, list) and len(m) == rows
        for b in range(rows):
            if want["margin"][b] < MARGIN or want["tie"][b]:
                continue
            compared += 1
            assert tok[b] == want["tokens"][b] and p_close(pr[b], want["probs"][b]), (step, b, tok, want["tokens"])
            w = float(want["mu"][b])
            assert abs(m[b] - w) <= c["mirostat_eta"] * 4e-5 + 4 * float(np.spacing(np.float32(abs(w)))), (step, b, m, want["mu"])
            if step == 0:                                                   # the first call is the fixture's own
                assert tok[b] == z["tokens"][i, b] and p_close(m[b], z["mu"][i, b])
        mu = [float(x) for x in want["mu"]]                                 # carried over (the oracle's: the decided rows' equal it)
    assert compared >= 4


@pytest.mark.gpu
def test_return_top_tokens_and_temperature_last():
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    dropin = _dropin()
    compared, seen = 0, set()
    z = np.load(gold.OUT)
    for i, (lg, st, c, mu, rnd) in enumerate(gold.cases()):
        # every fixture case with the report or a post-softmax temperature (mirostat: the test above; typical + report: refused;
        # greedy settings take the drop-in's arg-max branch, which this feature leaves as it is; tfs: the binding still refuses it,
        # tests/test_sampling.py pins that)
        if st[0] < 0.01 or st[1] == 1 or 0 < c["tfs"] < 1 or c["mirostat"] or not (c["num_probs"] or c["post_temperature"] != 1.0) or (c["num_probs"] and 0 < c["typical"] < 1):
            continue
        want = chain.sample_chain(lg, st[0], st[1], st[2], st[3], rnd, c, mu)
        tok, pr, m, kt, kp = call(dropin, lg, st, c, mu, rnd)
        assert m == []
        K = c["num_probs"]
        for b in range(lg.shape[0]):
            if want["margin"][b] < MARGIN or want["tie"][b]:
                continue
            compared += 1
            seen.add((K, c["post_temperature"] != 1.0))
            assert tok[b] == z["tokens"][i, b] and p_close(pr[b], z["probs"][i, b]), (i, b, tok, z["tokens"][i])
            if K:
                assert kt.dtype == np.int64 and np.array_equal(kt[b], z["ktokens"][i, b, :K]), (kt[b], z["ktokens"][i, b, :K])
                assert all(p_close(a, w) for a, w in zip(kp[b], z["kprobs"][i, b, :K]))
    assert compared >= 8 and (5, False) in seen and any(t for _, t in seen), (compared, seen)


@pytest.mark.gpu
def test_refused_settings_keep_raising():
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    dropin = _dropin()
    lg = np.random.default_rng(1).standard_normal((1, 128)).astype(np.float32)
    with pytest.raises(NotImplementedError, match="XTC"):
        call(dropin, lg, (0.8, 50, 0.8, 0.0), dict(gold.NEUTRAL), None, 0.5, xtc=0.5)
    with pytest.raises(NotImplementedError, match="typical"):
        call(dropin, lg, (0.8, 50, 0.8, 0.0), dict(gold.NEUTRAL, typical=0.5, num_probs=3), None, 0.5)
    with pytest.raises(NotImplementedError, match="tfs"):
        call(dropin, lg, (0.8, 50, 0.8, 0.0), dict(gold.NEUTRAL, tfs=0.5), None, 0.5)
    with pytest.raises(NotImplementedError, match="top_k"):
        call(dropin, lg, (0.8, 0, 0.8, 0.0), dict(gold.NEUTRAL), None, 0.5)
