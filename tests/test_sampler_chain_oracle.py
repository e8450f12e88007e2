"""tests/sampler_chain_oracle.py against the executed reference (CPU).

The fixture tests/golden/reference_sampler_chain.npz holds what the reference's own stage functions gave for
tests/golden/make_golden_sampler_chain.py's cases; the numpy restatement must reproduce it bit for bit -- tokens, probability
bits, candidate counts, mirostat's mu bits, the top tokens and their probability bits -- and, where oracle/_ref is built, the
live library on a seeded sweep of settings.  The last test is the condition under which tests/test_sampler_chain_op.py may
skip undecided rows without hiding a failure."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import make_golden_sampler_chain as gold        # noqa: E402
import sampler_chain_oracle as chain            # noqa: E402

MARGIN = 2e-5                                    # tests/test_sampling.py's


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def oracle_results():
    """the oracle on every fixture case, computed once"""
    return [chain.sample_chain(np.asarray(lg, dtype=np.float32), st[0], st[1], st[2], st[3], rnd, c, mu)
            for lg, st, c, mu, rnd in gold.cases()]


def test_oracle_reproduces_the_executed_reference_fixture(oracle_results):
    z = np.load(gold.OUT)
    cases = gold.cases()
    assert len(cases) == z["tokens"].shape[0] >= 38
    both_quirks = fillers = few = 0
    for i, ((lg, st, c, mu, rnd), r) in enumerate(zip(cases, oracle_results)):
        R, K = lg.shape[0], c["num_probs"]
        assert np.array_equal(r["tokens"], z["tokens"][i, :R]), (i, c)
        assert np.array_equal(bits(r["probs"]), bits(z["probs"][i, :R])), (i, c)
        assert np.array_equal(r["counts"], z["num_candidates"][i, :R]), (i, c)
        assert np.array_equal(bits(r["mu"]), bits(z["mu"][i, :R])), (i, c)
        assert np.array_equal(r["ktokens"], z["ktokens"][i, :R, :K]), (i, c)
        assert np.array_equal(bits(r["kprobs"]), bits(z["kprobs"][i, :R, :K])), (i, c)
        both_quirks += int((r["counts"] == st[1] + 2).sum())
        fillers += int(K > 0 and (r["kprobs"] == 0).any())
        few += int(0 < c["tfs"] < 1 and (r["counts"] < 3).any())
    # the fixture reaches: top-a AND min-p each handing back n + 1, filler ids in the report, tfs below 3 candidates
    assert both_quirks >= 1 and fillers >= 2 and few >= 1


def test_oracle_reproduces_the_live_reference():
    if not os.path.exists(gold.LIB):
        pytest.skip("oracle/_ref/libsampling_ref.so not built (needs the reference's sources at build time)")
    fns = gold.load()
    rng = np.random.default_rng(41)
    for trial in range(24):
        v = int(rng.integers(40, 500))
        rows = int(rng.integers(1, 4))
        lg = (rng.standard_normal((rows, v)) * rng.uniform(0.5, 5)).astype(np.float32)
        st = (float(rng.uniform(0.3, 1.6)), int(rng.integers(1, min(v - 1, 200))), float(rng.choice([0.0, 0.4, 0.9])),
              float(rng.choice([0.0, 0.02, 0.2])))
        c = dict(gold.NEUTRAL)
        pick = lambda p: rng.random() < p
        if pick(0.3): c["top_a"] = float(rng.choice([0.0001, 0.1, 0.5]))
        if pick(0.3): c["tfs"] = float(rng.uniform(0.3, 0.99))
        if pick(0.3): c["typical"] = float(rng.uniform(0.1, 0.95))
        if pick(0.3): c.update(mirostat=True, mirostat_tau=float(rng.uniform(1, 5)), mirostat_eta=float(rng.uniform(0.05, 0.5)))
        if pick(0.3): c["post_temperature"] = float(rng.uniform(0.5, 2.0))
        if pick(0.2): c.update(min_temp=0.3, max_temp=float(rng.uniform(0.8, 2.0)), temp_exponent=float(rng.uniform(0.5, 2)))
        if pick(0.3): c["smoothing_factor"] = float(rng.uniform(0.3, 2.0))
        if pick(0.3): c["skew"] = float(rng.uniform(-1, 1))
        if pick(0.3): c["num_probs"] = int(rng.integers(1, 33))
        mu = [float(rng.choice([0.0, 3.0])) for _ in range(rows)] if c["mirostat"] else None
        rnd = float(rng.random())
        t, p, nc, m, kt, kp = gold.run_reference(fns, lg, st, c, mu, rnd)
        r = chain.sample_chain(lg, st[0], st[1], st[2], st[3], rnd, c, mu)
        assert np.array_equal(t, r["tokens"]) and np.array_equal(bits(p), bits(r["probs"])) and np.array_equal(nc, r["counts"]), (trial, st, c)
        assert np.array_equal(bits(m), bits(r["mu"])), (trial, st, c)
        assert np.array_equal(kt, r["ktokens"]) and np.array_equal(bits(kp), bits(r["kprobs"])), (trial, st, c)


def test_undecided_rows_are_at_most_a_fifth_of_the_fixture(oracle_results):
    total = sum(len(r["tokens"]) for r in oracle_results)
    undecided = sum(int(((r["margin"] < MARGIN) | r["tie"]).sum()) for r in oracle_results)
    assert undecided <= total / 5, (undecided, total)
