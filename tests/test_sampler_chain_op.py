"""exl2_sample_rows_chain (csrc/sampling.hip, the CHAIN instantiations) against tests/sampler_chain_oracle.py, which
tests/test_sampler_chain_oracle.py pins to the executed reference bit for bit.

The kernel must give the oracle's token, candidate count, mu and top tokens on every row the oracle calls decided (no threshold
comparison closer than tests/test_sampling.py's 2e-5, no equal sort keys); at least four fifths of the fixture's rows are
compared.  On the emulation build the transcendentals are the host's libm; only the GPU run puts the device's against the margin."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import make_golden_sampler_chain as gold        # noqa: E402
import sampler_chain_oracle as chain            # noqa: E402

MARGIN = 2e-5
_oracle = {}


def oracle_on_fixture():
    """computed once, shared, never modified"""
    if not _oracle:
        _oracle["r"] = [chain.sample_chain(np.asarray(lg, dtype=np.float32), st[0], st[1], st[2], st[3], rnd, c, mu)
                        for lg, st, c, mu, rnd in gold.cases()]
    return _oracle["r"]


def p_close(got, want):
    return abs(float(got) - float(want)) <= 2e-5 * max(1.0, float(want)) + 1e-6


def run_kernel(be, lg, st, c, mu, rnd):
    torch = be.torch
    rows = lg.shape[0]
    K = int(c["num_probs"])
    out_t = torch.zeros(rows, dtype=torch.int32, device=be.device)
    out_p = torch.zeros(rows, dtype=torch.float32, device=be.device)
    kw = {k: v for k, v in c.items() if k != "num_probs"}
    mu_t = kt = kp = None
    cnt = torch.zeros(rows, dtype=torch.int32, device=be.device)
    kw["out_counts"] = cnt
    if c["mirostat"]:
        mu_t = be.t(np.asarray(mu, dtype=np.float32))
        kw["mirostat_mu"] = mu_t
    if K:
        kt = torch.zeros((rows, K), dtype=torch.int32, device=be.device)
        kp = torch.zeros((rows, K), dtype=torch.float32, device=be.device)
        kw.update(out_ktokens=kt, out_kprobs=kp)
    be.ext.sample_rows_chain(be.t(lg), st[0], st[1], st[2], st[3], rnd, out_t, out_p, **kw)
    return (be.n(out_t), be.n(out_p), None if mu_t is None else be.n(mu_t), None if kt is None else be.n(kt),
            None if kp is None else be.n(kp), be.n(cnt))


def test_chain_equals_oracle_on_the_fixture_cases(be):
    compared = total = 0
    for i, ((lg, st, c, mu, rnd), want) in enumerate(zip(gold.cases(), oracle_on_fixture())):
        tok, pr, mu_got, kt, kp, cnt = run_kernel(be, lg, st, c, mu, rnd)
        for r in range(lg.shape[0]):
            total += 1
            if want["margin"][r] < MARGIN or want["tie"][r]:
                continue
            compared += 1
            assert tok[r] == want["tokens"][r], (i, r, c, tok, want["tokens"], want["margin"])
            assert p_close(pr[r], want["probs"][r]), (i, r, c, pr, want["probs"])
            assert cnt[r] == want["counts"][r], (i, r, c, cnt, want["counts"])
            if c["mirostat"]:
                eta, m = float(c["mirostat_eta"]), float(want["mu"][r])
                assert abs(float(mu_got[r]) - m) <= eta * 4e-5 + 4 * float(np.spacing(np.float32(abs(m)))), (i, r, mu_got, want["mu"])
            if c["num_probs"]:
                assert np.array_equal(kt[r], want["ktokens"][r]), (i, r, c, kt[r], want["ktokens"][r])
                assert all(p_close(a, b) for a, b in zip(kp[r], want["kprobs"][r])), (i, r, kp[r], want["kprobs"][r])
    assert compared >= 0.8 * total, (compared, total)


@pytest.mark.parametrize("dtype", [np.float16, np.float32])
def test_neutral_chain_is_sample_rows_bit_for_bit(be, dtype):
    torch = be.torch
    rng = np.random.default_rng(7)
    for vocab, rows, st, rnd in ((96, 3, (0.8, 50, 0.8, 0.02), 0.37), (4096, 2, (1.0, 64, 0.0, 0.001), 0.81),
                                 (997, 1, (1.2, 9, 0.9, 0.0), 0.05), (300, 2, (1.0, 1, 0.0, 0.0), 0.5)):
        lg = be.t((rng.standard_normal((rows, vocab)) * 3).astype(dtype))
        outs = []
        for fn in (be.ext.sample_rows, be.ext.sample_rows_chain):
            t = torch.zeros(rows, dtype=torch.int32, device=be.device)
            p = torch.zeros(rows, dtype=torch.float32, device=be.device)
            ws = fn(lg, st[0], st[1], st[2], st[3], rnd, t, p)
            outs.append((be.n(t).copy(), be.n(p).view(np.uint32).copy(), be.n(ws).view(np.uint32).copy()))
        assert all(np.array_equal(a, b) for a, b in zip(*outs)), (vocab, rows, st)


def test_random_sweep_tfs_typical_skew(be):
    """One row, the random point swept over its range: a wrong order of the candidates after the sorts shows as wrong tokens."""
    rng = np.random.default_rng(13)
    lg = (rng.standard_normal((1, 200)) * 2).astype(np.float32)
    c = dict(gold.NEUTRAL, tfs=0.95, typical=0.8, skew=0.6)
    compared, seen = 0, set()
    for rnd in np.linspace(0.0, 0.99999, 33):
        want = chain.sample_chain(lg, 1.0, 40, 0.0, 0.0, float(rnd), c)
        tok, pr, _, _, _, _ = run_kernel(be, lg, (1.0, 40, 0.0, 0.0), c, None, float(rnd))
        if want["margin"][0] < MARGIN or want["tie"][0]:
            continue
        compared += 1
        seen.add(int(tok[0]))
        assert tok[0] == want["tokens"][0], (rnd, tok, want["tokens"], want["margin"])
        assert p_close(pr[0], want["probs"][0])
    assert compared >= 26 and len(seen) >= 4


def test_per_row_random_divides_the_temperature_once(be):
    """the step form with per-row points: every row is a batch-1 call of the reference (no recurrence, no compounding division)"""
    torch = be.torch
    rng = np.random.default_rng(3)
    lg = (rng.standard_normal((3, 128)) * 2).astype(np.float32)
    pts = [0.21, 0.64, 0.93]
    c = dict(gold.NEUTRAL, smoothing_factor=0.6)
    want = chain.sample_chain(lg, 1.0, 30, 0.0, 0.0, 0.0, c, per_row_random=pts)
    t = torch.zeros(3, dtype=torch.int32, device=be.device); p = torch.zeros(3, dtype=torch.float32, device=be.device)
    ws = torch.empty((3, 128), dtype=torch.float32, device=be.device)
    be.ext.sample_rows_chain_step(be.t(lg), 1.0, 30, 0.0, 0.0, be.t(np.asarray(pts, dtype=np.float32)),
                                  torch.zeros(1, dtype=torch.int32, device=be.device), t, p, ws, None, None, pos_inc=0,
                                  per_row_random=True, smoothing_factor=0.6)
    got = be.n(t)
    decided = [r for r in range(3) if want["margin"][r] >= MARGIN]
    assert len(decided) >= 2
    for r in decided:
        assert got[r] == want["tokens"][r], (r, got, want["tokens"])


def test_refused_settings_raise_with_the_reason(be):
    torch = be.torch
    lg = be.t(np.zeros((1, 64), dtype=np.float32))
    t, p = torch.zeros(1, dtype=torch.int32, device=be.device), torch.zeros(1, dtype=torch.float32, device=be.device)
    kt, kp = torch.zeros((1, 4), dtype=torch.int32, device=be.device), torch.zeros((1, 4), dtype=torch.float32, device=be.device)
    kt33, kp33 = torch.zeros((1, 33), dtype=torch.int32, device=be.device), torch.zeros((1, 33), dtype=torch.float32, device=be.device)
    call = lambda k=10, **kw: be.ext.sample_rows_chain(lg, 1.0, k, 0.0, 0.0, 0.5, t, p, **kw)
    with pytest.raises(RuntimeError, match="stale buffer"):
        call(xtc_probability=0.3)
    with pytest.raises(RuntimeError, match="partial order"):
        call(typical=0.5, out_ktokens=kt, out_kprobs=kp)
    for k in (0, 501, 64):
        with pytest.raises(RuntimeError):
            call(k)
    for bad in ({"out_ktokens": kt33, "out_kprobs": kp33}, {"tfs": -0.1}, {"tfs": 1.5}, {"typical": -0.1}, {"typical": 1.2},
                {"top_a": -0.5}, {"smoothing_factor": -1.0}, {"mirostat": True, "mirostat_tau": 1.0, "mirostat_eta": 0.1}):
        with pytest.raises(RuntimeError):
            call(**bad)
    with pytest.raises(TypeError):
        call(no_such_setting=1.0)
    call(typical=0.5)                                                # (each half of the refused combination alone is served)
    call(out_ktokens=kt, out_kprobs=kp)
