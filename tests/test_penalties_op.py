"""exl2_apply_penalties (csrc/penalties.hip) against the executed reference: apply_rep_penalty_cpu (cpp/sampling.cpp:20-110) followed
by the token-bias add (sampler.py:427-429).  Every comparison is bit for bit (`view(np.uint32)`): the fixture
tests/golden/reference_penalties.npz and the `rep_penalty_logits` of reference_sampling.npz were written by running the reference;
the drop-in's host `apply_rep_penalty`, which tests/test_sampling.py pins to the same reference, serves the shapes the fixture does
not hold."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "dropin"))
import make_golden_penalties as gpen         # noqa: E402
import make_golden_sampling as gold          # noqa: E402

_shared = {}


def fixture():
    """(cases, npz), loaded once and never changed"""
    if "fx" not in _shared:
        _shared["fx"] = (gpen.cases(), np.load(os.path.join(ROOT, "tests", "golden", "reference_penalties.npz")))
    return _shared["fx"]


def dropin():
    import exllamav2_ext
    return exllamav2_ext


def host_walk(seq, lg, st):
    """the drop-in's host route (pinned to the reference by tests/test_sampling.py): seq int [rows, L], lg fp32 [rows, vocab]"""
    want = torch.from_numpy(np.ascontiguousarray(lg, dtype=np.float32).copy()).view(lg.shape[0], 1, -1)
    dropin().apply_rep_penalty(torch.from_numpy(np.ascontiguousarray(seq, dtype=np.int64)), st[0], st[1], st[2], st[3], st[4], want)
    return want.view(lg.shape[0], -1).numpy()


def run_kernel(be, lg, seqs, st, dtype=np.float32, ld=None, bias=None, garbage=7, share=False, tail=None, out_fill=0.0):
    """lg [rows, vocab]; seqs: one sequence per row (lists of different lengths are fine).  Returns (out [rows, vocab], the device
    logits after the launch)."""
    rows, vocab = lg.shape
    ld = ld or vocab
    padded = np.full((rows, ld), 50.0, dtype=dtype)
    padded[:, :vocab] = lg.astype(dtype)
    n_seq = 1 if share else rows
    stride = max(len(s) for s in seqs) + 3
    hist = np.full((n_seq, stride), garbage, dtype=np.int32)
    for r in range(n_seq):
        hist[r, :len(seqs[r])] = np.asarray(seqs[r], dtype=np.int64).astype(np.int32)
    pos = np.array([len(seqs[r]) - 1 for r in range(n_seq)], dtype=np.int32)
    out = torch.full((rows, vocab), out_fill, dtype=torch.float32, device=be.device)
    dl = be.t(padded)
    be.ext.apply_penalties(dl, out, be.t(hist), be.t(pos), st[0], st[1], st[2], st[3], st[4],
                           token_bias=None if bias is None else be.t(bias.astype(np.float32)), vocab=vocab,
                           rows_share_sequence=share, tail=None if tail is None else be.t(np.asarray(tail, dtype=np.int32)))
    return be.n(out), be.n(dl)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float32).view(np.uint32), np.ascontiguousarray(b, dtype=np.float32).view(np.uint32))


def test_fixture_covers_what_it_promises():
    cases, z = fixture()
    assert len(cases) == len([k for k in z.files if k.startswith("idx_")])
    assert {c[1] for c in cases} == {257, 2048}
    assert {len(c[2]) for c in cases if c[0].startswith("len")} == {1, 2, 63, 64, 65, 1023, 1025, 2500}
    assert {c[4] for c in cases} == set(gpen.SETTINGS) and len(gpen.SETTINGS) == 8
    assert any(c[5] for c in cases) and any(not c[5] for c in cases)
    # the empty window and the neutral settings change nothing; everything else changes something
    for i, c in enumerate(cases):
        assert (z[f"idx_{i}"].size == 0) == (c[4] in ((1.3, 0, 0, 0.2, 0.1), (1.0, -1, 0, 0.0, 0.0))), (i, c[0], c[4])


def test_fp32_logits_equal_the_fixture(be):
    cases, z = fixture()
    for i, (name, vocab, seq, lg, st, half) in enumerate(cases):
        got, _ = run_kernel(be, lg[None], [seq], st)
        assert same_bits(got[0], gpen.expected(z, i, lg)), (i, name, vocab, len(seq), st)


def test_fp16_logits_equal_the_fixture(be):
    cases, z = fixture()
    n = 0
    for i, (name, vocab, seq, lg, st, half) in enumerate(cases):
        if not half:
            continue
        got, _ = run_kernel(be, lg[None], [seq], st, dtype=np.float16)
        assert same_bits(got[0], gpen.expected(z, i, lg)), (i, name, vocab, len(seq), st)
        n += 1
    assert n >= 20


def test_rep_penalty_logits_of_the_sampling_fixture(be):
    z = np.load(os.path.join(ROOT, "tests", "golden", "reference_sampling.npz"))
    seq, lg = gold.rep_cases()
    for i, st in enumerate(gold.REP_SETTINGS):
        got, _ = run_kernel(be, lg, list(seq), st)
        assert same_bits(got, z["rep_penalty_logits"][i]), st


def test_three_rows_with_their_own_positions(be):
    cases, z = fixture()
    for vocab in (257, 2048):
        for st in gpen.SETTINGS:
            pick = [i for i, c in enumerate(cases) if c[1] == vocab and c[4] == st][:3]
            if len(pick) < 3:
                continue
            lg = np.stack([cases[i][3] for i in pick])
            got, _ = run_kernel(be, lg, [cases[i][2] for i in pick], st)
            for r, i in enumerate(pick):
                assert same_bits(got[r], gpen.expected(z, i, cases[i][3])), (vocab, st, r, cases[i][0])


@pytest.mark.parametrize("dtype", [np.float32, np.float16])
def test_row_stride_wider_than_the_vocabulary(be, dtype):
    cases, z = fixture()
    for vocab, ld in ((257, 260), (257, 263), (2048, 2112)):
        pick = [i for i, c in enumerate(cases) if c[1] == vocab and c[5] and z[f"idx_{i}"].size > 0][:2]
        lg = np.stack([cases[i][3] for i in pick])
        st = cases[pick[0]][4]
        if cases[pick[1]][4] != st:
            pick = pick[:1]; lg = lg[:1]
        got, after = run_kernel(be, lg, [cases[i][2] for i in pick], st, dtype=dtype, ld=ld)
        for r, i in enumerate(pick):
            assert same_bits(got[r], gpen.expected(z, i, cases[i][3])), (vocab, ld, r)
        # the input is read only: the logits and the padding behind them are what they were
        assert np.all(after[:, vocab:] == 50.0) and np.array_equal(after[:, :vocab], lg.astype(dtype))


def test_token_bias_after_the_penalties(be):
    cases, z = fixture()
    rng = np.random.default_rng(3)
    for vocab in (257, 2048):
        i = next(i for i, c in enumerate(cases) if c[1] == vocab and c[0] == "len1025" and z[f"idx_{i}"].size > 0)
        name, _, seq, lg, st, half = cases[i]
        bias = (rng.standard_normal(vocab) * 2).astype(np.float32)
        bias[rng.integers(0, vocab, size=9)] = -np.inf
        bias[int(seq[-1]) % vocab] = -np.inf                         # a penalised id among the banned ones
        bias[::7] = 0.0
        got, _ = run_kernel(be, lg[None], [seq], st, bias=bias)
        assert same_bits(got[0], gpen.expected(z, i, lg) + bias), (vocab, st)
        # bias alone, neutral penalties: float(logits) + bias
        got, _ = run_kernel(be, lg[None], [seq], (1.0, -1, 0, 0.0, 0.0), bias=bias, dtype=np.float16 if half else np.float32)
        assert same_bits(got[0], lg + bias)


def test_nothing_behind_the_position_is_read(be):
    cases, z = fixture()
    i = next(i for i, c in enumerate(cases) if c[1] == 2048 and c[0] == "len65" and z[f"idx_{i}"].size > 0)
    name, vocab, seq, lg, st, half = cases[i]
    a, _ = run_kernel(be, lg[None], [seq], st, garbage=7)
    b, _ = run_kernel(be, lg[None], [seq], st, garbage=int(seq[0]))
    c, _ = run_kernel(be, lg[None], [seq], st, garbage=-5, out_fill=np.nan)
    want = gpen.expected(z, i, lg)
    assert same_bits(a[0], want) and same_bits(b[0], want) and same_bits(c[0], want)


def random_settings(rng):
    return (float(rng.choice([1.0, 1.025, 1.1, 1.3, 0.9])), int(rng.choice([-1, 0, 1, 5, 100, 1024, 5000])),
            int(rng.choice([0, 0, 1, 7, 64, 700, 2000])), float(rng.choice([0.0, 0.0, 0.1, 0.013])), float(rng.choice([0.0, 0.05, 0.3])))


def test_random_sweep_against_the_host_walk(be):
    rng = np.random.default_rng(101)
    for trial in range(20):
        vocab = int(rng.integers(2, 4097)); L = int(rng.integers(1, 3001))
        st = random_settings(rng)
        distinct = int(rng.choice([vocab + 10, 300, 17]))            # all over the vocabulary, text-like, a handful of ids
        seq = rng.integers(0, distinct, size=(1, L))
        lg = (rng.standard_normal((1, vocab)) * 3).astype(np.float32)
        got, _ = run_kernel(be, lg, list(seq), st)
        assert same_bits(got, host_walk(seq, lg, st)), (trial, vocab, L, st, distinct)


@pytest.mark.parametrize("vocab", [32000, 151936])
def test_real_vocabularies_with_a_4096_token_window(be, vocab):
    rng = np.random.default_rng(vocab)
    L = 4096
    lg = (rng.standard_normal((2, vocab)) * 3).astype(np.float16)
    seq = np.stack([rng.integers(0, vocab, size=L), rng.integers(0, 400, size=L) * 37 % vocab])      # spread out / text-like
    for st in ((1.025, -1, 0, 0.0, 0.0), (1.2, 1024, 1024, 0.1, 0.1), (1.1, 0, 4200, 0.05, 0.0)):    # (the last: a decay range beyond the LDS stage)
        got, _ = run_kernel(be, lg.astype(np.float32), list(seq), st, dtype=np.float16, ld=vocab + 64)
        assert same_bits(got, host_walk(seq, lg.astype(np.float32), st)), (vocab, st)


def test_rows_that_share_a_sequence_append_the_tail(be):
    rng = np.random.default_rng(12)
    for vocab, L in ((257, 40), (2048, 1500)):
        base = rng.integers(0, min(vocab + 5, 300), size=L)
        tail = np.array([int(base[-1]), int(base[3]), vocab - 1, int(base[-1])])
        lg = (rng.standard_normal((5, vocab)) * 3).astype(np.float32)
        for st in ((1.025, -1, 0, 0.0, 0.0), (1.3, 8, 8, 0.3, 0.2), (1.15, 100, 700, 0.05, 0.02)):
            got, _ = run_kernel(be, lg, [base], st, share=True, tail=tail)
            for r in range(5):
                one, _ = run_kernel(be, lg[r:r + 1], [np.concatenate([base, tail[:r]])], st)
                assert same_bits(got[r], one[0]), (vocab, st, r)
                assert same_bits(one, host_walk(np.concatenate([base, tail[:r]])[None], lg[r:r + 1], st))


def test_refusals(be):
    t = be.torch
    lg = be.t(np.zeros((1, 64), dtype=np.float32))
    out = t.zeros((1, 64), dtype=t.float32, device=be.device)
    hist = be.t(np.zeros((1, 16), dtype=np.int32)); pos = be.t(np.array([3], dtype=np.int32))
    lib = be.ext.lib
    ptr = lambda x: x.data_ptr()
    def call(logits=lg, o=out, h=hist, p=pos, vocab=64, ld=64, sustain=-1, decay=0, ramps=None):
        return lib.exl2_apply_penalties(ptr(logits), 1, 1, vocab, ld, None if o is None else ptr(o), None if h is None else ptr(h), 16,
                                        None if p is None else ptr(p), 0, 0, None, 1.1, sustain, decay, 0.0, 0.0,
                                        None if ramps is None else ptr(ramps), None, None)
    assert call() == 0
    ramps = be.t(np.ones((3, 4), dtype=np.float32))
    for kw in (dict(o=None), dict(h=None), dict(p=None), dict(decay=-1, ramps=ramps), dict(sustain=-2), dict(decay=4), dict(vocab=64, ld=60)):
        assert call(**kw) < 0, kw
        assert "apply_penalties" in lib.last_error()
    assert call(decay=4, ramps=ramps) == 0
    with pytest.raises(RuntimeError, match="out, history and hist_pos"):
        be.ext.apply_penalties(lg, None, hist, pos, 1.1)
    with pytest.raises(RuntimeError, match="tail"):
        be.ext.apply_penalties(be.t(np.zeros((3, 64), dtype=np.float32)), t.zeros((3, 64), dtype=t.float32, device=be.device), hist, pos, 1.1,
                               rows_share_sequence=True)


def test_ramp_table_is_the_sequential_fp32_sum():
    from exllamav2_amd.ext import ExtC
    f32 = np.float32
    r = ExtC.penalty_ramps(1.15, 700, 0.05, 0.02).numpy()
    assert r.shape == (3, 700) and r.dtype == np.float32
    for c, (start, target) in enumerate(((1.15, 1.0), (0.05, 0.0), (0.02, 0.0))):
        v, d = f32(start), (f32(target) - f32(start)) / f32(700)
        for k in range(700):
            assert r[c, k] == v
            v = f32(v + d)
    assert ExtC.penalty_ramps(1.2, 0, 0.1, 0.1) is None


def test_dropin_takes_the_kernel_for_device_logits(be):
    if be.is_emu:
        pytest.skip("the drop-in binds the HIP library: its device route needs the device")
    rng = np.random.default_rng(8)
    seq = rng.integers(0, 4100, size=(2, 500))
    lg = (rng.standard_normal((2, 4096)) * 3).astype(np.float32)
    for st in ((1.025, -1, 0, 0.0, 0.0), (1.2, 100, 300, 0.1, 0.05)):
        dev = be.t(lg).view(2, 1, -1)
        dropin().apply_rep_penalty(torch.from_numpy(seq), st[0], st[1], st[2], st[3], st[4], dev)
        assert same_bits(be.n(dev).reshape(2, -1), host_walk(seq, lg, st)), st


def test_kernel_equals_the_live_reference(be):
    if not os.path.exists(gold.LIB):
        pytest.skip("oracle/_ref/libsampling_ref.so not built (needs the reference tree at build time)")
    lib = gold.load()
    rng = np.random.default_rng(77)
    for trial in range(10):
        vocab = int(rng.integers(3, 3000)); L = int(rng.integers(1, 2000))
        st = random_settings(rng)
        seq = rng.integers(0, int(rng.choice([vocab + 10, 50])), size=(1, L)).astype(np.int64)
        lg = (rng.standard_normal((1, vocab)) * 3).astype(np.float32)
        want = gold.run_reference_rep_penalty(lib, seq, lg, st)
        got, _ = run_kernel(be, lg, list(seq), st)
        assert same_bits(got, want), (trial, vocab, L, st)
