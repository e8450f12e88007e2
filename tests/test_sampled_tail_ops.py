"""The two additions the sampled speculative step needs: exl2_sample_rows_step2's per-row random points (csrc/sampling.hip) and
exl2_spec_accept_draft2's random counter (csrc/spec_decode.hip).  Both are compared with launches of the entries that existed
before, bit for bit; the older modes must be what they were."""
import numpy as np
import pytest

SETTINGS = [(0.8, 50, 0.8, 0.0), (1.0, 40, 0.0, 0.05), (1.3, 7, 0.9, 0.0)]


def one_row(be, lg, st, rnd):
    t = be.torch
    tok = t.zeros(1, dtype=t.int32, device=be.device); pr = t.zeros(1, dtype=t.float32, device=be.device)
    be.ext.sample_rows(be.t(lg), st[0], st[1], st[2], st[3], float(rnd), tok, pr)
    return int(be.n(tok)[0]), be.n(pr).view(np.uint32)[0]


def step(be, lg, st, randoms, c, per_row, log=True):
    t = be.torch
    rows, vocab = lg.shape
    tok = t.full((rows,), -1, dtype=t.int32, device=be.device); pr = t.zeros(rows, dtype=t.float32, device=be.device)
    ws = t.empty((rows, vocab), dtype=t.float32, device=be.device)
    hist = t.full((rows, 8), -3, dtype=t.int32, device=be.device) if log else None
    pos = t.full((rows,), 2, dtype=t.int32, device=be.device) if log else None
    counter = be.t(np.array([c], dtype=np.int32))
    be.ext.sample_rows_step(be.t(lg), st[0], st[1], st[2], st[3], be.t(randoms), counter, tok, pr, ws, hist, pos,
                            pos_inc=1 if log else 0, per_row_random=per_row)
    assert int(be.n(counter)[0]) == c                                # the sampler never advances the counter
    if log:
        assert np.array_equal(be.n(hist)[:, 3], be.n(tok)) and np.all(be.n(pos) == 3)
    return be.n(tok), be.n(pr).view(np.uint32)


@pytest.mark.parametrize("dtype", [np.float32, np.float16])
def test_per_row_random_points(be, dtype):
    rng = np.random.default_rng(41)
    n = 6
    randoms = rng.random(n).astype(np.float32)
    for vocab in (300, 2048):
        lg = (rng.standard_normal((4, vocab)) * 3).astype(np.float16).astype(dtype)
        for st in SETTINGS:
            for c in (0, 1, 4, 5, 17):                                # 4, 5, 17: the index wraps inside the four rows
                tok, pr = step(be, lg, st, randoms, c, True, log=c != 1)
                for r in range(4):
                    want = one_row(be, lg[r:r + 1], st, randoms[(c + r) % n])
                    assert (int(tok[r]), pr[r]) == want, (vocab, st, c, r)
    # rows of identical logits draw different tokens: the points really differ per row
    same = np.repeat((rng.standard_normal((1, 300)) * 0.5).astype(dtype), 4, axis=0)
    tok, _ = step(be, same, (1.0, 200, 0.0, 0.0), np.array([0.05, 0.35, 0.65, 0.95], dtype=np.float32), 0, True)
    assert len(set(tok.tolist())) == 4


def test_recurrence_mode_is_unchanged(be):
    """the mode every caller used so far: all rows share randoms[counter % n] through the reference's recurrence -- the same tokens
    and probabilities as sample_rows with that point as its scalar argument"""
    t = be.torch
    rng = np.random.default_rng(42)
    randoms = rng.random(5).astype(np.float32)
    lg = (rng.standard_normal((4, 1000)) * 3).astype(np.float16)
    for st in SETTINGS:
        for c in (0, 3, 7):
            tok, pr = step(be, lg, st, randoms, c, False)
            wt = t.zeros(4, dtype=t.int32, device=be.device); wp = t.zeros(4, dtype=t.float32, device=be.device)
            be.ext.sample_rows(be.t(lg), st[0], st[1], st[2], st[3], float(randoms[c % 5]), wt, wp)
            assert np.array_equal(tok, be.n(wt)) and np.array_equal(pr, be.n(wp).view(np.uint32)), (st, c)


def accept(be, K, n_acc, counter0, draft_only=False):
    """one accept launch with and one without the counter on the same inputs: (state without, state with, counter after)"""
    rng = np.random.default_rng(7 * K + n_acc)
    seq = rng.integers(0, 4, size=12).astype(np.int32)
    cand = rng.integers(10, 20, size=K + 1).astype(np.int32)
    drafts = cand[:K].copy()
    if n_acc < K:
        drafts[n_acc] += 1
    out = []
    for with_counter in (False, True):
        hist = np.full((12 + K + 4,), -5, dtype=np.int32); hist[:12] = seq
        ids = np.concatenate([seq[-1:], drafts]).astype(np.int32)
        th, ti, tp = be.t(hist), be.t(ids), be.t(np.array([11], dtype=np.int32))
        ts = be.t(np.zeros(K + 3, dtype=np.int32))
        tc = be.t(np.array([counter0, -9], dtype=np.int32))
        be.ext.spec_accept_draft(None if draft_only else be.t(cand), ti, th, tp, None if draft_only else ts, K, 3, draft_only=draft_only,
                                 rand_counter=tc[:1] if with_counter else None)
        out.append((be.n(th).tolist(), be.n(ti).tolist(), be.n(tp).tolist(), be.n(ts).tolist(), be.n(tc).tolist()))
    return out


@pytest.mark.parametrize("K", [3, 7])
def test_accept_advances_the_random_counter(be, K):
    for n_acc in (0, K // 2, K):
        plain, counted = accept(be, K, n_acc, 100)
        assert plain[:4] == counted[:4]                              # history, ids, position, stats: the call without the counter
        assert plain[2] == [11 + n_acc + 1] and plain[3][1] == n_acc
        assert plain[4] == [100, -9] and counted[4] == [100 + n_acc + 1, -9]
    plain, counted = accept(be, K, 0, 100, draft_only=True)
    assert plain == counted and counted[4] == [100, -9] and counted[2] == [11]
