"""exl2_spec_accept_draft (csrc/spec_decode.hip) against the plain-Python restatement of its two rules (tests/spec_decode_oracle.py):
ids, pos, history and stats bit for bit, guard words around history and ids untouched."""
import numpy as np
import pytest

from tests import spec_decode_oracle as SO

GUARD = 4
G_H, G_I = -77001, -77002


def launch(be, seq, K, N, cand=None, drafts=None, forced=None, hist_len=None, stats=None, fill=-5):
    """One launch behind a sequence whose tokens 0 .. p are `seq` (p = len(seq) - 1, seq[p] = the step's input token) with the given
    drafts; cand None: the draft-only form.  Compares everything with the restatement and returns its (ids, history, pos, stats, n_acc)."""
    p = len(seq) - 1
    draft_only = cand is None
    hist_len = hist_len if hist_len is not None else p + K + 2 + 3
    hist = np.full((hist_len,), fill, dtype=np.int32)
    hist[:p + 1] = seq
    ids = np.array([seq[p]] + list(drafts if drafts is not None else [fill] * K), dtype=np.int32)
    stats = np.array(stats if stats is not None else [3, 5] + list(range(K + 1)) + [G_I], dtype=np.int32)
    want = SO.accept_draft(cand, ids, hist, p, stats, K, N, forced=forced, draft_only=draft_only)

    hbuf = np.concatenate([np.full((GUARD,), G_H, np.int32), hist, np.full((GUARD,), G_H, np.int32)])
    ibuf = np.concatenate([np.full((GUARD,), G_I, np.int32), ids, np.full((GUARD,), G_I, np.int32)])
    t_h, t_i, t_p, t_s = be.t(hbuf), be.t(ibuf), be.t(np.array([p], dtype=np.int32)), be.t(stats)
    t_c = None if draft_only else be.t(np.asarray(cand, dtype=np.int32))
    t_f = None if forced is None else be.t(np.asarray(forced, dtype=np.int32))
    be.ext.spec_accept_draft(t_c, t_i[GUARD:GUARD + K + 1], t_h[GUARD:GUARD + hist_len], t_p, t_s, K, N, forced=t_f, draft_only=draft_only)
    g_h, g_i, g_p, g_s = be.n(t_h), be.n(t_i), be.n(t_p), be.n(t_s)
    assert np.all(g_h[:GUARD] == G_H) and np.all(g_h[GUARD + hist_len:] == G_H), "guard words around history"
    assert np.all(g_i[:GUARD] == G_I) and np.all(g_i[GUARD + K + 1:] == G_I), "guard words around ids"
    assert g_i[GUARD:GUARD + K + 1].tolist() == want[0], (g_i[GUARD:GUARD + K + 1].tolist(), want[0])
    assert g_h[GUARD:GUARD + hist_len].tolist() == want[1]
    assert int(g_p[0]) == want[2]
    assert g_s.tolist() == want[3]
    return want


def step_inputs(rng, truth, K, n_acc):
    """cand = the K + 1 true tokens, drafts = the first n_acc of them, then a wrong one, then anything"""
    cand = [int(t) for t in truth[:K + 1]]
    drafts = cand[:n_acc] + ([cand[n_acc] + 1] if n_acc < K else []) + [int(t) for t in rng.integers(0, 4, size=max(0, K - n_acc - 1))]
    return cand, drafts


@pytest.mark.parametrize("N", [1, 3, 7])
@pytest.mark.parametrize("K", [1, 3, 7, 15])
def test_every_acceptance_length(be, K, N):
    rng = np.random.default_rng(100 * K + N)
    for n_acc in range(K + 1):
        seq = rng.integers(0, 4, size=int(rng.integers(1, 40))).tolist()
        cand, drafts = step_inputs(rng, rng.integers(0, 4, size=K + 1), K, n_acc)
        got = launch(be, seq, K, N, cand, drafts)
        assert got[4] == n_acc and got[2] == len(seq) + n_acc


def test_no_match_repeats_the_last_token(be):
    got = launch(be, [10, 11, 12, 13], 3, 3, cand=[14, 15, 16, 17], drafts=[14, 15, 0])
    assert got[4] == 2 and got[0] == [16, 16, 16, 16]


def test_match_only_at_one_token(be):
    # suffix ... 8 3: "8 3" and "9 8 3" occur nowhere else, 3 does (followed by 6 7)
    got = launch(be, [1, 3, 6, 7, 9, 8], 3, 3, cand=[3, 0, 0, 0], drafts=[2, 2, 2])
    assert got[4] == 0 and got[0] == [3, 6, 7, 9]


def test_longer_earlier_match_beats_shorter_later(be):
    # suffix 1 2 3: the trigram sits early (then 50 51), a later "2 3" (then 60) and a still later "3" (then 70) must lose
    seq = [1, 2, 3, 50, 51, 9, 2, 3, 60, 9, 9, 3, 70, 1, 2]
    got = launch(be, seq, 2, 3, cand=[3, 0, 0], drafts=[0, 0])
    assert got[0] == [3, 50, 51]
    # ... with a context of two tokens the later bigram wins, with one the latest single token
    assert launch(be, seq, 2, 2, cand=[3, 0, 0], drafts=[0, 0])[0] == [3, 60, 9]
    assert launch(be, seq, 2, 1, cand=[3, 0, 0], drafts=[0, 0])[0] == [3, 70, 1]


def test_latest_match_wins_among_equal_lengths(be):
    seq = [1, 2, 30, 1, 2, 40, 1, 2, 50, 7, 1]
    got = launch(be, seq, 3, 2, cand=[2, 0, 0, 0], drafts=[0, 0, 0])
    assert got[0] == [2, 50, 7, 1]


@pytest.mark.parametrize("period", [1, 2, 3])
def test_continuation_runs_into_the_drafts(be, period):
    unit = [[5], [1, 2], [1, 2, 3]][period - 1]
    seq = [8, 9] + unit * 2
    cand = [unit[0]] + [0] * 7
    got = launch(be, seq, 7, 3, cand=cand, drafts=[99] * 7)
    assert got[4] == 0
    want = [(unit * 8)[(1 + i) % period] for i in range(7)]
    assert got[0] == [unit[0]] + want


def test_ngram_made_of_tokens_this_launch_accepted(be):
    # the suffix 1 2 3 ends in two tokens logged by this launch; its earlier occurrence is old
    got = launch(be, [1, 2, 3, 4, 8, 1], 3, 3, cand=[2, 3, 0, 0], drafts=[2, 0, 0])
    assert got[4] == 1 and got[0] == [3, 4, 8, 1]
    # the match itself consists of tokens logged by this launch only
    got = launch(be, [1, 2, 3], 3, 3, cand=[9, 9, 9, 9], drafts=[9, 9, 9])
    assert got[4] == 3 and got[0] == [9, 9, 9, 9]
    got = launch(be, [1, 2, 3], 3, 3, cand=[7, 6, 7, 6], drafts=[7, 6, 7])
    assert got[4] == 3 and got[0] == [6, 7, 6, 7]


@pytest.mark.parametrize("N", [1, 3, 7])
def test_shortest_sequences(be, N):
    rng = np.random.default_rng(N)
    launch(be, [2], 3, N)                                                  # L = 1, draft only
    for L in (N, N + 1):
        seq = rng.integers(0, 2, size=L).tolist()
        launch(be, seq, 3, N)                                              # draft only at L
        if L >= 2:
            for n_acc in range(min(L - 2, 3) + 1):                         # accept form: L = p + n_acc + 2
                p = L - n_acc - 2
                cand, drafts = step_inputs(rng, rng.integers(0, 2, size=4), 3, n_acc)
                assert launch(be, seq[:p + 1], 3, N, cand, drafts)[2] + 1 == L


@pytest.mark.parametrize("L,hist_len", [(5000, 5100), (3000, 3100)])
def test_long_history_every_thread_strides(be, L, hist_len):
    rng = np.random.default_rng(L)
    seq = (1000 + np.arange(L - 1)).tolist()                               # all distinct ...
    for at in (0, 1, 700, 2047, L - 400):                                  # ... but for one planted trigram
        s = list(seq)
        s[at:at + 3] = [1, 2, 3]
        s[-2:] = [1, 2]
        got = launch(be, s, 7, 3, cand=[3] + [0] * 7, drafts=[0] * 7, hist_len=hist_len)
        assert got[0][1:] == s[at + 3:at + 10]
    s = rng.integers(0, 4, size=L - 1).tolist()
    launch(be, s, 7, 7, cand=rng.integers(0, 4, size=8).tolist(), drafts=rng.integers(0, 4, size=7).tolist(), hist_len=hist_len)


def test_match_at_both_ends_of_the_range(be):
    # j = n - 1: the sequence's first n tokens are the only earlier occurrence
    got = launch(be, [1, 2, 3, 40, 41, 42, 43, 1, 2], 2, 3, cand=[3, 0, 0], drafts=[0, 0])
    assert got[0] == [3, 40, 41]
    # j = L - 2: the occurrence ends one token before the end
    got = launch(be, [9, 8, 5, 5], 2, 3, cand=[5, 0, 0], drafts=[0, 0])
    assert got[0] == [5, 5, 5]
    got = launch(be, [9, 8, 7, 5], 2, 1, cand=[5, 0, 0], drafts=[0, 0])
    assert got[0] == [5, 5, 5]


@pytest.mark.parametrize("n_acc", [0, 2, 3])
def test_history_that_ends_with_the_step(be, n_acc):
    """hist_len exactly L + K: at full acceptance the launch logs the last word of the array"""
    rng = np.random.default_rng(n_acc)
    seq = rng.integers(0, 4, size=20).tolist()
    cand, drafts = step_inputs(rng, rng.integers(0, 4, size=4), 3, n_acc)
    L = len(seq) + n_acc + 1
    launch(be, seq, 3, 3, cand, drafts, hist_len=L + 3)


def test_position_outside_the_log_changes_nothing(be):
    K, hist_len = 3, 12
    hist = np.arange(hist_len, dtype=np.int32)
    for p in (hist_len - K - 1, hist_len, -1):
        t_h, t_i, t_p = be.t(hist), be.t(np.array([1, 2, 3, 4], np.int32)), be.t(np.array([p], np.int32))
        t_s, t_c = be.t(np.zeros((K + 3,), np.int32)), be.t(np.array([2, 3, 4, 5], np.int32))
        be.ext.spec_accept_draft(t_c, t_i, t_h, t_p, t_s, K, 3)
        assert be.n(t_h).tolist() == hist.tolist() and be.n(t_i).tolist() == [1, 2, 3, 4]
        assert be.n(t_p).tolist() == [p] and not be.n(t_s).any()


def test_forced_drafts(be):
    forced = list(range(100, 130))
    seq = forced[:10]
    got = launch(be, seq, 3, 3, cand=forced[10:14], drafts=forced[10:12] + [0], forced=forced)
    assert got[4] == 2 and got[0] == forced[12:16]
    # running off the end of the forced tokens: the sequence's last token from there on
    got = launch(be, forced[:27], 7, 3, cand=forced[27:] + [1, 2, 3, 4, 5], drafts=forced[27:] + [0] * 4, forced=forced)
    assert got[4] == 3 and got[0] == [1] + [1] * 7
    got = launch(be, forced[:25], 7, 3, cand=forced[25:] + [1, 2, 3], drafts=[0] * 7, forced=forced)
    assert got[4] == 0 and got[0] == [125, 126, 127, 128, 129, 125, 125, 125]
    launch(be, forced[:5], 3, 3, forced=forced)                            # draft only
    launch(be, forced[:5], 3, 3, forced=[])


def test_argument_checks(be):
    t = lambda n: be.t(np.zeros((n,), np.int32))
    with pytest.raises(RuntimeError, match="K 16"):
        be.ext.spec_accept_draft(t(17), t(17), t(64), t(1), t(19), 16, 3)
    with pytest.raises(RuntimeError, match="n-gram context 8"):
        be.ext.spec_accept_draft(t(4), t(4), t(64), t(1), t(6), 3, 8)
    with pytest.raises(RuntimeError, match="K \\+ 1"):
        be.ext.spec_accept_draft(t(4), t(5), t(64), t(1), t(6), 3, 3)
    with pytest.raises(RuntimeError, match="hist_len"):
        be.ext.spec_accept_draft(t(4), t(4), t(4), t(1), t(6), 3, 3)


def test_random_histories(be):
    """200 seeded histories over four symbols: matches of every length are the rule, not the exception"""
    rng = np.random.default_rng(2024)
    seen = set()
    for _ in range(200):
        K = int(rng.choice([1, 2, 3, 4, 7, 15])); N = int(rng.integers(1, 8))
        seq = rng.integers(0, 4, size=int(rng.integers(1, 120))).tolist()
        if rng.integers(0, 8) == 0:
            launch(be, seq, K, N)
            continue
        n_acc = int(rng.integers(0, K + 1))
        cand, drafts = step_inputs(rng, rng.integers(0, 4, size=K + 1), K, n_acc)
        got = launch(be, seq, K, N, cand, drafts)
        seen.add(got[4])
    assert {0, 1, 2, 3} <= seen


def test_consecutive_launches_follow_the_restatement(be):
    """a decode loop in miniature: each launch's drafts are verified by the next against a periodic 'model'"""
    K, N, hist_len = 3, 3, 64
    truth = ([4, 5, 6, 7, 5] * 16)[:hist_len]
    t_h = be.t(np.array(truth[:3] + [0] * (hist_len - 3), np.int32))
    t_i, t_p, t_s = be.t(np.array([truth[2], 0, 0, 0], np.int32)), be.t(np.array([2], np.int32)), be.t(np.zeros((K + 3,), np.int32))
    be.ext.spec_accept_draft(None, t_i, t_h, t_p, None, K, N, draft_only=True)
    ids, hist, p, stats = be.n(t_i).tolist(), be.n(t_h).tolist(), 2, [0] * (K + 3)
    assert ids == SO.accept_draft(None, [truth[2], 0, 0, 0], hist, 2, stats, K, N, draft_only=True)[0]
    for _ in range(10):
        # the arg-max of row i = the true token behind position p + i, provided the drafts before it were right
        cand = [truth[p + 1 + i] for i in range(K + 1)]
        be.ext.spec_accept_draft(be.t(np.array(cand, np.int32)), t_i, t_h, t_p, t_s, K, N)
        ids, hist, p, stats, _ = SO.accept_draft(cand, ids, hist, p, stats, K, N)
        assert be.n(t_i).tolist() == ids and be.n(t_h).tolist() == hist and be.n(t_p).tolist() == [p] and be.n(t_s).tolist() == stats
    assert hist[:p + 1] == truth[:p + 1] and stats[1] > 0
