"""Plain-Python restatement of the speculative greedy step's accept rule and draft rule (include/exl2_hip.h,
exl2_spec_accept_draft).  Lists and loops only: no kernel code, nothing shared with csrc/spec_decode.hip."""


def draft(seq, K, N, forced=None):
    """The K drafts behind seq (a list of tokens, the next step's input token last)."""
    L = len(seq)
    if forced is not None:
        return [int(forced[L + i]) if L + i < len(forced) else int(seq[L - 1]) for i in range(K)]
    for n in range(min(N, L - 1), 0, -1):
        suffix = seq[L - n:L]
        for j in range(L - 2, n - 2, -1):                    # the largest j in [n - 1, L - 2]
            if seq[j - n + 1:j + 1] == suffix:
                ext = list(seq)
                for i in range(K):                           # overlapping copy: a source behind the end is a draft made before
                    ext.append(ext[j + 1 + i])
                return [int(t) for t in ext[L:]]
    return [int(seq[L - 1])] * K


def accept_draft(cand, ids, history, pos, stats, K, N, forced=None, draft_only=False):
    """One launch on copies of the arrays; returns (ids, history, pos, stats, n_acc).  n_acc is None for a draft-only launch."""
    ids, history, stats = [int(t) for t in ids], [int(t) for t in history], [int(t) for t in stats]
    p = int(pos)
    assert len(ids) == K + 1 and 1 <= K <= 15 and 1 <= N <= 7
    if draft_only:
        assert 0 <= p and p + 1 <= len(history)
        assert history[p] == ids[0]
        ids[1:] = draft(history[:p + 1], K, N, forced)
        return ids, history, p, stats, None
    assert 0 <= p and p + K + 2 <= len(history) and len(cand) == K + 1 and len(stats) >= K + 3
    n_acc = 0
    while n_acc < K and ids[n_acc + 1] == int(cand[n_acc]):
        n_acc += 1
    for i in range(n_acc + 1):
        history[p + 1 + i] = int(cand[i])
    p1 = p + n_acc + 1
    ids[0] = int(cand[n_acc])
    stats[0] += 1
    stats[1] += n_acc
    stats[2 + n_acc] += 1
    ids[1:] = draft(history[:p1 + 1], K, N, forced)
    return ids, history, p1, stats, n_acc
