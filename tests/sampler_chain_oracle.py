"""Oracle for the rest of the reference's sampler chain (csrc/sampling.hip, the CHAIN instantiations): a numpy fp32 restatement
of smoothing, top-a, tfs, typical, mirostat, post-softmax / dynamic temperature, skew and the top-token report in sample_basic's
order (exllamav2_ext/ext_sampling.cpp:153-296 over cpp/sampling.cpp), on top of oracle/sampling.py's stages.

TEST INFRASTRUCTURE ONLY.  Pinned by execution: tests/golden/reference_sampler_chain.npz holds what the reference's own stage
functions (oracle/_ref/libsampling_ref.so) return for tests/golden/make_golden_sampler_chain.py's cases, and
tests/test_sampler_chain_oracle.py checks this file against it bit for bit.  logf / powf / expf / log2f are libm's (ctypes), the
functions the compiled reference calls.

Per row the oracle also reports
  * margin: how far the closest threshold comparison was from flipping (the kernel's softmax sum is a tree sum and its
    transcendentals are the device's: a decision closer than that may fall the other way without anything being wrong);
  * tie: two candidates had equal keys in a sort (the reference's quicksort leaves them in no defined order; the kernel orders
    them by token id), or the reference's sort stopped early (the report's partial sort) in an order a full sort does not give.
"""
from __future__ import annotations

import ctypes
import ctypes.util
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import sampling as osamp            # noqa: E402

F32 = np.float32
_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _n, _k in (("logf", 1), ("expf", 1), ("log2f", 1), ("powf", 2)):
    getattr(_libm, _n).restype = ctypes.c_float
    getattr(_libm, _n).argtypes = [ctypes.c_float] * _k

NEUTRAL = {"top_a": 0.0, "tfs": 0.0, "typical": 0.0, "post_temperature": 1.0, "min_temp": 0.0, "max_temp": 0.0,
           "temp_exponent": 1.0, "smoothing_factor": 0.0, "skew": 0.0, "mirostat": False, "mirostat_tau": 0.0,
           "mirostat_eta": 0.0, "num_probs": 0}
EPS = F32(1e-8)


def logf(x): return F32(_libm.logf(float(x)))
def expf(x): return F32(_libm.expf(float(x)))
def log2f(x): return F32(_libm.log2f(float(x)))
def powf(x, y): return F32(_libm.powf(float(x), float(y)))


def softmax(logits, temperature, flt, exponent2: bool):
    """cpp/sampling.cpp:113-162 with the quadratic exponent (l *= -l) of smoothing."""
    if not exponent2:
        return osamp.softmax(logits, temperature, flt)
    v = logits.shape[0]
    l32 = logits.astype(F32)
    itemp = F32(1.0) / F32(temperature)
    maxl, maxi = F32(-1e38), 0
    for i in range(v):
        if flt is not None and not flt[i]:
            continue
        if l32[i] > maxl:
            maxl, maxi = l32[i], i
    out = np.zeros(v, dtype=F32)
    esum = F32(0.0)
    for i in range(v):
        if flt is not None and not flt[i]:
            continue
        l = F32(l32[i] - maxl)
        l = F32(l * F32(-l))
        e = expf(F32(l * itemp))
        out[i] = e
        esum = F32(esum + e)
    isum = F32(1.0) / esum
    for i in range(v):
        out[i] = F32(out[i] * isum) if (flt is None or flt[i]) else F32(0.0)
    return out, maxi


def _swap(A, B, i, j):
    A[i], A[j] = A[j], A[i]
    B[i], B[j] = B[j], B[i]


def pre_sort(P, I, n, st):
    """cpp/sampling.cpp:399-421."""
    i, j = 0, n - 1
    for k in range(n):
        if F32(0.5e-8) <= P[k] <= F32(2e-8):
            st["margin"] = 0.0                    # the 1e-8 cut itself is undecided
    while i <= j:
        if P[j] < EPS:
            j -= 1
            continue
        if P[i] >= EPS:
            i += 1
            continue
        _swap(P, I, i, j)
        i += 1
        j -= 1
    return i


def quicksort(A, X, low, high, max_index, desc: bool):
    """cpp/sampling.cpp:301-394 (pivot = last entry, short segments by bubble passes, recursion only into segments that
    start at or before max_index).  out-of-order test: desc a < b, asc a > b."""
    bad = (lambda a, b: a < b) if desc else (lambda a, b: a > b)
    stack = [(low, high)]
    while stack:
        low, high = stack.pop()
        if low >= high:
            continue
        m = high - low
        if m <= 4:
            for last in range(m, 0, -1):
                for q in range(low, low + last):
                    if bad(A[q], A[q + 1]):
                        _swap(A, X, q, q + 1)
            continue
        pivot = A[high]
        i = low - 1
        for j in range(low, high):
            if not bad(A[j], pivot):
                i += 1
                _swap(A, X, i, j)
        _swap(A, X, i + 1, high)
        pos = i + 1
        # (the two recursions are independent of each other: any order)
        if max_index == 0 or pos <= max_index:
            stack.append((pos + 1, high))
        if max_index == 0 or low <= max_index:
            stack.append((low, pos - 1))


def _note_ties(keys, st):
    if len(np.unique(np.asarray(keys, dtype=F32).view(np.uint32))) != len(keys):
        st["tie"] = True


def sort_descending(P, I, n, max_index, st):
    """cpp/sampling.cpp:424-440.  Marks the row when equal keys were sorted, or when the partial sort left an order a full
    sort would not."""
    pre = pre_sort(P, I, n, st)
    _note_ties(P[:pre], st)
    if 0 < max_index < pre:
        full = np.sort(P[:pre])[::-1]
        quicksort(P, I, 0, pre - 1, max_index, True)
        if not np.array_equal(full, P[:pre]):
            st["tie"] = True
    else:
        quicksort(P, I, 0, pre - 1, max_index, True)
    return pre


def top_a(P, I, n, ta, st):
    top = P[0]
    for i in range(1, n):
        if P[i] > top:
            top = P[i]
    thr = F32(F32(F32(ta) * top) * top)
    st["margin"] = min(st["margin"], min(abs(float(P[i]) - float(thr)) for i in range(n + 1)))
    return osamp.keep_threshold(P, I, n, thr)


def tfs(P, I, n, z, st):
    if n < 3:
        return n
    nc = sort_descending(P, I, n, n, st)
    d = np.zeros(max(nc - 2, 0), dtype=F32)
    dsum = F32(0.0)
    for i in range(nc - 2):
        d[i] = abs(F32(F32(F32(-P[i]) + F32(F32(2.0) * P[i + 1])) - P[i + 2]))
        dsum = F32(dsum + d[i])
    with np.errstate(divide="ignore"):
        dsum_i = F32(1.0) / dsum
    k, cum, z = 0, F32(0.0), F32(z)
    while k < nc - 2:
        cum = F32(cum + F32(d[k] * dsum_i))
        st["margin"] = min(st["margin"], abs(float(cum) - float(z)))
        if cum > z:
            break
        k += 1
    return k + 1


def typical(P, I, n, typ, st):
    r = pre_sort(P, I, n, st)
    y = np.zeros(r, dtype=F32)
    neg = F32(0.0)
    for i in range(r):
        y[i] = F32(P[i] + logf(F32(P[i] + F32(1e-10))))
        neg = F32(neg + F32(P[i] * y[i]))
    dev = np.array([abs(F32(y[i] - neg)) for i in range(r)], dtype=F32)
    order = np.arange(r, dtype=np.int64)
    _note_ties(dev, st)
    quicksort(dev, order, 0, r - 1, r, False)
    tp_, ti_ = P[:r].copy(), I[:r].copy()
    cum, num, typ = F32(0.0), 0, F32(typ)
    while True:
        j = int(order[num])
        P[num], I[num] = tp_[j], ti_[j]
        cum = F32(cum + tp_[j])
        st["margin"] = min(st["margin"], abs(float(cum) - float(typ)))
        if cum >= typ:
            break
        num += 1
        if num >= r:
            break
    return max(num, 1)


def mirostat_pre(P, I, n, mu, tau, st):
    mu = F32(mu)
    if mu == F32(0.0):
        mu = F32(F32(tau) * F32(2.0))
    nc = sort_descending(P, I, n, n, st)
    target = powf(F32(2.0), F32(-mu))
    k = 1
    while k < nc:
        st["margin"] = min(st["margin"], abs(float(P[k]) - float(target)))
        if P[k] < target:
            break
        k += 1
    return k


def mirostat_post(p_chosen, mu, tau, eta):
    mu = F32(mu)
    if mu == F32(0.0):
        mu = F32(F32(tau) * F32(2.0))
    surprise = F32(-log2f(p_chosen))
    return F32(mu + F32(F32(eta) * F32(F32(tau) - surprise)))


def post_temperature(P, n, temperature, min_temp, max_temp, exponent):
    temperature, min_temp, max_temp = F32(temperature), F32(min_temp), F32(max_temp)
    if max_temp > min_temp:
        ent = F32(0.0)
        for i in range(n):
            if P[i] > F32(0.0):
                ent = F32(ent - F32(P[i] * logf(P[i])))
        mx = F32(-logf(F32(1.0) / F32(n)))
        if mx == F32(0.0):
            mx = F32(1.0)
        temperature = F32(min_temp + F32(F32(max_temp - min_temp) * powf(F32(ent / mx), F32(exponent))))
    itemp = F32(1.0) / temperature
    s = F32(0.0)
    for i in range(n):
        P[i] = powf(P[i], itemp)
        s = F32(s + P[i])
    ips = F32(1.0) / s
    for i in range(n):
        P[i] = F32(P[i] * ips)


def report(P, I, n, num_probs):
    """ext_sampling.cpp:244-268, the filler ids as the loop runs (`k = 0` inside the for: the rescan resumes at 1)."""
    kt, kp = np.zeros(num_probs, dtype=np.int32), np.zeros(num_probs, dtype=F32)
    j = 0
    while j < n and j < num_probs:
        if P[j] == F32(0.0):
            break
        kt[j], kp[j] = I[j], P[j]
        j += 1
    fake = 0
    while j < num_probs:
        k = 0
        while k < n:
            if I[k] == fake:
                fake += 1
                k = 0
            k += 1
        kt[j], kp[j] = fake, F32(0.0)
        fake += 1
        j += 1
    return kt, kp


def sample_chain(logits, temperature, k, tp, mp, random, chain=None, mu=None, logit_filter=None, per_row_random=None):
    """sample_basic (ext_sampling.cpp:137-301) for every setting the device sampler covers.  logits [bsz, vocab]; chain: NEUTRAL's
    keys; mu: list of bsz floats (mirostat).  per_row_random: a list of points, one per row -- every row is then a batch-1 call
    (no recurrence, the temperature divided by smoothing_factor once).
    Returns a dict: tokens, probs, counts, mu, ktokens, kprobs, margin [bsz], tie [bsz]."""
    c = dict(NEUTRAL)
    c.update(chain or {})
    bsz, vocab = logits.shape
    temperature = F32(temperature)
    if temperature < F32(0.01):
        temperature, k = F32(1.0), 1
    random = F32(random)
    K = int(c["num_probs"])
    out = {"tokens": np.zeros(bsz, np.int32), "probs": np.zeros(bsz, F32), "counts": np.zeros(bsz, np.int32),
           "mu": np.zeros(bsz, F32), "ktokens": np.zeros((bsz, K), np.int32), "kprobs": np.zeros((bsz, K), F32),
           "margin": np.ones(bsz), "tie": np.zeros(bsz, bool)}
    mu = [0.0] * bsz if mu is None else list(mu)
    for b in range(bsz):
        st = {"margin": 1.0, "tie": False}
        if per_row_random is not None:
            random = F32(per_row_random[b])
            t_row = F32(temperature / F32(c["smoothing_factor"])) if c["smoothing_factor"] > 0 else temperature
        else:
            if c["smoothing_factor"] > 0:
                temperature = F32(temperature / F32(c["smoothing_factor"]))
            t_row = temperature
        flt = None if logit_filter is None else logit_filter[b].astype(bool)
        P0, maxi = softmax(logits[b], t_row, flt, c["smoothing_factor"] > 0)
        P = np.zeros(vocab + 8, dtype=F32)
        P[:vocab] = P0
        I = np.zeros(vocab + 8, dtype=np.int64)
        I[:vocab] = np.arange(vocab)
        n = vocab
        assert 0 < k < vocab
        if k > 1:
            srt = np.sort(P0)[::-1]
            if srt[k] > 0 and srt[k - 1] != srt[k]:
                st["margin"] = min(st["margin"], float(srt[k - 1] - srt[k]) / float(srt[k - 1]) * 1e2)
        n = osamp.top_k(P, I, n, k, maxi)
        osamp.normalize(P, n)
        if n > 1 and 0.0 < tp < 1.0:
            n, m = osamp.top_p(P, I, n, tp)
            st["margin"] = min(st["margin"], m)
            osamp.normalize(P, n)
        if n > 1 and c["top_a"] > 0.0:
            n = top_a(P, I, n, c["top_a"], st)
            osamp.normalize(P, n)
        if n > 1 and 0.0 < mp < 1.0:
            n, m = osamp.min_p(P, I, n, mp)
            st["margin"] = min(st["margin"], m)
            osamp.normalize(P, n)
        if n > 1 and 0.0 < c["tfs"] < 1.0:
            n = tfs(P, I, n, c["tfs"], st)
            osamp.normalize(P, n)
        if n > 1 and 0.0 < c["typical"] < 1.0:
            n = typical(P, I, n, c["typical"], st)
            osamp.normalize(P, n)
        if n > 1 and c["mirostat"]:
            n = mirostat_pre(P, I, n, mu[b], c["mirostat_tau"], st)
            osamp.normalize(P, n)
        if n > 1 and (F32(c["post_temperature"]) != F32(1.0) or F32(c["max_temp"]) > F32(c["min_temp"])):
            post_temperature(P, n, c["post_temperature"], c["min_temp"], c["max_temp"], c["temp_exponent"])
        if K or c["skew"] != 0.0:
            sort_descending(P, I, n, K, st)
        if K:
            out["ktokens"][b], out["kprobs"][b] = report(P, I, n, K)
        rs = random
        if c["skew"] != 0.0:
            rs = powf(random, expf(F32(-F32(c["skew"]))))
        radj = F32(float(rs) * 0.9998)
        tok, pr, m = osamp.multinomial(P, I, n, radj)
        st["margin"] = min(st["margin"], m)
        out["tokens"][b], out["probs"][b], out["counts"][b] = tok, pr, n
        if c["mirostat"]:
            out["mu"][b] = mirostat_post(pr, mu[b], c["mirostat_tau"], c["mirostat_eta"])
        out["margin"][b], out["tie"][b] = st["margin"], st["tie"]
        if bsz > 1 and per_row_random is None:
            random = osamp.next_random(random)
    return out
