#!/usr/bin/env python3
"""Generates tests/golden/reference_sampler_chain.npz by EXECUTING the reference's CPU sampler stages: the functions of
cpp/sampling.cpp as oracle/_ref/libsampling_ref.so exports them (C++-mangled names, read with `nm -D`), called through ctypes in
the order sample_basic calls them (ext_sampling.cpp:153-296).  The softmax is `softmax_cpu_nonavx2`, not the AVX2 dispatch.
What sample_basic does between the stage calls (the report loop, the skewed random point, the batch recurrence) is restated
here; only results are recorded.

Cases: vocabularies of 40-700 entries, 1-3 rows, fp32 logits (standard_normal x scale, NOT rounded to fp16, so that candidate
ties do not occur), each stage alone and in combinations, + one 32 000-entry fp16 row.

Run from the repo root:  python tests/golden/make_golden_sampler_chain.py
"""
import ctypes
import ctypes.util
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LIB = os.path.join(ROOT, "oracle", "_ref", "libsampling_ref.so")
OUT = os.path.join(ROOT, "tests", "golden", "reference_sampler_chain.npz")
F32 = np.float32
MAX_ROWS, MAX_PROBS = 3, 32

c_i, c_f, c_p = ctypes.c_int, ctypes.c_float, ctypes.c_void_p
STAGES = {
    "softmax": ("_Z19softmax_cpu_nonavx2ifPKfPKbfPf", c_i, [c_i, c_f, c_p, c_p, c_f, c_p]),
    "top_k": ("_Z9top_k_cpuiPfPiii", c_i, [c_i, c_p, c_p, c_i, c_i]),
    "normalize": ("_Z13normalize_cpuiPf", None, [c_i, c_p]),
    "top_p": ("_Z9top_p_cpuiPfPif", c_i, [c_i, c_p, c_p, c_f]),
    "top_a": ("_Z9top_a_cpuiPfPif", c_i, [c_i, c_p, c_p, c_f]),
    "min_p": ("_Z9min_p_cpuiPfPif", c_i, [c_i, c_p, c_p, c_f]),
    "tfs": ("_Z7tfs_cpuiPfPif", c_i, [c_i, c_p, c_p, c_f]),
    "typical": ("_Z11typical_cpuiPfPif", c_i, [c_i, c_p, c_p, c_f]),
    "mirostat_pre": ("_Z16mirostat_pre_cpuiPfPifff", c_i, [c_i, c_p, c_p, c_f, c_f, c_f]),
    "mirostat_post": ("_Z17mirostat_post_cpuiPfPifff", c_f, [c_i, c_p, c_p, c_f, c_f, c_f]),
    "post_temperature": ("_Z24post_softmax_temperatureiPfPiffff", c_i, [c_i, c_p, c_p, c_f, c_f, c_f, c_f]),
    "sort_descending": ("_Z15sort_descendingiPfPii", c_i, [c_i, c_p, c_p, c_i]),
    "multinomial": ("_Z15multinomial_cpuiPfPif", c_i, [c_i, c_p, c_p, c_f]),
}

NEUTRAL = {"top_a": 0.0, "tfs": 0.0, "typical": 0.0, "post_temperature": 1.0, "min_temp": 0.0, "max_temp": 0.0,
           "temp_exponent": 1.0, "smoothing_factor": 0.0, "skew": 0.0, "mirostat": False, "mirostat_tau": 0.0,
           "mirostat_eta": 0.0, "num_probs": 0}

# (vocab, rows, scale, (temperature, top_k, top_p, min_p), chain settings, mu of the rows or None)
SPECS = [
    (300, 1, 3.0, (0.8, 50, 0.8, 0.0), {}, None),
    (300, 3, 2.0, (1.0, 40, 0.0, 0.0), {"smoothing_factor": 0.7}, None),                      # the compounding division
    (257, 3, 1.5, (1.2, 30, 0.9, 0.0), {"smoothing_factor": 1.6}, None),
    (300, 2, 3.0, (1.0, 50, 0.0, 0.0), {"top_a": 0.2}, None),
    (120, 2, 2.0, (1.5, 12, 0.0, 0.001), {"top_a": 0.0001}, None),                            # top-a AND min-p hand back n + 1
    (120, 1, 2.0, (2.0, 9, 0.97, 0.0005), {"top_a": 0.00005}, None),
    (500, 2, 2.5, (1.0, 100, 0.0, 0.0), {"tfs": 0.9}, None),
    (500, 1, 1.0, (1.0, 200, 0.95, 0.0), {"tfs": 0.5}, None),
    (64, 2, 6.0, (0.7, 20, 0.2, 0.0), {"tfs": 0.8}, None),                                     # tfs with fewer than 3 candidates
    (40, 1, 8.0, (1.0, 2, 0.0, 0.0), {"tfs": 0.8}, None),
    (400, 2, 2.0, (1.0, 80, 0.0, 0.0), {"typical": 0.6}, None),
    (400, 1, 3.0, (0.9, 60, 0.9, 0.0), {"typical": 0.2}, None),
    (700, 3, 1.0, (1.0, 300, 0.0, 0.0), {"typical": 0.9}, None),
    (300, 2, 3.0, (1.0, 50, 0.0, 0.0), {"mirostat": True, "mirostat_tau": 1.5, "mirostat_eta": 0.1}, [0.0, 0.0]),
    (300, 2, 3.0, (1.0, 50, 0.0, 0.0), {"mirostat": True, "mirostat_tau": 1.5, "mirostat_eta": 0.1}, [2.25, 4.5]),
    (600, 1, 2.0, (0.8, 120, 0.9, 0.0), {"mirostat": True, "mirostat_tau": 3.0, "mirostat_eta": 0.3}, [5.0]),
    (300, 2, 3.0, (1.0, 50, 0.9, 0.0), {"post_temperature": 0.7}, None),                      # temperature_last
    (300, 1, 2.0, (1.0, 64, 0.0, 0.02), {"post_temperature": 1.8}, None),
    (300, 2, 2.0, (1.0, 50, 0.0, 0.0), {"min_temp": 0.5, "max_temp": 1.5, "temp_exponent": 1.0}, None),
    (450, 3, 3.0, (1.0, 90, 0.95, 0.0), {"min_temp": 0.2, "max_temp": 2.0, "temp_exponent": 2.5}, None),
    (300, 2, 3.0, (0.9, 50, 0.9, 0.0), {"skew": 0.7}, None),
    (300, 1, 2.0, (1.1, 40, 0.0, 0.0), {"skew": -1.2}, None),
    (300, 2, 3.0, (0.8, 50, 0.8, 0.0), {"num_probs": 5}, None),
    (300, 1, 2.0, (1.0, 100, 0.0, 0.0), {"num_probs": 32}, None),
    (200, 2, 6.0, (0.7, 30, 0.3, 0.0), {"num_probs": 12}, None),                               # more slots than candidates: filler ids
    (48, 1, 9.0, (1.0, 6, 0.5, 0.0), {"num_probs": 20}, None),
    (90, 1, 2.0, (1.0, 1, 0.0, 0.0), {"num_probs": 4, "mirostat": True, "mirostat_tau": 2.0, "mirostat_eta": 0.2}, [0.0]),  # greedy
    (300, 2, 2.0, (1.0, 60, 0.9, 0.02), {"top_a": 0.1, "tfs": 0.95}, None),
    (300, 2, 2.0, (1.0, 60, 0.0, 0.0), {"tfs": 0.9, "typical": 0.7, "skew": 0.4}, None),
    (512, 3, 2.5, (0.9, 128, 0.95, 0.01), {"typical": 0.8, "post_temperature": 0.8}, None),
    (300, 2, 3.0, (1.0, 50, 0.9, 0.0), {"mirostat": True, "mirostat_tau": 2.0, "mirostat_eta": 0.2, "post_temperature": 0.9,
                                        "top_a": 0.05}, [0.0, 3.0]),
    (300, 2, 3.0, (1.0, 50, 0.9, 0.0), {"mirostat": True, "mirostat_tau": 2.0, "mirostat_eta": 0.2, "num_probs": 5}, [0.0, 0.0]),
    (350, 3, 2.0, (1.0, 70, 0.0, 0.0), {"smoothing_factor": 0.9, "tfs": 0.9, "num_probs": 3}, None),
    (300, 2, 2.0, (1.0, 50, 0.0, 0.05), {"skew": 0.5, "num_probs": 8, "min_temp": 0.6, "max_temp": 1.4, "temp_exponent": 0.5}, None),
    (640, 2, 4.0, (1.3, 500, 0.0, 0.0), {"tfs": 0.97}, None),
    (640, 1, 1.0, (1.0, 500, 0.0, 0.0), {"typical": 0.95, "skew": -0.3}, None),
    (700, 1, 2.0, (1.0, 500, 0.99, 0.0), {"mirostat": True, "mirostat_tau": 6.0, "mirostat_eta": 0.1, "skew": 0.2}, [0.0]),
    (300, 1, 3.0, (0.005, 50, 0.8, 0.0), {"tfs": 0.5, "num_probs": 3}, None),                  # temperature < 0.01: greedy
    (301, 2, 2.0, (1.0, 33, 0.0, 0.0), {"top_a": 0.3, "typical": 0.5, "mirostat": True, "mirostat_tau": 1.0, "mirostat_eta": 0.5},
     [1.0, 0.0]),
    (32000, 1, 2.5, (0.8, 50, 0.9, 0.0), {"tfs": 0.95, "typical": 0.9, "post_temperature": 0.85, "skew": 0.3}, None),   # fp16 row
]


def cases():
    """[(logits [rows, vocab] (fp32; the 32 000-entry one fp16), (T, k, p, mp), chain dict (NEUTRAL's keys), mu list or None, random)]"""
    rng = np.random.default_rng(29)
    out = []
    for vocab, rows, scale, st, chain, mu in SPECS:
        lg = (rng.standard_normal((rows, vocab)) * scale).astype(np.float32)
        if vocab == 32000:
            lg = lg.astype(np.float16)
        c = dict(NEUTRAL)
        c.update(chain)
        out.append((lg, st, c, mu, float(rng.random())))
    return out


def load():
    if os.path.isdir(os.path.join(os.environ.get("EXL2_REFERENCE", "/root/reference"), "exllamav2", "exllamav2_ext", "cpp")):
        subprocess.check_call([os.path.join(ROOT, "oracle", "ref_build", "build.sh")], stdout=subprocess.DEVNULL)
    dll = ctypes.CDLL(LIB)
    fns = {}
    for name, (sym, res, args) in STAGES.items():
        f = getattr(dll, sym)
        f.restype, f.argtypes = res, args
        fns[name] = f
    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    for n, k in (("expf", 1), ("powf", 2)):
        getattr(libm, n).restype = c_f
        getattr(libm, n).argtypes = [c_f] * k
    fns["expf"], fns["powf"] = libm.expf, libm.powf
    return fns


def run_reference(fns, logits, st, c, mu, random):
    """The stage calls of sample_basic.  Returns tokens, probs, counts, mu, ktokens, kprobs (per row)."""
    bsz, vocab = logits.shape
    lg = np.ascontiguousarray(logits, dtype=np.float32)
    temperature, top_k, top_p, min_p = F32(st[0]), int(st[1]), st[2], st[3]
    K = int(c["num_probs"])
    P = np.zeros(vocab + 64, dtype=np.float32)
    I = np.zeros(vocab + 64, dtype=np.int32)
    p_, i_ = P.ctypes.data, I.ctypes.data
    if temperature < F32(0.01):
        temperature, top_k = F32(1.0), 1
    random = F32(random)
    mu = [0.0] * bsz if mu is None else [float(m) for m in mu]
    toks, prs, ncs = np.zeros(bsz, np.int32), np.zeros(bsz, F32), np.zeros(bsz, np.int32)
    mus, kts, kps = np.zeros(bsz, F32), np.zeros((bsz, K), np.int32), np.zeros((bsz, K), F32)
    for b in range(bsz):
        exponent = 1.0
        if c["smoothing_factor"] > 0:
            exponent = 2.0
            temperature = F32(temperature / F32(c["smoothing_factor"]))
        P[:] = 0
        maxlogit = fns["softmax"](vocab, float(temperature), lg[b].ctypes.data, None, exponent, p_)
        I[:] = 0
        I[:vocab] = np.arange(vocab)
        n = vocab
        if 0 < top_k < vocab:
            n = fns["top_k"](n, p_, i_, top_k, maxlogit); fns["normalize"](n, p_)
        if n > 1 and 0.0 < top_p < 1.0:
            n = fns["top_p"](n, p_, i_, top_p); fns["normalize"](n, p_)
        if n > 1 and c["top_a"] > 0.0:
            n = fns["top_a"](n, p_, i_, c["top_a"]); fns["normalize"](n, p_)
        if n > 1 and 0.0 < min_p < 1.0:
            n = fns["min_p"](n, p_, i_, min_p); fns["normalize"](n, p_)
        if n > 1 and 0.0 < c["tfs"] < 1.0:
            n = fns["tfs"](n, p_, i_, c["tfs"]); fns["normalize"](n, p_)
        if n > 1 and 0.0 < c["typical"] < 1.0:
            n = fns["typical"](n, p_, i_, c["typical"]); fns["normalize"](n, p_)
        if n > 1 and c["mirostat"]:
            n = fns["mirostat_pre"](n, p_, i_, mu[b], c["mirostat_tau"], c["mirostat_eta"]); fns["normalize"](n, p_)
        if n > 1 and (F32(c["post_temperature"]) != F32(1.0) or F32(c["max_temp"]) > F32(c["min_temp"])):
            n = fns["post_temperature"](n, p_, i_, c["post_temperature"], c["min_temp"], c["max_temp"], c["temp_exponent"])
        if K or c["skew"] != 0.0:
            fns["sort_descending"](n, p_, i_, K)
        if K:
            j = 0
            while j < n and j < K and P[j] != 0.0:
                kts[b, j], kps[b, j] = I[j], P[j]
                j += 1
            fake = 0
            while j < K:
                k = 0
                while k < n:
                    if I[k] == fake:
                        fake += 1
                        k = 0
                    k += 1
                kts[b, j], kps[b, j] = fake, 0.0
                fake += 1
                j += 1
        rs = random
        if c["skew"] != 0.0:
            rs = F32(fns["powf"](float(random), float(F32(fns["expf"](float(F32(-F32(c["skew"]))))))))
        radj = F32(float(rs) * 0.9998)
        fns["multinomial"](n, p_, i_, float(radj))
        toks[b], prs[b], ncs[b] = I[0], P[0], n
        if c["mirostat"]:
            mus[b] = fns["mirostat_post"](n, p_, i_, mu[b], c["mirostat_tau"], c["mirostat_eta"])
        if bsz > 1:
            r = random
            for _ in range(10):
                r = F32(float(r) + (1.337 + float(random)))
                r = F32(r * r)
                r = F32(np.fmod(r, F32(1.0)))
            random = r
    return toks, prs, ncs, mus, kts, kps


def main():
    fns = load()
    cs = cases()
    n = len(cs)
    z = {"tokens": np.full((n, MAX_ROWS), -1, np.int32), "probs": np.zeros((n, MAX_ROWS), F32),
         "num_candidates": np.zeros((n, MAX_ROWS), np.int32), "mu": np.zeros((n, MAX_ROWS), F32),
         "ktokens": np.full((n, MAX_ROWS, MAX_PROBS), -1, np.int32), "kprobs": np.zeros((n, MAX_ROWS, MAX_PROBS), F32)}
    for i, (lg, st, c, mu, rnd) in enumerate(cs):
        t, p, nc, m, kt, kp = run_reference(fns, lg, st, c, mu, rnd)
        r, K = lg.shape[0], int(c["num_probs"])
        z["tokens"][i, :r], z["probs"][i, :r], z["num_candidates"][i, :r], z["mu"][i, :r] = t, p, nc, m
        z["ktokens"][i, :r, :K], z["kprobs"][i, :r, :K] = kt, kp
    np.savez_compressed(OUT, **z)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes, {n} cases)")


if __name__ == "__main__":
    sys.exit(main())
