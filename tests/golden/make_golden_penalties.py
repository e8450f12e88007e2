#!/usr/bin/env python3
"""Generates tests/golden/reference_penalties.npz by EXECUTING the reference's apply_rep_penalty_cpu (cpp/sampling.cpp:20-110,
compiled as it lies; oracle/ref_build/sampling_driver.cpp exports it as ref_apply_rep_penalty) on the cases of `cases()`: two
vocabularies (257: not a multiple of 4; 2048), sequence lengths around the kernel's strides and beyond the vocabulary, ids drawn
from a range slightly wider than the vocabulary, a sequence of one repeated id, ids 0 and vocab - 1, logits of exactly 0.0 and -inf
at penalised ids, and eight settings (empty window, long ramp with a frequency penalty inside it, neutral, a sustain range longer
than the sequence, and the four of make_golden_sampling.REP_SETTINGS).

The reference changes only the logits of ids inside the window, so the fixture keeps, per case, the indices whose bits changed and
their new values (`idx_<i>`, `val_<i>`); `expected(z, i, logits)` puts them back into a copy of the input.  The inputs are not
stored: `cases()` regenerates them from its seed.

Run from the repo root:  python tests/golden/make_golden_penalties.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden_sampling as gold          # noqa: E402

ROOT = gold.ROOT
PATH = os.path.join(ROOT, "tests", "golden", "reference_penalties.npz")

# (penalty, sustain, decay, frequency, presence)
SETTINGS = list(gold.REP_SETTINGS) + [(1.3, 0, 0, 0.2, 0.1), (1.15, 100, 700, 0.05, 0.02), (1.0, -1, 0, 0.0, 0.0), (1.2, 5000, 10, 0.1, 0.0)]
LENGTHS = [1, 2, 63, 64, 65, 1023, 1025, 2500]
VOCABS = [257, 2048]


def cases():
    """[(name, vocab, sequence int64 [L], logits fp32 [vocab], settings, fp16_representable)]"""
    rng = np.random.default_rng(29)
    out = []

    def logits(vocab, half):
        lg = (rng.standard_normal(vocab) * 3).astype(np.float32)
        return lg.astype(np.float16).astype(np.float32) if half else lg

    def add(name, vocab, seq, lg, st, half):
        out.append((name, vocab, np.ascontiguousarray(seq, dtype=np.int64), np.ascontiguousarray(lg, dtype=np.float32), st, half))

    for vi, vocab in enumerate(VOCABS):
        for li, L in enumerate(LENGTHS):
            seq = rng.integers(0, vocab + 9, size=L)               # ids >= vocab: outside the vocabulary, still walk steps
            for k in range(3):
                half = len(out) % 2 == 0
                add(f"len{L}", vocab, seq, logits(vocab, half), SETTINGS[(3 * li + k + vi) % len(SETTINGS)], half)
        for st in (SETTINGS[0], SETTINGS[1], SETTINGS[3], SETTINGS[5]):
            add("one_id", vocab, np.full(300, 5), logits(vocab, True), st, True)
        seq = rng.integers(0, vocab, size=64)
        seq[3] = 0; seq[40] = vocab - 1; seq[63] = 0
        for st in (SETTINGS[1], SETTINGS[2]):
            add("edges", vocab, seq, logits(vocab, False), st, False)
        seq = rng.integers(0, vocab, size=65)
        seq[-2] = (seq[-1] + 1) % vocab
        for st in (SETTINGS[0], SETTINGS[1], SETTINGS[3], SETTINGS[5]):
            lg = logits(vocab, True)
            lg[seq[-1]] = 0.0
            lg[seq[-2]] = -np.inf
            add("zero_inf", vocab, seq, lg, st, True)
    return out


def expected(z, i, lg):
    want = lg.copy()
    want[z[f"idx_{i}"]] = z[f"val_{i}"]
    return want


def main():
    lib = gold.load()
    arrays = {}
    for i, (name, vocab, seq, lg, st, half) in enumerate(cases()):
        got = gold.run_reference_rep_penalty(lib, seq[None], lg[None], st)[0]
        changed = np.nonzero(got.view(np.uint32) != lg.view(np.uint32))[0]
        # what the sparse form relies on: nothing outside the window's ids moves
        inside = np.zeros(vocab, dtype=bool)
        inside[seq[(seq >= 0) & (seq < vocab)]] = True
        assert inside[changed].all(), name
        arrays[f"idx_{i}"] = changed.astype(np.int32)
        arrays[f"val_{i}"] = got[changed]
    np.savez_compressed(PATH, **arrays)
    print(f"wrote {PATH} ({os.path.getsize(PATH)} bytes, {len(cases())} cases)")


if __name__ == "__main__":
    sys.exit(main())
