#!/usr/bin/env python3
"""Times the device sampler (csrc/sampling.hip, exl2_sample_rows) on an MI355X: one JSON line per (vocabulary, rows, setting),
microseconds per launch from HIP events on the launching stream (100 launches after 10 warm-up ones), next to the greedy
arg-max kernel of the decode graph on the same logits.  Usage: python tools/sampler_bench.py > profiles/rNN_sampler_bench.jsonl

--chain: the rest of the sampler chain (exl2_sample_rows_chain) instead -- vocabulary 32 000, one row: the default-settings launch of
exl2_sample_rows in five rounds (its run-to-run spread), the chain entry with every setting neutral, then each stage alone at top_k = 50
and 500; written to profiles/sampler_chain.json (--out).  --default-only: just the five rounds of the default launch, as one JSON line
(for a run on another build of the library through EXL2_HIP_LIB, e.g. the parent commit's)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from exllamav2_amd.ext import ext_c  # noqa: E402


def timed(fn, reps=100, warm=10):
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


CHAIN_STAGES = (("neutral", {}), ("smoothing_factor 0.8", {"smoothing_factor": 0.8}), ("top_a 0.1", {"top_a": 0.1}),
                ("tfs 0.95", {"tfs": 0.95}), ("typical 0.9", {"typical": 0.9}),
                ("mirostat tau 5 eta 0.1", {"mirostat": True, "mirostat_tau": 5.0, "mirostat_eta": 0.1}),
                ("temperature_last 0.8", {"post_temperature": 0.8}),
                ("dynamic temperature 0.5..1.5", {"min_temp": 0.5, "max_temp": 1.5, "temp_exponent": 1.0}),
                ("skew 0.5", {"skew": 0.5}), ("return_top_tokens 5", {"num_probs": 5}), ("return_top_tokens 32", {"num_probs": 32}))


def chain_main(a):
    dev = "cuda:0"
    vocab, rows = 32000, 1
    g = torch.Generator(device="cpu"); g.manual_seed(0)
    lg = (torch.randn((rows, vocab), generator=g) * 2.5).to(torch.float16).to(dev)
    tok = torch.zeros(rows, dtype=torch.int32, device=dev)
    pr = torch.zeros(rows, dtype=torch.float32, device=dev)
    ws = torch.empty((rows, vocab), dtype=torch.float32, device=dev)
    rounds = sorted(round(timed(lambda: ext_c.sample_rows(lg, 0.8, 50, 0.8, 0.0, 0.37, tok, pr, workspace=ws), reps=200), 2) for _ in range(5))
    res = {"vocab": vocab, "rows": rows, "default_T0.8_k50_p0.8_sample_rows_us": {"min": rounds[0], "median": rounds[2], "max": rounds[4]}}
    if a.default_only:
        print(json.dumps(res), flush=True)
        return
    res["chain_us"] = {}
    for k in (50, 500):
        for name, kw in CHAIN_STAGES:
            kw = dict(kw)
            n_probs = kw.pop("num_probs", 0)
            if kw.get("mirostat"):
                kw["mirostat_mu"] = torch.zeros(rows, dtype=torch.float32, device=dev)
            if n_probs:
                kw["out_ktokens"] = torch.zeros((rows, n_probs), dtype=torch.int32, device=dev)
                kw["out_kprobs"] = torch.zeros((rows, n_probs), dtype=torch.float32, device=dev)
            us = timed(lambda: ext_c.sample_rows_chain(lg, 1.0, k, 0.0, 0.0, 0.37, tok, pr, workspace=ws, **kw), reps=200)
            res["chain_us"][f"k{k} {name}"] = round(us, 2)
        res["chain_us"][f"k{k} sample_rows"] = round(timed(lambda: ext_c.sample_rows(lg, 1.0, k, 0.0, 0.0, 0.37, tok, pr, workspace=ws), reps=200), 2)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chain", action="store_true")
    ap.add_argument("--default-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "sampler_chain.json"))
    a = ap.parse_args()
    if a.chain or a.default_only:
        return chain_main(a)
    dev = "cuda:0"
    g = torch.Generator(device="cpu"); g.manual_seed(0)
    for vocab in (32000, 128256):
        for rows in (1, 16):
            lg = (torch.randn((rows, vocab), generator=g) * 2.5).to(torch.float16).to(dev)
            tok = torch.zeros(rows, dtype=torch.int32, device=dev)
            pr = torch.zeros(rows, dtype=torch.float32, device=dev)
            ws = torch.empty((rows, vocab), dtype=torch.float32, device=dev)
            us_arg = timed(lambda: ext_c.argmax_rows(lg, tok, vocab))
            for name, st in (("default T0.8 k50 p0.8", (0.8, 50, 0.8, 0.0)), ("k500 p0.95 minp0.02", (1.0, 500, 0.95, 0.02)),
                             ("k2", (1.0, 2, 0.0, 0.0))):
                us = timed(lambda: ext_c.sample_rows(lg, st[0], st[1], st[2], st[3], 0.37, tok, pr, workspace=ws))
                print(json.dumps({"vocab": vocab, "rows": rows, "setting": name, "sample_rows_us": round(us, 2),
                                  "argmax_rows_us": round(us_arg, 2), "logits_bytes": rows * vocab * 2}), flush=True)


if __name__ == "__main__":
    main()
