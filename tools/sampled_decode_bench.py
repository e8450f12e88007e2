#!/usr/bin/env python3
"""Sampled decoding with the reference's penalties on the device (csrc/penalties.hip), measured on an MI355X in one process:

  kernels   exl2_apply_penalties alone, microseconds per launch from HIP events on the launching stream (100 launches after 10
            warm-up ones, the method of tools/sampler_bench.py), fp16 logits of 32000 and 151936 entries, windows of 128 / 1920 /
            4096 tokens, the reference's default settings and (1.2, 1024, 1024, 0.1, 0.1), ids all different and text-like (300
            distinct ids) -- next to the sample_rows launch on the same logits in the same run, which is the yardstick.
  decode    the synthetic Llama-2-7B at 4.0 bpw that bench.py builds, batch 1, FP16 cache: greedy, sampled without penalties,
            sampled with the default penalty, at 128 / 1920 / ~4000 cached tokens; speculative K = 3 greedy and sampled (default
            penalty) with forced drafts at full and zero acceptance and with the n-gram drafter.  Configurations are interleaved over
            `--rounds` rounds (order alternating); per configuration the median window and the spread of its windows.

    python tools/sampled_decode_bench.py [--rounds 5] [--out profiles/sampled_penalties.json] [--vocab N] [--layers N] [--skip-decode]

--vocab / --layers shrink the model (rehearsals); the output says so."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from exllamav2_amd import ExLlamaV2, ExLlamaV2Cache, ExLlamaV2Config, GreedyGraphDecoder, SpeculativeGraphDecoder  # noqa: E402
from exllamav2_amd.ext import ext_c  # noqa: E402
from exllamav2_amd.synth import synth_checkpoint  # noqa: E402

DEFAULT = (0.8, 50, 0.8, 0.0)
DEFAULT_PEN = dict(token_repetition_penalty=1.025, token_repetition_range=-1)
K = 3


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


def kernel_rows(dev):
    rows = []
    rng = np.random.default_rng(0)
    for vocab in (32000, 151936):
        lg = torch.from_numpy((rng.standard_normal((1, vocab)) * 2.5).astype(np.float16)).to(dev)
        out = lg.to(torch.float32)
        tok = torch.zeros(1, dtype=torch.int32, device=dev); pr = torch.zeros(1, dtype=torch.float32, device=dev)
        ws = torch.empty((1, vocab), dtype=torch.float32, device=dev)
        us_sample = timed(lambda: ext_c.sample_rows(lg, *DEFAULT, 0.37, tok, pr, workspace=ws))
        us_sample32 = timed(lambda: ext_c.sample_rows(out, *DEFAULT, 0.37, tok, pr, workspace=ws))
        for window in (128, 1920, 4096):
            for ids_name, ids in (("all different", rng.permutation(vocab)[:window]), ("text-like, 300 distinct", rng.integers(0, 300, size=window) * 101 % vocab)):
                hist = torch.from_numpy(ids.astype(np.int32)[None]).to(dev).contiguous()
                pos = torch.tensor([window - 1], dtype=torch.int32, device=dev)
                for st_name, st in (("default 1.025 whole context", (1.025, -1, 0, 0.0, 0.0)), ("1.2 / 1024 / 1024 / 0.1 / 0.1", (1.2, 1024, 1024, 0.1, 0.1))):
                    ramps = ext_c.penalty_ramps(st[0], st[2], st[3], st[4])
                    ramps = None if ramps is None else ramps.to(dev)
                    us = timed(lambda: ext_c.apply_penalties(lg, out, hist, pos, *st, ramps=ramps))
                    rows.append({"vocab": vocab, "window": window, "ids": ids_name, "settings": st_name, "apply_penalties_us": round(us, 2),
                                 "sample_rows_fp16_us": round(us_sample, 2), "sample_rows_fp32_us": round(us_sample32, 2),
                                 "below_the_sampler": bool(us < us_sample)})
                    print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--tokens", type=int, default=64)
    ap.add_argument("--vocab", type=int, default=0)
    ap.add_argument("--layers", type=int, default=0)
    ap.add_argument("--skip-decode", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = "cuda:0"
    torch.cuda.set_device(dev)
    result = {"device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "kernels": kernel_rows(dev)}
    if not a.skip_decode:
        result["decode"] = decode_rows(a, dev)
    print(json.dumps(result), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


def decode_rows(a, dev):
    max_seq = 4096
    over = {}
    if a.vocab: over["vocab_size"] = a.vocab
    if a.layers: over["num_hidden_layers"] = a.layers
    cfg = ExLlamaV2Config.llama2_7b(max_seq_len=max_seq, max_input_len=256, **over)
    model = ExLlamaV2(cfg, device=dev).load(synth_checkpoint(cfg, dev, recipe="4.0bpw", seed=0))
    torch.cuda.synchronize()
    n = a.tokens
    rng = np.random.default_rng(1)
    text = torch.from_numpy((rng.integers(0, 300, size=(1, max_seq)) * 101 % cfg.vocab_size).astype(np.int64))     # text-like context
    rnds = [float(x) for x in rng.random(4 * n).astype(np.float32)]

    plain = GreedyGraphDecoder(model, ExLlamaV2Cache(model, batch_size=1, max_seq_len=max_seq), batch_size=1).capture()
    nopen = GreedyGraphDecoder(model, ExLlamaV2Cache(model, batch_size=1, max_seq_len=max_seq), batch_size=1).capture_sampled(*DEFAULT)
    pen = GreedyGraphDecoder(model, ExLlamaV2Cache(model, batch_size=1, max_seq_len=max_seq), batch_size=1).capture_sampled(*DEFAULT, **DEFAULT_PEN)
    t = time.perf_counter()
    while time.perf_counter() - t < 4.0:        # clock ramp
        plain.reset(torch.tensor([1]), 0); plain.run(64); torch.cuda.synchronize()

    configs = {}                                 # name -> (prepare(), run() -> tokens emitted)

    def add_plain(name, dec, ctx, how):
        def prep(): dec.reset(text[:, ctx], ctx, prompt_ids=text[:, :ctx + 1])
        def run():
            if how == "greedy": dec.run(n)
            elif how == "nopen": dec.run_sampled(n, *DEFAULT, randoms=rnds)
            else: dec.run_sampled(n, *DEFAULT, randoms=rnds, **DEFAULT_PEN)
            return n
        configs[name] = (prep, run, dec)

    for ctx in (128, 1920, max_seq - n - 32):
        add_plain(f"greedy ctx={ctx}", plain, ctx, "greedy")
        add_plain(f"sampled no penalties ctx={ctx}", nopen, ctx, "nopen")
        add_plain(f"sampled default penalty ctx={ctx}", pen, ctx, "pen")

    # forced drafts: the continuation a decoder emits is recorded by THAT decoder's own graph (the emitted tokens do not depend on the
    # drafts), then handed to it as its drafts -- right as recorded, or every one of them made wrong
    ctx = 128
    prompt = text[0, :ctx + 1]
    steps_full, steps_zero = (4 * n - K) // (K + 1), n

    def spec(name, drafter, accept, sampled, steps):
        cache = ExLlamaV2Cache(model, batch_size=1, max_seq_len=max_seq)
        model.forward(prompt[None, :-1], cache, preprocess_only=True)
        if drafter == "forced":
            dec = SpeculativeGraphDecoder(model, cache, num_draft_tokens=K, drafter="forced", forced=torch.zeros(ctx + 1 + 4 * n, dtype=torch.int64))
        else:
            dec = SpeculativeGraphDecoder(model, cache, num_draft_tokens=K, max_ngram=4)
        dec.capture()
        if sampled:
            dec.capture_sampled(*DEFAULT, **DEFAULT_PEN)
        if drafter == "forced":
            dec.reset(prompt)
            if sampled: dec.run_sampled(4 * n, *DEFAULT, randoms=rnds * 4, **DEFAULT_PEN)
            else: dec.run(4 * n)
            assert dec.sync() - ctx >= 4 * n
            rec = dec.history[:ctx + 1 + 4 * n].cpu().to(torch.int64)
            if not accept:
                rec[ctx + 1:] = (rec[ctx + 1:] + 1) % cfg.vocab_size
            dec.set_forced(rec)
        def prep(): dec.reset(prompt)
        def run():
            if sampled: dec.run_sampled(steps, *DEFAULT, randoms=rnds + rnds, **DEFAULT_PEN)
            else: dec.run(steps)
            return None                          # emitted tokens: the device's counters
        configs[name] = (prep, run, dec)

    spec("spec greedy K=3 forced a=1.0", "forced", True, False, steps_full)
    spec("spec greedy K=3 forced a=0.0", "forced", False, False, steps_zero)
    spec("spec greedy K=3 ngram", "ngram", None, False, steps_zero)
    spec("spec sampled K=3 forced a=1.0", "forced", True, True, steps_full)
    spec("spec sampled K=3 forced a=0.0", "forced", False, True, steps_zero)
    spec("spec sampled K=3 ngram", "ngram", None, True, steps_zero)

    tok_s = {name: [] for name in configs}
    extra = {}

    def window(name, timed_=True):
        prep, run, dec = configs[name]
        prep(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        emitted = run(); torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if emitted is None:
            st = dec.stats()
            emitted = st["emitted"]
            extra[name] = {"steps": st["steps"], "tokens_per_step": round(st["tokens_per_step"], 4), "accept_histogram": st["hist"],
                           "ms_per_step": round(1e3 * dt / st["steps"], 4)}
        if timed_:
            tok_s[name].append(emitted / dt)

    names = list(configs)
    for name in names:
        window(name, timed_=False)
    for rnd in range(a.rounds):
        for name in (names if rnd % 2 == 0 else names[::-1]):
            window(name)
        print(json.dumps({"round": rnd, "tok_s": {k: round(v[-1], 1) for k, v in tok_s.items()}}), flush=True)
    rows = []
    for name in names:
        v = tok_s[name]
        rows.append({"config": name, "tok_s": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1),
                     "ms_per_token": round(1e3 / statistics.median(v), 4), **extra.get(name, {})})
    for _, _, dec in configs.values():
        dec.free()
    model.unload()
    return {"model": "llama2_7b (synthetic)", "overrides": over, "recipe": "4.0bpw", "batch": 1, "cache": "fp16", "tokens_per_window": n,
            "rounds": a.rounds, "rows": rows}


if __name__ == "__main__":
    main()
