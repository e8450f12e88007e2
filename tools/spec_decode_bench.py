#!/usr/bin/env python3
"""Speculative greedy decoding (exllamav2_amd/speculative.py) against the plain GreedyGraphDecoder on the synthetic Llama-2-7B at
4.0 bpw that bench.py builds, batch 1, FP16 cache, empty context, everything in one process:

    plain        one graph launch per token
    forced       K in {1, 3, 7} drafts per step = the tokens a plain run recorded, each made wrong with probability 1 - a (seeded
                 Bernoulli per draft) for a in {0, 0.5, 0.8, 1.0}: the cost of a verify step and what it buys at a known acceptance
    ngram        the device's n-gram drafter on the same continuation

The configurations are interleaved over `--rounds` rounds (the order alternates), the median window is reported.  A window = the
steps that consume the recorded continuation once, repeated until it holds >= `--min-steps` steps; only the steps between two device
synchronisations are timed (the reset in front of each repeat is not).  Per configuration: ms per verify step, its ratio to the plain
step, tokens per step (from the device's counters), tokens/s.  Break-even: a step pays when it accepts more than (ratio - 1) drafts.

    python tools/spec_decode_bench.py [--rounds 5] [--tokens 256] [--out profiles/spec_decode.json] [--vocab N] [--layers N]

--vocab / --layers shrink the model (rehearsals); the output says so.  Exit status 3: ran to the end but K = 3 at full acceptance did
not beat the plain decoder, or a verify step left the chained kernels.
"""
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
from exllamav2_amd.synth import synth_checkpoint  # noqa: E402

KS = (1, 3, 7)
ACCEPT = (0.0, 0.5, 0.8, 1.0)
FIRST = 1                                   # the one-token prompt (bench.py starts its windows from it too)


def corrupt(seq, K, accept, vocab, seed):
    """forced tokens by sequence index: `seq` with every draft the decoder will make wrong with probability 1 - accept.  Returns
    (forced, steps that stay inside the recorded tokens)."""
    rng = np.random.default_rng(seed)
    forced = np.array(seq, dtype=np.int64)
    L, steps = 1, 0
    while L + K < len(forced):
        ok = rng.random(K) < accept
        n_acc = K if ok.all() else int(np.argmin(ok))
        if n_acc < K:
            forced[L + n_acc] = (forced[L + n_acc] + 1) % vocab
        L += n_acc + 1
        steps += 1
    return forced, steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--tokens", type=int, default=256)
    ap.add_argument("--min-steps", type=int, default=128)
    ap.add_argument("--vocab", type=int, default=0)
    ap.add_argument("--layers", type=int, default=0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = "cuda:0"
    torch.cuda.set_device(dev)
    max_seq = 4096                          # zero acceptance at K = 7: tokens x 8 rows of pessimistic bound
    over = {}
    if a.vocab: over["vocab_size"] = a.vocab
    if a.layers: over["num_hidden_layers"] = a.layers
    cfg = ExLlamaV2Config.llama2_7b(max_seq_len=max_seq, max_input_len=256, **over)
    if over:
        print(json.dumps({"note": "NOT the full llama2_7b preset", "overrides": over}), flush=True)
    model = ExLlamaV2(cfg, device=dev).load(synth_checkpoint(cfg, dev, recipe="4.0bpw", seed=0))
    ext = model.ext
    torch.cuda.synchronize()

    # ---- the continuation every configuration decodes: a plain run from the one-token prompt ---------------------------------------
    plain = GreedyGraphDecoder(model, ExLlamaV2Cache(model, batch_size=1, max_seq_len=max_seq), batch_size=1).capture()
    t = time.perf_counter()
    while time.perf_counter() - t < 4.0:    # clock ramp
        plain.reset(torch.tensor([FIRST]), 0); plain.run(64); torch.cuda.synchronize()
    plain.reset(torch.tensor([FIRST]), 0)
    plain.run(a.tokens); torch.cuda.synchronize()
    recorded = plain.tokens(0, a.tokens).cpu().numpy()[0].astype(np.int64)
    seq = np.concatenate([[FIRST], recorded])

    # ---- configurations: name -> (decoder, prepare(), steps per repeat) --------------------------------------------------------------
    prompt = torch.tensor([FIRST])
    configs, info = {}, {}

    def add_plain():
        def reset(): plain.reset(prompt, 0)
        configs["plain"] = (plain, reset, a.tokens)
        info["plain"] = {"drafter": None, "K": 0, "chained": plain.chain is not None}

    add_plain()
    for K in KS:
        dec = SpeculativeGraphDecoder(model, ExLlamaV2Cache(model, batch_size=1, max_seq_len=max_seq), num_draft_tokens=K,
                                      drafter="forced", forced=torch.from_numpy(seq)).capture()
        ext.chain_route_counts(reset=True)
        dec.reset(prompt); dec.run(1, use_graph=False); dec.sync()
        lean, flat = ext.chain_route_counts(reset=True)
        route = {"chained": dec.chain is not None, "lean_launches_per_step": lean, "flat_launches_per_step": flat,
                 "regrouped": {str(k): v for k, v in (dec.chain or {}).get("group_override", {}).items()}}
        for acc in ACCEPT:
            forced, steps = corrupt(seq, K, acc, cfg.vocab_size, seed=1000 * K + int(acc * 100))
            ft = torch.from_numpy(forced)
            def reset(dec=dec, ft=ft): dec.set_forced(ft); dec.reset(prompt)
            name = f"forced K={K} a={acc}"
            configs[name] = (dec, reset, steps)
            info[name] = {"drafter": "forced", "K": K, "accept_probability": acc, **route}
        ng = SpeculativeGraphDecoder(model, ExLlamaV2Cache(model, batch_size=1, max_seq_len=max_seq), num_draft_tokens=K, max_ngram=4).capture()
        ng.reset(prompt)
        out = ng.generate(a.tokens).cpu().numpy().astype(np.int64)
        same = int(np.argmin(out == recorded)) if not np.array_equal(out, recorded) else a.tokens
        def reset(ng=ng): ng.reset(prompt)
        name = f"ngram K={K}"
        configs[name] = (ng, reset, ng.stats()["steps"])
        info[name] = {"drafter": "ngram", "K": K, "max_ngram": 4, "tokens_equal_to_plain_run": same, **route}

    # ---- timed windows, interleaved ----------------------------------------------------------------------------------------------
    step_s = {n: [] for n in configs}
    tok_step = {}

    def window(name, timed=True):
        dec, reset, steps = configs[name]
        reps = max(1, -(-a.min_steps // steps))
        total = 0.0
        for _ in range(reps):
            reset(); torch.cuda.synchronize()
            t0 = time.perf_counter()
            dec.run(steps); torch.cuda.synchronize()
            total += time.perf_counter() - t0
        if timed:
            step_s[name].append(total / (reps * steps))
        if name != "plain":
            st = dec.stats()
            assert st["steps"] == steps, (name, st, steps)
            tok_step[name] = st["tokens_per_step"]
            got = dec.tokens(0, min(st["emitted"], a.tokens)).cpu().numpy().astype(np.int64)
            n = len(got)
            info[name]["tokens_equal_to_plain_run"] = int(np.argmin(got == recorded[:n])) if not np.array_equal(got, recorded[:n]) else n
            info[name]["tokens_emitted_per_repeat"] = st["emitted"]
            info[name]["accept_histogram"] = st["hist"]

    names = list(configs)
    for n in names:
        window(n, timed=False)              # every shape once, untimed
    for rnd in range(a.rounds):
        for n in (names if rnd % 2 == 0 else names[::-1]):
            window(n)
        print(json.dumps({"round": rnd, "ms_per_step": {n: round(1e3 * step_s[n][-1], 4) for n in names}}), flush=True)

    med = {n: statistics.median(step_s[n]) for n in names}
    rows = []
    for n in names:
        tps = 1.0 if n == "plain" else tok_step[n]
        rows.append({"config": n, **info[n], "steps_per_repeat": configs[n][2], "ms_per_step": round(1e3 * med[n], 4),
                     "ratio_to_plain_step": round(med[n] / med["plain"], 4), "tokens_per_step": round(tps, 4),
                     "tok_s": round(tps / med[n], 1), "speedup": round(tps / med[n] * med["plain"], 4),
                     "all_ms_per_step": [round(1e3 * x, 4) for x in step_s[n]]})
    full3 = next(r for r in rows if r["config"] == "forced K=3 a=1.0")
    result = {"model": "llama2_7b (synthetic)", "overrides": over, "recipe": "4.0bpw", "batch": 1, "cache": "fp16", "context": 0,
              "recorded_tokens": a.tokens, "rounds": a.rounds, "min_steps_per_window": a.min_steps,
              "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"),
              "plain_tok_s": round(1.0 / med["plain"], 1), "rows": rows,
              "break_even_accepted_drafts_per_step": {str(K): round(next(r for r in rows if r["config"] == f"forced K={K} a=0.0")["ratio_to_plain_step"] - 1.0, 4) for K in KS},
              "k3_full_acceptance_beats_plain": bool(full3["speedup"] > 1.0)}
    print(json.dumps(result), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")
    chained = all(r.get("chained", True) for r in rows)
    for dec, _, _ in configs.values():
        dec.free()
    model.unload()
    sys.exit(0 if result["k3_full_acceptance_beats_plain"] and chained else 3)


if __name__ == "__main__":
    main()
