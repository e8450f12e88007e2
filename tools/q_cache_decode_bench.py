#!/usr/bin/env python3
"""Greedy decode rate of Llama-2-7B 4.0bpw, bs = 1, on GreedyGraphDecoder per KV-cache type: fp16 | q4 | q6 | q8 on the default route
(chained step, one HIP graph per token; quantized caches attend straight from their codes) and each quantized type on the UNPACK route
(EXL2_Q4_FUSED=0, EXL2_CHAIN=0: q_to_fp16_kv of the live range + fp16 attention + fp16_to_q_kv per layer and step -- the only route a
Q6 / Q8 cache had before csrc/attn_q4.hip took 8-bit codes).  Two windows: empty cache and 1920 tokens cached.  Variants are
interleaved over `--rounds` rounds, medians reported.  Then, per quantized type, both routes decode from the SAME 1920-token prompt and
their logits are compared at the model tolerance (0.03 + |x| 2^-8: tests/test_model.py).

    python tools/q_cache_decode_bench.py [--rounds 3] [--steps 64] [--out profiles/q68_decode.json] [--model llama2-7b|tiny]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from exllamav2_amd import ExLlamaV2, ExLlamaV2Config, GreedyGraphDecoder  # noqa: E402
from exllamav2_amd.cache import cache_class  # noqa: E402
from exllamav2_amd.synth import synth_checkpoint  # noqa: E402

VARIANTS = [("fp16", "default"), ("q4", "default"), ("q6", "default"), ("q8", "default"), ("q4", "unpack"), ("q6", "unpack"), ("q8", "unpack")]


def set_route(model, route):
    for attn, _ in model.layers:
        attn.q4_fused = route != "unpack"
    os.environ["EXL2_CHAIN"] = "0" if route == "unpack" else "1"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--model", default="llama2-7b")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = "cuda:0"
    torch.cuda.set_device(dev)
    max_seq = 2048
    cfg = ExLlamaV2Config.llama2_7b(max_seq_len=max_seq, max_input_len=256) if a.model == "llama2-7b" else ExLlamaV2Config.tiny_test(max_seq_len=max_seq)
    model = ExLlamaV2(cfg, device=dev).load(synth_checkpoint(cfg, dev, recipe="4.0bpw", seed=0))
    torch.cuda.synchronize()
    rates = {v: {0: [], 1920: []} for v in VARIANTS}
    chained = {}
    for rnd in range(a.rounds):
        for v in VARIANTS:
            cache_type, route = v
            set_route(model, route)
            cache = cache_class(cache_type)(model, batch_size=1, max_seq_len=max_seq)
            dec = GreedyGraphDecoder(model, cache, batch_size=1).capture()
            chained[v] = dec.chain is not None
            if rnd == 0 and v == VARIANTS[0]:                          # clock ramp before the first timed window
                t = time.perf_counter()
                while time.perf_counter() - t < 4.0:
                    dec.reset(torch.tensor([1]), 0); dec.run(64); torch.cuda.synchronize()
            for ctx in (0, 1920):
                dec.reset(torch.tensor([1]), ctx)
                dec.run(a.warmup); torch.cuda.synchronize()
                t0 = time.perf_counter()
                dec.run(a.steps); torch.cuda.synchronize()
                rates[v][ctx].append(a.steps / (time.perf_counter() - t0))
            dec.free()
            del dec, cache
            print(json.dumps({"round": rnd, "cache": cache_type, "route": route, "tok_s_empty": round(rates[v][0][-1], 1),
                              "tok_s_ctx1920": round(rates[v][1920][-1], 1)}), flush=True)
    # ---- outputs at the timed size: both routes from the same 1920-token prompt ---------------------------------------------------
    ids = torch.from_numpy(__import__("numpy").random.default_rng(0).integers(0, cfg.vocab_size, size=(1, 1920)))
    compare = {}
    for cache_type in ("q4", "q6", "q8"):
        logits, toks = {}, {}
        for route in ("default", "unpack"):
            set_route(model, route)
            cache = cache_class(cache_type)(model, batch_size=1, max_seq_len=max_seq)
            for attn, _ in model.layers:
                attn.q4_fused = False                                  # (the prompt goes in by the same kernels on both sides)
            model.forward(ids, cache, preprocess_only=True)
            set_route(model, route)
            dec = GreedyGraphDecoder(model, cache, batch_size=1).capture()
            dec.reset(torch.tensor([1]), 1920)
            dec.run(1); torch.cuda.synchronize()
            logits[route] = dec.logits[:, :cfg.vocab_size].float().cpu().double().numpy()
            dec.run(7); torch.cuda.synchronize()
            toks[route] = dec.tokens(1920, 8).cpu().numpy().tolist()
            dec.free()
            del dec, cache
        want, got = logits["unpack"], logits["default"]
        rel = float((abs(got - want) / (0.03 + abs(want) * 2.0 ** -8)).max())
        compare[cache_type] = {"first_step_worst_logit_error_over_model_tolerance": round(rel, 4), "within_tolerance": rel <= 1.0,
                               "tokens_default": toks["default"][0], "tokens_unpack": toks["unpack"][0]}
        print(json.dumps({"cache": cache_type, **compare[cache_type]}), flush=True)
    set_route(model, "default")
    result = {"model": a.model, "recipe": "4.0bpw", "batch": 1, "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds,
              "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "variants": [], "outputs_at_ctx1920": compare}
    med = {}
    for v in VARIANTS:
        med[v] = {ctx: statistics.median(rates[v][ctx]) for ctx in (0, 1920)}
        result["variants"].append({"cache": v[0], "route": v[1], "chained": chained[v], "tok_s_empty": round(med[v][0], 1),
                                   "tok_s_ctx1920": round(med[v][1920], 1),
                                   "all_empty": [round(x, 1) for x in rates[v][0]], "all_ctx1920": [round(x, 1) for x in rates[v][1920]]})
    ok = all(med[(c, "default")][ctx] >= med[(c, "unpack")][ctx] for c in ("q6", "q8") for ctx in (0, 1920))
    ok = ok and all(compare[c]["within_tolerance"] for c in ("q6", "q8"))
    result["required_relations_hold"] = ok
    print(json.dumps(result), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")
    model.unload()
    sys.exit(0 if ok else 3)                                      # (3: ran to the end, a required relation does not hold)


if __name__ == "__main__":
    main()
