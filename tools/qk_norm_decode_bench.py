#!/usr/bin/env python3
"""Greedy decode rate of a synthetic Qwen3-8B (q / k head norm) at 4.0 bpw, bs = 1, FP16 cache, on GreedyGraphDecoder (chained step,
one HIP graph per token) in the two forms of the head norm:

    fused     the norm inside the one-launch decode attention (csrc/attn_fused_body.h, NORM) -- EXL2_QK_NORM_FUSED=1
    separate  a launch of its own behind the q | k | v projections (csrc/head_norm.hip)       -- EXL2_QK_NORM_FUSED=0

Two windows (empty cache, 1920 tokens cached); the forms are interleaved over `--rounds` rounds, medians reported.  Then both forms
decode from the same 1920-token prompt and their logits and tokens are compared (the two forms share one device function for the norm:
they must agree bit for bit).

    python tools/qk_norm_decode_bench.py [--rounds 5] [--steps 128] [--out profiles/qk_norm_decode.json] [--vocab N] [--layers N]

--vocab / --layers shrink the model (a width a kernel does not cover yet, a smaller card); the output says so.
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

from exllamav2_amd import ExLlamaV2, ExLlamaV2Cache, ExLlamaV2Config, GreedyGraphDecoder  # noqa: E402
from exllamav2_amd.synth import synth_checkpoint  # noqa: E402

FORMS = ["fused", "separate"]
WINDOWS = (0, 1920)


def set_form(model, form):
    for attn, _ in model.layers:
        attn.qk_norm_fused = form == "fused"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--vocab", type=int, default=0)
    ap.add_argument("--layers", type=int, default=0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = "cuda:0"
    torch.cuda.set_device(dev)
    max_seq = 2048
    over = {}
    if a.vocab: over["vocab_size"] = a.vocab
    if a.layers: over["num_hidden_layers"] = a.layers
    cfg = ExLlamaV2Config.qwen3_8b(max_seq_len=max_seq, max_input_len=256, **over)
    if over:
        print(json.dumps({"note": "NOT the full qwen3_8b preset", "overrides": over}), flush=True)
    model = ExLlamaV2(cfg, device=dev).load(synth_checkpoint(cfg, dev, recipe="4.0bpw", seed=0))
    torch.cuda.synchronize()
    rates = {f: {w: [] for w in WINDOWS} for f in FORMS}
    chained = {}
    for rnd in range(a.rounds):
        for form in (FORMS if rnd % 2 == 0 else FORMS[::-1]):          # neither form always runs first in a round
            set_form(model, form)
            cache = ExLlamaV2Cache(model, batch_size=1, max_seq_len=max_seq)
            dec = GreedyGraphDecoder(model, cache, batch_size=1).capture()
            chained[form] = dec.chain is not None
            if rnd == 0 and not rates[FORMS[0]][0] and not rates[FORMS[1]][0]:      # clock ramp before the first timed window
                t = time.perf_counter()
                while time.perf_counter() - t < 4.0:
                    dec.reset(torch.tensor([1]), 0); dec.run(64); torch.cuda.synchronize()
            for ctx in WINDOWS:
                dec.reset(torch.tensor([1]), ctx)
                dec.run(a.warmup); torch.cuda.synchronize()
                t0 = time.perf_counter()
                dec.run(a.steps); torch.cuda.synchronize()
                rates[form][ctx].append(a.steps / (time.perf_counter() - t0))
            dec.free()
            del dec, cache
            print(json.dumps({"round": rnd, "form": form, "tok_s_empty": round(rates[form][0][-1], 1),
                              "tok_s_ctx1920": round(rates[form][1920][-1], 1)}), flush=True)
    # ---- outputs at the timed size: both forms from the same 1920-token prompt ------------------------------------------------------
    ids = torch.from_numpy(np.random.default_rng(0).integers(0, cfg.vocab_size, size=(1, 1920)))
    logits, toks = {}, {}
    for form in FORMS:
        set_form(model, form)
        cache = ExLlamaV2Cache(model, batch_size=1, max_seq_len=max_seq)
        model.forward(ids, cache, preprocess_only=True)
        dec = GreedyGraphDecoder(model, cache, batch_size=1).capture()
        dec.reset(torch.tensor([1]), 1920)
        dec.run(1); torch.cuda.synchronize()
        logits[form] = dec.logits[:, :cfg.vocab_size].cpu().numpy().copy()
        dec.run(7); torch.cuda.synchronize()
        toks[form] = dec.tokens(1920, 8).cpu().numpy().tolist()[0]
        dec.free()
        del dec, cache
    same = bool(np.array_equal(logits["fused"].view(np.uint16), logits["separate"].view(np.uint16))) and toks["fused"] == toks["separate"]
    set_form(model, "fused")
    med = {f: {w: statistics.median(rates[f][w]) for w in WINDOWS} for f in FORMS}
    result = {"model": "qwen3_8b (synthetic)", "overrides": over, "recipe": "4.0bpw", "batch": 1, "cache": "fp16", "steps": a.steps, "warmup": a.warmup,
              "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"),
              "forms": [{"form": f, "chained": chained[f], "tok_s_empty": round(med[f][0], 1), "tok_s_ctx1920": round(med[f][1920], 1),
                         "all_empty": [round(x, 1) for x in rates[f][0]], "all_ctx1920": [round(x, 1) for x in rates[f][1920]]} for f in FORMS],
              "outputs_at_ctx1920": {"logits_and_tokens_bit_identical": same, "tokens": toks["fused"]},
              "faster_form": {str(w): max(FORMS, key=lambda f: med[f][w]) for w in WINDOWS}}
    print(json.dumps(result), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")
    model.unload()
    sys.exit(0 if same and all(chained.values()) else 3)          # (3: ran to the end, the forms differ or a step was not chained)


if __name__ == "__main__":
    main()
