"""Decode rate of Qwen3-MoE blocks: synthetic qwen3_30b_a3b (hidden 2048, 128 experts of width 768, top 8) at 4.0 bpw with --layers N
of its 48 layers (default 8), FP16 cache, GreedyGraphDecoder (one captured graph per token, the block inside the chained step), batch 1
and batch 16.  Two forms of the block: the pair jobs (csrc/modules.hip: logits -> select + hand-out -> gate|up -> down -> combine, five
launches per layer) and the per-expert launch loop (EXL2_MOE_NO_LEAN=1: norm, logits, select, then three launches per expert, 387 per
layer -- the independent route the tests compare against).

Run by hand on an MI355X from the repository root:

    python tools/qwen3_moe_decode_bench.py [--layers 8]      # clock ramp, then the forms INTERLEAVED window by window, median of 5

Both decoders of a batch size live in one process on one model and alternate, so clock and memory state drift hits both alike.
Writes profiles/qwen3_moe_decode.json: tok/s, us per step and layer, the bytes one token streams (model.weight_bytes(): router + 8
experts per layer, attention, head) and the fraction of 8 TB/s that rate is, every window of every form."""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("EXL2_ENV_DYNAMIC", "1")            # (the library's switches are read per call: the two forms are captured in one process)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from exllamav2_amd import ExLlamaV2, ExLlamaV2Cache, ExLlamaV2Config, GreedyGraphDecoder  # noqa: E402
from exllamav2_amd.synth import synth_checkpoint  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "qwen3_moe_decode.json")
STEPS, WARMUP, WINDOWS, RAMP_S = 64, 8, 5, 3.0
HBM_BYTES_PER_S = 8e12


def decoder(model, cache, bs: int, loop: bool):
    if loop: os.environ["EXL2_MOE_NO_LEAN"] = "1"
    try:
        dec = GreedyGraphDecoder(model, cache, batch_size=bs)
        assert dec.chain is not None
        dec.capture()
    finally:
        os.environ.pop("EXL2_MOE_NO_LEAN", None)
    return dec


def window(dec, bs: int) -> float:
    dec.reset(torch.arange(1, bs + 1), 0); dec.run(WARMUP); torch.cuda.synchronize()
    t0 = time.perf_counter(); dec.run(STEPS); torch.cuda.synchronize()
    return time.perf_counter() - t0


def summary(dts, bs: int, layers: int, step_bytes: int):
    dt = sorted(dts)[len(dts) // 2]
    per_step = dt / STEPS
    return {"tokens_per_s": round(bs * STEPS / dt, 1), "us_per_step": round(per_step * 1e6, 2), "us_per_step_and_layer": round(per_step * 1e6 / layers, 2),
            "fraction_of_8TBps_at_one_token_bytes": round(step_bytes / per_step / HBM_BYTES_PER_S, 4),
            "windows_tokens_per_s": [round(bs * STEPS / d, 1) for d in dts],
            "spread": round((max(dts) - min(dts)) / dt, 4)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--layers", type=int, default=8)
    p.add_argument("--batches", default="1,16")
    p.add_argument("--no-loop", action="store_true", help="skip the per-expert loop form")
    a = p.parse_args()
    cfg = ExLlamaV2Config.qwen3_30b_a3b(num_hidden_layers=a.layers, max_seq_len=1024, max_input_len=64, max_batch_size=16)
    model = ExLlamaV2(cfg, device="cuda:0").load(synth_checkpoint(cfg, "cuda:0", recipe="4.0bpw", seed=0))
    step_bytes = int(model.weight_bytes())
    result = {"model": f"qwen3_30b_a3b 4.0bpw synthetic, {a.layers} of 48 layers, FP16 cache, chained step, graph replay, forms interleaved",
              "steps": STEPS, "warmup": WARMUP, "windows": WINDOWS, "layers": a.layers, "weight_bytes_per_token": step_bytes, "batches": {}}
    for bs in [int(b) for b in a.batches.split(",")]:
        cache = ExLlamaV2Cache(model, batch_size=bs, max_seq_len=1024)
        forms = {"pair_jobs": False} if a.no_loop else {"pair_jobs": False, "per_expert_loop": True}
        decs = {k: decoder(model, cache, bs, v) for k, v in forms.items()}
        t = time.perf_counter()
        while time.perf_counter() - t < RAMP_S:
            for d in decs.values():
                d.reset(torch.arange(1, bs + 1), 0); d.run(16); torch.cuda.synchronize()
        dts = {k: [] for k in decs}
        for _ in range(WINDOWS):
            for k, d in decs.items():
                dts[k].append(window(d, bs))
        toks = {k: d.tokens(0, STEPS).cpu().tolist() for k, d in decs.items()}
        res = {k: summary(dts[k], bs, a.layers, step_bytes) for k in decs}
        if len(decs) > 1:
            res["same_tokens"] = toks["pair_jobs"] == toks["per_expert_loop"]
            res["speedup_over_loop"] = round(res["pair_jobs"]["tokens_per_s"] / res["per_expert_loop"]["tokens_per_s"], 3)
        for d in decs.values(): d.free()
        result["batches"][str(bs)] = res
        del cache
    model.unload()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    json.dump(result, open(OUT, "w"), indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
