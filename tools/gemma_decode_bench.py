"""Decode rate of a Gemma-2 model: synthetic gemma2_9b 4.0 bpw, batch 1, FP16 cache, GreedyGraphDecoder (one captured graph per token,
module by module: an fp32 residual stream never takes the chained kernels) with the norm bridge (csrc/gemma_ops.hip: one launch for the
two norms at every module boundary) and with the handles' own two launches (EXL2_NORM_BRIDGE=0).

Run by hand on an MI355X from the repository root:

    python tools/gemma_decode_bench.py                 # clock ramp, then the two forms INTERLEAVED window by window, median of each

Both decoders live in one process on one model and one cache and alternate, so clock and memory state drift hits both alike.  Writes
profiles/gemma_decode.json (ms per step, tok/s, every window, both forms)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from exllamav2_amd import ExLlamaV2, ExLlamaV2Cache, ExLlamaV2Config, GreedyGraphDecoder  # noqa: E402
from exllamav2_amd.synth import synth_checkpoint  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "gemma_decode.json")
STEPS, WARMUP, WINDOWS, RAMP_S = 128, 16, 7, 4.0


def decoder(model, cache, bridge: bool):
    os.environ["EXL2_NORM_BRIDGE"] = "1" if bridge else "0"
    try:
        dec = GreedyGraphDecoder(model, cache, batch_size=1).capture()
    finally:
        os.environ.pop("EXL2_NORM_BRIDGE", None)
    assert dec.chain is None and dec.norm_bridge == bridge
    return dec


def window(dec) -> float:
    dec.reset(torch.tensor([1]), 0); dec.run(WARMUP); torch.cuda.synchronize()
    t0 = time.perf_counter(); dec.run(STEPS); torch.cuda.synchronize()
    return time.perf_counter() - t0


def summary(dts):
    dt = sorted(dts)[len(dts) // 2]
    return {"tokens_per_s": round(STEPS / dt, 1), "ms_per_step": round(dt / STEPS * 1e3, 4),
            "windows_tokens_per_s": [round(STEPS / d, 1) for d in dts]}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--model", default="gemma2-9b", choices=["gemma2-9b", "gemma2-2b", "tiny"])
    a = p.parse_args()
    kw = dict(max_seq_len=2048, max_input_len=256)
    if a.model == "tiny":
        cfg = ExLlamaV2Config._gemma2(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                                      head_dim=64, vocab_size=320, query_pre_attn_scalar=64.0, **kw)
    else:
        cfg = (ExLlamaV2Config.gemma2_9b if a.model == "gemma2-9b" else ExLlamaV2Config.gemma2_2b)(**kw)
    model = ExLlamaV2(cfg, device="cuda:0").load(synth_checkpoint(cfg, "cuda:0", recipe="4.0bpw", seed=0))
    cache = ExLlamaV2Cache(model, batch_size=1, max_seq_len=2048)
    decs = {"bridge": decoder(model, cache, True), "two_launch_norms": decoder(model, cache, False)}
    t = time.perf_counter()
    while time.perf_counter() - t < RAMP_S:
        for d in decs.values():
            d.reset(torch.tensor([1]), 0); d.run(32); torch.cuda.synchronize()
    dts = {k: [] for k in decs}
    for _ in range(WINDOWS):
        for k, d in decs.items():
            dts[k].append(window(d))
    result = {"model": f"{a.model} 4.0bpw synthetic, bs=1, FP16 cache, module route, graph replay, forms interleaved",
              "steps": STEPS, "warmup": WARMUP, "windows": WINDOWS}
    for k in decs:
        result[k] = summary(dts[k])
        decs[k].free()
    result["bridge_speedup"] = round(result["bridge"]["tokens_per_s"] / result["two_launch_norms"]["tokens_per_s"], 4)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    json.dump(result, open(OUT, "w"), indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
