"""Decode rate of LayerNorm models: synthetic aya_23_8b (Cohere: parallel blocks) and starcoder2_7b (sequential blocks), 4.0 bpw, batch 1,
FP16 cache, GreedyGraphDecoder (one captured graph per token, module by module: a LayerNorm model never takes the chained kernels).
aya_23_8b runs in two forms: with the parallel bridge (csrc/layer_norm.hip: the two adds that end a block and the next block's norm into
both copies, one launch) and with the separate launches (EXL2_PARALLEL_BRIDGE=0: add, add, norm, norm).  starcoder2_7b has no bridge;
its rate is recorded once.

Run by hand on an MI355X from the repository root:

    python tools/layernorm_decode_bench.py             # clock ramp, then the two forms INTERLEAVED window by window, median of each

Both decoders of a model live in one process on one model and one cache and alternate, so clock and memory state drift hits both alike.
Writes profiles/layernorm_decode.json (ms per step, tok/s, every window, every form)."""
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

OUT = os.path.join(ROOT, "profiles", "layernorm_decode.json")
STEPS, WARMUP, WINDOWS, RAMP_S = 128, 16, 5, 3.0
TINY = dict(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, head_dim=64, vocab_size=320)


def decoder(model, cache, bridge: bool):
    os.environ["EXL2_PARALLEL_BRIDGE"] = "1" if bridge else "0"
    try:
        dec = GreedyGraphDecoder(model, cache, batch_size=1).capture()
    finally:
        os.environ.pop("EXL2_PARALLEL_BRIDGE", None)
    assert dec.chain is None and dec.parallel_bridge == (bridge and model.config.parallel_decoder_blocks)
    return dec


def window(dec) -> float:
    dec.reset(torch.tensor([1]), 0); dec.run(WARMUP); torch.cuda.synchronize()
    t0 = time.perf_counter(); dec.run(STEPS); torch.cuda.synchronize()
    return time.perf_counter() - t0


def summary(dts):
    dt = sorted(dts)[len(dts) // 2]
    return {"tokens_per_s": round(STEPS / dt, 1), "ms_per_step": round(dt / STEPS * 1e3, 4),
            "windows_tokens_per_s": [round(STEPS / d, 1) for d in dts]}


def measure(name: str, cfg) -> dict:
    model = ExLlamaV2(cfg, device="cuda:0").load(synth_checkpoint(cfg, "cuda:0", recipe="4.0bpw", seed=0))
    cache = ExLlamaV2Cache(model, batch_size=1, max_seq_len=2048)
    forms = {"bridge": True, "separate_launches": False} if cfg.parallel_decoder_blocks else {"module_route": True}
    decs = {k: decoder(model, cache, v) for k, v in forms.items()}
    t = time.perf_counter()
    while time.perf_counter() - t < RAMP_S:
        for d in decs.values():
            d.reset(torch.tensor([1]), 0); d.run(32); torch.cuda.synchronize()
    dts = {k: [] for k in decs}
    for _ in range(WINDOWS):
        for k, d in decs.items():
            dts[k].append(window(d))
    res = {"model": f"{name} 4.0bpw synthetic, bs=1, FP16 cache, module route, graph replay" + (", forms interleaved" if len(decs) > 1 else "")}
    for k in decs:
        res[k] = summary(dts[k])
        decs[k].free()
    if "bridge" in res:
        res["bridge_speedup"] = round(res["bridge"]["tokens_per_s"] / res["separate_launches"]["tokens_per_s"], 4)
    model.unload()
    del model, cache
    torch.cuda.empty_cache()
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--models", default="aya-23-8b,starcoder2-7b", help="comma-separated: aya-23-8b, starcoder2-7b, tiny-cohere, tiny-starcoder2")
    a = p.parse_args()
    kw = dict(max_seq_len=2048, max_input_len=256)
    makers = {"aya-23-8b": lambda: ExLlamaV2Config.aya_23_8b(**kw), "starcoder2-7b": lambda: ExLlamaV2Config.starcoder2_7b(**kw),
              "tiny-cohere": lambda: ExLlamaV2Config._cohere(**(TINY | kw)), "tiny-starcoder2": lambda: ExLlamaV2Config._starcoder2(**(TINY | kw))}
    result = {"steps": STEPS, "warmup": WARMUP, "windows": WINDOWS, "models": {}}
    for name in a.models.split(","):
        result["models"][name] = measure(name, makers[name]())
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    json.dump(result, open(OUT, "w"), indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
