"""Decode rate with LoRA adapters: synthetic Llama-2-7B 4.0 bpw, batch 1, GreedyGraphDecoder on the module-by-module route
(EXL2_CHAIN=0) without an adapter, with one rank-16 and with one rank-64 adapter on all seven projections.

Run by hand on an MI355X from the repository root:

    python tools/lora_bench.py                     # rates: clock ramp, then the median of five windows (as bench.py times its windows)
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/lora_bench.py --trace-run 64     # the launches' own time, a run of its own

The first form writes profiles/lora_decode.json; `--stats-csv <kernel_stats.csv>` folds the per-kernel totals of a trace run into it
(time of lora_down_kernel / lora_up_kernel and the launches per token and layer)."""
import argparse
import csv
import json
import os
import sys
import time

os.environ.setdefault("EXL2_CHAIN", "0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from exllamav2_amd import ExLlamaV2, ExLlamaV2Cache, ExLlamaV2Config, GreedyGraphDecoder  # noqa: E402
from exllamav2_amd.synth import synth_checkpoint  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "lora_decode.json")
STEPS, WARMUP, WINDOWS, RAMP_S = 128, 16, 5, 4.0


class SynthLora:
    """an adapter attached directly (no file): A [in, r], B [r, out] fp16 on every dense projection"""

    def __init__(self, model, rank: int, seed: int):
        g = torch.Generator(device="cpu").manual_seed(seed)
        self.rank, self.linears = rank, list(model.linear_modules().values())
        for lin in self.linears:
            a = (torch.randn((lin.in_features, rank), generator=g) / lin.in_features ** 0.5).half().to(model.device)
            b = (0.05 * torch.randn((rank, lin.out_features), generator=g) / rank ** 0.5).half().to(model.device)
            lin.lora_a_tensors[self], lin.lora_b_tensors[self] = a, b
        model.update_loras()

    def detach(self, model):
        for lin in self.linears:
            lin.lora_a_tensors.pop(self, None); lin.lora_b_tensors.pop(self, None)
        model.update_loras()


def rate(model, cache, loras):
    dec = GreedyGraphDecoder(model, cache, batch_size=1, loras=loras).capture()
    assert dec.chain is None
    t = time.perf_counter()
    while time.perf_counter() - t < RAMP_S:
        dec.reset(torch.tensor([1]), 0); dec.run(64); torch.cuda.synchronize()
    dts = []
    for _ in range(WINDOWS):
        dec.reset(torch.tensor([1]), 0); dec.run(WARMUP); torch.cuda.synchronize()
        t0 = time.perf_counter(); dec.run(STEPS); torch.cuda.synchronize()
        dts.append(time.perf_counter() - t0)
    dec.free()
    dt = sorted(dts)[len(dts) // 2]
    return {"tokens_per_s": round(STEPS / dt, 1), "ms_per_step": round(dt / STEPS * 1e3, 4),
            "windows_tokens_per_s": [round(STEPS / d, 1) for d in dts]}


def fold_stats(path: str, result: dict, tokens: int, layers: int):
    rows = list(csv.DictReader(open(path)))
    name = lambda r: r.get("Name") or r.get("KernelName") or ""
    calls = lambda r: int(r.get("Calls") or r.get("Count") or 0)
    total = lambda r: float(r.get("TotalDurationNs") or r.get("TotalDuration(ns)") or 0.0)
    lora = [r for r in rows if "lora_" in name(r)]
    result["trace"] = {
        "tokens": tokens,
        "lora_launches_per_layer": round(sum(calls(r) for r in lora) / tokens / layers, 2),
        "lora_us_per_layer": round(sum(total(r) for r in lora) / 1e3 / tokens / layers, 3),
        "launches_per_layer": round(sum(calls(r) for r in rows) / tokens / layers, 2),
        "kernels": {name(r)[:60]: {"calls": calls(r), "us": round(total(r) / 1e3, 1)} for r in lora}}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--trace-run", type=int, default=0, help="decode this many tokens with the rank-16 adapter and exit (for rocprofv3)")
    p.add_argument("--stats-csv", default=None, help="kernel_stats.csv of a --trace-run: folded into the JSON")
    p.add_argument("--model", default="llama2-7b", choices=["llama2-7b", "tiny"])
    a = p.parse_args()
    cfg = (ExLlamaV2Config.llama2_7b(max_seq_len=2048, max_input_len=256) if a.model == "llama2-7b"
           else ExLlamaV2Config.tiny_test(max_seq_len=2048))
    if a.stats_csv:
        result = json.load(open(OUT)) if os.path.exists(OUT) else {}
        fold_stats(a.stats_csv, result, int(os.environ.get("LORA_TRACE_TOKENS", "64")), cfg.num_hidden_layers)
        json.dump(result, open(OUT, "w"), indent=1)
        print(json.dumps(result.get("trace")))
        return
    model = ExLlamaV2(cfg, device="cuda:0").load(synth_checkpoint(cfg, "cuda:0", recipe="4.0bpw", seed=0))
    cache = ExLlamaV2Cache(model, batch_size=1, max_seq_len=2048)
    if a.trace_run:
        lora = SynthLora(model, 16, 1)
        dec = GreedyGraphDecoder(model, cache, batch_size=1, loras=[lora])
        dec.reset(torch.tensor([1]), 0); dec.run(a.trace_run, use_graph=False); torch.cuda.synchronize()
        return
    result = {"model": f"{a.model} 4.0bpw synthetic, bs=1, EXL2_CHAIN=0 (module route), graph replay",
              "steps": STEPS, "warmup": WARMUP, "windows": WINDOWS}
    result["no_adapter"] = rate(model, cache, None)
    for rank in (16, 64):
        lora = SynthLora(model, rank, rank)
        result[f"rank_{rank}_all_seven"] = rate(model, cache, [lora])
        lora.detach(model)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    json.dump(result, open(OUT, "w"), indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
