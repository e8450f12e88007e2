#!/usr/bin/env python3
"""Decode attention kernel timing per shape (fused one-launch kernel), HIP events around 200 back-to-back launches.
--caches: the same step per cache type (fp16 | q4 | q6 | q8; quantized: attention from the codes against unpack + attend + re-quantize)."""
import os, sys, json
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from exllamav2_amd.ext import ext_c as ext

def run(nh, kvh, hd, ctx, pages=80, quiet=False):
    dev = "cuda"
    q = torch.randn((1, 1, nh, hd), device=dev, dtype=torch.float16)
    kn = torch.randn((1, 1, kvh, hd), device=dev, dtype=torch.float16)
    vn = torch.randn((1, 1, kvh, hd), device=dev, dtype=torch.float16)
    kc = torch.randn((pages, 256, kvh, hd), device=dev, dtype=torch.float16)
    vc = torch.randn((pages, 256, kvh, hd), device=dev, dtype=torch.float16)
    out = torch.empty_like(q)
    sin = torch.zeros((pages * 256, hd), device=dev, dtype=torch.float16); cos = torch.ones_like(sin)
    sl = torch.tensor([ctx], dtype=torch.int32, device=dev)
    bt = torch.arange(pages, dtype=torch.int32, device=dev).view(1, pages)
    scratch = torch.zeros((ext.paged_attn_scratch_bytes(nh, hd, 64) // 4 + 16,), dtype=torch.float32, device=dev)
    cnt = torch.zeros((4096,), dtype=torch.int32, device=dev)
    f = lambda: ext.attn_decode_fused(q, kn, vn, kc, vc, out, sin, cos, sl, bt, 0, 2, scratch, cnt)
    for _ in range(5): f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    n = 60 if quiet else 200
    for _ in range(n): f()
    e1.record(); torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / n
    kvb = 2 * ctx * kvh * hd * 2
    if quiet:
        return us
    print(json.dumps({"heads": nh, "kv_heads": kvh, "head_dim": hd, "ctx": ctx, "us": round(us, 2), "kv_MB": round(kvb / 1e6, 2),
                      "GBs": round(kvb / us / 1e3, 1)}), flush=True)
    return us

def run_caches(nh, kvh, hd, ctx, out_path=None, reps=7, n=60):
    """One decode attention step of one layer per cache type and route at `ctx` cached keys: the fp16 one-launch kernel, attention
    straight from the codes (`direct`: the one-launch step of csrc/attn_q4.hip at 4 / 6 / 8 bits) and, per quantized width, `unpack` =
    q_to_fp16_kv of the live range + RoPE / append + the fp16 attention launch + fp16_to_q_kv of the step (what a quantized cache costs
    without the direct route).  Variants interleaved, `reps` rounds of `n` back-to-back steps each, medians; GB/s = the bytes a
    variant's format holds for the live keys (codes + scales | fp16) over its time."""
    import statistics
    dev = "cuda"
    pages = (ctx + 1 + 255) // 256 + 1
    q = torch.randn((1, 1, nh, hd), device=dev, dtype=torch.float16)
    kn = torch.randn((1, 1, kvh, hd), device=dev, dtype=torch.float16)
    vn = torch.randn((1, 1, kvh, hd), device=dev, dtype=torch.float16)
    kc = torch.randn((pages, 256, kvh, hd), device=dev, dtype=torch.float16)
    vc = torch.randn((pages, 256, kvh, hd), device=dev, dtype=torch.float16)
    out = torch.empty_like(q)
    sin = torch.zeros((pages * 256, hd), device=dev, dtype=torch.float16); cos = torch.ones_like(sin)
    sl = torch.tensor([ctx], dtype=torch.int32, device=dev)
    bt = torch.arange(pages, dtype=torch.int32, device=dev).view(1, pages)
    scratch = torch.zeros((ext.paged_attn_scratch_bytes(nh, hd, 64) // 4 + 16,), dtype=torch.float32, device=dev)
    cnt = torch.zeros((4096,), dtype=torch.int32, device=dev)
    variants = {"fp16": (lambda: ext.attn_decode_fused(q, kn, vn, kc, vc, out, sin, cos, sl, bt, 0, 2, scratch, cnt), 2 * hd * 2)}
    keep = []
    for wbits in (4, 6, 8):
        kb, vb = (8 if wbits >= 6 else 4), (8 if wbits == 8 else 4)
        kq = torch.zeros((pages, 256, kvh, hd * kb // 8), device=dev, dtype=torch.uint8)
        vq = torch.zeros((pages, 256, kvh, hd * vb // 8), device=dev, dtype=torch.uint8)
        ks = torch.zeros((pages, 256, kvh, hd // 32), device=dev, dtype=torch.float16); vs = torch.zeros_like(ks)
        full = torch.tensor([pages * 256 - 256], dtype=torch.int32, device=dev)
        zero = torch.zeros((1,), dtype=torch.int32, device=dev)
        ext.fp16_to_q_kv(kc, kq, ks, vc, vq, vs, 1, 0, pages * 256 - 256, 256, zero, bt, wbits)      # real codes: the whole range packed
        tk, tv = torch.zeros_like(kc), torch.zeros_like(vc)
        keep.append((kq, vq, ks, vs, tk, tv, full, zero))
        per_key = hd * kb // 8 + hd * vb // 8 + 2 * (hd // 32) * 2

        def direct(kq=kq, ks=ks, vq=vq, vs=vs, wbits=wbits):
            assert ext.attn_q_decode_fused(q, kn, vn, kq, ks, vq, vs, out, sin, cos, sl, bt, 0, 2, scratch, cnt, wbits)

        def unpack(kq=kq, ks=ks, vq=vq, vs=vs, tk=tk, tv=tv, wbits=wbits):
            ext.q_to_fp16_kv(kq, tk, ks, vq, tv, vs, 1, 0, 0, 256, sl, bt, wbits)
            assert ext.attn_decode_fused(q, kn, vn, tk, tv, out, sin, cos, sl, bt, 0, 2, scratch, cnt)
            ext.fp16_to_q_kv(tk, kq, ks, tv, vq, vs, 1, 0, 1, 256, sl, bt, wbits)
        variants[f"q{wbits} direct"] = (direct, per_key)
        variants[f"q{wbits} unpack"] = (unpack, per_key)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for f, _ in variants.values():                                 # warm-up (and clock ramp) before anything is timed
        for _ in range(20): f()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(reps):
        for name, (f, _) in variants.items():
            e0.record()
            for _ in range(n): f()
            e1.record(); torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / n)
    rows = []
    for name, (_, per_key) in variants.items():
        us = statistics.median(times[name])
        row = {"heads": nh, "kv_heads": kvh, "head_dim": hd, "ctx": ctx, "variant": name, "us": round(us, 2), "us_min": round(min(times[name]), 2),
               "us_max": round(max(times[name]), 2), "bytes_per_key_per_kv_head": per_key, "GBs": round(ctx * kvh * per_key / us / 1e3, 1)}
        rows.append(row)
        print(json.dumps(row), flush=True)
        if out_path:
            with open(out_path, "a") as fh:
                fh.write(json.dumps(row) + "\n")
    return rows


if __name__ == "__main__":
    if "--caches" in sys.argv:
        # fp16 | q4 | q6 | q8, the quantized ones direct and unpack:  --caches [--out FILE.jsonl]
        out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
        bad = []
        for nh, kvh in ((32, 32), (64, 8), (32, 8)):
            for ctx in (2000, 8000, 16000):
                rows = {r["variant"]: r["us"] for r in run_caches(nh, kvh, 128, ctx, out_path)}
                bad += [(nh, kvh, ctx, w) for w in (4, 6, 8) if not rows[f"q{w} direct"] < rows[f"q{w} unpack"]]
        if bad:
            print("direct NOT faster than unpack at:", bad, flush=True)
        sys.exit(3 if bad else 0)                                  # (3: ran to the end, the relation does not hold)
    if "--sweep" in sys.argv:
        # splits x keys-per-split sweep at long contexts (EXL2_ATT_NSPLIT_MAX / EXL2_ATT_KPS are read per launch)
        for nh, kvh in ((32, 32), (64, 8)):
            for ctx in (2000, 8000, 16000):
                for nsplit, kps in ((0, 0), (16, 64), (32, 64), (32, 128), (64, 64), (64, 128), (64, 256)):
                    os.environ.pop("EXL2_ATT_NSPLIT_MAX", None); os.environ.pop("EXL2_ATT_KPS", None)
                    if nsplit: os.environ["EXL2_ATT_NSPLIT_MAX"] = str(nsplit); os.environ["EXL2_ATT_KPS"] = str(kps)
                    print(json.dumps({"nsplit_max": nsplit or "policy", "kps": kps or "default"}), end=" ", flush=True)
                    run(nh, kvh, 128, ctx)
        sys.exit(0)
    if "--sweep2" in sys.argv:
        # finer grid behind the split policy of csrc/attn.hip: best (splits, keys per split) per shape and context
        for nh, kvh, pages in ((32, 32, 140), (64, 8, 140), (32, 8, 140)):
            for ctx in (500, 1000, 2000, 4000, 8000, 16000, 32000):
                best = None
                for nsplit in (4, 8, 16, 24, 32, 48, 64):
                    for kps in (64, 128, 256, 512, 1024):
                        if nsplit * kps < ctx / 4 and nsplit < 64: continue          # (far too few splits for this context)
                        os.environ["EXL2_ATT_NSPLIT_MAX"] = str(nsplit); os.environ["EXL2_ATT_KPS"] = str(kps)
                        us = run(nh, kvh, 128, ctx, pages=pages, quiet=True)
                        if best is None or us < best[0]: best = (us, nsplit, kps)
                        print(json.dumps({"heads": nh, "kv_heads": kvh, "ctx": ctx, "nsplit_max": nsplit, "kps": kps, "us": round(us, 2)}), flush=True)
                os.environ.pop("EXL2_ATT_NSPLIT_MAX", None); os.environ.pop("EXL2_ATT_KPS", None)
                pol = run(nh, kvh, 128, ctx, pages=pages, quiet=True)
                print(json.dumps({"heads": nh, "kv_heads": kvh, "ctx": ctx, "BEST": {"us": round(best[0], 2), "nsplit_max": best[1], "kps": best[2]}, "policy_us": round(pol, 2)}), flush=True)
        sys.exit(0)
    for nh, kvh in ((32, 32), (64, 8), (32, 8)):
        for ctx in (64, 2000, 16000):
            run(nh, kvh, 128, ctx)
