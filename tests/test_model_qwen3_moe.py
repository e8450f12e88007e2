"""End to end with Qwen3-MoE blocks (q / k head norm attention + a 128-expert top-8 sparse MLP): prompt logits through model.forward,
decode through the chained GreedyGraphDecoder (the block inside the chain, one captured graph per token on the GPU) against
tests/qwen3_moe_oracle.Qwen3MoeOracleModel -- the shape of tests/test_moe.py::test_moe_model_equals_oracle.

Top-k is discontinuous: a (row, step) pair is compared where the oracle's router gap (qwen3_moe_oracle.router_gap: the distance between
the 8th and the 9th logit in fp16 steps, minimum over the layers) is above 8; at most a third of the pairs may be left out.  With the
oracle's own tokens fed back 1 of 5, 3 of 15 and 21 of 80 pairs are below that gap at batch 1 / 3 / 16 (seed 11, found with the oracle
alone); the device's tokens may differ from the oracle's where logits tie.  The checkpoint is drawn on the CPU and moved to the
backend's device (torch's CPU and GPU generators differ), so both backends run the checkpoint those figures belong to."""
import numpy as np
import pytest
import torch

from exllamav2_amd.cache import ExLlamaV2Cache
from exllamav2_amd.config import ExLlamaV2Config
from exllamav2_amd.model import ExLlamaV2, GreedyGraphDecoder
from exllamav2_amd.synth import synth_checkpoint
from tests.qwen3_moe_oracle import Qwen3MoeOracleModel

GAP = 8.0


def _cfg(**kw):
    d = dict(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1, head_dim=64,
             vocab_size=96, max_seq_len=256, max_input_len=32, max_batch_size=16, num_experts=128, num_experts_per_token=8,
             use_qk_norm=True, norm_eps=1e-6, arch="qwen3_moe")
    d.update(kw)
    return ExLlamaV2Config(**d)


def _to_device(ck: dict, device):
    return {k: ({kk: vv.to(device) for kk, vv in v.items()} if isinstance(v, dict) else v.to(device)) for k, v in ck.items()}


def _build(device, ext, cfg, seed=11, oracle=True):
    ck = synth_checkpoint(cfg, "cpu", recipe="4.0bpw", seed=seed)
    orc = Qwen3MoeOracleModel(cfg, ck) if oracle else None                 # (before load(): it re-lays the tensors out in place)
    model = ExLlamaV2(cfg, device=device, ext=ext).load(_to_device(ck, device))
    return model, orc


@pytest.mark.parametrize("batch", [1, 3, 16])
def test_qwen3_moe_model_equals_oracle(be, batch):
    cfg = _cfg()
    model, oracle = _build(be.device, be.ext, cfg)
    assert all(attn.q_norm is not None and mlp.num_experts == 128 for attn, mlp in model.layers)
    cache = ExLlamaV2Cache(model, batch_size=batch, max_seq_len=256)
    ids = (np.array([[5, 17, 42, 7]]) + 13 * np.arange(batch)[:, None]) % cfg.vocab_size
    oracle.reset(batch)
    skipped, compared = 0, 0

    def compare(got, want):
        nonlocal skipped, compared
        ok = oracle.router_gap > GAP
        skipped += int((~ok).sum()); compared += int(ok.sum())
        err, tol = np.abs(got - want)[ok], (0.03 + np.abs(want) * 2.0 ** -8)[ok]
        if ok.any():
            print(f"batch {batch}: worst error / bound = {float((err / tol).max()):.3f} over {int(ok.sum())} rows")
        assert np.all(err <= tol), float((err / tol).max())

    want = oracle.forward(ids)[:, -1]
    compare(be.n(model.forward(torch.from_numpy(ids), cache)).astype(np.float64)[:, -1], want)
    tok = want.argmax(-1).astype(np.int64)
    dec = GreedyGraphDecoder(model, cache, batch_size=batch)
    assert dec.chain is not None                # (the attention half chained, the block publishing its result: in_m = "moe")
    if not be.is_emu:
        dec.capture()
    dec.reset(torch.from_numpy(tok), ids.shape[1])
    for step in range(4):
        dec.run(1, use_graph=not be.is_emu)
        assert dec.chain is not None
        want = oracle.forward(tok[:, None])[:, -1]
        compare(be.n(dec.logits).astype(np.float64)[:, :cfg.vocab_size], want)
        tok = be.n(dec.tokens(ids.shape[1] + step, 1))[:, 0].astype(np.int64)
    assert compared + skipped == 5 * batch and 3 * skipped <= compared + skipped, (compared, skipped)
    dec.free()
    model.unload()


@pytest.mark.parametrize("rows", [1, 4, 16])
def test_qwen3_moe_fused_front_is_bit_identical(be, rows, monkeypatch):
    """the norm inside the logits launch against the norm as a launch of its own (EXL2_MOE_UNFUSED_FRONT=1) in front of the same
    pair jobs: same routing weights, same block output, bit for bit (tests/test_moe.py::test_moe_fused_front_is_bit_identical at 128
    experts)"""
    cfg = _cfg(hidden_size=256, intermediate_size=512, num_hidden_layers=1, num_attention_heads=4, num_key_value_heads=2)
    model, _ = _build(be.device, be.ext, cfg, seed=21, oracle=False)
    moe = model.layers[0][1]
    x = torch.from_numpy(np.random.default_rng(rows).standard_normal((rows, 1, cfg.hidden_size)).astype(np.float16)).to(be.device)
    outs = []
    for unfused in ("0", "1"):
        if unfused == "1": monkeypatch.setenv("EXL2_MOE_UNFUSED_FRONT", "1")
        y = x.clone()
        moe.forward(y)
        outs.append((be.n(y).copy(), be.n(moe.temp_logits[:rows]).copy()))
    assert np.all((outs[0][1] != 0).sum(-1) == 8)
    assert np.array_equal(outs[0][1].view(np.uint16), outs[1][1].view(np.uint16))      # routing weights
    assert np.array_equal(outs[0][0].view(np.uint16), outs[1][0].view(np.uint16))      # block output
    model.unload()


@pytest.mark.gpu
def test_qwen3_moe_graph_replays_with_other_experts():
    """batch 1: the SAME captured graph replayed twice with different tokens, so different experts (the hand-out is part of the graph,
    the experts are not) -- logits and routing equal to the eager steps, bit for bit"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    cfg = _cfg()
    model, _ = _build("cuda:0", None, cfg, oracle=False)
    first = torch.tensor([23])
    runs = {}
    for use_graph in (True, False):
        cache = ExLlamaV2Cache(model, batch_size=1, max_seq_len=256)
        dec = GreedyGraphDecoder(model, cache, batch_size=1)
        assert dec.chain is not None
        if use_graph: dec.capture()
        dec.reset(first, 0)
        steps = []
        for _ in range(3):
            dec.run(1, use_graph=use_graph)
            torch.cuda.synchronize()
            steps.append((dec.logits.cpu().numpy().copy(), [mlp.temp_logits[:1].cpu().numpy().copy() for _, mlp in model.layers]))
        runs[use_graph] = (steps, dec.tokens(0, 3).cpu().numpy().copy())
        dec.free()
    picked = set()
    for (lg, wg), (le, we) in zip(runs[True][0], runs[False][0]):
        assert np.array_equal(lg.view(np.uint16), le.view(np.uint16))
        for a, b in zip(wg, we):
            assert np.array_equal(a.view(np.uint16), b.view(np.uint16)) and (a != 0).sum() == 8
        picked.add(tuple(np.nonzero(wg[0][0])[0].tolist()))
    assert np.array_equal(runs[True][1], runs[False][1])
    assert len(picked) >= 2, picked                # (the replays selected different experts)
    model.unload()
