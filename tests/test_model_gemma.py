"""End to end with Gemma-2 / Gemma-3 blocks: fp32 residual stream, post norms, GELU, scaled embedding, a sliding window on the windowed
layers, score and logit caps, query_pre_attn_scalar -- tiny synthetic models against tests/gemma_oracle.GemmaOracleModel.

The bar is check_logits at 1 x, the project's model tolerance, with no row left out; every step is fed the oracle's own tokens.
Checkpoints are drawn on the CPU (torch's CPU and GPU generators differ) and moved to the backend's device.  All cases run at seed 0.
"""
import numpy as np
import pytest
import torch

from exllamav2_amd.cache import ExLlamaV2Cache, ExLlamaV2Cache_Q4
from exllamav2_amd.config import ExLlamaV2Config
from exllamav2_amd.model import ExLlamaV2, GreedyGraphDecoder
from exllamav2_amd.synth import synth_checkpoint
from tests.gemma_oracle import GemmaOracleModel, layer_is_windowed
from tests.test_model import tiny_cfg, check_logits, confident, LOGIT_TOL

STEPS = 3
GEMMA = dict(residual_fp32=True, post_norms=True, norm_constant_bias=1.0, normalize_embeddings=True, mlp_act_func="gelu", norm_eps=1e-6,
             query_pre_attn_scalar=100.0, sliding_window=8, alternating_swa=True)
CASES = {
    "gemma2-hd64": dict(head_dim=64, attn_logit_softcapping=50.0, final_logit_softcapping=30.0),
    "gemma2-hd128": dict(head_dim=128, attn_logit_softcapping=50.0, final_logit_softcapping=30.0),
    "gemma3-hd64": dict(head_dim=64, use_qk_norm=True, sliding_window_pattern=2, rotary_embedding_base_alt=100.0),
}


def gemma_cfg(case: str, **kw):
    return tiny_cfg(**(GEMMA | CASES[case] | kw))


def _to_device(ck: dict, device):
    return {k: ({kk: vv.to(device) for kk, vv in v.items()} if isinstance(v, dict) else v.to(device)) for k, v in ck.items()}


def _build(be, cfg, recipe="4.0bpw", seed=0, **oracle_kw):
    ck = synth_checkpoint(cfg, "cpu", recipe=recipe, seed=seed)
    oracle = GemmaOracleModel(cfg, ck, **oracle_kw)                        # (before load(): it re-lays the tensors out in place)
    model = ExLlamaV2(cfg, device=be.device, ext=be.ext).load(_to_device(ck, be.device))
    return model, oracle


def oracle_run(oracle, ids, steps: int, feed=None):
    """[(ids of the call, logits)]: the prompt, then `steps` single tokens -- the arg-max of the previous call, or feed[i]"""
    oracle.reset(ids.shape[0])
    out = [(ids, oracle.forward(ids))]
    for i in range(steps):
        nxt = np.argmax(out[-1][1][:, -1], axis=-1)[:, None] if feed is None else feed[i]
        out.append((nxt, oracle.forward(nxt)))
    return out


def _check_step(got, w):
    check_logits(got, w)
    conf = confident(w[:, -1])
    assert np.array_equal(got[:, -1].argmax(-1)[conf], w[:, -1].argmax(-1)[conf])
    return int(conf.sum())


@pytest.mark.parametrize("prompt", [20, 5])
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("case", list(CASES))
def test_prefill_then_decode(be, monkeypatch, case, batch, prompt):
    """the prompt through model.forward (20 tokens: the MFMA prefill with a window that clips), then 3 decode steps three ways:
    contiguous model.forward, the paged GreedyGraphDecoder with the norm bridge and with the handles' own norms (eager; captured as one
    graph where the backend has graphs) -- identical tokens, every logit within the model tolerance of the oracle"""
    cfg = gemma_cfg(case, max_batch_size=batch)
    model, oracle = _build(be, cfg)
    assert [a.window for a, _ in model.layers] == [8, 0] and model.layers[0][0].post_layernorm is not None
    assert (model.layers[0][0].sin is model.sin_alt) == (case == "gemma3-hd64")
    ids = np.random.default_rng(1000 + batch + prompt).integers(0, cfg.vocab_size, size=(batch, prompt))
    want = oracle_run(oracle, ids, STEPS)

    # contiguous
    cache = ExLlamaV2Cache(model, batch_size=batch)
    logits = model.forward(torch.from_numpy(want[0][0]), cache, last_id_only=False)
    assert logits.dtype == torch.float16
    check_logits(be.n(logits), want[0][1])
    n_conf = 0
    for nxt, w in want[1:]:
        n_conf += _check_step(be.n(model.forward(torch.from_numpy(nxt), cache)), w)
    assert n_conf >= 1, "vacuous token check"

    # paged decoder over the same cache rows: the decode steps again, positions read on the device
    runs = {}
    modes = [("bridge", "1", False), ("two-launch", "0", False)] + ([] if be.is_emu else [("bridge-graph", "1", True)])
    for name, env, graph in modes:
        monkeypatch.setenv("EXL2_NORM_BRIDGE", env)
        dec = GreedyGraphDecoder(model, cache, batch_size=batch)
        assert dec.chain is None and dec.norm_bridge == (env == "1") and dec.x.dtype == torch.float32
        if graph:
            dec.capture()
        toks, n_conf = [], 0
        for i, (nxt, w) in enumerate(want[1:]):
            dec.reset(torch.from_numpy(nxt[:, 0]), prompt + i)
            dec.run(1, use_graph=graph)
            got = be.n(dec.logits)[:, None, :cfg.vocab_size]
            n_conf += _check_step(got, w)
            toks.append(be.n(dec.ids).copy())
        assert n_conf >= 1, "vacuous token check"
        runs[name] = np.stack(toks)
        dec.free()
    for name in runs:
        assert np.array_equal(runs[name], runs["bridge"]), f"{name}: tokens differ from the bridge's"
    model.unload()


def test_window_and_caps_matter(be):
    """the oracle without the window gives other logits for a 20-token prompt (the window clipped), and the model follows the windowed one"""
    cfg = gemma_cfg("gemma2-hd64")
    model, oracle = _build(be, cfg)
    ck = synth_checkpoint(cfg, "cpu", seed=0)
    no_window = GemmaOracleModel(cfg, ck, use_window=False)
    ids = np.random.default_rng(7).integers(0, cfg.vocab_size, size=(1, 20))
    w = oracle_run(oracle, ids, 0)[0][1]
    nw = oracle_run(no_window, ids, 0)[0][1]
    assert np.array_equal(w[:, :9], nw[:, :9])                              # the first window + 1 tokens see everything either way
    assert float(np.abs(w[:, 9:] - nw[:, 9:]).max()) > 4 * LOGIT_TOL
    cache = ExLlamaV2Cache(model, batch_size=1)
    got = be.n(model.forward(torch.from_numpy(ids), cache, last_id_only=False))
    check_logits(got, w)
    assert np.all(np.abs(got.astype(np.float64)) <= cfg.final_logit_softcapping)
    model.unload()


def test_refusals(be):
    cfg = gemma_cfg("gemma2-hd64", num_key_value_heads=8, num_attention_heads=8, hidden_size=512, intermediate_size=512)
    model, _ = _build(be, cfg)
    q4 = ExLlamaV2Cache_Q4(model, batch_size=1)
    with pytest.raises(RuntimeError, match="quantized cache"):
        GreedyGraphDecoder(model, q4, batch_size=1)
    with pytest.raises(RuntimeError, match="quantized cache"):
        model.forward(torch.zeros((1, 3), dtype=torch.long), q4)
    model.unload()
    from exllamav2_amd.pipeline import PipelineStage
    from exllamav2_amd.tensor_p import ExLlamaV2TP
    with pytest.raises(RuntimeError, match="fp32 residual"):
        PipelineStage(cfg, 0, 1, be.device, 1, 256, ext=be.ext)
    with pytest.raises(RuntimeError, match="fp32 residual"):
        ExLlamaV2TP(cfg, 0, 2, device=be.device, ext=be.ext)


def test_config_and_synth():
    """presets and the reference's window rule (model.py:111-121); existing checkpoints do not change for a seed"""
    c = ExLlamaV2Config.gemma2_9b()
    assert (c.hidden_size, c.num_hidden_layers, c.head_dim, c.residual_fp32, c.post_norms, c.mlp_act_func) == (3584, 42, 256, True, True, "gelu")
    assert [c.layer_window(i) for i in range(4)] == [4096, 0, 4096, 0] and not c.layer_rope_alt(0)
    assert c.softmax_scale() == 256.0 ** -0.5 and ExLlamaV2Config.gemma2_27b().softmax_scale() == 144.0 ** -0.5
    assert ExLlamaV2Config.gemma2_2b().hidden_size == 2304
    g3 = ExLlamaV2Config.gemma3_4b()
    assert g3.use_qk_norm and g3.sliding_window_pattern == 6 and not g3.final_logit_softcapping
    assert [g3.layer_window(i) > 0 for i in range(12)] == [True] * 5 + [False] + [True] * 5 + [False]
    assert all(g3.layer_rope_alt(i) == (g3.layer_window(i) > 0) for i in range(12))
    for i in range(12):
        assert layer_is_windowed(g3, i) == (g3.layer_window(i) > 0) and layer_is_windowed(c, i) == (c.layer_window(i) > 0)
    plain = ExLlamaV2Config.llama2_7b()
    assert plain.layer_window(0) == 0 and plain.softmax_scale() == 128 ** -0.5 and not plain.residual_fp32
    with pytest.raises(ValueError, match="Gemma-1"):
        tiny_cfg(normalize_embeddings=True)
    with pytest.raises(ValueError, match="post_norms"):
        tiny_cfg(residual_fp32=True)
    base = synth_checkpoint(tiny_cfg(), "cpu", seed=3)
    gem = synth_checkpoint(gemma_cfg("gemma2-hd64"), "cpu", seed=3)
    for k, v in base.items():
        if isinstance(v, dict):
            assert all(torch.equal(v[kk], gem[k][kk]) for kk in v)
        elif "norm" in k:
            assert torch.equal(v, (gem[k] + 1.0).half())                    # on disk without the constant bias
        else:
            assert torch.equal(v, gem[k])
    new = sorted(set(gem) - set(base))
    assert new == sorted(f"model.layers.{i}.{n}" for i in range(2) for n in ("pre_feedforward_layernorm", "post_feedforward_layernorm"))
