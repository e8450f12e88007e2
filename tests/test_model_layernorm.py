"""End to end with LayerNorm models: sequential blocks with biased norms and projections and an ungated GELU MLP (StarCoder2), parallel
blocks with one bias-free norm, GPT-J rotary and a logit scale (Cohere), the latter also with a LayerNorm over the q / k heads -- tiny
synthetic models against tests/layernorm_oracle.LayerNormOracleModel.

The bar is check_logits at 1 x, the project's model tolerance, with no row left out; every step is fed the oracle's own tokens.
Checkpoints are drawn on the CPU (torch's CPU and GPU generators differ) and moved to the backend's device.  The seed of a case is the
first one for which the ORACLE's steps hold a confident token (top-1 / top-2 margin above 4 x the tolerance) -- the oracle decides,
never the code under test."""
import functools

import numpy as np
import pytest
import torch

from exllamav2_amd.cache import ExLlamaV2Cache
from exllamav2_amd.config import ExLlamaV2Config
from exllamav2_amd.model import ExLlamaV2, GreedyGraphDecoder
from exllamav2_amd.synth import synth_checkpoint
from tests.layernorm_oracle import LayerNormOracleModel
from tests.test_model import tiny_cfg, check_logits, confident

STEPS = 3
STARCODER2 = dict(norm="layernorm", norm_bias=True, mlp_gate=False, mlp_act_func="gelu", attention_bias_qkv=True, attention_bias_o=True,
                  mlp_bias=True)
COHERE = dict(norm="layernorm", parallel_decoder_blocks=True, rope_style=1, logit_scale=0.0625)
CASES = {
    "starcoder2-hd64": STARCODER2 | dict(head_dim=64),
    "starcoder2-hd128": STARCODER2 | dict(head_dim=128),
    "cohere-hd64": COHERE | dict(head_dim=64),
    "cohere-hd128": COHERE | dict(head_dim=128),
    "cohere-plus": COHERE | dict(head_dim=64, use_qk_norm=True, headnorm_rms=False),
}


def ln_cfg(case: str, **kw):
    return tiny_cfg(**(CASES[case] | kw))


def _to_device(ck: dict, device):
    return {k: ({kk: vv.to(device) for kk, vv in v.items()} if isinstance(v, dict) else v.to(device)) for k, v in ck.items()}


def oracle_run(oracle, ids, steps: int):
    """[(ids of the call, logits)]: the prompt, then `steps` single tokens, each the arg-max of the previous call"""
    oracle.reset(ids.shape[0])
    out = [(ids, oracle.forward(ids))]
    for _ in range(steps):
        nxt = np.argmax(out[-1][1][:, -1], axis=-1)[:, None]
        out.append((nxt, oracle.forward(nxt)))
    return out


@functools.lru_cache(maxsize=None)
def _reference(case: str, batch: int, prompt: int):
    """(seed, the oracle's run) of a case, computed once and shared: the first seed whose decode steps hold a confident token"""
    cfg = ln_cfg(case, max_batch_size=batch)
    ids = np.random.default_rng(1000 + batch + prompt).integers(0, cfg.vocab_size, size=(batch, prompt))
    for seed in range(8):
        ck = synth_checkpoint(cfg, "cpu", seed=seed)
        want = oracle_run(LayerNormOracleModel(cfg, ck), ids, STEPS)
        if sum(int(confident(w[:, -1]).sum()) for _, w in want[1:]) >= 1:
            return seed, want
    raise AssertionError("no seed with a confident token")


def _check_step(got, w):
    check_logits(got, w)
    conf = confident(w[:, -1])
    assert np.array_equal(got[:, -1].argmax(-1)[conf], w[:, -1].argmax(-1)[conf])
    return int(conf.sum())


@pytest.mark.parametrize("prompt", [20, 5])
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("case", list(CASES))
def test_prefill_then_decode(be, monkeypatch, case, batch, prompt):
    """the prompt through model.forward (20 tokens: the MFMA route), then 3 decode steps three ways: contiguous model.forward, the paged
    GreedyGraphDecoder with the parallel bridge and with the separate launches (eager; captured as one graph where the backend has graphs)
    -- identical tokens and bit-identical logits between the decoder runs, every logit within the model tolerance of the oracle"""
    cfg = ln_cfg(case, max_batch_size=batch)
    seed, want = _reference(case, batch, prompt)
    model = ExLlamaV2(cfg, device=be.device, ext=be.ext).load(_to_device(synth_checkpoint(cfg, "cpu", seed=seed), be.device))
    parallel = bool(cfg.parallel_decoder_blocks)
    assert (len(model.block_norms) == cfg.num_hidden_layers) == parallel and all(a.window == 0 for a, _ in model.layers)

    cache = ExLlamaV2Cache(model, batch_size=batch)
    logits = model.forward(torch.from_numpy(want[0][0]), cache, last_id_only=False)
    assert logits.dtype == torch.float16
    check_logits(be.n(logits), want[0][1])
    n_conf = 0
    for nxt, w in want[1:]:
        n_conf += _check_step(be.n(model.forward(torch.from_numpy(nxt), cache)), w)
    assert n_conf >= 1, "vacuous token check"

    runs = {}
    modes = [("bridge", "1", False), ("separate", "0", False)] + ([] if be.is_emu else [("bridge-graph", "1", True)])
    for name, env, graph in modes:
        monkeypatch.setenv("EXL2_PARALLEL_BRIDGE", env)
        dec = GreedyGraphDecoder(model, cache, batch_size=batch)
        assert dec.chain is None and dec.parallel_bridge == (parallel and env == "1") and dec.x.dtype == torch.float16
        if graph:
            dec.capture()
        toks, lg, n_conf = [], [], 0
        for i, (nxt, w) in enumerate(want[1:]):
            dec.reset(torch.from_numpy(nxt[:, 0]), prompt + i)
            dec.run(1, use_graph=graph)
            got = be.n(dec.logits)[:, None, :cfg.vocab_size].copy()
            n_conf += _check_step(got, w)
            toks.append(be.n(dec.ids).copy()); lg.append(got)
        assert n_conf >= 1, "vacuous token check"
        runs[name] = (np.stack(toks), np.stack(lg))
        dec.free()
    for name, (toks, lg) in runs.items():
        assert np.array_equal(toks, runs["bridge"][0]), f"{name}: tokens differ from the bridge's"
        assert np.array_equal(lg.view(np.uint16), runs["bridge"][1].view(np.uint16)), f"{name}: logits differ from the bridge's"
    model.unload()


def test_logit_scale_and_biases_matter():
    """the oracle without the logit scale, and without the norm biases, gives other logits: the checks above can tell"""
    for case, strip in (("cohere-hd64", dict(logit_scale=1.0)), ("starcoder2-hd64", None)):
        cfg = ln_cfg(case)
        ck = synth_checkpoint(cfg, "cpu", seed=0)
        ids = np.random.default_rng(7).integers(0, cfg.vocab_size, size=(1, 6))
        w = oracle_run(LayerNormOracleModel(cfg, ck), ids, 0)[0][1]
        if strip:
            other = oracle_run(LayerNormOracleModel(ln_cfg(case, **strip), ck), ids, 0)[0][1]
        else:
            other = oracle_run(LayerNormOracleModel(cfg, {k: v for k, v in ck.items() if not k.endswith("layernorm.bias")}), ids, 0)[0][1]
        with pytest.raises(AssertionError):
            check_logits(other, w)


def test_refusals(be):
    cfg = ln_cfg("starcoder2-hd64")
    model = ExLlamaV2(cfg, device=be.device, ext=be.ext).load(_to_device(synth_checkpoint(cfg, "cpu", seed=0), be.device))
    cache = ExLlamaV2Cache(model, batch_size=1)
    lora = object()
    with pytest.raises(RuntimeError, match="LoRA adapters are not built for a LayerNorm"):
        model.forward(torch.zeros((1, 3), dtype=torch.long), cache, loras=[lora])
    with pytest.raises(RuntimeError, match="LoRA adapters are not built for a LayerNorm"):
        GreedyGraphDecoder(model, cache, batch_size=1, loras=[lora])
    with pytest.raises(RuntimeError, match="LoRA adapters are not built for a LayerNorm"):
        model.update_loras()
    model.unload()
    from exllamav2_amd.pipeline import PipelineStage
    from exllamav2_amd.tensor_p import ExLlamaV2TP
    for case in ("starcoder2-hd64", "cohere-hd64"):
        with pytest.raises(RuntimeError, match="LayerNorm"):
            PipelineStage(ln_cfg(case), 0, 1, be.device, 1, 256, ext=be.ext)
        with pytest.raises(RuntimeError, match="LayerNorm"):
            ExLlamaV2TP(ln_cfg(case), 0, 2, device=be.device, ext=be.ext)


def test_config_and_synth():
    """presets, the config's own checks, and: existing checkpoints do not change for a seed"""
    s = ExLlamaV2Config.starcoder2_7b()
    assert (s.hidden_size, s.intermediate_size, s.num_hidden_layers, s.num_attention_heads, s.num_key_value_heads) == (4608, 18432, 32, 36, 4)
    assert s.layernorm and s.norm_bias and not s.mlp_gate and s.mlp_act_func == "gelu" and s.rope_style == 2
    assert s.sliding_window == 4096 and all(s.layer_window(i) == 0 for i in range(4))
    assert ExLlamaV2Config.starcoder2_3b().hidden_size == 3072 and ExLlamaV2Config.starcoder2_15b().num_hidden_layers == 40
    c = ExLlamaV2Config.command_r_35b()
    assert c.layernorm and c.parallel_decoder_blocks and c.rope_style == 1 and c.logit_scale == 0.0625 and not c.norm_bias
    assert ExLlamaV2Config.aya_23_8b().num_key_value_heads == 8
    assert not ExLlamaV2Config.llama2_7b().layernorm
    with pytest.raises(ValueError, match="LayerNorm"):
        tiny_cfg(parallel_decoder_blocks=True)
    with pytest.raises(ValueError, match="LayerNorm"):
        tiny_cfg(norm="layernorm", residual_fp32=True, post_norms=True)
    with pytest.raises(ValueError, match="DBRX"):
        tiny_cfg(norm="layernorm", num_experts=4)
    base = synth_checkpoint(tiny_cfg(), "cpu", seed=3)
    sc = synth_checkpoint(ln_cfg("starcoder2-hd64"), "cpu", seed=3)
    co = synth_checkpoint(ln_cfg("cohere-hd64"), "cpu", seed=3)
    assert not any("gate_proj" in k for k in sc) and not any("post_attention_layernorm" in k for k in co)
    assert "model.norm.bias" in sc and "model.layers.0.input_layernorm.bias" in sc and "model.norm.bias" not in co
    assert all("bias" in sc[f"model.layers.1.{n}"] for n in ("self_attn.q_proj", "self_attn.o_proj", "mlp.up_proj", "mlp.down_proj"))
    for k, v in base.items():                                                # Cohere's tensors are the plain model's draws
        if k in co:
            assert all(torch.equal(v[kk], co[k][kk]) for kk in v) if isinstance(v, dict) else torch.equal(v, co[k])
