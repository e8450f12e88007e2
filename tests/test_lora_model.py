"""LoRA adapters end to end: ExLlamaV2Lora loads a PEFT adapter directory, ExLlamaV2.forward(..., loras=[...]) and
GreedyGraphDecoder(..., loras=[...]) apply it -- tiny synthetic Llama against the oracle with the same adapters
(tests/lora_oracle.py: LoraOracleModel, the reference's kernel composition q_attn.cu:266-344 / q_mlp.cu:176-235 restated).

Bar: check_logits at 1 x LOGIT_TOL over every row; tokens where the oracle is confident.  Every case also asserts that the oracle's
logits WITH the adapters differ from those without by more than 10 x LOGIT_TOL somewhere: a path that adds nothing cannot pass."""
import json
import os

import numpy as np
import pytest
import torch
from safetensors.torch import save_file

from exllamav2_amd.cache import ExLlamaV2Cache, ExLlamaV2Cache_Q4
from exllamav2_amd.lora import ExLlamaV2Lora
from exllamav2_amd.model import ExLlamaV2, GreedyGraphDecoder
from exllamav2_amd.synth import synth_checkpoint
from oracle.model import OracleModel
from tests.lora_oracle import LoraOracleModel, PROJ_KEYS
from tests.test_model import tiny_cfg, check_logits, confident, LOGIT_TOL

F16 = np.float16
SCALING = 0.5


def lora_cfg(**kw):
    d = dict(hidden_size=256, intermediate_size=512, num_attention_heads=4, num_key_value_heads=2, head_dim=64)
    d.update(kw)
    return tiny_cfg(**d)


def _dims(cfg, proj):
    h, q, kv, i = cfg.hidden_size, cfg.num_attention_heads * cfg.head_dim, cfg.num_key_value_heads * cfg.head_dim, cfg.intermediate_size
    return {"self_attn.q_proj": (h, q), "self_attn.k_proj": (h, kv), "self_attn.v_proj": (h, kv), "self_attn.o_proj": (q, h),
            "mlp.gate_proj": (h, i), "mlp.up_proj": (h, i), "mlp.down_proj": (i, h)}[proj]


def write_adapter(path, cfg, seed, r, projections=PROJ_KEYS, alpha=12.0, rslora=True, amp=1.0, extra=None, config_extra=None):
    """A PEFT adapter directory (adapter_config.json + adapter_model.safetensors): `base_model.model.` key prefix, lora_A [r, in] /
    lora_B [out, r], one bf16 tensor, one fp32, the rest fp16, an all-zero bias entry.  Returns the oracle's form of the adapter:
    {"model.layers.<i>.<proj>": (A fp16 [in, r], B fp16 [r, out] pre-scaled)} for lora_scaling = SCALING."""
    os.makedirs(path, exist_ok=True)
    rng = np.random.default_rng(seed)
    scale = SCALING * (alpha * np.sqrt(r) if rslora else alpha) / r
    tensors, oracle = {}, {}
    n = 0
    for i in range(cfg.num_hidden_layers):
        for proj in projections:
            K, N = _dims(cfg, proj)
            a = torch.from_numpy((rng.standard_normal((r, K)) / np.sqrt(K)).astype(np.float32))
            b = torch.from_numpy((amp * rng.standard_normal((N, r)) / (np.sqrt(r) * scale)).astype(np.float32))
            dt = (torch.bfloat16, torch.float32, torch.float16)[min(n, 2)]
            a, b = a.to(dt), b.to(dt)
            n += 1
            pre = f"base_model.model.model.layers.{i}.{proj}"
            tensors[pre + ".lora_A.weight"], tensors[pre + ".lora_B.weight"] = a.contiguous(), b.contiguous()
            oracle[f"model.layers.{i}.{proj}"] = (a.float().t().to(torch.float16).numpy().copy(),
                                                  (b.float().t() * np.float32(scale)).to(torch.float16).numpy().copy())
    tensors["base_model.model.model.layers.0.self_attn.q_proj.bias"] = torch.zeros(8, dtype=torch.float16)
    tensors.update(extra or {})
    save_file(tensors, os.path.join(path, "adapter_model.safetensors"))
    cfgj = {"r": r, "lora_alpha": alpha, "use_rslora": rslora, "peft_type": "LORA"}
    cfgj.update(config_extra or {})
    with open(os.path.join(path, "adapter_config.json"), "w") as f:
        json.dump(cfgj, f)
    return oracle


def build(be, cfg, tmp_path, n_adapters, seed=0, recipe="4.0bpw"):
    ck = synth_checkpoint(cfg, be.device, recipe=recipe, seed=seed)
    oracle, plain = LoraOracleModel(cfg, ck), OracleModel(cfg, ck)
    model = ExLlamaV2(cfg, device=be.device, ext=be.ext).load(ck)
    specs = [dict(r=8, projections=PROJ_KEYS), dict(r=20, projections=("self_attn.q_proj", "self_attn.v_proj"))][:n_adapters]
    loras, oracle.active = [], []
    for j, sp in enumerate(specs):
        d = str(tmp_path / f"adapter{j}")
        oracle.active.append(write_adapter(d, cfg, 100 + seed + j, amp=0.25, **sp))
        loras.append(ExLlamaV2Lora.from_directory(model, d, lora_scaling=SCALING))
        assert loras[-1].bias_ignored and loras[-1].lora_r == sp["r"]
    return model, oracle, plain, loras


def _moved(want, want_plain):
    """the adapters matter: somewhere the oracle's logits move by more than 10 x LOGIT_TOL"""
    assert np.abs(want - want_plain).max() > 10 * LOGIT_TOL, np.abs(want - want_plain).max()


@pytest.mark.parametrize("chunked", [False, True])
@pytest.mark.parametrize("n_adapters", [1, 2])
def test_prefill_then_decode_with_adapters(be, tmp_path, n_adapters, chunked):
    cfg = lora_cfg(max_input_len=8 if chunked else 64)          # 2 sequences x 9 tokens: 3 chunks of 4 rows per sequence, or one
    model, oracle, plain, loras = build(be, cfg, tmp_path, n_adapters, seed=n_adapters)
    cache = ExLlamaV2Cache(model, batch_size=2)
    oracle.reset(2); plain.reset(2)
    ids = np.random.default_rng(3).integers(0, cfg.vocab_size, size=(2, 9))
    logits = model.forward(torch.from_numpy(ids), cache, last_id_only=False, loras=loras)
    want, wp = oracle.forward(ids), plain.forward(ids)
    check_logits(be.n(logits), want)
    _moved(want, wp)
    nxt = np.argmax(want[:, -1], axis=-1)[:, None]
    n_conf = 0
    for _ in range(4):
        logits = be.n(model.forward(torch.from_numpy(nxt), cache, loras=loras))
        want = oracle.forward(nxt)
        check_logits(logits, want)
        conf = confident(want[:, -1])
        assert np.array_equal(logits[:, -1].argmax(-1)[conf], np.argmax(want[:, -1], -1)[conf])
        n_conf += int(conf.sum())
        nxt = np.argmax(want[:, -1], axis=-1)[:, None]
    assert n_conf >= 1, "vacuous token check"
    model.unload()


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("cache_type", ["fp16", "q4"])
def test_graph_decoder_with_adapters(be, tmp_path, cache_type, batch):
    """GreedyGraphDecoder(loras=...): the module-by-module step, eager and (on the GPU) as one captured graph per token"""
    cfg = lora_cfg()
    q4 = cache_type == "q4"
    model, oracle, plain, loras = build(be, cfg, tmp_path, 2, seed=10 + batch)
    first = np.random.default_rng(batch).integers(0, cfg.vocab_size, size=(batch,))
    for captured in ([False] if be.is_emu else [False, True]):
        cache = (ExLlamaV2Cache_Q4 if q4 else ExLlamaV2Cache)(model, batch_size=batch)
        dec = GreedyGraphDecoder(model, cache, batch_size=batch, loras=loras)
        assert dec.chain is None
        if captured:
            dec.capture()
        dec.reset(torch.from_numpy(first), 0)
        oracle.reset(batch); plain.reset(batch)
        tok, n_conf, moved = first.copy(), 0, 0.0
        for i in range(4):
            dec.run(1, use_graph=captured)
            want = oracle.forward(tok[:, None], q4_cache=q4)[:, -1]
            moved = max(moved, float(np.abs(want - plain.forward(tok[:, None], q4_cache=q4)[:, -1]).max()))
            check_logits(be.n(dec.logits)[:, None, :cfg.vocab_size], want[:, None])
            g = be.n(dec.tokens(i, 1))[:, 0]
            conf = confident(want)
            assert np.array_equal(g[conf], want.argmax(-1)[conf])
            n_conf += int(conf.sum())
            tok = g.copy()
            if q4:                      # follow the device's cache codes (oracle/model.py: q4_adopt), as the Q4 decoder tests do
                for layer in range(cfg.num_hidden_layers):
                    flipped = oracle.q4_adopt(layer, be.n(cache.key_states[layer]), be.n(cache.key_scales[layer]),
                                              be.n(cache.value_states[layer]), be.n(cache.value_scales[layer]), i + 1)
                    assert flipped < 0.01 / (i + 1) + 0.002, (i, layer, flipped)
                    plain.q4_adopt(layer, be.n(cache.key_states[layer]), be.n(cache.key_scales[layer]),
                                   be.n(cache.value_states[layer]), be.n(cache.value_scales[layer]), i + 1)
        assert n_conf >= 1, "vacuous token check"
        assert moved > 10 * LOGIT_TOL, moved
        dec.free()
    model.unload()


def test_unload_restores_the_plain_model_bit_for_bit(be, tmp_path):
    cfg = lora_cfg()
    model, oracle, plain, loras = build(be, cfg, tmp_path, 2, seed=5)
    never = ExLlamaV2(cfg, device=be.device, ext=be.ext).load(synth_checkpoint(cfg, be.device, seed=5))
    ids = torch.from_numpy(np.random.default_rng(5).integers(0, cfg.vocab_size, size=(1, 6)))
    with_l = be.n(model.forward(ids, ExLlamaV2Cache(model, batch_size=1), last_id_only=False, loras=loras)).copy()
    ref = be.n(never.forward(ids, ExLlamaV2Cache(never, batch_size=1), last_id_only=False)).copy()
    assert not np.array_equal(with_l, ref)
    # attached but not listed: the plain launches
    assert np.array_equal(be.n(model.forward(ids, ExLlamaV2Cache(model, batch_size=1), last_id_only=False)), ref)
    for l in loras:
        l.unload()
    assert np.array_equal(be.n(model.forward(ids, ExLlamaV2Cache(model, batch_size=1), last_id_only=False)), ref)
    model.unload(); never.unload()


def test_loader_refusals(be, tmp_path):
    cfg = lora_cfg(num_hidden_layers=1)
    model = ExLlamaV2(cfg, device=be.device, ext=be.ext).load(synth_checkpoint(cfg, be.device, seed=6))
    qv = ("self_attn.q_proj", "self_attn.v_proj")
    pre = "base_model.model.model.layers.0.self_attn.q_proj"
    cases = {
        "fan": (dict(config_extra={"fan_in_fan_out": True}), "fan_in_fan_out"),
        "bias": (dict(extra={pre + ".bias": torch.full((8,), 0.5, dtype=torch.float16)}), "bias"),
        "shape": (dict(extra={pre + ".lora_A.weight": torch.zeros((8, cfg.hidden_size + 32), dtype=torch.float16)}), "shape"),
        "head": (dict(extra={"base_model.model.lm_head.weight": torch.zeros((cfg.vocab_size, cfg.hidden_size), dtype=torch.float16)}), "lm_head"),
    }
    for name, (kw, match) in cases.items():
        d = str(tmp_path / name)
        write_adapter(d, cfg, 1, 8, projections=qv, **kw)
        with pytest.raises(ValueError, match=match):
            ExLlamaV2Lora.from_directory(model, d)
        assert not any(lin.lora_a_tensors or lin.lora_b_tensors for lin in model.linear_modules().values())
    d = str(tmp_path / "rank")
    write_adapter(d, cfg, 1, 257, projections=qv)
    with pytest.raises(RuntimeError, match="256"):
        ExLlamaV2Lora.from_directory(model, d)
    assert not any(lin.lora_a_tensors or lin.lora_b_tensors for lin in model.linear_modules().values())
    model.unload()
