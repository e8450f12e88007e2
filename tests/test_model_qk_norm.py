"""End to end with the q / k head norm (cfg.use_qk_norm: Qwen3-style attention): prefill + decode on the module route, the chained
GreedyGraphDecoder over FP16 (head norm folded into the attention launch, or as a launch of its own) and Q4 caches -- tiny synthetic
models against tests/qk_norm_oracle.QKNormOracleModel.

The bar is check_logits at 1 x, the project's model tolerance, with no row left out.  So that a rounding-point difference cannot be
mistaken for a defect, the checkpoints' seeds are chosen WITH THE ORACLE ALONE (oracle_spread below; never with the device): per case,
the first seed counting up from 0 at which QKNormOracleModel's logits under its two admissible roundings ("reference": fp16 where the
reference's kernels round; "chain": where the chained kernels round) differ by at most 0.5 x that tolerance at every row of every
step of the case.  Checkpoints are drawn on the CPU (torch's CPU and GPU generators differ) and moved to the backend's device, and
every step is fed the oracle's own tokens, so the trajectory a seed was chosen for is the one the test runs.
"""
import numpy as np
import pytest
import torch

from exllamav2_amd.cache import ExLlamaV2Cache, ExLlamaV2Cache_Q4
from exllamav2_amd.model import ExLlamaV2, GreedyGraphDecoder
from exllamav2_amd.synth import synth_checkpoint
from tests.qk_norm_oracle import QKNormOracleModel
from tests.test_model import tiny_cfg, check_logits, confident, LOGIT_TOL


def module_cfg(hd: int, rms: bool, **kw):
    return tiny_cfg(head_dim=hd, use_qk_norm=True, headnorm_rms=rms, **kw)


def chain_cfg(hd: int, rms: bool = True):
    return tiny_cfg(num_attention_heads=4, num_key_value_heads=2, head_dim=hd, intermediate_size=384, use_qk_norm=True, headnorm_rms=rms)


def q4_cfg(hd: int):
    # (kv width = the codec's 512-element block: the cache's direct route, as tests/test_chain.py::test_q4_cache_decodes_on_the_chain)
    return tiny_cfg(num_attention_heads=512 // hd, num_key_value_heads=512 // hd, head_dim=hd, hidden_size=512, intermediate_size=512,
                    use_qk_norm=True)


def first_ids(cfg, seed: int, batch: int, prefill: int):
    return np.random.default_rng(1000 + seed).integers(0, cfg.vocab_size, size=(batch, prefill))


def oracle_run(oracle, ids, steps: int, feed=None, **fw):
    """[(ids of the call, logits)]: the prompt, then `steps` single tokens -- the arg-max of the previous call, or feed[i]"""
    oracle.reset(ids.shape[0])
    out = [(ids, oracle.forward(ids, **fw))]
    for i in range(steps):
        nxt = np.argmax(out[-1][1][:, -1], axis=-1)[:, None] if feed is None else feed[i]
        out.append((nxt, oracle.forward(nxt, **fw)))
    return out


def oracle_spread(cfg, recipe: str, seed: int, batch: int, prefill: int, steps: int) -> float:
    """the seed rule's figure: the largest distance between the oracle's two roundings over the case's trajectory (the tokens are the
    reference rounding's), in units of the model tolerance"""
    ck = synth_checkpoint(cfg, "cpu", recipe=recipe, seed=seed)
    a = oracle_run(QKNormOracleModel(cfg, ck, rounding="reference"), first_ids(cfg, seed, batch, prefill), steps)
    b = oracle_run(QKNormOracleModel(cfg, ck, rounding="chain"), a[0][0], steps, feed=[t for t, _ in a[1:]])
    return max(float((np.abs(wa - wb) / (LOGIT_TOL + np.abs(wa) * 2.0 ** -8)).max()) for (_, wa), (_, wb) in zip(a, b))


def _to_device(ck: dict, device):
    return {k: ({kk: vv.to(device) for kk, vv in v.items()} if isinstance(v, dict) else v.to(device)) for k, v in ck.items()}


def _build(be, cfg, recipe: str, seed: int):
    ck = synth_checkpoint(cfg, "cpu", recipe=recipe, seed=seed)
    oracle = QKNormOracleModel(cfg, ck)                                    # (before load(): it re-lays the tensors out in place)
    model = ExLlamaV2(cfg, device=be.device, ext=be.ext).load(_to_device(ck, be.device))
    assert all(attn.q_norm is not None for attn, _ in model.layers)
    return model, oracle


# seeds by the rule in the module docstring (tools: python -m tests.test_model_qk_norm prints the table)
MODULE_CASES = {   # (hd, rms) -> seed; batch 2, prompt of 5, 2 decode steps
    (64, True): 0, (64, False): 0, (128, True): 0, (128, False): 0,
}
CHUNKED_CASES = {  # rms -> seed; batch 1, prompt of 10 in chunks of 4
    True: 0, False: 0,
}
CHAIN_CASES = {    # (hd, recipe, batch) -> seed; one first token, 3 decode steps
    (64, "4.0bpw", 1): 0, (64, "4.0bpw", 3): 0, (64, "gptq-4bit-128g", 1): 0, (64, "gptq-4bit-128g", 3): 0,
    (128, "4.0bpw", 1): 0, (128, "4.0bpw", 3): 0, (128, "gptq-4bit-128g", 1): 0, (128, "gptq-4bit-128g", 3): 0,
}
Q4_CASES = {       # (hd, recipe, batch) -> seed; one first token, 3 decode steps (the rule is evaluated on the FP16-cache oracle)
    (64, "4.0bpw", 1): 0, (64, "gptq-4bit-128g", 3): 0, (128, "4.0bpw", 3): 0, (128, "gptq-4bit-128g", 1): 0,
}
STEPS = 3


def case_specs():
    """(table name, key, cfg, recipe, batch, prompt length, decode steps) of every seeded case -- what the rule is evaluated on"""
    for (hd, rms) in MODULE_CASES:
        yield "MODULE_CASES", (hd, rms), module_cfg(hd, rms), "4.0bpw", 2, 5, 2
    for rms in CHUNKED_CASES:
        yield "CHUNKED_CASES", rms, module_cfg(64, rms, max_input_len=4), "4.0bpw", 1, 10, 0
    for (hd, recipe, batch) in CHAIN_CASES:
        yield "CHAIN_CASES", (hd, recipe, batch), chain_cfg(hd), recipe, batch, 1, STEPS
    for (hd, recipe, batch) in Q4_CASES:
        yield "Q4_CASES", (hd, recipe, batch), q4_cfg(hd), recipe, batch, 1, STEPS


def test_seeds_follow_the_rule():
    """one case per table re-evaluated here (the whole table: python -m tests.test_model_qk_norm)"""
    tables = {"MODULE_CASES": MODULE_CASES, "CHUNKED_CASES": CHUNKED_CASES, "CHAIN_CASES": CHAIN_CASES, "Q4_CASES": Q4_CASES}
    seen = set()
    for name, key, cfg, recipe, batch, prefill, steps in case_specs():
        if name in seen:
            continue
        seen.add(name)
        seed = tables[name][key]
        assert oracle_spread(cfg, recipe, seed, batch, prefill, steps) <= 0.5
        assert all(oracle_spread(cfg, recipe, s, batch, prefill, steps) > 0.5 for s in range(seed))


# ---- module route -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged"])
@pytest.mark.parametrize("hd,rms", list(MODULE_CASES))
def test_prefill_then_decode_module_route(be, monkeypatch, hd, rms, paged):
    """prompt through the prefill kernels, then decode steps module by module: contiguous cache (model.forward) or paged positions
    read on the device (GreedyGraphDecoder without the chain)"""
    monkeypatch.setenv("EXL2_CHAIN", "0")
    cfg = module_cfg(hd, rms)
    seed = MODULE_CASES[(hd, rms)]
    model, oracle = _build(be, cfg, "4.0bpw", seed)
    want = oracle_run(oracle, first_ids(cfg, seed, 2, 5), 2)
    cache = ExLlamaV2Cache(model, batch_size=2)
    logits = model.forward(torch.from_numpy(want[0][0]), cache, last_id_only=False)
    check_logits(be.n(logits), want[0][1])
    dec = GreedyGraphDecoder(model, cache, batch_size=2) if paged else None
    assert dec is None or dec.chain is None
    n_conf = 0
    for i, (nxt, w) in enumerate(want[1:]):
        if paged:
            dec.reset(torch.from_numpy(nxt[:, 0]), 5 + i)
            dec.run(1, use_graph=False)
            got = be.n(dec.logits)[:, None, :cfg.vocab_size]
        else:
            got = be.n(model.forward(torch.from_numpy(nxt), cache))
        check_logits(got, w)
        conf = confident(w[:, -1])
        assert np.array_equal(got[:, -1].argmax(-1)[conf], w[:, -1].argmax(-1)[conf])
        n_conf += int(conf.sum())
    assert n_conf >= 1, "vacuous token check"
    if dec is not None:
        dec.free()
    model.unload()


@pytest.mark.parametrize("rms", list(CHUNKED_CASES))
def test_chunked_prefill(be, rms):
    cfg = module_cfg(64, rms, max_input_len=4)                              # 10 tokens in chunks of 4, 4, 2
    seed = CHUNKED_CASES[rms]
    model, oracle = _build(be, cfg, "4.0bpw", seed)
    want = oracle_run(oracle, first_ids(cfg, seed, 1, 10), 0)
    cache = ExLlamaV2Cache(model, batch_size=1)
    logits = model.forward(torch.from_numpy(want[0][0]), cache, last_id_only=False)
    check_logits(be.n(logits), want[0][1])
    assert cache.current_seq_len == 10
    model.unload()


# ---- chained decoder ---------------------------------------------------------------------------------------------------------------

def _decode_chained(be, cfg, recipe, batch, seed, cache_cls, q4: bool):
    model, oracle = _build(be, cfg, recipe, seed)
    fp16_oracle = None
    if q4:                                                                  # the tokens of the rule's trajectory: the FP16-cache oracle's
        fp16_oracle = oracle_run(QKNormOracleModel(cfg, synth_checkpoint(cfg, "cpu", recipe=recipe, seed=seed)), first_ids(cfg, seed, batch, 1), STEPS)
    cache = cache_cls(model, batch_size=batch)
    dec = GreedyGraphDecoder(model, cache, batch_size=batch)
    assert dec.chain is not None
    be.ext.chain_route_counts(reset=True)
    if not be.is_emu:
        dec.capture()
    tok = first_ids(cfg, seed, batch, 1)
    oracle.reset(batch)
    n_conf = 0
    for i in range(STEPS + 1):
        dec.reset(torch.from_numpy(tok[:, 0]), i)
        dec.run(1, use_graph=not be.is_emu)
        want = oracle.forward(tok, q4_cache=q4)[:, -1]
        got = be.n(dec.logits)[:, :cfg.vocab_size]
        check_logits(got[:, None], want[:, None])
        g = be.n(dec.tokens(i, 1))[:, 0]
        assert np.array_equal(g, got.argmax(-1))
        conf = confident(want)
        assert np.array_equal(g[conf], want.argmax(-1)[conf])
        n_conf += int(conf.sum())
        if q4:
            # the oracle continues from the codes the device wrote (a 4-bit code flips on a one-ulp difference: tests/test_chain.py)
            for layer in range(cfg.num_hidden_layers):
                flipped = oracle.q4_adopt(layer, be.n(cache.key_states[layer]), be.n(cache.key_scales[layer]),
                                          be.n(cache.value_states[layer]), be.n(cache.value_scales[layer]), i + 1)
                assert flipped < 0.01 / (i + 1) + 0.002, (i, layer, flipped)
            tok = fp16_oracle[i + 1][0] if i < STEPS else tok
        else:
            tok = want.argmax(-1)[:, None]
    assert n_conf >= 1, "no step had a confident oracle margin: the token check would be vacuous"
    assert dec.chain is not None and sum(be.ext.chain_route_counts()) > 0
    dec.free()
    model.unload()


@pytest.mark.parametrize("form", ["fused", "separate"])
@pytest.mark.parametrize("hd,recipe,batch", list(CHAIN_CASES))
def test_chained_decoder_fp16_cache(be, monkeypatch, hd, recipe, batch, form):
    """fused: the norm inside the one-launch attention (csrc/attn_fused_body.h NORM); separate (EXL2_QK_NORM_FUSED=0): a launch of its
    own behind the projections -- the two must not be told apart by the oracle"""
    monkeypatch.setenv("EXL2_QK_NORM_FUSED", "1" if form == "fused" else "0")
    taken = {"fused": 0, "plain": 0}
    inner = be.ext.attn_decode_fused

    def spy(*a, **k):
        taken["fused" if k.get("head_norm") is not None else "plain"] += 1
        return inner(*a, **k)
    monkeypatch.setattr(be.ext, "attn_decode_fused", spy)
    _decode_chained(be, chain_cfg(hd), recipe, batch, CHAIN_CASES[(hd, recipe, batch)], ExLlamaV2Cache, q4=False)
    assert (taken["fused"] > 0) == (form == "fused") and (taken["plain"] > 0) == (form == "separate"), taken


@pytest.mark.parametrize("hd,recipe,batch", list(Q4_CASES))
def test_chained_decoder_q4_cache(be, hd, recipe, batch):
    """quantized cache: the norm stays a launch of its own ahead of the one-launch attention of csrc/attn_q4.hip"""
    _decode_chained(be, q4_cfg(hd), recipe, batch, Q4_CASES[(hd, recipe, batch)], ExLlamaV2Cache_Q4, q4=True)


def test_checkpoints_without_the_norm_are_unchanged():
    """the norm weights come from a generator of their own: every other tensor of a layer is the same draw with and without them"""
    a = synth_checkpoint(tiny_cfg(), "cpu", seed=3)
    b = synth_checkpoint(tiny_cfg(use_qk_norm=True), "cpu", seed=3)
    assert set(b) - set(a) == {f"model.layers.{i}.self_attn.{n}" for i in range(2) for n in ("q_norm", "k_norm")}
    for k, v in a.items():
        for x, y in (zip(v.values(), b[k].values()) if isinstance(v, dict) else [(v, b[k])]):
            assert torch.equal(x, y), k
    qn = b["model.layers.0.self_attn.q_norm"]
    assert qn.shape == (2, 64) and qn.dtype == torch.float16 and not torch.equal(qn[0], qn[1])


if __name__ == "__main__":
    # the seed tables by the rule: for every case the first seed from 0 whose two oracle roundings stay within 0.5 x the tolerance
    for name, key, cfg, recipe, batch, prefill, steps in case_specs():
        seed, tried = 0, []
        while True:
            s = oracle_spread(cfg, recipe, seed, batch, prefill, steps)
            tried.append(round(s, 3))
            if s <= 0.5:
                break
            seed += 1
        print(f"{name}[{key!r}] = {seed}    # spreads from seed 0: {tried}", flush=True)
