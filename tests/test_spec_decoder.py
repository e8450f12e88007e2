"""SpeculativeGraphDecoder (exllamav2_amd/speculative.py) against the float64 oracle, teacher-forced on the device's own tokens:
every verify step's kept rows, the accept bookkeeping, the stale rows a rejection leaves, the page boundary, the un-chained route,
capture(), the n-gram drafter end to end, and the shapes the decoder refuses."""
import numpy as np
import pytest
import torch

from exllamav2_amd import SpeculativeGraphDecoder
from exllamav2_amd.cache import ExLlamaV2Cache, ExLlamaV2Cache_Q4
from exllamav2_amd.model import ExLlamaV2, GreedyGraphDecoder
from exllamav2_amd.synth import synth_checkpoint
from oracle.model import OracleModel
from tests.test_model import LOGIT_TOL, tiny_cfg, check_logits, confident

_models = {}


def built(be, **cfg_kw):
    """(cfg, oracle, model) of the test configuration, made once per backend and shared (nothing in it changes)"""
    key = (be.name, tuple(sorted(cfg_kw.items())))
    if key not in _models:
        cfg = tiny_cfg(**(dict(num_attention_heads=4, num_key_value_heads=2, intermediate_size=384) | cfg_kw))
        ck = synth_checkpoint(cfg, be.device, recipe="4.0bpw", seed=11)
        oracle = OracleModel(cfg, ck)
        _models[key] = (cfg, oracle, ExLlamaV2(cfg, device=be.device, ext=be.ext).load(ck))
    return _models[key]


def prefilled(be, model, prompt):
    cache = ExLlamaV2Cache(model, batch_size=1)
    if len(prompt) > 1:
        model.forward(torch.from_numpy(np.asarray(prompt[:-1])[None]), cache, preprocess_only=True)
    return cache


def plain_greedy(be, model, prompt, n, cache=None):
    """the tokens of the plain one-row decoder behind the prompt (it writes cache rows behind the prompt's only)"""
    cache = cache or prefilled(be, model, prompt)
    dec = GreedyGraphDecoder(model, cache, batch_size=1)
    if not be.is_emu:
        dec.capture()
    dec.reset(torch.tensor([int(prompt[-1])]), len(prompt) - 1)
    dec.run(n, use_graph=not be.is_emu)
    toks = be.n(dec.tokens(len(prompt) - 1, n))[0].astype(np.int64).copy()
    dec.free()
    return toks


def forced_with_plan(prompt, toks, K, plan, vocab):
    """forced tokens (by sequence index) = the true continuation, with draft index c of step t made wrong for c = plan[t] < K
    (c == K: the step's drafts are all right) -- so step t accepts plan[t] drafts"""
    forced = np.concatenate([np.asarray(prompt, dtype=np.int64), toks])
    L = len(prompt)
    for c in plan:
        if c < K:
            forced[L + c] = (forced[L + c] + 1) % vocab
        L += c + 1
    assert L + K <= len(forced), "record more plain tokens"
    return forced


def run_checked(be, cfg, oracle, dec, prompt, n_steps):
    """n_steps verify steps, each checked alone: the kept rows' logits against the oracle teacher-forced on the device's own tokens,
    the emitted tokens against the device's logits and (where the oracle is confident) the oracle's, the position, the counters.
    Returns (emitted tokens, confident flags, accepted counts)."""
    K = dec.K
    oracle.reset(1)
    if len(prompt) > 1:
        oracle.forward(np.asarray(prompt[:-1])[None])
    p = len(prompt) - 1
    emitted, conf_all, accs = [], [], []
    hist = np.zeros((K + 1,), dtype=np.int64)
    for t in range(n_steps):
        dec.run(1, use_graph=not be.is_emu)
        p1 = dec.sync()
        n_acc = p1 - p - 1
        assert 0 <= n_acc <= K, (p, p1)
        seq = be.n(dec.history)[:p1 + 1].astype(np.int64)
        inp, out = seq[p:p1], seq[p + 1:p1 + 1]
        oracle.seq_len = p                                   # the rows a rejection left behind are rewritten, as on the device
        want = oracle.forward(inp[None])[0]
        got = be.n(dec.logits)[:n_acc + 1, :cfg.vocab_size]
        check_logits(got[None], want[None])
        assert np.array_equal(out, got.argmax(-1))           # the device emits the arg-max of its own logits
        conf = confident(want)
        assert np.array_equal(out[conf], want.argmax(-1)[conf])
        hist[n_acc] += 1
        st = dec.stats()
        assert (st["steps"], st["accepted"], st["hist"]) == (t + 1, int(sum(accs)) + n_acc, hist.tolist())
        assert int(be.n(dec.ids)[0]) == out[-1]
        emitted += out.tolist(); conf_all += conf.tolist(); accs.append(n_acc)
        p = p1
    assert sum(conf_all) >= 1, "no position had a confident oracle margin: the token check would be vacuous"
    return np.array(emitted), np.array(conf_all), accs


def oracle_greedy(oracle, prompt, n):
    """the oracle's own greedy continuation: drafts for a test whose checks do not depend on which of them are accepted"""
    oracle.reset(1)
    w = oracle.forward(np.asarray(prompt)[None])[0, -1]
    toks = []
    for _ in range(n):
        toks.append(int(np.argmax(w)))
        w = oracle.forward(np.array([[toks[-1]]]))[0, -1]
    return np.array(toks, dtype=np.int64)


def make_forced(be, K, plan, prompt_len=5, seed=3, toks=None, from_oracle=False, **cfg_kw):
    """a decoder with forced drafts behind a prefilled prompt: the plain decoder's tokens (one prefill serves both decoders),
    made wrong where the plan says"""
    cfg, oracle, model = built(be, **cfg_kw)
    prompt = np.random.default_rng(seed).integers(0, cfg.vocab_size, size=prompt_len)
    cache = prefilled(be, model, prompt)
    n = sum(c + 1 for c in plan) + K
    if toks is None:
        toks = oracle_greedy(oracle, prompt, n) if from_oracle else plain_greedy(be, model, prompt, n, cache)
    forced = forced_with_plan(prompt, toks, K, plan, cfg.vocab_size)
    dec = SpeculativeGraphDecoder(model, cache, num_draft_tokens=K, drafter="forced", forced=torch.from_numpy(forced))
    return cfg, oracle, dec, prompt, toks


@pytest.mark.parametrize("K", [3, 7])
def test_forced_drafts_every_acceptance_length(be, K):
    """(K = 3: the <= 4-row form of the lean kernel, K = 7: its ROWS form)"""
    plan = [t % (K + 1) for t in range(K + 1)] + [K]
    cfg, oracle, dec, prompt, toks = make_forced(be, K, plan)
    assert dec.chain is not None
    if not be.is_emu:
        dec.capture()
    dec.reset(torch.from_numpy(prompt))
    emitted, conf, accs = run_checked(be, cfg, oracle, dec, prompt, len(plan))
    assert dec.chain is not None
    assert all(h > 0 for h in dec.stats()["hist"]), (accs, plan)
    # greedy verification: the emitted tokens are the plain decoder's, up to the first position the oracle is not sure of
    first = int(np.argmin(conf)) if not conf.all() else len(conf)
    assert np.array_equal(emitted[:first], toks[:first])
    dec.free()


def test_rejected_rows_leave_nothing_behind(be):
    K = 3
    cfg, oracle, dec, prompt, _ = make_forced(be, K, [0, K])
    if not be.is_emu:
        dec.capture()
    dec.reset(torch.from_numpy(prompt))
    _, _, accs = run_checked(be, cfg, oracle, dec, prompt, 2)
    assert accs == [0, K]                                    # the second step's four rows sat on the first step's rejected ones
    dec.free()


def test_rows_across_the_page_boundary(be):
    K = 3
    plan = [K, 0, 1, K, 2, K]
    cfg, oracle, dec, prompt, _ = make_forced(be, K, plan, prompt_len=255, from_oracle=True, max_seq_len=512)
    assert dec.chain is not None
    if not be.is_emu:
        dec.capture()
    dec.reset(torch.from_numpy(prompt))                      # the first step's rows sit at positions 254 .. 257
    run_checked(be, cfg, oracle, dec, prompt, len(plan))
    dec.free()


def test_unchained_route(be, monkeypatch):
    K = 3
    plan = [t % (K + 1) for t in range(K + 2)]
    cfg, oracle, dec, prompt, toks = make_forced(be, K, plan)
    dec.reset(torch.from_numpy(prompt))
    chained, conf_c, _ = run_checked(be, cfg, oracle, dec, prompt, len(plan))
    monkeypatch.setenv("EXL2_CHAIN", "0")
    cfg, oracle, dec2, prompt, _ = make_forced(be, K, plan, toks=toks)
    assert dec2.chain is None and dec.chain is not None
    if not be.is_emu:
        dec2.capture()
    dec2.reset(torch.from_numpy(prompt))
    plain, conf_p, _ = run_checked(be, cfg, oracle, dec2, prompt, len(plan))
    n = min(len(chained), len(plain))
    first = int(np.argmin((conf_c[:n] & conf_p[:n]))) if not (conf_c[:n] & conf_p[:n]).all() else n
    assert first >= 1 and np.array_equal(chained[:first], plain[:first])
    dec.free(); dec2.free()


def test_rows_the_attention_launch_declines_take_the_module_route(be):
    """8 rows x 8 query heads per kv head = 64 query rows per kv head: beyond the one-launch attention (32), so the chain declines and
    the step runs module by module -- never something else"""
    K = 7
    cfg, oracle, dec, prompt, _ = make_forced(be, K, [K, 2, 0], from_oracle=True, num_attention_heads=8, num_key_value_heads=1)
    assert dec.chain is not None                             # (the decision falls at the first step: warm-up or eager)
    if not be.is_emu:
        dec.capture()
    dec.reset(torch.from_numpy(prompt))
    run_checked(be, cfg, oracle, dec, prompt, 3)
    assert dec.chain is None
    dec.free()


def test_capture_disturbs_nothing(be):
    if be.is_emu:
        pytest.skip("graph capture needs the device")
    K = 3
    cfg, oracle, dec, prompt, toks = make_forced(be, K, [K], prompt_len=9)
    dec.reset(torch.from_numpy(prompt))
    dec.run(1, use_graph=False)
    dec.sync()
    want = be.n(dec.logits).copy()
    want_hist = be.n(dec.history).copy()
    cfg, oracle, dec2, prompt, _ = make_forced(be, K, [K], prompt_len=9, toks=toks)
    dec2.reset(torch.from_numpy(prompt))
    dec2.capture()                                           # after the prompt and the reset: ids, pos, stats, log and K/V must survive
    dec2.run(1)
    dec2.sync()
    assert np.array_equal(be.n(dec2.logits).view(np.uint16), want.view(np.uint16))
    assert np.array_equal(be.n(dec2.history), want_hist) and dec2.stats()["steps"] == 1
    dec.free(); dec2.free()


def test_ngram_drafter_end_to_end(be):
    cfg, oracle, model = built(be)
    rng = np.random.default_rng(5)
    prompt = np.tile(rng.integers(0, cfg.vocab_size, size=12), 4)
    L, n = len(prompt), 24
    cache = prefilled(be, model, prompt)
    plain = plain_greedy(be, model, prompt, n, cache)
    dec = SpeculativeGraphDecoder(model, cache, num_draft_tokens=3, max_ngram=4)
    if not be.is_emu:
        dec.capture()
    dec.reset(torch.from_numpy(prompt))
    out = be.n(dec.generate(n)).astype(np.int64)
    assert out.shape == (n,)
    st = dec.stats()
    assert st["emitted"] == dec.sync() - (L - 1) >= n and st["steps"] <= n
    assert st["tokens_per_step"] == st["emitted"] / st["steps"]
    oracle.reset(1)
    want = oracle.forward(np.concatenate([prompt, out[:-1]])[None])[0, L - 1:]
    # the device picks the arg-max of logits that are each within one tolerance of the oracle's: the oracle's value of the
    # token it picked is within two tolerances of the oracle's maximum
    picked = want[np.arange(n), out]
    tol2 = (LOGIT_TOL + np.abs(want.max(axis=-1)) * 2.0 ** -8) + (LOGIT_TOL + np.abs(picked) * 2.0 ** -8)
    assert np.all(want.max(axis=-1) - picked <= tol2), float((want.max(axis=-1) - picked).max())
    conf = confident(want)
    assert conf.sum() >= 1 and np.array_equal(out[conf], want.argmax(-1)[conf])
    first = int(np.argmin(conf)) if not conf.all() else n
    assert np.array_equal(out[:first], plain[:first])
    dec.free()


def test_refusals(be):
    cfg, oracle, model = built(be)
    with pytest.raises(RuntimeError, match="quantized cache"):
        SpeculativeGraphDecoder(model, ExLlamaV2Cache_Q4(model, batch_size=1))
    with pytest.raises(RuntimeError, match="one sequence"):
        SpeculativeGraphDecoder(model, ExLlamaV2Cache(model, batch_size=2))
    cache = ExLlamaV2Cache(model, batch_size=1)
    with pytest.raises(RuntimeError, match="17 rows"):
        SpeculativeGraphDecoder(model, cache, num_draft_tokens=16)
    with pytest.raises(RuntimeError, match="forced"):
        SpeculativeGraphDecoder(model, cache, drafter="forced")
    from tests.test_model_gemma import gemma_cfg
    gcfg = gemma_cfg("gemma2-hd64")
    gemma = ExLlamaV2(gcfg, device=be.device, ext=be.ext).load(synth_checkpoint(gcfg, be.device, recipe="4.0bpw", seed=1))
    with pytest.raises(RuntimeError, match="fp32 residual stream"):
        SpeculativeGraphDecoder(gemma, ExLlamaV2Cache(gemma, batch_size=1))
    gemma.unload()
    dec = SpeculativeGraphDecoder(model, cache)
    dec.reset(torch.tensor([1, 2, 3]))
    with pytest.raises(RuntimeError, match="exceed the cache"):
        dec.run(cfg.max_seq_len)
    with pytest.raises(RuntimeError, match="sampling with speculation"):
        dec.run_sampled(1, 1.0, 40)
    dec.free()
