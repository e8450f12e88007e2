"""Sampled decoding with the reference's penalties and token bias on the device: GreedyGraphDecoder.capture_sampled / run_sampled and
SpeculativeGraphDecoder's sampled verification.  Every route -- the sampler inside the eager step, the captured graph (device
only), the uncaptured route, and a hand-made loop that reads the logits back, applies the drop-in's HOST penalty walk (pinned to the
reference by tests/test_sampling.py) and the bias, and samples each row with ext.sample_rows -- must emit identical tokens: all of
them run our own sampler on bit-identical fp32 logits with the same random points, so nothing here needs a margin."""
import os
import sys

import numpy as np
import pytest
import torch

from exllamav2_amd import SpeculativeGraphDecoder
from exllamav2_amd.cache import ExLlamaV2Cache, ExLlamaV2Cache_Q4
from exllamav2_amd.model import ExLlamaV2, GreedyGraphDecoder
from exllamav2_amd.synth import synth_checkpoint
from tests.test_model import tiny_cfg
from tests.test_spec_decoder import forced_with_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dropin"))

DEFAULT = (0.8, 50, 0.8, 0.0)                                        # ExLlamaV2Sampler.Settings(): temperature, top_k, top_p, min_p
DEFAULT_PEN = dict(token_repetition_penalty=1.025, token_repetition_range=-1)            # ... and its repetition penalty
STRONG_PEN = dict(token_repetition_penalty=1.3, token_repetition_range=8, token_repetition_decay=8,
                  token_frequency_penalty=0.3, token_presence_penalty=0.2)
N_TOKENS = 24
_models = {}


def built(be):
    if be.name not in _models:
        cfg = tiny_cfg(num_attention_heads=4, num_key_value_heads=2, intermediate_size=384, vocab_size=1000)
        _models[be.name] = (cfg, ExLlamaV2(cfg, device=be.device, ext=be.ext).load(synth_checkpoint(cfg, be.device, recipe="4.0bpw", seed=11)))
    return _models[be.name]


def prompts_of(cfg, b, seed=5):
    """[b, 42]: 14 tokens three times over -- tokens repeat, and the n-gram drafter finds matches"""
    rng = np.random.default_rng(seed)
    return np.stack([np.tile(rng.integers(0, cfg.vocab_size, size=14), 3) for _ in range(b)])


def randoms_of(n, seed=9):
    return [float(x) for x in np.random.default_rng(seed).random(n).astype(np.float32)]


def host_penalised(lg, seqs, pen, bias):
    """penalties, then bias, as the reference applies them on the host: lg fp32 [rows, vocab], one sequence per row"""
    import exllamav2_ext as dropin
    out = np.ascontiguousarray(lg, dtype=np.float32).copy()
    for r, seq in enumerate(seqs):
        row = torch.from_numpy(out[r:r + 1]).view(1, 1, -1)
        dropin.apply_rep_penalty(torch.from_numpy(np.asarray(seq, dtype=np.int64)[None]), pen.get("token_repetition_penalty", 1.0),
                                 pen.get("token_repetition_range", -1), pen.get("token_repetition_decay", 0),
                                 pen.get("token_frequency_penalty", 0.0), pen.get("token_presence_penalty", 0.0), row)
        if bias is not None:
            dropin.fast_fadd_cpu(row, torch.from_numpy(bias).view(1, 1, -1))
    return out


def sample_host_rows(be, lg, st, rnd):
    """ext.sample_rows on fp32 rows with one point (rows behind the first: the reference's recurrence)"""
    t = be.torch
    tok = t.zeros(lg.shape[0], dtype=t.int32, device=be.device); pr = t.zeros(lg.shape[0], dtype=t.float32, device=be.device)
    be.ext.sample_rows(be.t(lg), st[0], st[1], st[2], st[3], float(rnd), tok, pr)
    return be.n(tok).astype(np.int64)


def plain_decoder(be, prompts, with_prompt=True):
    cfg, model = built(be)
    b, L = prompts.shape
    cache = ExLlamaV2Cache(model, batch_size=b)
    model.forward(torch.from_numpy(prompts[:, :-1]), cache, preprocess_only=True)
    dec = GreedyGraphDecoder(model, cache, batch_size=b)
    if not be.is_emu:
        dec.capture()
    dec.reset(torch.from_numpy(prompts[:, -1]), L - 1, prompt_ids=torch.from_numpy(prompts) if with_prompt else None)
    return cfg, dec


def plain_tokens(be, prompts, route, st, pen, bias, rnds, n=N_TOKENS):
    """int64 [b, n]: the tokens of one route of the plain decoder"""
    cfg, dec = plain_decoder(be, prompts)
    L = prompts.shape[1]
    kw = dict(pen)
    if bias is not None:
        kw["token_bias"] = torch.from_numpy(bias)
    if route in ("eager", "graph"):
        dec.capture_sampled(*st, n_randoms=64, **kw)
        assert (dec._sampled["graph"] is not None) == (not be.is_emu)
        dec.run_sampled(n, *st, randoms=rnds, use_graph=route == "graph", **kw)
    elif route == "uncaptured":
        dec.run_sampled(n, *st, randoms=rnds, use_graph=not be.is_emu, **kw)
    else:
        seqs = [list(prompts[r]) for r in range(prompts.shape[0])]
        for i in range(n):
            dec.run(1, use_graph=False)                                 # the step; its arg-max token is replaced below
            lg = be.n(dec.logits)[:, :cfg.vocab_size].astype(np.float32)
            assert np.array_equal(be.n(dec.history)[:, :L + i], np.asarray(seqs))
            tok = sample_host_rows(be, host_penalised(lg, seqs, pen, bias), st, rnds[i])
            with dec._on_stream():
                dec.ids.copy_(be.t(tok.astype(np.int32)))
                dec.history[:, L + i].copy_(dec.ids)
            for r in range(len(seqs)):
                seqs[r].append(int(tok[r]))
    toks = be.n(dec.tokens(L - 1, n)).astype(np.int64).copy()
    assert np.array_equal(be.n(dec.ids), toks[:, -1]) and int(be.n(dec.cache_seqlens)[0]) == L - 1 + n
    dec.free()
    return toks


def routes(be):
    return ["eager", "uncaptured", "hand"] + ([] if be.is_emu else ["graph"])


def all_routes_agree(be, prompts, st, pen, bias, rnds):
    got = {route: plain_tokens(be, prompts, route, st, pen, bias, rnds) for route in routes(be)}
    for route, toks in got.items():
        assert np.array_equal(toks, got["hand"]), (route, toks, got["hand"])
    return got["hand"]


def test_reference_default_settings(be):
    cfg, _ = built(be)
    prompts, rnds = prompts_of(cfg, 1), randoms_of(N_TOKENS)
    toks = all_routes_agree(be, prompts, DEFAULT, DEFAULT_PEN, None, rnds)
    assert toks.shape == (1, N_TOKENS)


def test_strong_penalties_and_a_banned_token(be):
    cfg, _ = built(be)
    prompts, rnds = prompts_of(cfg, 1), randoms_of(N_TOKENS)
    free = plain_tokens(be, prompts, "eager", DEFAULT, {}, None, rnds)
    banned = int(free[0, 0])
    bias = np.zeros(cfg.vocab_size, dtype=np.float32)
    bias[banned] = -np.inf
    bias[(banned + 1) % cfg.vocab_size] = 0.25
    toks = all_routes_agree(be, prompts, DEFAULT, STRONG_PEN, bias, rnds)
    assert not np.array_equal(toks, free)
    assert banned not in toks


def test_batch_of_two_prompts(be):
    cfg, _ = built(be)
    prompts, rnds = prompts_of(cfg, 2, seed=6), randoms_of(N_TOKENS, seed=10)
    assert not np.array_equal(prompts[0], prompts[1])
    toks = all_routes_agree(be, prompts, DEFAULT, STRONG_PEN, None, rnds)
    assert toks.shape == (2, N_TOKENS) and not np.array_equal(toks[0], toks[1])


def test_unknown_history_is_refused_and_neutral_settings_change_nothing(be):
    cfg, _ = built(be)
    prompts, rnds = prompts_of(cfg, 1), randoms_of(8)
    _, dec = plain_decoder(be, prompts, with_prompt=False)
    with pytest.raises(RuntimeError, match="prompt_ids"):
        dec.run_sampled(4, *DEFAULT, randoms=rnds, use_graph=False, **DEFAULT_PEN)
    dec.capture_sampled(*DEFAULT, n_randoms=16, **DEFAULT_PEN)
    with pytest.raises(RuntimeError, match="prompt_ids"):
        dec.run_sampled(4, *DEFAULT, randoms=rnds, use_graph=False, **DEFAULT_PEN)
    # a window that stays inside what reset() was told is fine: the last token only
    dec.run_sampled(2, *DEFAULT, randoms=rnds, use_graph=False, token_repetition_penalty=1.2, token_repetition_range=1)
    with pytest.raises(RuntimeError, match="first_ids"):
        dec.reset(torch.tensor([3]), 2, prompt_ids=torch.tensor([[1, 2, 4]]))
    with pytest.raises(TypeError, match="unknown setting"):
        dec.run_sampled(1, *DEFAULT, randoms=rnds, token_repetition_penalti=1.1)
    dec.free()
    without = plain_tokens(be, prompts, "eager", DEFAULT, {}, None, rnds, n=8)
    neutral = dict(token_repetition_penalty=1.0, token_repetition_range=-1, token_repetition_decay=0, token_frequency_penalty=0.0,
                   token_presence_penalty=0.0)
    for route in routes(be):
        if route != "hand":
            assert np.array_equal(plain_tokens(be, prompts, route, DEFAULT, neutral, None, rnds, n=8), without), route
    _, dec = plain_decoder(be, prompts)
    dec.capture_sampled(*DEFAULT, **neutral)
    assert dec._sampled["pen"] is None                               # neutral settings: the launches are the ones without them
    dec.free()


# ---- speculative ----------------------------------------------------------------------------------------------------------
K = 3
N_STEPS = 6


def spec_decoder(be, prompt, forced):
    cfg, model = built(be)
    cache = ExLlamaV2Cache(model, batch_size=1)
    model.forward(torch.from_numpy(prompt[None, :-1]), cache, preprocess_only=True)
    if forced is None:
        return cfg, SpeculativeGraphDecoder(model, cache, num_draft_tokens=K, max_ngram=4)
    return cfg, SpeculativeGraphDecoder(model, cache, num_draft_tokens=K, drafter="forced", forced=torch.from_numpy(forced))


def spec_state(be, dec, counter):
    p = dec.sync()
    st = dec.stats()
    return (be.n(dec.history)[:p + 1].tolist(), p, (st["steps"], st["accepted"], st["hist"]), st["emitted"], int(counter),
            be.n(dec.ids).tolist())


def spec_run(be, prompt, forced, route, st, pen, bias, rnds):
    cfg, dec = spec_decoder(be, prompt, forced)
    kw = dict(pen)
    if bias is not None:
        kw["token_bias"] = torch.from_numpy(bias)
    if route in ("eager", "graph"):
        dec.capture_sampled(*st, n_randoms=len(rnds), **kw)
        assert (dec._sampled["graph"] is not None) == (not be.is_emu)
        dec.reset(torch.from_numpy(prompt))
        dec.run_sampled(N_STEPS, *st, randoms=rnds, use_graph=route == "graph", **kw)
        out = spec_state(be, dec, be.n(dec._sampled["counter"])[0])
        dec.free()
        return out
    # the hand-made loop: the decoder's own forward over the K + 1 rows (its greedy tail is undone), everything behind the logits
    # on the host or by one-row launches
    dec.reset(torch.from_numpy(prompt))
    seq = [int(x) for x in prompt]
    c, steps, accepted, hist = 0, 0, 0, [0] * (K + 1)
    for _ in range(N_STEPS):
        p = len(seq) - 1
        ids = be.n(dec.ids).astype(np.int64)
        assert dec.sync() == p and ids[0] == seq[-1]
        dec.run(1, use_graph=False)
        dec.sync()
        lg = be.n(dec.logits)[:, :cfg.vocab_size].astype(np.float32)
        pl = host_penalised(lg, [seq + ids[1:1 + r].tolist() for r in range(K + 1)], pen, bias)
        tok = [int(sample_host_rows(be, pl[r:r + 1], st, rnds[c + r])[0]) for r in range(K + 1)]
        n_acc = 0
        while n_acc < K and ids[n_acc + 1] == tok[n_acc]:
            n_acc += 1
        seq += tok[:n_acc + 1]
        c += n_acc + 1; steps += 1; accepted += n_acc; hist[n_acc] += 1
        with dec._on_stream():
            dec.history.zero_()
            dec.history[:len(seq)].copy_(be.t(np.asarray(seq, dtype=np.int32)))
            dec.cache_seqlens.fill_(len(seq) - 1)
            dec.ids[:1].fill_(seq[-1])
            be.ext.spec_accept_draft(None, dec.ids, dec.history, dec.cache_seqlens, None, dec.K, dec.N, forced=dec.forced, draft_only=True)
        dec.pos = len(seq) - 1
    out = (seq, len(seq) - 1, (steps, accepted, hist), steps + accepted, c, be.n(dec.ids).tolist())
    dec.free()
    return out


def spec_routes_agree(be, prompt, forced, st, pen, bias, rnds):
    got = {route: spec_run(be, prompt, forced, route, st, pen, bias, rnds) for route in ["eager", "hand"] + ([] if be.is_emu else ["graph"])}
    for route, state in got.items():
        assert state == got["hand"], (route, state, got["hand"])
    history, pos, stats, emitted, counter, _ = got["hand"]
    assert emitted == counter == pos - (len(prompt) - 1)             # one random point per emitted token
    return got["hand"]


@pytest.mark.parametrize("plan", ["right", "wrong_from_second", "all_wrong"])
def test_speculative_forced_drafts(be, plan):
    cfg, _ = built(be)
    prompt = prompts_of(cfg, 1)[0]
    rnds = randoms_of(N_STEPS * (K + 1))
    # the unspeculated sampled tokens for the same points: what right drafts are
    toks = plain_tokens(be, prompt[None], "eager", DEFAULT, DEFAULT_PEN, None, rnds + randoms_of(K + 8, seed=1), n=N_STEPS * (K + 1) + K)[0]
    steps = {"right": [K] * N_STEPS, "wrong_from_second": [1] * N_STEPS, "all_wrong": [0] * N_STEPS}[plan]
    forced = forced_with_plan(prompt, toks, K, steps, cfg.vocab_size)
    history, pos, stats, emitted, counter, _ = spec_routes_agree(be, prompt, forced, DEFAULT, DEFAULT_PEN, None, rnds)
    assert stats[0] == N_STEPS
    if plan == "right":
        assert stats[1] >= 1                                         # (the 4-row step's logits may differ from the 1-row step's in the last bit)
    else:
        assert stats[1] < K * N_STEPS


def test_speculative_ngram_drafter_with_strong_penalties_and_bias(be):
    cfg, _ = built(be)
    prompt = prompts_of(cfg, 1)[0]
    rnds = randoms_of(N_STEPS * (K + 1), seed=4)
    bias = np.zeros(cfg.vocab_size, dtype=np.float32)
    bias[int(prompt[0])] = -np.inf
    bias[int(prompt[1])] = 0.5
    history, pos, stats, emitted, counter, _ = spec_routes_agree(be, prompt, None, DEFAULT, STRONG_PEN, bias, rnds)
    assert int(prompt[0]) not in history[len(prompt):]
    spec_routes_agree(be, prompt, None, DEFAULT, DEFAULT_PEN, None, rnds)
    spec_routes_agree(be, prompt, None, DEFAULT, {}, None, rnds)     # no penalties: the sampler reads the fp16 logits directly


def test_speculative_refusals_hold_on_the_sampled_entry(be):
    cfg, model = built(be)
    with pytest.raises(RuntimeError, match="quantized cache"):
        SpeculativeGraphDecoder(model, ExLlamaV2Cache_Q4(model, batch_size=1))
    with pytest.raises(RuntimeError, match="one sequence"):
        SpeculativeGraphDecoder(model, ExLlamaV2Cache(model, batch_size=2))
    dec = SpeculativeGraphDecoder(model, ExLlamaV2Cache(model, batch_size=1), num_draft_tokens=K)
    dec.reset(torch.tensor([1, 2, 3]))
    with pytest.raises(RuntimeError, match="capture_sampled first"):
        dec.run_sampled(1, *DEFAULT)
    dec.capture_sampled(*DEFAULT, n_randoms=8, **DEFAULT_PEN)
    dec.reset(torch.tensor([1, 2, 3]))
    with pytest.raises(RuntimeError, match="settings differ"):
        dec.run_sampled(1, *DEFAULT)
    with pytest.raises(RuntimeError, match="settings differ"):
        dec.run_sampled(1, 0.7, 50, 0.8, 0.0, **DEFAULT_PEN)
    with pytest.raises(RuntimeError, match="random points"):
        dec.run_sampled(3, *DEFAULT, **DEFAULT_PEN)                  # 3 x (K + 1) = 12 > 8
    with pytest.raises(RuntimeError, match="exceed the cache"):
        dec.capture_sampled(*DEFAULT, n_randoms=4096, **DEFAULT_PEN).run_sampled(cfg.max_seq_len // (K + 1), *DEFAULT, **DEFAULT_PEN)
    dec.run_sampled(2, *DEFAULT, **DEFAULT_PEN, use_graph=not be.is_emu)
    assert dec.stats()["steps"] == 2
    dec.free()
