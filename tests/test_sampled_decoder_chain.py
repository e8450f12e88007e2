"""GreedyGraphDecoder with the rest of the reference's sampler chain inside the decode step (capture_sampled / run_sampled with the
reference Settings' names; csrc/sampling.hip CHAIN, exl2_sample_rows_chain_step)."""
import numpy as np
import pytest

N_TOKENS = 8
CHAIN = dict(mirostat=True, mirostat_tau=2.0, mirostat_eta=0.3, temperature_last=True, top_a=0.05, return_top_tokens=4)
BASE = (0.85, 40, 0.9, 0.0)                                  # temperature, top_k, top_p, min_p


@pytest.fixture
def tiny(be):
    import torch
    from exllamav2_amd.cache import ExLlamaV2Cache
    from exllamav2_amd.config import ExLlamaV2Config
    from exllamav2_amd.model import ExLlamaV2, GreedyGraphDecoder
    from exllamav2_amd.synth import synth_checkpoint
    cfg = ExLlamaV2Config.tiny_test(max_seq_len=256)
    model = ExLlamaV2(cfg, device=be.device, ext=be.ext).load(synth_checkpoint(cfg, be.device, seed=5))

    def decoder():
        cache = ExLlamaV2Cache(model, batch_size=2, max_seq_len=256)
        dec = GreedyGraphDecoder(model, cache, batch_size=2)
        if be.device != "cpu":
            dec.capture()
        dec.reset(torch.tensor([7, 19]), 0)
        return dec

    yield cfg, decoder
    model.unload()


def rnds(n=N_TOKENS):
    rng = np.random.default_rng(17)
    return [float(x) for x in rng.random(n)]


def test_captured_chain_step_equals_eager_steps_and_a_host_loop(be, tiny):
    cfg, decoder = tiny
    torch = be.torch
    graph = be.device != "cpu"
    runs = []
    for use_graph in (graph, False):
        dec = decoder()
        dec.capture_sampled(*BASE, n_randoms=16, **CHAIN)
        assert float(dec.mirostat_mu.abs().sum()) == 0.0                    # reset by capture_sampled
        dec.run_sampled(N_TOKENS, *BASE, randoms=rnds(), use_graph=use_graph, **CHAIN)
        runs.append((be.n(dec.tokens(0, N_TOKENS)).copy(), be.n(dec.mirostat_mu).view(np.uint32).copy(),
                     be.n(dec.top_tokens).copy(), be.n(dec.top_probs).view(np.uint32).copy()))
        dec.free()
    for a, b in zip(*runs):
        assert np.array_equal(a, b)
    assert (runs[0][1] != 0).all()                                            # mu moved off "not initialised"

    # the same tokens from a host loop of sample_rows_chain calls on each step's logits (one captured token per call so that
    # the logits of every step can be read)
    dec = decoder()
    dec.capture_sampled(*BASE, n_randoms=16, **CHAIN)
    mu = torch.zeros(2, dtype=torch.float32, device=be.device)
    kt = torch.zeros((2, 4), dtype=torch.int32, device=be.device); kp = torch.zeros((2, 4), dtype=torch.float32, device=be.device)
    t = torch.zeros(2, dtype=torch.int32, device=be.device); p = torch.zeros(2, dtype=torch.float32, device=be.device)
    for i, rnd in enumerate(rnds()):
        dec.run_sampled(1, *BASE, randoms=[rnd], use_graph=graph, **CHAIN)
        be.n(dec.ids)                                                         # (the decoder runs on its own stream: wait for the step)
        be.ext.sample_rows_chain(dec.logits, 1.0, BASE[1], BASE[2], BASE[3], rnd, t, p, vocab=cfg.vocab_size, top_a=CHAIN["top_a"],
                                 post_temperature=BASE[0], mirostat=True, mirostat_tau=CHAIN["mirostat_tau"],
                                 mirostat_eta=CHAIN["mirostat_eta"], mirostat_mu=mu, out_ktokens=kt, out_kprobs=kp)
        assert np.array_equal(be.n(t), be.n(dec.tokens(i, 1))[:, 0]), i
        assert np.array_equal(be.n(t), runs[0][0][:, i]), i
        assert np.array_equal(be.n(mu).view(np.uint32), be.n(dec.mirostat_mu).view(np.uint32)), i
    assert np.array_equal(be.n(kt), runs[0][2]) and np.array_equal(be.n(kp).view(np.uint32), runs[0][3])
    dec.free()


def test_neutral_chain_settings_are_todays_run_sampled(be, tiny):
    cfg, decoder = tiny
    graph = be.device != "cpu"
    outs = []
    for kw in ({}, dict(top_a=0.0, tfs=1.0, typical=0.0, temperature_last=False, smoothing_factor=0.0, skew=0.0, mirostat=False,
                        return_top_tokens=0)):
        for captured in ((True, False) if kw else (True,)):
            dec = decoder()
            if captured:
                dec.capture_sampled(*BASE, n_randoms=16, **kw)
                assert dec._sampled["chain"] is None                          # the same launches as without the settings
            dec.run_sampled(N_TOKENS, *BASE, randoms=rnds(), use_graph=graph, **kw)
            outs.append(be.n(dec.tokens(0, N_TOKENS)).copy())
            dec.free()
    for o in outs[1:]:
        assert np.array_equal(outs[0], o)


def test_uncaptured_route_and_unknown_settings(be, tiny):
    """run_sampled without capture_sampled launches the chain behind each step; mu carries over between calls"""
    cfg, decoder = tiny
    graph = be.device != "cpu"
    dec = decoder()
    dec.capture_sampled(*BASE, n_randoms=16, **CHAIN)
    dec.run_sampled(N_TOKENS, *BASE, randoms=rnds(), use_graph=graph, **CHAIN)
    want = be.n(dec.tokens(0, N_TOKENS)).copy(), be.n(dec.mirostat_mu).view(np.uint32).copy()
    dec.free()
    dec = decoder()
    r = rnds()
    dec.run_sampled(5, *BASE, randoms=r[:5], use_graph=graph, **CHAIN)
    dec.run_sampled(N_TOKENS - 5, *BASE, randoms=r[5:], use_graph=graph, **CHAIN)
    assert np.array_equal(be.n(dec.tokens(0, N_TOKENS)), want[0])
    assert np.array_equal(be.n(dec.mirostat_mu).view(np.uint32), want[1])
    with pytest.raises(TypeError):
        dec.run_sampled(1, *BASE, randoms=[0.5], no_such_setting=1)
    with pytest.raises(RuntimeError, match="partial order"):
        dec.run_sampled(1, *BASE, randoms=[0.5], use_graph=graph, typical=0.5, return_top_tokens=3)
    dec.free()
