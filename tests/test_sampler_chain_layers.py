"""The host layers around the sampler chain: the settings record has ONE layout (the header's, which csrc/sampling.hip includes)
and the ctypes Structure follows it; SpeculativeGraphDecoder knows none of the chain keywords; the decoder's top-token attributes
follow the buffers a captured step writes."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT

N_TOKENS = 4
BASE = (0.85, 40, 0.9, 0.0)


def test_ctypes_record_has_the_layout_of_the_header(tmp_path):
    from exllamav2_amd._lib import SampleChain
    header = open(os.path.join(ROOT, "include", "exl2_hip.h")).read()
    body = re.search(r"typedef struct exl2_sample_chain\s*\{(.*?)\}\s*exl2_sample_chain;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"\*?\s*([a-z_]+)\s*(?:,|$)", decl.strip())]
    assert names == [f[0] for f in SampleChain._fields_]
    # the sampler's source takes the record from the header, it defines none of its own
    src = open(os.path.join(ROOT, "exllamav2_amd", "csrc", "sampling.hip")).read()
    assert "include/exl2_hip.h" in src and "typedef struct exl2_sample_chain" not in src
    cc = os.environ.get("CC") or shutil.which("cc") or shutil.which("gcc") or shutil.which("clang") or "/opt/rocm/lib/llvm/bin/clang"
    prog = tmp_path / "layout.c"
    lines = "".join(f'    printf("{n} %zu\\n", offsetof(exl2_sample_chain, {n}));\n' for n in names)
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "exl2_hip.h"\nint main(void) {\n'
                    '    printf("sizeof %zu\\n", sizeof(exl2_sample_chain));\n' + lines + "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["sizeof"]) == ctypes.sizeof(SampleChain)
    for n in names:
        assert int(got[n]) == getattr(SampleChain, n).offset, n


@pytest.fixture
def tiny(be):
    from exllamav2_amd.config import ExLlamaV2Config
    from exllamav2_amd.model import ExLlamaV2
    from exllamav2_amd.synth import synth_checkpoint
    cfg = ExLlamaV2Config.tiny_test(max_seq_len=256)
    model = ExLlamaV2(cfg, device=be.device, ext=be.ext).load(synth_checkpoint(cfg, be.device, seed=5))
    yield cfg, model
    model.unload()


def test_speculative_decoder_refuses_every_chain_keyword(be, tiny):
    """it keeps accepting exactly what it accepted before the chain: a chain keyword is an unknown setting, never dropped"""
    from exllamav2_amd.cache import ExLlamaV2Cache
    from exllamav2_amd.model import GreedyGraphDecoder
    from exllamav2_amd.speculative import SpeculativeGraphDecoder
    cfg, model = tiny
    dec = SpeculativeGraphDecoder(model, ExLlamaV2Cache(model, batch_size=1, max_seq_len=256), num_draft_tokens=3)
    values = dict(top_a=0.1, tfs=0.9, typical=0.5, temperature_last=True, smoothing_factor=0.5, min_temp=0.5, max_temp=1.5,
                  temp_exponent=2.0, skew=0.3, mirostat=True, mirostat_tau=2.0, mirostat_eta=0.2, return_top_tokens=4)
    assert set(values) == set(GreedyGraphDecoder.CHAIN_DEFAULTS)
    for k, v in values.items():
        with pytest.raises(TypeError, match=k):
            dec.capture_sampled(*BASE, n_randoms=16, **{k: v})
    with pytest.raises(TypeError, match="mirostat"):
        dec.capture_sampled(*BASE, n_randoms=16, token_repetition_penalty=1.1, mirostat=True, top_a=0.1)
    assert getattr(dec, "_sampled", None) is None and getattr(dec, "mirostat_mu", None) is None and getattr(dec, "top_tokens", None) is None
    dec.free()


def test_top_tokens_follow_the_captured_steps_buffers(be, tiny):
    """capture with K = 4, an uncaptured run with K = 5, then the captured settings again: `top_tokens` is what that step wrote"""
    import torch
    from exllamav2_amd.cache import ExLlamaV2Cache
    from exllamav2_amd.model import GreedyGraphDecoder
    cfg, model = tiny
    graph = be.device != "cpu"
    rnds = [float(x) for x in np.random.default_rng(23).random(3 * N_TOKENS)]

    def decoder():
        dec = GreedyGraphDecoder(model, ExLlamaV2Cache(model, batch_size=2, max_seq_len=256), batch_size=2)
        if graph:
            dec.capture()
        dec.reset(torch.tensor([7, 19]), 0)
        return dec

    dec = decoder()
    dec.capture_sampled(*BASE, n_randoms=16, return_top_tokens=4)
    captured = dec.top_tokens
    dec.run_sampled(N_TOKENS, *BASE, randoms=rnds[:N_TOKENS], use_graph=graph, return_top_tokens=4)
    dec.run_sampled(N_TOKENS, *BASE, randoms=rnds[N_TOKENS:2 * N_TOKENS], use_graph=graph, return_top_tokens=5)
    assert dec.top_tokens.shape[-1] == 5
    dec.run_sampled(N_TOKENS, *BASE, randoms=rnds[2 * N_TOKENS:], use_graph=graph, return_top_tokens=4)
    assert dec.top_tokens is captured and dec.top_tokens.shape[-1] == 4
    got_t, got_p = be.n(dec.top_tokens).copy(), be.n(dec.top_probs).copy()
    assert (got_p[:, 0] > 0).all()
    # the report of the last step: its first entry's probability is the largest, and the sampled token is among the candidates
    # a host launch on the same logits reports
    t = torch.zeros(2, dtype=torch.int32, device=be.device); p = torch.zeros(2, dtype=torch.float32, device=be.device)
    kt = torch.zeros((2, 4), dtype=torch.int32, device=be.device); kp = torch.zeros((2, 4), dtype=torch.float32, device=be.device)
    be.n(dec.ids)
    be.ext.sample_rows_chain(dec.logits, BASE[0], BASE[1], BASE[2], BASE[3], rnds[-1], t, p, vocab=cfg.vocab_size,
                             out_ktokens=kt, out_kprobs=kp)
    assert np.array_equal(be.n(kt), got_t) and np.array_equal(be.n(kp).view(np.uint32), got_p.view(np.uint32))
    dec.free()
