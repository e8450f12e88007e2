"""Gemma-2 through the drop-in: `softcap_` (ext_element.cpp:28-50), and the UNMODIFIED reference loading a synthetic Gemma-2 model
directory (fp32 residual stream, post norms, GELU, scaled embedding, sliding window, both soft caps) and playing its greedy loop on
dropin/exllamav2_ext.py -> libexl2_hip.so, logits against tests/gemma_oracle.GemmaOracleModel.

Where the reference package comes from: as tests/test_dropin_reference.py::_reference_pkg; absent -> skipped."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.conftest import ROOT
from tests.test_dropin_reference import _reference_pkg, _dropin
from tests import gemma_oracle as GO


@pytest.mark.gpu
def test_softcap_through_the_dropin():
    """the drop-in's softcap_ is real: float and half in place, any other dtype refused as the reference refuses it"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    E = _dropin()
    rng = np.random.default_rng(0)
    x = (rng.standard_normal(333) * 40).astype(np.float32)
    for dtype, np_dtype in ((torch.float32, np.float32), (torch.float16, np.float16)):
        t = torch.from_numpy(x.astype(np_dtype)).to("cuda:0")
        E.softcap_(t, 30.0)
        want = GO.softcap(x.astype(np_dtype), 30.0)
        got = t.cpu().numpy().astype(np.float64)
        assert np.all(np.abs(got - want) <= (2.0 ** -20 if dtype == torch.float32 else 2.0 ** -10) * np.abs(want) + 1e-7)
    with pytest.raises(RuntimeError, match="wrong dtype"):
        E.softcap_(torch.zeros(8, dtype=torch.bfloat16, device="cuda:0"), 30.0)


def test_softcap_is_no_longer_out_of_scope():
    try:
        E = _dropin()
    except Exception as e:                                      # the drop-in binds libexl2_hip.so at import
        pytest.skip(f"drop-in not importable here: {e}")
    with pytest.raises(RuntimeError, match="no CPU path"):       # a CPU tensor reaches the binding's own check: the name is served
        E.softcap_(torch.zeros(8), 30.0)


@pytest.mark.gpu
@pytest.mark.parametrize("fast", ["1", "0"], ids=["exl2_fast", "ctypes"])
def test_unmodified_reference_runs_gemma2_on_the_dropin(tmp_path, fast):
    ref = _reference_pkg()
    if ref is None:
        pytest.skip("no copy of the reference's host package on this machine")
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    from exllamav2_amd.config import ExLlamaV2Config
    from exllamav2_amd.synth import synth_checkpoint
    from exllamav2_amd.synth_dir import write_model_dir
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        from run_reference_dropin import GEMMA_PROMPT
    finally:
        sys.path.pop(0)
    cfg = ExLlamaV2Config(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                          head_dim=64, vocab_size=320, max_seq_len=256, max_input_len=32, norm_eps=1e-6, arch="gemma2",
                          residual_fp32=True, post_norms=True, norm_constant_bias=1.0, normalize_embeddings=True, mlp_act_func="gelu",
                          attn_logit_softcapping=50.0, final_logit_softcapping=30.0, query_pre_attn_scalar=100.0, sliding_window=8,
                          alternating_swa=True)
    ck = synth_checkpoint(cfg, "cpu", seed=0, down_act_order=True)
    oracle = GO.GemmaOracleModel(cfg, ck)
    model_dir = write_model_dir(str(tmp_path / "model"), cfg, ck)
    out = str(tmp_path / "out.npz")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "dropin"), ROOT, ref]), EXL2_DROPIN_FAST=fast)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_reference_dropin.py"), model_dir, out, "gemma"],
                       env=env, capture_output=True, text=True, cwd=str(tmp_path), timeout=900)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    got = np.load(out)
    ids = np.array([list(GEMMA_PROMPT)])
    assert ids.shape[1] - 1 > cfg.sliding_window                  # the window clips inside the prompt
    oracle.reset(1)
    want = oracle.forward(ids)
    tol = lambda w: 0.03 + np.abs(w) * 2.0 ** -8
    g = got["prefill"][..., :cfg.vocab_size].astype(np.float64)
    print("prefill max err/tol", float((np.abs(g - want) / tol(want)).max()))
    assert np.all(np.abs(g - want) <= tol(want))
    n_conf = 0
    for i, tok in enumerate(got["tokens"]):
        top2 = np.sort(want[0, -1])[-2:]
        if top2[1] - top2[0] > 0.12:
            assert int(tok) == int(np.argmax(want[0, -1])), i
            n_conf += 1
        want = oracle.forward(np.array([[int(tok)]]))
        g = got["steps"][:, i:i + 1, :cfg.vocab_size].astype(np.float64)
        assert np.all(np.abs(g - want) <= tol(want)), i
    assert n_conf >= 1, "vacuous token check"
