"""LayerNorm models through the drop-in: `layer_norm` / `layer_norm_` (ext_norm.cpp), and the UNMODIFIED reference loading a synthetic
StarCoder2 and a synthetic Cohere model directory (its ExLlamaV2LayerNorm and ExLlamaV2ParallelDecoder modules, module handles made with
layernorm_is_rms = False resp. without norm and residual) and playing its greedy loop on dropin/exllamav2_ext.py -> libexl2_hip.so,
logits against tests/layernorm_oracle.LayerNormOracleModel.  Three routes: the compiled binding, the ctypes route, and the compiled
binding with the module chain's self-check on (EXL2_MODULE_CHAIN_VERIFY=1: every hand-off is re-derived and a mismatch raises).

Where the reference package comes from: as tests/test_dropin_reference.py::_reference_pkg; absent -> skipped."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.conftest import ROOT
from tests.test_dropin_reference import _reference_pkg, _dropin
from tests import layernorm_oracle as LO
from tests.test_model_layernorm import CASES


@pytest.mark.gpu
def test_layer_norm_through_the_dropin():
    """the drop-in's layer_norm / layer_norm_ are real: with and without bias, in place, against the restatement at one fp16 ulp"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    E = _dropin()
    from exllamav2_amd.ext import none_tensor
    rng = np.random.default_rng(0)
    x = (rng.standard_normal((3, 136)) * 3 + 1).astype(np.float16)
    w = (1 + 0.2 * rng.standard_normal(136)).astype(np.float16)
    b = (0.5 * rng.standard_normal(136)).astype(np.float16)
    dev = lambda a: torch.from_numpy(a.copy()).to("cuda:0")
    for bias in (None, b):
        want, tol = LO.layer_norm_tol(x, w, bias, 1e-5)
        y = torch.zeros((3, 136), dtype=torch.float16, device="cuda:0")
        E.layer_norm(dev(x), dev(w), none_tensor if bias is None else dev(bias), y, 1e-5)
        assert np.all(np.abs(y.cpu().numpy().astype(np.float64) - want.astype(np.float64)) <= tol)
        xt = dev(x)
        E.layer_norm_(xt, dev(w), none_tensor if bias is None else dev(bias), 1e-5)
        assert torch.equal(xt, y)


def test_layer_norm_is_no_longer_out_of_scope():
    try:
        E = _dropin()
    except Exception as e:                                      # the drop-in binds libexl2_hip.so at import
        pytest.skip(f"drop-in not importable here: {e}")
    x, w = torch.zeros((2, 64), dtype=torch.float16), torch.ones((64,), dtype=torch.float16)
    with pytest.raises(RuntimeError, match="no CPU path"):       # a CPU tensor reaches the binding's own check: the name is served
        E.layer_norm(x, w, w, x.clone(), 1e-5)
    with pytest.raises(RuntimeError, match="no CPU path"):
        E.layer_norm_(x, w, w, 1e-5)


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["exl2_fast", "ctypes", "exl2_fast-selfcheck"])
@pytest.mark.parametrize("case", ["starcoder2-hd64", "cohere-hd64"])
def test_unmodified_reference_runs_layernorm_models_on_the_dropin(tmp_path, case, route):
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
                          vocab_size=320, max_seq_len=256, max_input_len=32, arch=case.split("-")[0], **CASES[case])
    # down_proj keeps its own act-order where the MLP has no biases (as tests/test_dropin_gemma.py).  With one, the reference's loader
    # re-orders the columns of up_proj's weights and scales to down_proj's order (mlp.py:162-164 -> linear.py:156-158) but leaves up_proj's
    # bias as it was: a biased MLP with an act-ordered down_proj is outside what the reference host computes correctly, whatever extension
    # serves it
    ck = synth_checkpoint(cfg, "cpu", seed=0, down_act_order=not cfg.mlp_bias)
    oracle = LO.LayerNormOracleModel(cfg, ck)
    model_dir = write_model_dir(str(tmp_path / "model"), cfg, ck)
    out = str(tmp_path / "out.npz")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "dropin"), ROOT, ref]),
               EXL2_DROPIN_FAST="0" if route == "ctypes" else "1", EXL2_MODULE_CHAIN_VERIFY="1" if route.endswith("selfcheck") else "0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_reference_dropin.py"), model_dir, out, "layernorm"],
                       env=env, capture_output=True, text=True, cwd=str(tmp_path), timeout=900)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    got = np.load(out)
    ids = np.array([list(GEMMA_PROMPT)])
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
