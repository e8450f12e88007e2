"""Qwen3-MoE through the drop-in: the UNMODIFIED reference (architecture.py:450-466 Qwen3MoeForCausalLM, moe_mlp.py) loading a synthetic
Qwen3-MoE model directory (128 experts, top 8, q / k head norm) and running on dropin/exllamav2_ext.py -> libexl2_hip.so: a prompt of six
rows (the reference's torch loop over the experts), single-token steps (`ext_c.q_moe_mlp_forward_` at one row: the pair-job route) and
one call of three rows -- which the drop-in computes as forward_torch (moe_mlp.py:255-323) does for EVERY row; the reference's own
kernel launches only the experts of row 0 there (q_mlp.cu:403-435).  Logits against tests/qwen3_moe_oracle.Qwen3MoeOracleModel under
its router-gap rule (tests/test_model_qwen3_moe.py).

Where the reference package comes from: as tests/test_dropin_reference.py::_reference_pkg; absent -> skipped."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.conftest import ROOT
from tests.test_dropin_reference import _reference_pkg
from tests.test_model_qwen3_moe import _cfg, GAP
from tests.qwen3_moe_oracle import Qwen3MoeOracleModel


def test_qwen3_moe_model_dir_is_written_in_the_reference_form(tmp_path):
    """the directory's names: config.json of Qwen3MoeForCausalLM, .mlp.experts.{e}.gate_proj | up_proj | down_proj, .mlp.gate, the head norms"""
    import json
    from safetensors import safe_open
    from exllamav2_amd.synth import synth_checkpoint
    from exllamav2_amd.synth_dir import write_model_dir
    cfg = _cfg(num_hidden_layers=1, num_experts=64, num_experts_per_token=4)
    ck = synth_checkpoint(cfg, "cpu", recipe="4.0bpw", seed=0)
    d = write_model_dir(str(tmp_path / "model"), cfg, ck)
    c = json.load(open(os.path.join(d, "config.json")))
    assert c["architectures"] == ["Qwen3MoeForCausalLM"] and c["model_type"] == "qwen3_moe" and c["norm_topk_prob"] is True
    assert (c["num_experts"], c["num_experts_per_tok"], c["moe_intermediate_size"]) == (64, 4, cfg.intermediate_size)
    with safe_open(os.path.join(d, "model.safetensors"), "pt") as f:
        keys = set(f.keys())
    p = "model.layers.0"
    for e in (0, 63):
        for w in ("gate_proj", "up_proj", "down_proj"):
            assert f"{p}.mlp.experts.{e}.{w}.q_weight" in keys
    assert f"{p}.mlp.gate.weight" in keys and f"{p}.self_attn.q_norm.weight" in keys and f"{p}.self_attn.k_norm.weight" in keys
    assert not any("block_sparse_moe" in k for k in keys)


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["exl2_fast", "ctypes"])
def test_unmodified_reference_runs_qwen3_moe_on_the_dropin(tmp_path, route):
    ref = _reference_pkg()
    if ref is None:
        pytest.skip("no copy of the reference's host package on this machine")
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    from exllamav2_amd.synth import synth_checkpoint
    from exllamav2_amd.synth_dir import write_model_dir
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        from run_reference_dropin import QWEN3_MOE_PROMPT
    finally:
        sys.path.pop(0)
    # headnorm_rms=False: the reference's host passes `archparams.headnorm == "rmsnorm"` to make_q_attn (attn.py:303) and its default
    # is "layernorm" (architecture.py:219; only Gemma3 sets "rmsnorm"), so on ITS host a Qwen3-MoE model's q / k head norm removes the
    # mean -- the oracle restates what that host asks the extension for.  The prompt and the three tokens were chosen with the oracle
    # alone: every prompt position has a router gap above 8 (the smallest is 9.0), so do steps 0, 2 and 3 (13.2, 41.8, 13.6; step 1: 5.1)
    cfg = _cfg(vocab_size=320, headnorm_rms=False)
    ck = synth_checkpoint(cfg, "cpu", recipe="4.0bpw", seed=11)
    oracle = Qwen3MoeOracleModel(cfg, ck)
    model_dir = write_model_dir(str(tmp_path / "model"), cfg, ck)
    out = str(tmp_path / "out.npz")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "dropin"), ROOT, ref]), EXL2_DEBUG_ROUTE="1",
               EXL2_DROPIN_FAST="0" if route == "ctypes" else "1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_reference_dropin.py"), model_dir, out, "qwen3_moe"],
                       env=env, capture_output=True, text=True, cwd=str(tmp_path), timeout=900)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "q_moe_mlp route: pairs rows=1 experts=128 jobs=8" in r.stderr, r.stderr[-1500:]
    assert "q_moe_mlp route: pairs rows=3 experts=128 jobs=24" in r.stderr, r.stderr[-1500:]
    got = np.load(out)
    tol = lambda w: 0.03 + np.abs(w) * 2.0 ** -8
    compared = 0
    oracle.reset(1)
    want = oracle.forward(np.array([list(QWEN3_MOE_PROMPT)]))
    # the prompt (the reference's torch loop): every position whose own router decision is clear in the oracle
    for pos in np.nonzero(oracle.router_gap_pos[0] > GAP)[0]:
        g, w = got["prefill"][:, pos, :cfg.vocab_size].astype(np.float64), want[:, pos]
        print(f"prompt position {pos}: worst error / bound = {float((np.abs(g - w) / tol(w)).max()):.3f}")
        assert np.all(np.abs(g - w) <= tol(w)), pos
        compared += 1
    for i, tok in enumerate(got["tokens"]):
        w = oracle.forward(np.array([[int(tok)]]))[:, -1]
        if oracle.router_gap[0] <= GAP:
            continue
        g = got["steps"][:, i, :cfg.vocab_size].astype(np.float64)
        print(f"step {i}: worst error / bound = {float((np.abs(g - w) / tol(w)).max()):.3f}")
        assert np.all(np.abs(g - w) <= tol(w)), i
        compared += 1
    assert compared >= 8, compared                         # (six prompt positions and at least two steps)
    # the three-row call: every row against the oracle
    oracle.reset(3)
    w = oracle.forward(got["batch3_ids"])[:, -1]
    ok = oracle.router_gap > GAP
    g = got["batch3"][:, -1, :cfg.vocab_size].astype(np.float64)
    print(f"three rows: worst error / bound = {(np.abs(g - w) / tol(w)).max(-1)}, clear {ok}")
    assert ok.sum() >= 2, oracle.router_gap
    assert np.all((np.abs(g - w) <= tol(w))[ok])
