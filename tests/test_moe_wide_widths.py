"""One sparse-MoE block at Qwen3-30B-A3B's widths (hidden 2048, 128 experts of width 768, top 8; 4.0 bpw) on the MI355X: the shapes the
lean decode kernel may decline (N = 768, K = 768) must stay on the pair-job route -- the idea of
tests/test_chain.py::test_llama2_70b_widths_stay_on_the_lean_kernel.  Rows 1 and 4 against OracleModel.moe_mlp (moe_mlp.py:255-323
semantics); only the experts the ORACLE's router selects are reconstructed on the host (that is the test's time, ~10 s)."""
import dataclasses

import numpy as np
import pytest
import torch

from oracle import modules as OMod
from tests.qwen3_moe_oracle import router_gap

F16 = np.float16


@pytest.mark.gpu
def test_qwen3_30b_a3b_widths_stay_on_the_pair_jobs(capfd, monkeypatch):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from exllamav2_amd.config import ExLlamaV2Config
    from exllamav2_amd.synth import synth_checkpoint
    from exllamav2_amd.model import ExLlamaV2
    from oracle.model import OracleModel
    cfg = dataclasses.replace(ExLlamaV2Config.qwen3_30b_a3b(max_seq_len=256, max_input_len=16, max_batch_size=16), num_hidden_layers=1, vocab_size=512)
    ck = synth_checkpoint(cfg, "cuda:0", recipe="4.0bpw", seed=3)
    pfx = "model.layers.0"
    rng = np.random.default_rng(5)
    xs = {rows: rng.standard_normal((rows, cfg.hidden_size)).astype(F16) for rows in (1, 4)}
    # the oracle's own routing says which experts it needs (before load(): it re-lays the tensors out in place)
    norm_w, gate = ck[pfx + ".post_attention_layernorm"].cpu().numpy(), ck[pfx + ".block_sparse_moe.gate"].cpu().numpy()
    need = set()
    for x in xs.values():
        raw = (OMod.rms_norm(x, norm_w, cfg.norm_eps).astype(np.float32) @ gate.astype(np.float32).T).astype(F16)
        need |= set(np.nonzero(OMod.moe_route(raw, cfg.num_experts_per_token)[1].any(0))[0].tolist())
    sub = {k: v for k, v in ck.items() if not isinstance(v, dict) and k.startswith(pfx)}
    sub.update({f"{pfx}.block_sparse_moe.experts.{e}.{w}": ck[f"{pfx}.block_sparse_moe.experts.{e}.{w}"] for e in need for w in ("w1", "w2", "w3")})
    oracle = OracleModel(cfg, sub)
    model = ExLlamaV2(cfg, device="cuda:0").load(ck)
    moe = model.layers[0][1]
    worst = 0.0
    for rows, x in xs.items():
        n = OMod.rms_norm(x, oracle.w[pfx + ".post_attention_layernorm"], cfg.norm_eps)
        raw = (n.astype(np.float32) @ gate.astype(np.float32).T).astype(F16)
        ok = router_gap(raw, cfg.num_experts_per_token) > 4                       # (tests/test_moe.py::_moe_case's 4-ulp rule)
        oracle.router_margin = np.full((rows,), np.inf)
        want = oracle.moe_mlp(x, n, pfx).astype(np.float64)
        xt = torch.from_numpy(x).to("cuda:0").view(rows, 1, -1).contiguous()
        monkeypatch.setenv("EXL2_DEBUG_ROUTE", "1")
        capfd.readouterr()
        moe.forward(xt)
        torch.cuda.synchronize()
        err_out = capfd.readouterr().err
        monkeypatch.delenv("EXL2_DEBUG_ROUTE")
        assert f"q_moe_mlp route: pairs rows={rows} experts=128 jobs={rows * 8}" in err_out, err_out      # not the per-expert loop
        got = xt.view(rows, -1).float().cpu().numpy().astype(np.float64)
        assert np.all(np.isfinite(got))
        w = moe.temp_logits[:rows].cpu().numpy()
        assert np.all((w != 0).sum(-1) == 8)
        assert np.array_equal((w != 0)[ok], OMod.moe_route(raw, 8)[1][ok])
        # the bar of tests/test_moe.py::test_moe_layer_mixtral_widths (one fp16 rounding per expert contribution in the oracle, none here)
        err, tol = np.abs(got - want)[ok], (np.abs(want) * 2.0 ** -8 + 8e-3)[ok]
        assert ok.sum() >= max(1, rows - 1), "too many router near-ties"
        assert np.all(err <= tol), (rows, float(err.max()), float((err / tol).max()))
        assert np.abs(want - x.astype(np.float64)).mean() > 0.05                   # a visible update (0.23 with a CPU-drawn checkpoint of these widths)
        worst = max(worst, float((err / tol).max()))
    print(f"qwen3-30b-a3b-width MoE block: worst error / tolerance = {worst:.3f}")
    model.unload()
