"""Checker for Qwen3-MoE blocks (Qwen3MoeForCausalLM: q / k head norm attention + a sparse-MoE MLP with 128 experts, top 8): the attention
of tests/qk_norm_oracle.py with OracleModel.moe_mlp (ExLlamaV2MoEMLP.forward_torch, moe_mlp.py:255-323) as the block.  "reference"
rounding, FP16 cache.  TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import numpy as np

from oracle import modules as OM
from tests.qk_norm_oracle import QKNormOracleModel

F16 = np.float16


def router_gap(raw, k: int):
    """raw fp16 router logits [rows, E] -> per row (l_k - l_{k+1}) / (max(|l_k|, 1) 2^-10), l_k / l_{k+1} the k-th / (k + 1)-th largest:
    the gap in fp16 steps of the logit, tests/test_moe.py::_moe_case's relative rule (it compares rows with a gap > 4).
    OracleModel.router_margin is a PROBABILITY gap (> 2e-3): with 128 experts a selected probability is ~0.03 and the gaps ~0.003 --
    it would leave almost every row out."""
    srt = np.sort(np.asarray(raw).astype(np.float32), axis=-1)[:, ::-1]
    if k >= srt.shape[1]:
        return np.full((srt.shape[0],), np.inf)
    return (srt[:, k - 1] - srt[:, k]) / (np.maximum(np.abs(srt[:, k - 1]), 1.0) * 2.0 ** -10)


class Qwen3MoeOracleModel(QKNormOracleModel):
    """forward() records router_gap[row of the batch]: the minimum over the layers of router_gap() at the call's LAST position, the one
    whose logits the tests compare"""

    def forward(self, ids: np.ndarray, q4_cache: bool = False) -> np.ndarray:
        if self.rounding != "reference" or q4_cache:
            raise NotImplementedError("Qwen3MoeOracleModel: reference rounding, FP16 cache")
        c = self.cfg
        b, s = ids.shape
        past = self.seq_len
        x = self.w["model.embed_tokens"][ids.reshape(-1)].reshape(b * s, c.hidden_size).astype(F16)
        self.router_margin = np.full((b * s,), np.inf)
        gap = np.full((b * s,), np.inf)
        for i in range(c.num_hidden_layers):
            p = f"model.layers.{i}"
            n = OM.rms_norm(x, self.w[p + ".input_layernorm"], c.norm_eps)
            q = self.linear(n, p + ".self_attn.q_proj").astype(F16).reshape(b, s, c.num_attention_heads, c.head_dim)
            k = self.linear(n, p + ".self_attn.k_proj").astype(F16).reshape(b, s, c.num_key_value_heads, c.head_dim)
            v = self.linear(n, p + ".self_attn.v_proj").astype(F16).reshape(b, s, c.num_key_value_heads, c.head_dim)
            q, k = self._qk(q, k, p)
            a = self._attend(i, q, k, v, past, False)
            x = (x.astype(np.float64) + self.linear(a, p + ".self_attn.o_proj")).astype(F16)
            n = OM.rms_norm(x, self.w[p + ".post_attention_layernorm"], c.norm_eps)
            raw = (n.astype(np.float32) @ self.w[p + ".block_sparse_moe.gate"].astype(np.float32).T).astype(F16)   # (moe_mlp's own first line)
            gap = np.minimum(gap, router_gap(raw, c.num_experts_per_token))
            x = self.moe_mlp(x, n, p)
        self.seq_len = past + s
        self.router_margin = self.router_margin.reshape(b, s).min(axis=1)
        self.router_gap = gap.reshape(b, s)[:, -1]
        self.router_gap_pos = gap.reshape(b, s)                            # (every position of the call)
        logits = self.linear(OM.rms_norm(x, self.w["model.norm"], c.norm_eps), "lm_head")
        return logits[:, :c.vocab_size].reshape(b, s, c.vocab_size)
