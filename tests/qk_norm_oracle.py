"""Checker for the q / k head norm (Qwen3-style attention): the reference's head_norm_kernel (head_norm.cu:9-141) restated in
float64, and OracleModel with that norm between the projections and RoPE (q_attn.cu:285-289).  TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import numpy as np

from oracle import modules as OM
from oracle.model import OracleModel

F16 = np.float16


def head_norm(x, w, b, eps: float, rms: bool):
    """x fp16 [..., heads, hd], w (b or None) fp16 [heads, hd] -> (float64 value before any rounding of the result, fp16 result).

    Roundings as in the kernel: every element widened and clamped to +-65504; y = fp16_rn(x * w * rsqrt(mean(x^2) + eps)) (RMS) or the
    same with d = x - mean(x) (LayerNorm over the head); with a bias a SECOND fp16 operation, y = fp16(y + b).  The float64 value
    returned for a biased call is (unrounded norm) + b."""
    xf = np.clip(np.asarray(x, dtype=F16).astype(np.float64), -65504.0, 65504.0)
    wf = np.asarray(w, dtype=F16).astype(np.float64)
    hd = xf.shape[-1]
    if not rms:
        xf = xf - xf.sum(-1, keepdims=True) / hd
    r = 1.0 / np.sqrt((xf ** 2).sum(-1, keepdims=True) / hd + eps)
    y64 = xf * wf * r
    with np.errstate(over="ignore"):
        y16 = y64.astype(F16)
    if b is None:
        return y64, y16
    bf = np.asarray(b, dtype=F16)
    return y64 + bf.astype(np.float64), OM.hadd(y16, np.broadcast_to(bf, y16.shape))


class QKNormOracleModel(OracleModel):
    """OracleModel whose attention normalises q over num_heads and k over num_kv_heads -- after their fp16 rounding, before RoPE;
    v untouched -- with `{layer}.self_attn.q_norm / k_norm`, eps = cfg.norm_eps, form = cfg.headnorm_rms.  Both roundings
    ("reference", "chain"), FP16 and Q4 cache; dense MLP."""

    def _qk(self, q, k, p: str):
        c = self.cfg
        rms = bool(getattr(c, "headnorm_rms", True))
        q = head_norm(q, self.w[p + ".self_attn.q_norm"], None, c.norm_eps, rms)[1]
        k = head_norm(k, self.w[p + ".self_attn.k_norm"], None, c.norm_eps, rms)[1]
        return q, k

    def _attend(self, i: int, q, k, v, past: int, q4_cache: bool):
        c = self.cfg
        b, s = q.shape[0], q.shape[1]
        pos = np.full((b,), past)
        q = OM.rope_(q, self.sin, self.cos, pos, c.rope_style == 2)
        k = OM.rope_(k, self.sin, self.cos, pos, c.rope_style == 2)
        if q4_cache:
            st = self._q4_state(b)
            d = st["kv_dim"]
            self._q4_get(i, past)
            st["temp_k"][:, past * d:(past + s) * d] = k.reshape(b, s * d)
            st["temp_v"][:, past * d:(past + s) * d] = v.reshape(b, s * d)
            kk = st["temp_k"][:, :(past + s) * d].reshape(b, past + s, c.num_key_value_heads, c.head_dim)
            vv = st["temp_v"][:, :(past + s) * d].reshape(b, past + s, c.num_key_value_heads, c.head_dim)
            a = OM.attention(q, kk, vv)
            self._q4_store(i, past, s)
        else:
            self.k_cache[i, :, past:past + s] = k
            self.v_cache[i, :, past:past + s] = v
            a = OM.attention(q, self.k_cache[i, :, :past + s], self.v_cache[i, :, :past + s])
        return a.reshape(b * s, c.num_attention_heads * c.head_dim)

    def forward(self, ids: np.ndarray, q4_cache: bool = False) -> np.ndarray:
        c = self.cfg
        chain = self.rounding == "chain"
        if chain and q4_cache:
            raise NotImplementedError("QKNormOracleModel(rounding='chain'): FP16 cache only")
        b, s = ids.shape
        past = self.seq_len
        x = self.w["model.embed_tokens"][ids.reshape(-1)].reshape(b * s, c.hidden_size).astype(F16)
        self.router_margin = np.full((b,), np.inf)

        def proj(x, n, norm_key, key):
            return self._norm_linear(x, norm_key, key) if chain else self.linear(n, key)

        for i in range(c.num_hidden_layers):
            p = f"model.layers.{i}"
            if (p + ".block_sparse_moe.gate") in self.w:
                raise NotImplementedError("QKNormOracleModel: dense MLP only")
            nk = p + ".input_layernorm"
            n = None if chain else OM.rms_norm(x, self.w[nk], c.norm_eps)
            q = proj(x, n, nk, p + ".self_attn.q_proj").astype(F16).reshape(b, s, c.num_attention_heads, c.head_dim)
            k = proj(x, n, nk, p + ".self_attn.k_proj").astype(F16).reshape(b, s, c.num_key_value_heads, c.head_dim)
            v = proj(x, n, nk, p + ".self_attn.v_proj").astype(F16).reshape(b, s, c.num_key_value_heads, c.head_dim)
            q, k = self._qk(q, k, p)
            a = self._attend(i, q, k, v, past, q4_cache)
            x = (x.astype(np.float64) + self.linear(a, p + ".self_attn.o_proj")).astype(F16)
            nk = p + ".post_attention_layernorm"
            if chain:
                g = self._norm_linear(x, nk, p + ".mlp.gate_proj")
                u = self._norm_linear(x, nk, p + ".mlp.up_proj")
                y = np.clip((g / (1.0 + np.exp(-g))) * u, -65504.0, 65504.0).astype(F16)
            else:
                n = OM.rms_norm(x, self.w[nk], c.norm_eps)
                y = OM.silu_mul(self.linear(n, p + ".mlp.gate_proj").astype(F16), self.linear(n, p + ".mlp.up_proj").astype(F16))
            x = (x.astype(np.float64) + self.linear(y, p + ".mlp.down_proj")).astype(F16)
        self.seq_len = past + s
        if chain:
            logits = self._norm_linear(x, "model.norm", "lm_head")
        else:
            logits = self.linear(OM.rms_norm(x, self.w["model.norm"], c.norm_eps), "lm_head")
        return logits[:, :c.vocab_size].reshape(b, s, c.vocab_size)
