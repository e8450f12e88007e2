"""Checker for Gemma-2 / Gemma-3 blocks: an fp32 residual stream with post norms (architecture.py:576, :601, :955-957), GELU, a
sliding window on some layers, score and logit soft caps -- restated in float64 with the reference's rounding points (q_attn.cu:268-279,
:337-339, q_mlp.cu:183, :230, model.py:1043-1044):
  * the pre-norm reads the fp32 stream and leaves fp16 rows (temp_state);
  * every projection output is fp16;
  * the post norm reads the fp16 projection output and is ADDED to the stream in fp32;
  * the final norm leaves fp16 rows, the head fp16 logits, the cap works on those.
Built from oracle.modules (rms_norm's numerics, attention(window_left=, softcap=)) and the reconstructed weights.  TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import numpy as np

from oracle import modules as OM
from oracle.model import OracleModel
from tests.qk_norm_oracle import head_norm

F16, F32, F64 = np.float16, np.float32, np.float64


def rms_norm_any(x, w, eps: float, out_f32: bool = False):
    """oracle.modules.rms_norm for either input format (rms_norm.cu:68-76, :92-99, :118, :137-142): fp16 input is clamped to +-65504, fp32
    input is not; sum of squares in float64, the scale rounded to fp32, (x * w) * r in fp32; fp16 or fp32 out."""
    x = np.asarray(x)
    xf = np.clip(x.astype(F32), -65504.0, 65504.0) if x.dtype == F16 else x.astype(F32)
    ss = (xf.astype(F64) ** 2).sum(axis=-1, keepdims=True)
    rmf = (1.0 / np.sqrt(ss / x.shape[-1] + eps)).astype(F32)
    y = (xf * np.asarray(w, dtype=F16).astype(F32)[None, :]) * rmf
    return y.astype(F32) if out_f32 else y.astype(F16)


def post_norm_add(t16, w, x32, eps: float):
    """x + rmsnorm(t) * w: fp16 in, added to the fp32 stream in fp32 (the add_residual form of rms_norm.cu:137-142)."""
    return (rms_norm_any(np.asarray(t16, dtype=F16), w, eps, out_f32=True) + np.asarray(x32, dtype=F32)).astype(F32)


def gelu_mul(g16, u16):
    """act_mul with GELU (q_mlp_activation.cuh:23-34, :54-112): tanh form in fp32 -> fp16, times up in fp16, clamped."""
    x = np.asarray(g16, dtype=F16).astype(F64)
    a = (0.5 * x * (1.0 + np.tanh(0.797884560803 * (x + 0.044715 * x * x * x)))).astype(F16)
    return np.clip(OM.hmul(a, u16).astype(F32), -65504.0, 65504.0).astype(F16)


def softcap(x, cap: float):
    """cap * tanh(x / cap) in float64 (softcap.cu:8-64); the caller rounds."""
    return cap * np.tanh(np.asarray(x).astype(F64) / cap)


def embed(table16, ids, scale: float):
    """embedding.py:184-187: `.float()`, then one fp32 multiply by the scale as an fp32 number."""
    return np.asarray(table16, dtype=F16)[ids].astype(F32) * F32(scale)


def layer_is_windowed(cfg, idx: int) -> bool:
    """model.py:111-121: only with alternating_swa; pattern > 1: the layers with (idx + 1) % pattern != 0, else the even layers."""
    if not getattr(cfg, "sliding_window", 0) or not getattr(cfg, "alternating_swa", False):
        return False
    pattern = getattr(cfg, "sliding_window_pattern", 1)
    if pattern > 1:
        return (idx + 1) % pattern != 0
    return idx % 2 == 0


class GemmaOracleModel(OracleModel):
    """OracleModel for a config with residual_fp32 and post norms.  The checkpoint holds the norm weights as on disk: the constant bias
    (rmsnorm.py:57-59, headnorm.py:78-79) is added in fp16 here, as at load.  use_window=False drops the sliding window (tests use it to show that the
    window clipped).  FP16 cache, dense MLP."""

    def __init__(self, cfg, ck: dict, use_window: bool = True):
        super().__init__(cfg, ck)
        self.use_window = use_window
        b = float(getattr(cfg, "norm_constant_bias", 0.0))
        if b:
            for k in list(self.w):
                if k.endswith(("layernorm", ".q_norm", ".k_norm")) or k == "model.norm":       # (headnorm.py:78-79: head norms too)
                    self.w[k] = (self.w[k].astype(F16) + F16(b)).astype(F16)
        base_alt = getattr(cfg, "rotary_embedding_base_alt", None)
        self.sin_alt = self.cos_alt = None
        if base_alt:
            self.sin_alt, self.cos_alt = OM.rope_tables(cfg.max_seq_len, cfg.head_dim, base_alt, cfg.rope_style == 2)

    def forward(self, ids: np.ndarray, q4_cache: bool = False) -> np.ndarray:
        """ids int [b, q_len] -> float64 [b, q_len, vocab]: the cap of the fp16 logits when the config caps them, else the unrounded
        logits like OracleModel."""
        assert not q4_cache
        c = self.cfg
        b, s = ids.shape
        past = self.seq_len
        scale = float(c.hidden_size) ** 0.5 if getattr(c, "normalize_embeddings", False) else 1.0
        x = embed(self.w["model.embed_tokens"], ids.reshape(-1), scale).reshape(b * s, c.hidden_size)
        qs = getattr(c, "query_pre_attn_scalar", None)
        sm_scale = float(qs) ** -0.5 if qs else None
        acap = float(getattr(c, "attn_logit_softcapping", 0.0) or 0.0)
        gelu = getattr(c, "mlp_act_func", "silu") == "gelu"
        for i in range(c.num_hidden_layers):
            p = f"model.layers.{i}"
            win = layer_is_windowed(c, i)
            n = rms_norm_any(x, self.w[p + ".input_layernorm"], c.norm_eps)
            q = self.linear(n, p + ".self_attn.q_proj").astype(F16).reshape(b, s, c.num_attention_heads, c.head_dim)
            k = self.linear(n, p + ".self_attn.k_proj").astype(F16).reshape(b, s, c.num_key_value_heads, c.head_dim)
            v = self.linear(n, p + ".self_attn.v_proj").astype(F16).reshape(b, s, c.num_key_value_heads, c.head_dim)
            if getattr(c, "use_qk_norm", False):
                rms = bool(getattr(c, "headnorm_rms", True))
                q = head_norm(q, self.w[p + ".self_attn.q_norm"], None, c.norm_eps, rms)[1]
                k = head_norm(k, self.w[p + ".self_attn.k_norm"], None, c.norm_eps, rms)[1]
            sin, cos = (self.sin_alt, self.cos_alt) if (win and self.sin_alt is not None) else (self.sin, self.cos)
            pos = np.full((b,), past)
            q = OM.rope_(q, sin, cos, pos, c.rope_style == 2)
            k = OM.rope_(k, sin, cos, pos, c.rope_style == 2)
            self.k_cache[i, :, past:past + s] = k
            self.v_cache[i, :, past:past + s] = v
            a = OM.attention(q, self.k_cache[i, :, :past + s], self.v_cache[i, :, :past + s], scale=sm_scale,
                             window_left=c.sliding_window if (win and self.use_window) else -1, softcap=acap)
            a = a.reshape(b * s, c.num_attention_heads * c.head_dim)
            t = self.linear(a, p + ".self_attn.o_proj").astype(F16)
            x = post_norm_add(t, self.w[p + ".post_attention_layernorm"], x, c.norm_eps)
            n = rms_norm_any(x, self.w[p + ".pre_feedforward_layernorm"], c.norm_eps)
            g = self.linear(n, p + ".mlp.gate_proj").astype(F16)
            u = self.linear(n, p + ".mlp.up_proj").astype(F16)
            y = gelu_mul(g, u) if gelu else OM.silu_mul(g, u)
            t = self.linear(y, p + ".mlp.down_proj").astype(F16)
            x = post_norm_add(t, self.w[p + ".post_feedforward_layernorm"], x, c.norm_eps)
        self.seq_len = past + s
        self.router_margin = np.full((b,), np.inf)
        n = rms_norm_any(x, self.w["model.norm"], c.norm_eps)
        logits = self.linear(n, "lm_head")[:, :c.vocab_size]
        fcap = float(getattr(c, "final_logit_softcapping", 0.0) or 0.0)
        if fcap:
            logits = softcap(logits.astype(F16), fcap)
        return logits.reshape(b, s, c.vocab_size)
