"""Checker for LayerNorm models (StarCoder2: architecture.py:656-676; Cohere: :704-721): layer_norm.cu restated in float64 with its
rounding points, and the two block forms built from it and oracle.modules.  TEST INFRASTRUCTURE ONLY.

layer_norm (layer_norm.cu:31-159):
  * fp16 inputs widened to fp32 and clamped to +-65504;
  * mean = (sum) * (1 / dim) -- the sum is taken in float64 here, the mean rounded to fp32;
  * d = x - mean in fp32; the variance is the sum of d * d (float64 here), never E[x^2] - mean^2;
  * rsvar = rsqrt(sum * (1 / dim) + eps) rounded to fp32;
  * n = fp16_rn((d * w) * rsvar), the two products rounded to fp32 in that order;
  * + bias as an fp16 add, then + residual as an fp16 add.
Blocks:
  * sequential (StarCoder2): LN(+bias) -> biased q/k/v -> NeoX RoPE -> attention -> biased o_proj + residual; LN(+bias) -> c_fc + bias
    -> GELU (tanh form, fp32 -> fp16) -> c_proj + bias + residual;
  * parallel (Cohere, parallel_decoder.py:137-143): n = LN(x); a = attention(n) and m = mlp(n) WITHOUT residual, fp16; x += a; x += m
    as two fp16 adds in that order; GPT-J RoPE; optional LayerNorm over the heads (use_qk_norm, headnorm_rms=False); logit_scale folded
    into the head at load (ext.py:336: q_scale_max *= scale / 256 in fp16; :363 for GPTQ), i.e. the head reconstructed from those scales."""
from __future__ import annotations

import numpy as np

from oracle import exl2 as OX
from oracle import modules as OM
from oracle.model import OracleModel, _lin_tensors, _np
from tests.qk_norm_oracle import head_norm

F16, F32, F64 = np.float16, np.float32, np.float64


def hadd(a, b):
    """one fp16 add, round to nearest even (exact sum in float64)"""
    with np.errstate(over="ignore"):                                 # (a sum beyond 65504 is inf, as in the kernels)
        return (np.asarray(a, dtype=F16).astype(F64) + np.asarray(b, dtype=F16).astype(F64)).astype(F16)


def layer_norm(x, w, b, eps: float, residual=None, parts: bool = False):
    """x fp16 [rows, dim], w fp16 [dim], b fp16 [dim] or None, residual fp16 [rows, dim] or None -> fp16 [rows, dim].
    parts=True: (result, pre) with pre the fp32 value in front of the fp16 rounding."""
    x = np.asarray(x, dtype=F16)
    dim = x.shape[-1]
    r_dim = F64(F32(1.0) / F32(dim))
    xf = np.clip(x.astype(F32), -65504.0, 65504.0)
    mean = (xf.astype(F64).sum(axis=-1, keepdims=True) * r_dim).astype(F32)
    d = (xf - mean).astype(F32)
    var = (d.astype(F64) ** 2).sum(axis=-1, keepdims=True) * r_dim
    rsvar = (1.0 / np.sqrt(var + F64(F32(eps)))).astype(F32)
    pre = ((d * np.asarray(w, dtype=F16).astype(F32)[None, :]).astype(F32) * rsvar).astype(F32)
    y = pre.astype(F16)
    if b is not None:
        y = hadd(y, np.broadcast_to(np.asarray(b, dtype=F16)[None, :], y.shape))
    if residual is not None:
        y = hadd(y, residual)
    return (y, pre) if parts else y


def ulp16(v):
    """spacing of fp16 at magnitude |v| (normal range; subnormals: 2^-24)"""
    a = np.maximum(np.abs(np.asarray(v, dtype=F64)), 2.0 ** -14)
    return 2.0 ** (np.floor(np.log2(a)) - 10)


def layer_norm_tol(x, w, b, eps, residual=None):
    """(want, tol): one fp16 ulp of the largest magnitude among the pre-bias value, the bias, the residual and the result -- the fp16
    adds behind the rounding point can cancel, so a 1-ulp flip of the normed value is the only admissible difference."""
    want, pre = layer_norm(x, w, b, eps, residual, parts=True)
    mag = np.maximum(np.abs(pre.astype(F64)), np.abs(want.astype(F64)))
    if b is not None:
        mag = np.maximum(mag, np.abs(np.asarray(b, dtype=F64))[None, :])
    if residual is not None:
        mag = np.maximum(mag, np.abs(np.asarray(residual, dtype=F64)))
    return want, ulp16(mag)


def gelu(x16):
    """q_mlp_activation.cuh:23-34 without a gate: tanh form in fp32 -> fp16"""
    x = np.asarray(x16, dtype=F16).astype(F64)
    return (0.5 * x * (1.0 + np.tanh(0.797884560803 * (x + 0.044715 * x * x * x)))).astype(F16)


def silu(x16):
    x = np.asarray(x16, dtype=F16).astype(F64)
    return (x / (1.0 + np.exp(-x))).astype(F16)


class LayerNormOracleModel(OracleModel):
    """OracleModel for a config with norm == "layernorm": sequential blocks, or parallel ones with parallel_decoder_blocks.  The
    checkpoint holds `<norm>.bias` next to a norm's weight when norm_bias is set.  FP16 cache, dense MLP."""

    def __init__(self, cfg, ck: dict):
        super().__init__(cfg, ck)
        assert not getattr(cfg, "alternating_swa", False), "no layer of these architectures is windowed (model.py:111-121)"
        s = float(getattr(cfg, "logit_scale", 1.0))
        if s != 1.0:
            head = ck["lm_head"]
            if "qweight" in head:                                        # ext.py:363: scales *= prescale, in fp16
                t = {k: _np(v).copy() for k, v in head.items() if k in ("qweight", "qzeros", "scales", "g_idx")}
                t["scales"] = (t["scales"].astype(F16).astype(F32) * F32(s)).astype(F16)
                self.w["lm_head"] = OX.gptq_reconstruct(t).astype(F32)
            else:                                                        # ext.py:336: q_scale_max *= prescale / 256, in fp16
                self.w["lm_head"] = OX.exl2_reconstruct(_lin_tensors(head), prescale=s).astype(F32)

    def _ln(self, x, key):
        return layer_norm(x, self.w[key], self.w.get(key + ".bias"), self.cfg.norm_eps)

    def attn(self, n, p, b, s, past, i):
        c = self.cfg
        q = self.linear(n, p + ".self_attn.q_proj").astype(F16).reshape(b, s, c.num_attention_heads, c.head_dim)
        k = self.linear(n, p + ".self_attn.k_proj").astype(F16).reshape(b, s, c.num_key_value_heads, c.head_dim)
        v = self.linear(n, p + ".self_attn.v_proj").astype(F16).reshape(b, s, c.num_key_value_heads, c.head_dim)
        if getattr(c, "use_qk_norm", False):
            rms = bool(getattr(c, "headnorm_rms", True))
            q = head_norm(q, self.w[p + ".self_attn.q_norm"], None, c.norm_eps, rms)[1]
            k = head_norm(k, self.w[p + ".self_attn.k_norm"], None, c.norm_eps, rms)[1]
        pos = np.full((b,), past)
        q = OM.rope_(q, self.sin, self.cos, pos, c.rope_style == 2)
        k = OM.rope_(k, self.sin, self.cos, pos, c.rope_style == 2)
        self.k_cache[i, :, past:past + s] = k
        self.v_cache[i, :, past:past + s] = v
        a = OM.attention(q, self.k_cache[i, :, :past + s], self.v_cache[i, :, :past + s])
        return self.linear(a.reshape(b * s, c.num_attention_heads * c.head_dim), p + ".self_attn.o_proj")

    def mlp(self, n, p):
        c = self.cfg
        is_gelu = getattr(c, "mlp_act_func", "silu") == "gelu"
        u = self.linear(n, p + ".mlp.up_proj").astype(F16)
        if getattr(c, "mlp_gate", True):
            g = self.linear(n, p + ".mlp.gate_proj").astype(F16)
            if is_gelu:
                y = np.clip(OM.hmul(gelu(g), u).astype(F32), -65504.0, 65504.0).astype(F16)
            else:
                y = OM.silu_mul(g, u)
        else:
            y = gelu(u) if is_gelu else silu(u)
        return self.linear(y, p + ".mlp.down_proj")

    def forward(self, ids: np.ndarray, q4_cache: bool = False) -> np.ndarray:
        assert not q4_cache
        c = self.cfg
        b, s = ids.shape
        past = self.seq_len
        x = self.w["model.embed_tokens"][ids.reshape(-1)].reshape(b * s, c.hidden_size).astype(F16)
        for i in range(c.num_hidden_layers):
            p = f"model.layers.{i}"
            if getattr(c, "parallel_decoder_blocks", False):
                n = self._ln(x, p + ".input_layernorm")
                a = self.attn(n, p, b, s, past, i).astype(F16)
                m = self.mlp(n, p).astype(F16)
                x = hadd(hadd(x, a), m)
            else:
                n = self._ln(x, p + ".input_layernorm")
                x = (x.astype(F64) + self.attn(n, p, b, s, past, i)).astype(F16)
                n = self._ln(x, p + ".post_attention_layernorm")
                x = (x.astype(F64) + self.mlp(n, p)).astype(F16)
        self.seq_len = past + s
        self.router_margin = np.full((b,), np.inf)
        n = self._ln(x, "model.norm")
        return self.linear(n, "lm_head")[:, :c.vocab_size].reshape(b, s, c.vocab_size)
