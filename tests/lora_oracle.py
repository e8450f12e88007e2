"""Checker for the LoRA adapters: apply_loras_cuda (cuda/lora.cu:5-34) restated in float64, and OracleModel with adapters where the
reference's kernel composition applies them (q_attn.cu:281-283,344; q_mlp.cu:196-197,235).  TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import numpy as np

from oracle import modules as OM
from oracle.model import OracleModel

F16 = np.float16
F64 = np.float64

PROJ_KEYS = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj",
             "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj")


def make_adapter(rng, K: int, N: int, r: int, amp: float = 1.0):
    """(A fp16 [K, r], B fp16 [r, N]) with x A ~ N(0, 1) for x ~ N(0, 1) and the whole term ~ N(0, amp^2)."""
    a = (rng.standard_normal((K, r)) / np.sqrt(K)).astype(F16)
    b = (amp * rng.standard_normal((r, N)) / np.sqrt(r)).astype(F16)
    return a, b


def lora_terms(x, out_in, pairs):
    """-> (want, slack): want = out_in + sum_l t16_l B_l with t16_l = fp16(x A_l), both products in float64; slack = 2^-11 *
    sum_l |t16_l| |B_l|, the one-ulp uncertainty of where the low-rank intermediate rounds."""
    want = np.asarray(out_in, dtype=F16).astype(F64)
    slack = np.zeros_like(want)
    for a, b in pairs:
        t16 = (x.astype(F64) @ a.astype(F64)).astype(F16).astype(F64)
        want = want + t16 @ b.astype(F64)
        slack = slack + np.abs(t16) @ np.abs(b.astype(F64))
    return want, slack * 2.0 ** -11


def lora_add16(x, base16, pairs):
    """the fp16 tensor the reference leaves: base (already fp16) plus the adapters' terms, rounded once"""
    if not pairs:
        return np.asarray(base16, dtype=F16)
    return lora_terms(x, base16, pairs)[0].astype(F16)


class LoraOracleModel(OracleModel):
    """OracleModel ("reference" rounding, dense MLP, FP16 and Q4 cache) with adapters.  An adapter is a dict
    {"model.layers.<i>.<projection>": (A fp16 [K, r], B fp16 [r, N], B pre-scaled)}; `active` lists those of the next forward()."""

    active: list = []

    def _lin16(self, n, key):
        return lora_add16(n, self.linear(n, key).astype(F16), [ad[key] for ad in self.active if key in ad])

    def _res16(self, x, y, key):
        """x + y W rounded to fp16 (the residual add of o_proj / down_proj), then the adapters on top of it"""
        base = (x.astype(F64) + self.linear(y, key)).astype(F16)
        return lora_add16(y, base, [ad[key] for ad in self.active if key in ad])

    def forward(self, ids: np.ndarray, q4_cache: bool = False) -> np.ndarray:
        assert self.rounding == "reference"
        c = self.cfg
        b, s = ids.shape
        past = self.seq_len
        x = self.w["model.embed_tokens"][ids.reshape(-1)].reshape(b * s, c.hidden_size).astype(F16)
        self.router_margin = np.full((b,), np.inf)
        for i in range(c.num_hidden_layers):
            p = f"model.layers.{i}"
            n = OM.rms_norm(x, self.w[p + ".input_layernorm"], c.norm_eps)
            q = self._lin16(n, p + ".self_attn.q_proj").reshape(b, s, c.num_attention_heads, c.head_dim)
            k = self._lin16(n, p + ".self_attn.k_proj").reshape(b, s, c.num_key_value_heads, c.head_dim)
            v = self._lin16(n, p + ".self_attn.v_proj").reshape(b, s, c.num_key_value_heads, c.head_dim)
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
            a = a.reshape(b * s, c.num_attention_heads * c.head_dim)
            x = self._res16(x, a, p + ".self_attn.o_proj")
            n = OM.rms_norm(x, self.w[p + ".post_attention_layernorm"], c.norm_eps)
            y = OM.silu_mul(self._lin16(n, p + ".mlp.gate_proj"), self._lin16(n, p + ".mlp.up_proj"))
            x = self._res16(x, y, p + ".mlp.down_proj")
        self.seq_len = past + s
        n = OM.rms_norm(x, self.w["model.norm"], c.norm_eps)
        return self.linear(n, "lm_head")[:, :c.vocab_size].reshape(b, s, c.vocab_size)
