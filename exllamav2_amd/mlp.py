"""ExLlamaV2MLP (reference mlp.py:150-223 load/make_q_mlp, :318-361 forward)."""
from __future__ import annotations

import torch

from .ext import none_tensor
from .linear import ExLlamaV2Linear


class ExLlamaV2MLP:
    def __init__(self, model, key: str, layer_idx: int):
        cfg = model.config
        self.model, self.ext, self.key, self.layer_idx = model, model.ext, key, layer_idx
        gated = bool(getattr(cfg, "mlp_gate", True))                                # False: act(up) -> down (StarCoder2)
        self.gate_proj = ExLlamaV2Linear(self.ext, key + ".mlp.gate_proj", cfg.hidden_size, cfg.intermediate_size, model) if gated else None
        self.up_proj = ExLlamaV2Linear(self.ext, key + ".mlp.up_proj", cfg.hidden_size, cfg.intermediate_size, model)
        self.down_proj = ExLlamaV2Linear(self.ext, key + ".mlp.down_proj", cfg.intermediate_size, cfg.hidden_size, model)
        self.q_handle = None

    def load(self, ck: dict):
        cfg, m = self.model.config, self.model
        for lin in self.linears():
            lin.load(ck[lin.key])
        post = getattr(cfg, "post_norms", False)
        parallel = bool(getattr(cfg, "parallel_decoder_blocks", False))            # no norm, no residual: as the attention module
        ln = getattr(cfg, "norm", "rmsnorm") == "layernorm"
        # with post norms the MLP's pre-norm is `.pre_feedforward_layernorm` and `.post_feedforward_layernorm` follows down_proj
        # (architecture.py:566-569); `.post_attention_layernorm` then belongs to the attention module
        nk = self.key + (".pre_feedforward_layernorm" if post else ".post_attention_layernorm")
        self.post_attention_layernorm = None if parallel else m.norm_weight(ck[nk])
        self.post_attention_layernorm_bias = None if parallel else ck.get(nk + ".bias")
        self.post_layernorm = m.norm_weight(ck[self.key + ".post_feedforward_layernorm"]) if post else None
        self.q_handle = self.ext.make_q_mlp(                                     # mlp.py:204-223
            none_tensor if self.post_attention_layernorm is None else self.post_attention_layernorm,
            none_tensor if self.post_attention_layernorm_bias is None else self.post_attention_layernorm_bias, not ln, cfg.norm_eps,
            None if self.gate_proj is None else self.gate_proj.q_handle, self.up_proj.q_handle, self.down_proj.q_handle,
            m.temp_state, m.temp_a, m.temp_b, none_tensor, m.max_rows, getattr(cfg, "mlp_act_func", "silu") == "gelu", not parallel,
            none_tensor if self.post_layernorm is None else self.post_layernorm, none_tensor, bool(getattr(cfg, "residual_fp32", False)), False)
        return self

    def linears(self):
        return [lin for lin in (self.gate_proj, self.up_proj, self.down_proj) if lin is not None]

    def unload(self):
        if self.q_handle is not None:
            self.ext.free_q_mlp(self.q_handle)
            self.q_handle = None
        for lin in self.linears():
            lin.unload()

    def update_loras(self) -> int:
        """mlp.py:525-544: hands the adapters attached to the three linears to the handle; returns the largest rank"""
        return self.ext.q_mlp_set_loras(self.q_handle, self.gate_proj.lora_table(), self.up_proj.lora_table(), self.down_proj.lora_table())

    def forward(self, hidden_states: torch.Tensor, loras=None):
        """mlp.py:353: ext_c.q_mlp_forward_ in place, for every row count (<= 16 rows: the fused decode launches; above:
        row pre-pass + dequantize-into-MFMA GEMMs, csrc/modules.hip:exl2_q_mlp_forward).  loras: the ExLlamaV2Lora adapters to apply."""
        self.ext.q_mlp_forward_(self.q_handle, hidden_states, loras=[id(l) for l in loras] if loras else None)
        return hidden_states

    def forward_normed(self, xn: torch.Tensor):
        """The MLP for a caller that owns the norms (a post-norm block): xn fp16 [rows, hidden], already normed; down_proj's output is
        left in the model's temp_state, the post norm is the caller's (ext.norm_bridge)."""
        self.ext.q_mlp_forward_normed(self.q_handle, xn)
