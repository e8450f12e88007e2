"""ExLlamaV2LayerNorm (reference layernorm.py:11-125)."""
from __future__ import annotations

import torch

from .ext import none_tensor


class ExLlamaV2LayerNorm:
    def __init__(self, ext, key: str, weight: torch.Tensor, bias: torch.Tensor | None, eps: float):
        self.ext = ext
        self.key = key
        self.weight = weight
        self.bias = bias
        self.variance_epsilon = eps

    def forward(self, hidden_states: torch.Tensor) -> torch.Tensor:
        """layernorm.py:99-125 -> ext_c.layer_norm"""
        out = torch.empty_like(hidden_states)
        d = hidden_states.shape[-1]
        self.ext.layer_norm(hidden_states.view(-1, d), self.weight, none_tensor if self.bias is None else self.bias,
                            out.view(-1, d), self.variance_epsilon)
        return out
