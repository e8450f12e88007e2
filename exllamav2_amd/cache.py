"""KV caches (reference cache.py): FP16 and Q4 / Q6 / Q8, contiguous [batch, max_seq_len, kv_heads, head_dim] per layer, or paged
views [pages, 256, kv_heads, head_dim] of the same storage (attn.py:504-505)."""
from __future__ import annotations

import torch

from .ext import none_tensor

PAGE_SIZE = 256                                           # generator/dynamic.py:33


class ExLlamaV2Cache:
    """FP16 cache (cache.py:230-300)."""

    def __init__(self, model, batch_size: int = 1, max_seq_len: int | None = None):
        cfg = model.config
        self.model = model
        self.batch_size = batch_size
        self.max_seq_len = max_seq_len or cfg.max_seq_len
        self.current_seq_len = 0
        shape = (batch_size, self.max_seq_len, cfg.num_key_value_heads, cfg.head_dim)
        n_layers = len(model.layers) if model.layers else cfg.num_hidden_layers          # layers held by this device
        self.key_states = [torch.zeros(shape, dtype=torch.float16, device=model.device) for _ in range(n_layers)]
        self.value_states = [torch.zeros(shape, dtype=torch.float16, device=model.device) for _ in range(n_layers)]

    def get_kv_state(self, layer_idx: int, batch_size: int, offset: int, width: int, page_size: int = 0,
                     cache_seqlens=None, block_table=None):
        return self.key_states[layer_idx], self.value_states[layer_idx]

    def store_kv_state(self, layer_idx: int, batch_size: int, offset: int, width: int, page_size: int = 0,
                       cache_seqlens=None, block_table=None):
        pass

    def paged_view(self, layer_idx: int):
        cfg = self.model.config
        k = self.key_states[layer_idx].view(-1, PAGE_SIZE, cfg.num_key_value_heads, cfg.head_dim)
        v = self.value_states[layer_idx].view(-1, PAGE_SIZE, cfg.num_key_value_heads, cfg.head_dim)
        return k, v

    def footprint(self) -> int:
        return sum(t.numel() * t.element_size() for t in self.key_states + self.value_states)


class ExLlamaV2Cache_Q4(ExLlamaV2Cache):
    """Q4 cache (cache.py:409-606): uint8 codes + fp16 scales per 32 elements; one shared fp16 temp pair per device.
    get_kv_state dequantizes the live range into the temp, store_kv_state re-quantizes the touched blocks."""

    wbits = 4
    k_bits, v_bits = 4, 4                                 # code width of each side (cache.cu:259-276)

    def __init__(self, model, batch_size: int = 1, max_seq_len: int | None = None):
        cfg = model.config
        self.model = model
        self.ext = model.ext
        self.batch_size = batch_size
        self.max_seq_len = max_seq_len or cfg.max_seq_len
        self.current_seq_len = 0
        kvh, hd, dev = cfg.num_key_value_heads, cfg.head_dim, model.device
        kshape = (batch_size, self.max_seq_len, kvh, hd * self.k_bits // 8)
        vshape = (batch_size, self.max_seq_len, kvh, hd * self.v_bits // 8)
        sshape = (batch_size, self.max_seq_len, kvh, hd // 32)
        L = len(model.layers) if model.layers else cfg.num_hidden_layers
        self.key_states = [torch.zeros(kshape, dtype=torch.uint8, device=dev) for _ in range(L)]
        self.value_states = [torch.zeros(vshape, dtype=torch.uint8, device=dev) for _ in range(L)]
        self.key_scales = [torch.zeros(sshape, dtype=torch.float16, device=dev) for _ in range(L)]
        self.value_scales = [torch.zeros(sshape, dtype=torch.float16, device=dev) for _ in range(L)]
        tshape = (batch_size, self.max_seq_len, kvh, hd)
        self.temp_k = torch.zeros(tshape, dtype=torch.float16, device=dev)       # cache.py:464-469
        self.temp_v = torch.zeros(tshape, dtype=torch.float16, device=dev)

    def get_kv_state(self, layer_idx, batch_size, offset, width, page_size=0, cache_seqlens=None, block_table=None):
        """cache.py:472-514"""
        if width > 0 or page_size:
            self.ext.q_to_fp16_kv(self.key_states[layer_idx], self.temp_k, self.key_scales[layer_idx],
                                  self.value_states[layer_idx], self.temp_v, self.value_scales[layer_idx],
                                  batch_size, offset, width, page_size,
                                  cache_seqlens if cache_seqlens is not None else none_tensor,
                                  block_table if block_table is not None else none_tensor, self.wbits)
        return self.temp_k, self.temp_v

    def store_kv_state(self, layer_idx, batch_size, offset, width, page_size=0, cache_seqlens=None, block_table=None):
        """cache.py:517-556"""
        if width > 0:
            self.ext.fp16_to_q_kv(self.temp_k, self.key_states[layer_idx], self.key_scales[layer_idx],
                                  self.temp_v, self.value_states[layer_idx], self.value_scales[layer_idx],
                                  batch_size, offset, width, page_size,
                                  cache_seqlens if cache_seqlens is not None else none_tensor,
                                  block_table if block_table is not None else none_tensor, self.wbits)

    def paged_view(self, layer_idx):
        cfg = self.model.config
        return (self.temp_k.view(-1, PAGE_SIZE, cfg.num_key_value_heads, cfg.head_dim),
                self.temp_v.view(-1, PAGE_SIZE, cfg.num_key_value_heads, cfg.head_dim))

    def q_views(self, layer_idx, paged: bool):
        """(k_codes, k_scales, v_codes, v_scales) of a layer for attention straight from the codes (attn_q4.hip): contiguous
        [b, T, KVH, .] or, paged, [pages, 256, KVH, .]; the last dimension of a code tensor follows its side's width."""
        ts = (self.key_states[layer_idx], self.key_scales[layer_idx], self.value_states[layer_idx], self.value_scales[layer_idx])
        if not paged:
            return ts
        kvh = self.model.config.num_key_value_heads
        return tuple(t.view(-1, PAGE_SIZE, kvh, t.shape[-1]) for t in ts)

    def q4_views(self, layer_idx, paged: bool):
        """q_views under its first name (the Q4 cache came first)"""
        return self.q_views(layer_idx, paged)

    def footprint(self) -> int:
        ts = self.key_states + self.value_states + self.key_scales + self.value_scales
        return sum(t.numel() * t.element_size() for t in ts)


class ExLlamaV2Cache_Q6(ExLlamaV2Cache_Q4):
    """Q6 cache (cache.py:609-632): 8-bit keys (one byte per element), 4-bit values."""

    wbits = 6
    k_bits, v_bits = 8, 4


class ExLlamaV2Cache_Q8(ExLlamaV2Cache_Q4):
    """Q8 cache (cache.py:633-656): 8-bit keys and values."""

    wbits = 8
    k_bits, v_bits = 8, 8


CACHE_TYPES = {"fp16": ExLlamaV2Cache, "q4": ExLlamaV2Cache_Q4, "q6": ExLlamaV2Cache_Q6, "q8": ExLlamaV2Cache_Q8}


def cache_class(cache_type: str):
    """the cache class of a `--cache` name; unknown names are an error, not FP16"""
    try:
        return CACHE_TYPES[cache_type]
    except KeyError:
        raise ValueError(f"cache type {cache_type!r}: expected one of {sorted(CACHE_TYPES)}") from None
