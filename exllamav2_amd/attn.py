"""ExLlamaV2Attention (reference attn.py:241-330 load/make_q_attn, :1017-1196 forward, :466-638 forward_paged)."""
from __future__ import annotations

import functools
import os

import torch

from .ext import none_tensor
from .linear import ExLlamaV2Linear


class ExLlamaV2Attention:
    def __init__(self, model, key: str, layer_idx: int):
        cfg = model.config
        self.model, self.ext, self.key, self.layer_idx = model, model.ext, key, layer_idx
        h = cfg.hidden_size
        self.q_proj = ExLlamaV2Linear(self.ext, key + ".self_attn.q_proj", h, cfg.num_attention_heads * cfg.head_dim, model)
        self.k_proj = ExLlamaV2Linear(self.ext, key + ".self_attn.k_proj", h, cfg.num_key_value_heads * cfg.head_dim, model)
        self.v_proj = ExLlamaV2Linear(self.ext, key + ".self_attn.v_proj", h, cfg.num_key_value_heads * cfg.head_dim, model)
        self.o_proj = ExLlamaV2Linear(self.ext, key + ".self_attn.o_proj", cfg.num_attention_heads * cfg.head_dim, h, model)
        self.pre_layernorm = None
        self.q_handle = None
        self.fused_decode = os.environ.get("EXL2_ATTN_FUSED", "1") != "0"       # A/B switch for measurements
        self.q4_fused = os.environ.get("EXL2_Q4_FUSED", "1") != "0"
        # Q4 decode steps in two launches (RoPE + pack of the new rows; attention with the split merge inside) instead of four
        # (EXL2_Q4_LAUNCHES=4: the round-4 sequence rope_kv_append -> fp16_to_q_kv -> paged_attn_q4 -> its combine launch) ...
        self.q4_two_launches = os.environ.get("EXL2_Q4_LAUNCHES", "1") != "4"
        # ... or ONE (RoPE + pack + attention + merge: csrc/attn_q4.hip, the FUSED form; head_dim 128) -- EXL2_Q4_LAUNCHES=2 keeps two
        self.q4_one_launch = os.environ.get("EXL2_Q4_LAUNCHES", "1") == "1"
        # q / k head norm (cfg.use_qk_norm) in the chained step on an FP16 cache: folded into the one-launch attention (csrc/attn_fused_body.h,
        # NORM) -- EXL2_QK_NORM_FUSED=0: a launch of its own behind the projections (csrc/head_norm.hip), the form every other route uses
        self.qk_norm_fused = os.environ.get("EXL2_QK_NORM_FUSED", "1") != "0"
        self.q_norm = self.k_norm = None

    def _q_entries(self, wbits: int):
        """(one-launch step, RoPE + pack, attention from the codes) of a quantized cache: the Q4 mirrors, or the width-carrying ones
        bound to 6 / 8 bits -- same kernels (csrc/attn_q4.hip, csrc/cache_q.hip), same switches"""
        ext = self.ext
        if wbits == 4:
            return ext.attn_q4_decode_fused, ext.rope_quant_append_q4, ext.paged_attn_q4
        return (functools.partial(ext.attn_q_decode_fused, wbits=wbits), functools.partial(ext.rope_quant_append_q, wbits=wbits),
                functools.partial(ext.paged_attn_q, wbits=wbits))

    def load(self, ck: dict):
        cfg, m = self.model.config, self.model
        for lin in (self.q_proj, self.k_proj, self.v_proj, self.o_proj):
            lin.load(ck[lin.key])
        # a parallel block (Cohere) owns the one norm of the layer: its attention handle has neither norm nor residual and overwrites
        # the normed rows it is given (parallel_decoder.py:47-55)
        parallel = bool(getattr(cfg, "parallel_decoder_blocks", False))
        ln = getattr(cfg, "norm", "rmsnorm") == "layernorm"
        self.pre_layernorm = None if parallel else m.norm_weight(ck[self.key + ".input_layernorm"])
        self.pre_layernorm_bias = None if parallel else ck.get(self.key + ".input_layernorm.bias")
        post = getattr(cfg, "post_norms", False)
        self.post_layernorm = m.norm_weight(ck[self.key + ".post_attention_layernorm"]) if post else None
        # per-layer sliding window and rotary table (model.py:111-121): window_left keys to the left, 0 = all
        gi = int(self.key.rsplit(".", 1)[1])                                    # global layer index ("model.layers.N"); layer_idx is local
        self.window = cfg.layer_window(gi)
        self.sin, self.cos = (m.sin_alt, m.cos_alt) if cfg.layer_rope_alt(gi) else (m.sin, m.cos)
        if getattr(cfg, "use_qk_norm", False):                                  # attn.py:196-198, 285-289
            # (the constant bias of the architecture's norms goes to the head norms too: headnorm.py:78-79)
            self.q_norm = self._head_norm_weight(m.norm_weight(ck[self.key + ".self_attn.q_norm"]), cfg.num_attention_heads, "q")
            self.k_norm = self._head_norm_weight(m.norm_weight(ck[self.key + ".self_attn.k_norm"]), cfg.num_key_value_heads, "k")
        qn = none_tensor if self.q_norm is None else self.q_norm
        kn = none_tensor if self.k_norm is None else self.k_norm
        self.q_handle = self.ext.make_q_attn(                                   # attn.py:300-330
            none_tensor if self.pre_layernorm is None else self.pre_layernorm,
            none_tensor if self.pre_layernorm_bias is None else self.pre_layernorm_bias, not ln,
            bool(getattr(cfg, "headnorm_rms", True)), cfg.norm_eps,
            self.q_proj.q_handle, self.k_proj.q_handle, self.v_proj.q_handle, self.o_proj.q_handle,
            m.temp_state, none_tensor, m.max_rows, cfg.hidden_size, cfg.num_attention_heads, cfg.num_key_value_heads,
            cfg.head_dim, cfg.max_seq_len, not parallel, cfg.rope_style, cfg.head_dim, qn, kn,
            none_tensor if self.post_layernorm is None else self.post_layernorm,
            none_tensor, bool(getattr(cfg, "residual_fp32", False)), False)
        return self

    def _head_norm_weight(self, w: torch.Tensor, heads: int, kind: str) -> torch.Tensor:
        """[heads, head_dim] fp16 on the module's device (a [head_dim] weight is shared by the heads: headnorm.py:59-66);
        kind "q" | "k": which head range a tensor-parallel rank cuts out (tensor_p.TPAttention)"""
        hd = self.model.config.head_dim
        if w.dim() == 1:
            w = w.view(1, hd).expand(heads, hd)
        if tuple(w.shape) != (heads, hd):
            raise RuntimeError(f"{self.key}: head-norm weight of shape {tuple(w.shape)}, expected ({heads}, {hd})")
        return w.to(device=self.model.device, dtype=torch.float16).contiguous()

    def chain_skip_head_norm(self, cache) -> bool:
        """chained step on an FP16 cache: q / k leave the projections un-normalised, attend_chain's launch normalises them"""
        return self.q_norm is not None and self.qk_norm_fused and not getattr(cache, "wbits", 0)

    def unload(self):
        if self.q_handle is not None:
            self.ext.free_q_attn(self.q_handle)                                  # attn handle before its linears
            self.q_handle = None
        for lin in (self.q_proj, self.k_proj, self.v_proj, self.o_proj):
            lin.unload()

    def update_loras(self) -> int:
        """attn.py:1545-1566: hands the adapters attached to the four linears to the handle (which copies them); returns the largest rank"""
        return self.ext.q_attn_set_loras(self.q_handle, self.q_proj.lora_table(), self.k_proj.lora_table(), self.v_proj.lora_table(),
                                         self.o_proj.lora_table())

    def forward(self, hidden_states: torch.Tensor, cache, past_len: int = 0, cache_seqlens=None, block_table=None, loras=None):
        """In place on hidden_states [b, q_len, hidden] (residual add in o_proj's epilogue).

        Contiguous mode (attn.py:1017-1196): scalar `past_len`, cache viewed [b, max_seq_len, kvh, hd].
        Paged mode (attn.py:466-638): `cache_seqlens` int32 [b] + `block_table` int32 [b, pages] on the device,
        cache viewed [pages, 256, kvh, hd]; positions are read on the device (graph-capturable).
        loras: the ExLlamaV2Lora adapters to apply (attn.py:1017-1031)."""
        b, q_len, _ = hidden_states.shape
        if loras:
            if type(self) is not ExLlamaV2Attention:
                raise RuntimeError(f"{type(self).__name__}: LoRA adapters are not built for this attention module")
            ids = [id(l) for l in loras]
            q, k, v = self._project_qkv(hidden_states, b, q_len, ids)
            attn_out = self._attend(q, k, v, cache, past_len, cache_seqlens, block_table)
            return self._project_out(hidden_states, attn_out, b, q_len, ids)
        q, k, v = self._project_qkv(hidden_states, b, q_len)
        attn_out = self._attend(q, k, v, cache, past_len, cache_seqlens, block_table)
        return self._project_out(hidden_states, attn_out, b, q_len)

    def _project_qkv(self, hidden_states, b: int, q_len: int, lora_ids=None):
        """Front half (q_attn_forward_1, q_attn.cu:153-317): RMSNorm + q/k/v projections into the scratch rows; RoPE is
        applied later, inside the attention launch."""
        cfg, m, ext = self.model.config, self.model, self.ext
        rows = b * q_len
        q = m.temp_q[:rows].view(b, q_len, cfg.num_attention_heads, cfg.head_dim)
        k = m.temp_k[:rows].view(b, q_len, cfg.num_key_value_heads, cfg.head_dim)
        v = m.temp_v[:rows].view(b, q_len, cfg.num_key_value_heads, cfg.head_dim)
        ext.q_attn_forward_1(self.q_handle, hidden_states, b, q_len, 0, none_tensor, q, k, v, m.sin, m.cos,
                             loras=lora_ids, apply_rope=False)
        return q, k, v

    def forward_normed(self, xn: torch.Tensor, b: int, q_len: int, cache, past_len: int = 0, cache_seqlens=None, block_table=None):
        """The module for a caller that owns the norms (a post-norm block): xn fp16 [b * q_len, hidden], already normed.  o_proj's output
        is left in the model's temp_state; the post norm is the caller's (ext.norm_bridge)."""
        cfg, m, ext = self.model.config, self.model, self.ext
        rows = b * q_len
        q = m.temp_q[:rows].view(b, q_len, cfg.num_attention_heads, cfg.head_dim)
        k = m.temp_k[:rows].view(b, q_len, cfg.num_key_value_heads, cfg.head_dim)
        v = m.temp_v[:rows].view(b, q_len, cfg.num_key_value_heads, cfg.head_dim)
        ext.q_attn_forward_1_normed(self.q_handle, xn, b, q_len, 0, none_tensor, q, k, v, m.sin, m.cos, apply_rope=False)
        attn_out = self._attend(q, k, v, cache, past_len, cache_seqlens, block_table)
        ext.q_attn_forward_2_normed(self.q_handle, attn_out, b, q_len)

    def attend_extras(self, cache):
        """(window_left, softcap) when this layer's attention needs the launches that carry them -- a window that can clip inside this
        cache, or a score cap -- else None: the one-launch decode attention (csrc/attn_fused_body.h) carries neither."""
        cap = float(getattr(self.model.config, "attn_logit_softcapping", 0.0) or 0.0)
        win = getattr(self, "window", 0)
        clips = win > 0 and win + 1 < cache.max_seq_len
        return (win if clips else -1, cap) if (clips or cap) else None

    def _attend(self, q, k, v, cache, past_len, cache_seqlens, block_table):
        """RoPE(q, new k) + KV append + attention over the (paged or contiguous, FP16 or Q4 / Q6 / Q8) cache -> attn_out rows."""
        cfg, m, ext = self.model.config, self.model, self.ext
        b, q_len = q.shape[0], q.shape[1]
        rows = b * q_len
        paged = block_table is not None
        if cache is None:
            raise RuntimeError("ExLlamaV2Attention.forward: a cache is required")
        attn_out = m.temp_attn[:rows].view(b, q_len, cfg.num_attention_heads, cfg.head_dim)
        # quantized cache (Q4 / Q6 / Q8), decode-sized step: attend straight from the codes (attn_q4.hip) -- the reference unpacks the whole live
        # range to an fp16 temp for every layer of every step (cache.py:472-514)
        # (the step's own K/V are attended in fp16 and quantised afterwards, the reference's order)
        wbits = getattr(cache, "wbits", 0)
        scale = cfg.softmax_scale()
        sin, cos = getattr(self, "sin", None), getattr(self, "cos", None)
        if sin is None: sin, cos = m.sin, m.cos
        extras = self.attend_extras(cache)
        if wbits and (extras is not None or scale != cfg.head_dim ** -0.5 or sin is not m.sin):
            raise RuntimeError(f"{self.key}: a quantized cache together with a sliding window, a score cap, a softmax scale or a rotary table "
                               f"of the layer's own is not built (the kernels that attend from the codes carry none of them)")
        q4_direct = (wbits in (4, 6, 8) and hasattr(cache, "q4_views") and self.q4_fused and q_len <= 8
                     and q_len * (cfg.num_attention_heads // cfg.num_key_value_heads) <= 64
                     and cfg.head_dim in (64, 128, 256)
                     and (cfg.num_key_value_heads * cfg.head_dim) % 512 == 0)     # codec blocks (512 elements) must not span tokens
        if paged:
            if not q4_direct:
                cache.get_kv_state(self.layer_idx, b, 0, 0, 256, cache_seqlens, block_table)
            kc, vc = cache.paged_view(self.layer_idx)
            sl, bt, past = cache_seqlens, block_table, 0
        else:
            if q4_direct:
                kc, vc = cache.get_kv_state(self.layer_idx, b, 0, 0)           # width 0: the temp pair, nothing unpacked
            else:
                kc, vc = cache.get_kv_state(self.layer_idx, b, 0, past_len)
            sl, bt, past = None, None, past_len
        if q4_direct:
            # new K/V -> (rotated) into the fp16 staging rows -> quantised into the cache -> attention over codes
            kq, ks, vq, vs = cache.q4_views(self.layer_idx, paged)
            two = getattr(self, "q4_two_launches", False)
            one_launch, rope_pack, attn_codes = self._q_entries(wbits)
            if getattr(self, "q4_one_launch", False) and one_launch(
                    q, k, v, kq, ks, vq, vs, attn_out, m.sin, m.cos, sl, bt, past, cfg.rope_style, m.attn_scratch, m.attn_counters):
                return attn_out
            if not (two and rope_pack(q, k, v, kq, ks, vq, vs, m.sin, m.cos, past if not paged else 0,
                                      sl if paged else none_tensor, bt if paged else none_tensor, cfg.rope_style)):
                ext.rope_kv_append(q, k, v, kc, vc, m.sin, m.cos, past if not paged else 0,
                                   sl if paged else none_tensor, bt if paged else none_tensor, cfg.rope_style)
                if paged:
                    cache.store_kv_state(self.layer_idx, b, 0, q_len, 256, cache_seqlens, block_table)
                else:
                    cache.store_kv_state(self.layer_idx, b, past_len, q_len)
            ok = attn_codes(q, kq, ks, vq, vs, attn_out, sl, bt, len_const=past, len_offset=q_len,
                            scratch=m.attn_scratch, k_new=k, v_new=v, counters=m.attn_counters if two else None)
            if not ok:
                raise RuntimeError("ExLlamaV2Attention: attention from the cache's codes rejected a shape it was selected for")
        else:
            # decode-shaped steps: one launch does RoPE + append + attention + split merge; otherwise three launches.  A layer with a
            # clipping window or a score cap always takes the three: rope_kv_append, then the attention launches that carry both
            wl, cap = extras if extras is not None else (-1, 0.0)
            fused = extras is None and self.fused_decode and ext.attn_decode_fused(
                q, k, v, kc, vc, attn_out, sin, cos, sl, bt, past, cfg.rope_style, m.attn_scratch, m.attn_counters, softmax_scale=scale)
            if not fused:
                ext.rope_kv_append(q, k, v, kc, vc, sin, cos, past if not paged else 0,
                                   sl if paged else none_tensor, bt if paged else none_tensor, cfg.rope_style)
                # many query rows: MFMA flash attention (csrc/attn_prefill.hip); decode-shaped: the split-KV kernel
                if not (q_len > 16 and ext.flash_prefill(q, kc, vc, attn_out, sl, bt, len_const=past, len_offset=q_len,
                                                         softmax_scale=scale, window_left=wl, softcap=cap)):
                    ext.paged_attn(q, kc, vc, attn_out, sl, bt, len_const=past, len_offset=q_len, softmax_scale=scale,
                                   scratch=m.attn_scratch, window_left=wl, softcap=cap)
            if paged:
                cache.store_kv_state(self.layer_idx, b, 0, q_len, 256, cache_seqlens, block_table)
            else:
                cache.store_kv_state(self.layer_idx, b, past_len, q_len)
        return attn_out

    def q4_chain_capable(self, cache) -> bool:
        """the chained step can attend straight from this quantized cache's codes (Q4 / Q6 / Q8; the conditions of _attend's
        q4_direct at q_len 1)"""
        cfg = self.model.config
        return (getattr(cache, "wbits", 0) in (4, 6, 8) and hasattr(cache, "q4_views") and self.q4_fused
                and cfg.num_attention_heads // cfg.num_key_value_heads <= 64 and cfg.head_dim in (64, 128, 256)
                and (cfg.num_key_value_heads * cfg.head_dim) % 512 == 0)

    def attend_chain(self, q, k, v, cache, cache_seqlens, block_table, out_invperm, head_norm_pending: bool = False,
                     rope_now=None, identity_table: bool = False):
        """Decode attention of the chained step (model.GreedyGraphDecoder), output written in o_proj's packed order.  Paged
        FP16 cache: the one-launch kernel.  Paged Q4 / Q6 / Q8 cache: RoPE + pack of the new rows (csrc/cache_q.hip: rope_quant_q4_kernel),
        attention straight from the codes with the split merge inside (csrc/attn_q4.hip) -- the two launches of _attend's q4_direct route.  Raises when
        the shape needs another path (the decoder then un-chains).  head_norm_pending: q / k come un-normalised (q_attn_forward_1_chain
        with skip_head_norm) -- the FP16 cache's launch normalises them in registers (csrc/attn_fused_body.h, NORM).
        rope_now / identity_table: handed to the FP16 cache's launch (ext.attn_decode_fused)."""
        cfg, m, ext = self.model.config, self.model, self.ext
        b, q_len = q.shape[0], q.shape[1]
        if getattr(cache, "wbits", 0):
            if head_norm_pending:
                raise RuntimeError("attend_chain: a quantized cache's attention takes normalised q / k")
            if not self.q4_chain_capable(cache):
                raise RuntimeError("attend_chain: shape not covered by the Q4 attention kernel")
            attn_out = m.temp_attn[:b * q_len].view(b, q_len, cfg.num_attention_heads, cfg.head_dim)
            kq, ks, vq, vs = cache.q4_views(self.layer_idx, True)
            two = getattr(self, "q4_two_launches", False)
            one_launch, rope_pack, attn_codes = self._q_entries(cache.wbits)
            if getattr(self, "q4_one_launch", False) and one_launch(
                    q, k, v, kq, ks, vq, vs, attn_out, m.sin, m.cos, cache_seqlens, block_table, 0, cfg.rope_style, m.attn_scratch,
                    m.attn_counters, out_invperm=out_invperm):
                return attn_out
            if not (two and rope_pack(q, k, v, kq, ks, vq, vs, m.sin, m.cos, 0, cache_seqlens, block_table, cfg.rope_style)):
                kc, vc = cache.paged_view(self.layer_idx)
                ext.rope_kv_append(q, k, v, kc, vc, m.sin, m.cos, 0, cache_seqlens, block_table, cfg.rope_style)
                cache.store_kv_state(self.layer_idx, b, 0, q_len, 256, cache_seqlens, block_table)
            if not attn_codes(q, kq, ks, vq, vs, attn_out, cache_seqlens, block_table, len_const=0, len_offset=q_len,
                              scratch=m.attn_scratch, k_new=k, v_new=v, out_invperm=out_invperm,
                              counters=m.attn_counters if two else None):
                raise RuntimeError("attend_chain: shape not covered by the Q4 attention kernel")
            return attn_out
        kc, vc = cache.paged_view(self.layer_idx)
        attn_out = m.temp_attn[:b * q_len].view(b, q_len, cfg.num_attention_heads, cfg.head_dim)
        hn = (self.q_norm, self.k_norm, cfg.norm_eps, cfg.headnorm_rms) if head_norm_pending else None
        if not ext.attn_decode_fused(q, k, v, kc, vc, attn_out, m.sin, m.cos, cache_seqlens, block_table, 0, cfg.rope_style,
                                     m.attn_scratch, m.attn_counters, out_invperm=out_invperm, head_norm=hn,
                                     rope_now=rope_now, identity_table=identity_table):
            raise RuntimeError("attend_chain: shape not covered by the one-launch attention kernel")
        return attn_out

    def _project_out(self, hidden_states, attn_out, b: int, q_len: int, lora_ids=None):
        """Back half (q_attn_forward_2, q_attn.cu:319-345): x += attn_out . Wo"""
        self.ext.q_attn_forward_2(self.q_handle, hidden_states, attn_out, b, q_len, loras=lora_ids)
        return hidden_states

