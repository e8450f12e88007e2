"""ExLlamaV2 model runtime for the Llama family (reference model.py:78-173 module list, :764-933 forward chunking,
:936-1054 forward_chunk) on one device, plus the whole-step greedy decode graph used by the benchmark."""
from __future__ import annotations

import math

import os

import torch

from .attn import ExLlamaV2Attention
from .cache import PAGE_SIZE
from .config import ExLlamaV2Config
from .ext import ext_c, none_tensor
from .layernorm import ExLlamaV2LayerNorm
from .linear import ExLlamaV2Linear
from .mlp import ExLlamaV2MLP
from .moe_mlp import ExLlamaV2MoEMLP
from .rmsnorm import ExLlamaV2RMSNorm


def rope_tables(cfg: ExLlamaV2Config, device, base: float | None = None):
    """device.py:118-169: fp16 sin/cos [max_seq_len, head_dim]; `base`: another rope base than the config's (rotary_embedding_base_alt)."""
    base = cfg.rotary_embedding_base if base is None else base
    inv_freq = 1.0 / (base ** (torch.arange(0, cfg.head_dim, 2, device=device).float() / cfg.head_dim))
    t = torch.arange(cfg.max_seq_len, device=device, dtype=torch.float32)
    freqs = torch.einsum("i,j->ij", t, inv_freq)
    emb = torch.cat((freqs, freqs), dim=-1) if cfg.rope_style == 2 else torch.repeat_interleave(freqs, 2, dim=-1)
    return emb.sin().half().contiguous(), emb.cos().half().contiguous()


def _dense_mlp_linears(mlp) -> list:
    """gate (absent in an ungated MLP), up and down of a dense MLP module"""
    return [lin for lin in (mlp.gate_proj, mlp.up_proj, mlp.down_proj) if lin is not None]


class ExLlamaV2:
    _live_on_device: dict = {}          # loaded models per device (the library's staging scratch is per device and stream)
    def __init__(self, config: ExLlamaV2Config, device="cuda:0", ext=None):
        self.config = config
        self.device = torch.device(device)
        self.ext = ext or ext_c
        cfg = config
        # per-device scratch arena (device.py:102-115): sized for one forward chunk
        # rows of one forward chunk: max_input_len x max_batch_size, as the reference sizes its scratch (model.py:195,
        # attn.py:315, mlp.py:216) -- prefill GEMMs want the tallest chunk the arena allows (288 GB: 8 x 2048 rows of a 7B are 1 GB)
        self.max_rows = cfg.max_input_len * max(1, cfg.max_batch_size)
        r, dev = self.max_rows, self.device
        self.temp_state = torch.empty((r, cfg.hidden_size), dtype=torch.float16, device=dev)
        self.temp_a = torch.empty((r, cfg.intermediate_size), dtype=torch.float16, device=dev)
        self.temp_b = torch.empty((r, cfg.intermediate_size), dtype=torch.float16, device=dev)
        self.temp_q = torch.empty((r, cfg.num_attention_heads * cfg.head_dim), dtype=torch.float16, device=dev)
        self.temp_k = torch.empty((r, cfg.num_key_value_heads * cfg.head_dim), dtype=torch.float16, device=dev)
        self.temp_v = torch.empty((r, cfg.num_key_value_heads * cfg.head_dim), dtype=torch.float16, device=dev)
        self.temp_attn = torch.empty((r, cfg.num_attention_heads * cfg.head_dim), dtype=torch.float16, device=dev)
        sb = self.ext.paged_attn_scratch_bytes(min(r, 64) * cfg.num_attention_heads, cfg.head_dim, 64)
        self.attn_scratch = torch.empty((sb // 4 + 16,), dtype=torch.float32, device=dev)
        self.attn_counters = torch.zeros((16384,), dtype=torch.int32, device=dev)     # split hand-off tickets (attn.hip)
        # parallel decoder blocks (Cohere): the two normed copies of the stream the attention and the MLP of a block run in place on
        self.par_a = self.par_b = None
        if cfg.parallel_decoder_blocks:
            self.par_a = torch.empty((r, cfg.hidden_size), dtype=torch.float16, device=dev)
            self.par_b = torch.empty((r, cfg.hidden_size), dtype=torch.float16, device=dev)
        self.block_norms = []                             # per layer (weight, bias | None): the .input_layernorm a parallel block owns
        self._dq = None                                   # reconstruct target of ExLlamaV2Linear.forward(force_recons=True)
        self.sin, self.cos = rope_tables(cfg, dev)
        # windowed layers of a model whose local attention has its own rope base (Gemma-3) rotate with a second table
        self.sin_alt, self.cos_alt = rope_tables(cfg, dev, cfg.rotary_embedding_base_alt) if cfg.rotary_embedding_base_alt else (None, None)
        self.modules = []
        self.layers = []
        self.embed_tokens = None
        self.norm = None
        self.lm_head = None
        self.loaded = False

    def dq_scratch(self, k: int, n: int, device) -> torch.Tensor:
        """fp16 [k, n] view of the per-device dequantisation scratch (reference: temp_dq, device.py:102-115); grows on demand"""
        if self._dq is None or self._dq.numel() < k * n:
            self._dq = torch.empty((k * n,), dtype=torch.float16, device=device)
        return self._dq[:k * n].view(k, n)

    def norm_weight(self, w: torch.Tensor) -> torch.Tensor:
        """an RMSNorm weight as the kernels take it: the architecture's constant bias added in fp16 (rmsnorm.py:57-59)"""
        b = float(getattr(self.config, "norm_constant_bias", 0.0) or 0.0)
        return (w + b).to(torch.float16).contiguous() if b else w

    def check_cache(self, cache) -> None:
        """a clear error for a cache this model's attention cannot use (the attention modules raise the same at their first call)"""
        if getattr(cache, "wbits", 0) and any(a.attend_extras(cache) is not None or getattr(a, "sin", self.sin) is not self.sin for a, _ in self.layers):
            raise RuntimeError("a quantized cache together with a sliding window or a score cap is not built: the kernels that attend "
                               "from the codes carry neither (use the FP16 cache)")
        if getattr(cache, "wbits", 0) and self.config.softmax_scale() != self.config.head_dim ** -0.5:
            raise RuntimeError("a quantized cache together with query_pre_attn_scalar is not built (use the FP16 cache)")

    def load(self, ck: dict, layers=None):
        """model.py:266-351: build the module handles from a checkpoint dict.  `layers` = the global layer indices this
        device owns (layer split, model.py:176-263); embedding / final norm + head are built when their tensors are in
        `ck`.  KV-cache slots are indexed by LOCAL layer position."""
        cfg = self.config
        self.embed_tokens = ck.get("model.embed_tokens")
        self.layer_ids = list(range(cfg.num_hidden_layers) if layers is None else layers)
        for local_idx, i in enumerate(self.layer_ids):
            key = f"model.layers.{i}"
            attn = ExLlamaV2Attention(self, key, local_idx).load(ck)
            if getattr(cfg, "num_experts", 0):
                mlp = ExLlamaV2MoEMLP(self, key, local_idx, cfg.num_experts, cfg.num_experts_per_token).load(ck)
            else:
                mlp = ExLlamaV2MLP(self, key, local_idx).load(ck)
            self.layers.append((attn, mlp))
            self.modules += [attn, mlp]
            if cfg.parallel_decoder_blocks:
                self.block_norms.append((ck[key + ".input_layernorm"], ck.get(key + ".input_layernorm.bias")))
        vpad = (cfg.vocab_size + 31) // 32 * 32
        self.vocab_padded = vpad
        if "lm_head" in ck:
            if cfg.layernorm:
                self.norm = ExLlamaV2LayerNorm(self.ext, "model.norm", ck["model.norm"], ck.get("model.norm.bias"), cfg.norm_eps)
            else:
                self.norm = ExLlamaV2RMSNorm(self.ext, "model.norm", self.norm_weight(ck["model.norm"]), cfg.norm_eps)
            # logit_scale is folded into the head's scales in fp16, as the reference's loader does (model.py:148 -> ext.py:336, :363)
            self.lm_head = ExLlamaV2Linear(self.ext, "lm_head", cfg.hidden_size, vpad, self).load(ck["lm_head"], prescale=cfg.logit_scale)
        if not self.loaded:
            ExLlamaV2._live_on_device[str(self.device)] = ExLlamaV2._live_on_device.get(str(self.device), 0) + 1
        self.loaded = True
        return self

    def unload(self):
        for attn, mlp in self.layers:
            attn.unload(); mlp.unload()
        if self.lm_head: self.lm_head.unload()
        was_loaded = self.loaded
        self.layers, self.modules, self.loaded = [], [], False
        # the staging buffers of this device's streams (csrc/qgemm_prefill.hip: activations up to 360 MB per stream, decoded weight
        # fragments K x N x 2 bytes) are shared by every model of the device and their addresses sit in captured graphs (a decoder
        # of 5-16 sequences): they go when the LAST loaded model of the device goes -- a draft model unloading must not pull
        # them from under the main model's graphs
        if was_loaded:
            k = str(self.device)
            ExLlamaV2._live_on_device[k] = max(0, ExLlamaV2._live_on_device.get(k, 1) - 1)
            if ExLlamaV2._live_on_device[k] == 0:
                self.ext.release_scratch(self.device)

    def linear_modules(self) -> dict:
        """key -> ExLlamaV2Linear of the layers' dense projections (what a LoRA adapter may target: exllamav2_amd/lora.py)"""
        out = {}
        for attn, mlp in self.layers:
            lins = [attn.q_proj, attn.k_proj, attn.v_proj, attn.o_proj]
            if hasattr(mlp, "gate_proj"):
                lins += _dense_mlp_linears(mlp)
            out.update({lin.key: lin for lin in lins})
        return out

    def update_loras(self) -> int:
        """model.py:355-364: every module rebuilds its adapter table from what is attached to its linears.  Graphs captured with the
        previous tables must not be replayed afterwards.  Returns the largest rank."""
        if self.config.layernorm:
            raise RuntimeError("LoRA adapters are not built for a LayerNorm model (StarCoder2, Cohere)")
        return max([m.update_loras() for m in self.modules if hasattr(m, "update_loras")] + [0])

    def weight_bytes(self) -> int:
        """Algorithmic bytes one token streams through the linears.  A sparse-MoE layer streams
        its router plus `num_experts_per_token` of its experts per token (moe_mlp.py:238-253)."""
        n = self.lm_head.weight_bytes() if self.lm_head else 0
        for attn, mlp in self.layers:
            for lin in (attn.q_proj, attn.k_proj, attn.v_proj, attn.o_proj):
                n += lin.weight_bytes()
            if hasattr(mlp, "gate_proj"):
                n += sum(lin.weight_bytes() for lin in _dense_mlp_linears(mlp))
            else:
                per_expert = sum(l.weight_bytes() for l in mlp.w1 + mlp.w2 + mlp.w3) // mlp.num_experts
                n += per_expert * mlp.num_experts_per_token + mlp.gate.numel() * 2
        return n

    # ---- forward ------------------------------------------------------------------------------------------------------

    def forward_chunk(self, input_ids: torch.Tensor, cache, past_len: int = 0, cache_seqlens=None, block_table=None,
                      last_id_only: bool = True, preprocess_only: bool = False, loras=None):
        """model.py:936-1054.  input_ids [b, q_len] (any device); returns logits [b, q_len | 1, vocab] or None.
        loras: the ExLlamaV2Lora adapters to apply in every layer (None / empty: the plain launches)."""
        cfg = self.config
        b, q_len = input_ids.shape
        assert b * q_len <= self.max_rows, "chunk larger than the scratch arena"
        if cfg.residual_fp32:
            return self._forward_chunk_fp32(input_ids, cache, past_len, cache_seqlens, block_table, last_id_only, preprocess_only, loras)
        if cfg.layernorm and loras:
            raise RuntimeError("LoRA adapters are not built for a LayerNorm model (StarCoder2, Cohere)")
        x = self.embed_tokens[input_ids.to(self.device).reshape(-1)].view(b, q_len, cfg.hidden_size).contiguous()
        if cfg.parallel_decoder_blocks:
            self._parallel_layers(x, b, q_len, cache, past_len, cache_seqlens, block_table)
            layers = []
        else:
            layers = self.layers
        for attn, mlp in layers:
            if loras:
                attn.forward(x, cache, past_len, cache_seqlens, block_table, loras=loras)
                mlp.forward(x, loras=loras)
                continue
            attn.forward(x, cache, past_len, cache_seqlens, block_table)
            mlp.forward(x)
        if preprocess_only:
            return None
        if last_id_only:
            x = x[:, -1:, :].contiguous()
        x = self.norm.forward(x)
        logits = self.lm_head.forward(x)
        return logits[..., :cfg.vocab_size]

    def _parallel_layers(self, x, b: int, q_len: int, cache, past_len, cache_seqlens, block_table, final_norm_out=None, bridge: bool = True):
        """The layers of a model with parallel decoder blocks (parallel_decoder.py:137-143) on the fp16 stream x [b, q_len, hidden], in
        place: per block n = LN(x), a = attn(n) and m = mlp(n) on two copies of n (handles without norm and residual: they overwrite the
        rows they are given), x += a, x += m as two fp16 adds in that order.  One launch (ext.parallel_bridge) does the two adds and the
        next block's norm into both copies; bridge=False, or a shape it declines: add, add, norm, norm as launches of their own --
        bit-identical.  final_norm_out: the last bridge also leaves the final norm of x there (the decoder's step)."""
        cfg, ext = self.config, self.ext
        rows = b * q_len
        x2 = x.view(rows, cfg.hidden_size)
        n0, n1 = self.par_a[:rows], self.par_b[:rows]

        def boundary(a, m, w, bias, o0, o1):
            bias = none_tensor if bias is None else bias
            if bridge and ext.parallel_bridge(x2, a, m, w, bias, o0, o1, cfg.norm_eps):
                return
            if a is not none_tensor:
                ext.add_f16_(x2, a)
                ext.add_f16_(x2, m)
            if w is not none_tensor:
                ext.layer_norm(x2, w, bias, o0, cfg.norm_eps)
                if o1 is not none_tensor:
                    ext.layer_norm(x2, w, bias, o1, cfg.norm_eps)

        boundary(none_tensor, none_tensor, self.block_norms[0][0], self.block_norms[0][1], n0, n1)
        for i, (attn, mlp) in enumerate(self.layers):
            attn.forward(n0.view(b, q_len, cfg.hidden_size), cache, past_len, cache_seqlens, block_table)
            mlp.forward(n1.view(b, q_len, cfg.hidden_size))
            if i + 1 < len(self.layers):
                boundary(n0, n1, self.block_norms[i + 1][0], self.block_norms[i + 1][1], n0, n1)
            elif final_norm_out is not None:
                boundary(n0, n1, self.norm.weight, self.norm.bias, final_norm_out, none_tensor)
            else:
                boundary(n0, n1, none_tensor, None, none_tensor, none_tensor)

    def embed_scale(self) -> float:
        cfg = self.config
        return float(cfg.hidden_size) ** 0.5 if cfg.normalize_embeddings else 1.0

    def _forward_chunk_fp32(self, input_ids, cache, past_len, cache_seqlens, block_table, last_id_only, preprocess_only, loras):
        """forward_chunk of a model with an fp32 residual stream (Gemma-2 / Gemma-3): fp32 x from the scaled embedding
        (embedding.py:184-187), every module through its handle (pre-norm fp32 -> fp16, post norm added in fp32), the final norm
        fp32 -> fp16, the head, the cap on the fp16 logits (model.py:1043-1044)."""
        cfg, ext = self.config, self.ext
        if loras:
            raise RuntimeError("LoRA adapters are not built for a model with an fp32 residual stream")
        b, q_len = input_ids.shape
        ids = input_ids.to(device=self.device, dtype=torch.int32).reshape(-1).contiguous()
        x = torch.empty((b, q_len, cfg.hidden_size), dtype=torch.float32, device=self.device)
        ext.embed_rows_f32(self.embed_tokens, ids, x.view(b * q_len, cfg.hidden_size), self.embed_scale())
        for attn, mlp in self.layers:
            attn.forward(x, cache, past_len, cache_seqlens, block_table)
            mlp.forward(x)
        if preprocess_only:
            return None
        if last_id_only:
            x = x[:, -1:, :].contiguous()
        xn = torch.empty(x.shape, dtype=torch.float16, device=self.device)
        ext.rms_norm(x.view(-1, cfg.hidden_size), self.norm.weight, xn.view(-1, cfg.hidden_size), cfg.norm_eps)
        logits = self.lm_head.forward(xn)
        if cfg.final_logit_softcapping:
            ext.softcap_(logits, cfg.final_logit_softcapping)
        return logits[..., :cfg.vocab_size]

    def forward(self, input_ids: torch.Tensor, cache, last_id_only: bool = True, preprocess_only: bool = False,
                input_mask=None, loras=None):
        """model.py:764-933: contiguous-cache forward with chunked prefill; advances cache.current_seq_len."""
        b, q_len = input_ids.shape
        chunk = max(1, self.max_rows // b)                    # model.py:833 effective_max_input_len
        past = cache.current_seq_len
        assert past + q_len <= cache.max_seq_len, "sequence exceeds cache"
        out = None
        pos = 0
        while pos < q_len:
            n = min(chunk, q_len - pos)
            last = pos + n == q_len
            r = self.forward_chunk(input_ids[:, pos:pos + n], cache, past + pos,
                                   last_id_only=last_id_only, preprocess_only=preprocess_only or (last_id_only and not last),
                                   loras=loras)
            if r is not None:
                out = r if (out is None or last_id_only) else torch.cat([out, r], dim=1)
            pos += n
        cache.current_seq_len = past + q_len
        return out


class _PartialSums:
    """Host-side layout of one buffer of partial sums of squares of the chained step.  A producer launch writes its rows packed,
    `[rows, P]` with P = the number of partials per row it published (known when the launch returns); a consumer launch reads
    `[rows, P]` from one base pointer.  Launches of a step may group the rows differently (csrc/qgemv_lean.hip ROWS form: the rows
    that fit in LDS depend on K), so groups are packed one behind the other and a consumer's rows must come out contiguous with one
    P -- which they do whenever the producer groups they span published the same P."""

    def __init__(self, buf: torch.Tensor, rows: int):
        self.buf, self.rows = buf.view(-1), rows
        self.pos, self.count = [0] * rows, [1] * rows
        self.next = 0

    def begin(self):
        """a producer pass over all rows starts"""
        self.next = 0

    def out(self, r0: int, r1: int) -> torch.Tensor:
        self._pending = (r0, r1, self.next)
        return self.buf[self.next:]

    def done(self, count: int):
        r0, r1, start = self._pending
        if start + (r1 - r0) * count > self.buf.numel():
            raise RuntimeError("chained decode: partial sums exceed their buffer: shape not covered by the chained decode kernel")
        for r in range(r0, r1):
            self.pos[r], self.count[r] = start + (r - r0) * count, count
        self.next = start + (r1 - r0) * count

    def inp(self, r0: int, r1: int, what: str):
        c = self.count[r0]
        if any(self.count[r] != c or self.pos[r] != self.pos[r0] + (r - r0) * c for r in range(r0, r1)):
            raise RuntimeError(f"chained decode: {what} rows {r0}..{r1 - 1} were produced with different numbers of partial sums: "
                               f"shape not covered by the chained decode kernel")
        return self.buf[self.pos[r0]:], c


class GreedyGraphDecoder:
    """One greedy decode step (embedding -> all layers -> norm -> head -> argmax -> advance positions) captured as a HIP
    graph.  Procedure = test_inference.py:604-609 (forward(ids[:, -1:], cache); argmax; append) with the token feedback
    and the position counters kept on the device, so a token costs one graph launch and no host synchronisation."""

    def __init__(self, model: ExLlamaV2, cache, batch_size: int = 1, max_new_tokens: int = 4096, loras=None):
        """loras: ExLlamaV2Lora adapters every step applies.  Such a decoder takes the module-by-module step (the chained decode
        kernels carry no adapters), still one captured graph per token."""
        self.model, self.cache, self.b = model, cache, batch_size
        self.q_len = 1                # rows per sequence of a step (b = sequences x q_len; speculative.SpeculativeGraphDecoder: K + 1)
        self.loras = list(loras) if loras else None
        cfg, dev = model.config, model.device
        pages_per_seq = cache.max_seq_len // PAGE_SIZE
        assert cache.max_seq_len % PAGE_SIZE == 0
        # contiguous cache rows seen through an identity block table (attn_params.py:241-257 "is_sequential")
        self.block_table = (torch.arange(batch_size * pages_per_seq, dtype=torch.int32, device=dev)
                            .view(batch_size, pages_per_seq).contiguous())
        self.cache_seqlens = torch.zeros((batch_size,), dtype=torch.int32, device=dev)
        self.ids = torch.zeros((batch_size,), dtype=torch.int32, device=dev)
        self.history = torch.zeros((batch_size, cache.max_seq_len + 2), dtype=torch.int32, device=dev)
        self.fp32 = bool(cfg.residual_fp32)
        # a LayerNorm model decodes module by module (the chained kernels publish sums of squares for an RMS consumer); parallel blocks:
        # one ext.parallel_bridge launch per block boundary, EXL2_PARALLEL_BRIDGE=0: the separate launches (A/B runs, the identity test)
        self.layernorm = bool(cfg.layernorm)
        self.parallel_bridge = bool(cfg.parallel_decoder_blocks) and os.environ.get("EXL2_PARALLEL_BRIDGE", "1") != "0"
        if self.layernorm and self.loras:
            raise RuntimeError("LoRA adapters are not built for a LayerNorm model (StarCoder2, Cohere)")
        if self.fp32 and self.loras:
            raise RuntimeError("LoRA adapters are not built for a model with an fp32 residual stream")
        model.check_cache(cache)
        self.x = torch.zeros((batch_size, 1, cfg.hidden_size), dtype=torch.float32 if self.fp32 else torch.float16, device=dev)
        self.xn = torch.zeros((batch_size, 1, cfg.hidden_size), dtype=torch.float16, device=dev)
        # fp32 residual stream: one launch for the two norms at every module boundary (ext.norm_bridge); EXL2_NORM_BRIDGE=0: the
        # handles' own two launches (the A/B of tools/gemma_decode_bench.py, and the tests)
        self.norm_bridge = self.fp32 and os.environ.get("EXL2_NORM_BRIDGE", "1") != "0"
        self.logits = torch.zeros((batch_size, model.vocab_padded), dtype=torch.float16, device=dev)
        self.graph = None
        # capture is not permitted on the legacy default stream: the decoder owns a stream (device.py:67-72 does too)
        self.stream = torch.cuda.Stream(device=dev) if dev.type == "cuda" else None
        self.chain = None
        self.pos = 0                  # host mirror of cache_seqlens (all rows advance together): bounds are checked here,
        self.limit = min(cache.max_seq_len, cfg.max_seq_len)      # the kernels index pages / sin-cos rows unchecked
        if os.environ.get("EXL2_CHAIN", "1") != "0" and not self.loras and not self.fp32 and not self.layernorm:
            self._setup_chain()
        if os.environ.get("EXL2_CHAIN_OVERLAP", "0") != "0" and (self.chain is None or "flags" not in self.chain):
            raise RuntimeError("EXL2_CHAIN_OVERLAP=1 asked for the experimental overlapped chain, but this model / cache / batch is "
                               "not chain-capable (dense layers with shared q|k|v and gate|up permutations, FP16 cache, <= 16 rows)")

    def _setup_chain(self):
        """Chained decode (csrc/qgemv_flat.hip): every producer of the residual stream leaves it in its consumer's packed
        (act-order) order + partial sums of squares.  Needs: dense layers whose q/k/v and gate/up share a permutation (every
        quantizer-written checkpoint), an FP16 or Q4 / Q6 / Q8 paged-view cache, a head on this device, <= 16 rows."""
        m, ext, cfg = self.model, self.model.ext, self.model.config
        if self.b > 16 or m.lm_head is None or m.embed_tokens is None:
            return
        # (the chained attention launch carries no window, score cap, softmax scale or second rotary table)
        if cfg.softmax_scale() != cfg.head_dim ** -0.5 or cfg.final_logit_softcapping or any(
                attn.attend_extras(self.cache) is not None or getattr(attn, "sin", m.sin) is not m.sin for attn, _ in m.layers):
            return
        if getattr(self.cache, "wbits", 0) and not all(attn.q4_chain_capable(self.cache) for attn, _ in m.layers):
            return
        if os.environ.get("EXL2_CHAIN_OVERLAP", "0") != "0" and any(getattr(attn, "q_norm", None) is not None for attn, _ in m.layers):
            return                  # (the q / k head norm is not built for the experimental overlapped chain)
        plan = []
        for attn, mlp in m.layers:
            if mlp.q_handle is None or attn.q_handle is None:
                return
            cap_a, in_a, o_inv, nw_a = ext.q_attn_chain_info(attn.q_handle)
            if hasattr(mlp, "gate_proj"):
                cap_m, in_m, nw_m = ext.q_mlp_chain_info(mlp.q_handle)
            elif hasattr(mlp, "num_experts") and os.environ.get("EXL2_CHAIN_MOE", "1") != "0" and "EXL2_CHAIN_OVERLAP" not in os.environ:
                # a sparse-MoE block (round 6): the attention half of the layer is chained (q|k|v from the published hand-off, o_proj
                # accumulating into x without publishing), the block itself reads x (its front kernel norms and routes), and its
                # result is published for the next layer's q|k|v by one small launch -- in_m = "moe" marks it
                cap_m, in_m, nw_m = True, "moe", None
            else:
                return
            if not (cap_a and cap_m):
                return
            plan.append((in_a, o_inv, in_m, nw_a, nw_m))
        dev = m.device
        head_perm, head_inv = ext.q_matrix_perm_info(m.lm_head.q_handle)
        norm_head = torch.empty_like(m.norm.weight)
        ext.gather_f16(m.norm.weight, head_perm, norm_head)
        self.chain = {
            "plan": plan, "head_inv": head_inv, "norm_head": norm_head,
            "xp_a": torch.zeros((self.b, cfg.hidden_size), dtype=torch.float16, device=dev),
            "xp_b": torch.zeros((self.b, cfg.hidden_size), dtype=torch.float16, device=dev),
            "ss_a": torch.zeros((self.b, 512), dtype=torch.float32, device=dev),
            "ss_b": torch.zeros((self.b, 512), dtype=torch.float32, device=dev),
        }
        # the rotary rows of the step's position, looked up once by the step's first launch for all layers (csrc/attn_fused_body.h: ROPE_NOW)
        if cfg.rope_style == 2 and m.sin is not None and tuple(m.sin.shape[1:]) == (cfg.head_dim,) and not getattr(self.cache, "wbits", 0):
            self.chain["rope_now"] = torch.zeros((self.b, 2, cfg.head_dim), dtype=torch.float16, device=dev)
        # 5-16 sequences (round 4): every q_gemm launch runs on the lean kernel, whose ROWS form stages the whole rows once per
        # workgroup when rows x (K + 8) x 2 bytes fit in LDS (csrc/qgemv_lean.hip) -- launches with a larger K (down_proj) run as
        # row groups, each group streaming the weights again (the later ones from the memory-side cache).  EXL2_CHAIN_ROWGROUPS=N
        # forces groups of N rows for every launch, 0 = one group whatever the kernel underneath makes of it.
        rg = os.environ.get("EXL2_CHAIN_ROWGROUPS", "auto")
        if rg != "auto" and int(rg) > 0 and self.b > 4:
            self.chain["group_rows"] = int(rg)
        self.chain["group_auto"] = rg == "auto"
        # overlapped chain (csrc/chain_sync.h, EXPERIMENTAL): launches alternate between the decoder's stream and a second
        # one, each waits for its predecessor through words in memory.  5 launches per layer + the head (+ the gate's block).
        if os.environ.get("EXL2_CHAIN_OVERLAP", "0") != "0":
            self.chain["flags"] = torch.zeros((5 * len(plan) + 4, ext.SYNC_BLOCK_WORDS), dtype=torch.int32, device=dev)
            # (another PRIORITY class: torch hands out streams from a pool and two of them may share a hardware queue -- the launches
            # of the two graphs would then run one after the other and every wait of the first would spin until it gives up;
            # queues of different priorities are never shared)
            self.chain["stream_b"] = torch.cuda.Stream(device=dev, priority=-1) if dev.type == "cuda" else None
            if dev.type == "cuda":
                self.chain["ev_pre"], self.chain["ev_b"] = torch.cuda.Event(), torch.cuda.Event()
            self.graph_b = None
        # 5-16 sequences, EXL2_XP_TILED=1 (round 4, measured SLOWER than the default and therefore off: profiles/history/r04_xp_tiled_sweep.txt
        # -- 7B bs = 16: 6460 vs 6652 tok/s, bs = 5: 2251 vs 2565): the hand-off buffers xp in the layout the matrix cores read
        # ([K / 8][16 rows][8]: include/exl2_hip.h, exl2_chain_set_tiled) -- q|k|v, gate|up and the head then take the lean kernel's
        # XMEM form (A operands straight from memory, no staged copy); o_proj keeps the ROWS form (attention writes row-major).
        # The default keeps that layout for ONE hand-off only: gate|up -> down where down's rows do not fit the LDS (csrc/modules.hip)
        if (self.b > 4 and "flags" not in self.chain and rg == "auto" and int(os.environ.get("EXL2_LEAN_XMEM", "1")) >= 1
                and os.environ.get("EXL2_XP_TILED", "0") != "0" and os.environ.get("EXL2_LEAN", "1") != "0"):
            self.chain["xp_tiled"] = True
            for name in ("xp_a", "xp_b"):
                self.chain[name] = torch.zeros((16, cfg.hidden_size), dtype=torch.float16, device=dev)

    def step_chain(self):
        m, ext, cfg, ch = self.model, self.model.ext, self.model.config, self.chain
        b, plan = self.b, ch["plan"]
        x2 = self.x.view(b, cfg.hidden_size)
        seqs, q_len = b // self.q_len, self.q_len
        q = m.temp_q[:b].view(seqs, q_len, cfg.num_attention_heads, cfg.head_dim)
        k = m.temp_k[:b].view(seqs, q_len, cfg.num_key_value_heads, cfg.head_dim)
        v = m.temp_v[:b].view(seqs, q_len, cfg.num_key_value_heads, cfg.head_dim)
        qr, kr, vr = q.view(b, -1), k.view(b, -1), v.view(b, -1)      # the same rows, one per index: what a row group slices
        xp_a, xp_b, ss_a, ss_b = ch["xp_a"], ch["xp_b"], ch["ss_a"], ch["ss_b"]
        overlap = "flags" in ch
        # Row groups: a launch of the lean kernel takes the rows whose staged copy fits in LDS (<= 16; <= 4 in its wave-private
        # form); more sequences run that launch once per group of rows.  A group's (xp, ss) live in its own rows of the buffers;
        # attention takes all rows in one launch.  Launches with different K may use different groupings: the number of partial
        # sums of squares per row a producer published must then be the same for all its groups (checked).
        def groups_for(K):
            g = ch.get("group_override", {}).get(K)            # what a declined launch of this K was regrouped to (_launch_step)
            if overlap or (b <= 4 and not g):
                return [(0, b)]
            g = g or ch.get("group_rows")
            if not g:
                if not ch.get("group_auto", True):
                    return [(0, b)]
                lds = int(os.environ.get("EXL2_CHAIN_ROWS_LDS", 132 * 1024))     # rows next to ~26 KB of scale rows and partial sums
                fit = lds // ((K + 8) * 2)
                # (rows that do not fit: the lean kernel's XMEM form reads the A operands from memory -- one launch for all rows;
                # EXL2_LEAN_XMEM=0: its row groups of round 4's first form)
                xmem = int(os.environ.get("EXL2_LEAN_XMEM", "1")) >= 1
                g = b if (fit >= b or xmem) else (fit if fit >= 5 else 4)
                g = -(-b // -(-b // g))                             # equal groups: 16 rows at 6 per launch -> 6 + 5 + 5
            return [(r, min(r + g, b)) for r in range(0, b, g)]

        groups_h = groups_for(cfg.hidden_size)                    # q|k|v, gate|up, head: K = hidden
        groups_o = groups_for(cfg.num_attention_heads * cfg.head_dim)
        groups_d = groups_for(cfg.intermediate_size)              # down: K = intermediate
        groups = groups_h
        pa, pb = _PartialSums(ss_a, b), _PartialSums(ss_b, b)
        pa.begin()
        tiled = bool(ch.get("xp_tiled")) and groups_h == groups_o == groups_d == [(0, b)]
        if tiled:
            ext.chain_set_tiled(True)
        try:
            for r0, r1 in groups:
                rn = ch.get("rope_now")
                ext.embed_rows_chain(m.embed_tokens, self.ids[r0:r1], x2[r0:r1], plan[0][0], plan[0][3], xp_a[r0:r1], pa.out(r0, r1),
                                     self.cache_seqlens[r0:r1], m.sin, m.cos, None if rn is None else rn[r0:r1])
                pa.done(1)
        except Exception:
            ext.chain_set_tiled(False)
            raise
        if overlap:
            sa = self.stream.cuda_stream if self.stream is not None else None
            sb = ch["stream_b"].cuda_stream if ch["stream_b"] is not None else None
            ext.chain_overlap_begin(ch["flags"], sa, sb)
        try:
            # partial sums of squares per row a launch published: the count depends on which kernel took the launch (qgemv_lean:
            # one per 16-column tile, qgemv_flat: one per workgroup) and a 4-row group and a 3-row group of the same matrix may be
            # taken by different kernels -- the consumer may group the rows differently, so all groups must agree
            for i, (attn, mlp) in enumerate(m.layers):
                in_a, o_inv, in_m, nw_a, nw_m = plan[i]
                # (a q / k head norm: folded into the FP16 cache's attention launch, a launch of its own ahead of a quantized cache's)
                skip_hn = attn.chain_skip_head_norm(self.cache)
                for r0, r1 in groups_h:
                    ss, cnt = pa.inp(r0, r1, "q|k|v")
                    ext.q_attn_forward_1_chain(attn.q_handle, xp_a[r0:r1], ss, cnt, r1 - r0, qr[r0:r1], kr[r0:r1], vr[r0:r1], skip_head_norm=skip_hn)
                # (self.block_table is the identity: the launch may address the rows directly)
                ao = attn.attend_chain(q, k, v, self.cache, self.cache_seqlens, self.block_table, o_inv, head_norm_pending=skip_hn,
                                       rope_now=ch.get("rope_now"), identity_table=True).view(b, -1)
                # every producer of the residual stream publishes it times its consumer's norm weight, in that consumer's order
                nxt, nxt_w = (plan[i + 1][0], plan[i + 1][3]) if i + 1 < len(plan) else (ch["head_inv"], ch["norm_head"])
                if in_m == "moe":
                    for r0, r1 in groups_o:
                        ext.q_attn_forward_2_chain(attn.q_handle, x2[r0:r1], ao[r0:r1], r1 - r0, None, None, None, None)
                    pa.begin()
                    if groups_h == [(0, b)]:
                        pa.done(ext.q_moe_mlp_forward_chain(mlp.q_handle, x2, b, nxt, nxt_w, xp_a, pa.out(0, b)))
                    else:
                        mlp.forward(self.x)
                        for r0, r1 in groups_h:
                            ext.publish_rows(x2[r0:r1], r1 - r0, cfg.hidden_size, nxt, nxt_w, xp_a[r0:r1], pa.out(r0, r1))
                            pa.done(1)
                    continue
                pb.begin()
                for r0, r1 in groups_o:
                    pb.done(ext.q_attn_forward_2_chain(attn.q_handle, x2[r0:r1], ao[r0:r1], r1 - r0, in_m, nw_m, xp_b[r0:r1], pb.out(r0, r1)))
                if groups_h == groups_d and os.environ.get("EXL2_CHAIN_SPLIT_MLP", "0") != "1":     # (1: test hook)
                    pa.begin()
                    for r0, r1 in groups_h:
                        ss, cnt = pb.inp(r0, r1, "gate|up")
                        pa.done(ext.q_mlp_forward_chain(mlp.q_handle, x2[r0:r1], xp_b[r0:r1], ss, cnt, r1 - r0, nxt, nxt_w,
                                                        xp_a[r0:r1], pa.out(r0, r1)))
                else:
                    # the halves separately: gate | up over its groups, then down over its own
                    for r0, r1 in groups_h:
                        ss, cnt = pb.inp(r0, r1, "gate|up")
                        ext.q_mlp_forward_chain_part(mlp.q_handle, 1, r0, x2[r0:r1], xp_b[r0:r1], ss, cnt, r1 - r0, None, None, None, None)
                    pa.begin()
                    for r0, r1 in groups_d:
                        pa.done(ext.q_mlp_forward_chain_part(mlp.q_handle, 2, r0, x2[r0:r1], None, None, 0, r1 - r0, nxt, nxt_w,
                                                             xp_a[r0:r1], pa.out(r0, r1)))
            for r0, r1 in groups_h:
                ss, cnt = pa.inp(r0, r1, "head")
                ext.gemm_half_q_half_chain(xp_a[r0:r1], ss, cnt, cfg.norm_eps, m.lm_head.q_handle, self.logits[r0:r1], r1 - r0)
        finally:
            if tiled:
                ext.chain_set_tiled(False)
            n_launches = ext.chain_overlap_end() if overlap else 0
        # greedy sampling + position increment behind the head: on the stream the head went to
        import contextlib
        on_b = overlap and ch["stream_b"] is not None and (n_launches - 1) % 2 == 1
        with (torch.cuda.stream(ch["stream_b"]) if on_b else contextlib.nullcontext()):
            self._select_token()

    def _select_token(self):
        """last launch(es) of a step: greedy arg-max, or -- while a sampled graph is being captured / run eagerly -- the device
        sampler reading its random point from the decoder's buffer, + the counter increment"""
        ext, cfg = self.model.ext, self.model.config
        sm = getattr(self, "_sampling", None)
        if sm is None:
            ext.argmax_rows(self.logits, self.ids, cfg.vocab_size, self.history, self.cache_seqlens, pos_inc=1)
            return
        logits = self._penalised_logits(sm)
        ch = sm.get("chain")
        if ch is None:
            ext.sample_rows_step(logits, sm["temperature"], sm["top_k"], sm["top_p"], sm["min_p"], sm["randoms"], sm["counter"],
                                 self.ids, sm["probs"], sm["ws"], self.history, self.cache_seqlens, pos_inc=1, vocab=cfg.vocab_size)
        else:
            ext.sample_rows_chain_step(logits, ch["temperature"], sm["top_k"], sm["top_p"], sm["min_p"], sm["randoms"], sm["counter"],
                                       self.ids, sm["probs"], sm["ws"], self.history, self.cache_seqlens, pos_inc=1,
                                       vocab=cfg.vocab_size, **ch["kw"])
        ext.add_i32_(sm["counter"], 1)

    # ---- the rest of the reference sampler's chain (sampler.py:54-110 Settings names), on the device: csrc/sampling.hip CHAIN -------
    CHAIN_DEFAULTS = {"top_a": 0.0, "tfs": 0.0, "typical": 0.0, "temperature_last": False, "smoothing_factor": 0.0, "min_temp": 0.0,
                      "max_temp": 0.0, "temp_exponent": 1.0, "skew": 0.0, "mirostat": False, "mirostat_tau": 1.5,
                      "mirostat_eta": 0.1, "return_top_tokens": 0}

    def _split_settings(self, kw: dict):
        """(chain settings, penalty settings) of the keywords of a sampled run"""
        chain = {k: v for k, v in kw.items() if k in self.CHAIN_DEFAULTS}
        return chain, {k: v for k, v in kw.items() if k not in self.CHAIN_DEFAULTS}

    def _chain_state(self, kw: dict, temperature: float, old=None):
        """The chain settings of a sampled run as what the launch needs: None when all of them are neutral -- the sampled step is
        then exactly the launch without them.  temperature_last moves the temperature behind the truncation stages like
        sampler.py:540-559 does (softmax at 1, post-softmax temperature = the setting).  mu lives in `self.mirostat_mu` (fp32 [batch],
        0 = not yet initialised), the top tokens and their probabilities of the LAST sampled step in `self.top_tokens` /
        `self.top_probs` ([batch, return_top_tokens]): a report needs the step it is made for, and a captured step can only write
        to addresses fixed at capture.  `old`: a state (the captured step's) that is returned as it is when its settings are these --
        its buffers are the ones the captured launch writes, and `top_tokens` / `top_probs` point at them again."""
        st = self.CHAIN_DEFAULTS | kw
        K = int(st["return_top_tokens"])
        key = (float(st["top_a"]), float(st["tfs"]), float(st["typical"]), bool(st["temperature_last"]), float(st["smoothing_factor"]),
               float(st["min_temp"]), float(st["max_temp"]), float(st["temp_exponent"]), float(st["skew"]), bool(st["mirostat"]),
               float(st["mirostat_tau"]), float(st["mirostat_eta"]), K)
        active = (key[0] > 0 or 0 < key[1] < 1 or 0 < key[2] < 1 or (key[3] and float(temperature) != 1.0) or key[4] > 0
                  or key[6] > key[5] or key[8] != 0 or key[9] or K > 0)
        if not active:
            return None
        if old is not None and old["key"] == key + (float(temperature),):
            if "out_ktokens" in old["kw"]:
                self.top_tokens, self.top_probs = old["kw"]["out_ktokens"], old["kw"]["out_kprobs"]
            return old
        dev = self.logits.device
        kwargs = {"top_a": key[0], "tfs": key[1], "typical": key[2], "post_temperature": float(temperature) if key[3] else 1.0,
                  "min_temp": key[5], "max_temp": key[6], "temp_exponent": key[7], "smoothing_factor": key[4], "skew": key[8],
                  "mirostat": key[9], "mirostat_tau": key[10], "mirostat_eta": key[11]}
        if key[9]:
            if getattr(self, "mirostat_mu", None) is None:
                self.mirostat_mu = torch.zeros((self.b,), dtype=torch.float32, device=dev)
            kwargs["mirostat_mu"] = self.mirostat_mu
        if K > 0:
            if getattr(self, "top_tokens", None) is None or self.top_tokens.shape[-1] != K:
                self.top_tokens = torch.zeros((self.b, K), dtype=torch.int32, device=dev)
                self.top_probs = torch.zeros((self.b, K), dtype=torch.float32, device=dev)
            kwargs["out_ktokens"], kwargs["out_kprobs"] = self.top_tokens, self.top_probs
        return {"key": key + (float(temperature),), "temperature": 1.0 if key[3] else float(temperature), "kw": kwargs}

    # ---- the reference sampler's penalties and token bias (sampler.py:408-429), on the device: csrc/penalties.hip --------------
    PENALTY_DEFAULTS = {"token_repetition_penalty": 1.0, "token_repetition_range": -1, "token_repetition_decay": 0,
                        "token_frequency_penalty": 0.0, "token_presence_penalty": 0.0, "token_bias": None}

    def _penalty_state(self, kw: dict, old=None):
        """The penalty / bias settings of a sampled run (the reference Settings' names) as what the launches need: None when all of
        them are neutral -- the sampled step is then exactly the launches without them.  `old`: a state whose buffers are reused
        when its settings are these."""
        unknown = set(kw) - set(self.PENALTY_DEFAULTS)
        if unknown:
            raise TypeError(f"sampled decoding: unknown setting(s) {sorted(unknown)}")
        st = self.PENALTY_DEFAULTS | kw
        bias = st["token_bias"]
        key = (float(st["token_repetition_penalty"]), int(st["token_repetition_range"]), int(st["token_repetition_decay"]),
               float(st["token_frequency_penalty"]), float(st["token_presence_penalty"]))
        if key[0] == 1.0 and key[3] == 0.0 and key[4] == 0.0 and bias is None:
            return None
        if key[1] < -1 or key[2] < 0:
            raise RuntimeError(f"sampled decoding: token_repetition_range {key[1]} / token_repetition_decay {key[2]}")
        cfg, dev = self.model.config, self.logits.device
        if bias is not None:
            bias = bias.detach().reshape(-1).to(torch.float32).cpu()
            if bias.numel() < cfg.vocab_size:
                raise RuntimeError("sampled decoding: token_bias must hold one entry per token of the vocabulary")
            bias = bias[:cfg.vocab_size].contiguous()
        if old is not None and old["key"] == key and (bias is None) == (old["bias"] is None) and (
                bias is None or torch.equal(bias, old["bias_host"])):
            return old
        ramps = self.model.ext.penalty_ramps(key[0], key[2], key[3], key[4])
        return {"key": key, "bias_host": bias, "bias": None if bias is None else bias.to(dev),
                "ramps": None if ramps is None else ramps.to(dev),
                "out": torch.zeros((self.b, cfg.vocab_size), dtype=torch.float32, device=dev)}

    def _penalised_logits(self, sm, pos_offset: int = 0):
        """penalties, then bias (the reference's order), from the step's fp16 logits into the sampled state's fp32 buffer; the logits
        themselves when the settings are neutral"""
        pen = sm.get("pen")
        if pen is None:
            return self.logits
        k = pen["key"]
        self.model.ext.apply_penalties(self.logits, pen["out"], self.history, self.cache_seqlens, k[0], k[1], k[2], k[3], k[4],
                                       ramps=pen["ramps"], token_bias=pen["bias"], vocab=self.model.config.vocab_size,
                                       pos_offset=pos_offset)
        return pen["out"]

    def _check_window_known(self, pen):
        """the penalties look at history[:, beg .. pos]: a window that starts below what reset() was told is refused"""
        if pen is None:
            return
        _, sustain, decay = pen["key"][:3]
        seq_len = self.pos + 1
        beg = max(seq_len - (seq_len if sustain == -1 else sustain) - decay, 0)
        if beg < getattr(self, "_known_from", 0) and seq_len - beg > 0:
            raise RuntimeError(f"sampled decoding: the penalties look back to sequence index {beg}, but the token log is known from "
                               f"{self._known_from} on only -- pass prompt_ids to reset()")

    def _overlapped(self) -> bool:
        return self.chain is not None and "flags" in self.chain and self.chain.get("stream_b") is not None

    def _ordered(self, launch):
        """One step of the overlapped chain = launches on two streams that are not joined inside the step.  At the step's
        boundaries each stream is put behind the other: stream B behind everything stream A was given before the step (the
        previous step's half included), stream A behind stream B's previous half; after the last step of run() stream A
        is put behind stream B once more.  (Events between graph launches, not inside them.)"""
        ch = self.chain
        ch["ev_pre"].record(self.stream)
        ch["stream_b"].wait_event(ch["ev_pre"])
        self.stream.wait_event(ch["ev_b"])
        launch()
        ch["ev_b"].record(ch["stream_b"])

    def step_eager(self):
        if self._overlapped():
            self._ordered(self._launch_step)
            if self._overlapped():
                self.stream.wait_event(self.chain["ev_b"])
            return
        self._launch_step()

    def _launch_step(self):
        while self.chain is not None:
            try:
                return self.step_chain()
            except RuntimeError as e:
                if "not covered" not in str(e):
                    raise
                # the optimistic grouping (all rows in one launch: the lean kernel's wave-private / ROWS / XMEM forms) is a guess
                # about what the kernel's host plan accepts -- XMEM is one register pass (K <= ~12 k at 4 bits), the wave-private
                # form stages rows x K-slice per wave: down_proj of a Mixtral / Llama-3 width (K = 14336) declines 5+ rows, of a
                # 70B (K = 28672) 3+.  Before giving up the WHOLE chain, regroup the launch kind that declined: row groups of
                # 4, then 2, then 1.  (a step that failed half-way is simply redone: it starts from the embedding and re-appends
                # the same cache row)
                if not self._overlapped() and self._regroup(str(e)):
                    continue
                if self._overlapped():
                    # the experimental overlapped mode never falls back silently: a run that asked for it and did not get it
                    # must not be mistaken for a measurement of it
                    raise RuntimeError("EXL2_CHAIN_OVERLAP=1: a launch of the step is outside the chained kernels (" + str(e) +
                                       "); unset EXL2_CHAIN_OVERLAP") from e
                self.chain = None               # a shape outside the chained kernels: the module-by-module route below
        m, ext, cfg = self.model, self.model.ext, self.model.config
        if self.fp32:
            return self._launch_step_fp32()
        if self.layernorm:
            return self._launch_step_layernorm()
        ext.embed_rows(m.embed_tokens, self.ids, self.x.view(self.b, cfg.hidden_size))
        for attn, mlp in m.layers:
            if self.loras:
                attn.forward(self.x, self.cache, 0, self.cache_seqlens, self.block_table, loras=self.loras)
                mlp.forward(self.x, loras=self.loras)
                continue
            attn.forward(self.x, self.cache, 0, self.cache_seqlens, self.block_table)
            mlp.forward(self.x)
        ext.rms_norm(self.x.view(self.b, -1), m.norm.weight, self.xn.view(self.b, -1), cfg.norm_eps)
        ext.gemm_half_q_half(self.xn.view(self.b, -1), m.lm_head.q_handle, self.logits)
        self._select_token()

    def _launch_step_layernorm(self):
        """The step of a LayerNorm model, module by module.  Sequential blocks (StarCoder2): the handles' own norms.  Parallel blocks
        (Cohere): the attention in place on one normed copy, the MLP on the other, one bridge launch per block -- the last one leaves the
        final norm in xn."""
        m, ext, cfg, b = self.model, self.model.ext, self.model.config, self.b
        x2 = self.x.view(b, cfg.hidden_size)
        xn = self.xn.view(b, cfg.hidden_size)
        ext.embed_rows(m.embed_tokens, self.ids, x2)
        if cfg.parallel_decoder_blocks:
            m._parallel_layers(self.x, b, 1, self.cache, 0, self.cache_seqlens, self.block_table, final_norm_out=xn, bridge=self.parallel_bridge)
        else:
            for attn, mlp in m.layers:
                attn.forward(self.x, self.cache, 0, self.cache_seqlens, self.block_table)
                mlp.forward(self.x)
            ext.layer_norm(x2, m.norm.weight, none_tensor if m.norm.bias is None else m.norm.bias, xn, cfg.norm_eps)
        ext.gemm_half_q_half(xn, m.lm_head.q_handle, self.logits)
        self._select_token()

    def _launch_step_fp32(self):
        """The step of a model with an fp32 residual stream (Gemma-2 / Gemma-3), module by module.  With the bridge the decoder owns the
        norms: pre-norm of layer 0, then per layer the attention's `_normed` entries, a bridge (post-attention norm into x, pre-MLP
        norm out), the MLP's `_normed` entry, a bridge (post-MLP norm into x, the next layer's pre-norm -- or the final norm -- out):
        2 norm launches per layer instead of 4.  The normed rows and the projections' outputs share the model's temp_state."""
        m, ext, cfg, b = self.model, self.model.ext, self.model.config, self.b
        x2 = self.x.view(b, cfg.hidden_size)
        ext.embed_rows_f32(m.embed_tokens, self.ids, x2, m.embed_scale())
        ts = m.temp_state[:b]
        bridged = self.norm_bridge
        if bridged:
            ext.rms_norm(x2, m.layers[0][0].pre_layernorm, ts, cfg.norm_eps)
            for i, (attn, mlp) in enumerate(m.layers):
                attn.forward_normed(ts, b, 1, self.cache, 0, self.cache_seqlens, self.block_table)
                self._bridge(ts, x2, attn.post_layernorm, mlp.post_attention_layernorm, ts)
                mlp.forward_normed(ts)
                last = i + 1 == len(m.layers)
                self._bridge(ts, x2, mlp.post_layernorm, m.norm.weight if last else m.layers[i + 1][0].pre_layernorm,
                             self.xn.view(b, -1) if last else ts)
        else:
            for attn, mlp in m.layers:
                attn.forward(self.x, self.cache, 0, self.cache_seqlens, self.block_table)
                mlp.forward(self.x)
            ext.rms_norm(x2, m.norm.weight, self.xn.view(b, -1), cfg.norm_eps)
        ext.gemm_half_q_half(self.xn.view(b, -1), m.lm_head.q_handle, self.logits)
        if cfg.final_logit_softcapping:
            ext.softcap_(self.logits, cfg.final_logit_softcapping)
        self._select_token()

    def _bridge(self, t, x, w_post, w_next, n):
        ext, eps = self.model.ext, self.model.config.norm_eps
        if not ext.norm_bridge(t, x, w_post, w_next, n, eps):
            # a hidden size the bridge does not cover: the two launches it stands for
            ext.rms_norm_add(t, w_post, x, eps)
            ext.rms_norm(x, w_next, n, eps)

    def _regroup(self, msg: str) -> bool:
        """a chained launch was declined ("<entry point>: shape not covered"): smaller row groups for launches of its K"""
        cfg = self.model.config
        if "(down)" in msg: K = cfg.intermediate_size
        elif "q_attn_forward_2" in msg: K = cfg.num_attention_heads * cfg.head_dim
        else: K = cfg.hidden_size
        ov = self.chain.setdefault("group_override", {})
        cur = ov.get(K) or self.b
        for g in (4, 2, 1):
            if g < cur:
                ov[K] = g
                return True
        return False

    def _on_stream(self):
        import contextlib
        return torch.cuda.stream(self.stream) if self.stream is not None else contextlib.nullcontext()

    def capture(self):
        """Warm-up + capture run two throw-away steps; they are pointed at the LAST cache slot, whose K/V rows are
        saved and restored, so capturing never disturbs a cache that already holds a prompt."""
        ext = self.model.ext
        torch.cuda.synchronize()
        scratch_pos = self.limit - 1
        with self._on_stream():
            saved_state = (self.cache_seqlens.clone(), self.ids.clone())
            slot_tensors = list(self.cache.key_states) + list(self.cache.value_states)
            # quantized caches: the scales of the scratch slot too (they sit at the same [batch, position] index)
            slot_tensors += list(getattr(self.cache, "key_scales", [])) + list(getattr(self.cache, "value_scales", []))
            saved_kv = [t[:, scratch_pos].clone() for t in slot_tensors]
            self.cache_seqlens.fill_(scratch_pos)
            self.step_eager()                               # warm-up: lazy one-time setup must not happen under capture
            self.cache_seqlens.fill_(scratch_pos)
            self.stream.synchronize()
            if self._overlapped():
                # two graphs, one per stream, replayed side by side (the branches of ONE forked graph are run one after the
                # other on this stack: tools/probes/fork_probe.hip)
                sb = self.chain["stream_b"]
                sb.synchronize()
                ext.graph_begin_capture(self.stream.cuda_stream)
                ext.graph_begin_capture(sb.cuda_stream)
                try:
                    self._launch_step()
                finally:
                    self.graph = ext.graph_end_capture(self.stream.cuda_stream)
                    self.graph_b = ext.graph_end_capture(sb.cuda_stream)
            else:
                ext.graph_begin_capture(self.stream.cuda_stream)
                try:
                    self._launch_step()
                finally:
                    self.graph = ext.graph_end_capture(self.stream.cuda_stream)
            self.cache_seqlens.copy_(saved_state[0]); self.ids.copy_(saved_state[1])
            for t, s in zip(slot_tensors, saved_kv):
                t[:, scratch_pos].copy_(s)
            self.stream.synchronize()
        return self

    def reset(self, first_ids: torch.Tensor, seq_len: int = 0, prompt_ids=None):
        """prompt_ids (int [b, seq_len + 1], last column = first_ids): the sequences so far, logged in history[:, :seq_len + 1] for
        the sampler's penalties; without it only history[:, seq_len] = first_ids is known."""
        seq_len = int(seq_len)
        first = first_ids.to(torch.int32).view(-1)
        if prompt_ids is not None:
            prompt = prompt_ids.to(torch.int32).view(self.b, -1)
            if prompt.shape[1] != seq_len + 1:
                raise RuntimeError(f"decode: prompt_ids holds {prompt.shape[1]} tokens per sequence, seq_len + 1 = {seq_len + 1} are expected")
            if not torch.equal(prompt[:, -1].cpu(), first.cpu()):
                raise RuntimeError("decode: the last column of prompt_ids must be first_ids")
        with self._on_stream():
            self.ids.copy_(first)
            self.cache_seqlens.fill_(seq_len)
            if prompt_ids is not None:
                self.history[:, :seq_len + 1].copy_(prompt)
            elif 0 <= seq_len < self.history.shape[1]:
                self.history[:, seq_len].copy_(first)
        self._known_from = 0 if prompt_ids is not None else seq_len
        self.pos = seq_len

    def run(self, n_tokens: int, use_graph: bool = True):
        ext = self.model.ext
        if self.pos + n_tokens > self.limit:
            raise RuntimeError(f"decode: {self.pos} cached + {n_tokens} new tokens exceed the cache / max_seq_len ({self.limit})")
        self.pos += n_tokens
        with self._on_stream():
            sptr = self.stream.cuda_stream if self.stream is not None else None
            two = use_graph and self.graph is not None and getattr(self, "graph_b", None) is not None and self._overlapped()
            for _ in range(n_tokens):
                if two:
                    bptr = self.chain["stream_b"].cuda_stream
                    self._ordered(lambda: (ext.graph_launch(self.graph, sptr), ext.graph_launch(self.graph_b, bptr)))
                elif use_graph and self.graph is not None:
                    ext.graph_launch(self.graph, sptr)
                else:
                    self.step_eager()
            if two:
                self.stream.wait_event(self.chain["ev_b"])

    def capture_sampled(self, temperature: float, top_k: int, top_p: float = 0.0, min_p: float = 0.0, n_randoms: int = 4096,
                        **settings):
        """A second step graph whose last launches are the device sampler (exl2_sample_rows_step) + its counter increment instead
        of the arg-max: `run_sampled` with these settings then replays ONE graph per token -- the random points are read from a
        device buffer the host fills before the run (n_randoms tokens ahead at most per fill).
        penalties: token_repetition_penalty / _range / _decay, token_frequency_penalty, token_presence_penalty, token_bias (fp32
        [vocab]) -- the reference Settings' names and meaning (sampler.py:54-69, 408-429).  Any of them off its neutral value puts
        exl2_apply_penalties in front of the sampler, inside the same graph.
        The rest of the reference's chain by its Settings' names -- top_a, tfs, typical, temperature_last, smoothing_factor, min_temp,
        max_temp, temp_exponent, skew, mirostat, mirostat_tau, mirostat_eta, return_top_tokens: any of them off its neutral value
        makes the sampler launch exl2_sample_rows_chain_step (all neutral: the same launches as without them).  `mirostat_mu` is reset
        here; `top_tokens` / `top_probs` hold the report of the last step."""
        ext, cfg = self.model.ext, self.model.config
        if self._overlapped():
            raise RuntimeError("capture_sampled: not available on the experimental overlapped chain")
        dev = self.logits.device
        chain_kw, penalties = self._split_settings(settings)
        sm = {"temperature": float(temperature), "top_k": int(top_k), "top_p": float(top_p), "min_p": float(min_p),
              "randoms": torch.zeros((int(n_randoms),), dtype=torch.float32, device=dev),
              "counter": torch.zeros((1,), dtype=torch.int32, device=dev),
              "probs": torch.zeros((self.b,), dtype=torch.float32, device=dev),
              "ws": torch.empty((self.b, cfg.vocab_size), dtype=torch.float32, device=dev)}
        sm["pen"] = self._penalty_state(penalties)
        sm["chain"] = self._chain_state(chain_kw, temperature)
        sm["graph"] = None
        if dev.type == "cuda":
            greedy_graph, self.graph = self.graph, None
            self._sampling = sm
            try:
                self.capture()                                   # same warm-up / scratch-slot protocol, the sampler as the last launches
                sm["graph"] = self.graph
            finally:
                self.graph = greedy_graph
                self._sampling = None
        sm["counter"].zero_()
        if getattr(self, "mirostat_mu", None) is not None:
            self.mirostat_mu.zero_()                              # (the warm-up steps of the capture have sampled: mu starts over)
        old = getattr(self, "_sampled", None)
        if old is not None and old.get("graph") is not None:
            ext.graph_free(old["graph"])                          # a re-capture with new settings replaces the old sampled graph
        self._sampled = sm
        return self

    def run_sampled(self, n_tokens: int, temperature: float, top_k: int, top_p: float = 0.0, min_p: float = 0.0,
                    randoms=None, seed: int = 0, use_graph: bool = True, **settings):
        """Decode `n_tokens` tokens per sequence with the DEVICE sampler (csrc/sampling.hip; the reference's sample_basic for
        these settings: ext_sampling.cpp:93-301) instead of the arg-max: per token the step's graph, then one
        `sample_rows` launch on the step's logits that overwrites the token fed to the next step, then the token log.
        The only thing the host supplies per token is the random point (`randoms[i]`, or `random.Random(seed)` like the
        reference's `random.random()` per sampling call, sampler.py:351) -- as a launch argument; nothing is read back, so
        the loop stays asynchronous like run().  Rows of a batch share the point through the reference's recurrence.
        penalties: as capture_sampled; applied on the device ahead of the sampler on either route.  The chain settings (top_a, tfs,
        typical, temperature_last, smoothing_factor, min_temp, max_temp, temp_exponent, skew, mirostat*, return_top_tokens): as
        capture_sampled; mu carries over from call to call in `mirostat_mu` like the reference's Settings carry it."""
        import random as _random
        chain_kw, penalties = self._split_settings(settings)
        ext, cfg = self.model.ext, self.model.config
        if self._overlapped():
            raise RuntimeError("run_sampled: not available on the experimental overlapped chain")
        if self.pos + n_tokens > self.limit:
            raise RuntimeError(f"decode: {self.pos} cached + {n_tokens} new tokens exceed the cache / max_seq_len ({self.limit})")
        if randoms is None:
            rng = _random.Random(seed)
            randoms = [rng.random() for _ in range(n_tokens)]
        if len(randoms) < n_tokens:
            raise RuntimeError("run_sampled: one random point per token is needed")
        sm = getattr(self, "_sampled", None)
        pen = self._penalty_state(penalties, old=(sm or {}).get("pen") or getattr(self, "_sample_pen", None))
        self._check_window_known(pen)
        ch = self._chain_state(chain_kw, temperature, old=(sm or {}).get("chain"))
        if (sm is not None and n_tokens <= sm["randoms"].numel() and pen is sm.get("pen")
                and (ch or {}).get("key") == (sm.get("chain") or {}).get("key")
                and (sm["temperature"], sm["top_k"], sm["top_p"], sm["min_p"]) == (float(temperature), int(top_k), float(top_p), float(min_p))):
            # settings of capture_sampled: the sampler is part of the step; the random points travel as ONE copy before the run,
            # then one graph launch per token (eager steps of the same launches where there is no graph)
            pts = torch.tensor([float(r) for r in randoms[:n_tokens]], dtype=torch.float32)
            self.pos += n_tokens
            with self._on_stream():
                sptr = self.stream.cuda_stream if self.stream is not None else None
                sm["randoms"][:n_tokens].copy_(pts, non_blocking=False)
                sm["counter"].zero_()
                if use_graph and sm.get("graph") is not None:
                    for _ in range(n_tokens):
                        ext.graph_launch(sm["graph"], sptr)
                else:
                    self._sampling = sm
                    try:
                        for _ in range(n_tokens):
                            self.step_eager()
                    finally:
                        self._sampling = None
            return
        if getattr(self, "_sample_ws", None) is None:
            dev = self.logits.device
            self._sample_ws = torch.empty((self.b, cfg.vocab_size), dtype=torch.float32, device=dev)
            self._sample_probs = torch.zeros((self.b,), dtype=torch.float32, device=dev)
        self._sample_pen = pen
        p0 = self.pos
        self.pos += n_tokens
        with self._on_stream():
            sptr = self.stream.cuda_stream if self.stream is not None else None
            for i in range(n_tokens):
                if use_graph and self.graph is not None:
                    ext.graph_launch(self.graph, sptr)
                else:
                    self.step_eager()
                # the step's own arg-max has written its token to ids / history[:, p0 + i + 1]; the sampled one replaces both
                # (the position is one ahead already: the penalties' sequence ends at the step's input token)
                logits = self.logits if pen is None else self._penalised_logits({"pen": pen}, pos_offset=-1)
                if ch is None:
                    ext.sample_rows(logits, temperature, top_k, top_p, min_p, float(randoms[i]), self.ids, self._sample_probs,
                                    workspace=self._sample_ws, vocab=cfg.vocab_size)
                else:
                    ext.sample_rows_chain(logits, ch["temperature"], top_k, top_p, min_p, float(randoms[i]), self.ids,
                                          self._sample_probs, workspace=self._sample_ws, vocab=cfg.vocab_size, **ch["kw"])
                self.history[:, p0 + i + 1].copy_(self.ids)

    def tokens(self, start: int, n: int) -> torch.Tensor:
        """tokens generated at positions start+1 .. start+n (history[b, pos] = token sampled after `pos` cached tokens)."""
        return self.history[:, start + 1:start + 1 + n]

    def free(self):
        sm = getattr(self, "_sampled", None)
        if sm is not None and sm.get("graph") is not None:
            self.model.ext.graph_free(sm["graph"])
        self._sampled = None
        if self.graph is not None:
            self.model.ext.graph_free(self.graph)
            self.graph = None
        if getattr(self, "graph_b", None) is not None:
            self.model.ext.graph_free(self.graph_b)
            self.graph_b = None
