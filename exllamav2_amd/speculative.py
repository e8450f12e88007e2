"""Speculative decoding of one sequence: K drafted tokens are verified by one forward over K + 1 rows, the longest prefix the
model's own choice confirms is kept -- and the whole verify step (embedding -> layers -> head -> arg-max or sampler -> accept -> next
drafts) stays one captured graph with no host round trip, like model.GreedyGraphDecoder's.

Procedure = the reference's ExLlamaV2DynamicGenerator(use_ngram_draft=True) (exllamav2/generator/dynamic.py:1009-1058 drafting,
:1139- verification); the drafter is a rule of our own on the device (csrc/spec_decode.hip: latest longest n-gram match, overlapping
copy).  Greedy verification makes the emitted tokens independent of the drafts.  Sampled verification (capture_sampled / run_sampled)
samples every row with a random point of its own, after the reference's penalties over the row's own sequence -- the log plus the
drafts that must have been accepted for the row to count -- and accepts a draft when the sampled token equals it; a random point is
consumed per EMITTED token, so the tokens are those of unspeculated sampled decoding with the same points."""
from __future__ import annotations

import os

import torch

from .model import ExLlamaV2, GreedyGraphDecoder


class SpeculativeGraphDecoder(GreedyGraphDecoder):
    """num_draft_tokens = K: a step feeds the rows ids[0 .. K] of ONE sequence at positions p .. p + K.  max_ngram: the drafter
    matches contexts of up to max_ngram - 1 tokens.  drafter "forced": the drafts are forced[L + i] (forced[j] = the token the
    caller expects at sequence index j) -- tests and controlled acceptance rates."""

    def __init__(self, model: ExLlamaV2, cache, num_draft_tokens: int = 3, max_ngram: int = 4, drafter: str = "ngram",
                 forced=None, loras=None):
        cfg, dev = model.config, model.device
        K = int(num_draft_tokens)
        if cache.batch_size != 1:
            raise RuntimeError(f"speculative decoding serves one sequence: the cache holds {cache.batch_size} (batch > 1 is not built)")
        if K < 1 or K + 1 > 16:
            raise RuntimeError(f"speculative decoding: {K} drafts + 1 = {K + 1} rows per step; the chained decode kernels take 2..16 rows")
        if not 2 <= int(max_ngram) <= 8:
            raise RuntimeError(f"speculative decoding: max_ngram {max_ngram} must be in 2..8 (contexts of 1..7 tokens)")
        if getattr(cache, "wbits", 0):
            raise RuntimeError("speculative decoding is not built for a quantized cache (use the FP16 cache)")
        if loras:
            raise RuntimeError("speculative decoding is not built with LoRA adapters")
        if cfg.residual_fp32:
            raise RuntimeError("speculative decoding is not built for a model with an fp32 residual stream")
        if cfg.layernorm:
            raise RuntimeError("speculative decoding is not built for a LayerNorm model (StarCoder2, Cohere)")
        if getattr(cfg, "num_experts", 0):
            raise RuntimeError("speculative decoding is not built for a sparse-MoE model")
        if os.environ.get("EXL2_CHAIN_OVERLAP", "0") != "0":
            raise RuntimeError("speculative decoding is not built for the experimental overlapped chain: unset EXL2_CHAIN_OVERLAP")
        if drafter not in ("ngram", "forced") or (drafter == "forced") != (forced is not None):
            raise RuntimeError("speculative decoding: drafter is \"ngram\", or \"forced\" together with the forced tokens")
        # the chain set-up, the partial-sum bookkeeping and the regroup ladder of a decoder of K + 1 rows ...
        super().__init__(model, cache, batch_size=K + 1)
        self.K, self.s, self.N, self.q_len = K, K + 1, int(max_ngram) - 1, K + 1
        # ... which are the rows of one sequence: one table row, one length, one token log
        pages = self.block_table.shape[1]
        self.block_table = torch.arange(pages, dtype=torch.int32, device=dev).view(1, pages).contiguous()
        self.cache_seqlens = torch.zeros((1,), dtype=torch.int32, device=dev)
        self.x, self.xn = self.x.view(1, self.s, cfg.hidden_size), self.xn.view(1, self.s, cfg.hidden_size)
        full = self.limit
        # a step at position p writes the K/V rows p .. p + K and logs up to history[p + 1 + K]
        self.limit = full - K
        self.history = torch.zeros((full + K + 2,), dtype=torch.int32, device=dev)
        self.cand = torch.zeros((self.s,), dtype=torch.int32, device=dev)
        self.stats_buf = torch.zeros((K + 3,), dtype=torch.int32, device=dev)
        self.forced = None
        if forced is not None:
            self.forced = torch.zeros((int(forced.numel()),), dtype=torch.int32, device=dev)
            self.set_forced(forced)
        if self.chain is not None:
            # the rows sit at positions p .. p + K: the attention launch takes their rotary rows from the tables
            self.chain.pop("rope_now", None)

    def set_forced(self, forced: torch.Tensor):
        """replace the forced tokens in place (a captured graph keeps the buffer and its length)"""
        if self.forced is None or forced.numel() != self.forced.numel():
            raise RuntimeError("set_forced: the forced tokens keep the length the decoder was made with")
        f = forced.reshape(-1).to(torch.int64)
        if f.numel() and (int(f.min()) < 0 or int(f.max()) >= self.model.config.vocab_size):
            raise RuntimeError("set_forced: token outside the vocabulary")
        with self._on_stream():
            self.forced.copy_(f.to(torch.int32))

    # Rejected rows: a step at cache length p writes the K/V rows p .. p + K of every layer and keeps p' = p + n_acc + 1 of them; the
    # rows p' .. p + K stay in the cache, stale.  Nothing reads them: row i of the next step attends keys 0 .. p' + i only, and that
    # step first rewrites p' .. p' + K, which covers p' .. p + K because p' + K >= p + K.  So no row is ever rolled back.
    def _select_token(self):
        ext, cfg = self.model.ext, self.model.config
        sm = getattr(self, "_sampling", None)
        if sm is None:
            ext.argmax_rows(self.logits, self.cand, cfg.vocab_size)
            ext.spec_accept_draft(self.cand, self.ids, self.history, self.cache_seqlens, self.stats_buf, self.K, self.N, forced=self.forced)
            return
        # sampled verification: penalties over each row's own sequence, one random point per row, the counter moves with the tokens kept
        logits = self._penalised_logits(sm)
        ext.sample_rows_step(logits, sm["temperature"], sm["top_k"], sm["top_p"], sm["min_p"], sm["randoms"], sm["counter"],
                             self.cand, sm["probs"], sm["ws"], None, None, pos_inc=0, vocab=cfg.vocab_size, per_row_random=True)
        ext.spec_accept_draft(self.cand, self.ids, self.history, self.cache_seqlens, self.stats_buf, self.K, self.N, forced=self.forced,
                              rand_counter=sm["counter"])

    def _penalised_logits(self, sm, pos_offset: int = 0):
        pen = sm.get("pen")
        if pen is None:
            return self.logits
        k = pen["key"]
        self.model.ext.apply_penalties(self.logits, pen["out"], self.history, self.cache_seqlens, k[0], k[1], k[2], k[3], k[4],
                                       ramps=pen["ramps"], token_bias=pen["bias"], vocab=self.model.config.vocab_size,
                                       rows_share_sequence=True, tail=self.ids[1:], pos_offset=pos_offset)
        return pen["out"]

    def capture(self):
        """Warm-up + capture run two throw-away steps pointed at the LAST K + 1 cache slots; their K/V rows on all layers, ids,
        pos, stats and the token-log entries the steps touch are saved and restored: capturing never disturbs a prefilled prompt."""
        ext = self.model.ext
        torch.cuda.synchronize()
        s = self.s
        p = self.limit - 1                                   # rows p .. p + K = the last s slots
        with self._on_stream():
            saved = [t.clone() for t in (self.cache_seqlens, self.ids, self.stats_buf, self.cand)]
            saved_hist = self.history[p:p + s + 1].clone()
            slot_tensors = list(self.cache.key_states) + list(self.cache.value_states)
            saved_kv = [t[:, p:p + s].clone() for t in slot_tensors]
            self.cache_seqlens.fill_(p)
            self.step_eager()                                # warm-up: lazy one-time setup must not happen under capture
            self.cache_seqlens.fill_(p)
            self.stream.synchronize()
            ext.graph_begin_capture(self.stream.cuda_stream)
            try:
                self._launch_step()
            finally:
                self.graph = ext.graph_end_capture(self.stream.cuda_stream)
            for t, c in zip((self.cache_seqlens, self.ids, self.stats_buf, self.cand), saved):
                t.copy_(c)
            self.history[p:p + s + 1].copy_(saved_hist)
            for t, c in zip(slot_tensors, saved_kv):
                t[:, p:p + s].copy_(c)
            self.stream.synchronize()
        return self

    def reset(self, prompt_ids: torch.Tensor):
        """prompt_ids: the L tokens of the sequence so far; the first L - 1 are in the cache already
        (model.forward(prompt[:, :-1], cache, preprocess_only=True)), the last one is the first step's input."""
        ids = prompt_ids.reshape(-1).to(torch.int64)
        L = int(ids.numel())
        if L < 1 or L - 1 > self.limit:
            raise RuntimeError(f"decode: a prompt of {L} tokens does not fit the cache / max_seq_len ({self.limit} + {self.K} draft rows)")
        if int(ids.min()) < 0 or int(ids.max()) >= self.model.config.vocab_size:
            raise RuntimeError("decode: prompt token outside the vocabulary")
        with self._on_stream():
            self.history[:L].copy_(ids.to(torch.int32))
            self.ids[:1].copy_(ids[-1:].to(torch.int32))
            self.cache_seqlens.fill_(L - 1)
            self.stats_buf.zero_()
            self.model.ext.spec_accept_draft(None, self.ids, self.history, self.cache_seqlens, None, self.K, self.N,
                                             forced=self.forced, draft_only=True)
        self.pos = L - 1

    def run(self, n_steps: int, use_graph: bool = True):
        """n_steps verify steps, asynchronously.  A step advances the position by 1 .. K + 1, which the host does not see: the
        bound is checked for the most (sync() brings the host's figure back to the true one)."""
        ext = self.model.ext
        if self.pos + n_steps * self.s > self.limit:
            raise RuntimeError(f"decode: {self.pos} cached + {n_steps} steps of up to {self.s} new tokens exceed the cache / "
                               f"max_seq_len ({self.limit} + {self.K} draft rows)")
        self.pos += n_steps * self.s
        with self._on_stream():
            sptr = self.stream.cuda_stream if self.stream is not None else None
            for _ in range(n_steps):
                if use_graph and self.graph is not None:
                    ext.graph_launch(self.graph, sptr)
                else:
                    self.step_eager()

    def sync(self) -> int:
        """waits for the steps given so far; returns the true cache length and takes it as the host's bound"""
        if self.stream is not None:
            self.stream.synchronize()
        self.pos = int(self.cache_seqlens.item())
        return self.pos

    def generate(self, max_new_tokens: int, steps_per_sync: int = 8) -> torch.Tensor:
        """int32 [max_new_tokens]: the tokens emitted behind the current position (the steps may have emitted a few more: tokens())"""
        start = self.sync()
        target = start + int(max_new_tokens)
        while True:
            p = self.sync()
            if p >= target:
                break
            n = min(int(steps_per_sync), target - p, (self.limit - p) // self.s)       # a step emits one token at least
            if n < 1:
                raise RuntimeError(f"decode: {p} cached + {target - p} new tokens exceed the cache / max_seq_len ({self.limit} + {self.K} draft rows)")
            self.run(n, use_graph=self.graph is not None)
        return self.tokens(start, int(max_new_tokens))

    def tokens(self, start: int, n: int) -> torch.Tensor:
        """tokens emitted at sequence indices start + 1 .. start + n (history[j] = the token at index j, prompt included)"""
        return self.history[start + 1:start + 1 + n]

    def stats(self) -> dict:
        self.sync()
        st = self.stats_buf.cpu().tolist()
        steps, accepted = st[0], st[1]
        return {"steps": steps, "accepted": accepted, "hist": st[2:2 + self.s], "emitted": steps + accepted,
                "tokens_per_step": (steps + accepted) / steps if steps else 0.0}

    # capture_sampled: GreedyGraphDecoder's -- capture() above with the sampled tail as the step's last launches.  The verify step's
    # sampler is exl2_sample_rows_step2 without the chain stages: this decoder knows none of the chain keywords, so top_a, tfs,
    # typical, mirostat*, temperature_last, smoothing_factor, min_temp / max_temp / temp_exponent, skew and return_top_tokens are
    # unknown settings here (TypeError), never silently dropped.
    CHAIN_DEFAULTS = {}

    def _chain_state(self, kw: dict, temperature: float, old=None):
        return None

    def run_sampled(self, n_steps: int, temperature: float, top_k: int, top_p: float = 0.0, min_p: float = 0.0,
                    randoms=None, seed: int = 0, use_graph: bool = True, **penalties):
        """n_steps sampled verify steps with the settings of capture_sampled, asynchronously like run().  The random points
        (`randoms`, or random.Random(seed)) are copied to the device once, for the most the run can consume -- n_steps x (K + 1),
        which the buffer of capture_sampled must hold; the counter restarts at 0 and ends at the number of tokens emitted."""
        import random as _random
        ext = self.model.ext
        sm = getattr(self, "_sampled", None)
        if sm is None:
            raise RuntimeError("run_sampled: sampling with speculation runs the step capture_sampled made -- call capture_sampled first")
        pen = self._penalty_state(penalties, old=sm.get("pen"))
        if pen is not sm.get("pen") or (sm["temperature"], sm["top_k"], sm["top_p"], sm["min_p"]) != (
                float(temperature), int(top_k), float(top_p), float(min_p)):
            raise RuntimeError("run_sampled: the settings differ from those of capture_sampled")
        need = int(n_steps) * self.s
        if need > sm["randoms"].numel():
            raise RuntimeError(f"run_sampled: {n_steps} steps may consume {need} random points, the buffer holds {sm['randoms'].numel()} "
                               f"(capture_sampled n_randoms)")
        if self.pos + need > self.limit:
            raise RuntimeError(f"decode: {self.pos} cached + {n_steps} steps of up to {self.s} new tokens exceed the cache / "
                               f"max_seq_len ({self.limit} + {self.K} draft rows)")
        if randoms is None:
            rng = _random.Random(seed)
            randoms = [rng.random() for _ in range(need)]
        if len(randoms) < need:
            raise RuntimeError(f"run_sampled: {need} random points are needed (one per row of every step)")
        pts = torch.tensor([float(r) for r in randoms[:need]], dtype=torch.float32)
        self.pos += need
        with self._on_stream():
            sptr = self.stream.cuda_stream if self.stream is not None else None
            sm["randoms"][:need].copy_(pts, non_blocking=False)
            sm["counter"].zero_()
            if use_graph and sm.get("graph") is not None:
                for _ in range(n_steps):
                    ext.graph_launch(sm["graph"], sptr)
            else:
                self._sampling = sm
                try:
                    for _ in range(n_steps):
                        self.step_eager()
                finally:
                    self._sampling = None
