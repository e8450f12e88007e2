"""Model hyper-parameters the hot path needs (subset of the reference's ExLlamaV2Config, config.py:58-196)."""
from __future__ import annotations

from dataclasses import dataclass, field


@dataclass
class ExLlamaV2Config:
    hidden_size: int = 4096
    intermediate_size: int = 11008
    num_hidden_layers: int = 32
    num_attention_heads: int = 32
    num_key_value_heads: int = 32
    head_dim: int = 128
    vocab_size: int = 32000
    max_seq_len: int = 4096
    norm_eps: float = 1e-5
    rotary_embedding_base: float = 10000.0
    rope_style: int = 2                     # RopeStyle.NEOX (architecture.py:109-112)
    max_batch_size: int = 1
    max_input_len: int = 2048               # chunk size of forward (config.py:196, model.py:833)
    arch: str = "llama"
    num_experts: int = 0                    # > 0: sparse-MoE MLP (moe_mlp.py; Mixtral: 8, Qwen3-MoE: 128), experts per token below
    num_experts_per_token: int = 2
    use_qk_norm: bool = False               # per-head norm of q / k between the projections and RoPE (architecture.py:446,459,609)
    headnorm_rms: bool = True               # its form: RMS (Qwen3, Gemma3, OLMo2) or LayerNorm over the head (Cohere)
    # Gemma-2 / Gemma-3 blocks (architecture.py:554-613).  The defaults are every other family's.
    residual_fp32: bool = False             # fp32 residual stream (residual_stream_fp32); such architectures have post norms (:955-957)
    post_norms: bool = False                # .post_attention_layernorm / .post_feedforward_layernorm behind o_proj / down_proj,
                                            # .pre_feedforward_layernorm ahead of the MLP (the "norm_1_post" / "norm_2" / "norm_2_post" keys)
    norm_constant_bias: float = 0.0         # added to every RMSNorm weight in fp16 at load (rmsnorm.py:57-59)
    normalize_embeddings: bool = False      # embedding rows times hidden_size ** 0.5, in fp32 (embedding.py:184-187)
    mlp_act_func: str = "silu"              # "silu" | "gelu"
    attn_logit_softcapping: float = 0.0     # cap * tanh(score / cap) on the scaled scores (attn.py:596-600); 0 = off
    final_logit_softcapping: float = 0.0    # the same on the logits (model.py:1043-1044)
    query_pre_attn_scalar: float = 0.0      # softmax scale = query_pre_attn_scalar ** -0.5 when set (attn.py:218-219)
    sliding_window: int = 0                 # keys a windowed layer sees to the left (flash-attn's window_size[0], attn.py:595)
    sliding_window_pattern: int = 1         # > 1: every pattern-th layer is global (Gemma-3: 6)
    alternating_swa: bool = False           # windowed and global layers alternate (model.py:111-121)
    rotary_embedding_base_alt: float = 0.0  # rope base of the windowed layers when they have their own (Gemma-3: 10000)
    # LayerNorm models (StarCoder2: architecture.py:656-676; Cohere: :704-721).  The defaults are every other family's.
    norm: str = "rmsnorm"                   # "rmsnorm" | "layernorm" (mean removed, optional bias: layer_norm.cu)
    norm_bias: bool = False                 # the LayerNorms carry a bias (StarCoder2)
    parallel_decoder_blocks: bool = False   # one .input_layernorm feeds attention and MLP, x += attn; x += mlp (parallel_decoder.py)
    mlp_gate: bool = True                   # False: ungated MLP, act(up) -> down (StarCoder2: c_fc / c_proj)
    attention_bias_qkv: bool = False        # biased q / k / v projections
    attention_bias_o: bool = False          # biased o_proj
    mlp_bias: bool = False                  # biased MLP projections
    logit_scale: float = 1.0                # folded into the head's scales at load (ext.py:336, :363)

    def __post_init__(self):
        if self.mlp_act_func not in ("silu", "gelu"):
            raise ValueError(f"mlp_act_func {self.mlp_act_func!r}: 'silu' or 'gelu'")
        if self.residual_fp32 and not self.post_norms:
            raise ValueError("residual_fp32 needs post_norms (the reference's check, architecture.py:955-957)")
        if self.normalize_embeddings and not self.residual_fp32:
            raise ValueError("normalize_embeddings without residual_fp32 (Gemma-1) is not built")
        if self.post_norms and not self.residual_fp32:
            raise ValueError("post_norms without residual_fp32 is not built in the native model")
        if self.residual_fp32 and self.num_experts:
            raise ValueError("a sparse-MoE MLP with an fp32 residual stream is not built")
        if self.norm not in ("rmsnorm", "layernorm"):
            raise ValueError(f"norm {self.norm!r}: 'rmsnorm' or 'layernorm'")
        if self.norm == "layernorm" and (self.residual_fp32 or self.post_norms):
            raise ValueError("residual_fp32 / post_norms together with LayerNorm are not built")
        if self.norm == "layernorm" and self.num_experts:
            raise ValueError("a sparse-MoE MLP with LayerNorm (DBRX) is not built")
        if self.norm == "layernorm" and self.norm_constant_bias:
            raise ValueError("norm_constant_bias belongs to RMSNorm architectures")
        if self.norm != "layernorm" and (self.norm_bias or self.parallel_decoder_blocks):
            raise ValueError("norm_bias / parallel_decoder_blocks are built for LayerNorm models only")
        if self.num_experts and not self.mlp_gate:
            raise ValueError("an ungated sparse-MoE MLP is not built")

    @property
    def layernorm(self) -> bool:
        return self.norm == "layernorm"

    def layer_window(self, layer_idx: int) -> int:
        """Keys to the left a layer attends to, 0 = all (model.py:111-121): with alternating_swa, pattern > 1 windows the layers with
        (idx + 1) % pattern != 0, pattern <= 1 the even ones."""
        if not self.alternating_swa or self.sliding_window <= 0:
            return 0
        if self.sliding_window_pattern > 1:
            return self.sliding_window if (layer_idx + 1) % self.sliding_window_pattern != 0 else 0
        return self.sliding_window if layer_idx % 2 == 0 else 0

    def layer_rope_alt(self, layer_idx: int) -> bool:
        """the layer rotates with the second sin / cos table (rotary_embedding_base_alt): windowed layers of a pattern > 1 model"""
        return bool(self.rotary_embedding_base_alt) and self.sliding_window_pattern > 1 and self.layer_window(layer_idx) > 0

    def softmax_scale(self) -> float:
        return float(self.query_pre_attn_scalar) ** -0.5 if self.query_pre_attn_scalar else float(self.head_dim) ** -0.5

    @staticmethod
    def llama2_7b(**kw):
        return ExLlamaV2Config(**kw)

    @staticmethod
    def tinyllama_1b(**kw):
        return ExLlamaV2Config(hidden_size=2048, intermediate_size=5632, num_hidden_layers=22, num_attention_heads=32,
                               num_key_value_heads=4, head_dim=64, vocab_size=32000, max_seq_len=2048, **kw)

    @staticmethod
    def llama2_70b(**kw):
        return ExLlamaV2Config(hidden_size=8192, intermediate_size=28672, num_hidden_layers=80, num_attention_heads=64,
                               num_key_value_heads=8, head_dim=128, **kw)

    @staticmethod
    def mixtral_8x7b(**kw):
        return ExLlamaV2Config(hidden_size=4096, intermediate_size=14336, num_hidden_layers=32, num_attention_heads=32,
                               num_key_value_heads=8, head_dim=128, vocab_size=32000, num_experts=8,
                               num_experts_per_token=2, arch="mixtral", **kw)

    @staticmethod
    def qwen3_8b(**kw):
        d = dict(hidden_size=4096, intermediate_size=12288, num_hidden_layers=36, num_attention_heads=32,
                 num_key_value_heads=8, head_dim=128, vocab_size=151936, norm_eps=1e-6, rotary_embedding_base=1e6,
                 use_qk_norm=True, arch="qwen3")
        d.update(kw)
        return ExLlamaV2Config(**d)

    @staticmethod
    def qwen3_0_6b(**kw):
        d = dict(hidden_size=1024, intermediate_size=3072, num_hidden_layers=28, num_attention_heads=16,
                 num_key_value_heads=8, head_dim=128, vocab_size=151936, norm_eps=1e-6, rotary_embedding_base=1e6,
                 use_qk_norm=True, arch="qwen3")
        d.update(kw)
        return ExLlamaV2Config(**d)

    # Qwen3-MoE (Qwen3MoeForCausalLM; architecture.py:450-466): Qwen3 attention with q / k head norm, every MLP a sparse-MoE block of 128
    # experts, 8 per token; intermediate_size is the EXPERTS' width, as the reference reads moe_intermediate_size into it (config.py:326).
    # The hyper-parameters are written from memory of the published configs and could not be checked against them where this was
    # written -- check them against the checkpoint's config.json before relying on them (nothing in the test-suite depends on them
    # beyond the widths of tests/test_moe_wide_widths.py).
    @staticmethod
    def _qwen3_moe(**d):
        base = dict(num_key_value_heads=4, head_dim=128, vocab_size=151936, norm_eps=1e-6, rotary_embedding_base=1e6, use_qk_norm=True,
                    num_experts=128, num_experts_per_token=8, arch="qwen3_moe")
        base.update(d)
        return ExLlamaV2Config(**base)

    @staticmethod
    def qwen3_30b_a3b(**kw):
        return ExLlamaV2Config._qwen3_moe(**(dict(hidden_size=2048, intermediate_size=768, num_hidden_layers=48, num_attention_heads=32) | kw))

    @staticmethod
    def qwen3_235b_a22b(**kw):
        return ExLlamaV2Config._qwen3_moe(**(dict(hidden_size=4096, intermediate_size=1536, num_hidden_layers=94, num_attention_heads=64) | kw))

    @staticmethod
    def _gemma2(**d):
        base = dict(vocab_size=256000, max_seq_len=8192, norm_eps=1e-6, rotary_embedding_base=10000.0, arch="gemma2",
                    residual_fp32=True, post_norms=True, norm_constant_bias=1.0, normalize_embeddings=True, mlp_act_func="gelu",
                    attn_logit_softcapping=50.0, final_logit_softcapping=30.0, sliding_window=4096, alternating_swa=True)
        base.update(d)
        return ExLlamaV2Config(**base)

    @staticmethod
    def gemma2_2b(**kw):
        return ExLlamaV2Config._gemma2(**(dict(hidden_size=2304, intermediate_size=9216, num_hidden_layers=26, num_attention_heads=8,
                                               num_key_value_heads=4, head_dim=256, query_pre_attn_scalar=256.0) | kw))

    @staticmethod
    def gemma2_9b(**kw):
        return ExLlamaV2Config._gemma2(**(dict(hidden_size=3584, intermediate_size=14336, num_hidden_layers=42, num_attention_heads=16,
                                               num_key_value_heads=8, head_dim=256, query_pre_attn_scalar=256.0) | kw))

    @staticmethod
    def gemma2_27b(**kw):
        return ExLlamaV2Config._gemma2(**(dict(hidden_size=4608, intermediate_size=36864, num_hidden_layers=46, num_attention_heads=32,
                                               num_key_value_heads=16, head_dim=128, query_pre_attn_scalar=144.0) | kw))

    @staticmethod
    def gemma3_4b(**kw):
        """the text model of Gemma-3 4B: q / k head norm, five windowed layers (their own rope base) per global one, no soft caps"""
        return ExLlamaV2Config._gemma2(**(dict(hidden_size=2560, intermediate_size=10240, num_hidden_layers=34, num_attention_heads=8,
                                               num_key_value_heads=4, head_dim=256, vocab_size=262208, query_pre_attn_scalar=256.0,
                                               rotary_embedding_base=1e6, rotary_embedding_base_alt=10000.0, sliding_window=1024,
                                               sliding_window_pattern=6, use_qk_norm=True, attn_logit_softcapping=0.0,
                                               final_logit_softcapping=0.0, arch="gemma3") | kw))

    # StarCoder2 and Cohere: the hyper-parameters below are written from memory of the published configs and could not be checked
    # against them where this was written -- check them against the checkpoint's config.json before relying on them (nothing in the
    # test-suite depends on them).
    @staticmethod
    def _starcoder2(**d):
        """LayerNorm with bias, biased projections, ungated GELU MLP, NeoX rotary.  sliding_window is recorded as the checkpoints state
        it; like the reference (model.py:111-121: no `swa` architecture flag for StarCoder2) no layer applies it."""
        base = dict(vocab_size=49152, head_dim=128, max_seq_len=16384, norm_eps=1e-5, rotary_embedding_base=1e5, arch="starcoder2",
                    norm="layernorm", norm_bias=True, mlp_gate=False, mlp_act_func="gelu", attention_bias_qkv=True,
                    attention_bias_o=True, mlp_bias=True, sliding_window=4096)
        base.update(d)
        return ExLlamaV2Config(**base)

    @staticmethod
    def starcoder2_3b(**kw):
        return ExLlamaV2Config._starcoder2(**(dict(hidden_size=3072, intermediate_size=12288, num_hidden_layers=30, num_attention_heads=24,
                                                   num_key_value_heads=2) | kw))

    @staticmethod
    def starcoder2_7b(**kw):
        return ExLlamaV2Config._starcoder2(**(dict(hidden_size=4608, intermediate_size=18432, num_hidden_layers=32, num_attention_heads=36,
                                                   num_key_value_heads=4) | kw))

    @staticmethod
    def starcoder2_15b(**kw):
        return ExLlamaV2Config._starcoder2(**(dict(hidden_size=6144, intermediate_size=24576, num_hidden_layers=40, num_attention_heads=48,
                                                   num_key_value_heads=4) | kw))

    @staticmethod
    def _cohere(**d):
        """bias-free LayerNorm, one norm per block feeding attention and MLP in parallel, GPT-J rotary, logit_scale"""
        base = dict(vocab_size=256000, head_dim=128, max_seq_len=8192, norm_eps=1e-5, rotary_embedding_base=8e6, rope_style=1,
                    arch="cohere", norm="layernorm", parallel_decoder_blocks=True, logit_scale=0.0625)
        base.update(d)
        return ExLlamaV2Config(**base)

    @staticmethod
    def command_r_35b(**kw):
        return ExLlamaV2Config._cohere(**(dict(hidden_size=8192, intermediate_size=22528, num_hidden_layers=40, num_attention_heads=64,
                                               num_key_value_heads=64) | kw))

    @staticmethod
    def aya_23_8b(**kw):
        return ExLlamaV2Config._cohere(**(dict(hidden_size=4096, intermediate_size=14336, num_hidden_layers=32, num_attention_heads=32,
                                               num_key_value_heads=8) | kw))

    @staticmethod
    def tiny_test(**kw):
        d = dict(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4,
                 num_key_value_heads=2, head_dim=64, vocab_size=320, max_seq_len=512, max_input_len=64)
        d.update(kw)
        return ExLlamaV2Config(**d)
