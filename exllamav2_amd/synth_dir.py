"""A synthetic EXL2 checkpoint as a MODEL DIRECTORY (config.json + model.safetensors) in the reference's on-disk format,
so that the reference's own loader (config.py:214-, stloader.py, module.py:116-121) can read what `synth.py` draws.

Tensor names and dtypes follow SURVEY.md A.1: `<key>.q_weight` int32, `.q_invperm` int32, `.q_scale` int32,
`.q_scale_max` fp16, `.q_groups` int16; norms / embedding `<key>.weight` fp16.  (`q_perm` is derived at load time,
module.py:120; `q_group_map` by make_group_map, ext.py:340-345.)
"""
from __future__ import annotations

import json
import os

import torch


def write_model_dir(path: str, cfg, ck: dict) -> str:
    from safetensors.torch import save_file
    os.makedirs(path, exist_ok=True)
    tensors = {}
    for key, v in ck.items():
        if isinstance(v, dict):
            for name in ("q_weight", "q_invperm", "q_scale", "q_scale_max", "q_groups", "bias"):
                if name in v:
                    tensors[f"{key}.{name}"] = v[name].detach().cpu().contiguous()
        elif key.endswith(".bias"):
            tensors[key] = v.detach().cpu().contiguous()                  # a LayerNorm's bias sits next to its weight
        else:
            tensors[f"{key}.weight"] = v.detach().cpu().contiguous()
    save_file(tensors, os.path.join(path, "model.safetensors"))
    config = {
        "architectures": ["LlamaForCausalLM"], "model_type": "llama",
        "hidden_size": cfg.hidden_size, "intermediate_size": cfg.intermediate_size,
        "num_hidden_layers": cfg.num_hidden_layers, "num_attention_heads": cfg.num_attention_heads,
        "num_key_value_heads": cfg.num_key_value_heads, "head_dim": cfg.head_dim, "vocab_size": cfg.vocab_size,
        "max_position_embeddings": cfg.max_seq_len, "rms_norm_eps": cfg.norm_eps, "rope_theta": cfg.rotary_embedding_base,
        "hidden_act": "silu", "bos_token_id": 1, "eos_token_id": 2, "pad_token_id": 0, "tie_word_embeddings": False,
        "torch_dtype": "float16",
    }
    if getattr(cfg, "num_experts", 0) and getattr(cfg, "use_qk_norm", False):
        # Qwen3-MoE (architecture.py:450-466): .mlp.experts.{e}.gate_proj | up_proj | down_proj (the internal w1 | w3 | w2), the router
        # .mlp.gate, the head norms .self_attn.q_norm / .k_norm; config.py:322-326 reads num_experts / num_experts_per_tok /
        # moe_intermediate_size
        # (the directory does not say which form the head norm has: the reference decides by architecture -- `headnorm = "layernorm"`
        # unless the architecture sets it, architecture.py:219, and Qwen3 / Qwen3-MoE do not)
        if getattr(cfg, "residual_fp32", False) or getattr(cfg, "norm", "rmsnorm") == "layernorm":
            raise NotImplementedError("write_model_dir: a sparse-MoE config with head norm is written in the Qwen3-MoE form only")
        config.update({"architectures": ["Qwen3MoeForCausalLM"], "model_type": "qwen3_moe", "num_experts": cfg.num_experts,
                       "num_experts_per_tok": cfg.num_experts_per_token, "moe_intermediate_size": cfg.intermediate_size,
                       "norm_topk_prob": True})
        for key in list(tensors):
            new = key.replace(".block_sparse_moe.gate.", ".mlp.gate.")
            if ".block_sparse_moe.experts." in new:
                new = new.replace(".block_sparse_moe.experts.", ".mlp.experts.")
                for ours, theirs in ((".w1.", ".gate_proj."), (".w3.", ".up_proj."), (".w2.", ".down_proj.")):
                    new = new.replace(ours, theirs)
            if new != key:
                tensors[new] = tensors.pop(key)
        save_file(tensors, os.path.join(path, "model.safetensors"))
    elif getattr(cfg, "num_experts", 0):
        # a sparse-MoE checkpoint in the reference's Mixtral form (architecture.py:291-305: block_sparse_moe.gate / experts.*.w1|w2|w3,
        # config.py:322-323: num_local_experts / num_experts_per_tok)
        config.update({"architectures": ["MixtralForCausalLM"], "model_type": "mixtral",
                       "num_local_experts": cfg.num_experts, "num_experts_per_tok": cfg.num_experts_per_token})
    if getattr(cfg, "residual_fp32", False):
        # Gemma-2 (architecture.py:554-576): fp32 residual stream, the four norms per layer, GELU, both soft caps.  The norm tensors
        # of `ck` are already stored without the constant bias the reference's loader adds (synth.py; rmsnorm.py:57-59), and the
        # quantized lm_head is found under its own key before the tied-embedding alternative (module.py:107-112)
        if getattr(cfg, "use_qk_norm", False) or getattr(cfg, "sliding_window_pattern", 1) > 1:
            raise NotImplementedError("write_model_dir: only the Gemma-2 form of an fp32-residual config is written")
        config.update({"architectures": ["Gemma2ForCausalLM"], "model_type": "gemma2", "hidden_act": "gelu_pytorch_tanh",
                       "hidden_activation": "gelu_pytorch_tanh", "head_dim": cfg.head_dim,
                       "attn_logit_softcapping": cfg.attn_logit_softcapping or None,
                       "final_logit_softcapping": cfg.final_logit_softcapping or None,
                       "query_pre_attn_scalar": cfg.query_pre_attn_scalar or cfg.head_dim,
                       "sliding_window": cfg.sliding_window})
    if getattr(cfg, "norm", "rmsnorm") == "layernorm":
        # the reference's tensor names (architecture.py:656-676, :704-721): StarCoder2's MLP is .mlp.c_fc / .mlp.c_proj, Cohere has a single
        # .input_layernorm per block; the quantized lm_head is found under its own key before the tied-embedding alternative
        del config["rms_norm_eps"]
        if cfg.parallel_decoder_blocks:
            if cfg.norm_bias or not cfg.mlp_gate or cfg.rope_style != 1:
                raise NotImplementedError("write_model_dir: a parallel LayerNorm config is written in the Cohere form only")
            config.update({"architectures": ["CohereForCausalLM"], "model_type": "cohere", "layer_norm_eps": cfg.norm_eps,
                           "logit_scale": cfg.logit_scale, "use_qk_norm": bool(cfg.use_qk_norm)})
        else:
            if cfg.mlp_gate or not (cfg.norm_bias and cfg.attention_bias_qkv and cfg.attention_bias_o and cfg.mlp_bias) or cfg.rope_style != 2:
                raise NotImplementedError("write_model_dir: a sequential LayerNorm config is written in the StarCoder2 form only")
            config.update({"architectures": ["Starcoder2ForCausalLM"], "model_type": "starcoder2", "layer_norm_epsilon": cfg.norm_eps,
                           "hidden_act": "gelu_pytorch_tanh", "use_bias": True})
            for key in list(tensors):
                for ours, theirs in ((".mlp.up_proj.", ".mlp.c_fc."), (".mlp.down_proj.", ".mlp.c_proj.")):
                    if ours in key:
                        tensors[key.replace(ours, theirs)] = tensors.pop(key)
            save_file(tensors, os.path.join(path, "model.safetensors"))
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(config, f)
    return path


def write_tokenizer(path: str, vocab_size: int) -> None:
    """A tiny HF tokenizer.json (byte-level BPE without merges: ids 0 / 1 / 2 = <pad> / <s> / </s>, 3..258 = the 256 byte
    symbols, the rest filler tokens) so that the reference's ExLlamaV2Tokenizer (tokenizer/tokenizer.py:122-) and with it
    ExLlamaV2DynamicGenerator can be constructed on a synthetic model directory.  Needs the `tokenizers` package (host
    side, load time only)."""
    from tokenizers import Tokenizer, models, pre_tokenizers, decoders
    assert vocab_size >= 259
    vocab = {"<pad>": 0, "<s>": 1, "</s>": 2}
    for ch in pre_tokenizers.ByteLevel.alphabet():
        pass
    alphabet = sorted(pre_tokenizers.ByteLevel.alphabet())
    for i, ch in enumerate(alphabet):
        vocab[ch] = 3 + i
    for i in range(3 + len(alphabet), vocab_size):
        vocab[f"<filler{i}>"] = i
    tok = Tokenizer(models.BPE(vocab=vocab, merges=[], unk_token=None))
    tok.pre_tokenizer = pre_tokenizers.ByteLevel(add_prefix_space=False)
    tok.decoder = decoders.ByteLevel()
    tok.save(os.path.join(path, "tokenizer.json"))
    with open(os.path.join(path, "tokenizer_config.json"), "w") as f:
        json.dump({"bos_token": "<s>", "eos_token": "</s>", "pad_token": "<pad>"}, f)
