"""ExLlamaV2Lora (reference lora.py:18-214): loads a PEFT LoRA adapter and attaches it to a loaded model's linear layers.

The rules of the reference's loader, restated:
  * adapter_config.json gives `r` and `lora_alpha`; the adapter's scale is lora_scaling * alpha / r, with alpha multiplied by sqrt(r)
    when `use_rslora` is set.  The scale is folded into B once, here, so the forward path never sees it.
  * `fan_in_fan_out` adapters are refused.
  * tensors come from `.safetensors` (safetensors.torch) or a torch pickle (`.bin`, torch.load); `*.original_module.weight` and
    `*.modules_to_save.weight` copies are skipped.
  * a tensor's target is the part of its name from `model.layers.` on: `model.layers.<i>.<part>.<projection>.lora_A|lora_B.weight`,
    whatever prefix PEFT put in front.  lora_A is [r, in_features], lora_B [out_features, r]: both are checked against the target
    linear, transposed (so the forward multiplies rows from the left) and converted to fp16.
  * a bias entry is ignored when it is all zeros (`bias_ignored` is then set) and refused otherwise.
  * replacement `lm_head` / `embed_tokens` tensors (adapters trained with resized vocabularies) are refused by name: not built here.
"""
from __future__ import annotations

import json
import math
import os

import torch


class ExLlamaV2Lora:

    @staticmethod
    def from_directory(model, directory: str, lora_scaling: float = 1.0):
        """lora.py:30-42: adapter_config.json + adapter_model.safetensors | adapter_model.bin in `directory`"""
        config_path = os.path.join(directory, "adapter_config.json")
        for name in ("adapter_model.safetensors", "adapter_model.bin"):
            lora_path = os.path.join(directory, name)
            if os.path.exists(lora_path):
                return ExLlamaV2Lora(model, config_path, lora_path, lora_scaling)
        raise ValueError(f"no adapter_model.safetensors or adapter_model.bin in {directory}")

    def __init__(self, model, lora_config_path: str, lora_path: str, lora_scaling: float = 1.0):
        self.model = model
        self.config = model.config
        self.lora_config_path, self.lora_path = lora_config_path, lora_path
        self.tensors = {}                      # "model.layers.<i>.<part>.<proj>.lora_A|lora_B.weight" -> fp16 tensor on the model's device
        self.target_modules = {}               # the same keys -> ExLlamaV2Linear
        self.bias_ignored = False
        if not model.loaded:
            raise ValueError("ExLlamaV2Lora: load the model first")

        with open(lora_config_path, encoding="utf8") as f:
            cfg = json.load(f)
        self.lora_r = int(cfg["r"])
        alpha = float(cfg["lora_alpha"])
        if cfg.get("use_rslora", False):
            alpha *= math.sqrt(self.lora_r)
        self.lora_alpha = alpha
        self.lora_scaling = float(lora_scaling) * alpha / self.lora_r
        if cfg.get("fan_in_fan_out", False):
            raise ValueError("ExLlamaV2Lora: fan_in_fan_out adapters are not supported")

        if lora_path.endswith(".safetensors"):
            from safetensors.torch import load_file
            f = load_file(lora_path, device="cpu")
        else:
            f = torch.load(lora_path, map_location="cpu")

        linears = model.linear_modules()
        staged = []
        for key, tensor in f.items():
            if key.endswith((".original_module.weight", ".modules_to_save.weight")):
                continue
            if key.endswith(("lm_head.weight", "embed_tokens.weight")):
                raise ValueError(f"ExLlamaV2Lora: {key}: replacement lm_head / embed_tokens tensors are not built in this runtime")
            i = key.find("model.layers.")
            if i < 0:
                raise ValueError(f"ExLlamaV2Lora: unsupported layer in {lora_path}: {key}")
            target_key = key[i:]
            parts = target_key.split(".")
            half = parts[-2]
            if half == "bias" or parts[-1] == "bias":
                if float(tensor.float().abs().max()) > 1e-6:
                    raise ValueError(f"ExLlamaV2Lora: unsupported bias target in {lora_path}: {key}")
                self.bias_ignored = True
                continue
            if half not in ("lora_A", "lora_B"):
                raise ValueError(f"ExLlamaV2Lora: unsupported layer in {lora_path}: {key}")
            lin = linears.get(".".join(parts[:-2]))
            if lin is None:
                raise ValueError(f"ExLlamaV2Lora: {key} targets no linear layer of this model")
            if tensor.dtype not in (torch.float16, torch.bfloat16, torch.float32):
                raise ValueError(f"ExLlamaV2Lora: unsupported tensor dtype {tensor.dtype} in {lora_path}")
            ok = tensor.dim() == 2 and (tensor.shape[1] == lin.in_features if half == "lora_A" else tensor.shape[0] == lin.out_features)
            if not ok:
                raise ValueError(f"ExLlamaV2Lora: incompatible tensor shape in {lora_path}: {key} {tuple(tensor.shape)}")
            t = tensor.float().t()
            if half == "lora_B":
                t = t * self.lora_scaling
            staged.append((target_key, lin, half, t.to(torch.float16).contiguous().to(model.device)))

        # (nothing is attached before the whole file has been accepted)
        for target_key, lin, half, t in staged:
            (lin.lora_a_tensors if half == "lora_A" else lin.lora_b_tensors)[self] = t
            self.tensors[target_key] = t
            self.target_modules[target_key] = lin
        try:
            model.update_loras()
        except Exception:
            self._detach()
            model.update_loras()
            raise

    def _detach(self):
        for lin in self.target_modules.values():
            lin.lora_a_tensors.pop(self, None)
            lin.lora_b_tensors.pop(self, None)
        self.tensors, self.target_modules = {}, {}

    def unload(self):
        """lora.py:197-214: detach from every target and rebuild the modules' adapter tables"""
        self._detach()
        self.model.update_loras()
