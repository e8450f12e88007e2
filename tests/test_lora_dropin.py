"""LoRA adapters through the drop-in `exllamav2_ext` (dropin/exllamav2_ext.py, dropin/_exl2_fast.cpp), called the way the reference
host calls it: q_attn_set_loras / q_mlp_set_loras with one {id(lora): tensor} dict per projection half (attn.py:1545-1564,
mlp.py:525-542), the module forwards with the `loras` id list and a `loras_temp` tensor of max_rank x rows (attn.py:1128-1141).

A host written here plays module calls on ONE residual tensor, steps with and without adapters interleaved, through the ctypes route
and through the compiled binding (skipped where _exl2_fast is not built).  Calls with adapters equal the native module calls
(exllamav2_amd.ext) bit for bit on both routes, and so do the plain calls of the ctypes route.  The compiled binding serves plain
decode-sized calls with the chained kernels (another kernel, the same arithmetic): those are held to the bar tests/test_dropin_fast.py
holds them to, and the binding's counters show that the call behind an adapter step made its own hand-off instead of using one
published before the adapters changed x.  The reference is not imported."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from exllamav2_amd.ext import none_tensor
from exllamav2_amd.model import ExLlamaV2
from exllamav2_amd.synth import synth_checkpoint
from tests.conftest import ROOT
from tests.lora_oracle import make_adapter
from tests.test_dropin_fast import cfg_small


class FakeLora:
    """what the reference keys its dicts by: id(lora object)"""


def load_dropin(be, monkeypatch):
    """dropin/exllamav2_ext.py bound to the backend's library, its per-token calls on the ctypes route"""
    import exllamav2_amd.ext as X
    monkeypatch.setattr(X, "ext_c", be.ext)
    monkeypatch.setenv("EXL2_DROPIN_FAST", "0")
    spec = importlib.util.spec_from_file_location("exllamav2_ext_under_test", os.path.join(ROOT, "dropin", "exllamav2_ext.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _fast_or_skip(be):
    from exllamav2_amd import build
    if not os.path.exists(build.FAST_OUT):
        pytest.skip("dropin/_exl2_fast.so is not built")
    from tests.test_dropin_fast import load_fast
    return load_fast(be)


@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("route", ["ctypes", "compiled"])
def test_reference_style_host_with_adapters_interleaved(be, monkeypatch, route, rows):
    E = load_dropin(be, monkeypatch)
    fast = _fast_or_skip(be) if route == "compiled" else None
    F = fast if fast is not None else E
    cfg = cfg_small(num_hidden_layers=1)
    model = ExLlamaV2(cfg, device=be.device, ext=be.ext).load(synth_checkpoint(cfg, be.device, seed=9))
    attn, mlp = model.layers[0]
    H, KVH, hd, hid = cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim, cfg.hidden_size
    rng = np.random.default_rng(rows)
    dims = {"q": (hid, H * hd), "k": (hid, KVH * hd), "v": (hid, KVH * hd), "o": (H * hd, hid),
            "gate": (hid, cfg.intermediate_size), "up": (hid, cfg.intermediate_size), "down": (cfg.intermediate_size, hid)}
    l1, l2 = FakeLora(), FakeLora()
    A, B = {n: {} for n in dims}, {n: {} for n in dims}
    for lora, r, names in ((l1, 8, tuple(dims)), (l2, 20, ("q", "v"))):
        for n in names:
            a, b = make_adapter(rng, *dims[n], r, amp=0.5)
            A[n][id(lora)], B[n][id(lora)] = be.t(a), be.t(b)
    max_rank = max(E.q_attn_set_loras(attn.q_handle, A["q"], B["q"], A["k"], B["k"], A["v"], B["v"], A["o"], B["o"]),
                   E.q_mlp_set_loras(mlp.q_handle, A["gate"], B["gate"], A["up"], B["up"], A["down"], B["down"]))
    assert max_rank == 20
    loras_temp = torch.zeros((max_rank * rows,), dtype=torch.float16, device=be.device)

    x = be.t((0.5 * rng.standard_normal((1, rows, hid))).astype(np.float16))           # ONE residual tensor for the whole run
    xr = x.clone()                                                                        # the native calls' copy
    new = lambda n: torch.zeros((1, rows, n), dtype=torch.float16, device=be.device)
    close = lambda a, b: np.all(np.abs(be.n(a).astype(np.float64) - be.n(b)) <= 0.03 + np.abs(be.n(b).astype(np.float64)) * 2.0 ** -8)
    if fast is not None:
        fast.set_chain(True); fast.reset()
    for step, ids in enumerate([[], [id(l1), id(l2)], [], [id(l2)], [], [], []]):
        exact = bool(ids) or fast is None
        same = torch.equal if exact else close
        ao = be.t(rng.standard_normal((1, rows, H * hd)).astype(np.float16))
        q, k, v, qr, kr, vr = new(H * hd), new(KVH * hd), new(KVH * hd), new(H * hd), new(KVH * hd), new(KVH * hd)
        if fast is not None: fast.stats(True)
        F.q_attn_forward_1(attn.q_handle, x, 1, rows, step, none_tensor, q, k, v, model.sin, model.cos, ids, loras_temp if ids else none_tensor)
        if fast is not None and not ids and step > 0:
            st = fast.stats(True)
            # behind an adapter step (2, 4) nothing published may be used: the call makes its own hand-off from x.  Step 5 does too (the
            # binding learns there that this attention follows this MLP on x); step 6 then starts from what step 5's MLP published.
            assert (st["published"], st["chained"]) == ((0, 1) if step == 6 else (1, 0)), (step, st)
        be.ext.q_attn_forward_1(attn.q_handle, xr, 1, rows, step, none_tensor, qr, kr, vr, model.sin, model.cos, loras=ids)
        assert same(q, qr) and same(k, kr) and same(v, vr), (route, step, "forward_1")
        F.q_attn_forward_2(attn.q_handle, x, ao, 1, rows, ids, loras_temp if ids else none_tensor)
        be.ext.q_attn_forward_2(attn.q_handle, xr, ao, 1, rows, loras=ids)
        assert same(x, xr), (route, step, "forward_2")
        F.q_mlp_forward_(mlp.q_handle, x, ids, loras_temp if ids else none_tensor)
        be.ext.q_mlp_forward_(mlp.q_handle, xr, loras=ids)
        assert same(x, xr), (route, step, "mlp")
        if not exact:
            xr.copy_(x)                 # (follow the route under test: each plain step is compared alone)
    # the adapters mattered: a step with them differs from the same step without
    y0, y1 = x.clone(), x.clone()
    be.ext.q_mlp_forward_(mlp.q_handle, y0)
    be.ext.q_mlp_forward_(mlp.q_handle, y1, loras=[id(l1)])
    assert not torch.equal(y0, y1)
    if fast is not None:
        fast.forget_module(attn.q_handle); fast.forget_module(mlp.q_handle)
    model.unload()


def test_dropin_refusals_and_empty_tables(be, monkeypatch):
    E = load_dropin(be, monkeypatch)
    cfg = cfg_small(num_hidden_layers=1)
    model = ExLlamaV2(cfg, device=be.device, ext=be.ext).load(synth_checkpoint(cfg, be.device, seed=9))
    attn, mlp = model.layers[0]
    assert E.q_attn_set_loras(attn.q_handle, {}, {}, {}, {}, {}, {}, {}, {}) == 0          # what a host without adapters does at load
    assert E.q_mlp_set_loras(mlp.q_handle, {}, {}, {}, {}, {}, {}) == 0
    x = torch.zeros((1, cfg.hidden_size), dtype=torch.float16, device=be.device)
    with pytest.raises(RuntimeError, match="MoE"):
        E.q_moe_mlp_forward_(0, x, [1], none_tensor)
    model.unload()
