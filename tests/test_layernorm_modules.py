"""q_attn / q_mlp handles of LayerNorm models at the operator boundary: a LayerNorm pre-norm with or without bias (StarCoder2), biased
q / k / v / o and MLP projections, an ungated MLP, and the norm-less, residual-less handles a parallel block builds (Cohere:
parallel_decoder.py:47-62 -- the projection output OVERWRITES the rows the module was given).  1, 3 and 17 rows: the decode launches and the
MFMA route.

Checker: tests/layernorm_oracle.py (layer_norm.cu restated) and the reconstructed weights.  Bars: those of tests/test_gemma_modules.py
for the same entries, term for term:
  * q / k / v: 3 x half_tol of the exact projection (one fp16 rounding, RoPE of a value one ulp off);
  * o_proj / down_proj into the fp16 stream: half_tol of the exact projection plus 2^-10 of the sum for the fp16 add (or store), plus
    2^-11 of sum |a_k w_k|: the kernels scale a quantization group AFTER its dot product (csrc/qgemv_common.h) where the oracle multiplies
    weights rounded to fp16 one by one.  tests/test_gemma_modules.py names that term and lets the 2^-10 of its (fp32, large) stream hold
    it; a residual-less handle has no stream to hold it, so it is written out here;
  * act(up) resp. act(gate) * up: |d gelu| <= 1.13, |d silu| <= 1.1, so dy <= slope dg |u| + |act(g)| du + 2^-10 |y|, carried through |W_down|."""
import numpy as np
import pytest
import torch

from oracle import exl2 as OX
from oracle import modules as OM
from tests import layernorm_oracle as LO
from tests.util import exl2_to_torch, gptq_to_torch, half_tol
from exllamav2_amd.ext import none_tensor

F16, F32, F64 = np.float16, np.float32, np.float64
HID, INTER, NH, NKV, HD, MAXSEQ, MAXROWS = 256, 512, 4, 2, 64, 64, 64
EPS = 1e-5
ROWS = [1, 3, 17]
DIMS = {"q": (HID, NH * HD), "k": (HID, NKV * HD), "v": (HID, NKV * HD), "o": (NH * HD, HID),
        "gate": (HID, INTER), "up": (HID, INTER), "down": (INTER, HID)}
# norm: None (the block owns it) | "ln" | "ln+bias"; residual: has_residual; bias: biased projections; gate: gated MLP; gelu; neox
CASES = {
    "starcoder2": dict(norm="ln+bias", residual=True, bias=True, gate=False, gelu=True, neox=True),
    "ln-plain": dict(norm="ln", residual=True, bias=False, gate=True, gelu=False, neox=True),
    "cohere": dict(norm=None, residual=False, bias=False, gate=True, gelu=False, neox=False),
    "parallel-biased": dict(norm=None, residual=False, bias=True, gate=False, gelu=True, neox=False),
}


def _lin(be, k, n, seed, gptq, bias):
    if gptq:
        t = OX.synth_gptq(k, n, 128, seed=seed, act_order=False)
        ref, w = OX.gptq_reconstruct(t), gptq_to_torch(be, t)
    else:
        t = OX.synth_exl2(k, n, [(5, 32, 32), (4, 32, k - 32)], seed=seed, act_order=True, sigma=0.06)      # ~4.0 bpw
        ref, w = OX.exl2_reconstruct(t), exl2_to_torch(be, t)
    b = None
    if bias:
        b = (0.2 * np.random.default_rng(9000 + seed).standard_normal(n)).astype(F16)
        w["bias"] = be.t(b)
    return ref.astype(F64), b, be.ext.make_q_matrix_from_dict(w, None), w


class Block:
    def __init__(self, be, case, gptq=False, seed=240, post=False, residual_fp32=False):
        self.be, self.c = be, CASES[case]
        c = self.c
        self.refs, self.bias, self.hs, self.keep = {}, {}, {}, []
        for i, (name, (k, n)) in enumerate(DIMS.items()):
            if name == "gate" and not c["gate"]:
                continue
            self.refs[name], self.bias[name], self.hs[name], w = _lin(be, k, n, seed + i, gptq, c["bias"])
            self.keep.append(w)
        rng = np.random.default_rng(seed)
        self.w = {n: (1 + 0.1 * rng.standard_normal(HID)).astype(F16) for n in ("ln_attn", "ln_mlp")}
        self.b = {n: (0.1 * rng.standard_normal(HID)).astype(F16) for n in ("ln_attn", "ln_mlp")}
        self.wt = {n: be.t(v) for n, v in self.w.items()}
        self.bt = {n: be.t(v) for n, v in self.b.items()}
        z = lambda n: torch.zeros((MAXROWS, n), dtype=torch.float16, device=be.device)
        self.temp_state, self.temp_a, self.temp_b = z(HID), z(INTER), z(INTER)
        self.attn = self.mlp = None
        self.sin, self.cos = OM.rope_tables(MAXSEQ, HD, neox=c["neox"])
        self.sin_t, self.cos_t = be.t(self.sin), be.t(self.cos)
        try:
            norm = lambda n: (self.wt[n] if c["norm"] else none_tensor, self.bt[n] if c["norm"] == "ln+bias" else none_tensor)
            pw = self.wt["ln_attn"] if post else none_tensor
            wa, ba = norm("ln_attn")
            self.attn = be.ext.make_q_attn(wa, ba, False, False, EPS, self.hs["q"], self.hs["k"], self.hs["v"], self.hs["o"], self.temp_state,
                                           none_tensor, MAXROWS, HID, NH, NKV, HD, MAXSEQ, c["residual"], 2 if c["neox"] else 1, HD,
                                           none_tensor, none_tensor, pw, none_tensor, residual_fp32, False)
            wm, bm = norm("ln_mlp")
            self.mlp = be.ext.make_q_mlp(wm, bm, False, EPS, self.hs.get("gate"), self.hs["up"], self.hs["down"], self.temp_state, self.temp_a,
                                         self.temp_b, none_tensor, MAXROWS, c["gelu"], c["residual"], pw, none_tensor, residual_fp32, False)
        except Exception:
            self.free()
            raise

    def ln(self, x, which):
        c = self.c
        if not c["norm"]:
            return x
        return LO.layer_norm(x, self.w[which], self.b[which] if c["norm"] == "ln+bias" else None, EPS)

    def lin(self, a, name):
        y = a.astype(F64) @ self.refs[name]
        return y if self.bias[name] is None else y + self.bias[name].astype(F64)

    def qkv_buffers(self, rows):
        z = lambda n: torch.zeros((1, rows, n), dtype=torch.float16, device=self.be.device)
        return z(NH * HD), z(NKV * HD), z(NKV * HD)

    def free(self):
        if self.attn: self.be.ext.free_q_attn(self.attn)
        if self.mlp: self.be.ext.free_q_mlp(self.mlp)
        for v in self.hs.values():
            self.be.ext.free_q_matrix(v)


def _check(got, want, tol, what):
    err = np.abs(got.astype(F64) - want.astype(F64))
    worst = float((err / tol).max())
    print(f"{what}: max err/tol = {worst:.3f}")
    assert got.shape == want.shape and np.all(err <= tol), f"{what}: max err/tol {worst:.3f}"


def _mlp_want(blk, x):
    """-> (the fp16 rows the MLP leaves in x, bar)"""
    c = blk.c
    n = blk.ln(x, "ln_mlp")
    u64 = blk.lin(n, "up")
    u16 = u64.astype(F16)
    act = LO.gelu if c["gelu"] else LO.silu
    slope = 1.13 if c["gelu"] else 1.1
    if c["gate"]:
        g64 = blk.lin(n, "gate")
        g16 = g64.astype(F16)
        y = np.clip(OM.hmul(act(g16), u16).astype(F32), -65504.0, 65504.0).astype(F16)
        dy = slope * half_tol(g64, HID) * np.abs(u16.astype(F64)) + np.abs(act(g16).astype(F64)) * half_tol(u64, HID) \
            + 2.0 ** -10 * np.abs(y.astype(F64)) + 1e-6
    else:
        y = act(u16)
        dy = slope * half_tol(u64, HID) + 2.0 ** -10 * np.abs(y.astype(F64)) + 1e-6
    t64 = blk.lin(y, "down")
    want = ((x.astype(F64) if c["residual"] else 0.0) + t64).astype(F16)
    tol = half_tol(t64, INTER) + dy @ np.abs(blk.refs["down"]) + 2.0 ** -10 * np.abs(want.astype(F64)) \
        + 2.0 ** -11 * (np.abs(y.astype(F64)) @ np.abs(blk.refs["down"]))
    return want, tol


@pytest.mark.parametrize("case,gptq", [(c, False) for c in CASES] + [("starcoder2", True), ("cohere", True)],
                         ids=[c + "-exl2" for c in CASES] + ["starcoder2-gptq", "cohere-gptq"])
def test_layernorm_block(be, case, gptq):
    blk = Block(be, case, gptq)
    ext, c = be.ext, blk.c
    try:
        for rows in ROWS:
            rng = np.random.default_rng(400 + rows)
            past = 5
            x = (rng.standard_normal((rows, HID)) * 2.0 + 0.5).astype(F16)
            a = rng.standard_normal((rows, NH * HD)).astype(F16)
            xt = be.t(x.reshape(1, rows, HID))
            q, k, v = blk.qkv_buffers(rows)
            ext.q_attn_forward_1(blk.attn, xt, 1, rows, past, none_tensor, q, k, v, blk.sin_t, blk.cos_t)
            assert np.array_equal(be.n(xt).reshape(rows, HID).view(np.uint16), x.view(np.uint16))      # forward_1 does not write the rows
            n = blk.ln(x, "ln_attn")
            for name, heads, got in (("q", NH, q), ("k", NKV, k), ("v", NKV, v)):
                ex = blk.lin(n, name)
                w16 = ex.astype(F16)
                if name != "v":
                    w16 = OM.rope_(w16.reshape(1, rows, heads, HD), blk.sin, blk.cos, np.array([past]), neox=c["neox"]).reshape(rows, heads * HD)
                _check(be.n(got).reshape(rows, -1), w16, 3 * half_tol(ex, HID), f"{case} {name} rows={rows}")
            # o_proj: added to the rows (has_residual) or stored over them
            ext.q_attn_forward_2(blk.attn, xt, be.t(a.reshape(1, rows, -1)), 1, rows)
            t64 = blk.lin(a, "o")
            want1 = ((x.astype(F64) if c["residual"] else 0.0) + t64).astype(F16)
            x1 = be.n(xt).reshape(rows, HID).copy()
            tol1 = half_tol(t64, NH * HD) + 2.0 ** -10 * np.abs(want1.astype(F64)) + 2.0 ** -11 * (np.abs(a.astype(F64)) @ np.abs(blk.refs["o"]))
            _check(x1, want1, tol1, f"{case} o_proj rows={rows}")
            # the MLP: on the stream (sequential) or on a second copy of the block's normed rows (parallel)
            xm = x1 if c["residual"] else x
            xmt = be.t(xm.reshape(1, rows, HID))
            ext.q_mlp_forward_(blk.mlp, xmt)
            want2, tol2 = _mlp_want(blk, xm)
            x2 = be.n(xmt).reshape(rows, HID).copy()
            _check(x2, want2, tol2, f"{case} mlp rows={rows}")
            assert not np.array_equal(x2.view(np.uint16), xm.view(np.uint16))
    finally:
        blk.free()


def test_layernorm_handles_stay_off_the_chain(be):
    blk = Block(be, "starcoder2")
    try:
        assert not be.ext.q_attn_chain_info(blk.attn)[0] and not be.ext.q_mlp_chain_info(blk.mlp)[0]
    finally:
        blk.free()


def test_refusals(be):
    ext = be.ext
    with pytest.raises(RuntimeError, match="post norm next to a LayerNorm"):
        Block(be, "ln-plain", post=True).free()
    with pytest.raises(RuntimeError, match="fp32 residual"):
        Block(be, "ln-plain", residual_fp32=True).free()
    blk = Block(be, "starcoder2")
    try:
        la = torch.zeros((HID, 8), dtype=torch.float16, device=be.device)
        lb = torch.zeros((8, NH * HD), dtype=torch.float16, device=be.device)
        with pytest.raises(RuntimeError, match="LayerNorm"):
            ext.q_attn_set_loras(blk.attn, {1: (la, lb, 8)}, {}, {}, {})
        lb2 = torch.zeros((8, INTER), dtype=torch.float16, device=be.device)
        with pytest.raises(RuntimeError, match="LayerNorm"):
            ext.q_mlp_set_loras(blk.mlp, {}, {1: (la, lb2, 8)}, {})
    finally:
        blk.free()


def test_compiled_binding_runs_layernorm_handles_plain(be):
    """dropin/_exl2_fast.cpp on handles that are not chain-capable: the module chain stands aside, the results are the ctypes route's bit
    for bit -- also for the two calls of a parallel block on two copies of the normed rows (parallel_decoder.py:137-143), with the
    chain's self-check on"""
    from tests.test_dropin_fast import load_fast
    fast = load_fast(be)
    ext = be.ext
    for case in ("starcoder2", "cohere"):
        blk = Block(be, case)
        try:
            rows, past = 3, 5
            rng = np.random.default_rng(78)
            x = (rng.standard_normal((1, rows, HID)) * 2.0).astype(F16)
            a = be.t(rng.standard_normal((1, rows, NH * HD)).astype(F16))
            fast.stats(True)
            fast.set_verify(True)
            outs = []
            for route in ("ctypes", "fast", "fast"):                                 # (twice: what the first pass learnt must not engage)
                xa = be.t(x)
                xb = xa if blk.c["residual"] else xa.clone()                         # parallel: the second module runs on a clone
                q, k, v = blk.qkv_buffers(rows)
                if route == "fast":
                    fast.q_attn_forward_1(blk.attn, xa, 1, rows, past, none_tensor, q, k, v, blk.sin_t, blk.cos_t, [], none_tensor)
                    fast.q_attn_forward_2(blk.attn, xa, a, 1, rows, [], none_tensor)
                    fast.q_mlp_forward_(blk.mlp, xb, [], none_tensor)
                else:
                    ext.q_attn_forward_1(blk.attn, xa, 1, rows, past, none_tensor, q, k, v, blk.sin_t, blk.cos_t)
                    ext.q_attn_forward_2(blk.attn, xa, a, 1, rows)
                    ext.q_mlp_forward_(blk.mlp, xb)
                outs.append([be.n(t).copy() for t in (q, k, v, xa, xb)])
            for o in outs[1:]:
                for g, w in zip(o, outs[0]):
                    assert np.array_equal(g.view(np.uint8), w.view(np.uint8))
            st = fast.stats(False)
            assert st["plain"] == 6 and st["chained"] == 0 and st["published"] == 0
        finally:
            fast.set_verify(False)
            fast.forget_module(blk.attn); fast.forget_module(blk.mlp)
            blk.free()
