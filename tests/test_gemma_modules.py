"""q_attn / q_mlp handles with an fp32 residual stream (Gemma-2 / Gemma-3 blocks), at the operator boundary.

Checker: tests/gemma_oracle.py -- pre-norm fp32 -> fp16, every projection -> fp16, GELU(gate) * up -> fp16, the post norm of the fp16
projection output added to the stream in fp32 (q_attn.cu:268-279, :337-339, q_mlp.cu:183, :230).

Bars, those of tests/test_qattn_op.py and tests/test_lora_modules.py for the same entries (derived there, every element compared):
  * q / k / v: 3 x half_tol of the exact projection (one fp16 rounding, RoPE of a value one ulp off);
  * the post-norm branch, tests/test_lora_modules.py's bar term for term: the error of t = fp16(y W) times |w| * rsqrt(mean t^2 + eps),
    plus 2^-9 |norm| for the scale's relative error and the norm's rounding, plus 2^-10 of the sum.  That last term is sized there for
    the fp16 residual add; the add is fp32 here, and what the term still has to cover is that the kernels scale a quantization group
    AFTER its dot product (csrc/qgemv_common.h) where the oracle multiplies weights rounded to fp16 one by one: up to 2^-11 of
    sum |a_k w_k| in t, which half_tol's floor does not hold for every element of a GPTQ projection (weights of ~0.1);
  * GELU(gate) * up: |d gelu| <= 1.13, so dy <= 1.13 dg |u| + |gelu(g)| du + 2^-10 |y|, carried through |W_down|.
The form for callers that own the norms (the `_normed` entries + exl2_norm_bridge) must leave the same stream bit for bit."""
import numpy as np
import pytest
import torch

from oracle import exl2 as OX
from oracle import modules as OM
from tests import gemma_oracle as GO
from tests.util import exl2_to_torch, gptq_to_torch, half_tol
from exllamav2_amd.ext import none_tensor

F16, F32, F64 = np.float16, np.float32, np.float64
HID, INTER, NH, NKV, HD, MAXSEQ, MAXROWS = 256, 512, 4, 2, 64, 64, 64
EPS = 1e-6
ROWS = [1, 5, 40]
ATTN_DIMS = {"q": (HID, NH * HD), "k": (HID, NKV * HD), "v": (HID, NKV * HD), "o": (NH * HD, HID)}
MLP_DIMS = {"gate": (HID, INTER), "up": (HID, INTER), "down": (INTER, HID)}


def _lin(be, k, n, seed, gptq):
    if gptq:
        t = OX.synth_gptq(k, n, 128, seed=seed, act_order=False)
        ref, w = OX.gptq_reconstruct(t), gptq_to_torch(be, t)
    else:
        t = OX.synth_exl2(k, n, [(5, 32, 32), (4, 32, k - 32)], seed=seed, act_order=True, sigma=0.06)      # ~4.0 bpw
        ref, w = OX.exl2_reconstruct(t), exl2_to_torch(be, t)
    return ref.astype(F64), be.ext.make_q_matrix_from_dict(w, None), w


class Block:
    """one attention handle and one MLP handle with residual_fp32, sharing temp_state as the native model's do"""

    def __init__(self, be, gptq, residual_fp32=True, post=True, seed=140):
        self.be = be
        self.refs, self.hs, self.keep = {}, {}, []
        for i, (name, (k, n)) in enumerate({**ATTN_DIMS, **MLP_DIMS}.items()):
            self.refs[name], self.hs[name], w = _lin(be, k, n, seed + i, gptq)
            self.keep.append(w)
        rng = np.random.default_rng(seed)
        self.w = {n: (1 + 0.1 * rng.standard_normal(HID)).astype(F16) for n in ("ln_attn", "post_attn", "ln_mlp", "post_mlp")}
        self.wt = {n: be.t(v) for n, v in self.w.items()}
        z = lambda n: torch.zeros((MAXROWS, n), dtype=torch.float16, device=be.device)
        self.temp_state, self.temp_a, self.temp_b = z(HID), z(INTER), z(INTER)
        pa = self.wt["post_attn"] if post else none_tensor
        pm = self.wt["post_mlp"] if post else none_tensor
        self.attn = self.mlp = None
        try:
            self._make(be, pa, pm, residual_fp32)
        except Exception:
            self.free()
            raise
        self.sin, self.cos = OM.rope_tables(MAXSEQ, HD, neox=True)
        self.sin_t, self.cos_t = be.t(self.sin), be.t(self.cos)

    def _make(self, be, pa, pm, residual_fp32):
        self.attn = be.ext.make_q_attn(self.wt["ln_attn"], none_tensor, True, False, EPS, self.hs["q"], self.hs["k"], self.hs["v"], self.hs["o"],
                                       self.temp_state, none_tensor, MAXROWS, HID, NH, NKV, HD, MAXSEQ, True, 2, HD, none_tensor, none_tensor,
                                       pa, none_tensor, residual_fp32, False)
        self.mlp = be.ext.make_q_mlp(self.wt["ln_mlp"], none_tensor, True, EPS, self.hs["gate"], self.hs["up"], self.hs["down"], self.temp_state,
                                     self.temp_a, self.temp_b, none_tensor, MAXROWS, True, True, pm, none_tensor, residual_fp32, False)

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


def _post_norm_want(t64, pw, x32, k_terms, extra=0.0):
    """-> (fp32 stream the reference leaves, bar) for t = fp16(t64) normed with pw and added to x32"""
    t16 = t64.astype(F16)
    tf = np.clip(t16.astype(F64), -65504, 65504)
    r = 1.0 / np.sqrt((tf ** 2).sum(-1, keepdims=True) / HID + EPS)
    n64 = tf * pw.astype(F64) * r
    want = GO.post_norm_add(t16, pw, x32, EPS)
    tol = (half_tol(t64, k_terms) + extra) * np.abs(pw.astype(F64)) * r + 2.0 ** -9 * np.abs(n64) + 2.0 ** -10 * np.abs(want.astype(F64))
    return want, tol


def _mlp_want(blk, x32):
    n = GO.rms_norm_any(x32, blk.w["ln_mlp"], EPS)
    g64, u64 = n.astype(F64) @ blk.refs["gate"], n.astype(F64) @ blk.refs["up"]
    g16, u16 = g64.astype(F16), u64.astype(F16)
    y = GO.gelu_mul(g16, u16)
    g = g16.astype(F64)
    gelu = 0.5 * g * (1.0 + np.tanh(0.797884560803 * (g + 0.044715 * g ** 3)))
    dy = 1.13 * half_tol(g64, HID) * np.abs(u16.astype(F64)) + np.abs(gelu) * half_tol(u64, HID) + 2.0 ** -10 * np.abs(y.astype(F64)) + 1e-6
    t64 = y.astype(F64) @ blk.refs["down"]
    return _post_norm_want(t64, blk.w["post_mlp"], x32, INTER, extra=dy @ np.abs(blk.refs["down"]))


@pytest.mark.parametrize("gptq", [False, True], ids=["exl2", "gptq"])
def test_fp32_residual_block(be, gptq):
    blk = Block(be, gptq)
    ext = be.ext
    try:
        for rows in ROWS:
            rng = np.random.default_rng(300 + rows)
            past = 5
            x = (rng.standard_normal((rows, HID)) * 4.0).astype(F32)
            a = rng.standard_normal((rows, NH * HD)).astype(F16)
            # ---- the handles' own norms: q_attn_forward_1 / _2 and q_mlp_forward_ on fp32 x
            xt = be.t(x.reshape(1, rows, HID))
            q, k, v = blk.qkv_buffers(rows)
            ext.q_attn_forward_1(blk.attn, xt, 1, rows, past, none_tensor, q, k, v, blk.sin_t, blk.cos_t)
            assert np.array_equal(be.n(xt).reshape(rows, HID), x)                     # forward_1 does not write the stream
            n = GO.rms_norm_any(x, blk.w["ln_attn"], EPS)
            for name, heads, got in (("q", NH, q), ("k", NKV, k), ("v", NKV, v)):
                ex = OX.gemm_ref(n, blk.refs[name], exact=True)
                w16 = ex.astype(F16)
                if name != "v":
                    w16 = OM.rope_(w16.reshape(1, rows, heads, HD), blk.sin, blk.cos, np.array([past]), neox=True).reshape(rows, heads * HD)
                _check(be.n(got).reshape(rows, -1), w16, 3 * half_tol(ex, HID), f"{name} rows={rows}")
            ext.q_attn_forward_2(blk.attn, xt, be.t(a.reshape(1, rows, -1)), 1, rows)
            want1, tol1 = _post_norm_want(a.astype(F64) @ blk.refs["o"], blk.w["post_attn"], x, NH * HD)
            x1 = be.n(xt).reshape(rows, HID).copy()
            assert x1.dtype == F32
            _check(x1, want1, tol1, f"o + post norm rows={rows}")
            ext.q_mlp_forward_(blk.mlp, xt)
            want2, tol2 = _mlp_want(blk, x1)
            x2 = be.n(xt).reshape(rows, HID).copy()
            _check(x2, want2, tol2, f"mlp rows={rows}")
            assert not np.array_equal(x2, x1)

            # ---- the caller owns the norms: `_normed` entries + the bridge
            ts = blk.temp_state[:rows]
            xo = be.t(x)
            xn = torch.zeros((rows, HID), dtype=torch.float16, device=be.device)
            ext.rms_norm(xo, blk.wt["ln_attn"], xn, EPS)
            q2, k2, v2 = blk.qkv_buffers(rows)
            ext.q_attn_forward_1_normed(blk.attn, xn, 1, rows, past, none_tensor, q2, k2, v2, blk.sin_t, blk.cos_t)
            for g1, g2 in ((q, q2), (k, k2), (v, v2)):
                assert np.array_equal(be.n(g1).view(np.uint16), be.n(g2).view(np.uint16))
            ext.q_attn_forward_2_normed(blk.attn, be.t(a), 1, rows)
            assert ext.norm_bridge(ts, xo, blk.wt["post_attn"], blk.wt["ln_mlp"], ts, EPS)
            assert np.array_equal(be.n(xo).view(np.uint32), x1.view(np.uint32)), "stream after attention differs from the handle's"
            # the next module's input: the two-launch norm of the same stream, within the bridge bound (tests/test_norm_bridge.py)
            n_two = torch.zeros((rows, HID), dtype=torch.float16, device=be.device)
            ext.rms_norm(be.t(x1), blk.wt["ln_mlp"], n_two, EPS)
            got_n, want_n = be.n(ts).copy(), be.n(n_two)
            key = lambda h: np.where(h.view(np.uint16) & 0x8000, -(h.view(np.uint16).astype(np.int32) & 0x7FFF), h.view(np.uint16).astype(np.int32))
            assert np.all(np.abs(key(got_n) - key(want_n)) <= 1)
            assert int((got_n.view(np.uint16) != want_n.view(np.uint16)).sum()) <= rows * HID // 1000
            # the MLP from the two-launch rows: bit for bit the handle's stream (down_proj's output stays in temp_state for the bridge)
            ext.q_mlp_forward_normed(blk.mlp, n_two)
            assert ext.norm_bridge(ts, xo, blk.wt["post_mlp"], none_tensor, none_tensor, EPS)
            assert np.array_equal(be.n(xo).view(np.uint32), x2.view(np.uint32)), "stream after the MLP differs from the handle's"
    finally:
        blk.free()


def test_refusals(be):
    ext = be.ext
    # an fp32 residual stream without post norms: the reference's own sanity check (architecture.py:955-957)
    with pytest.raises(RuntimeError, match="post norm"):
        Block(be, False, residual_fp32=True, post=False).free()
    blk = Block(be, False)
    half = Block(be, False, residual_fp32=False)
    try:
        rows = 2
        x32 = torch.zeros((1, rows, HID), dtype=torch.float32, device=be.device)
        x16 = torch.zeros((1, rows, HID), dtype=torch.float16, device=be.device)
        a = torch.zeros((1, rows, NH * HD), dtype=torch.float16, device=be.device)
        for b_, bad in ((blk, x16), (half, x32)):
            q, k, v = b_.qkv_buffers(rows)
            with pytest.raises(RuntimeError, match="expected dtype"):
                ext.q_attn_forward_1(b_.attn, bad, 1, rows, 0, none_tensor, q, k, v, b_.sin_t, b_.cos_t)
            with pytest.raises(RuntimeError, match="expected dtype"):
                ext.q_attn_forward_2(b_.attn, bad, a, 1, rows)
            with pytest.raises(RuntimeError, match="expected dtype"):
                ext.q_mlp_forward_(b_.mlp, bad)
        # adapters: the reference adds them into `(half*) hidden_state` (q_attn.cu:344)
        la = torch.zeros((HID, 8), dtype=torch.float16, device=be.device)
        lb = torch.zeros((8, NH * HD), dtype=torch.float16, device=be.device)
        with pytest.raises(RuntimeError, match="fp32 residual"):
            ext.q_attn_set_loras(blk.attn, {1: (la, lb, 8)}, {}, {}, {})
        lb2 = torch.zeros((8, INTER), dtype=torch.float16, device=be.device)
        with pytest.raises(RuntimeError, match="fp32 residual"):
            ext.q_mlp_set_loras(blk.mlp, {}, {1: (la, lb2, 8)}, {})
        assert ext.lib.exl2_q_attn_residual_fp32(blk.attn) == 1 and ext.lib.exl2_q_mlp_residual_fp32(half.mlp) == 0
    finally:
        blk.free(); half.free()


def test_compiled_binding_hands_fp32_handles_to_the_plain_entries(be):
    """dropin/_exl2_fast.cpp: the module forwards with an fp32 x on an fp32-residual handle give the ctypes route's result bit for bit,
    never through the module chain, and a dtype that does not match the handle is refused there too"""
    from tests.test_dropin_fast import load_fast
    fast = load_fast(be)
    ext = be.ext
    blk, half = Block(be, False), Block(be, False, residual_fp32=False)
    try:
        rows, past = 3, 5
        rng = np.random.default_rng(77)
        x = (rng.standard_normal((1, rows, HID)) * 4.0).astype(F32)
        a = be.t(rng.standard_normal((1, rows, NH * HD)).astype(F16))
        fast.stats(True)
        outs = []
        for route in ("ctypes", "fast"):
            xt = be.t(x)
            q, k, v = blk.qkv_buffers(rows)
            if route == "fast":
                fast.q_attn_forward_1(blk.attn, xt, 1, rows, past, none_tensor, q, k, v, blk.sin_t, blk.cos_t, [], none_tensor)
                fast.q_attn_forward_2(blk.attn, xt, a, 1, rows, [], none_tensor)
                fast.q_mlp_forward_(blk.mlp, xt, [], none_tensor)
            else:
                ext.q_attn_forward_1(blk.attn, xt, 1, rows, past, none_tensor, q, k, v, blk.sin_t, blk.cos_t)
                ext.q_attn_forward_2(blk.attn, xt, a, 1, rows)
                ext.q_mlp_forward_(blk.mlp, xt)
            outs.append([be.n(t).copy() for t in (q, k, v, xt)])
        for g, w in zip(outs[1], outs[0]):
            assert np.array_equal(g.view(np.uint8), w.view(np.uint8))
        st = fast.stats(False)
        assert st["plain"] == 3 and st["chained"] == 0 and st["published"] == 0
        x16 = torch.zeros((1, rows, HID), dtype=torch.float16, device=be.device)
        x32 = torch.zeros((1, rows, HID), dtype=torch.float32, device=be.device)
        q, k, v = blk.qkv_buffers(rows)
        for b_, bad, msg in ((blk, x16, "float32"), (half, x32, "float16")):
            with pytest.raises(RuntimeError, match=msg):
                fast.q_attn_forward_1(b_.attn, bad, 1, rows, past, none_tensor, q, k, v, b_.sin_t, b_.cos_t, [], none_tensor)
            with pytest.raises(RuntimeError, match=msg):
                fast.q_attn_forward_2(b_.attn, bad, a, 1, rows, [], none_tensor)
            with pytest.raises(RuntimeError, match=msg):
                fast.q_mlp_forward_(b_.mlp, bad, [], none_tensor)
    finally:
        for b_ in (blk, half):
            fast.forget_module(b_.attn); fast.forget_module(b_.mlp)
            b_.free()
