"""q_attn_forward_1 / q_attn_forward_2 / q_mlp_forward_ with the `loras` id list, at the operator boundary.

Checker: the oracle's reference-rounding restatement of the modules (RMSNorm -> fp16, each projection -> fp16, act * up -> fp16,
residual adds -> fp16; q_attn.cu:266-344, q_mlp.cu:176-235) plus the adapters' terms (tests/lora_oracle.py).

Bars (derived, not measured; every element compared).  Writing ht(v) = half_tol(v, K) for one fp16 rounding of a K-term sum and
`slack` for the one-ulp uncertainty of where the low-rank intermediate rounds:
  * a projection with adapters has two roundings -- the projection's store, then the adapters' add: ht(base) + ht(want) + slack;
  * RoPE rotates pairs (l, r): the bar of an element is its own plus its partner's plus ht(result) for the rotation's own roundings;
  * act(gate) * up: |d silu| <= 1.1, so dy <= 1.1 dg |u| + |silu(g)| du + 2^-10 |y|, and that error goes through down_proj and its
    adapters with the absolute values of their weights;
  * the post-norm branch: the error of t = fp16(y Wd) times |w| * rsqrt(mean t^2 + eps), plus 2^-9 |norm| for the scale's own
    relative error and the norm's rounding, plus 2^-10 of the sum for the fp16 residual add."""
import numpy as np
import pytest
import torch

from oracle import exl2 as OX
from oracle import modules as OM
from tests.lora_oracle import lora_terms, lora_add16, make_adapter
from tests.util import exl2_to_torch, gptq_to_torch, half_tol
from exllamav2_amd.ext import none_tensor

F16, F64 = np.float16, np.float64
HID, INTER, NH, NKV, HD, MAXSEQ, MAXROWS = 256, 512, 4, 2, 64, 64, 32
EPS = 1e-5
ROWS = [1, 16, 17]
ATTN_DIMS = {"q": (HID, NH * HD), "k": (HID, NKV * HD), "v": (HID, NKV * HD), "o": (NH * HD, HID)}
MLP_DIMS = {"gate": (HID, INTER), "up": (HID, INTER), "down": (INTER, HID)}


def _lin(be, k, n, seed, gptq):
    if gptq:
        t = OX.synth_gptq(k, n, 128, seed=seed, act_order=False)
        ref, w = OX.gptq_reconstruct(t), gptq_to_torch(be, t)
    else:
        t = OX.synth_exl2(k, n, [(5, 32, 32), (4, 32, k - 32)], seed=seed, act_order=True, sigma=0.06)
        ref, w = OX.exl2_reconstruct(t), exl2_to_torch(be, t)
    return ref.astype(F64), be.ext.make_q_matrix_from_dict(w, None), w


def _adapters(be, dims, which, seed):
    """two adapters: id 21 (rank 8) on the projections `which`, id 22 (rank 20) on the first of them only -> ({name: {id: tensors}},
    {name: [(A, B) numpy in id order]})"""
    rng = np.random.default_rng(seed)
    tables, pairs = {n: {} for n in dims}, {n: [] for n in dims}
    for i, r, names in ((21, 8, which), (22, 20, which[:1])):
        for n in names:
            a, b = make_adapter(rng, *dims[n], r, amp=0.5)
            tables[n][i] = (be.t(a), be.t(b), r)
            pairs[n].append((a, b))
    return tables, pairs


class Attn:
    def __init__(self, be, gptq, post, which, seed=40):
        self.be = be
        self.refs, self.hs, self.keep = {}, {}, []
        for i, (name, (k, n)) in enumerate(ATTN_DIMS.items()):
            self.refs[name], self.hs[name], w = _lin(be, k, n, seed + i, gptq)
            self.keep.append(w)
        rng = np.random.default_rng(seed)
        self.nw = (1 + 0.1 * rng.standard_normal(HID)).astype(F16)
        self.pw = (1 + 0.1 * rng.standard_normal(HID)).astype(F16) if post else None
        self.keep += [be.t(self.nw), torch.zeros((MAXROWS, HID), dtype=torch.float16, device=be.device),
                      be.t(self.pw) if post else none_tensor]
        self.h = be.ext.make_q_attn(self.keep[-3], none_tensor, True, False, EPS, self.hs["q"], self.hs["k"], self.hs["v"], self.hs["o"],
                                    self.keep[-2], none_tensor, MAXROWS, HID, NH, NKV, HD, MAXSEQ, True, 2, HD, none_tensor, none_tensor,
                                    self.keep[-1], none_tensor, False, False)
        self.tables, self.pairs = _adapters(be, ATTN_DIMS, which, seed + 7)
        assert be.ext.q_attn_set_loras(self.h, self.tables["q"], self.tables["k"], self.tables["v"], self.tables["o"]) == 20
        self.sin, self.cos = OM.rope_tables(MAXSEQ, HD, neox=True)

    def free(self):
        self.be.ext.free_q_attn(self.h)
        for v in self.hs.values():
            self.be.ext.free_q_matrix(v)


def _two_roundings(x, ref, pairs, c_in=None):
    """-> (fp16 the reference leaves, bar): base = fp16(c_in + x W), then the adapters"""
    base64 = x.astype(F64) @ ref + (0.0 if c_in is None else c_in.astype(F64))
    base16 = base64.astype(F16)
    if not pairs:
        return base16, half_tol(base64, x.shape[1])
    want, slack = lora_terms(x, base16, pairs)
    return want.astype(F16), half_tol(base64, x.shape[1]) + half_tol(want, x.shape[1]) + slack


def _check(got, want16, tol, what):
    err = np.abs(got.astype(F64) - want16.astype(F64))
    worst = float((err / tol).max())
    print(f"{what}: max err/tol = {worst:.3f}")
    assert got.shape == want16.shape and np.all(err <= tol), f"{what}: max err/tol {worst:.3f}"


@pytest.mark.parametrize("which", [("q", "v"), ("q", "k", "v", "o")], ids=["qv", "all"])
@pytest.mark.parametrize("gptq", [False, True], ids=["exl2", "gptq"])
def test_attention_with_adapters(be, gptq, which):
    at = Attn(be, gptq, False, which)
    sin, cos = be.t(at.sin), be.t(at.cos)
    for rows in ROWS:
        rng = np.random.default_rng(rows)
        past = 5
        x = rng.standard_normal((1, rows, HID)).astype(F16)
        q = torch.zeros((1, rows, NH * HD), dtype=torch.float16, device=be.device)
        k = torch.zeros((1, rows, NKV * HD), dtype=torch.float16, device=be.device)
        v = torch.zeros_like(k)
        be.ext.q_attn_forward_1(at.h, be.t(x), 1, rows, past, none_tensor, q, k, v, sin, cos, [21, 22], none_tensor)
        n = OM.rms_norm(x.reshape(rows, HID), at.nw, EPS)
        for name, heads, got in (("q", NH, q), ("k", NKV, k), ("v", NKV, v)):
            w16, tol = _two_roundings(n, at.refs[name], at.pairs[name])
            if name != "v":
                w16 = OM.rope_(w16.reshape(1, rows, heads, HD), at.sin, at.cos, np.array([past]), neox=True).reshape(rows, heads * HD)
                t4 = tol.reshape(rows, heads, 2, HD // 2)
                tol = (t4 + t4[:, :, ::-1]).reshape(rows, heads * HD) + half_tol(w16.astype(F64), HID)
            _check(be.n(got).reshape(rows, -1), w16, tol, f"{name} rows={rows}")
        # forward_2: x += a Wo, then o's adapters reading a
        a = rng.standard_normal((1, rows, NH * HD)).astype(F16)
        xt = be.t(x)
        be.ext.q_attn_forward_2(at.h, xt, be.t(a), 1, rows, [21, 22], none_tensor)
        w16, tol = _two_roundings(a.reshape(rows, -1), at.refs["o"], at.pairs["o"], c_in=x.reshape(rows, HID))
        _check(be.n(xt).reshape(rows, HID), w16, tol, f"o rows={rows}")
    at.free()


def test_attention_post_layernorm_and_empty_list(be):
    at = Attn(be, False, True, ("q", "k", "v", "o"))
    for rows in ROWS:
        rng = np.random.default_rng(100 + rows)
        x = rng.standard_normal((1, rows, HID)).astype(F16)
        a = rng.standard_normal((1, rows, NH * HD)).astype(F16)
        xt = be.t(x)
        be.ext.q_attn_forward_2(at.h, xt, be.t(a), 1, rows, [22, 21], none_tensor)
        a2 = a.reshape(rows, -1)
        t64 = a2.astype(F64) @ at.refs["o"]
        t16 = t64.astype(F16)
        tf = np.clip(t16.astype(F64), -65504, 65504)
        r = 1.0 / np.sqrt((tf ** 2).sum(-1, keepdims=True) / HID + EPS)
        n64 = tf * at.pw.astype(F64) * r
        x1 = OM.hadd(x.reshape(rows, HID), OM.rms_norm(t16, at.pw, EPS))
        want, slack = lora_terms(a2, x1, at.pairs["o"][::-1])
        tol = (half_tol(t64, NH * HD) * np.abs(at.pw.astype(F64)) * r + 2.0 ** -9 * np.abs(n64) + 2.0 ** -10 * np.abs(x1.astype(F64))
               + half_tol(want, NH * HD) + slack)
        _check(be.n(xt).reshape(rows, HID), want.astype(F16), tol, f"post-norm o rows={rows}")
        # an empty list: the existing entry point, bit for bit (python route and the C entry with n_loras = 0)
        outs = []
        for mode in ("plain", "empty", "c0"):
            xt, a_t = be.t(x), be.t(a)
            if mode == "c0":
                be.ext.lib.check(be.ext.lib.exl2_q_attn_forward_2_loras(at.h, xt.data_ptr(), a_t.data_ptr(), 1, rows, 0, None, be.ext._stream(xt)))
            else:
                be.ext.q_attn_forward_2(at.h, xt, a_t, 1, rows, *(([], none_tensor) if mode == "empty" else ()))
            outs.append(be.n(xt).copy())
        assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])
        assert not np.array_equal(outs[0].reshape(rows, HID), want.astype(F16))
    at.free()


class MLP:
    def __init__(self, be, gptq, gated, post, which, seed=60):
        self.be, self.gated = be, gated
        self.refs, self.hs, self.keep = {}, {}, []
        for i, (name, (k, n)) in enumerate(MLP_DIMS.items()):
            if name == "gate" and not gated: continue
            self.refs[name], self.hs[name], w = _lin(be, k, n, seed + i, gptq)
            self.keep.append(w)
        rng = np.random.default_rng(seed)
        self.nw = (1 + 0.1 * rng.standard_normal(HID)).astype(F16)
        self.pw = (1 + 0.1 * rng.standard_normal(HID)).astype(F16) if post else None
        z = lambda n: torch.zeros((MAXROWS, n), dtype=torch.float16, device=be.device)
        self.keep += [be.t(self.nw), z(HID), z(INTER), z(INTER), be.t(self.pw) if post else none_tensor]
        nwt, ts, ta, tb, pwt = self.keep[-5:]
        self.h = be.ext.make_q_mlp(nwt, none_tensor, True, EPS, self.hs.get("gate", 0), self.hs["up"], self.hs["down"], ts, ta, tb,
                                   none_tensor, MAXROWS, False, True, pwt, none_tensor, False, False)
        self.tables, self.pairs = _adapters(be, MLP_DIMS, which, seed + 7)
        be.ext.q_mlp_set_loras(self.h, self.tables["gate"], self.tables["up"], self.tables["down"])

    def want(self, x, ids_order):
        """-> (fp16 result, bar) for the adapters in the order listed"""
        rev = ids_order == [22, 21]
        P = {n: (p[::-1] if rev else p) for n, p in self.pairs.items()}
        n = OM.rms_norm(x, self.nw, EPS)
        u16, du = _two_roundings(n, self.refs["up"], P["up"])
        if self.gated:
            g16, dg = _two_roundings(n, self.refs["gate"], P["gate"])
            y = OM.silu_mul(g16, u16)
            g = g16.astype(F64)
            silu = g / (1.0 + np.exp(-g))
            dy = 1.1 * dg * np.abs(u16.astype(F64)) + np.abs(silu) * du + 2.0 ** -10 * np.abs(y.astype(F64)) + 1e-6
        else:
            u = u16.astype(F64)
            y = (u / (1.0 + np.exp(-u))).astype(F16)
            dy = 1.1 * du + 2.0 ** -11 * np.abs(y.astype(F64)) + 1e-6
        wd = np.abs(self.refs["down"])
        wl = sum((np.abs(a.astype(F64)) @ np.abs(b.astype(F64)) for a, b in P["down"]), np.zeros_like(wd))
        if self.pw is None:
            w16, tol = _two_roundings(y, self.refs["down"], P["down"], c_in=x)
            return w16, tol + dy @ (wd + wl)
        t64 = y.astype(F64) @ self.refs["down"]
        t16 = t64.astype(F16)
        tf = np.clip(t16.astype(F64), -65504, 65504)
        r = 1.0 / np.sqrt((tf ** 2).sum(-1, keepdims=True) / HID + EPS)
        n64 = tf * self.pw.astype(F64) * r
        x1 = OM.hadd(x, OM.rms_norm(t16, self.pw, EPS))
        want, slack = lora_terms(y, x1, P["down"])
        tol = ((half_tol(t64, INTER) + dy @ wd) * np.abs(self.pw.astype(F64)) * r + 2.0 ** -9 * np.abs(n64) + 2.0 ** -10 * np.abs(x1.astype(F64))
               + half_tol(want, INTER) + slack + dy @ wl)
        return want.astype(F16), tol

    def free(self):
        self.be.ext.free_q_mlp(self.h)
        for v in self.hs.values():
            self.be.ext.free_q_matrix(v)


@pytest.mark.parametrize("which", [("up",), ("gate", "up", "down")], ids=["up", "all"])
@pytest.mark.parametrize("gptq", [False, True], ids=["exl2", "gptq"])
@pytest.mark.parametrize("gated", [True, False], ids=["gated", "gateless"])
def test_mlp_with_adapters(be, gated, gptq, which):
    if not gated:
        which = tuple(n for n in which if n != "gate")
    m = MLP(be, gptq, gated, False, which)
    for rows in ROWS:
        x = np.random.default_rng(rows).standard_normal((rows, HID)).astype(F16)
        xt = be.t(x)
        be.ext.q_mlp_forward_(m.h, xt, [21, 22], none_tensor)
        w16, tol = m.want(x, [21, 22])
        _check(be.n(xt), w16, tol, f"mlp rows={rows}")
        plain = be.t(x)
        be.ext.q_mlp_forward_(m.h, plain)
        assert not np.array_equal(be.n(plain), be.n(xt))
        # an empty list: the existing entry point, bit for bit
        for mode in ("empty", "c0"):
            e = be.t(x)
            if mode == "c0":
                be.ext.lib.check(be.ext.lib.exl2_q_mlp_forward_loras(m.h, e.data_ptr(), rows, 0, None, be.ext._stream(e)))
            else:
                be.ext.q_mlp_forward_(m.h, e, [], none_tensor)
            assert np.array_equal(be.n(e), be.n(plain))
    m.free()


def test_mlp_post_layernorm(be):
    m = MLP(be, False, True, True, ("gate", "up", "down"))
    for rows in ROWS:
        x = np.random.default_rng(50 + rows).standard_normal((rows, HID)).astype(F16)
        xt = be.t(x)
        be.ext.q_mlp_forward_(m.h, xt, [22, 21], none_tensor)
        w16, tol = m.want(x, [22, 21])
        _check(be.n(xt), w16, tol, f"post-norm mlp rows={rows}")
    m.free()


def test_refusals(be):
    x = torch.zeros((1, HID), dtype=torch.float16, device=be.device)
    f32 = torch.zeros((1, 8), dtype=torch.float32, device=be.device)
    with pytest.raises(RuntimeError, match="MoE"):
        be.ext.q_moe_mlp_forward_(0, x, [1], none_tensor)
    with pytest.raises(RuntimeError, match="chained"):
        be.ext.q_attn_forward_1_chain(0, x, f32, 1, 1, x, x, x, loras=[1])
    with pytest.raises(RuntimeError, match="chained"):
        be.ext.q_attn_forward_2_chain(0, x, x, 1, None, None, x, f32, loras=[1])
    with pytest.raises(RuntimeError, match="chained"):
        be.ext.q_mlp_forward_chain(0, x, x, f32, 1, 1, None, None, x, f32, loras=[1])
    with pytest.raises(RuntimeError, match="chained"):
        be.ext.q_moe_mlp_forward_chain(0, x, 1, None, None, x, f32, loras=[1])
    # a handle made without scratch (tensor-parallel load) takes no adapters
    refs, hs, keep = {}, {}, []
    for i, (name, (k, n)) in enumerate(MLP_DIMS.items()):
        refs[name], hs[name], w = _lin(be, k, n, 80 + i, False)
        keep.append(w)
    nw = be.t(np.ones(HID, F16))
    h = be.ext.make_q_mlp(nw, none_tensor, True, EPS, hs["gate"], hs["up"], hs["down"], none_tensor, none_tensor, none_tensor,
                          none_tensor, MAXROWS, False, True, none_tensor, none_tensor, False, False)
    a, b = (be.t(t) for t in make_adapter(np.random.default_rng(0), HID, INTER, 8))
    with pytest.raises(RuntimeError, match="without scratch"):
        be.ext.q_mlp_set_loras(h, {}, {1: (a, b, 8)}, {})
    be.ext.free_q_mlp(h)
    for v in hs.values():
        be.ext.free_q_matrix(v)
