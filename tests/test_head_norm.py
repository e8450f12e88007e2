"""The q / k head norm (Qwen3-style attention): csrc/head_norm.hip at the op level, through q_attn_forward_1 and through the drop-in.

Reference: head_norm_kernel (head_norm.cu:9-141) as ext_norm.cpp:159-212 and q_attn.cu:285-289 call it.  Checker: the float64
restatement in tests/qk_norm_oracle.py, itself pinned against the reference's own ExLlamaV2HeadNorm.forward_torch
(tests/golden/reference_head_norm.npz).
"""
import os

import numpy as np
import pytest
import torch

from oracle import exl2 as OX
from oracle import modules as OM
from tests.qk_norm_oracle import head_norm as oracle_head_norm
from tests.util import exl2_to_torch, gptq_to_torch, half_tol
from exllamav2_amd.ext import none_tensor

F16 = np.float16
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_head_norm.npz")


def _u16(a):
    return np.ascontiguousarray(a).view(np.uint16)


def _check(got, y64, pre64=None):
    """half_tol against the unrounded float64 value; with a bias at |pre-bias| + |result| (the pre-bias rounding may flip one ulp)"""
    at = np.abs(y64) if pre64 is None else np.abs(pre64) + np.abs(y64)
    err = np.abs(got.astype(np.float64) - y64)
    assert np.all(np.isfinite(got.astype(np.float32)))
    assert np.all(err <= half_tol(at, got.shape[-1])), float((err / half_tol(at, got.shape[-1])).max())


# ---- the kernel against the oracle ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("rows", [1, 3, 17])
@pytest.mark.parametrize("heads", [1, 5])
@pytest.mark.parametrize("hd", [64, 96, 128, 256])
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("rms", [True, False])
def test_head_norm_matches_oracle(be, rms, bias, hd, heads, rows, inplace):
    rng = np.random.default_rng(hd * 1000 + heads * 100 + rows * 4 + 2 * int(rms) + int(bias))
    x = (rng.standard_normal((rows, heads, hd)) * rng.uniform(0.2, 3.0, size=(rows, heads, 1)) + 0.3).astype(F16)
    w = (1 + 0.1 * rng.standard_normal((heads, hd))).astype(F16)
    b = (0.2 * rng.standard_normal((heads, hd))).astype(F16) if bias else None
    xt, wt = be.t(x), be.t(w)
    bt = be.t(b) if bias else none_tensor
    if inplace:
        be.ext.head_norm_(xt, wt, bt, 1e-6, rms)
        got = be.n(xt)
    else:
        yt = torch.zeros_like(xt)
        be.ext.head_norm(xt, wt, bt, yt, 1e-6, rms)
        got = be.n(yt)
        assert np.array_equal(_u16(be.n(xt)), _u16(x))
    pre64, _ = oracle_head_norm(x, w, None, 1e-6, rms)
    y64, _ = oracle_head_norm(x, w, b, 1e-6, rms)
    _check(got, y64, pre64 if bias else None)


@pytest.mark.parametrize("hd", [64, 96, 256])
@pytest.mark.parametrize("rms", [True, False])
def test_head_norm_edge_rows(be, rms, hd):
    """a row of +inf / -inf / 65504 entries is clamped like the reference clamps it (finite result); an all-zero row stays zero"""
    rng = np.random.default_rng(5 + hd)
    heads = 3
    x = rng.standard_normal((3, heads, hd)).astype(F16)
    x[0, :, 0::3] = np.inf; x[0, :, 1::3] = -np.inf; x[0, :, 2::3] = 65504.0
    x[0, 1, :7] = 1.0
    x[1] = 0.0
    w = (1 + 0.1 * rng.standard_normal((heads, hd))).astype(F16)
    xt = be.t(x)
    be.ext.head_norm_(xt, be.t(w), none_tensor, 1e-5, rms)
    got = be.n(xt)
    y64, y16 = oracle_head_norm(x, w, None, 1e-5, rms)
    assert np.all(np.isfinite(y16.astype(np.float32)))
    _check(got, y64)
    assert np.all(got[1] == 0.0)


def test_head_norm_argument_checks(be):
    x = torch.zeros((2, 3, 64), dtype=torch.float16, device=be.device)
    w = torch.ones((3, 64), dtype=torch.float16, device=be.device)
    with pytest.raises(RuntimeError, match="must be half"):
        be.ext.head_norm(x.float(), w, none_tensor, x, 1e-5, True)
    with pytest.raises(RuntimeError, match="incompatible shapes"):
        be.ext.head_norm(x, w[:2], none_tensor, x, 1e-5, True)
    with pytest.raises(RuntimeError, match="incompatible shapes"):
        be.ext.head_norm(x, w, w[:, :32].contiguous(), x, 1e-5, True)
    x2 = torch.zeros((2, 3, 260), dtype=torch.float16, device=be.device)
    with pytest.raises(RuntimeError, match="head_dim"):
        be.ext.head_norm_(x2, torch.ones((3, 260), dtype=torch.float16, device=be.device), none_tensor, 1e-5, True)


# ---- the oracle and the device against the reference's own forward_torch ---------------------------------------------------------

def _golden_cases():
    g = np.load(GOLDEN)
    n = int(g["n_cases"])
    return [dict(x=g[f"x_{i}"], w=g[f"w_{i}"], y=g[f"y_{i}"], eps=float(g[f"eps_{i}"]), rms=bool(g[f"rms_{i}"])) for i in range(n)]


def test_oracle_matches_reference_forward_torch():
    cases = _golden_cases()
    assert len(cases) == 12 and {c["x"].shape[-1] for c in cases} == {64, 128, 256} and {c["rms"] for c in cases} == {True, False}
    for c in cases:
        y64, y16 = oracle_head_norm(c["x"], c["w"], None, c["eps"], c["rms"])
        assert np.all(np.abs(c["y"].astype(np.float64) - y64) <= half_tol(y64, c["x"].shape[-1]))


def test_device_matches_reference_forward_torch(be):
    for c in _golden_cases():
        xt = be.t(c["x"])
        be.ext.head_norm_(xt, be.t(c["w"]), none_tensor, c["eps"], c["rms"])
        want = c["y"].astype(np.float64)
        # two fp16 roundings of the same value (the reference multiplies in torch's order): one fp16 ulp apart at the most, and an
        # ulp is at most 2^-10 of the value -- half_tol's relative term
        assert np.all(np.abs(be.n(xt).astype(np.float64) - want) <= half_tol(want, c["x"].shape[-1]))


# ---- the q + k launch and the norm + RoPE launch: bit for bit the launches they replace ------------------------------------------

def _qk(rng, b, s, nh, kvh, hd):
    q = (rng.standard_normal((b, s, nh, hd)) * 1.5).astype(F16)
    k = (rng.standard_normal((b, s, kvh, hd)) * 0.7 + 0.1).astype(F16)
    qn = (1 + 0.1 * rng.standard_normal((nh, hd))).astype(F16)
    kn = (1 + 0.1 * rng.standard_normal((kvh, hd))).astype(F16)
    return q, k, qn, kn


@pytest.mark.parametrize("rms", [True, False])
@pytest.mark.parametrize("b,s,nh,kvh,hd", [(1, 1, 4, 2, 64), (3, 2, 5, 1, 96), (2, 3, 8, 2, 128), (1, 5, 3, 3, 256)])
def test_qk_launch_equals_two_head_norm_calls(be, rms, b, s, nh, kvh, hd):
    rng = np.random.default_rng(b * 100 + hd)
    q, k, qn, kn = _qk(rng, b, s, nh, kvh, hd)
    q1, k1, q2, k2 = be.t(q), be.t(k), be.t(q), be.t(k)
    qnt, knt = be.t(qn), be.t(kn)
    be.ext.head_norm_qk(q1, k1, qnt, knt, 1e-6, rms)
    be.ext.head_norm_(q2, qnt, none_tensor, 1e-6, rms)
    be.ext.head_norm_(k2, knt, none_tensor, 1e-6, rms)
    assert np.array_equal(_u16(be.n(q1)), _u16(be.n(q2))) and np.array_equal(_u16(be.n(k1)), _u16(be.n(k2)))
    assert not np.array_equal(_u16(be.n(q1)), _u16(q))


@pytest.mark.parametrize("rms", [True, False])
@pytest.mark.parametrize("neox", [True, False])
@pytest.mark.parametrize("positions", ["past_len", "past_lens", "past_lens_only"])
@pytest.mark.parametrize("nh,kvh,hd,rot", [(4, 2, 64, 64), (5, 1, 96, 64), (2, 2, 128, 128), (2, 1, 256, 256), (3, 1, 64, 40)])
def test_norm_rope_launch_equals_head_norm_then_rope(be, rms, neox, positions, nh, kvh, hd, rot):
    """rot = sincos_size (a partial rotary width; 40 is no multiple of 16: the entry point then runs its two launches)"""
    b, s, max_seq = 3, 2, 64
    rng = np.random.default_rng(nh * 1000 + hd + rot)
    q, k, qn, kn = _qk(rng, b, s, nh, kvh, hd)
    sin, cos = OM.rope_tables(max_seq, rot, neox=neox)
    sint, cost = be.t(sin), be.t(cos)
    offs = be.t(np.array([0, 17, 30], dtype=np.int32))
    past, off = {"past_len": (5, none_tensor), "past_lens": (4, offs), "past_lens_only": (-1, offs)}[positions]
    q1, k1, q2, k2 = be.t(q), be.t(k), be.t(q), be.t(k)
    qnt, knt = be.t(qn), be.t(kn)
    be.ext.head_norm_qk(q1, k1, qnt, knt, 1e-6, rms, sin=sint, cos=cost, past_len=past, offsets=off, neox_style=neox)
    be.ext.head_norm_(q2, qnt, none_tensor, 1e-6, rms)
    be.ext.head_norm_(k2, knt, none_tensor, 1e-6, rms)
    unrot = be.n(q2).copy()
    be.ext.rope_(q2, sint, cost, past, nh, hd, off, neox)
    be.ext.rope_(k2, sint, cost, past, kvh, hd, off, neox)
    assert np.array_equal(_u16(be.n(q1)), _u16(be.n(q2))) and np.array_equal(_u16(be.n(k1)), _u16(be.n(k2)))
    assert not np.array_equal(_u16(be.n(q2)), _u16(unrot))


# ---- q_attn_forward_1 with norms against the oracle composition linear -> fp16 -> head_norm -> rope ------------------------------

HID, NH, NKV, HD, MAXSEQ = 256, 4, 2, 64, 64


def _make_attn(be, kind: str, rms: bool, make_q_attn=None):
    refs, hs, owned = {}, {}, []
    shared = None
    for i, (name, k, n) in enumerate((("q", HID, NH * HD), ("k", HID, NKV * HD), ("v", HID, NKV * HD), ("o", NH * HD, HID))):
        if kind == "exl2":
            t = OX.synth_exl2(k, n, [(5, 32, 32), (4, 32, k - 32)], seed=140 + i, act_order=True, sigma=0.06)
            if name == "q": shared = t["q_invperm"]
            if name in ("k", "v"): t["q_invperm"] = shared.copy()      # one Hessian for q / k / v: one permutation (chain-capable)
            refs[name] = OX.exl2_reconstruct(t)
            w = exl2_to_torch(be, t)
        else:
            t = OX.synth_gptq(k, n, 64, seed=240 + i, act_order=False)
            refs[name] = OX.gptq_reconstruct(t)
            w = gptq_to_torch(be, t)
        hs[name] = be.ext.make_q_matrix_from_dict(w, None)
        owned.append(w)
    rng = np.random.default_rng(7)
    nw = (1 + 0.1 * rng.standard_normal(HID)).astype(F16)
    qn = (1 + 0.1 * rng.standard_normal((NH, HD))).astype(F16)
    kn = (1 + 0.1 * rng.standard_normal((NKV, HD))).astype(F16)
    temp_state = torch.zeros((64, HID), dtype=torch.float16, device=be.device)
    keep = (be.t(nw), be.t(qn), be.t(kn), temp_state, owned)
    h = (make_q_attn or be.ext.make_q_attn)(keep[0], none_tensor, True, rms, 1e-6, hs["q"], hs["k"], hs["v"], hs["o"], temp_state, none_tensor,
                           64, HID, NH, NKV, HD, MAXSEQ, True, 2, HD, keep[1], keep[2], none_tensor, none_tensor, False, False)
    sin, cos = OM.rope_tables(MAXSEQ, HD, neox=True)
    return dict(h=h, hs=hs, refs=refs, nw=nw, qn=qn, kn=kn, rms=rms, sin=sin, cos=cos, keep=keep)


def _free_attn(be, a):
    be.ext.free_q_attn(a["h"])
    for v in a["hs"].values():
        be.ext.free_q_matrix(v)


@pytest.fixture(params=[("exl2", True), ("gptq", True), ("exl2", False)], ids=["exl2-rms", "gptq-rms", "exl2-layernorm"])
def attn(be, request):
    a = _make_attn(be, *request.param)
    yield a
    _free_attn(be, a)


def _want(a, x, positions, rope: bool):
    """(q, k, v) fp16 as the oracle composes them + the float64 values the tolerance is taken at (before the rotation)"""
    b, s, _ = x.shape
    n = OM.rms_norm(x.reshape(b * s, HID), a["nw"], 1e-6)
    lin = {name: OX.gemm_ref(n, a["refs"][name], exact=True).reshape(b, s, heads, HD) for name, heads in (("q", NH), ("k", NKV), ("v", NKV))}
    q64, q = oracle_head_norm(lin["q"].astype(F16), a["qn"], None, 1e-6, a["rms"])
    k64, k = oracle_head_norm(lin["k"].astype(F16), a["kn"], None, 1e-6, a["rms"])
    if rope:
        q = OM.rope_(q, a["sin"], a["cos"], positions, neox=True)
        k = OM.rope_(k, a["sin"], a["cos"], positions, neox=True)
    return (q, k, lin["v"].astype(F16)), (q64, k64, lin["v"])


def _close(got, want16, exact64):
    """tests/test_qattn_op.py's bound: the q_gemm tolerance x 3 (the projection may land one ulp off, norm and rotation carry it on)"""
    err = np.abs(got.astype(np.float64) - want16.astype(np.float64))
    return np.all(err <= 3 * half_tol(exact64, HID))


@pytest.mark.parametrize("apply_rope", [True, False])
@pytest.mark.parametrize("b,q_len", [(1, 1), (3, 1), (1, 20)])
def test_forward_1_with_head_norm(be, attn, apply_rope, b, q_len):
    """rows 1 and 3: the decode kernels; 20: the prefill pre-pass"""
    rng = np.random.default_rng(31 + b + q_len)
    past = 4
    offs = np.arange(b, dtype=np.int32) * 7
    x = rng.standard_normal((b, q_len, HID)).astype(F16)
    q = torch.zeros((b, q_len, NH, HD), dtype=torch.float16, device=be.device)
    k = torch.zeros((b, q_len, NKV, HD), dtype=torch.float16, device=be.device)
    v = torch.zeros_like(k)
    be.ext.q_attn_forward_1(attn["h"], be.t(x), b, q_len, past, be.t(offs), q, k, v, be.t(attn["sin"]), be.t(attn["cos"]),
                            apply_rope=apply_rope)
    (wq, wk, wv), (eq, ek, ev) = _want(attn, x, offs + past, apply_rope)
    assert _close(be.n(q), wq, eq) and _close(be.n(k), wk, ek) and _close(be.n(v), wv, ev)
    # the norm really happened: the plain projections are far away
    plain, _ = _want(dict(attn, qn=np.ones_like(attn["qn"]), kn=np.ones_like(attn["kn"])), x, offs + past, apply_rope)
    assert not _close(be.n(q), plain[0], eq)


@pytest.mark.parametrize("variant", ["chain", "chain_skip", "chain_rope"])
@pytest.mark.parametrize("rows", [1, 3])
def test_forward_1_chain_with_head_norm(be, attn, variant, rows):
    """the chain entries fed from publish_rows: normalised q / k (rotated by chain_rope), un-normalised with skip_head_norm"""
    ext = be.ext
    cap, in_inv, _, nw_perm = ext.q_attn_chain_info(attn["h"])
    assert cap
    qn_ptr, kn_ptr, eps, rms = ext.q_attn_head_norm_info(attn["h"])
    assert qn_ptr == attn["keep"][1].data_ptr() and kn_ptr == attn["keep"][2].data_ptr() and rms == attn["rms"] and abs(eps - 1e-6) < 1e-12
    rng = np.random.default_rng(77 + rows)
    x = rng.standard_normal((rows, 1, HID)).astype(F16)
    xt = be.t(x).view(rows, HID)
    xp = torch.zeros_like(xt)
    ss = torch.zeros((rows,), dtype=torch.float32, device=be.device)
    ext.publish_rows(xt, rows, HID, in_inv, nw_perm, xp, ss)
    q = torch.zeros((rows, 1, NH, HD), dtype=torch.float16, device=be.device)
    k = torch.zeros((rows, 1, NKV, HD), dtype=torch.float16, device=be.device)
    v = torch.zeros_like(k)
    past = 6
    if variant == "chain_rope":
        ext.q_attn_forward_1_chain_rope(attn["h"], xp, ss, 1, rows, 1, past, none_tensor, q, k, v, be.t(attn["sin"]), be.t(attn["cos"]))
    else:
        ext.q_attn_forward_1_chain(attn["h"], xp, ss, 1, rows, q, k, v, skip_head_norm=variant == "chain_skip")
    a = dict(attn, qn=np.ones_like(attn["qn"]), kn=np.ones_like(attn["kn"])) if variant == "chain_skip" else attn
    (wq, wk, wv), (eq, ek, ev) = _want(a, x, np.full((rows,), past), variant == "chain_rope")
    if variant == "chain_skip":
        n = OM.rms_norm(x.reshape(rows, HID), attn["nw"], 1e-6)
        eq = OX.gemm_ref(n, attn["refs"]["q"], exact=True).reshape(rows, 1, NH, HD)
        ek = OX.gemm_ref(n, attn["refs"]["k"], exact=True).reshape(rows, 1, NKV, HD)
        wq, wk = eq.astype(F16), ek.astype(F16)
    assert _close(be.n(q), wq, eq) and _close(be.n(k), wk, ek) and _close(be.n(v), wv, ev)


def test_make_q_attn_wants_both_norms(be):
    a = _make_attn(be, "exl2", True)
    try:
        hs, keep = a["hs"], a["keep"]
        with pytest.raises(RuntimeError, match="come together"):
            be.ext.make_q_attn(keep[0], none_tensor, True, True, 1e-6, hs["q"], hs["k"], hs["v"], hs["o"], keep[3], none_tensor,
                               64, HID, NH, NKV, HD, MAXSEQ, True, 2, HD, keep[1], none_tensor, none_tensor, none_tensor, False, False)
    finally:
        _free_attn(be, a)


# ---- the drop-in: exllamav2_ext.head_norm / head_norm_ / make_q_attn(... q_norm, k_norm ...) in the reference's argument order ---

def _load_dropin(be, monkeypatch, route: str):
    """a fresh copy of dropin/exllamav2_ext.py bound to the backend under test: per-token calls on the ctypes route
    (EXL2_DROPIN_FAST=0) or on the compiled binding (dropin/_exl2_fast.cpp)"""
    import importlib.util
    import exllamav2_amd.ext as host_ext
    from exllamav2_amd import _lib, build
    from tests.conftest import ROOT, build_emu_if_needed
    monkeypatch.setattr(host_ext, "ext_c", be.ext)
    monkeypatch.setenv("EXL2_DROPIN_FAST", "0" if route == "ctypes" else "1")
    if route == "compiled":
        build.build_fast()
    spec = importlib.util.spec_from_file_location(f"exllamav2_ext_{route}_{be.name}", os.path.join(ROOT, "dropin", "exllamav2_ext.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert (mod._fast is not None) == (route == "compiled")
    if route == "compiled":
        mod._fast.init(build_emu_if_needed() if be.is_emu else _lib.HIP_LIB_PATH, be.is_emu)
    return mod


@pytest.mark.parametrize("route", ["ctypes", "compiled"])
def test_dropin_head_norm(be, monkeypatch, route):
    E = _load_dropin(be, monkeypatch, route)
    rng = np.random.default_rng(3)
    x = (rng.standard_normal((2, 3, 5, 128)) * 2).astype(F16)                # [b, s, heads, hd] as attn.py hands it over
    w = (1 + 0.1 * rng.standard_normal((5, 128))).astype(F16)
    b = (0.1 * rng.standard_normal((5, 128))).astype(F16)
    for rms in (True, False):
        for bias in (None, b):
            y64, _ = oracle_head_norm(x, w, bias, 1e-6, rms)
            pre64, _ = oracle_head_norm(x, w, None, 1e-6, rms)
            xt, yt = be.t(x), torch.zeros((2, 3, 5, 128), dtype=torch.float16, device=be.device)
            E.head_norm(xt, be.t(w), none_tensor if bias is None else be.t(bias), yt, 1e-6, rms)
            _check(be.n(yt), y64, None if bias is None else pre64)
            E.head_norm_(xt, be.t(w), none_tensor if bias is None else be.t(bias), 1e-6, rms)
            assert np.array_equal(_u16(be.n(xt)), _u16(be.n(yt)))


@pytest.mark.parametrize("route", ["ctypes", "compiled"])
def test_dropin_q_attn_with_head_norm(be, monkeypatch, route):
    """make_q_attn with q_norm / k_norm, then q_attn_forward_1 as attn.py:1128-1141 calls it -- twice: on the compiled route the second
    call of a module may run from a published hand-off (dropin/_exl2_fast.cpp)"""
    E = _load_dropin(be, monkeypatch, route)
    a = _make_attn(be, "exl2", True, make_q_attn=E.make_q_attn)
    try:
        sin, cos = be.t(a["sin"]), be.t(a["cos"])
        for step, past in enumerate((3, 4)):
            rng = np.random.default_rng(50 + step)
            x = rng.standard_normal((1, 1, HID)).astype(F16)
            q = torch.zeros((1, 1, NH * HD), dtype=torch.float16, device=be.device)
            k = torch.zeros((1, 1, NKV * HD), dtype=torch.float16, device=be.device)
            v = torch.zeros_like(k)
            E.q_attn_forward_1(a["h"], be.t(x), 1, 1, past, none_tensor, q, k, v, sin, cos, [], none_tensor)
            (wq, wk, wv), (eq, ek, ev) = _want(a, x, np.array([past]), True)
            assert _close(be.n(q).reshape(1, 1, NH, HD), wq, eq) and _close(be.n(k).reshape(1, 1, NKV, HD), wk, ek)
            assert _close(be.n(v).reshape(1, 1, NKV, HD), wv, ev)
    finally:
        if route == "compiled":
            E._fast.forget_module(a["h"])
        _free_attn(be, a)
