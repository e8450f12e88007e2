"""Q6 and Q8 KV caches (ExLlamaV2Cache_Q6 / _Q8: reference cache.py:609-656, cache.cu:259-276 -- Q6 = 8-bit keys + 4-bit values,
Q8 = 8-bit both) on the kernels that serve the Q4 cache: attention straight from the codes (csrc/attn_q4.hip at the code widths
(8, 4) and (8, 8)), the one- and two-launch decode step, the chained decode step.

Checkers: the numpy oracle's attention over q8_unpack / q4_unpack of the SAME codes (op level, the bar of the Q4 tests in
tests/test_ops.py), the codec itself (rope_kv_append + fp16_to_q_kv: bit-exact against the reference's kernels in tests/test_ops.py)
for what a step writes, and OracleModelQ below -- OracleModel.forward(q4_cache=True) with the 8-bit sides going through q8_pack /
q8_unpack -- at model level."""
import copy
import os

import numpy as np
import pytest
import torch

from exllamav2_amd.cache import ExLlamaV2Cache, ExLlamaV2Cache_Q4, ExLlamaV2Cache_Q6, ExLlamaV2Cache_Q8
from exllamav2_amd.model import ExLlamaV2, GreedyGraphDecoder
from exllamav2_amd.synth import synth_checkpoint
from oracle.model import OracleModel
from oracle import modules as OM
from tests.test_model import LOGIT_TOL, tiny_cfg, check_logits, confident

F16 = np.float16
CACHES = {4: ExLlamaV2Cache_Q4, 6: ExLlamaV2Cache_Q6, 8: ExLlamaV2Cache_Q8}


def _bits(wbits):
    """(key bits, value bits) of a cache width"""
    return {4: (4, 4), 6: (8, 4), 8: (8, 8)}[wbits]


def _pack(x, bits):
    return OM.q8_pack(x) if bits == 8 else OM.q4_pack(x)


def _unpack(codes, scales, bits):
    return OM.q8_unpack(codes, scales) if bits == 8 else OM.q4_unpack(codes, scales)


def _attn_tol(want):
    """the bar of tests/test_ops.py's attention-from-Q4 tests (its _attn_tol + 2e-3): |want| * 2^-9 + 2e-3 + 2e-3"""
    return np.abs(want.astype(np.float32)) * 2.0 ** -9 + 2e-3 + 2e-3


def _close(got, want, what):
    err = np.abs(got.astype(np.float32) - want.astype(np.float32))
    print(what, "worst error / bar:", float((err / _attn_tol(want)).max()))
    assert np.all(err <= _attn_tol(want)), (what, float(err.max()))


def _scratch(be, rows, hd):
    return torch.zeros((be.ext.paged_attn_scratch_bytes(rows, hd, 16) // 4 + 1,), dtype=torch.float32, device=be.device)


class _Codes:
    """a random quantized cache of `shape` + (kvh, hd): oracle-packed codes / scales per side, their unpacked values, device copies"""

    def __init__(self, be, rng, shape, kvh, hd, wbits):
        self.be, self.shape, self.kvh, self.hd = be, tuple(shape), kvh, hd
        self.kb, self.vb = _bits(wbits)
        kf = rng.standard_normal(self.shape + (kvh, hd)).astype(F16)
        vf = rng.standard_normal(self.shape + (kvh, hd)).astype(F16)
        self.kq, self.ks = _pack(kf.reshape(-1), self.kb)
        self.vq, self.vs = _pack(vf.reshape(-1), self.vb)
        self.k_un = _unpack(self.kq, self.ks, self.kb).reshape(self.shape + (kvh, hd))
        self.v_un = _unpack(self.vq, self.vs, self.vb).reshape(self.shape + (kvh, hd))

    def host(self):
        s, kvh, hd = self.shape, self.kvh, self.hd
        return [self.kq.reshape(s + (kvh, hd * self.kb // 8)), self.ks.reshape(s + (kvh, hd // 32)),
                self.vq.reshape(s + (kvh, hd * self.vb // 8)), self.vs.reshape(s + (kvh, hd // 32))]

    def dev(self, view_pages=0):
        ts = [self.be.t(x) for x in self.host()]
        if view_pages:
            ts = [t.view(-1, view_pages, self.kvh, t.shape[-1]) for t in ts]
        return ts


# ---- 1. attention from the codes == attention over the unpacked cache ------------------------------------------------------------

@pytest.mark.parametrize("wbits", [6, 8])
@pytest.mark.parametrize("hd,nh,kvh,s,paged", [(128, 4, 4, 1, False), (128, 8, 2, 1, True), (64, 8, 8, 2, False), (256, 2, 2, 1, True)])
def test_attention_from_q68_cache(be, wbits, hd, nh, kvh, s, paged):
    """test_attention_from_q4_cache's shapes at 6 and 8 bits: one split and several, paged and contiguous."""
    rng = np.random.default_rng(40)
    b, T = 2, 512
    total = np.array([300, 511], dtype=np.int32)
    c = _Codes(be, rng, (b, T), kvh, hd, wbits)
    q = rng.standard_normal((b, s, nh, hd)).astype(F16)
    want = np.stack([OM.attention(q[i:i + 1], c.k_un[i:i + 1, :total[i]], c.v_un[i:i + 1, :total[i]])[0] for i in range(b)])
    scratch = _scratch(be, b * s * nh, hd)
    seq = be.t(total - s)
    for nsplit in (1, 3):
        out = torch.zeros((b, s, nh, hd), dtype=torch.float16, device=be.device)
        table = be.t(np.array([[0, 1], [2, 3]], dtype=np.int32)) if paged else None
        assert be.ext.paged_attn_q(be.t(q), *c.dev(256 if paged else 0), out, seq, table, wbits, len_const=0, len_offset=s,
                                   nsplit=nsplit, scratch=scratch)
        _close(be.n(out), want, ("from codes", wbits, hd, nsplit))


@pytest.mark.parametrize("wbits", [6, 8])
@pytest.mark.parametrize("hd,nh,kvh,s", [(128, 4, 4, 1), (128, 8, 2, 3), (64, 4, 4, 2), (256, 2, 1, 1)])
def test_attention_from_q68_cache_with_fp16_new_tokens(be, wbits, hd, nh, kvh, s):
    """keys below total - s from the codes, the step's own s keys / values from k_new / v_new in fp16"""
    rng = np.random.default_rng(41)
    b, T = 2, 256
    total = np.array([77, 256], dtype=np.int32)
    c = _Codes(be, rng, (b, T), kvh, hd, wbits)
    kn = rng.standard_normal((b, s, kvh, hd)).astype(F16)
    vn = rng.standard_normal((b, s, kvh, hd)).astype(F16)
    q = rng.standard_normal((b, s, nh, hd)).astype(F16)
    want = []
    for i in range(b):
        kk = np.concatenate([c.k_un[i, :total[i] - s], kn[i]])[None]
        vv = np.concatenate([c.v_un[i, :total[i] - s], vn[i]])[None]
        want.append(OM.attention(q[i:i + 1], kk, vv)[0])
    want = np.stack(want)
    scratch = _scratch(be, b * s * nh, hd)
    for nsplit in (1, 2):
        out = torch.zeros((b, s, nh, hd), dtype=torch.float16, device=be.device)
        assert be.ext.paged_attn_q(be.t(q), *c.dev(), out, be.t(total - s), None, wbits, len_const=0, len_offset=s, nsplit=nsplit,
                                   scratch=scratch, k_new=be.t(kn), v_new=be.t(vn))
        _close(be.n(out), want, ("fp16 new tokens", wbits, hd, nsplit))


@pytest.mark.parametrize("wbits", [6, 8])
@pytest.mark.parametrize("hd,nh,kvh,s,paged", [(128, 4, 4, 1, True), (64, 8, 8, 1, False), (128, 8, 2, 2, True)])
def test_attention_from_q68_cache_in_consumer_order(be, wbits, hd, nh, kvh, s, paged):
    """out_invperm: feature n of a token row lands at out[row, out_invperm[n]] (the chained decode step's form)"""
    rng = np.random.default_rng(43)
    b, T = 2, 512
    total = np.array([130, 400], dtype=np.int32)
    c = _Codes(be, rng, (b, T), kvh, hd, wbits)
    kn = rng.standard_normal((b, s, kvh, hd)).astype(F16); vn = rng.standard_normal((b, s, kvh, hd)).astype(F16)
    q = rng.standard_normal((b, s, nh, hd)).astype(F16)
    want = []
    for i in range(b):
        kk = np.concatenate([c.k_un[i, :total[i] - s], kn[i]])[None]; vv = np.concatenate([c.v_un[i, :total[i] - s], vn[i]])[None]
        want.append(OM.attention(q[i:i + 1], kk, vv)[0])
    want = np.stack(want).reshape(b * s, nh * hd)
    invperm = rng.permutation(nh * hd).astype(np.uint16)
    want_p = np.zeros_like(want); want_p[:, invperm] = want
    inv_t = be.t(invperm.view(np.int16))
    scratch = _scratch(be, b * s * nh, hd)
    table = be.t(np.array([[0, 1], [2, 3]], dtype=np.int32)) if paged else None
    for nsplit in (1, 3):
        out = torch.zeros((b, s, nh, hd), dtype=torch.float16, device=be.device)
        assert be.ext.paged_attn_q(be.t(q), *c.dev(256 if paged else 0), out, be.t(total - s), table, wbits, len_const=0, len_offset=s,
                                   nsplit=nsplit, scratch=scratch, k_new=be.t(kn), v_new=be.t(vn), out_invperm=inv_t.data_ptr())
        _close(be.n(out).reshape(b * s, nh * hd), want_p, ("consumer order", wbits, hd, nsplit))


# ---- 2. ticket merge == combine launch -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("wbits", [6, 8])
@pytest.mark.parametrize("hd,nh,kvh,s", [(128, 8, 2, 1), (128, 16, 2, 1), (64, 4, 4, 3)])
def test_attention_from_q68_cache_merges_its_splits_in_the_launch(be, wbits, hd, nh, kvh, s, monkeypatch):
    """with tickets the last split to finish merges inside the launch: bit-identical to attention + combine launch, tickets left at
    zero -- also for a sequence short enough for ONE split (40 keys) on a grid sized for many"""
    monkeypatch.setenv("EXL2_Q4_RB", "4")
    rng = np.random.default_rng(47)
    b, T = 3, 2048
    total = np.array([1500, 40, 700], dtype=np.int32)
    c = _Codes(be, rng, (b, T), kvh, hd, wbits)
    kn = rng.standard_normal((b, s, kvh, hd)).astype(F16); vn = rng.standard_normal((b, s, kvh, hd)).astype(F16)
    q = rng.standard_normal((b, s, nh, hd)).astype(F16)
    scratch = _scratch(be, b * s * nh, hd)
    counters = torch.zeros((256,), dtype=torch.int32, device=be.device)
    args = (be.t(q), *c.dev())
    for nsplit in (1, 4, 7):
        outs = []
        for cnt in (None, counters):
            out = torch.zeros((b, s, nh, hd), dtype=torch.float16, device=be.device)
            assert be.ext.paged_attn_q(*args, out, be.t(total - s), None, wbits, len_const=0, len_offset=s, nsplit=nsplit, scratch=scratch,
                                       k_new=be.t(kn), v_new=be.t(vn), counters=cnt)
            outs.append(be.n(out))
        assert np.array_equal(outs[0].view(np.uint16), outs[1].view(np.uint16)), nsplit
        assert int(be.n(counters).astype(np.int64).sum()) == 0
    # too few tickets: the two-launch form runs (same result as without any)
    res = []
    for cnt in (None, counters[:1]):
        out = torch.zeros((b, s, nh, hd), dtype=torch.float16, device=be.device)
        assert be.ext.paged_attn_q(*args, out, be.t(total - s), None, wbits, len_const=0, len_offset=s, nsplit=4, scratch=scratch,
                                   k_new=be.t(kn), v_new=be.t(vn), counters=cnt)
        res.append(be.n(out))
    assert np.array_equal(res[0].view(np.uint16), res[1].view(np.uint16))


# ---- 3. the one-launch and the two-launch step write exactly the codec's codes -----------------------------------------------------

def _decode_step_case(be, monkeypatch, wbits, hd, nh, kvh, b, s, paged, style, rb, past, pages_per_seq, nsplit, rng):
    """One decode step three ways on the same inputs -- the codec (rope_kv_append into fp16 staging + fp16_to_q_kv(wbits)), the
    two-launch form (head_dim 128; declined at 64) and the one-launch form: codes and scales of the WHOLE cache bit-identical (the
    step's positions = the codec's bytes, everything else = what was there), q / k_new handling, tickets, attention output at the bar."""
    monkeypatch.setenv("EXL2_Q4_RB", str(rb))
    ps = 256
    T = ps * pages_per_seq
    table = rng.permutation(b * pages_per_seq).astype(np.int32).reshape(b, pages_per_seq)
    shape = (b * pages_per_seq, ps) if paged else (b, T)
    c = _Codes(be, rng, shape, kvh, hd, wbits)
    q = rng.standard_normal((b, s, nh, hd)).astype(F16)
    kn = rng.standard_normal((b, s, kvh, hd)).astype(F16); vn = rng.standard_normal((b, s, kvh, hd)).astype(F16)
    neox = style == 2
    sin, cos = OM.rope_tables(T + 8, hd, neox=neox)
    sint, cost = (be.t(sin), be.t(cos)) if style else (None, None)
    scratch = _scratch(be, b * s * nh, hd)
    counters = torch.zeros((b * s * nh + 8,), dtype=torch.int32, device=be.device)
    sl, bt = be.t(past), (be.t(table) if paged else None)
    what = (wbits, hd, b, s, nh, kvh, paged, style, rb, past.tolist(), nsplit)
    # the codec
    c0 = c.dev()
    kc = torch.zeros(shape + (kvh, hd), dtype=torch.float16, device=be.device); vc = torch.zeros_like(kc)
    q0, k0 = be.t(q), be.t(kn)
    be.ext.rope_kv_append(q0, k0, be.t(vn), kc, vc, sint, cost, 0, sl, bt, style)
    if paged:
        be.ext.fp16_to_q_kv(kc, c0[0], c0[1], vc, c0[2], c0[3], b, 0, s, ps, sl, bt, wbits)
    else:
        for i in range(b):
            be.ext.fp16_to_q_kv(kc[i:i + 1], c0[0][i:i + 1], c0[1][i:i + 1], vc[i:i + 1], c0[2][i:i + 1], c0[3][i:i + 1], 1, int(past[i]), s, 0,
                                None, None, wbits)
    want_codes = [be.n(x) for x in c0]
    # ... touched exactly the step's positions
    touched = np.zeros(shape, dtype=bool)
    for i in range(b):
        for j in range(s):
            pos = int(past[i]) + j
            touched[(table[i, pos // ps], pos % ps) if paged else (i, pos)] = True
    for w, h in zip(want_codes, c.host()):
        assert np.array_equal(w[~touched].view(np.uint8), h[~touched].view(np.uint8)), what
    assert not np.array_equal(want_codes[0][touched], c.host()[0][touched])
    # two launches
    c2 = c.dev()
    q2, k2 = be.t(q), be.t(kn)
    two = be.ext.rope_quant_append_q(q2, k2, be.t(vn), *c2, sint, cost, 0, sl, bt, style, wbits)
    assert two == (hd == 128), what
    if two:
        assert np.array_equal(be.n(q2).view(np.uint16), be.n(q0).view(np.uint16)) and np.array_equal(be.n(k2).view(np.uint16), be.n(k0).view(np.uint16))
        for x2, w in zip(c2, want_codes):
            assert np.array_equal(be.n(x2).view(np.uint8), w.view(np.uint8)), what
        out2 = torch.zeros((b, s, nh, hd), dtype=torch.float16, device=be.device)
        assert be.ext.paged_attn_q(q2, *c2, out2, sl, bt, wbits, len_const=0, len_offset=s, nsplit=nsplit, scratch=scratch,
                                   k_new=k2, v_new=be.t(vn), counters=counters)
    # one launch
    c1 = c.dev()
    q1, k1 = be.t(q), be.t(kn)
    out1 = torch.zeros((b, s, nh, hd), dtype=torch.float16, device=be.device)
    assert be.ext.attn_q_decode_fused(q1, k1, be.t(vn), *c1, out1, sint, cost, sl, bt, 0, style, scratch, counters, wbits, nsplit=nsplit), what
    assert np.array_equal(be.n(q1).view(np.uint16), q.view(np.uint16)) and np.array_equal(be.n(k1).view(np.uint16), kn.view(np.uint16))
    for x1, w in zip(c1, want_codes):
        assert np.array_equal(be.n(x1).view(np.uint8), w.view(np.uint8)), what
    assert int(be.n(counters).astype(np.int64).sum()) == 0
    if two:
        assert np.array_equal(be.n(out1).view(np.uint16), be.n(out2).view(np.uint16)), what
    # the oracle, end to end: attention over the unpacked old keys + the rotated new rows
    q_rot = OM.rope_(q, sin, cos, past, neox=neox) if style else q
    k_rot = OM.rope_(kn, sin, cos, past, neox=neox) if style else kn
    got = be.n(out1)
    for i in range(b):
        if paged:
            ko = np.concatenate([c.k_un[table[i, pg]] for pg in range(pages_per_seq)])[:past[i]]
            vo = np.concatenate([c.v_un[table[i, pg]] for pg in range(pages_per_seq)])[:past[i]]
        else:
            ko, vo = c.k_un[i, :past[i]], c.v_un[i, :past[i]]
        want = OM.attention(q_rot[i:i + 1], np.concatenate([ko, k_rot[i]])[None], np.concatenate([vo, vn[i]])[None])[0]
        _close(got[i], want, what + (i,))


@pytest.mark.parametrize("wbits", [6, 8])
@pytest.mark.parametrize("rb", [1, 2, 4])
@pytest.mark.parametrize("hd,nh,kvh,s,paged,style", [(128, 8, 4, 1, True, 2), (128, 8, 4, 3, False, 0), (128, 16, 4, 2, False, 2), (128, 4, 4, 1, True, 0),
                                                     (64, 16, 8, 1, True, 2), (64, 8, 8, 2, False, 0), (64, 8, 8, 3, False, 2), (64, 16, 8, 1, True, 0)])
def test_q68_decode_step_writes_the_codecs_codes(be, monkeypatch, wbits, rb, hd, nh, kvh, s, paged, style):
    """paged and contiguous, NeoX and no RoPE, head_dim 128 and 64, 1 / 2 / 4 query rows per workgroup; sequences of one split and of
    several, one crossing a page boundary (kv width = one codec block or two per token, so the codec touches the step's tokens only)"""
    rng = np.random.default_rng(53 + nh + s + wbits)
    past = np.array([700, 3, 255], dtype=np.int32)
    for nsplit in (1, 4):
        _decode_step_case(be, monkeypatch, wbits, hd, nh, kvh, 3, s, paged, style, rb, past, 4, nsplit, rng)


@pytest.mark.parametrize("seed", list(range(int(os.environ.get("EXL2_TEST_SEEDS", "8")))))        # (more seeds: a longer hunt, by hand)
def test_q68_decode_step_random_shapes(be, monkeypatch, seed):
    """seeded random shapes in the manner of test_attention_q4_decode_step_random_shapes, over both widths and both head sizes"""
    rng = np.random.default_rng(9000 + seed)
    wbits = int(rng.choice([6, 8])); hd = int(rng.choice([128, 64]))
    b = int(rng.integers(1, 5)); s = int(rng.integers(1, 9))
    kvh = int(rng.choice([4, 8])) * (128 // hd)                                 # (kv width a multiple of the codec's block)
    g = int(rng.choice([1, 2, 4, 8]))
    if s * g > 64:
        g = max(1, 64 // s); g = 1 << (g.bit_length() - 1)
    paged = bool(rng.integers(0, 2)); style = int(rng.choice([0, 1, 2]))
    pages_per_seq = int(rng.integers(2, 6))
    T = 256 * pages_per_seq
    past = np.array([int(rng.choice([0, 1, 30, 255, 256, 300, T - s])) for _ in range(b)], dtype=np.int32)
    past = np.minimum(past, T - s).astype(np.int32)
    _decode_step_case(be, monkeypatch, wbits, hd, kvh * g, kvh, b, s, paged, style, int(rng.choice([1, 2, 4])), past, pages_per_seq,
                      int(rng.choice([1, 2, 3, 8])), rng)


# ---- 4. unsupported shapes report "not handled"; a wrong width raises ---------------------------------------------------------------

@pytest.mark.parametrize("wbits", [6, 8])
def test_q68_unsupported_shapes_are_declined(be, wbits):
    kb, vb = _bits(wbits)

    def case(hd, nh, kvh, s):
        q = torch.zeros((1, s, nh, hd), dtype=torch.float16, device=be.device)
        kn = torch.zeros((1, s, kvh, hd), dtype=torch.float16, device=be.device)
        kq = torch.zeros((1, 256, kvh, hd * kb // 8), dtype=torch.uint8, device=be.device)
        vq = torch.zeros((1, 256, kvh, hd * vb // 8), dtype=torch.uint8, device=be.device)
        sc = torch.zeros((1, 256, kvh, hd // 32), dtype=torch.float16, device=be.device)
        out = torch.full((1, s, nh, hd), 3.0, dtype=torch.float16, device=be.device)
        return q, kn, kq, sc, vq, sc.clone(), out
    scratch = _scratch(be, 256, 256)
    counters = torch.zeros((256,), dtype=torch.int32, device=be.device)
    seq = be.t(np.array([5], dtype=np.int32))
    untouched = lambda out: bool((be.n(out) == F16(3.0)).all())
    # head_dim outside {64, 128, 256}; more than 64 query rows per kv head
    for hd, nh, kvh, s in ((96, 2, 2, 1), (128, 72, 1, 1), (128, 16, 1, 5)):
        q, kn, kq, ks, vq, vs, out = case(hd, nh, kvh, s)
        assert not be.ext.paged_attn_q(q, kq, ks, vq, vs, out, seq, None, wbits, len_offset=s, scratch=scratch)
        assert untouched(out)
    # the one-launch form: head_dim 256, head_dim 64 with an odd number of kv heads; the two-launch form: head_dim != 128
    for hd, nh, kvh in ((256, 2, 2), (64, 2, 1)):
        q, kn, kq, ks, vq, vs, out = case(hd, nh, kvh, 1)
        sin, cos = OM.rope_tables(16, hd, neox=True)
        assert not be.ext.attn_q_decode_fused(q, kn, kn.clone(), kq, ks, vq, vs, out, be.t(sin), be.t(cos), seq, None, 0, 2, scratch, counters, wbits)
        assert untouched(out) and int(be.n(kq).sum()) == 0 and int(be.n(vq).sum()) == 0
        assert not be.ext.rope_quant_append_q(q, kn, kn.clone(), kq, ks, vq, vs, be.t(sin), be.t(cos), 0, seq, None, 2, wbits)
        assert int(be.n(kq).sum()) == 0 and int(be.n(vq).sum()) == 0
    # code tensors of the other width are refused by the host mirror (the kernel would read past them)
    q, kn, kq, ks, vq, vs, out = case(128, 4, 4, 1)
    with pytest.raises(RuntimeError):
        be.ext.paged_attn_q(q, kq[..., :64].contiguous(), ks, vq, vs, out, seq, None, wbits, len_offset=1, scratch=scratch)


def test_q_entries_refuse_other_widths(be):
    """wbits outside {4, 6, 8}: an error from the library (EXL2_REQUIRE), and from the host mirror before it"""
    q = torch.zeros((1, 1, 4, 128), dtype=torch.float16, device=be.device)
    kn = torch.zeros((1, 1, 4, 128), dtype=torch.float16, device=be.device)
    kq = torch.zeros((1, 256, 4, 128), dtype=torch.uint8, device=be.device)
    sc = torch.zeros((1, 256, 4, 4), dtype=torch.float16, device=be.device)
    out = torch.zeros_like(q)
    seq = be.t(np.array([5], dtype=np.int32))
    scratch = _scratch(be, 64, 128)
    counters = torch.zeros((64,), dtype=torch.int32, device=be.device)
    lib, p = be.ext.lib, (lambda t: t.data_ptr())
    for wbits in (5, 0, 16):
        with pytest.raises(RuntimeError):
            be.ext.paged_attn_q(q, kq, sc, kq, sc, out, seq, None, wbits, len_offset=1, scratch=scratch)
        with pytest.raises(RuntimeError):
            lib.check(lib.exl2_paged_attn_q(p(q), p(kq), p(sc), p(kq), p(sc), None, None, p(out), p(seq), None, 1, 1, 4, 4, 128, 256, 0, 0, 1,
                                            128 ** -0.5, 1, 1, None, 0, None, wbits, None))
        with pytest.raises(RuntimeError):
            lib.check(lib.exl2_paged_attn_q_merged(p(q), p(kq), p(sc), p(kq), p(sc), None, None, p(out), p(seq), None, 1, 1, 4, 4, 128, 256, 0, 0, 1,
                                                   128 ** -0.5, 1, 1, None, 0, None, p(counters), 64, wbits, None))
        with pytest.raises(RuntimeError):
            lib.check(lib.exl2_attn_q_decode_fused(p(q), p(kn), p(kn), p(kq), p(sc), p(kq), p(sc), p(out), None, None, p(seq), None, 1, 1, 4, 4, 128,
                                                   256, 0, 0, 128 ** -0.5, 0, 0, 1, None, 0, p(counters), 64, None, wbits, None))
        with pytest.raises(RuntimeError):
            lib.check(lib.exl2_rope_quant_append_q(p(q), p(kn), p(kn), p(kq), p(sc), p(kq), p(sc), None, None, 1, 1, 4, 4, 128, 0, p(seq), None,
                                                   256, 0, 0, 0, wbits, None))
    assert int(be.n(kq).sum()) == 0 and float(be.n(out).astype(np.float32).sum()) == 0.0


# ---- the checker at model level ----------------------------------------------------------------------------------------------------

class OracleModelQ(OracleModel):
    """OracleModel.forward(q4_cache=True) for any cache width: the reference's ExLlamaV2Cache_Q4 / _Q6 / _Q8 semantics (cache.py:472-556,
    609-656) -- an 8-bit side goes through q8_pack / q8_unpack (one byte per element), a 4-bit side through q4_pack / q4_unpack."""

    def __init__(self, cfg, ck, wbits, **kw):
        super().__init__(cfg, ck, **kw)
        self.wbits = wbits
        self.side_bits = dict(zip("kv", _bits(wbits)))

    def _q4_state(self, batch):
        c = self.cfg
        if self.q4 is None:
            kv_dim = c.num_key_value_heads * c.head_dim
            q_block = 1                                                    # cache.py:452-457
            while (kv_dim * q_block) % 512:
                q_block += 1
            T = (c.max_seq_len + q_block - 1) // q_block * q_block
            L = c.num_hidden_layers
            st = dict(q_block=q_block, kv_dim=kv_dim)
            for side, bits in self.side_bits.items():
                st[side + "_codes"] = np.zeros((L, batch, T * kv_dim * bits // 8), dtype=np.uint8)
                st[side + "_scales"] = np.zeros((L, batch, T * kv_dim // 32), dtype=F16)
                st["temp_" + side] = np.zeros((batch, T * kv_dim), dtype=F16)
            self.q4 = st
        return self.q4

    def _q4_get(self, layer, past):
        st = self.q4
        if past == 0:
            return
        qb, d = st["q_block"], st["kv_dim"]
        hi = (past + qb - 1) // qb * qb
        for side, bits in self.side_bits.items():
            for r in range(st["temp_" + side].shape[0]):
                st["temp_" + side][r, :hi * d] = _unpack(st[side + "_codes"][layer, r, :hi * d * bits // 8],
                                                         st[side + "_scales"][layer, r, :hi * d // 32], bits)

    def _q4_store(self, layer, past, s):
        st = self.q4
        qb, d = st["q_block"], st["kv_dim"]
        lo = past // qb * qb
        hi = (past + s + qb - 1) // qb * qb
        for side, bits in self.side_bits.items():
            for r in range(st["temp_" + side].shape[0]):
                codes, scales = _pack(st["temp_" + side][r, lo * d:hi * d], bits)
                st[side + "_codes"][layer, r, lo * d * bits // 8:hi * d * bits // 8] = codes
                st[side + "_scales"][layer, r, lo * d // 32:hi * d // 32] = scales

    def q_adopt(self, layer, cache, be, n_tokens):
        """follow the device: the oracle's codes / scales of `layer`, tokens [0, n_tokens), become what the path under test left in
        `cache`.  Returns per side (bits, fraction of codes that differed, largest code difference, fraction of scales that differed,
        largest scale difference in fp16 ulp)."""
        st = self.q4
        d = st["kv_dim"]
        b = st["temp_k"].shape[0]
        res = {}
        for side, codes, scales in (("k", cache.key_states[layer], cache.key_scales[layer]), ("v", cache.value_states[layer], cache.value_scales[layer])):
            bits = self.side_bits[side]
            nc = n_tokens * d * bits // 8
            gc = be.n(codes).reshape(b, -1)[:, :nc]
            gs = be.n(scales).reshape(b, -1)[:, :n_tokens * d // 32]
            wc = st[side + "_codes"][layer][:, :nc]
            ws = st[side + "_scales"][layer][:, :n_tokens * d // 32]
            if bits == 4:
                delta = np.concatenate([(gc & 0xF).astype(np.int32) - (wc & 0xF), (gc >> 4).astype(np.int32) - (wc >> 4)], axis=-1)
            else:
                delta = gc.astype(np.int32) - wc
            ulp = np.abs(gs.view(np.int16).astype(np.int32) - ws.view(np.int16).astype(np.int32))
            res[side] = (bits, float((delta != 0).mean()), int(np.abs(delta).max(initial=0)), float((ulp != 0).mean()), int(ulp.max(initial=0)))
            st[side + "_codes"][layer][:, :nc] = gc
            st[side + "_scales"][layer][:, :n_tokens * d // 32] = gs.astype(F16)
        return res


# what "follow the device" may absorb per step (conditions, so that it cannot hide a wrong packer): every differing code differs by
# exactly 1; differing fraction of a 4-bit side < 0.01 (the figure of test_q4_cache_model_equals_q4_oracle), of an 8-bit side < 0.06;
# a differing scale at most 8 fp16 ulp away.  The 8-bit figures are twice what the reference-equivalent route alone (unpack everything,
# attend, re-quantize: kernels that are bit-exact against the reference's) shows on these inputs -- 0.0039 - 0.0281 of the 8-bit codes,
# scales 3 - 4 ulp -- because an 8-bit step is 1/16 of a 4-bit one: one fp16 ulp on a K / V element crosses a rounding boundary about
# ten times as often.
CODE_CAP = {4: 0.01, 8: 0.06}
SCALE_ULP_CAP = 8


def _check_adopted(res, what, cap=None, ulp_cap=SCALE_ULP_CAP):
    for side, (bits, frac, worst, sfrac, ulp) in res.items():
        print(what, "side", side, "bits", bits, "codes differing", round(frac, 5), "largest difference", worst, "scales differing", round(sfrac, 4), "worst ulp", ulp)
        assert worst <= 1, (what, side, worst)
        assert frac < (cap[bits] if cap else CODE_CAP[bits]), (what, side, bits, frac)
        assert ulp <= ulp_cap, (what, side, ulp)


# ---- 5. model level, both routes -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("wbits", [6, 8])
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("kvh,hd", [(4, 128), (2, 128), (1, 64)])
def test_q68_cache_model_equals_oracle(be, monkeypatch, wbits, fused, kvh, hd):
    """Prefill of 11 tokens + decode steps, batch 2, on ExLlamaV2Cache_Q6 / _Q8 through model.forward, in the form of
    test_q4_cache_model_equals_q4_oracle (same models, checkpoint seeds 7 / 8 / 9): kv widths 512 / 256 / 64 elements per token (q_block
    1 / 2 / 8; only 512 can take the route from the codes, the others unpack whatever `fused` says), every step at the model tolerance,
    the oracle following the device's codes under the caps above."""
    cfg = tiny_cfg(hidden_size=256, num_attention_heads=max(kvh, 2) if hd == 128 else 4, num_key_value_heads=kvh, head_dim=hd,
                   num_hidden_layers=2, intermediate_size=128)
    seed = {(4, 128): 7, (1, 64): 8, (2, 128): 9}[(kvh, hd)]
    ck = synth_checkpoint(cfg, be.device, seed=seed)
    oracle = OracleModelQ(cfg, ck, wbits)
    model = ExLlamaV2(cfg, device=be.device, ext=be.ext).load(ck)
    for attn, _ in model.layers:
        attn.q4_fused = fused
    cache = CACHES[wbits](model, batch_size=2)
    oracle.reset(2)
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, cfg.vocab_size, size=(2, 11))
    past = 0
    taken = {"direct": 0}
    for name in ("attn_q_decode_fused", "paged_attn_q"):       # the entries that attend from the codes: count what they served

        def spy(*a, _fn=getattr(be.ext, name), **k):
            ok = _fn(*a, **k)
            taken["direct"] += int(ok)
            return ok
        monkeypatch.setattr(be.ext, name, spy)

    def step(chunk):
        nonlocal past
        got = be.n(model.forward(torch.from_numpy(chunk), cache, last_id_only=False))
        want = oracle.forward(chunk, q4_cache=True)
        err = np.abs(got[..., :cfg.vocab_size].astype(np.float64) - want) / (LOGIT_TOL + np.abs(want) * 2.0 ** -8)
        print("past", past, "worst logit error / model tolerance", float(err.max()))
        check_logits(got[..., :cfg.vocab_size], want)
        past += chunk.shape[1]
        for layer in range(cfg.num_hidden_layers):
            _check_adopted(oracle.q_adopt(layer, cache, be, past), (wbits, fused, kvh, hd, past, layer))

    step(ids)                                                 # prefill: 11 tokens (an odd count: partial q_blocks)
    assert taken["direct"] == 0
    for t in (5, 9, 3, 60, 17):
        step(np.array([[t], [t + 1]]))
    assert taken["direct"] == (5 * cfg.num_hidden_layers if fused and kvh * hd % 512 == 0 else 0), taken
    model.unload()


@pytest.mark.parametrize("wbits", [6, 8])
def test_q68_cache_two_launch_step_in_the_model(be, monkeypatch, wbits):
    """the same with EXL2_Q4_LAUNCHES=2 (RoPE + pack, then attention from the codes: contiguous cache through model.forward)"""
    cfg = tiny_cfg(hidden_size=256, num_attention_heads=4, num_key_value_heads=4, head_dim=128, num_hidden_layers=2, intermediate_size=128)
    ck = synth_checkpoint(cfg, be.device, seed=7)
    oracle = OracleModelQ(cfg, ck, wbits)
    monkeypatch.setenv("EXL2_Q4_LAUNCHES", "2")
    model = ExLlamaV2(cfg, device=be.device, ext=be.ext).load(ck)
    cache = CACHES[wbits](model, batch_size=2)
    oracle.reset(2)
    ids = np.random.default_rng(7).integers(0, cfg.vocab_size, size=(2, 11))
    taken = {"two": 0}

    def spy(*a, _fn=be.ext.rope_quant_append_q, **k):
        ok = _fn(*a, **k)
        taken["two"] += int(ok)
        return ok
    monkeypatch.setattr(be.ext, "rope_quant_append_q", spy)
    past = 0
    for chunk in (ids, np.array([[5], [6]]), np.array([[9], [10]]), np.array([[3], [4]])):
        got = be.n(model.forward(torch.from_numpy(chunk), cache, last_id_only=False))
        check_logits(got[..., :cfg.vocab_size], oracle.forward(chunk, q4_cache=True))
        past += chunk.shape[1]
        for layer in range(cfg.num_hidden_layers):
            _check_adopted(oracle.q_adopt(layer, cache, be, past), (wbits, "two launches", past, layer))
    assert taken["two"] == 3 * cfg.num_hidden_layers, taken
    model.unload()


# ---- 6. chained decode -----------------------------------------------------------------------------------------------------------------

# Per-step cap on the codes the oracle may adopt in the chained-decode test (everything written so far is compared; with one codec
# block per token only the step's own token can differ, hence the 1 / (i + 1)).  4-bit sides: the figure of
# test_q4_cache_decodes_on_the_chain.  8-bit sides: twice the worst that the module-by-module UNPACK route (EXL2_Q4_FUSED=0,
# EXL2_CHAIN=0: existing kernels only) shows for the step's own token on the inputs of this test, see its docstring; the scale
# distance by the same rule (that route reaches 8 ulp on these inputs).
CHAIN_NEW_TOKEN_CAP8 = 2 * 36 / 512
CHAIN_SCALE_ULP_CAP = 2 * 8


def _chain_cap(i):
    return {4: 0.01 / (i + 1) + 0.002, 8: CHAIN_NEW_TOKEN_CAP8 / (i + 1)}


def _q68_chain_case(be, monkeypatch, cfg, wbits, recipe, batch, steps, chains=("1", "0"), stats=None):
    for chain in chains:
        monkeypatch.setenv("EXL2_CHAIN", chain)
        ck = synth_checkpoint(cfg, be.device, recipe=recipe, seed=16)
        oracle = OracleModelQ(cfg, ck, wbits)
        model = ExLlamaV2(cfg, device=be.device, ext=be.ext).load(ck)
        cache = CACHES[wbits](model, batch_size=batch)
        dec = GreedyGraphDecoder(model, cache, batch_size=batch)
        if stats is None:
            assert (dec.chain is not None) == (chain == "1")
        be.ext.chain_route_counts(reset=True)
        if not be.is_emu:
            dec.capture()
        first = np.array([3, 50][:batch])
        dec.reset(torch.from_numpy(first), 0)
        oracle.reset(batch)
        tok = first.copy()
        n_conf = 0
        for i in range(steps):
            dec.run(1, use_graph=not be.is_emu)
            want = oracle.forward(tok[:, None], q4_cache=True)[:, -1]
            got = be.n(dec.logits)[:, :cfg.vocab_size]
            check_logits(got[:, None], want[:, None])
            g = be.n(dec.tokens(i, 1))[:, 0]
            conf = confident(want)
            assert np.array_equal(g[conf], want.argmax(-1)[conf])
            n_conf += int(conf.sum())
            tok = g.copy()
            for layer in range(cfg.num_hidden_layers):
                res = oracle.q_adopt(layer, cache, be, i + 1)
                if stats is not None:
                    stats.extend((bits, frac * (i + 1), worst, ulp) for bits, frac, worst, _, ulp in res.values())
                else:
                    _check_adopted(res, (wbits, chain, i, layer), cap=_chain_cap(i), ulp_cap=CHAIN_SCALE_ULP_CAP)
        assert n_conf >= 1
        if stats is None:
            assert (sum(be.ext.chain_route_counts()) > 0) == (chain == "1")
        dec.free(); model.unload()


CHAIN_CASES = [("4.0bpw", 1, 64, "1"), ("2.5bpw", 2, 64, "1"), ("3.5bpw", 2, 64, "4"), ("4.0bpw", 1, 128, "1"),
               ("2.5bpw", 2, 128, "1"), ("4.0bpw", 1, 128, "2"), ("2.5bpw", 2, 128, "4")]


def _chain_cfg(hd):
    return tiny_cfg(num_attention_heads=512 // hd, num_key_value_heads=512 // hd, head_dim=hd, hidden_size=512, intermediate_size=512,
                    num_hidden_layers=2)


@pytest.mark.parametrize("wbits", [6, 8])
@pytest.mark.parametrize("recipe,batch,hd,launches", CHAIN_CASES)
def test_q68_cache_decodes_on_the_chain(be, monkeypatch, wbits, recipe, batch, hd, launches):
    """Q6 / Q8 cache on the chained route (one HIP graph per token on the GPU) and on the module-by-module route, the form and the
    cases of test_q4_cache_decodes_on_the_chain: the decoder is chained, the one- / two-launch entry was taken, logits at the model
    tolerance against OracleModelQ step by step, tokens where the oracle is confident, the codes each route wrote under the caps.

    Code cap of an 8-bit side, measured as the issue's yardstick prescribes (module-by-module unpack route, existing kernels only, on
    exactly these cases, emulation build; tools/q68_unpack_yardstick.py prints it).  Worst fraction of the step's own token's codes that
    differ from the oracle's, per case in the order of CHAIN_CASES -- Q6, 8-bit K side: 0.0703 0.0283 0.0371 0.0508 0.0283 0.0508 0.0283
    (its 4-bit V side: 0.0039 0.0039 0.0029 0.0098 0.0039 0.0098 0.0039); Q8, both sides: 0.0645 0.0371 0.0371 0.0625 0.0371 0.0625
    0.0371; every difference exactly 1; scales at most 8 (Q6) / 4 (Q8) fp16 ulp away.  Worst 8-bit figure 36 / 512 = 0.0703 (one token
    of 512 codes per layer and side: a coarse sample), times two: 0.1406 / (i + 1) at step i, since everything written so far is
    compared and only the step's own token can differ.  Scales: 2 x 8 ulp."""
    steps = 6
    monkeypatch.setenv("EXL2_Q4_LAUNCHES", launches)
    taken = {"one": 0, "two": 0}
    one_launch, two_launch = be.ext.attn_q_decode_fused, be.ext.rope_quant_append_q

    def spy_one(*a, **k):
        ok = one_launch(*a, **k)
        taken["one"] += int(ok)
        return ok

    def spy_two(*a, **k):
        ok = two_launch(*a, **k)
        taken["two"] += int(ok)
        return ok
    monkeypatch.setattr(be.ext, "attn_q_decode_fused", spy_one)
    monkeypatch.setattr(be.ext, "rope_quant_append_q", spy_two)
    _q68_chain_case(be, monkeypatch, _chain_cfg(hd), wbits, recipe, batch, steps)
    assert (taken["one"] > 0) == (launches == "1") and (taken["two"] > 0) == (hd == 128 and launches == "2"), taken


# ---- 7. Q8 is nearer to FP16 than Q4 is ------------------------------------------------------------------------------------------------

def test_q8_cache_nearer_to_fp16_than_q4(be):
    """Same model and inputs on FP16 / Q4 / Q8 caches (the form of test_q4_cache_decode_close_to_fp16, on a shape that attends from
    the codes): over the decode steps the device's Q8-to-FP16 logit distance is below its Q4-to-FP16 distance, and within the oracle's
    own Q8-to-FP16 distance plus twice the model tolerance."""
    cfg = tiny_cfg(hidden_size=256, num_attention_heads=4, num_key_value_heads=4, head_dim=128, num_hidden_layers=2, intermediate_size=128)
    ck = synth_checkpoint(cfg, be.device, seed=3)
    o16, o8 = OracleModel(cfg, ck), OracleModelQ(cfg, ck, 8)
    models = [ExLlamaV2(cfg, device=be.device, ext=be.ext).load(copy.deepcopy(ck)) for _ in range(3)]
    caches = [cls(m, batch_size=1) for cls, m in zip((ExLlamaV2Cache, ExLlamaV2Cache_Q4, ExLlamaV2Cache_Q8), models)]
    o16.reset(1); o8.reset(1)
    ids = np.random.default_rng(3).integers(0, cfg.vocab_size, size=(1, 8))
    d4 = d8 = do = tol = 0.0
    for n, chunk in enumerate((ids, np.array([[5]]), np.array([[41]]), np.array([[7]]))):
        a, b4, b8 = (be.n(m.forward(torch.from_numpy(chunk), c)).astype(np.float64)[..., :cfg.vocab_size] for m, c in zip(models, caches))
        w16, w8 = o16.forward(chunk)[:, -1:], o8.forward(chunk, q4_cache=True)[:, -1:]
        if n == 0:
            continue                                          # prefill attends over fp16 new tokens on every cache
        d4, d8 = max(d4, np.abs(b4 - a).max()), max(d8, np.abs(b8 - a).max())
        do = max(do, np.abs(w8 - w16).max())
        tol = max(tol, (LOGIT_TOL + np.abs(w16) * 2.0 ** -8).max())
    print("Q4 to FP16", d4, "Q8 to FP16", d8, "oracle Q8 to FP16", do, "model tolerance", tol)
    assert d8 < d4
    assert d8 <= do + 2 * tol
    for m in models:
        m.unload()


# ---- 8. host: cache selection ---------------------------------------------------------------------------------------------------------

def test_cache_selection_by_name():
    from exllamav2_amd import cache as C, pipeline, tensor_p
    import exllamav2_amd
    assert exllamav2_amd.ExLlamaV2Cache_Q6 is ExLlamaV2Cache_Q6 and exllamav2_amd.ExLlamaV2Cache_Q8 is ExLlamaV2Cache_Q8
    assert [C.cache_class(n) for n in ("fp16", "q4", "q6", "q8")] == [ExLlamaV2Cache, ExLlamaV2Cache_Q4, ExLlamaV2Cache_Q6, ExLlamaV2Cache_Q8]
    assert pipeline.cache_class is C.cache_class
    for bad in ("q5", "Q8", "", "fp8"):
        with pytest.raises(ValueError):
            C.cache_class(bad)
    assert (ExLlamaV2Cache_Q6.wbits, ExLlamaV2Cache_Q6.k_bits, ExLlamaV2Cache_Q6.v_bits) == (6, 8, 4)
    assert (ExLlamaV2Cache_Q8.wbits, ExLlamaV2Cache_Q8.k_bits, ExLlamaV2Cache_Q8.v_bits) == (8, 8, 8)
    import inspect
    assert "cache_class(" in inspect.getsource(tensor_p) and "cache_class(cache_type)" in inspect.getsource(pipeline.PipelineStage.__init__)


def test_pipeline_stage_builds_the_named_cache(be):
    """PipelineStage(cache_type=...) holds the cache class of that name, with the reference's shapes; an unknown name is an error"""
    from exllamav2_amd.pipeline import PipelineStage
    cfg = tiny_cfg(hidden_size=256, num_attention_heads=4, num_key_value_heads=4, head_dim=128, num_hidden_layers=1, intermediate_size=128)
    for name, cls, kd, vd in (("q6", ExLlamaV2Cache_Q6, 128, 64), ("q8", ExLlamaV2Cache_Q8, 128, 128), ("q4", ExLlamaV2Cache_Q4, 64, 64)):
        st = PipelineStage(cfg, 0, 1, be.device, n_seqs=1, max_seq_len=256, ext=be.ext, use_graph=False, cache_type=name)
        assert type(st.cache) is cls
        assert tuple(st.cache.key_states[0].shape) == (1, 256, 4, kd) and tuple(st.cache.value_states[0].shape) == (1, 256, 4, vd)
        assert tuple(st.cache.key_scales[0].shape) == (1, 256, 4, 4) and tuple(st.cache.temp_k.shape) == (1, 256, 4, 128)
        assert st.cache.q_views(0, True)[0].shape[:2] == (1, 256)
        st.model.unload()
    with pytest.raises(ValueError):
        PipelineStage(cfg, 0, 1, be.device, n_seqs=1, max_seq_len=256, ext=be.ext, use_graph=False, cache_type="q5")
