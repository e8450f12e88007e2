"""The two level-1 short cuts of the one-launch FP16 decode attention (csrc/attn_fused_body.h: SPEC_KV, ROPE_NOW) against the request
order they replace (EXL2_ATT_SPEC=0):

* split 0 of a launch without a block table (or with a table the caller declares to be the identity) requests its first batch of
  cached K / V rows before the cache length has arrived -- clamped addresses, lanes beyond the cached keys take zeros;
* a one-token step takes its rotary row from `rope_now`, which the step's first launch (embed_rows_chain) looked up once.

Neither changes a value, so everything is compared bit for bit: the attention output in o_proj's packed order, the appended cache
rows, the rest of the cache; in the chained decoder the logits and the tokens.  The EXL2_ATT_SPEC=0 side is pinned against the
oracle by tests/test_ops.py and tests/test_model.py.
"""
import numpy as np
import pytest
import torch

from exllamav2_amd.cache import ExLlamaV2Cache
from exllamav2_amd.config import ExLlamaV2Config
from exllamav2_amd.model import ExLlamaV2, GreedyGraphDecoder
from exllamav2_amd.synth import synth_checkpoint
from oracle import modules as OM

F16 = np.float16
SHAPES = {"mha": (4, 4, 128, 1), "gqa": (8, 2, 128, 1), "hd64": (4, 4, 64, 1), "two_seqs": (4, 4, 128, 2)}     # heads, kv heads, head_dim, rows
LENGTHS = [0, 1, 15, 16, 17, 63, 64, 127, 128, 129, 300]
NAN_BITS = np.array([0x7E00, 0xFFFF, 0x7C01, 0xFE00], dtype=np.uint16)        # quiet / negative / signalling fp16 NaNs


def _u16(a):
    return np.ascontiguousarray(a).view(np.uint16)


def _seqlens(length, b, cap):
    """sequence 0 at `length`; a second sequence at another entry of the list (its own rotary row, its own clamp)"""
    other = LENGTHS[(LENGTHS.index(length) + 4) % len(LENGTHS)] if length in LENGTHS else (length * 5 + 3) % cap
    return np.array([length, min(other, cap - 1)][:b], dtype=np.int32)


class Case:
    """one decode step's inputs: q / new k / new v, a cache of T rows per sequence whose rows >= the sequence's length are `fill`"""

    def __init__(self, shape, length, T, seed=0):
        self.nh, self.kvh, self.hd, self.b = SHAPES[shape]
        rng = np.random.default_rng(1000 * seed + 7 * length + self.hd + self.nh + T)
        b, nh, kvh, hd = self.b, self.nh, self.kvh, self.hd
        self.T, self.sl = T, _seqlens(length, b, T)
        self.q = rng.standard_normal((b, 1, nh, hd)).astype(F16)
        self.kn = (rng.standard_normal((b, 1, kvh, hd)) * 0.5).astype(F16)
        self.vn = rng.standard_normal((b, 1, kvh, hd)).astype(F16)
        self.kc = (rng.standard_normal((b, T, kvh, hd)) * 0.5).astype(F16)
        self.vc = rng.standard_normal((b, T, kvh, hd)).astype(F16)
        self.invperm = rng.permutation(nh * hd).astype(np.uint16)
        self.sin, self.cos = OM.rope_tables(T, hd, neox=True)
        self.rope_now = np.stack([np.stack([self.sin[p], self.cos[p]]) for p in self.sl]).astype(F16)       # what embed_rows_chain leaves

    def poisoned(self):
        kc, vc = self.kc.copy(), self.vc.copy()
        for i, p in enumerate(self.sl):
            n = kc[i, p:].size
            _u16(kc)[i, p:] = np.resize(NAN_BITS, n).reshape(kc[i, p:].shape)
            _u16(vc)[i, p:] = np.resize(NAN_BITS[::-1], n).reshape(vc[i, p:].shape)
        return kc, vc


def _launch(be, monkeypatch, c, spec, kct, vct, route="contiguous", with_rope_now=True):
    """one launch under EXL2_ATT_SPEC = spec (None: unset); kct / vct [b, T, kvh, hd] device tensors, updated in place"""
    if spec is None: monkeypatch.delenv("EXL2_ATT_SPEC", raising=False)
    else: monkeypatch.setenv("EXL2_ATT_SPEC", spec)
    dev = be.device
    out = torch.zeros((c.b, 1, c.nh, c.hd), dtype=torch.float16, device=dev)
    scratch = torch.zeros((be.ext.paged_attn_scratch_bytes(c.b * c.nh, c.hd, 64) // 4 + 1,), dtype=torch.float32, device=dev)
    counters = torch.zeros((256,), dtype=torch.int32, device=dev)
    inv = be.t(c.invperm.view(np.int16))
    rn = be.t(c.rope_now) if with_rope_now else None
    if route == "identity_table":
        assert c.T % 256 == 0
        pps = c.T // 256
        table = be.t(np.arange(c.b * pps, dtype=np.int32).reshape(c.b, pps))
        kv, vv = kct.view(c.b * pps, 256, c.kvh, c.hd), vct.view(c.b * pps, 256, c.kvh, c.hd)
        ok = be.ext.attn_decode_fused(be.t(c.q), be.t(c.kn), be.t(c.vn), kv, vv, out, be.t(c.sin), be.t(c.cos), be.t(c.sl), table, 0, 2,
                                      scratch, counters, out_invperm=inv.data_ptr(), rope_now=rn, identity_table=True)
    else:
        ok = be.ext.attn_decode_fused(be.t(c.q), be.t(c.kn), be.t(c.vn), kct, vct, out, be.t(c.sin), be.t(c.cos), be.t(c.sl), None, 0, 2,
                                      scratch, counters, out_invperm=inv.data_ptr(), rope_now=rn)
    assert ok
    res = be.n(out).copy()
    assert int(be.n(counters).astype(np.int64).sum()) == 0
    return res


def _check_same(be, c, got, want, what):
    """(out, k cache, v cache) of the two settings, bit for bit; the appended rows are where they belong"""
    (o1, k1, v1), (o0, k0, v0) = got, want
    assert np.array_equal(_u16(o1), _u16(o0)), what
    for i, p in enumerate(c.sl):
        assert np.array_equal(_u16(k1[i, p]), _u16(k0[i, p])) and np.array_equal(_u16(v1[i, p]), _u16(v0[i, p])), what
        assert np.array_equal(_u16(v1[i, p]), _u16(c.vn[i, 0])), what
        assert np.array_equal(_u16(k1[i, :p]), _u16(c.kc[i, :p])) and np.array_equal(_u16(v1[i, :p]), _u16(c.vc[i, :p])), what
    assert not np.isnan(o1.astype(np.float32)).any(), what


@pytest.mark.parametrize("route", ["contiguous", "identity_table"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_default_order_equals_spec_off(be, monkeypatch, shape, route):
    """every length of the list -- through the speculative window (128 keys of split 0) and across the one- / two-split boundary -- with a
    clean cache, and with every row at positions >= length holding fp16 NaN bit patterns: the output must not change by a bit"""
    for length in LENGTHS:
        c = Case(shape, length, 512)
        k0, v0 = be.t(c.kc), be.t(c.vc)
        want = (_launch(be, monkeypatch, c, "0", k0, v0, route), be.n(k0), be.n(v0))
        # (the launch as the callers without rope_now make it, too: the plain entry point)
        for rn in (True, False):
            k1, v1 = be.t(c.kc), be.t(c.vc)
            got = (_launch(be, monkeypatch, c, None, k1, v1, route, with_rope_now=rn), be.n(k1), be.n(v1))
            _check_same(be, c, got, want, (shape, route, length, "clean", rn))
            assert np.array_equal(_u16(got[1]), _u16(want[1])) and np.array_equal(_u16(got[2]), _u16(want[2]))
        # each short cut alone (the A/B switch's other two settings)
        for spec in ("1", "2"):
            k1, v1 = be.t(c.kc), be.t(c.vc)
            got = (_launch(be, monkeypatch, c, spec, k1, v1, route), be.n(k1), be.n(v1))
            _check_same(be, c, got, want, (shape, route, length, "spec=" + spec))
        pk, pv = c.poisoned()
        k1, v1 = be.t(pk), be.t(pv)
        got = (_launch(be, monkeypatch, c, None, k1, v1, route), be.n(k1), be.n(v1))
        _check_same(be, c, got, want, (shape, route, length, "poisoned"))
        # the poison beyond the appended row is still there, untouched
        for i, p in enumerate(c.sl):
            assert np.array_equal(_u16(got[1][i, p + 1:]), _u16(pk[i, p + 1:])) and np.array_equal(_u16(got[2][i, p + 1:]), _u16(pv[i, p + 1:]))


def _tail_of_own_segment(be, shape_, nbytes_seg=10 << 20):
    """a tensor of `shape_` whose last byte is the last byte of its allocator segment: no slack rows behind it.  (GPU: a request of
    10 MiB or more that no cached block can serve gets a segment of exactly its size; requests that landed inside an older segment
    are held until one does.  The tensor is the tail of that buffer.  The emulation twin has no segments.)"""
    n = int(np.prod(shape_))
    if be.is_emu:
        buf = torch.zeros((n + 4096,), dtype=torch.float16)
        return buf[-n:].view(shape_), buf
    held = []
    for _ in range(8):
        buf = torch.zeros((nbytes_seg // 2,), dtype=torch.float16, device=be.device)
        seg = [s for s in torch.cuda.memory_snapshot() if s["address"] <= buf.data_ptr() < s["address"] + s["total_size"]]
        if len(seg) == 1 and seg[0]["address"] + seg[0]["total_size"] == buf.data_ptr() + nbytes_seg:
            break
        held.append(buf)
    else:
        raise AssertionError("no buffer ended where its allocator segment ends")
    del held
    return buf[-n:].view(shape_), buf


@pytest.mark.parametrize("T", [32, 48])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_short_cache_speculative_rows_stay_inside(be, monkeypatch, shape, T):
    """a cache shorter than the speculative window (128 keys): the clamp keeps every speculative address inside the tensor, which ends
    where its allocator segment ends"""
    for length in [l for l in (0, 1, 31, 47) if l < T]:
        c = Case(shape, length, T)
        c.sl = np.array([length, (length + 13) % T][:c.b], dtype=np.int32)
        c.rope_now = np.stack([np.stack([c.sin[p], c.cos[p]]) for p in c.sl]).astype(F16)
        k0, v0 = be.t(c.kc), be.t(c.vc)
        want = (_launch(be, monkeypatch, c, "0", k0, v0), be.n(k0), be.n(v0))
        pk, pv = c.poisoned()
        (k1, kbuf), (v1, vbuf) = _tail_of_own_segment(be, c.kc.shape), _tail_of_own_segment(be, c.vc.shape)
        k1.copy_(be.t(pk)); v1.copy_(be.t(pv))
        got = (_launch(be, monkeypatch, c, None, k1, v1), be.n(k1), be.n(v1))
        _check_same(be, c, got, want, (shape, T, length))
        del k1, v1, kbuf, vbuf


def _tiny_model(be):
    cfg = ExLlamaV2Config(hidden_size=512, intermediate_size=1024, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=4,
                          head_dim=128, vocab_size=160, max_seq_len=256, max_input_len=32)
    ck = synth_checkpoint(cfg, be.device, recipe="4.0bpw", seed=11)
    return cfg, ExLlamaV2(cfg, device=be.device, ext=be.ext).load(ck)


@pytest.mark.parametrize("start", [0, 120])
def test_chained_decode_equals_spec_off(be, monkeypatch, start):
    """GreedyGraphDecoder (a captured graph on the GPU, eager on the emulation twin), 12 steps: logits and tokens of every step under the
    default and under EXL2_ATT_SPEC=0, bit for bit; rope_now after a step = the table rows of that step's position"""
    cfg, model = _tiny_model(be)
    steps = 12
    rng = np.random.default_rng(5)
    kv0 = [(rng.standard_normal((1, cfg.max_seq_len, cfg.num_key_value_heads, cfg.head_dim)) * 0.5).astype(F16) for _ in range(2 * cfg.num_hidden_layers)]
    runs = {}
    for spec in ("0", None):
        if spec is None: monkeypatch.delenv("EXL2_ATT_SPEC", raising=False)
        else: monkeypatch.setenv("EXL2_ATT_SPEC", spec)
        cache = ExLlamaV2Cache(model, batch_size=1)
        for i in range(cfg.num_hidden_layers):
            cache.key_states[i].copy_(be.t(kv0[2 * i])); cache.value_states[i].copy_(be.t(kv0[2 * i + 1]))
        dec = GreedyGraphDecoder(model, cache, batch_size=1)
        assert dec.chain is not None and "rope_now" in dec.chain
        if not be.is_emu:
            dec.capture()
        dec.reset(torch.tensor([3]), start)
        logits, ropes = [], []
        for _ in range(steps):
            dec.run(1, use_graph=not be.is_emu)
            logits.append(be.n(dec.logits).copy()); ropes.append(be.n(dec.chain["rope_now"]).copy())
        assert dec.chain is not None, "the step left the chained route"
        runs[spec] = (np.stack(logits), be.n(dec.tokens(start, steps)).copy(), ropes,
                      [be.n(t).copy() for t in cache.key_states + cache.value_states])
        dec.free()
    sin, cos = be.n(model.sin), be.n(model.cos)
    for k, r in enumerate(runs[None][2]):
        assert np.array_equal(_u16(r[0, 0]), _u16(sin[start + k])) and np.array_equal(_u16(r[0, 1]), _u16(cos[start + k])), k
    assert np.array_equal(_u16(runs[None][0]), _u16(runs["0"][0]))
    assert np.array_equal(runs[None][1], runs["0"][1])
    for a, b_ in zip(runs[None][3], runs["0"][3]):
        assert np.array_equal(_u16(a), _u16(b_))
    assert not np.isnan(runs[None][0].astype(np.float32)).any()
    model.unload()
