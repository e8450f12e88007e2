"""exl2_apply_loras (csrc/lora.hip) against float64: out += sum_l fp16(x A_l) B_l for a group of projections that read the same rows.

Checker (tests/lora_oracle.py: lora_terms): want = out_in + sum_l t16_l B_l with t16_l = fp16(x A_l), both products in float64.
Bar, derived and not measured: |got - want| <= half_tol(want, K) + 2^-11 * sum_l |t16_l| |B_l| -- the result's own fp16 rounding and
fp32 summation noise, plus the one-ulp uncertainty of where the low-rank intermediate rounds.  Every element is compared."""
import numpy as np
import pytest

from tests.lora_oracle import lora_terms, make_adapter
from tests.util import half_tol

F16 = np.float16
SHAPES = [(256, 512), (512, 96), (1056, 256)]
RANKS = [1, 8, 20, 64, 256]
ROWS = [1, 3, 16, 17, 40]
MAX_ROWS = 40


class Group:
    """A lora group on the backend with adapters {id: [(A, B) or None per projection]} (numpy fp16)."""

    def __init__(self, be, K, Ns, adapters, max_rows=MAX_ROWS):
        self.be, self.K, self.Ns, self.adapters = be, K, list(Ns), adapters
        self.h = be.ext.make_lora_group(K, self.Ns, max_rows)
        self.keep = []
        tables = [dict() for _ in self.Ns]
        for i, ents in adapters.items():
            for p, ent in enumerate(ents):
                if ent is None: continue
                ta, tb = be.t(ent[0]), be.t(ent[1])
                self.keep += [ta, tb]
                tables[p][i] = (ta, tb, ent[0].shape[1])
        self.max_rank = be.ext.lora_group_set_loras(self.h, tables)
        self.keep = []                  # the group owns copies: the caller's tensors may go away

    def run(self, ids, x, outs):
        tx = self.be.t(x)
        touts = [None if o is None else self.be.t(o) for o in outs]
        self.be.ext.apply_loras(self.h, ids, tx, touts)
        return [None if t is None else self.be.n(t) for t in touts]

    def check(self, ids, x, outs):
        got = self.run(ids, x, outs)
        for p, o in enumerate(outs):
            if o is None: continue
            pairs = [self.adapters[i][p] for i in ids if i in self.adapters and self.adapters[i][p] is not None]
            want, slack = lora_terms(x, o, pairs)
            err = np.abs(got[p].astype(np.float64) - want)
            tol = half_tol(want, self.K) + slack
            worst = float((err / tol).max())
            print(f"K={self.K} N={self.Ns[p]} rows={x.shape[0]} ids={ids}: max err/tol = {worst:.3f}")
            assert got[p].shape == want.shape and np.all(err <= tol), f"projection {p}: max err/tol {worst:.3f}"
            if not pairs:
                assert np.array_equal(got[p].view(np.uint16), o.view(np.uint16))      # nothing to add: not even a -0 loses its sign
        return got

    def free(self):
        self.be.ext.free_lora_group(self.h)


def _rows(rng, rows, K, N):
    x = rng.standard_normal((rows, K)).astype(F16)
    out = rng.standard_normal((rows, N)).astype(F16)
    out[0, :4] = [-0.0, 0.0, -0.0, 1.0]
    return x, out


@pytest.mark.parametrize("rank", RANKS)
@pytest.mark.parametrize("K,N", SHAPES)
def test_one_adapter(be, K, N, rank):
    rng = np.random.default_rng(1000 * rank + K + N)
    g = Group(be, K, [N], {7: [make_adapter(rng, K, N, rank)]})
    assert g.max_rank == rank
    for rows in ROWS:
        x, out = _rows(rng, rows, K, N)
        g.check([7], x, [out])
    g.free()


@pytest.mark.parametrize("r0,r1", [(1, 64), (20, 8), (256, 33)])
@pytest.mark.parametrize("K,N", SHAPES)
def test_two_adapters_of_different_rank(be, K, N, r0, r1):
    rng = np.random.default_rng(r0 * 7 + r1 + K)
    g = Group(be, K, [N], {11: [make_adapter(rng, K, N, r0)], 2 ** 40 + 5: [make_adapter(rng, K, N, r1)]})
    assert g.max_rank == max(r0, r1)
    for rows in (1, 17, 40):
        x, out = _rows(rng, rows, K, N)
        both = g.check([11, 2 ** 40 + 5], x, [out])[0]
        one = g.check([2 ** 40 + 5], x, [out])[0]
        assert not np.array_equal(both, one)
    g.free()


@pytest.mark.parametrize("rows", [1, 17])
def test_group_of_three_one_adapter_lacks_the_middle(be, rows):
    K, Ns = 256, [256, 128, 128]                      # q | k | v of the module tests
    rng = np.random.default_rng(rows)
    full = [make_adapter(rng, K, n, 8) for n in Ns]
    qv = [make_adapter(rng, K, Ns[0], 20), None, make_adapter(rng, K, Ns[2], 20)]
    g = Group(be, K, Ns, {1: full, 2: qv})
    x = rng.standard_normal((rows, K)).astype(F16)
    outs = [rng.standard_normal((rows, n)).astype(F16) for n in Ns]
    g.check([1, 2], x, outs)
    got = g.check([2], x, outs)                        # the middle projection has no listed adapter: untouched
    assert np.array_equal(got[1], outs[1])
    g.check([2], x, [outs[0], None, outs[2]])          # ... and needs no output
    g.free()


def test_unknown_id_is_skipped_and_runs_repeat(be):
    K, N = 512, 96
    rng = np.random.default_rng(5)
    g = Group(be, K, [N], {3: [make_adapter(rng, K, N, 20)]})
    x, out = _rows(rng, 17, K, N)
    a = g.check([99, 3], x, [out])[0]
    b = g.run([3], x, [out])[0]
    c = g.run([99, 3], x, [out])[0]
    assert np.array_equal(a.view(np.uint16), b.view(np.uint16)) and np.array_equal(a.view(np.uint16), c.view(np.uint16))
    none = g.run([99], x, [out])[0]
    assert np.array_equal(none.view(np.uint16), out.view(np.uint16))
    g.free()


def test_replacing_the_table(be):
    K, N = 256, 512
    rng = np.random.default_rng(6)
    g = Group(be, K, [N], {3: [make_adapter(rng, K, N, 64)]})
    x, out = _rows(rng, 3, K, N)
    g.check([3], x, [out])
    ta, tb = (be.t(m) for m in make_adapter(rng, K, N, 8))
    assert be.ext.lora_group_set_loras(g.h, [{4: (ta, tb, 8)}]) == 8
    got = g.run([3], x, [out])[0]                      # the table was REPLACED: id 3 is gone
    assert np.array_equal(got.view(np.uint16), out.view(np.uint16))
    assert be.ext.lora_group_set_loras(g.h, [{}]) == 0
    g.free()


def test_limits_raise(be):
    K, N = 256, 512
    rng = np.random.default_rng(7)
    h = be.ext.make_lora_group(K, [N], 16)
    a, b = (be.t(m) for m in make_adapter(rng, K, N, 257))
    with pytest.raises(RuntimeError, match="256"):
        be.ext.lora_group_set_loras(h, [{1: (a, b, 257)}])
    small = [tuple(be.t(m) for m in make_adapter(rng, K, N, 1)) for _ in range(9)]
    be.ext.lora_group_set_loras(h, [{i: small[i] for i in range(9)}])
    x, out = be.t(rng.standard_normal((1, K)).astype(F16)), be.t(np.zeros((1, N), F16))
    be.ext.apply_loras(h, list(range(8)), x, [out])
    with pytest.raises(RuntimeError, match="8"):
        be.ext.apply_loras(h, list(range(9)), x, [out])
    with pytest.raises(RuntimeError, match="max_rows"):
        be.ext.apply_loras(h, [0], be.t(np.zeros((17, K), F16)), [be.t(np.zeros((17, N), F16))])
    be.ext.free_lora_group(h)
    with pytest.raises(RuntimeError, match="32"):
        be.ext.make_lora_group(250, [N], 16)
