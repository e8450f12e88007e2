"""Every kernel csrc/qgemv_lean.hip builds (LEAN_DENSE_KERNELS, LEAN_MOE_KERNELS) against the float64 oracle, one case or more per
instantiation.

Which kernel a launch gets is decided by the host planner (qgemv_lean_launch / qgemv_lean_group_plan) from the shape, the row count,
the bit mix, the CU count, LDS budgets and environment hooks; the library counts its launches per instantiation
(exl2_lean_kernel_counts), so every case below states the kernel it is about and fails when the planner takes another one.  The
completeness test compares the keys of the case tables with the keys the library reports: an instantiation without a case fails, and
so does a case whose kernel is no longer built.

  * MATRIX_CASES: one matrix through exl2_gemm_half_q_half_chain -- key, numerics at the bar of
    test_gemm_chain_random_bit_mixes_and_depths, and the reference's parity relation gemm(I) == reconstruct() bit for bit;
  * DECODER_CASES: the pair kernels (gate|up) through a one-layer chained decoder, test_chain's _decode_and_check;
  * MOE_CASES: the grouped-expert kernels through one sparse-MoE block, the bar of tests/test_moe.py;
  * the DEP kernels (overlapped chain) run only inside a decoder, whose gate kernels are their producers:
    tests/test_chain.py::test_overlapped_chain_equals_serial_chain (OVERLAP_KEYS there).
"""
import collections

import numpy as np
import pytest
import torch

from exllamav2_amd.ext import LeanKey
from oracle import exl2 as OX
from oracle import modules as OM
from tests.test_model import tiny_cfg
from tests.util import exl2_to_torch, gptq_to_torch, half_tol


def dense(S, nslots, gptq=False, pair=False, rows=False, walk=False, dep=False, xmem=False, loads=False):
    return LeanKey(moe=False, gptq=gptq, S=S, nslots=nslots, pair=pair, rows=rows, walk=walk, dep=dep, xmem=xmem, loads=loads)


def moe(S, nslots, pair, walk=False):
    return LeanKey(moe=True, gptq=False, S=S, nslots=nslots, pair=pair, rows=False, walk=walk, dep=False, xmem=False, loads=False)


def launched(be):
    """{key: launches} since the last reset, the kernels that did not run left out; resets"""
    return {k: n for k, n in be.ext.lean_kernel_counts(reset=True).items() if n}


# keys no shape or hook makes the planner choose: {key: reason}.  Printed by the completeness test; may hold no key that a test or
# bench.py launches.
UNREACHABLE = {}


# ---- one matrix: exl2_gemm_half_q_half_chain ---------------------------------------------------------------------------------------

# bit mixes: two widths at least, g32 / g64 sections beside a g128 one, a partial item (a section whose length is no multiple of the
# 128 rows of an item) at a section end
MIX_1024 = [(5, 128, 128), (4, 128, 384), (4, 32, 256), (3, 64, 160), (2, 32, 96)]
# 50 items of mostly 4 bits: more than ONE register load of 8 waves (6 items each) -- the 16-wave geometry
MIX_6400 = [(5, 32, 160), (4, 128, 5984), (3, 64, 256)]
# one row of a long K: shares of several register loads (the LOADS form and the plain 16-wave form beside it)
MIX_18432 = [(4, 128, 256), (3, 32, 18016), (2, 64, 160)]

DRAWS = 32
MatrixCase = collections.namedtuple("MatrixCase", "id key fmt k n spec rows env")
MATRIX_CASES = [
    # <= 4 rows, wave-private slices
    MatrixCase("plain_s8", dense(8, 1), "exl2", 1024, 32, MIX_1024, 3, {}),
    MatrixCase("plain_s16_forced", dense(16, 1), "exl2", 1024, 32, MIX_1024, 1, {"EXL2_LEAN_S16": "1", "EXL2_LEAN_CUS": "256"}),
    MatrixCase("plain_s16_long_k", dense(16, 1), "exl2", 6400, 32, MIX_6400, 2, {}),
    MatrixCase("plain_two_tiles", dense(8, 2), "exl2", 1024, 64, MIX_1024, 4, {"EXL2_LEAN_TPW": "2"}),
    MatrixCase("gptq_plain_s8", dense(8, 1, gptq=True), "gptq", 1024, 32, 32, 3, {}),
    MatrixCase("gptq_plain_s16_forced", dense(16, 1, gptq=True), "gptq", 1024, 32, 128, 1, {"EXL2_LEAN_S16": "1", "EXL2_LEAN_CUS": "256"}),
    MatrixCase("gptq_plain_two_tiles", dense(8, 2, gptq=True), "gptq", 1024, 64, 64, 4, {"EXL2_LEAN_TPW": "2"}),
    # ROWS: 5-16 rows staged once per workgroup; two tiles per unit from 9 rows on, the workgroup walks
    MatrixCase("rows_s8", dense(8, 1, rows=True), "exl2", 1024, 32, MIX_1024, 8, {}),
    MatrixCase("rows_s16", dense(16, 1, rows=True), "exl2", 6400, 32, MIX_6400, 7, {}),
    MatrixCase("rows_walk", dense(8, 2, rows=True, walk=True), "exl2", 1024, 64, MIX_1024, 16, {"EXL2_LEAN_ROWS_GRID": "1"}),
    MatrixCase("gptq_rows_s8", dense(8, 1, gptq=True, rows=True), "gptq", 1024, 32, 128, 5, {}),
    MatrixCase("gptq_rows_s16", dense(16, 1, gptq=True, rows=True), "gptq", 6400, 32, 128, 6, {}),
    MatrixCase("gptq_rows_walk", dense(8, 2, gptq=True, rows=True, walk=True), "gptq", 1024, 64, 32, 9, {"EXL2_LEAN_ROWS_GRID": "1"}),
    # LOADS: one row, more tiles than CUs
    MatrixCase("loads", dense(8, 2, rows=True, walk=True, loads=True), "exl2", 18432, 64, MIX_18432, 1, {"EXL2_LEAN_CUS": "1"}),
    MatrixCase("loads_off_plain_s16", dense(16, 1), "exl2", 18432, 64, MIX_18432, 1, {"EXL2_LEAN_CUS": "1", "EXL2_LEAN_ROWS1": "0"}),
    # XMEM: the A operands from memory
    MatrixCase("xmem_s8", dense(8, 1, xmem=True), "exl2", 1024, 32, MIX_1024, 16, {"EXL2_LEAN_XMEM": "2"}),
    MatrixCase("xmem_s16", dense(16, 1, xmem=True), "exl2", 6400, 32, MIX_6400, 5, {"EXL2_LEAN_XMEM": "2"}),
    MatrixCase("gptq_xmem_s8", dense(8, 1, gptq=True, xmem=True), "gptq", 1024, 32, 64, 6, {"EXL2_LEAN_XMEM": "2"}),
    MatrixCase("gptq_xmem_s16", dense(16, 1, gptq=True, xmem=True), "gptq", 6400, 32, 128, 9, {"EXL2_LEAN_XMEM": "2"}),
]


def _matrix(be, case):
    """(reference weights [K, N], packed row -> input feature, handle, what the handle points into)"""
    if case.fmt == "gptq":
        t = OX.synth_gptq(case.k, case.n, case.spec, seed=61, act_order=True)
        t["scales"] = (t["scales"].astype(np.float32) * 0.6).astype(np.float16)      # (weights of the EXL2 cases' magnitude: std ~0.05)
        ref = OX.gptq_reconstruct(t)
        w = gptq_to_torch(be, t)
        h = be.ext.make_q_matrix_from_dict(w, None)
        perm, _ = OX.gptq_sequential_perm(t["g_idx"], case.k // case.spec)
        return ref, perm.astype(np.int64), h, w
    assert len({b for b, _, _ in case.spec}) >= 2 and {g for _, g, _ in case.spec} & {32, 64} and 128 in {g for _, g, _ in case.spec}
    assert any(rows % 128 for _, _, rows in case.spec)
    t = OX.synth_exl2(case.k, case.n, case.spec, seed=61, act_order=True, sigma=0.05)
    ref = OX.exl2_reconstruct(t)
    w = exl2_to_torch(be, t)
    return ref, np.argsort(t["q_invperm"]).astype(np.int64), be.ext.make_q_matrix_from_dict(w, None), w


def _activations(case, ref, perm):
    """random activations, norm weights and hand-off (x * norm weight in packed order, sum of squares) as in
    test_gemm_chain_random_bit_mixes_and_depths, the oracle's result and the bar: slack * half_tol.

    The oracle rounds rmsnorm(x) to fp16 once; the hand-off rounds x * w to fp16 and the finished sums are scaled by 1 / rms; a kernel
    that puts a group's scale on the fp32 partial sum differs from reconstruct()'s fp16 weights once more.  These roundings are
    independent, each ~2^-11 relative on every one of K terms: with exact arithmetic everywhere else the first two already sit
    0.5-0.9 of the bar apart at the worst of a few hundred outputs (measured with the float64 model below, not with a kernel), so
    whether a draw passes is a matter of its tail.  So that a case measures its kernel and not that tail, the activations are the
    draw of DRAWS at which the float64 model of the hand-off's rounding points is nearest to the oracle, in units of the bar: no
    kernel result enters the choice, and the bar is the same for every draw."""
    k, rows = case.k, case.rows
    slack = 2 * max(1.0, (k / 1024.0) ** 0.5)
    w64 = ref[perm].astype(np.float64)
    best = None
    for seed in range(DRAWS):
        rng = np.random.default_rng(1000 * rows + seed)
        x = (rng.standard_normal((rows, k)) * 2).astype(np.float16)
        nw = (1 + 0.1 * rng.standard_normal(k)).astype(np.float16)
        xp = (x.astype(np.float32) * nw.astype(np.float32)).astype(np.float16)[:, perm]
        ss = (x.astype(np.float32) ** 2).sum(-1, keepdims=True).astype(np.float32)
        want = OX.gemm_ref(OM.rms_norm(x, nw, 1e-5), ref, exact=True)
        bar = slack * half_tol(want, k)
        model = (xp.astype(np.float64) @ w64) / np.sqrt((x.astype(np.float64) ** 2).mean(-1, keepdims=True) + 1e-5)
        d = float((np.abs(model - want) / bar).max())
        if best is None or d < best[0]:
            best = (d, x, nw, xp, ss, want, bar)
    return best[1:]


def _identity_rows(case):
    """packed rows the parity relation is sampled at: the first and the last row of every bit-width section, the rows around the start
    of a partial item at a section end, and rows spread over the rest -- at most 64 launches of case.rows rows"""
    sections = [(128, case.k)] if case.fmt == "gptq" else [(g, rows) for _, g, rows in case.spec]
    must, a = [], 0
    for _, rows in sections:
        b = a + rows
        must += [a, b - 1]
        if rows % 128:
            p = a + rows // 128 * 128                                    # the partial item [p, b)
            must += [p, max(p - 1, a)]
        a = b
    launches = []
    for r in sorted(set(must)):                                         # a launch = case.rows consecutive packed rows holding r
        r0 = min(max(r - case.rows // 2, 0), case.k - case.rows)
        if not any(l0 <= r < l0 + case.rows for l0 in launches):
            launches.append(r0)
    rng = np.random.default_rng(5)
    room = 64 - len(launches)
    assert room >= 0, len(launches)
    launches += rng.choice(case.k - case.rows + 1, size=min(room, 24), replace=False).tolist()
    assert len(launches) <= 64 and all(any(l0 <= r < l0 + case.rows for l0 in launches) for r in must)
    return launches


@pytest.mark.parametrize("case", MATRIX_CASES, ids=[c.id for c in MATRIX_CASES])
def test_one_matrix_kernel(be, case, monkeypatch):
    """exl2_gemm_half_q_half_chain at the smallest shape that makes the planner take case.key: the launch is that kernel's and no
    other's; random activations against the oracle's reconstruct-then-matmul on rmsnorm(x) (the bar of
    test_gemm_chain_random_bit_mixes_and_depths); one-hot rows with sum(x^2) = K and eps = 0 return reconstruct()'s rows bit for bit
    (tests/test_chain.py::test_lean_kernel_identity_rows_equal_reconstruct)."""
    k, n, rows = case.k, case.n, case.rows
    ref, perm, h, keep = _matrix(be, case)
    for name, v in case.env.items():
        monkeypatch.setenv(name, v)
    x, nw, xp, ss, want, bar = _activations(case, ref, perm)
    c = torch.zeros((rows, n), dtype=torch.float16, device=be.device)
    be.ext.lean_kernel_counts(reset=True)
    be.ext.gemm_half_q_half_chain(be.t(xp), be.t(ss), 1, 1e-5, h, c, rows)         # (a declined launch raises)
    assert launched(be) == {case.key: 1}
    err = np.abs(be.n(c).astype(np.float64) - want) / bar
    assert np.all(err <= 1.0), float(err.max())
    # the parity relation, bit for bit
    ss1 = be.t(np.full((rows, 1), float(k), dtype=np.float32))
    launches = _identity_rows(case)
    for r0 in launches:
        eye = np.zeros((rows, k), dtype=np.float16)
        eye[np.arange(rows), r0 + np.arange(rows)] = 1.0
        c = torch.zeros((rows, n), dtype=torch.float16, device=be.device)
        be.ext.gemm_half_q_half_chain(be.t(eye), ss1, 1, 0.0, h, c, rows)
        got, rows_want = be.n(c), ref[perm[r0:r0 + rows]]
        assert np.array_equal(got.view(np.uint16), rows_want.view(np.uint16)), (r0, np.abs(got.astype(np.float32) - rows_want.astype(np.float32)).max())
    assert launched(be) == {case.key: len(launches)}
    be.ext.free_q_matrix(h)


# ---- the pair kernels: gate|up of a one-layer chained decoder ----------------------------------------------------------------------

# what a step of a one-layer decoder launches besides gate|up: q|k|v (three matrices), o_proj (accumulate + chain-out), down_proj,
# head.  EXL2_LEAN_CUS pins the CU count the planner sees, so that the emulator and the GPU plan alike.
# (hidden 1024 = 8 items per tile: every wave of a tile has a share, so a wrong index in any wave's part shows)
BASE = dict(hidden_size=1024, intermediate_size=1024, num_attention_heads=8, num_key_value_heads=2, head_dim=128)
WIDE = dict(hidden_size=8192, intermediate_size=64, num_attention_heads=2, num_key_value_heads=1, head_dim=128)
DecoderCase = collections.namedtuple("DecoderCase", "id key cfg recipe batch env step")
_G = "gptq-4bit-32g"
DECODER_CASES = [
    DecoderCase("pair_s4", dense(4, 2, pair=True), BASE, "3.5bpw", 1, {}, {dense(8, 1): 4, dense(4, 2, pair=True): 1}),
    DecoderCase("pair_s8_rows3", dense(8, 2, pair=True), BASE, "3.5bpw", 3, {}, {dense(8, 1): 4, dense(8, 2, pair=True): 1}),
    DecoderCase("pair_s8_one_row", dense(8, 2, pair=True), BASE, "2.5bpw", 1, {"EXL2_LEAN_PAIR4": "0"}, {dense(8, 1): 4, dense(8, 2, pair=True): 1}),
    # K = 8192 at 2.5 bpw: 16-19 items of 2 / 3 bits per wave of a 4-wave tile -- several register loads (its own instantiation)
    DecoderCase("pair_s4_loads", dense(4, 2, pair=True, walk=True), WIDE, "2.5bpw", 1, {},
                {dense(8, 1): 3, dense(16, 1): 1, dense(4, 2, pair=True, walk=True): 1}),
    DecoderCase("pair_rows_walk", dense(8, 2, pair=True, rows=True, walk=True), BASE, "3.5bpw", 6, {"EXL2_XP_TILED": "0", "EXL2_LEAN_ROWS_GRID": "1"},
                {dense(8, 1, rows=True): 4, dense(8, 2, pair=True, rows=True, walk=True): 1}),
    DecoderCase("pair_xmem", dense(8, 2, pair=True, xmem=True), BASE, "3.5bpw", 6, {"EXL2_LEAN_XMEM": "2"},
                {dense(8, 1, xmem=True): 4, dense(8, 2, pair=True, xmem=True): 1}),
    DecoderCase("gptq_pair_s4", dense(4, 2, gptq=True, pair=True), BASE, _G, 1, {}, {dense(8, 1, gptq=True): 4, dense(4, 2, gptq=True, pair=True): 1}),
    DecoderCase("gptq_pair_s8_rows3", dense(8, 2, gptq=True, pair=True), BASE, _G, 3, {}, {dense(8, 1, gptq=True): 4, dense(8, 2, gptq=True, pair=True): 1}),
    DecoderCase("gptq_pair_s4_loads", dense(4, 2, gptq=True, pair=True, walk=True), WIDE, _G, 1, {},
                {dense(8, 1, gptq=True): 3, dense(16, 1, gptq=True): 1, dense(4, 2, gptq=True, pair=True, walk=True): 1}),
    DecoderCase("gptq_pair_rows_walk", dense(8, 2, gptq=True, pair=True, rows=True, walk=True), BASE, _G, 6,
                {"EXL2_XP_TILED": "0", "EXL2_LEAN_ROWS_GRID": "1"},
                {dense(8, 1, gptq=True, rows=True): 4, dense(8, 2, gptq=True, pair=True, rows=True, walk=True): 1}),
    DecoderCase("gptq_pair_xmem", dense(8, 2, gptq=True, pair=True, xmem=True), BASE, _G, 6, {"EXL2_LEAN_XMEM": "2"},
                {dense(8, 1, gptq=True, xmem=True): 4, dense(8, 2, gptq=True, pair=True, xmem=True): 1}),
]


def whole_steps(counts, step):
    """how many times the launches of one step (a multiset of keys) were made, when `counts` is a whole number of steps; else None.
    (A decoder launches its steps when it runs them one by one and when it captures them into a graph: the number differs between
    the backends, the multiset of a step does not.)"""
    if set(counts) != set(step):
        return None
    n = {counts[k] // step[k] for k in step} if all(counts[k] % step[k] == 0 for k in step) else set()
    return n.pop() if len(n) == 1 else None


@pytest.mark.parametrize("case", DECODER_CASES, ids=[c.id for c in DECODER_CASES])
def test_pair_kernel_in_a_decoder(be, case, monkeypatch):
    """exl2_q_attn_forward_1_chain / _2_chain / exl2_q_mlp_forward_chain and the head as a one-layer chained decoder runs them, step
    by step against the oracle (tests/test_chain.py: _decode_and_check, the model tolerance): every launch of the run is one of
    case.step's kernels, in case.step's proportions -- gate|up on case.key."""
    from tests.test_chain import _decode_and_check
    monkeypatch.setenv("EXL2_LEAN_CUS", "256")
    for name, v in case.env.items():
        monkeypatch.setenv(name, v)
    cfg = tiny_cfg(num_hidden_layers=1, max_batch_size=16, **case.cfg)
    be.ext.lean_kernel_counts(reset=True)
    be.ext.chain_route_counts(reset=True)
    _decode_and_check(be, cfg, case.recipe, case.batch, steps=2, seed=5)
    counts = launched(be)
    assert case.key in case.step and (whole_steps(counts, case.step) or 0) >= 2, counts
    lean, flat = be.ext.chain_route_counts(reset=True)
    assert flat == 0 and lean == sum(counts.values())


# ---- the grouped-expert kernels: one sparse-MoE block -------------------------------------------------------------------------------

# (the experts' launches are planned when the module is made: the hooks are set before the model loads)
MoeCase = collections.namedtuple("MoeCase", "id key hidden inter recipe rows env launches")
MOE_CASES = [
    # one row: gate|up of the selected experts as 4-wave tile pairs, the weighted sum of their down projections in one 16-wave launch
    MoeCase("moe_pair_s4", moe(4, 2, True), 1024, 1024, "3.5bpw", 1, {}, {moe(4, 2, True): 1, moe(8, 2, True, walk=True): 1}),
    MoeCase("moe_down_pair_sum", moe(8, 2, True, walk=True), 1024, 1024, "4.0bpw", 1, {}, {moe(4, 2, True): 1, moe(8, 2, True, walk=True): 1}),
    MoeCase("moe_down_s8", moe(8, 1, False), 1024, 1024, "3.5bpw", 1, {"EXL2_MOE_NO_SUM": "1"}, {moe(4, 2, True): 1, moe(8, 1, False): 1}),
    MoeCase("moe_down_s16", moe(16, 1, False), 1024, 1024, "2.5bpw", 1, {"EXL2_MOE_NO_SUM": "1", "EXL2_LEAN_S16": "1"},
            {moe(4, 2, True): 1, moe(16, 1, False): 1}),
    MoeCase("moe_pair_s8_one_row", moe(8, 2, True), 1024, 1024, "3.5bpw", 1, {"EXL2_LEAN_PAIR4": "0"}, {moe(8, 2, True): 1, moe(8, 2, True, walk=True): 1}),
    MoeCase("moe_pair_s8_rows3", moe(8, 2, True), 1024, 1024, "3.5bpw", 3, {"EXL2_MOE_LEAN_ROWS": "1"}, {moe(8, 2, True): 1, moe(8, 1, False): 1}),
    # K = 8192 at 2.5 bpw: the pair with several register loads
    MoeCase("moe_pair_s4_loads", moe(4, 2, True, walk=True), 8192, 64, "2.5bpw", 1, {}, {moe(4, 2, True, walk=True): 1, moe(8, 2, True, walk=True): 1}),
]


@pytest.mark.parametrize("case", MOE_CASES, ids=[c.id for c in MOE_CASES])
def test_grouped_expert_kernel(be, case, monkeypatch):
    """exl2_q_moe_mlp_forward_ on one Mixtral-style block (4 experts, top 2) against the oracle's block at the bar of
    tests/test_moe.py (rows whose router decision is a near tie left out): the block's lean launches are case.launches."""
    from exllamav2_amd.config import ExLlamaV2Config
    from exllamav2_amd.model import ExLlamaV2
    from exllamav2_amd.synth import synth_checkpoint
    from oracle.model import OracleModel
    monkeypatch.setenv("EXL2_LEAN_CUS", "256")
    for name, v in case.env.items():
        monkeypatch.setenv(name, v)
    rows, hidden = case.rows, case.hidden
    cfg = ExLlamaV2Config(hidden_size=hidden, intermediate_size=case.inter, num_hidden_layers=1, num_attention_heads=2,
                          num_key_value_heads=1, head_dim=64, vocab_size=96, max_seq_len=256, max_input_len=32, max_batch_size=16,
                          num_experts=4, num_experts_per_token=2, arch="mixtral")
    ck = synth_checkpoint(cfg, be.device, recipe=case.recipe, seed=40)
    oracle = OracleModel(cfg, ck)
    model = ExLlamaV2(cfg, device=be.device, ext=be.ext).load(ck)
    block = model.layers[0][1]
    rng = np.random.default_rng(3)
    n_checked = 0
    for call in range(2):                                               # (another input: other experts through the same handle)
        x = torch.from_numpy((rng.standard_normal((rows, 1, hidden)) * 0.7).astype(np.float16)).to(be.device)
        y = x.clone()
        be.ext.lean_kernel_counts(reset=True)
        block.forward(y)
        assert launched(be) == case.launches and case.key in case.launches
        xh = be.n(x).reshape(rows, hidden)
        pfx = "model.layers.0"
        oracle.router_margin = np.full((rows,), np.inf)
        want = oracle.moe_mlp(xh, OM.rms_norm(xh, oracle.w[pfx + ".post_attention_layernorm"], cfg.norm_eps), pfx).astype(np.float64)
        ok = oracle.router_margin > 2e-3
        got = be.n(y).astype(np.float64).reshape(rows, hidden)
        tol = 0.01 + np.abs(want) * 2.0 ** -7
        assert np.all(np.abs(got - want)[ok] <= tol[ok]), float((np.abs(got - want)[ok] / tol[ok]).max())
        n_checked += int(ok.sum())
    assert n_checked >= 1, "every router decision was a near tie: the comparison would be vacuous"
    model.unload()


# ---- completeness ---------------------------------------------------------------------------------------------------------------------

def case_keys():
    from tests.test_chain import OVERLAP_KEYS
    return {c.key for c in MATRIX_CASES} | {c.key for c in DECODER_CASES} | {c.key for c in MOE_CASES} | set(OVERLAP_KEYS) | set(O_PROJ_KEYS.values())


def test_every_built_kernel_has_a_case(be):
    """the keys of the case tables are the keys the library reports: an instantiation added to LEAN_DENSE_KERNELS / LEAN_MOE_KERNELS
    without a case fails here, and so does a case (or an UNREACHABLE entry) whose kernel is no longer built"""
    built = set(be.ext.lean_kernel_counts())
    print(f"{len(built)} kernels built; UNREACHABLE: {UNREACHABLE}")
    assert len(built) >= 45
    assert not (case_keys() & set(UNREACHABLE))
    assert built - case_keys() - set(UNREACHABLE) == set(), "kernels without a case"
    assert (case_keys() | set(UNREACHABLE)) - built == set(), "cases of kernels that are not built"


# ---- o_proj above 512 tiles at 5-16 rows: two tiles per workgroup in the XMEM form -----------------------------------------------------

O_PROJ_KEYS = {"exl2": dense(8, 2, xmem=True), "gptq": dense(8, 2, gptq=True, xmem=True)}


@pytest.mark.parametrize("fmt", list(O_PROJ_KEYS))
def test_o_proj_two_tiles_operands_from_memory(be, fmt, monkeypatch):
    """exl2_q_attn_forward_2_chain (x += attn_out . Wo, then the hand-off for the next consumer) at a hidden size above 8192: a
    chain-out launch may publish 512 partial sums of squares per row, so from 513 tiles on a workgroup takes two tiles -- in the XMEM
    form that is a kernel of its own, which no model of the suite is wide enough to reach.  K = 1024 (every wave of a tile has a share), 8320 columns,
    5 rows; x against the float64 result of tests/test_qattn_op.py::test_forward_2_residual at the bar of the chained one-matrix launches
    (slack * half_tol, as in test_one_matrix_kernel: this is one), the hand-off against x."""
    from exllamav2_amd.ext import none_tensor
    hid, nh, hd, rows = 8320, 8, 128, 5
    mats, keep = {}, []
    for i, (name, k, n) in enumerate((("q", hid, nh * hd), ("k", hid, nh * hd), ("v", hid, nh * hd), ("o", nh * hd, hid))):
        if fmt == "gptq":
            t = OX.synth_gptq(k, n, 32, seed=70 + i, act_order=True)
            t["scales"] = (t["scales"].astype(np.float32) * 0.6).astype(np.float16)      # (as in _matrix)
            if name in "kv": t["g_idx"] = shared.copy()                 # (q, k and v of a checkpoint share their permutation: chain-capable)
            shared = t["g_idx"]
            ref, w = OX.gptq_reconstruct(t), gptq_to_torch(be, t)
            perm = OX.gptq_sequential_perm(t["g_idx"], k // 32)[0].astype(np.int64)
        else:
            t = OX.synth_exl2(k, n, [(5, 32, 32), (4, 32, k - 32)], seed=70 + i, act_order=True, sigma=0.06)
            if name in "kv": t["q_invperm"] = shared.copy()
            shared = t["q_invperm"]
            ref, w = OX.exl2_reconstruct(t), exl2_to_torch(be, t)
            perm = np.argsort(t["q_invperm"]).astype(np.int64)
        mats[name] = (ref, perm, be.ext.make_q_matrix_from_dict(w, None))
        keep.append(w)
    rng = np.random.default_rng(7)
    nw = be.t((1 + 0.1 * rng.standard_normal(hid)).astype(np.float16))
    temp_state = torch.zeros((16, hid), dtype=torch.float16, device=be.device)
    h = be.ext.make_q_attn(nw, none_tensor, True, False, 1e-5, mats["q"][2], mats["k"][2], mats["v"][2], mats["o"][2], temp_state, none_tensor,
                           16, hid, nh, nh, hd, 64, True, 2, hd, none_tensor, none_tensor, none_tensor, none_tensor, False, False)
    ref_o, perm_o, _ = mats["o"]
    x = rng.standard_normal((rows, hid)).astype(np.float16)
    a = rng.standard_normal((rows, nh * hd)).astype(np.float16)
    next_w = (1 + 0.1 * rng.standard_normal(hid)).astype(np.float16)
    xt, xp_out = be.t(x), torch.zeros((rows, hid), dtype=torch.float16, device=be.device)
    ss_out = torch.zeros((rows, 512), dtype=torch.float32, device=be.device)
    monkeypatch.setenv("EXL2_LEAN_XMEM", "2")
    be.ext.lean_kernel_counts(reset=True)
    npart = be.ext.q_attn_forward_2_chain(h, xt, be.t(a[:, perm_o]), rows, None, be.t(next_w), xp_out, ss_out)
    assert launched(be) == {O_PROJ_KEYS[fmt]: 1}
    want = OX.gemm_ref(a, ref_o, c_in=x, exact=True)
    got = be.n(xt)
    k = nh * hd
    err = np.abs(got.astype(np.float64) - want) / (2 * max(1.0, (k / 1024.0) ** 0.5) * half_tol(want, k))
    assert np.all(err <= 1.0), float(err.max())
    # the hand-off is made from the sums the launch stored: x times the norm weight (fp32 product, one rounding), sum of x^2 as 260 partials per row, row after row
    assert npart == hid // 32 and npart <= 512
    assert np.array_equal(be.n(xp_out).view(np.uint16), (got.astype(np.float32) * next_w.astype(np.float32)).astype(np.float16).view(np.uint16))
    assert np.allclose(be.n(ss_out).reshape(-1)[:rows * npart].reshape(rows, npart).sum(-1, dtype=np.float64), (got.astype(np.float64) ** 2).sum(-1), rtol=2.0 ** -18, atol=0)
    be.ext.free_q_attn(h)
    for _, _, hm in mats.values():
        be.ext.free_q_matrix(hm)
