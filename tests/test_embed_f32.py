"""exl2_embed_rows_f32 (csrc/gemma_ops.hip): out = float(table[ids]) * scale, the embedding of an fp32 residual stream
(embedding.py:184-187: `.float()`, then `*= hidden_size ** 0.5`).  One fp32 multiply per element: bit-exact against numpy's."""
import math

import numpy as np
import pytest
import torch

F16, F32 = np.float16, np.float32


@pytest.mark.parametrize("hidden", [128, 2304, 3584])
def test_embed_rows_f32_scaled(be, hidden):
    rng = np.random.default_rng(hidden)
    vocab = 37
    table = rng.standard_normal((vocab, hidden)).astype(F16)
    table[3, :3] = [65504.0, -65504.0, 0.0]
    ids = np.array([3, 0, 36, 3, 17], dtype=np.int32)
    out = torch.full((len(ids) + 1, hidden), 7.0, dtype=torch.float32, device=be.device)
    be.ext.embed_rows_f32(be.t(table), be.t(ids), out[:len(ids)], math.sqrt(hidden))
    want = table[ids].astype(F32) * F32(math.sqrt(hidden))
    got = be.n(out)
    assert np.array_equal(got[:len(ids)].view(np.uint32), want.view(np.uint32))
    assert np.all(got[len(ids)] == 7.0)                                  # the row behind the last one is not touched
    # scale 1: a plain widening gather
    be.ext.embed_rows_f32(be.t(table), be.t(ids), out[:len(ids)], 1.0)
    assert np.array_equal(be.n(out)[:len(ids)], table[ids].astype(F32))


def test_embed_rows_f32_out_of_range_ids(be):
    """an id outside the table reads the row exl2_embed_rows reads for it"""
    rng = np.random.default_rng(1)
    vocab, hidden = 11, 128
    table = rng.standard_normal((vocab, hidden)).astype(F16)
    ids = np.array([-5, 0, 10, 11, 4000], dtype=np.int32)
    half = torch.zeros((len(ids), hidden), dtype=torch.float16, device=be.device)
    be.ext.embed_rows(be.t(table), be.t(ids), half)
    out = torch.zeros((len(ids), hidden), dtype=torch.float32, device=be.device)
    be.ext.embed_rows_f32(be.t(table), be.t(ids), out, 2.0)
    assert np.array_equal(be.n(out), be.n(half).astype(F32) * F32(2.0))
    assert np.array_equal(be.n(half), table[np.clip(ids, 0, vocab - 1)])


def test_embed_rows_f32_refusals(be):
    table = torch.zeros((4, 128), dtype=torch.float16, device=be.device)
    ids = torch.zeros((2,), dtype=torch.int32, device=be.device)
    with pytest.raises(RuntimeError, match="dtype"):
        be.ext.embed_rows_f32(table, ids, torch.zeros((2, 128), dtype=torch.float16, device=be.device))
    with pytest.raises(RuntimeError, match="multiple of 8"):
        be.ext.embed_rows_f32(torch.zeros((4, 100), dtype=torch.float16, device=be.device), ids,
                              torch.zeros((2, 100), dtype=torch.float32, device=be.device))
