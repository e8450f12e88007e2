"""Tensor parallel with the q / k head norm (world_size 2, gloo, CPU emulation backend): each rank normalises ITS heads with its rows
of the per-head weights (tensor_p.TPAttention) and must produce the single-process model's logits."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.conftest import ROOT, build_emu_if_needed
from tests.test_tensor_p import LOGIT_TOL, PROMPT, N_DECODE, _emu_ext


def _cfg():
    from exllamav2_amd.config import ExLlamaV2Config
    return ExLlamaV2Config(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=4,
                           num_key_value_heads=2, head_dim=64, vocab_size=120, max_seq_len=256, max_input_len=32, use_qk_norm=True)


def _checkpoint(cfg):
    from exllamav2_amd.synth import synth_checkpoint
    return synth_checkpoint(cfg, "cpu", seed=9)


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from exllamav2_amd.cache import ExLlamaV2Cache
    from exllamav2_amd.tensor_p import ExLlamaV2TP, TPGreedyDecoder
    cfg = _cfg()
    ck = _checkpoint(cfg)
    model = ExLlamaV2TP(cfg, rank, world, device="cpu", ext=_emu_ext()).load(ck)
    for i, (attn, _) in enumerate(model.layers):
        # this rank's heads: rows [rank * H / N, (rank + 1) * H / N) of the per-head weights
        full_q, full_k = ck[f"model.layers.{i}.self_attn.q_norm"], ck[f"model.layers.{i}.self_attn.k_norm"]
        assert torch.equal(attn.q_norm, full_q[2 * rank:2 * rank + 2]) and torch.equal(attn.k_norm, full_k[rank:rank + 1])
    cache = ExLlamaV2Cache(model, batch_size=1, max_seq_len=256)
    logits = model.forward(torch.tensor([PROMPT]), cache, last_id_only=False)
    dec = TPGreedyDecoder(model, cache, batch_size=1)
    dec.reset(torch.tensor([int(torch.argmax(logits[0, -1]))]), len(PROMPT))
    dec.run(N_DECODE)
    np.save(os.path.join(out_dir, f"logits{rank}.npy"), logits.float().numpy())
    np.save(os.path.join(out_dir, f"tokens{rank}.npy"), dec.tokens(len(PROMPT), N_DECODE).numpy())
    dist.barrier()
    dist.destroy_process_group()


def test_tensor_parallel_with_head_norm_matches_single_process(tmp_path):
    world = 2
    build_emu_if_needed()
    mp.spawn(_worker, args=(world, 29561, str(tmp_path)), nprocs=world, join=True)
    l0, l1 = (np.load(tmp_path / f"logits{r}.npy") for r in range(world))
    t0, t1 = (np.load(tmp_path / f"tokens{r}.npy") for r in range(world))
    assert np.array_equal(l0, l1) and np.array_equal(t0, t1)                         # ranks agree bit for bit

    from exllamav2_amd.cache import ExLlamaV2Cache
    from exllamav2_amd.model import ExLlamaV2
    from tests.qk_norm_oracle import QKNormOracleModel
    cfg = _cfg()
    ck = _checkpoint(cfg)
    oracle = QKNormOracleModel(cfg, ck)
    oracle.reset(1)
    want = oracle.forward(np.array([PROMPT]))
    assert np.abs(l0.astype(np.float64) - want).max() < LOGIT_TOL                    # vs the CPU oracle
    model = ExLlamaV2(cfg, device="cpu", ext=_emu_ext()).load(ck)
    cache = ExLlamaV2Cache(model, batch_size=1, max_seq_len=256)
    single = model.forward(torch.tensor([PROMPT]), cache, last_id_only=False).float().numpy()
    assert np.abs(l0 - single).max() < LOGIT_TOL                                     # vs the single-process product path
    # ... and the norm is in the result: the same weights without it are far away
    from oracle.model import OracleModel
    plain = OracleModel(cfg, {k: v for k, v in _checkpoint(cfg).items() if not k.endswith(("q_norm", "k_norm"))})
    plain.reset(1)
    assert np.abs(plain.forward(np.array([PROMPT])) - want).max() > 4 * LOGIT_TOL
    # greedy tokens wherever the oracle's top-1 / top-2 margin exceeds 4x the logit tolerance
    tok = int(np.argmax(l0[0, -1]))
    checked = 0
    for i in range(N_DECODE):
        w = oracle.forward(np.array([[tok]]))[0, -1]
        top = np.sort(w)[-2:]
        if top[1] - top[0] > 4 * LOGIT_TOL:
            assert int(t0[0, i]) == int(np.argmax(w))
            checked += 1
        tok = int(t0[0, i])
    assert checked >= 1, "vacuous token check"
    model.unload()
