"""Non-absorbed MLA prefill on the CPU: the host-built plan, and the
tiny-deepseek-v3-wide engine with the path on against the path off (the
reference ops in fp32 evaluate the same math both ways)."""

import pytest
import torch

import arks_amd.ops as ops
from arks_amd.config import EngineConfig
from arks_amd.engine import LLMEngine, SamplingParams


def plan(q_lens, kv_lens, min_q, max_rows=10**6, qtile=None):
    return ops.build_mla_prefill_plan(q_lens, kv_lens, 4, "cpu", min_q,
                                      max_rows, qtile)


def test_plan_selection():
    assert plan([1, 4, 63], [50, 9, 63], 64) is None
    assert plan([300], [300], 0) is None            # 0 turns the path off
    p = plan([63, 64, 1, 200], [63, 100, 30, 200], 64)  # edge: q_len == min_q
    assert p.seqs == [1, 3] and p.total_kv == 300
    assert p.cu_seqlens_kv.tolist() == [0, 0, 100, 100, 300]
    assert p.rest_rows.tolist() == list(range(63)) + [127]
    assert p.rest_seqs.tolist() == [0, 2] and p.rest_cu.tolist() == [0, 63, 64]
    # the row cap: the second sequence no longer fits and stays absorbed,
    # the third still does
    p = plan([100, 100, 80], [100, 150, 80], 64, max_rows=200)
    assert p.seqs == [0, 2] and p.cu_seqlens_kv.tolist() == [0, 100, 100, 180]
    assert plan([100], [150], 64, max_rows=149) is None
    p = plan([70, 90], [70, 90], 1)                 # everything selected
    assert p.rest_rows is None and p.rest_seqs is None and p.rest_cu is None


@pytest.mark.parametrize("qtile", [None, 128, 256])
def test_plan_tiles_cover_every_row_once(qtile):
    q_lens, kv_lens = [300, 5, 128, 257], [377, 70, 128, 1000]
    p = plan(q_lens, kv_lens, 100, qtile=qtile)
    assert p.seqs == [0, 2, 3] and p.qtile == (qtile or 128)
    rows = sorted((s, r) for s, q0 in p.tiles.tolist()
                  for r in range(q0, min(q0 + p.qtile, q_lens[s])))
    assert rows == [(s, r) for s in p.seqs for r in range(q_lens[s])]
    depth = [min(kv_lens[s], kv_lens[s] - q_lens[s] + q0 + p.qtile)
             for s, q0 in p.tiles.tolist()]
    assert depth == sorted(depth, reverse=True)      # deepest tiles first
    # enough 256-row tiles x heads to fill the chip: the tall tile
    assert ops.build_mla_prefill_plan([4096], [4096], 16, "cpu", 1,
                                      10**6).qtile == 256


@pytest.mark.parametrize("min_q", [1, 2])
def test_engine_matches_absorbed_path(min_q):
    """Log-probabilities of the whole vocabulary at every step: a 40-token
    prompt, a prompt sharing its first 32 tokens (prefix cache hit), and a
    step that mixes the running decode with a new prompt. min_q = 2 keeps
    the decode row of the mixed step on the absorbed path."""
    first = [(7 * i + 3) % 500 for i in range(40)]

    def run(min_tokens):
        e = LLMEngine(EngineConfig(
            preset="tiny-deepseek-v3-wide", device="cpu", dtype="float32",
            kv_cache_blocks=32, max_model_len=128, max_num_seqs=4, seed=3,
            mla_prefill_min_tokens=min_tokens))
        sp = SamplingParams(max_tokens=3, ignore_eos=True, logprobs=512)
        e.add_request(first, sp)
        outs = []
        while e.has_work():
            outs += e.step()
        e.add_request(first[:32] + [11, 12, 13], sp)
        outs += e.step()
        e.add_request([1, 5, 9, 20, 31, 7], sp)
        while e.has_work():
            outs += e.step()
        assert e.prefix_cache_stats[0] > 0
        return torch.tensor([[o.top_logprobs[t] for t in range(512)]
                             for o in outs])

    got, want = run(min_q), run(0)
    assert got.shape == want.shape and got.shape[0] == 9
    assert (got - want).abs().max() < 1e-4
