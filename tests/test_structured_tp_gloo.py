"""Structured outputs under tensor parallelism (world_size=2 over gloo,
CPU): every rank builds the token table and the masks on its own, and both
must emit the same valid document with no extra broadcast."""

import multiprocessing as mp
import os
import socket

import pytest
import torch

from structured_testutil import MAX_TOKENS, SPECS, check, decode, longest

PROMPT = [10, 50, 99, 7, 120]


@pytest.fixture(autouse=True)
def _cpu_only_workers(monkeypatch):
    monkeypatch.setenv("HIP_VISIBLE_DEVICES", "-1")
    monkeypatch.setenv("CUDA_VISIBLE_DEVICES", "-1")


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _generate():
    from arks_amd.config import EngineConfig
    from arks_amd.engine import LLMEngine, SamplingParams

    torch.manual_seed(0)
    # no set_tokenizer: like a TP worker rank, the engine derives the token
    # table from load_tokenizer(cfg.model_path, ...) itself
    e = LLMEngine(EngineConfig(preset="tiny", device="cpu", kv_cache_blocks=256,
                               max_model_len=512))
    sps = [SamplingParams(max_tokens=MAX_TOKENS, structured=SPECS["json_schema"]),
           SamplingParams(max_tokens=MAX_TOKENS, structured=SPECS["regex"],
                          temperature=1.0, seed=7)]
    seqs = [e.add_request(list(PROMPT), sp) for sp in sps]
    while e.has_work():
        e.step()
    return [(s.output_token_ids, s.finish_reason) for s in seqs], e.model_cfg.eos_token_id


def _tp_worker(rank: int, world: int, port: int, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["RANK"] = str(rank)
    os.environ["WORLD_SIZE"] = str(world)
    try:
        from arks_amd.parallel import comm

        comm.init_tp(backend="gloo")
        out, _ = _generate()
        q.put(("ok", rank, out))
        comm.destroy_tp()
    except Exception as e:  # pragma: no cover
        import traceback

        q.put(("err", rank, f"{e}\n{traceback.format_exc()}"))


@pytest.mark.timeout(180)
def test_tp2_ranks_emit_the_same_valid_documents():
    for s in SPECS.values():
        assert MAX_TOKENS >= longest(s) + 1
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_tp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = [q.get(timeout=150) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    assert all(g[0] == "ok" for g in got), got
    outs = {g[1]: g[2] for g in got}
    assert outs[0] == outs[1]
    eos = 2
    for (toks, reason), kind in zip(outs[0], ("json_schema", "regex")):
        assert reason == "stop"
        check(kind, decode(toks, eos))
