"""W8 MoE experts under tensor parallelism (world_size=2 over gloo, CPU):
loading a block-scaled FP8 MoE checkpoint, every rank holds the e4m3 bytes
of its own experts only, the shared expert is split like a dense MLP, and
the TP=2 greedy tokens must equal TP=1.

The model is `tiny-qwen2moe-w4`: 8 heads x 32 and a shared width of 256
leave whole 128-blocks per rank."""

import multiprocessing as mp
import os
import socket

import pytest
import torch

from arks_amd.config import PRESET_CONFIGS

PROMPTS = [[1, 5, 9, 20, 31, 7], [3, 3, 7, 90]]
MAX_TOKENS = 6
PRESET = "tiny-qwen2moe-w4"


@pytest.fixture(autouse=True)
def _cpu_only_workers(monkeypatch):
    """gloo/CPU tests on every machine: the spawned ranks inherit an
    environment that hides any GPU."""
    monkeypatch.setenv("HIP_VISIBLE_DEVICES", "-1")
    monkeypatch.setenv("CUDA_VISIBLE_DEVICES", "-1")


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _generate(path, rank, world):
    """(tokens, local experts held) of one engine on the FP8 checkpoint at
    `path`; asserts that the rank's stacked buffers are the checkpoint's
    bytes of its own experts."""
    from safetensors.torch import load_file

    from arks_amd.config import EngineConfig
    from arks_amd.engine import LLMEngine, SamplingParams

    torch.manual_seed(0)
    e = LLMEngine(EngineConfig(device="cpu", kv_cache_blocks=128,
                               max_model_len=256, seed=2, model_path=path))
    assert e.runner.quantization == "fp8_block"
    moe = e.runner.model.layers[0].mlp
    assert moe.w8 and moe.shared.down_proj.w8
    assert "w13" not in dict(moe.named_parameters())
    El, I = moe.local_experts, moe.inter
    assert moe.expert_base == rank * El
    assert moe.w13_w8.shape[0] == El and moe.w2_w8_scales.shape[0] == El
    st = load_file(os.path.join(path, "model.safetensors"))
    for le in range(El):
        pre = f"model.layers.0.mlp.experts.{moe.expert_base + le}"
        for rows, name in ((moe.w13_w8[le, :I], "gate_proj"),
                           (moe.w13_w8[le, I:], "up_proj"),
                           (moe.w2_w8[le], "down_proj")):
            assert torch.equal(rows.view(torch.uint8),
                               st[f"{pre}.{name}.weight"].view(torch.uint8))
    out = e.generate(PROMPTS, SamplingParams(max_tokens=MAX_TOKENS,
                                             ignore_eos=True))
    return out, El * world


def _tp_worker(rank: int, world: int, port: int, q, path):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["RANK"] = str(rank)
    os.environ["WORLD_SIZE"] = str(world)
    try:
        from arks_amd.parallel import comm

        comm.init_tp(backend="gloo")
        out = ("ok", _generate(path, rank, world))
        if rank == 0:
            q.put(out)
        comm.destroy_tp()
    except Exception as e:  # pragma: no cover
        import traceback

        q.put(("err", f"{e}\n{traceback.format_exc()}"))


def _run_tp2(path):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_tp_worker, args=(r, 2, port, q, path))
             for r in range(2)]
    for p in procs:
        p.start()
    status, payload = q.get(timeout=150)
    for p in procs:
        p.join(timeout=60)
    return status, payload


@pytest.mark.timeout(180)
def test_tp2_fp8_moe_checkpoint_matches_tp1_gloo(tmp_path):
    from arks_amd.loader.safetensors_loader import save_fp8_checkpoint

    cfg = PRESET_CONFIGS[PRESET]
    path = str(tmp_path / "fp8")
    save_fp8_checkpoint(cfg, path, seed=6)
    ref, total = _generate(path, 0, 1)
    assert total == cfg.num_local_experts
    assert all(len(o) == MAX_TOKENS for o in ref)
    status, payload = _run_tp2(path)
    assert status == "ok", payload
    out, total2 = payload
    assert total2 == cfg.num_local_experts  # half of the experts per rank
    assert out == ref, f"TP=2 output {out} != TP=1 {ref}"
