"""The driver's bench contract, exercised for real: `bench.py` launched
under `torch.distributed.run` with world_size 2 (gloo, CPU, tiny preset) —
the exact shape of the driver's round-end SCALE run (which has never had
an 8-GPU node to run on), minus the GPUs. Asserts the single JSON line,
dp token aggregation across ranks, and the contract fields."""

import json
import os
import socket
import subprocess
import sys


def _free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


# gloo/CPU runs on every machine: the benchmark processes see no GPU, so a
# host with fewer GPUs than ranks runs them exactly as a host with none
_NO_GPU = {"HIP_VISIBLE_DEVICES": "-1", "CUDA_VISIBLE_DEVICES": "-1"}


def _run_bench(mode: str):
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", **_NO_GPU)
    cmd = [
        sys.executable, "-m", "torch.distributed.run",
        "--nnodes=1", "--nproc-per-node", "2",
        "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
        os.path.join(repo, "bench.py"),
        "--gpus", "2", "--steps", "3", "--warmup", "1",
        "--batch", "2", "--input-len", "32", "--model", "tiny",
        "--parallel", mode,
    ]
    return subprocess.run(cmd, cwd=repo, env=env, capture_output=True,
                          text=True, timeout=420)


def test_bench_dp2_gloo_contract():
    out = _run_bench("dp")
    assert out.returncode == 0, f"bench failed:\n{out.stdout}\n{out.stderr}"
    lines = [ln for ln in out.stdout.splitlines()
             if ln.startswith("{") and '"metric"' in ln]
    assert len(lines) == 1, f"expected exactly one JSON line:\n{out.stdout}"
    rec = json.loads(lines[0])
    assert rec["metric"] == "output_tok_s"
    assert rec["n_gpus"] == 2
    assert rec["steps"] == 3 and rec["warmup"] == 1
    assert rec["scaling"] == "weak"
    assert rec["higher_is_better"] is True
    assert rec["dtype"] == "bf16" and rec["data"] == "synthetic"
    assert rec["value"] > 0 and rec["ms_per_step"] > 0
    # dp aggregation: whole-job tokens = batch * steps * world / elapsed —
    # value must reflect BOTH ranks (2 * 2 * 3 tokens over the window)
    expected_tokens = 2 * 2 * 3
    approx_tokens = rec["value"] * (rec["ms_per_step"] * 3 / 1000.0)
    assert abs(approx_tokens - expected_tokens) / expected_tokens < 0.05


def _run_single(tmp_path, name, *extra):
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dump = tmp_path / name
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    env.update(_NO_GPU)
    out = subprocess.run(
        [sys.executable, os.path.join(repo, "bench.py"),
         "--gpus", "1", "--steps", "3", "--warmup", "1",
         "--batch", "3", "--input-len", "24", "--model", "tiny",
         "--dump-outputs", str(dump), *extra],
        cwd=repo, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, f"bench failed:\n{out.stdout}\n{out.stderr}"
    lines = [ln for ln in out.stdout.splitlines()
             if ln.startswith("{") and '"metric"' in ln]
    assert len(lines) == 1, f"expected exactly one JSON line:\n{out.stdout}"
    return json.loads(lines[0]), dump


def test_bench_dump_outputs_repeatable(tmp_path):
    """--dump-outputs writes the last timed step's outputs as float .npy
    files; the same arguments give the same arrays from run to run, and
    --full keeps the headline line's meaning."""
    import numpy as np

    rec_a, dump_a = _run_single(tmp_path, "a")
    rec_b, dump_b = _run_single(tmp_path, "b", "--full")
    for rec in (rec_a, rec_b):
        assert rec["metric"] == "output_tok_s" and rec["unit"] == "tok/s"
        assert rec["steps"] == 3 and rec["warmup"] == 1
        assert rec["higher_is_better"] is True and rec["dtype"] == "bf16"
        assert rec["ms_per_step"] > 0
        # value is tokens / elapsed over exactly --steps timed steps
        tokens = rec["value"] * rec["ms_per_step"] * 3 / 1000.0
        assert abs(tokens - 3 * 3) / 9 < 0.05
    names = sorted(p.name for p in dump_a.iterdir())
    assert names == sorted(p.name for p in dump_b.iterdir())
    assert "new_token_ids.npy" in names
    total = 0
    for name in names:
        a, b = np.load(dump_a / name), np.load(dump_b / name)
        assert a.dtype in (np.float32, np.float64)
        assert a.shape == b.shape and np.array_equal(a, b), name
        total += a.nbytes
    assert total <= 64 * 1024 * 1024
    assert np.load(dump_a / "new_token_ids.npy").shape == (3,)
    assert np.load(dump_a / "request_index.npy").tolist() == [0.0, 1.0, 2.0]


def test_bench_tp2_gloo_contract():
    """The TP bench path (one engine sharded over both ranks): rank 0
    emits the JSON line with strong scaling and un-multiplied tokens."""
    out = _run_bench("tp")
    assert out.returncode == 0, f"bench failed:\n{out.stdout}\n{out.stderr}"
    lines = [ln for ln in out.stdout.splitlines()
             if ln.startswith("{") and '"metric"' in ln]
    assert len(lines) == 1, f"expected exactly one JSON line:\n{out.stdout}"
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2
    assert rec["scaling"] == "strong"
    assert rec["config"]["parallelism"] == "tp2"
    assert rec["config"]["global_batch"] == 2
    assert rec["value"] > 0
