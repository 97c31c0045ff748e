"""The skinny GEMM's routing rule (ops._skinny_plan) against a literal table,
and the ARKS_SKINNY_TALLK_V gate. No GPU and no extension needed."""

import os
import subprocess
import sys

import pytest

import arks_amd.ops as ops

# (M, N, K) -> (config, nsplits, k_per_split, mrows). Generated from the
# commit before _skinny_plan existed: its ops.skinny_gemm was run on the CPU
# (meta tensors) against a recording stand-in for the extension, deferred and
# not, and the binding it called (plain = config 0, variant 7 = config 1),
# its split arguments and the slab height it sized the workspace and the
# handle with were noted down.
PLAN_TABLE = [
    # the Qwen2.5-7B decode projections: qkv, o_proj, down_proj
    ((64, 4608, 3584), (0, 8, 448, 64)),
    ((64, 3584, 3584), (0, 10, 384, 64)),
    ((17, 3584, 3584), (0, 10, 384, 32)),
    ((64, 3584, 18944), (1, 8, 2368, 64)),
    ((37, 3584, 18944), (0, 10, 1920, 48)),
    ((64, 37888, 3584), (0, 1, 3584, 64)),   # ntiles >= 384: no split
    ((4, 64, 512), (0, 2, 256, 16)),
    # the remaining shapes of test_ops_gpu.py::test_skinny_gemm
    ((1, 4608, 3584), (0, 8, 448, 16)),
    ((5, 64, 96), (0, 1, 96, 16)),
    ((33, 152064, 3584), (0, 1, 3584, 48)),
    ((64, 64, 128), (1, 1, 128, 64)),        # tall-K that ends up unsplit
    # the M > 48 boundary of the tall-K gate
    ((48, 3584, 18944), (0, 10, 1920, 48)),
    ((49, 3584, 18944), (1, 8, 2368, 64)),
    # shapes of test_splitk_fused_gpu.py, a K == N + 32 tall-K, and K >> N
    # above the 128-tile limit of the gate
    ((64, 256, 1024), (1, 4, 256, 64)),
    ((5, 64, 8192), (0, 32, 256, 16)),
    ((17, 192, 416), (0, 2, 224, 32)),       # round-to-32 of an uneven split
    ((1, 64, 512), (0, 2, 256, 16)),
    ((16, 128, 256), (0, 1, 256, 16)),
    ((64, 8192, 28672), (0, 4, 7168, 64)),
    ((49, 8128, 8160), (1, 4, 2048, 64)),
]


@pytest.mark.parametrize("shape,plan", PLAN_TABLE)
def test_skinny_plan_table(monkeypatch, shape, plan):
    monkeypatch.setattr(ops, "_SKINNY_TALLK_CONFIG", 1)
    assert ops._skinny_plan(*shape) == plan
    config, nsplits, k_per_split, mrows = plan
    K = shape[2]
    assert k_per_split % 32 == 0 and (nsplits - 1) * k_per_split < K
    assert nsplits * k_per_split >= K and shape[0] <= mrows <= 64


def test_non_temporal_choice_only_changes_the_tall_k_config(monkeypatch):
    monkeypatch.setattr(ops, "_SKINNY_TALLK_CONFIG", 2)
    for shape, plan in PLAN_TABLE:
        want = (2,) + plan[1:] if plan[0] == 1 else plan
        assert ops._skinny_plan(*shape) == want


def _import_ops_with(value):
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, ARKS_SKINNY_TALLK_V=value,
               HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    return subprocess.run(
        [sys.executable, "-c",
         "import arks_amd.ops as o; print('config', o._SKINNY_TALLK_CONFIG)"],
        cwd=repo, env=env, capture_output=True, text=True, timeout=120)


def test_tallk_env_rejects_values_of_removed_kernels():
    # read at import, so each value needs a fresh interpreter
    out = _import_ops_with("3")
    assert out.returncode != 0
    assert "ValueError" in out.stderr and "ARKS_SKINNY_TALLK_V" in out.stderr
    # names what is accepted
    assert "accepted values are 7" in out.stderr and "and 8" in out.stderr
    out = _import_ops_with("8")
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == ["config", "2"]
