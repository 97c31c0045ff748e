"""The split-K pending-result handle's ordering check, on the Python side of
the wrapper: a stale handle must raise before anything reaches the native
extension. A recording stand-in replaces the extension, so no GPU is needed."""

import pytest
import torch

import arks_amd.ops as ops


class _RecordingNative:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def op(*args):
            self.calls.append(name)
        return op


@pytest.fixture
def native(monkeypatch):
    fake = _RecordingNative()
    monkeypatch.setattr(ops, "_native", lambda: fake)
    monkeypatch.setattr(ops, "_SKINNY_WS", {})
    monkeypatch.setattr(ops, "_SKINNY_WS_GEN", {})
    return fake


def _operands():
    x = torch.zeros(4, 512, dtype=torch.bfloat16)
    w = torch.zeros(64, 512, dtype=torch.bfloat16)
    res = torch.zeros(4, 64, dtype=torch.bfloat16)
    nw = torch.ones(64, dtype=torch.bfloat16)
    return x, w, res, nw


def test_live_handle_reaches_the_fused_kernels(native):
    x, w, res, nw = _operands()
    h = ops.skinny_gemm(x, w, defer=True)
    assert isinstance(h, ops.SplitKPending)
    assert (h.nsplits, h.mrows, h.shape) == (2, 16, (4, 64))
    ops.fused_add_rmsnorm(h, res, nw)
    h.materialize()
    assert native.calls == ["skinny_gemm_partials", "splitk_add_rmsnorm",
                            "skinny_combine"]


def test_stale_handle_raises_and_launches_nothing(native):
    x, w, res, nw = _operands()
    h1 = ops.skinny_gemm(x, w, defer=True)
    h2 = ops.skinny_gemm(x, w, defer=True)  # overwrites the workspace
    launched = list(native.calls)
    assert launched == ["skinny_gemm_partials"] * 2
    with pytest.raises(RuntimeError, match="stale split-K handle"):
        ops.fused_add_rmsnorm(h1, res, nw)
    with pytest.raises(RuntimeError, match="stale split-K handle"):
        ops.rope_and_cache_splitk(None, h1, None, None, None, None, 64, 1)
    with pytest.raises(RuntimeError, match="stale split-K handle"):
        h1.materialize()
    assert native.calls == launched
    ops.fused_add_rmsnorm(h2, res, nw)
    assert native.calls == launched + ["splitk_add_rmsnorm"]


def test_materialising_gemm_also_retires_handles(native):
    x, w, res, nw = _operands()
    h = ops.skinny_gemm(x, w, defer=True)
    ops.skinny_gemm(x, w)  # plain call: GEMM + combine through the same ws
    with pytest.raises(RuntimeError, match="stale split-K handle"):
        ops.fused_add_rmsnorm(h, res, nw)


def test_unsplit_gemm_returns_a_tensor(native):
    # N = 64 * 384 tiles: nsplits == 1, nothing to defer
    x = torch.zeros(4, 64, dtype=torch.bfloat16)
    w = torch.zeros(64 * 384, 64, dtype=torch.bfloat16)
    y = ops.skinny_gemm(x, w, defer=True)
    assert isinstance(y, torch.Tensor) and y.shape == (4, 64 * 384)
