"""Routed bf16 MoE GEMM without a GPU: the reference and the shape rule."""

import pytest
import torch

import arks_amd.ops as ops
from arks_amd.config import PRESET_CONFIGS
from arks_amd.ops import ref


@pytest.mark.parametrize("src_div", [2, 1])
def test_ref_against_einsum_and_untouched_rows(src_div):
    """Local experts are global ids 1..3; the pairs of id 0 keep what a
    passed-in `out` held. ops.moe_bf16_gemm on CPU tensors is the reference."""
    E, K, N, k, T, base = 3, 64, 128, 2, 9, 1
    g = torch.Generator().manual_seed(2)
    ids = torch.rand(T, E + 1, generator=g).topk(k, dim=-1).indices.to(
        torch.int32)
    counts, pairs = ref.moe_route(ids, base, E)
    w = (torch.randn(E, K, N, generator=g) * 0.05).to(torch.bfloat16)
    a = (torch.randn(T * k // src_div, K, generator=g) * 0.5).to(
        torch.bfloat16)
    out = torch.full((T * k, N), -3.0, dtype=torch.bfloat16)
    got = ops.moe_bf16_gemm(a, w, counts, pairs, src_div, T, out=out)
    assert got is out
    flat = ids.reshape(-1).long() - base
    assert (flat < 0).any() and (flat >= 0).any()
    src = torch.arange(T * k) // src_div
    expect = torch.einsum("pk,pkn->pn", a[src].double(),
                          w[flat.clamp(min=0)].double())
    local = flat >= 0
    torch.testing.assert_close(out[local].double(), expect[local], atol=1e-3,
                               rtol=2 ** -7)
    assert (out[~local] == -3.0).all()


def test_shape_rule_on_the_presets():
    for name in ("qwen3-30b-a3b", "mixtral-8x7b", "tiny-moe-gpu", "tiny-moe"):
        cfg = PRESET_CONFIGS[name]
        H = cfg.hidden_size
        I = cfg.moe_intermediate_size or cfg.intermediate_size
        assert ops.moe_bf16_supported(H, 2 * I), name
        assert ops.moe_bf16_supported(I, H), name
    assert ops.moe_bf16_supported(1408, 2048)       # Qwen1.5-MoE down-proj
    assert not ops.moe_bf16_supported(96, 128)      # K % 64
    assert not ops.moe_bf16_supported(64, 192)      # N % 128
    assert not ops.moe_bf16_supported(0, 128)
