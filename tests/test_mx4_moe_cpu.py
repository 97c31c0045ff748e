"""MX4 MoE experts on the CPU: the references of the two routed grouped GEMMs,
and how an MXFP4 MoE checkpoint loads into the stacked MX4 storage of MoEMLP
(the CPU forward runs on exact bf16 stand-ins, so a checkpoint and its
dequantized twin compare bit for bit)."""

import dataclasses
import logging
import os

import pytest
import torch

import arks_amd.ops as ops
from arks_amd.config import PRESET_CONFIGS, ModelConfig
from arks_amd.loader.safetensors_loader import (load_model_weights,
                                                save_mx4_checkpoint)
from arks_amd.models import create_model
from arks_amd.ops import ref

CPU = torch.device("cpu")


@pytest.mark.parametrize("src_div", [2, 1])
def test_ref_moe_gemms_equal_a_loop_over_pairs(src_div):
    """Local experts are global ids 1 and 2 of 4: other pairs keep `out`."""
    E, n, kk, k, T, base = 2, 64, 256, 2, 9, 1
    g = torch.Generator().manual_seed(5)
    qs = [ref.mx4_quantize(torch.randn(n, kk, generator=g) * 0.05)
          for _ in range(E)]
    weight = tuple(torch.stack(t) for t in zip(*qs))
    ids = torch.rand(T, 4, generator=g).topk(k, dim=-1).indices.to(torch.int32)
    counts, pairs = ref.moe_route(ids, base, E)
    a = (torch.randn(T * k // src_div, kk, generator=g) * 0.5).to(
        torch.bfloat16)
    xq, xs = ref.mx4_quantize(a)
    sentinel = torch.full((T * k, n), -3.0, dtype=torch.bfloat16)
    a16 = ops.mx4_moe_gemm(a, weight, counts, pairs, src_div, T,
                           out=sentinel.clone())
    a4 = ops.mx4a4_moe_gemm(xq, xs, weight, counts, pairs, src_div, T,
                            out=sentinel.clone())
    flat = ids.reshape(-1)
    touched = 0
    for p in range(T * k):
        le = int(flat[p]) - base
        if not 0 <= le < E:
            assert (a16[p] == -3.0).all() and (a4[p] == -3.0).all(), p
            continue
        touched += 1
        w = ref.mx4_dequant(weight[0][le], weight[1][le])
        for got, act in ((a16, a.float()), (a4, ref.mx4_dequant(xq, xs))):
            expect = (act[p // src_div] @ w.t()).to(torch.bfloat16)
            assert torch.equal(got[p], expect), p
    assert 0 < touched < T * k


def _load(cfg, tmp_path, mutate=None, **save_kw):
    """(model from an MXFP4 checkpoint with MX4 experts, its bf16 twin)."""
    from safetensors.torch import load_file, save_file

    mx4, bf16 = str(tmp_path / "mx4"), str(tmp_path / "bf16")
    save_mx4_checkpoint(cfg, mx4, seed=6, dequantized_dir=bf16, **save_kw)
    if mutate is not None:
        f = os.path.join(mx4, "model.safetensors")
        st = load_file(f)
        mutate(st)
        save_file(st, f)
    ours = create_model(ModelConfig.from_pretrained(mx4))
    ours.prepare_mxfp4_checkpoint(experts=True)
    load_model_weights(ours, mx4, CPU)
    ours.finalize_mx4()
    twin = create_model(cfg)
    load_model_weights(twin, bf16, CPU)
    return ours, twin


@pytest.mark.parametrize("preset", ["tiny-qwen3moe-w4", "tiny-qwen2moe-w4"])
def test_checkpoint_loads_into_stacked_mx4_experts(tmp_path, preset, caplog):
    with caplog.at_level(logging.WARNING):
        ours, twin = _load(PRESET_CONFIGS[preset], tmp_path)
    assert not [r for r in caplog.records if "dequantized" in r.message]
    torch.manual_seed(1)
    for lo, lt in zip(ours.layers, twin.layers):
        moe, plain = lo.mlp, lt.mlp
        E, H, I = moe.local_experts, moe.hidden, moe.inter
        assert moe.mx4 and not moe.w4 and not moe.w8 and not plain.mx4
        assert "w13" not in dict(moe.named_parameters())
        assert moe.w13_mx4.shape == (E, 2 * I, H // 2)
        assert moe.w2_mx4_scales.shape == (E, H, I // 32)
        for which in ("w13", "w2"):
            full = getattr(plain, which).data
            assert torch.equal(getattr(moe, which), full)   # the stand-ins
            q, s = moe.mx4_weight(which)
            assert q.dtype == s.dtype == torch.uint8
            for e in range(E):
                # blocks run along K, so gate | up quantize as one tensor
                want_q, want_s = ref.mx4_quantize(full[e].t())
                assert torch.equal(q[e], want_q) and torch.equal(s[e], want_s)
        x = torch.randn(5, H).to(torch.bfloat16)
        assert torch.equal(moe(x), plain(x))


@pytest.mark.parametrize("how", ["missing", "255"])
def test_missing_or_nan_expert_scale_raises_naming_it(tmp_path, how):
    name = "model.layers.1.mlp.experts.2.down_proj.weight_scale"

    def mutate(st):
        if how == "missing":
            del st[name]
        else:
            st[name][3, 0] = 255

    with pytest.raises(ValueError) as ei:
        _load(PRESET_CONFIGS["tiny-qwen3moe-w4"], tmp_path, mutate=mutate)
    assert name in str(ei.value) and (how == "missing" or "255" in str(ei.value))


def test_unsupported_width_falls_back_and_warns_with_the_width(tmp_path,
                                                               caplog):
    cfg = dataclasses.replace(PRESET_CONFIGS["tiny-qwen3moe-w4"],
                              moe_intermediate_size=192)
    assert not ops.mx4_moe_supported(192, cfg.hidden_size)
    with caplog.at_level(logging.WARNING):
        ours, twin = _load(cfg, tmp_path)
    said = [r.getMessage() for r in caplog.records
            if "dequantized to bf16" in r.message]
    assert len(said) == 1 and "expert width=192" in said[0]
    moe = ours.layers[0].mlp
    assert not moe.mx4 and "w13" in dict(moe.named_parameters())
    assert torch.equal(moe.w13, twin.layers[0].mlp.w13)
    assert ours.layers[0].self_attn.qkv_proj.mx4
