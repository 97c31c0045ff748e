"""W8 MoE experts on the CPU: the reference of the routed grouped GEMM, the
W8 storage of MoEMLP and how a block-scaled FP8 MoE checkpoint loads into it.
The CPU forward of a W8 block runs the bf16 path on dequantized stand-ins, so
an FP8 checkpoint and its dequantized twin compare exactly."""

import dataclasses
import logging
import os

import pytest
import torch

import arks_amd.ops as ops
from arks_amd.config import PRESET_CONFIGS, EngineConfig
from arks_amd.engine import LLMEngine, SamplingParams
from arks_amd.loader.safetensors_loader import save_fp8_checkpoint
from arks_amd.models import create_model
from arks_amd.models.llama_family import MoEMLP
from arks_amd.ops import ref

PROMPTS = [[3, 1, 4, 1, 5], [9, 2, 6]]
SP = SamplingParams(max_tokens=6, ignore_eos=True)
MOE_PRESETS = ["tiny-qwen3moe-w4", "tiny-qwen2moe-w4"]


def _cpu_engine(**kw):
    return LLMEngine(EngineConfig(device="cpu", kv_cache_blocks=128,
                                  max_model_len=256, seed=2, **kw))


def _tensors(path):
    from safetensors.torch import load_file

    return load_file(os.path.join(path, "model.safetensors"))


def _u8(t):
    return t.view(torch.uint8)


# ------------------------------ reference op -------------------------------
def _random_experts(E, n, k, seed):
    w8s, scs = [], []
    for e in range(E):
        g = torch.Generator().manual_seed(seed + e)
        w8, blocks = ref.w8_quantize(torch.randn(n, k, generator=g) * 0.05)
        w8s.append(_u8(w8))
        scs.append(ref.w8_expand_scales(blocks, n))
    return (torch.stack(w8s).view(torch.float8_e4m3fn), torch.stack(scs))


@pytest.mark.parametrize("src_div", [2, 1])
def test_ref_moe_gemm_equals_a_loop_over_pairs(src_div):
    """Local experts are global ids 1 and 2 of 4, so some pairs belong to
    no local expert: their rows keep what `out` held."""
    E, n, kk, k, T, base = 2, 64, 256, 2, 9, 1
    w8, sc = _random_experts(E, n, kk, 3)
    g = torch.Generator().manual_seed(5)
    ids = torch.rand(T, 4, generator=g).topk(k, dim=-1).indices.to(
        torch.int32)
    counts, pairs = ref.moe_route(ids, base, E)
    a = (torch.randn(T * k // src_div, kk, generator=g) * 0.5).to(
        torch.bfloat16)
    out = torch.full((T * k, n), -3.0, dtype=torch.bfloat16)
    got = ref.w8_moe_gemm(a, (w8, sc), counts, pairs, src_div, out=out)
    assert got is out
    # the op's CPU path is the reference
    again = ops.w8_moe_gemm(a, (w8, sc), counts, pairs, src_div, T,
                            out=torch.full_like(out, -3.0))
    assert torch.equal(again, out)
    flat = ids.reshape(-1)
    touched = 0
    for p in range(T * k):
        le = int(flat[p]) - base
        if not 0 <= le < E:
            assert (out[p] == -3.0).all(), p
            continue
        touched += 1
        w = ref.w8_dequant(w8[le], sc[le])
        expect = (a[p // src_div].float() @ w.t()).to(torch.bfloat16)
        assert torch.equal(out[p], expect), p
    assert 0 < touched < T * k
    fresh = ref.w8_moe_gemm(a, (w8, sc), counts, pairs, src_div)
    assert fresh.shape == (T * k, n)
    mine = (flat >= base) & (flat < base + E)
    assert torch.equal(fresh[mine], out[mine])
    assert (fresh[~mine] == 0).all()


# ----------------------------- MoEMLP loading ------------------------------
NAMES = {"qwen": ("gate_proj", "up_proj", "down_proj"),
         "mixtral": ("w1", "w3", "w2")}


def _expert_tensors(mlp, style, seed=0):
    """{checkpoint name: tensor} of every local expert of `mlp` in FP8, and
    the (gate, up, down) quantized pairs per expert."""
    H, I = mlp.hidden, mlp.inter
    sub = "mlp" if style == "qwen" else "block_sparse_moe"
    out, per = {}, []
    for e in range(mlp.local_experts):
        trio = []
        for j, (leaf, (n, k)) in enumerate(zip(
                NAMES[style], ((I, H), (I, H), (H, I)))):
            g = torch.Generator().manual_seed(seed + 10 * e + j)
            w8, blocks = ref.w8_quantize(torch.randn(n, k, generator=g) * .05)
            stem = f"model.layers.0.{sub}.experts.{e}.{leaf}"
            out[f"{stem}.weight"] = w8
            out[f"{stem}.weight_scale_inv"] = blocks
            trio.append((w8, blocks))
        per.append(trio)
    return out, per


def _feed(mlp, tensors):
    proj = {"gate_proj": "gate", "up_proj": "up", "down_proj": "down",
            "w1": "gate", "w3": "up", "w2": "down"}
    for name, t in tensors.items():
        parts = name.split(".")
        mlp.load_fp8_expert(name, int(parts[5]), proj[parts[6]], parts[7], t)


def _block():
    cfg = dataclasses.replace(PRESET_CONFIGS["tiny-qwen3moe-w4"],
                              hidden_size=256, moe_intermediate_size=128)
    return MoEMLP(cfg)


@pytest.mark.parametrize("style", ["qwen", "mixtral"])
def test_moemlp_round_trip_stores_bytes_and_expanded_scales(style):
    mlp = _block()
    E, H, I = mlp.local_experts, mlp.hidden, mlp.inter
    mlp.init_w8("layers.0.mlp")
    assert mlp.w8 and not mlp.w4
    params = dict(mlp.named_parameters())
    assert "w13" not in params and "w2" not in params
    assert mlp.w13_w8.shape == (E, 2 * I, H)
    assert mlp.w13_w8.dtype == torch.float8_e4m3fn
    assert mlp.w13_w8_scales.shape == (E, H // 128, 2 * I)
    assert mlp.w2_w8.shape == (E, H, I)
    assert mlp.w2_w8_scales.shape == (E, I // 128, H)
    assert mlp.w13_w8_scales.dtype == torch.float32
    tensors, per = _expert_tensors(mlp, style)
    _feed(mlp, tensors)
    mlp.finalize_w8("layers.0.mlp")
    for e, ((g8, gs), (u8, us), (d8, ds)) in enumerate(per):
        assert torch.equal(_u8(mlp.w13_w8[e, :I]), _u8(g8))
        assert torch.equal(_u8(mlp.w13_w8[e, I:]), _u8(u8))
        assert torch.equal(_u8(mlp.w2_w8[e]), _u8(d8))
        assert torch.equal(mlp.w13_w8_scales[e, :, :I],
                           ref.w8_expand_scales(gs, I))
        assert torch.equal(mlp.w13_w8_scales[e, :, I:],
                           ref.w8_expand_scales(us, I))
        assert torch.equal(mlp.w2_w8_scales[e], ref.w8_expand_scales(ds, H))
        # the CPU stand-ins: dequantized in f32, rounded once, [in, out]
        gu = torch.cat([ref.w8_dequant(g8, ref.w8_expand_scales(gs, I)),
                        ref.w8_dequant(u8, ref.w8_expand_scales(us, I))])
        assert torch.equal(mlp.w13[e], gu.to(torch.bfloat16).t())
        assert torch.equal(
            mlp.w2[e],
            ref.w8_dequant(d8, ref.w8_expand_scales(ds, H))
            .to(torch.bfloat16).t())
    assert mlp.w13.dtype == torch.bfloat16
    assert "w13" not in dict(mlp.named_parameters())


def test_moemlp_wrong_shape_raises():
    mlp = _block()
    mlp.init_w8("layers.0.mlp")
    tensors, _ = _expert_tensors(mlp, "qwen")
    name = "model.layers.0.mlp.experts.1.up_proj.weight"
    with pytest.raises(ValueError, match=r"experts\.1\.up_proj\.weight.*shape"):
        mlp.load_fp8_expert(name, 1, "up", "weight", tensors[name][:-1])
    name = "model.layers.0.mlp.experts.1.down_proj.weight_scale_inv"
    with pytest.raises(ValueError, match=r"down_proj\.weight_scale_inv.*shape"):
        mlp.load_fp8_expert(name, 1, "down", "weight_scale_inv",
                            tensors[name].t())


@pytest.mark.parametrize("style", ["qwen", "mixtral"])
def test_moemlp_missing_scale_raises_naming_the_tensor(style):
    mlp = _block()
    mlp.init_w8("layers.0.mlp")
    tensors, _ = _expert_tensors(mlp, style)
    leaf = NAMES[style][2]
    sub = "mlp" if style == "qwen" else "block_sparse_moe"
    gone = f"model.layers.0.{sub}.experts.2.{leaf}.weight_scale_inv"
    del tensors[gone]
    _feed(mlp, tensors)
    with pytest.raises(ValueError) as ei:
        mlp.finalize_w8("layers.0.mlp")
    assert gone in str(ei.value)


def test_moemlp_plain_weight_for_a_w8_block_raises():
    mlp = _block()
    mlp.init_w8("layers.0.mlp")
    w = torch.zeros(mlp.inter, mlp.hidden, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="plain torch.bfloat16 weight"):
        mlp.load_fp8_expert("model.layers.0.mlp.experts.0.gate_proj.weight",
                            0, "gate", "weight", w)
    # and an FP8 tensor for a block that was never switched
    with pytest.raises(ValueError, match="not prepared for FP8"):
        _block().load_fp8_expert(
            "model.layers.0.mlp.experts.0.gate_proj.weight", 0, "gate",
            "weight", w.to(torch.float8_e4m3fn))


def test_moemlp_unsupported_width_raises_in_init():
    cfg = dataclasses.replace(PRESET_CONFIGS["tiny-qwen3moe-w4"],
                              moe_intermediate_size=192)
    mlp = MoEMLP(cfg)
    assert not mlp.w8_supported()
    with pytest.raises(ValueError, match=r"layers\.1\.mlp.*width 192"):
        mlp.init_w8("layers.1.mlp")
    assert not mlp.w8 and "w13" in dict(mlp.named_parameters())


# ------------------------------- CPU engine --------------------------------
@pytest.mark.parametrize("preset", MOE_PRESETS)
def test_engine_fp8_moe_checkpoint_holds_the_bytes_and_equals_bf16(
        tmp_path, preset):
    cfg = PRESET_CONFIGS[preset]
    fp8, bf16 = str(tmp_path / "fp8"), str(tmp_path / "bf16")
    save_fp8_checkpoint(cfg, fp8, seed=6, dequantized_dir=bf16)
    e = _cpu_engine(model_path=fp8)
    assert e.runner.quantization == "fp8_block"
    st = _tensors(fp8)
    I = cfg.moe_intermediate_size
    for li, layer in enumerate(e.runner.model.layers):
        mlp = layer.mlp
        assert mlp.w8 and not mlp.w4
        assert "w13" not in dict(mlp.named_parameters())
        for x in range(cfg.num_local_experts):
            pre = f"model.layers.{li}.mlp.experts.{x}"
            assert torch.equal(_u8(mlp.w13_w8[x, :I]),
                               _u8(st[f"{pre}.gate_proj.weight"]))
            assert torch.equal(_u8(mlp.w13_w8[x, I:]),
                               _u8(st[f"{pre}.up_proj.weight"]))
            assert torch.equal(_u8(mlp.w2_w8[x]),
                               _u8(st[f"{pre}.down_proj.weight"]))
            assert torch.equal(
                mlp.w2_w8_scales[x],
                ref.w8_expand_scales(st[f"{pre}.down_proj.weight_scale_inv"],
                                     cfg.hidden_size))
    assert (e.generate(PROMPTS, SP)
            == _cpu_engine(model_path=bf16).generate(PROMPTS, SP))


def test_engine_unsupported_width_falls_back_to_bf16(tmp_path, caplog):
    cfg = dataclasses.replace(PRESET_CONFIGS["tiny-qwen3moe-w4"],
                              moe_intermediate_size=192)
    fp8, bf16 = str(tmp_path / "fp8"), str(tmp_path / "bf16")
    save_fp8_checkpoint(cfg, fp8, seed=6, dequantized_dir=bf16)
    with caplog.at_level(logging.WARNING):
        e = _cpu_engine(model_path=fp8)
    said = [r.getMessage() for r in caplog.records
            if "dequantized to bf16" in r.getMessage()]
    assert len(said) == 1 and "192" in said[0]
    mlp = e.runner.model.layers[0].mlp
    assert not mlp.w8 and not hasattr(mlp, "w13_w8")
    assert "w13" in dict(mlp.named_parameters())
    assert e.runner.model.layers[0].self_attn.qkv_proj.w8
    assert (e.generate(PROMPTS, SP)
            == _cpu_engine(model_path=bf16).generate(PROMPTS, SP))


def test_engine_experts_on_the_skip_list_stay_bf16(tmp_path):
    cfg = PRESET_CONFIGS["tiny-qwen3moe-w4"]
    fp8, bf16 = str(tmp_path / "fp8"), str(tmp_path / "bf16")
    save_fp8_checkpoint(cfg, fp8, seed=6, dequantized_dir=bf16,
                        skip=("experts",))
    st = _tensors(fp8)
    assert (st["model.layers.0.mlp.experts.0.gate_proj.weight"].dtype
            == torch.bfloat16)
    e = _cpu_engine(model_path=fp8)
    layer = e.runner.model.layers[0]
    assert layer.self_attn.o_proj.w8
    assert not layer.mlp.w8
    assert "w13" in dict(layer.mlp.named_parameters())
    assert (e.generate(PROMPTS, SP)
            == _cpu_engine(model_path=bf16).generate(PROMPTS, SP))


def test_engine_half_skipped_experts_raise(tmp_path):
    cfg = PRESET_CONFIGS["tiny-qwen3moe-w4"]
    fp8 = str(tmp_path / "fp8")
    save_fp8_checkpoint(cfg, fp8, seed=6, skip=("experts.1",))
    with pytest.raises(ValueError, match="only some parts"):
        _cpu_engine(model_path=fp8)


# --------------------------- quantize_w8 in memory -------------------------
def test_quantize_w8_default_leaves_the_experts_bf16():
    m = create_model(PRESET_CONFIGS["tiny-qwen3moe-w4"])
    m.random_init(3)
    m.quantize_w8()
    mlp = m.layers[0].mlp
    assert m.layers[0].self_attn.qkv_proj.w8
    assert not mlp.w8 and "w13" in dict(mlp.named_parameters())


def test_quantize_w8_experts_switches_them():
    m = create_model(PRESET_CONFIGS["tiny-qwen3moe-w4"])
    m.random_init(3)
    mlp = m.layers[0].mlp
    w13 = mlp.w13.data.clone()
    I = mlp.inter
    m.quantize_w8(experts=True)
    assert mlp.w8 and "w13" not in dict(mlp.named_parameters())
    # gate and up are quantized as the separate tensors a checkpoint holds
    g8, gs = ref.w8_quantize(w13[1, :, :I].t())
    assert torch.equal(_u8(mlp.w13_w8[1, :I]), _u8(g8))
    assert torch.equal(mlp.w13_w8_scales[1, :, :I], ref.w8_expand_scales(gs, I))
    x = torch.randn(5, mlp.hidden).to(torch.bfloat16)
    assert torch.isfinite(mlp(x).float()).all()
    with pytest.raises(ValueError, match="needs an MoE model"):
        create_model(PRESET_CONFIGS["tiny"]).quantize_w8(experts=True)
