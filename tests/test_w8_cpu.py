"""Block-scaled FP8 checkpoints (W8A16) on the CPU: the format and reference
functions, the W8 layers, checkpoint loading, config errors and the engine.
The CPU path of a W8 layer is F.linear on the dequantized weight, so an FP8
checkpoint and its dequantized twin compare exactly; transformers' own reader
of the format is the independent oracle."""

import json
import os

import pytest
import torch
import torch.nn.functional as F

import arks_amd.ops as ops
from arks_amd.config import PRESET_CONFIGS, EngineConfig, ModelConfig
from arks_amd.engine import LLMEngine, SamplingParams
from arks_amd.loader.safetensors_loader import (
    load_model_weights, save_fp8_checkpoint,
)
from arks_amd.models import create_model
from arks_amd.ops import ref
from arks_amd.parallel.layers import (
    ColumnParallelLinear, RowParallelLinear, quantize_module_w8,
)

PROMPTS = [[3, 1, 4, 1, 5], [9, 2, 6]]
SP = SamplingParams(max_tokens=6, ignore_eos=True)
FP8_QC = {"quant_method": "fp8", "fmt": "e4m3", "activation_scheme": "dynamic",
          "weight_block_size": [128, 128]}


def _cpu_engine(**kw):
    return LLMEngine(EngineConfig(device="cpu", kv_cache_blocks=128,
                                  max_model_len=256, seed=2, **kw))


# ------------------------------ format ------------------------------------
def _e4m3_step(x):
    """Spacing of e4m3fn values around |x| <= 448: 2^-9 below the smallest
    normal 2^-6, else 2^(floor(log2 x) - 3)."""
    e = torch.floor(torch.log2(x.abs().clamp(min=2.0 ** -6)))
    return torch.pow(2.0, e - 3)


def test_quantize_dequant_error_at_most_half_an_e4m3_step():
    torch.manual_seed(2)
    w = (torch.randn(192, 384) * 0.05).to(torch.bfloat16)
    w[:128, 128:256] = 0.0          # a block of zeros
    w[130, 5] = 3.0                 # an outlier that sets its block's scale
    w8, blocks = ref.w8_quantize(w)
    assert w8.dtype == torch.float8_e4m3fn and w8.shape == (192, 384)
    assert blocks.dtype == torch.float32 and blocks.shape == (2, 3)
    assert torch.isfinite(blocks).all() and (blocks > 0).all()
    assert torch.isfinite(w8.float()).all()
    scales = ref.w8_expand_scales(blocks, 192)
    d = ref.w8_dequant(w8, scales)
    assert torch.equal(d[:128, 128:256], torch.zeros(128, 128))
    # the block maximum maps onto the top code exactly
    assert w8.float().abs().max() == 448.0
    s = scales.t().repeat_interleave(128, dim=1)        # [N, K]
    x = w.float() / s
    # round-to-nearest: half a step of the value's binade, plus the f32
    # rounding of w / s (relative 2^-24, i.e. < 2^-19 of half a step)
    bound = s * _e4m3_step(x) * 0.5 * (1 + 1e-5)
    assert ((d - w.float()).abs() <= bound).all()


def test_scale_expansion_equals_block_indexing():
    g = torch.Generator().manual_seed(1)
    for n, k in ((192, 256), (128, 128), (64, 384), (130, 200)):
        nb, kb = -(-n // 128), -(-k // 128)
        blocks = torch.rand(nb, kb, generator=g) + 0.5
        e = ref.w8_expand_scales(blocks, n)
        assert e.shape == (kb, n) and e.dtype == torch.float32
        for row in (0, 63, 127, 128, n - 1):
            if row < n:
                for c in range(kb):
                    assert e[c, row] == blocks[row // 128, c]
        w8 = torch.randn(n, k, generator=g).to(torch.float8_e4m3fn)
        d = ref.w8_dequant(w8, e)
        i, j = n - 1, k - 1
        assert d[i, j] == w8[i, j].float() * blocks[i // 128, j // 128]
    with pytest.raises(ValueError, match="do not cover N=300"):
        ref.w8_expand_scales(torch.ones(2, 2), 300)


# ------------------------------ layers ------------------------------------
@pytest.mark.parametrize("kind", ["column", "row"])
def test_w8_layer_equals_linear_on_dequantized_weight(kind):
    torch.manual_seed(3)
    if kind == "column":
        lin = ColumnParallelLinear(128, 192, bias=True)
        lin.bias.data.normal_(0, 0.05)
        x = torch.randn(7, 128, dtype=torch.bfloat16)
    else:
        lin = RowParallelLinear(256, 64, bias=False)
        x = torch.randn(7, 256, dtype=torch.bfloat16)
    lin.weight.data.normal_(0, 0.05)
    w = lin.weight.data.clone()
    quantize_module_w8(lin, kind)
    assert lin.w8 and lin.weight is None
    assert "weight" not in dict(lin.named_parameters())
    assert lin.w8_weight.dtype == torch.float8_e4m3fn
    assert lin.w8_weight.shape == w.shape
    assert lin.w8_scales.shape == (w.shape[1] // 128, w.shape[0])
    w8, blocks = ref.w8_quantize(w)
    assert torch.equal(lin.w8_weight.view(torch.uint8), w8.view(torch.uint8))
    wd = ref.w8_dequant(w8, ref.w8_expand_scales(blocks, w.shape[0]))
    wd = wd.to(torch.bfloat16)
    assert torch.equal(lin(x), F.linear(x, wd, lin.bias))
    # and ops.w8_linear's CPU path is the same definition
    assert torch.equal(ops.w8_linear(x, (lin.w8_weight, lin.w8_scales),
                                     lin.bias),
                       F.linear(x, wd, lin.bias))


def test_layer_shapes_the_kernel_cannot_run_raise_naming_the_layer():
    lin = RowParallelLinear(192, 64, bias=False)
    with pytest.raises(ValueError,
                       match=r"layers\.3\.mlp\.down_proj.*K=192 at TP=1"):
        quantize_module_w8(lin, "layers.3.mlp.down_proj")
    lin = ColumnParallelLinear(128, 96, bias=False)
    with pytest.raises(ValueError,
                       match=r"layers\.0\.self_attn\.qkv_proj.*N=96 at TP=1"):
        quantize_module_w8(lin, "layers.0.self_attn.qkv_proj")


# ---------------------------- checkpoints ---------------------------------
@pytest.fixture(scope="module")
def fp8_dirs(tmp_path_factory):
    root = tmp_path_factory.mktemp("fp8")
    dirs = {k: str(root / k) for k in ("fp8", "bf16", "skip", "skip_bf16")}
    cfg = PRESET_CONFIGS["tiny-gpu"]
    save_fp8_checkpoint(cfg, dirs["fp8"], seed=4, dequantized_dir=dirs["bf16"])
    save_fp8_checkpoint(cfg, dirs["skip"], seed=4,
                        dequantized_dir=dirs["skip_bf16"],
                        skip=("down_proj",))
    return dirs


def _header(path):
    import struct

    with open(os.path.join(path, "model.safetensors"), "rb") as f:
        (n,) = struct.unpack("<Q", f.read(8))
        return json.loads(f.read(n))


def test_written_checkpoint_has_the_published_layout(fp8_dirs):
    h = _header(fp8_dirs["fp8"])
    q = h["model.layers.0.self_attn.k_proj.weight"]
    assert q["dtype"] == "F8_E4M3" and q["shape"] == [256, 512]
    s = h["model.layers.0.self_attn.k_proj.weight_scale_inv"]
    assert s["dtype"] == "F32" and s["shape"] == [2, 4]
    assert h["model.layers.1.mlp.down_proj.weight_scale_inv"]["shape"] == [4, 8]
    for plain in ("model.embed_tokens.weight", "lm_head.weight",
                  "model.norm.weight",
                  "model.layers.0.input_layernorm.weight"):
        assert h[plain]["dtype"] == "BF16"
    assert "lm_head.weight_scale_inv" not in h
    with open(os.path.join(fp8_dirs["fp8"], "config.json")) as f:
        qc = json.load(f)["quantization_config"]
    assert {k: qc[k] for k in FP8_QC} == FP8_QC
    hs = _header(fp8_dirs["skip"])
    assert hs["model.layers.0.mlp.down_proj.weight"]["dtype"] == "BF16"
    assert "model.layers.0.mlp.down_proj.weight_scale_inv" not in hs


@pytest.mark.parametrize("which", ["fp8", "skip"])
def test_fp8_checkpoint_equals_its_dequantized_bf16_model(fp8_dirs, which):
    twin = {"fp8": "bf16", "skip": "skip_bf16"}[which]
    e = _cpu_engine(model_path=fp8_dirs[which])  # auto-detected
    assert e.runner.quantization == "fp8_block"
    layer = e.runner.model.layers[1]
    for mod in (layer.self_attn.qkv_proj, layer.self_attn.o_proj,
                layer.mlp.gate_up_proj):
        assert mod.w8 and mod.weight is None
        assert mod.w8_weight.dtype == torch.float8_e4m3fn
    assert layer.mlp.down_proj.w8 == (which == "fp8")
    assert not getattr(e.runner.model.lm_head, "w8", False)
    e_ref = _cpu_engine(model_path=fp8_dirs[twin])
    assert e_ref.runner.quantization is None
    assert torch.equal(layer.mlp.gate_up_proj.weight_qdq,
                       e_ref.runner.model.layers[1].mlp.gate_up_proj.weight)
    a = e.generate(PROMPTS, SP)
    assert all(len(o) == 6 for o in a)
    assert a == e_ref.generate(PROMPTS, SP)


def test_explicit_fp8_flag_means_the_checkpoints_own_format(fp8_dirs):
    e = _cpu_engine(model_path=fp8_dirs["fp8"], quantization="fp8")
    assert e.runner.quantization == "fp8_block"
    mod = e.runner.model.layers[0].mlp.gate_up_proj
    assert mod.w8 and not mod.fp8
    # on a bf16 checkpoint "fp8" is still the W8A8 path
    e = _cpu_engine(model_path=fp8_dirs["bf16"], quantization="fp8")
    assert e.runner.quantization == "fp8"
    mod = e.runner.model.layers[0].mlp.gate_up_proj
    assert mod.fp8 and not mod.w8


@pytest.mark.parametrize("mode", ["int4", "awq"])
def test_other_modes_on_fp8_checkpoint_raise(fp8_dirs, mode):
    with pytest.raises(ValueError, match="block-scaled FP8 checkpoint"):
        _cpu_engine(model_path=fp8_dirs["fp8"], quantization=mode)


def _forward_logits(model, cfg, token_ids):
    from arks_amd.engine.kv_cache import BlockAllocator
    from arks_amd.engine.forward_batch import ForwardBatch

    n = len(token_ids)
    nb = BlockAllocator.blocks_needed(n, 16)
    caches = [tuple(torch.zeros(nb, cfg.num_key_value_heads, 16, cfg.head_dim,
                                dtype=torch.float32) for _ in range(2))
              for _ in range(cfg.num_hidden_layers)]
    fb = ForwardBatch(
        is_prefill=True,
        input_ids=torch.tensor(token_ids, dtype=torch.int64),
        positions=torch.arange(n, dtype=torch.int64),
        slot_mapping=torch.arange(n, dtype=torch.int64),
        cu_seqlens=torch.tensor([0, n], dtype=torch.int32),
        seq_lens_list=[n],
        logits_indices=None,
    )
    with torch.no_grad():
        return model(fb, caches)


def test_format_oracle_transformers_reads_the_same_model(tmp_path):
    """transformers loads the written checkpoint with its own reader of the
    format (FineGrainedFP8Config(dequantize=True), float32) and must compute
    the logits our float32 model computes from the same files: within the
    2e-3 of test_model_parity.py, same argmax. Measured: 3.9e-7 (both sides
    dequantize in f32; transformers does not round through bf16 here)."""
    transformers = pytest.importorskip("transformers")
    path = str(tmp_path)
    cfg = PRESET_CONFIGS["tiny-qwen3"]
    save_fp8_checkpoint(cfg, path, seed=7)
    cfg_path = os.path.join(path, "config.json")
    with open(cfg_path) as f:
        hf_cfg = json.load(f)
    hf_cfg["model_type"] = "qwen3"  # AutoModel needs it; we do not read it
    with open(cfg_path, "w") as f:
        json.dump(hf_cfg, f)

    mc = ModelConfig.from_pretrained(path)
    assert mc.quant_method == "fp8_block"
    ours = create_model(mc, dtype=torch.float32)
    ours.prepare_fp8_checkpoint()
    load_model_weights(ours, path, torch.device("cpu"))
    ours.finalize_w8()
    assert ours.layers[0].mlp.down_proj.weight_qdq.dtype == torch.float32

    hf = transformers.AutoModelForCausalLM.from_pretrained(
        path,
        quantization_config=transformers.FineGrainedFP8Config(dequantize=True),
        dtype=torch.float32,
    )
    hf.eval()
    assert hf.model.layers[0].mlp.down_proj.weight.dtype == torch.float32
    ids = [1, 17, 300, 42, 42, 7, 99, 123, 8, 55, 4]
    logits = _forward_logits(ours, cfg, ids)
    with torch.no_grad():
        hf_logits = hf(torch.tensor([ids])).logits[0]
    diff = (logits - hf_logits).abs().max().item()
    print(f"fp8 checkpoint, ours vs transformers: max logits diff {diff}")
    assert diff < 2e-3, f"max logits diff {diff}"
    assert torch.equal(logits.argmax(-1), hf_logits.argmax(-1))


# ------------------------- malformed checkpoints ---------------------------
def _rewrite(src, dst, edit, qc_edit=None):
    """Copy checkpoint src to dst with its tensor dict (and optionally its
    quantization_config) edited."""
    from safetensors.torch import load_file, save_file

    os.makedirs(dst, exist_ok=True)
    tensors = load_file(os.path.join(src, "model.safetensors"))
    edit(tensors)
    save_file(tensors, os.path.join(dst, "model.safetensors"))
    with open(os.path.join(src, "config.json")) as f:
        cfg = json.load(f)
    if qc_edit is not None:
        qc_edit(cfg)
    with open(os.path.join(dst, "config.json"), "w") as f:
        json.dump(cfg, f)
    return dst


def test_scale_without_its_weight_raises(fp8_dirs, tmp_path):
    name = "model.layers.0.self_attn.o_proj.weight"
    d = _rewrite(fp8_dirs["fp8"], str(tmp_path / "a"),
                 lambda t: t.pop(name))
    with pytest.raises(ValueError, match=r"layers\.0\.self_attn\.o_proj.*"
                                         "scale without its weight"):
        _cpu_engine(model_path=d)


def test_fp8_tensor_on_a_model_not_prepared_raises(fp8_dirs, tmp_path):
    d = _rewrite(fp8_dirs["fp8"], str(tmp_path / "a"), lambda t: None,
                 lambda c: c.pop("quantization_config"))
    with pytest.raises(ValueError, match="not prepared for FP8"):
        _cpu_engine(model_path=d)
    # a module on the skip list that arrives in FP8 all the same
    d = _rewrite(fp8_dirs["fp8"], str(tmp_path / "b"), lambda t: None,
                 lambda c: c["quantization_config"].update(
                     modules_to_not_convert=["lm_head", "o_proj"]))
    with pytest.raises(ValueError, match=r"o_proj.*not prepared for FP8"):
        _cpu_engine(model_path=d)


def test_plain_tensor_where_w8_was_prepared_raises(fp8_dirs, tmp_path):
    d = _rewrite(fp8_dirs["skip"], str(tmp_path / "a"), lambda t: None,
                 lambda c: c["quantization_config"].update(
                     modules_to_not_convert=["lm_head"]))
    with pytest.raises(ValueError, match=r"down_proj.*prepared for FP8"):
        _cpu_engine(model_path=d)


def test_partly_quantized_fused_projection_raises_naming_it(fp8_dirs,
                                                            tmp_path):
    d = _rewrite(fp8_dirs["fp8"], str(tmp_path / "a"), lambda t: None,
                 lambda c: c["quantization_config"].update(
                     modules_to_not_convert=["lm_head", "k_proj"]))
    with pytest.raises(ValueError,
                       match=r"layers\.0\.self_attn\.qkv_proj.*all be FP8"):
        _cpu_engine(model_path=d)


def test_quantized_lm_head_is_dequantized_at_load(fp8_dirs, tmp_path):
    def edit(t):
        w8, blocks = ref.w8_quantize(t["lm_head.weight"])
        t["lm_head.weight"] = w8
        t["lm_head.weight_scale_inv"] = blocks

    d = _rewrite(fp8_dirs["fp8"], str(tmp_path / "a"), edit,
                 lambda c: c["quantization_config"].update(
                     modules_to_not_convert=[]))
    e = _cpu_engine(model_path=d)
    head = e.runner.model.lm_head
    assert not getattr(head, "w8", False)
    assert head.weight.dtype == torch.bfloat16
    from safetensors.torch import load_file

    t = load_file(os.path.join(d, "model.safetensors"))
    want = ref.w8_dequant(
        t["lm_head.weight"],
        ref.w8_expand_scales(t["lm_head.weight_scale_inv"], head.weight.shape[0]))
    assert torch.equal(head.weight.data, want.to(torch.bfloat16))
    assert all(len(o) == 6 for o in e.generate(PROMPTS, SP))


def test_e5m2_tensor_gives_a_clear_error(fp8_dirs, tmp_path):
    def edit(t):
        n = "model.layers.0.self_attn.o_proj.weight"
        t[n] = t[n].float().to(torch.float8_e5m2)

    d = _rewrite(fp8_dirs["fp8"], str(tmp_path / "a"), edit)
    with pytest.raises(ValueError, match="F8_E5M2"):
        _cpu_engine(model_path=d)
    from arks_amd.loader.safetensors_loader import _parse_header

    with pytest.raises(ValueError, match="F8_E5M2"):
        _parse_header(os.path.join(d, "model.safetensors"))
    # and the e4m3 entry the GPU loader's header parser needs is there
    _, ts = _parse_header(os.path.join(fp8_dirs["fp8"], "model.safetensors"))
    assert torch.float8_e4m3fn in {dt for _, dt, *_ in ts}


# --------------------------- config errors --------------------------------
@pytest.mark.parametrize("field,value", [
    ("fmt", "e5m2"), ("weight_block_size", [64, 64]),
    ("activation_scheme", "static"), ("scale_fmt", "ue8m0"),
])
def test_unsupported_fp8_config_names_the_field(tmp_path, field, value):
    hf = {"architectures": ["Qwen3ForCausalLM"],
          "quantization_config": dict(FP8_QC)}
    assert ModelConfig.from_hf_config(hf).quant_method == "fp8_block"
    hf["quantization_config"]["scale_fmt"] = "float"
    assert ModelConfig.from_hf_config(hf).quant_method == "fp8_block"
    hf["quantization_config"][field] = value
    with open(tmp_path / "config.json", "w") as f:
        json.dump(hf, f)
    with pytest.raises(ValueError, match=field):
        ModelConfig.from_pretrained(str(tmp_path))


def test_ignored_layers_is_an_alias(fp8_dirs, tmp_path):
    hf = {"architectures": ["Qwen3ForCausalLM"],
          "quantization_config": dict(FP8_QC, ignored_layers=["lm_head",
                                                              "down_proj"])}
    assert ModelConfig.from_hf_config(hf).quant_skip_modules == (
        "lm_head", "down_proj")

    def alias(c):
        qc = c["quantization_config"]
        qc["ignored_layers"] = qc.pop("modules_to_not_convert")

    d = _rewrite(fp8_dirs["skip"], str(tmp_path / "a"), lambda t: None, alias)
    e = _cpu_engine(model_path=d)
    layer = e.runner.model.layers[0]
    assert layer.mlp.gate_up_proj.w8 and not layer.mlp.down_proj.w8
    assert (e.generate(PROMPTS, SP)
            == _cpu_engine(model_path=fp8_dirs["skip_bf16"]).generate(
                PROMPTS, SP))


def test_skip_entries_match_whole_name_components():
    """"mlp.gate" names a router, not gate_proj."""
    m = create_model(
        ModelConfig(**{**PRESET_CONFIGS["tiny"].__dict__,
                       "quant_skip_modules": ("mlp.gate",
                                              "model.layers.1.self_attn")}))
    assert not m._w8_skipped("model.layers.0.mlp.gate_proj")
    assert m._w8_skipped("model.layers.0.mlp.gate")
    assert m._w8_skipped("model.layers.1.self_attn.q_proj")
    assert not m._w8_skipped("model.layers.11.self_attn.q_proj")


# -------------------------------- MoE --------------------------------------
@pytest.mark.parametrize("preset", ["tiny-qwen3moe-w4", "tiny-qwen2moe-w4"])
def test_moe_fp8_checkpoint_keeps_experts_bf16(tmp_path, preset, caplog):
    fp8, bf16 = str(tmp_path / "fp8"), str(tmp_path / "bf16")
    save_fp8_checkpoint(PRESET_CONFIGS[preset], fp8, seed=6,
                        dequantized_dir=bf16)
    h = _header(fp8)
    assert h["model.layers.0.mlp.experts.1.up_proj.weight"]["dtype"] == "F8_E4M3"
    assert h["model.layers.0.mlp.gate.weight"]["dtype"] == "BF16"
    import logging

    with caplog.at_level(logging.WARNING):
        e = _cpu_engine(model_path=fp8)
    said = [r for r in caplog.records if "dequantized to bf16" in r.message]
    assert len(said) == 1
    layer = e.runner.model.layers[0]
    assert layer.self_attn.qkv_proj.w8 and layer.self_attn.o_proj.w8
    assert layer.mlp.w13.dtype == torch.bfloat16
    assert layer.mlp.w2.dtype == torch.bfloat16
    assert not layer.mlp.w4
    if layer.mlp.shared is not None:
        assert layer.mlp.shared.gate_up_proj.w8
        assert layer.mlp.shared.down_proj.w8
    e_ref = _cpu_engine(model_path=bf16)
    assert torch.equal(layer.mlp.w13, e_ref.runner.model.layers[0].mlp.w13)
    assert e.generate(PROMPTS, SP) == e_ref.generate(PROMPTS, SP)


# ------------------------------- LoRA --------------------------------------
def test_w8_with_lora_generates_and_the_delta_reaches_the_layers(tmp_path):
    from lora_testutil import engine_cfg, make_adapters

    adapters = make_adapters("tiny", tmp_path)
    fp8 = str(tmp_path / "fp8")
    save_fp8_checkpoint(PRESET_CONFIGS["tiny"], fp8, seed=1)
    cfg = engine_cfg("tiny", "cpu", enable_lora=True, lora_modules=adapters)
    cfg.preset, cfg.model_path = None, fp8
    e = LLMEngine(cfg)
    assert e.runner.model.layers[0].self_attn.qkv_proj.w8
    sp = SamplingParams(max_tokens=5, ignore_eos=True)
    out = e.generate([[1, 5, 9, 20, 31, 7]] * 2, sp, lora=["a", None])
    assert all(len(o) == 5 for o in out)
    assert out[0] != out[1]


# ------------------------------ routing ------------------------------------
@pytest.mark.parametrize("m", [1, 16, 17, 33, 64])
@pytest.mark.parametrize("n,k", [(64, 128), (128, 384), (1024, 256),
                                 (4608, 3584), (3584, 3584), (37888, 3584),
                                 (3584, 18944), (192, 8192)])
def test_w8_plan_is_launchable(m, n, k):
    """Whatever numbers the routing rule holds, its plans must satisfy what
    the kernel requires: whole 128-blocks per split, splits that cover K
    with none empty, a tile width that divides N."""
    nw, nsplits, kps, mrows = ops._w8_plan(m, n, k)
    assert nw in (1, 2) and n % (64 * nw) == 0
    assert kps % 128 == 0 and kps >= 128
    assert nsplits >= 1 and (nsplits - 1) * kps < k <= nsplits * kps
    assert mrows == 16 * min(-(-m // 16), 4)
