"""MXFP4 checkpoints (MX4, W4A16) on the CPU: the format and reference
functions, the MX4 layers, config acceptance and refusals, checkpoint
loading and the engine. The CPU path of an MX4 layer is F.linear on the
dequantized weight, which bf16 holds exactly, so an MXFP4 checkpoint and its
dequantized twin compare token for token."""

import copy
import json
import logging
import os

import pytest
import torch
import torch.nn.functional as F

import arks_amd.ops as ops
from arks_amd.config import PRESET_CONFIGS, EngineConfig, ModelConfig
from arks_amd.engine import LLMEngine, SamplingParams
from arks_amd.loader.safetensors_loader import (
    _MX4_CONFIG, save_mx4_checkpoint, save_random_checkpoint,
)
from arks_amd.models import create_model
from arks_amd.ops import ref
from arks_amd.parallel.layers import (
    ColumnParallelLinear, RowParallelLinear, quantize_module_mx4,
)

PROMPTS = [[3, 1, 4, 1, 5], [9, 2, 6]]
SP = SamplingParams(max_tokens=6, ignore_eos=True)
E2M1 = torch.tensor(ref.MX4_VALUES)


def _cpu_engine(**kw):
    return LLMEngine(EngineConfig(device="cpu", kv_cache_blocks=128,
                                  max_model_len=256, seed=2, **kw))


# ------------------------------ format ------------------------------------
def test_format_constants_and_code_table():
    assert ref.MX4_BLOCK == 32
    assert ref.MX4_VALUES == (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
    # byte b: k = 2b in the low nibble, k = 2b + 1 in the high one; bit 3 of
    # a code is the sign
    packed = torch.tensor([[0x21, 0xF9] + [0] * 14], dtype=torch.uint8)
    scales = torch.tensor([[128]], dtype=torch.uint8)
    d = ref.mx4_dequant(packed, scales)
    assert d.shape == (1, 32) and d.dtype == torch.float32
    assert d[0, :4].tolist() == [1.0, 2.0, -1.0, -12.0]


@pytest.mark.parametrize("j", [-20, -7, 0, 5])
def test_e2m1_values_times_a_power_of_two_round_trip_exactly(j):
    g = torch.Generator().manual_seed(j + 100)
    both = torch.cat([E2M1, -E2M1])
    w = both[torch.randint(0, 16, (8, 64), generator=g)] * 2.0 ** j
    w[:, 0] = 6.0 * 2.0 ** j        # every block holds the top value
    w[:, 32] = -4.0 * 2.0 ** j      # ... or one in the top binade
    packed, scales = ref.mx4_quantize(w)
    assert packed.dtype == torch.uint8 and packed.shape == (8, 32)
    assert scales.dtype == torch.uint8 and scales.shape == (8, 2)
    # shared exponent = floor(log2(amax)) - 2 = j for amax in [4, 8) * 2^j
    assert (scales == 127 + j).all()
    assert torch.equal(ref.mx4_dequant(packed, scales), w)


def test_quantize_dequant_is_idempotent_and_rounds_to_nearest():
    torch.manual_seed(2)
    w = torch.randn(48, 256) * 0.05
    w[3, 7] = 3.0                    # an outlier that sets its block's scale
    packed, scales = ref.mx4_quantize(w)
    d = ref.mx4_dequant(packed, scales)
    p2, s2 = ref.mx4_quantize(d)
    assert torch.equal(p2, packed) and torch.equal(s2, scales)
    assert torch.equal(ref.mx4_dequant(p2, s2), d)
    # nearest: no e2m1 grid point of the block's scale is closer (saturated
    # elements excepted: they sit at the nearest end of the grid anyway)
    s = torch.ldexp(torch.ones(48, 8), scales.int() - 127)
    s = s.repeat_interleave(32, dim=1)
    grid = torch.cat([E2M1, -E2M1])[None, None, :] * s[:, :, None]
    best = (grid - w[:, :, None]).abs().amin(dim=2)
    assert torch.equal((d - w).abs(), best)
    # ties go to the even code: 0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2,
    # 2.5 -> 2, 3.5 -> 4, 5 -> 4 (next to a 6 that fixes the scale at 1)
    t = torch.zeros(1, 32)
    t[0, :8] = torch.tensor([6.0, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0])
    out = ref.mx4_dequant(*ref.mx4_quantize(t))
    assert out[0, :8].tolist() == [6.0, 0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0]


def test_saturation_at_six_times_the_scale():
    # amax 7.5 -> shared exponent floor(log2 7.5) - 2 = 0: 7.5 and -7 are
    # beyond the largest e2m1 value and saturate at +-6
    w = torch.zeros(1, 32)
    w[0, :3] = torch.tensor([7.5, -7.0, 5.9])
    packed, scales = ref.mx4_quantize(w)
    assert scales.tolist() == [[127]]
    assert ref.mx4_dequant(packed, scales)[0, :3].tolist() == [6.0, -6.0, 6.0]
    w = w * 2.0 ** 9
    packed, scales = ref.mx4_quantize(w)
    assert scales.tolist() == [[136]]
    assert ref.mx4_dequant(packed, scales)[0, :2].tolist() == [
        6.0 * 2 ** 9, -6.0 * 2 ** 9]


def test_zero_block_gets_scale_127():
    w = torch.randn(2, 64)
    w[1, 32:] = 0.0
    packed, scales = ref.mx4_quantize(w)
    assert scales[1, 1] == 127
    assert not packed[1, 16:].any()
    assert torch.equal(ref.mx4_dequant(packed, scales)[1, 32:],
                       torch.zeros(32))


def test_quantizer_keeps_scales_in_the_range_a_layer_accepts():
    w = torch.zeros(2, 32)
    w[0, 0], w[1, 0] = 2.0 ** -140, 2.0 ** 127
    _, scales = ref.mx4_quantize(w)
    assert scales[:, 0].tolist() == [ref.MX4_SCALE_MIN, ref.MX4_SCALE_MAX]
    with pytest.raises(ValueError, match="K % 32"):
        ref.mx4_quantize(torch.zeros(2, 48))


# ------------------------------ layers ------------------------------------
@pytest.mark.parametrize("kind", ["column", "row"])
def test_mx4_layer_equals_linear_on_dequantized_weight(kind):
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
    quantize_module_mx4(lin, kind)
    assert lin.mx4 and lin.weight is None
    assert "weight" not in dict(lin.named_parameters())
    assert lin.mx4_weight.dtype == lin.mx4_scales.dtype == torch.uint8
    assert lin.mx4_weight.shape == (w.shape[0], w.shape[1] // 2)
    assert lin.mx4_scales.shape == (w.shape[0], w.shape[1] // 32)
    packed, scales = ref.mx4_quantize(w)
    assert torch.equal(lin.mx4_weight, packed)
    assert torch.equal(lin.mx4_scales, scales)
    wd = ref.mx4_dequant(packed, scales)
    assert torch.equal(wd.to(torch.bfloat16).float(), wd)  # bf16 holds it
    wd = wd.to(torch.bfloat16)
    assert torch.equal(lin(x), F.linear(x, wd, lin.bias))
    # and ops.mx4_linear's CPU path is the same definition
    assert torch.equal(ops.mx4_linear(x, (lin.mx4_weight, lin.mx4_scales),
                                      lin.bias),
                       F.linear(x, wd, lin.bias))
    assert torch.equal(ops.mx4_dequant((lin.mx4_weight, lin.mx4_scales)), wd)


def test_layer_shapes_the_kernel_cannot_run_raise_naming_the_layer():
    lin = RowParallelLinear(192, 64, bias=False)
    with pytest.raises(ValueError,
                       match=r"layers\.3\.mlp\.down_proj.*K=192 at TP=1"):
        quantize_module_mx4(lin, "layers.3.mlp.down_proj")
    lin = ColumnParallelLinear(128, 96, bias=False)
    with pytest.raises(ValueError,
                       match=r"layers\.0\.self_attn\.qkv_proj.*N=96 at TP=1"):
        quantize_module_mx4(lin, "layers.0.self_attn.qkv_proj")


def test_mx4_takes_the_shared_plan_and_a_slab_limit_above_one_slab():
    assert ops.MX4_SLAB_MAX_M >= ops._WQ_SKINNY_MAX_M
    assert ops._mx4_plan is ops._wq_plan
    assert ops._MX4.name == "mx4"


# ------------------------------ config ------------------------------------
def _hf(**qc_edits):
    qc = copy.deepcopy(_MX4_CONFIG)
    qc["exclude"] = ["lm_head"]
    qc.update(qc_edits)
    return {"architectures": ["Qwen2ForCausalLM"], "quantization_config": qc}


def test_quark_mxfp4_config_is_accepted():
    mc = ModelConfig.from_hf_config(_hf())
    assert mc.quant_method == "mxfp4"
    assert mc.quant_skip_modules == ("lm_head",)
    # a dynamic activation spec is accepted and ignored (activations are
    # bf16 here), upper-case spellings too
    hf = _hf()
    g = hf["quantization_config"]["global_quant_config"]
    g["input_tensors"] = {"dtype": "fp4", "qscheme": "per_group",
                          "group_size": 32, "scale_format": "e8m0",
                          "is_dynamic": True}
    g["weight"]["scale_format"] = "E8M0"
    assert ModelConfig.from_hf_config(hf).quant_method == "mxfp4"
    # the export section is optional
    hf["quantization_config"].pop("export")
    assert ModelConfig.from_hf_config(hf).quant_method == "mxfp4"


@pytest.mark.parametrize("path,value,named", [
    (("global_quant_config", "weight", "dtype"), "int4", "weight.dtype"),
    (("global_quant_config", "weight", "dtype"), "fp8_e4m3", "weight.dtype"),
    (("global_quant_config", "weight", "qscheme"), "per_channel",
     "weight.qscheme"),
    (("global_quant_config", "weight", "group_size"), 128,
     "weight.group_size"),
    (("global_quant_config", "weight", "scale_format"), "float32",
     "weight.scale_format"),
    (("global_quant_config", "weight", "is_dynamic"), True,
     "weight.is_dynamic"),
    # static input scales
    (("global_quant_config", "input_tensors"),
     {"dtype": "fp8_e4m3", "is_dynamic": False}, "input_tensors"),
    (("global_quant_config", "output_tensors"),
     {"dtype": "fp8_e4m3", "is_dynamic": True}, "output_tensors"),
    (("global_quant_config", "bias"), {"dtype": "bf16"},
     r"global_quant_config\.bias"),
    (("layer_quant_config",), {"*down_proj": {"weight": {}}},
     "layer_quant_config"),
    (("layer_type_quant_config",), {"Linear": {"weight": {}}},
     "layer_type_quant_config"),
    (("export", "kv_cache_group"), ["*k_proj", "*v_proj"],
     r"export\.kv_cache_group"),
    (("export", "weight_format"), "fake_quantized",
     r"export\.weight_format"),
])
def test_unsupported_quark_config_names_the_field(tmp_path, path, value,
                                                  named):
    hf = _hf()
    node = hf["quantization_config"]
    for key in path[:-1]:
        node = node[key]
    node[path[-1]] = value
    with open(tmp_path / "config.json", "w") as f:
        json.dump(hf, f)
    with pytest.raises(ValueError,
                       match=f"unsupported quantization_config: .*{named}="):
        ModelConfig.from_pretrained(str(tmp_path))


def test_quark_without_a_weight_spec_is_refused():
    with pytest.raises(ValueError, match="global_quant_config"):
        ModelConfig.from_hf_config(
            {"quantization_config": {"quant_method": "quark"}})


def test_exclude_entries_are_names_or_fnmatch_patterns():
    mc = ModelConfig.from_hf_config(_hf(exclude=[
        "lm_head", "*.mlp.down_proj", "model.layers.1.self_attn.o_proj",
        "mlp.gate"]))
    assert mc.quant_skip_modules == (
        "lm_head", "*.mlp.down_proj", "model.layers.1.self_attn.o_proj",
        "mlp.gate")
    m = create_model(ModelConfig(**{**PRESET_CONFIGS["tiny"].__dict__,
                                    "quant_skip_modules":
                                        mc.quant_skip_modules}))
    assert m._mx4_skipped("model.layers.0.mlp.down_proj")
    assert m._mx4_skipped("model.layers.1.mlp.down_proj")
    assert not m._mx4_skipped("model.layers.0.mlp.gate_proj")
    assert m._mx4_skipped("model.layers.0.mlp.gate")
    assert m._mx4_skipped("model.layers.1.self_attn.o_proj")
    assert not m._mx4_skipped("model.layers.0.self_attn.o_proj")
    assert m._mx4_skipped("lm_head")
    with pytest.raises(ValueError, match="exclude="):
        ModelConfig.from_hf_config(_hf(exclude="lm_head"))


# ---------------------------- checkpoints ---------------------------------
@pytest.fixture(scope="module")
def mx4_dirs(tmp_path_factory):
    root = tmp_path_factory.mktemp("mx4")
    dirs = {k: str(root / k) for k in ("mx4", "bf16", "skip", "skip_bf16")}
    cfg = PRESET_CONFIGS["tiny"]
    save_mx4_checkpoint(cfg, dirs["mx4"], seed=4, dequantized_dir=dirs["bf16"])
    save_mx4_checkpoint(cfg, dirs["skip"], seed=4,
                        dequantized_dir=dirs["skip_bf16"],
                        skip=("*.down_proj",))
    return dirs


def _header(path):
    import struct

    with open(os.path.join(path, "model.safetensors"), "rb") as f:
        (n,) = struct.unpack("<Q", f.read(8))
        return json.loads(f.read(n))


def test_written_checkpoint_has_the_described_layout(mx4_dirs):
    h = _header(mx4_dirs["mx4"])
    q = h["model.layers.0.self_attn.k_proj.weight"]
    assert q["dtype"] == "U8" and q["shape"] == [64, 64]      # [N, K/2]
    s = h["model.layers.0.self_attn.k_proj.weight_scale"]
    assert s["dtype"] == "U8" and s["shape"] == [64, 4]       # [N, K/32]
    assert h["model.layers.1.mlp.down_proj.weight"]["shape"] == [128, 128]
    assert h["model.layers.1.mlp.down_proj.weight_scale"]["shape"] == [128, 8]
    for plain in ("model.embed_tokens.weight", "lm_head.weight",
                  "model.norm.weight", "model.layers.0.self_attn.q_proj.bias",
                  "model.layers.0.input_layernorm.weight"):
        assert h[plain]["dtype"] == "BF16"
    assert "lm_head.weight_scale" not in h
    with open(os.path.join(mx4_dirs["mx4"], "config.json")) as f:
        qc = json.load(f)["quantization_config"]
    assert qc["quant_method"] == "quark" and qc["exclude"] == ["lm_head"]
    assert qc["global_quant_config"]["weight"]["scale_format"] == "e8m0"
    hs = _header(mx4_dirs["skip"])
    assert hs["model.layers.0.mlp.down_proj.weight"]["dtype"] == "BF16"
    assert "model.layers.0.mlp.down_proj.weight_scale" not in hs


@pytest.mark.parametrize("which", ["mx4", "skip"])
def test_mx4_checkpoint_equals_its_dequantized_bf16_model(mx4_dirs, which):
    twin = {"mx4": "bf16", "skip": "skip_bf16"}[which]
    e = _cpu_engine(model_path=mx4_dirs[which])  # auto-detected
    assert e.runner.quantization == "mxfp4"
    layer = e.runner.model.layers[1]
    for mod in (layer.self_attn.qkv_proj, layer.self_attn.o_proj,
                layer.mlp.gate_up_proj):
        assert mod.mx4 and mod.weight is None
        assert mod.mx4_weight.dtype == mod.mx4_scales.dtype == torch.uint8
    assert layer.mlp.down_proj.mx4 == (which == "mx4")
    assert not getattr(e.runner.model.lm_head, "mx4", False)
    e_ref = _cpu_engine(model_path=mx4_dirs[twin])
    assert e_ref.runner.quantization is None
    assert torch.equal(layer.mlp.gate_up_proj.weight_qdq,
                       e_ref.runner.model.layers[1].mlp.gate_up_proj.weight)
    a = e.generate(PROMPTS, SP)
    assert all(len(o) == 6 for o in a)
    assert a == e_ref.generate(PROMPTS, SP)
    # the explicit flag means the same thing
    e2 = _cpu_engine(model_path=mx4_dirs[which], quantization="mxfp4")
    assert e2.runner.quantization == "mxfp4"
    assert e2.generate(PROMPTS, SP) == a


@pytest.mark.parametrize("mode", ["int4", "awq", "fp8"])
def test_other_modes_on_mxfp4_checkpoint_raise(mx4_dirs, mode):
    with pytest.raises(ValueError, match="MXFP4 checkpoint"):
        _cpu_engine(model_path=mx4_dirs["mx4"], quantization=mode)


def test_flag_conflicts_raise(mx4_dirs):
    with pytest.raises(ValueError, match="unknown quantization 'mxfp8'"):
        EngineConfig(quantization="mxfp8")
    with pytest.raises(ValueError, match="quantize_experts needs "
                                         "quantization='int4'"):
        EngineConfig(quantization="mxfp4", quantize_experts=True)


def test_mxfp4_flag_on_a_bf16_checkpoint_quantizes_at_load(mx4_dirs,
                                                           tmp_path):
    path = str(tmp_path / "plain")
    save_random_checkpoint(PRESET_CONFIGS["tiny"], path, seed=9)
    e_ref = _cpu_engine(model_path=path)
    e = _cpu_engine(model_path=path, quantization="mxfp4")
    assert e.runner.quantization == "mxfp4"
    for li, layer in enumerate(e.runner.model.layers):
        plain = e_ref.runner.model.layers[li]
        for get in (lambda l: l.self_attn.qkv_proj,
                    lambda l: l.self_attn.o_proj,
                    lambda l: l.mlp.gate_up_proj,
                    lambda l: l.mlp.down_proj):
            mod = get(layer)
            assert mod.mx4 and mod.weight is None
            assert "weight" not in dict(mod.named_parameters())
            packed, scales = ref.mx4_quantize(get(plain).weight.data)
            assert torch.equal(mod.mx4_weight, packed)
            assert torch.equal(mod.mx4_scales, scales)
    assert not getattr(e.runner.model.lm_head, "mx4", False)
    assert all(len(o) == 6 for o in e.generate(PROMPTS, SP))
    # quantizing the dequantized twin of an MXFP4 checkpoint at load gives
    # that checkpoint back (the quantizer is idempotent)
    e = _cpu_engine(model_path=mx4_dirs["bf16"], quantization="mxfp4")
    assert (e.generate(PROMPTS, SP)
            == _cpu_engine(model_path=mx4_dirs["mx4"]).generate(PROMPTS, SP))


# ------------------------- malformed checkpoints ---------------------------
def _rewrite(src, dst, edit, qc_edit=None):
    """Copy checkpoint src to dst with its tensor dict (and optionally its
    config) edited."""
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


@pytest.mark.parametrize("byte", [0, 1, 253, 255])
def test_scale_byte_outside_the_range_is_refused_naming_the_tensor(
        mx4_dirs, tmp_path, byte):
    name = "model.layers.1.mlp.up_proj.weight_scale"

    def edit(t):
        t[name][5, 2] = byte

    d = _rewrite(mx4_dirs["mx4"], str(tmp_path / "a"), edit)
    with pytest.raises(ValueError,
                       match=r"layers\.1\.mlp\.up_proj\.weight_scale.*"
                             rf"(\[\d+, {byte}\]|\[{byte}, \d+\])"):
        _cpu_engine(model_path=d)


@pytest.mark.parametrize("byte", [2, 252])
def test_scale_bytes_at_the_ends_of_the_range_load(mx4_dirs, tmp_path, byte):
    name = "model.layers.1.mlp.up_proj.weight_scale"

    def edit(t):
        t[name][5, 2] = byte

    d = _rewrite(mx4_dirs["mx4"], str(tmp_path / "a"), edit)
    e = _cpu_engine(model_path=d)
    assert torch.isfinite(e.runner.model.layers[1].mlp.gate_up_proj
                          .weight_qdq.float()).all()


def test_partly_quantized_fused_projection_raises_naming_it(mx4_dirs,
                                                            tmp_path):
    d = _rewrite(mx4_dirs["mx4"], str(tmp_path / "a"), lambda t: None,
                 lambda c: c["quantization_config"].update(
                     exclude=["lm_head", "*.k_proj"]))
    with pytest.raises(ValueError,
                       match=r"layers\.0\.self_attn\.qkv_proj.*all be MXFP4"):
        _cpu_engine(model_path=d)

    # and a k_proj that arrives in bf16 without being excluded
    def edit(t):
        n = "model.layers.0.self_attn.k_proj"
        t[f"{n}.weight"] = ref.mx4_dequant(
            t[f"{n}.weight"], t.pop(f"{n}.weight_scale")).to(torch.bfloat16)

    d = _rewrite(mx4_dirs["mx4"], str(tmp_path / "b"), edit)
    with pytest.raises(ValueError, match=r"k_proj.*prepared for MXFP4"):
        _cpu_engine(model_path=d)


def test_mx4_tensor_on_a_model_not_prepared_raises(mx4_dirs, tmp_path):
    d = _rewrite(mx4_dirs["mx4"], str(tmp_path / "a"), lambda t: None,
                 lambda c: c.pop("quantization_config"))
    with pytest.raises(ValueError, match="not prepared for MXFP4"):
        _cpu_engine(model_path=d)
    d = _rewrite(mx4_dirs["mx4"], str(tmp_path / "b"), lambda t: None,
                 lambda c: c["quantization_config"].update(
                     exclude=["lm_head", "*.o_proj"]))
    with pytest.raises(ValueError, match=r"o_proj.*not prepared for MXFP4"):
        _cpu_engine(model_path=d)


def test_weight_without_its_scale_raises(mx4_dirs, tmp_path):
    name = "model.layers.0.self_attn.o_proj.weight_scale"
    d = _rewrite(mx4_dirs["mx4"], str(tmp_path / "a"),
                 lambda t: t.pop(name))
    with pytest.raises(ValueError, match=r"layers\.0\.self_attn\.o_proj.*"
                                         r"no \['weight_scale'\]"):
        _cpu_engine(model_path=d)


def test_quantized_lm_head_is_dequantized_at_load(mx4_dirs, tmp_path):
    def edit(t):
        packed, scales = ref.mx4_quantize(t["lm_head.weight"])
        t["lm_head.weight"] = packed
        t["lm_head.weight_scale"] = scales

    d = _rewrite(mx4_dirs["mx4"], str(tmp_path / "a"), edit,
                 lambda c: c["quantization_config"].update(exclude=[]))
    e = _cpu_engine(model_path=d)
    head = e.runner.model.lm_head
    assert not getattr(head, "mx4", False)
    assert head.weight.dtype == torch.bfloat16
    from safetensors.torch import load_file

    t = load_file(os.path.join(d, "model.safetensors"))
    want = ref.mx4_dequant(t["lm_head.weight"], t["lm_head.weight_scale"])
    assert torch.equal(head.weight.data, want.to(torch.bfloat16))
    assert all(len(o) == 6 for o in e.generate(PROMPTS, SP))


# -------------------------------- MoE --------------------------------------
@pytest.mark.parametrize("preset", ["tiny-qwen3moe-w4", "tiny-qwen2moe-w4"])
def test_moe_mx4_checkpoint_keeps_routed_experts_bf16(tmp_path, preset,
                                                      caplog):
    mx4, bf16 = str(tmp_path / "mx4"), str(tmp_path / "bf16")
    save_mx4_checkpoint(PRESET_CONFIGS[preset], mx4, seed=6,
                        dequantized_dir=bf16)
    h = _header(mx4)
    assert h["model.layers.0.mlp.experts.1.up_proj.weight"]["dtype"] == "U8"
    assert h["model.layers.0.mlp.gate.weight"]["dtype"] == "BF16"
    with caplog.at_level(logging.WARNING):
        e = _cpu_engine(model_path=mx4)
    said = [r for r in caplog.records if "dequantized to bf16" in r.message]
    assert len(said) == 1
    layer = e.runner.model.layers[0]
    assert layer.self_attn.qkv_proj.mx4 and layer.self_attn.o_proj.mx4
    assert layer.mlp.w13.dtype == torch.bfloat16
    assert layer.mlp.w2.dtype == torch.bfloat16
    assert not layer.mlp.w4 and not layer.mlp.w8
    if layer.mlp.shared is not None:
        assert layer.mlp.shared.gate_up_proj.mx4
        assert layer.mlp.shared.down_proj.mx4
    e_ref = _cpu_engine(model_path=bf16)
    assert torch.equal(layer.mlp.w13, e_ref.runner.model.layers[0].mlp.w13)
    assert e.generate(PROMPTS, SP) == e_ref.generate(PROMPTS, SP)


# ------------------- LoRA, speculation, embeddings -------------------------
def test_mx4_with_lora_generates_and_the_delta_reaches_the_layers(tmp_path):
    from lora_testutil import engine_cfg, make_adapters

    adapters = make_adapters("tiny", tmp_path)
    mx4 = str(tmp_path / "mx4")
    save_mx4_checkpoint(PRESET_CONFIGS["tiny"], mx4, seed=1)
    cfg = engine_cfg("tiny", "cpu", enable_lora=True, lora_modules=adapters)
    cfg.preset, cfg.model_path = None, mx4
    e = LLMEngine(cfg)
    assert e.runner.model.layers[0].self_attn.qkv_proj.mx4
    sp = SamplingParams(max_tokens=5, ignore_eos=True)
    out = e.generate([[1, 5, 9, 20, 31, 7]] * 2, sp, lora=["a", None])
    assert all(len(o) == 5 for o in out)
    assert out[0] != out[1]


def test_mx4_with_ngram_speculation_is_greedy_exact(mx4_dirs):
    prompts = [[5, 6, 7, 5, 6, 7, 5, 6], [9, 2, 6]]
    sp = SamplingParams(max_tokens=10, ignore_eos=True)
    base = _cpu_engine(model_path=mx4_dirs["mx4"]).generate(prompts, sp)
    spec = _cpu_engine(model_path=mx4_dirs["mx4"],
                       speculative="ngram").generate(prompts, sp)
    assert spec == base


def test_mx4_embeddings_equal_the_dequantized_twins(mx4_dirs):
    prompts = [[3, 1, 4, 1, 5, 9, 2, 6], [9, 2, 6]]
    for mode in ("last", "mean"):
        a = _cpu_engine(model_path=mx4_dirs["mx4"]).embed(prompts,
                                                          {"mode": mode})
        b = _cpu_engine(model_path=mx4_dirs["bf16"]).embed(prompts,
                                                           {"mode": mode})
        assert len(a) == 2
        for x, y in zip(a, b):
            assert torch.equal(torch.as_tensor(x), torch.as_tensor(y))


# ------------------------------ routing ------------------------------------
@pytest.mark.parametrize("m", [1, 16, 17, 33, 64])
@pytest.mark.parametrize("n,k", [(64, 128), (128, 384), (1024, 256),
                                 (4608, 3584), (3584, 3584), (37888, 3584),
                                 (3584, 18944), (192, 8192)])
def test_mx4_plan_is_launchable(m, n, k):
    """Whatever numbers the routing rule holds, its plans must satisfy what
    the kernel requires: whole 128-chunks (four MX blocks) per split, splits
    that cover K with none empty, a tile width that divides N."""
    nw, nsplits, kps, mrows = ops._mx4_plan(m, n, k)
    assert nw in (1, 2) and n % (64 * nw) == 0
    assert kps % 128 == 0 and kps >= 128
    assert nsplits >= 1 and (nsplits - 1) * kps < k <= nsplits * kps
    assert mrows == 16 * min(-(-m // 16), 4)
