"""W4A16 (int4 / AWQ) on the CPU: the format and reference functions, the
quantized layers, checkpoint loading, config errors and the engine modes.
The CPU emulation of a W4 layer is F.linear on the bf16-rounded dequantized
weight, so everything here compares exactly."""

import json
import os

import pytest
import torch
import torch.nn.functional as F

from arks_amd.config import PRESET_CONFIGS, EngineConfig, ModelConfig
from arks_amd.engine import LLMEngine, SamplingParams
from arks_amd.loader.safetensors_loader import (
    _chunk_complete, _dangling_names, save_awq_checkpoint,
    save_random_checkpoint,
)
from arks_amd.ops import ref
from arks_amd.parallel.layers import (
    ColumnParallelLinear, RowParallelLinear, quantize_module_w4,
)

PROMPTS = [[3, 1, 4, 1, 5], [9, 2, 6]]
SP = SamplingParams(max_tokens=6, ignore_eos=True)


def _cpu_engine(**kw):
    if "model_path" not in kw:
        kw.setdefault("preset", "tiny")
    return LLMEngine(EngineConfig(device="cpu", kv_cache_blocks=128,
                                  max_model_len=256, seed=2, **kw))


# ------------------------------ format ------------------------------------
def test_awq_pack_unpack_roundtrip_and_known_word():
    g = torch.Generator().manual_seed(0)
    q = torch.randint(0, 16, (64, 256), generator=g, dtype=torch.uint8)
    z = torch.randint(0, 16, (64, 2), generator=g, dtype=torch.uint8)
    s = torch.rand(64, 2, generator=g).half().float()
    qweight, qzeros, scales = ref.awq_pack(q, z, s)
    assert qweight.dtype == torch.int32 and qweight.shape == (256, 8)
    assert qzeros.dtype == torch.int32 and qzeros.shape == (2, 8)
    assert scales.dtype == torch.float16 and scales.shape == (2, 64)
    q2, z2, s2 = ref.awq_unpack(qweight, qzeros, scales)
    assert torch.equal(q2, q) and torch.equal(z2, z) and torch.equal(s2, s)

    # logical columns 0..7 of one K row (the 1x8 case, repeated down the one
    # 128-group): nibble i holds column order[i], order = 0,2,4,6,1,3,5,7
    q = torch.arange(8, dtype=torch.uint8)[:, None].expand(8, 128).contiguous()
    qweight, _, _ = ref.awq_pack(q, torch.zeros(8, 1, dtype=torch.uint8),
                                 torch.ones(8, 1))
    assert qweight.shape == (128, 1)
    assert all((w & 0xFFFFFFFF) == 0x75316420 for w in qweight[:, 0].tolist())


def test_internal_pack_roundtrip_and_layout():
    g = torch.Generator().manual_seed(1)
    q = torch.randint(0, 16, (16, 256), generator=g, dtype=torch.uint8)
    z = torch.randint(0, 16, (16, 2), generator=g, dtype=torch.uint8)
    s = torch.rand(16, 2, generator=g).half().float()
    packed = ref.w4_pack(q, z, s)
    assert packed[0].shape == (16, 32) and packed[0].dtype == torch.int32
    assert packed[1].shape == (2, 16) and packed[1].dtype == torch.float16
    assert packed[2].shape == (2, 16) and packed[2].dtype == torch.uint8
    for a, b in zip(ref.w4_unpack(packed), (q, z, s)):
        assert torch.equal(a, b)
    # row-major over N: a row slice of the packed tensor is that row's weights
    sub = (packed[0][4:8], packed[1][:, 4:8], packed[2][:, 4:8])
    assert torch.equal(ref.w4_unpack(sub)[0], q[4:8])
    # elements 2p and 2p+1 of a word sit in nibbles p and p+4
    word = packed[0][3, 5].item() & 0xFFFFFFFF
    for e in range(8):
        nib = (e % 2) * 4 + e // 2
        assert (word >> (4 * nib)) & 0xF == q[3, 40 + e].item()


def test_group_size_other_than_128_rejected():
    with pytest.raises(ValueError, match="multiple of the group size 128"):
        ref.w4_quantize(torch.zeros(8, 192))
    qweight = torch.zeros(128, 1, dtype=torch.int32)
    with pytest.raises(ValueError, match="group size 128"):
        ref.awq_unpack(qweight, torch.zeros(2, 1, dtype=torch.int32),
                       torch.zeros(2, 8, dtype=torch.float16))  # group 64


def test_quantize_dequant_error_at_most_half_a_step():
    torch.manual_seed(2)
    w = (torch.randn(32, 384) * 0.05).to(torch.bfloat16)
    w[0, :128] = 0.25       # constant group
    w[1, 128:256] = 0.0     # all-zero group
    w[2, :128] = w[2, :128].abs() + 0.01   # all-positive group
    w[3, :128] = -w[3, :128].abs() - 0.01  # all-negative group
    q, z, s = ref.w4_quantize(w)
    assert q.dtype == torch.uint8 and z.dtype == torch.uint8
    assert int(q.max()) <= 15 and int(z.max()) <= 15
    assert torch.isfinite(s).all() and (s > 0).all()
    assert torch.equal(s, s.half().float())  # stored at f16 precision
    d = ref.w4_dequant(q, z, s)
    assert torch.isfinite(d).all()
    err = (d - w.float()).abs().reshape(32, 3, 128)
    # half a step, plus the f32 rounding of w/s and of (q - z) * s: a few
    # ulps of values below 16 steps, i.e. < 16 * 2^-22 of a step
    assert (err <= s[..., None] * (0.5 + 1e-5)).all()


# ------------------------------ layers ------------------------------------
@pytest.mark.parametrize("kind", ["column", "row"])
def test_quantized_layer_equals_linear_on_dequantized_weight(kind):
    torch.manual_seed(3)
    if kind == "column":
        lin = ColumnParallelLinear(128, 96, bias=True)
        lin.bias.data.normal_(0, 0.05)
        x = torch.randn(7, 128, dtype=torch.bfloat16)
    else:
        lin = RowParallelLinear(256, 64, bias=False)
        x = torch.randn(7, 256, dtype=torch.bfloat16)
    lin.weight.data.normal_(0, 0.05)
    w = lin.weight.data.clone()
    quantize_module_w4(lin, kind)
    assert lin.w4 and lin.weight is None
    assert "weight" not in dict(lin.named_parameters())
    wd = ref.w4_dequant(*ref.w4_quantize(w)).to(torch.bfloat16)
    assert torch.equal(lin(x), F.linear(x, wd, lin.bias))
    # and ops.w4_linear's CPU path is the same definition
    import arks_amd.ops as ops
    packed = (lin.w4_qweight, lin.w4_scales, lin.w4_zeros)
    assert torch.equal(ops.w4_linear(x, packed, lin.bias),
                       F.linear(x, wd, lin.bias))


def test_layer_with_k_off_the_group_raises_naming_it():
    lin = RowParallelLinear(192, 64, bias=False)
    with pytest.raises(ValueError, match=r"layers\.3\.mlp\.down_proj.*K=192"):
        quantize_module_w4(lin, "layers.3.mlp.down_proj")


# ------------------------------ engine ------------------------------------
def test_engine_int4_cpu_runs_deterministic():
    a = _cpu_engine(quantization="int4").generate(PROMPTS, SP)
    e = _cpu_engine(quantization="int4")
    layer = e.runner.model.layers[0]
    for mod in (layer.self_attn.qkv_proj, layer.self_attn.o_proj,
                layer.mlp.gate_up_proj, layer.mlp.down_proj):
        assert mod.w4 and mod.weight is None
    assert not getattr(e.runner.model.lm_head, "w4", False)
    b = e.generate(PROMPTS, SP)
    assert a == b and all(len(o) == 6 for o in a)
    # it is not the bf16 model
    plain = _cpu_engine()
    w = plain.runner.model.layers[0].mlp.down_proj.weight
    assert not torch.equal(layer.mlp.down_proj.weight_qdq, w)


def test_engine_int4_moe_keeps_experts_bf16():
    e = _cpu_engine(preset="tiny-moe", quantization="int4")
    layer = e.runner.model.layers[0]
    assert layer.self_attn.qkv_proj.w4
    assert layer.mlp.w13.dtype == torch.bfloat16
    out = e.generate(PROMPTS, SP)
    assert all(len(o) == 6 for o in out)


@pytest.fixture(scope="module")
def awq_dirs(tmp_path_factory):
    root = tmp_path_factory.mktemp("awq")
    dirs = {k: str(root / k) for k in ("awq", "bf16", "split")}
    cfg = PRESET_CONFIGS["tiny"]
    save_awq_checkpoint(cfg, dirs["awq"], seed=4, dequantized_dir=dirs["bf16"])
    save_awq_checkpoint(cfg, dirs["split"], seed=4, split_files=True)
    return dirs


def _model_logits(engine, prompt):
    """Last-position logits of one prefill through the engine's model."""
    runner = engine.runner
    seq = engine.add_request(list(prompt), SamplingParams(max_tokens=1,
                                                          ignore_eos=True))
    captured = {}
    real = runner.model.forward

    def spy(batch, kv):
        out = real(batch, kv)
        captured.setdefault("logits", out.detach().clone())
        return out

    runner.model.forward = spy
    try:
        while engine.has_work():
            engine.step()
    finally:
        runner.model.forward = real
    assert seq.output_token_ids
    return captured["logits"][-1]


@pytest.mark.parametrize("which", ["awq", "split"])
def test_awq_checkpoint_equals_its_dequantized_bf16_model(awq_dirs, which):
    if which == "split":
        files = sorted(f for f in os.listdir(awq_dirs["split"])
                       if f.endswith(".safetensors"))
        assert len(files) == 2
        from safetensors import safe_open
        with safe_open(os.path.join(awq_dirs["split"], files[0]), "pt") as f:
            names0 = set(f.keys())
        assert any(".gate_proj.qweight" in n for n in names0)
        assert not any(".up_proj." in n for n in names0)
    e_awq = _cpu_engine(model_path=awq_dirs[which])  # auto-detected
    assert e_awq.runner.quantization == "awq"
    layer = e_awq.runner.model.layers[1]
    assert layer.mlp.gate_up_proj.w4 and layer.self_attn.o_proj.w4
    e_ref = _cpu_engine(model_path=awq_dirs["bf16"])
    assert e_ref.runner.quantization is None
    assert torch.equal(layer.mlp.gate_up_proj.weight_qdq,
                       e_ref.runner.model.layers[1].mlp.gate_up_proj.weight)
    assert e_awq.generate(PROMPTS, SP) == e_ref.generate(PROMPTS, SP)
    la = _model_logits(e_awq, PROMPTS[0])
    lr = _model_logits(e_ref, PROMPTS[0])
    assert la.shape == lr.shape and torch.equal(la, lr)


def test_explicit_awq_flag_on_awq_checkpoint(awq_dirs):
    e = _cpu_engine(model_path=awq_dirs["awq"], quantization="awq")
    assert all(len(o) == 6 for o in e.generate(PROMPTS, SP))


def test_loader_partner_groups_use_their_own_suffix():
    pre = "model.layers.0.mlp"
    chunk = {f"{pre}.gate_proj.qweight": 0, f"{pre}.gate_proj.scales": 0,
             f"{pre}.up_proj.scales": 0}
    assert not _chunk_complete(chunk)
    assert _dangling_names(chunk) == {f"{pre}.gate_proj.qweight"}
    chunk[f"{pre}.up_proj.qweight"] = 0
    assert _chunk_complete(chunk) and not _dangling_names(chunk)
    att = "model.layers.0.self_attn"
    chunk = {f"{att}.q_proj.qzeros": 0, f"{att}.k_proj.qzeros": 0}
    assert _dangling_names(chunk) == set(chunk)
    # plain checkpoints: unchanged
    chunk = {f"{pre}.gate_proj.weight": 0}
    assert not _chunk_complete(chunk)
    chunk[f"{pre}.up_proj.weight"] = 0
    assert _chunk_complete(chunk)


# --------------------------- config errors --------------------------------
def _edit_config(path, **qc):
    cfg_path = os.path.join(path, "config.json")
    with open(cfg_path) as f:
        cfg = json.load(f)
    cfg["quantization_config"].update(qc)
    with open(cfg_path, "w") as f:
        json.dump(cfg, f)


@pytest.mark.parametrize("field,value", [
    ("group_size", 64), ("bits", 8), ("zero_point", False),
    ("version", "gemv"), ("quant_method", "gptq"),
])
def test_unsupported_quantization_config_names_the_field(tmp_path, field,
                                                         value):
    hf = {"architectures": ["Qwen2ForCausalLM"],
          "quantization_config": {"quant_method": "awq", "bits": 4,
                                  "group_size": 128, "zero_point": True,
                                  "version": "GEMM"}}
    assert ModelConfig.from_hf_config(hf).quant_method == "awq"
    hf["quantization_config"][field] = value
    with open(tmp_path / "config.json", "w") as f:
        json.dump(hf, f)
    with pytest.raises(ValueError, match=field):
        ModelConfig.from_pretrained(str(tmp_path))


def test_awq_flag_on_bf16_checkpoint_raises(awq_dirs):
    with pytest.raises(ValueError, match="needs an AWQ checkpoint"):
        _cpu_engine(model_path=awq_dirs["bf16"], quantization="awq")
    with pytest.raises(ValueError, match="needs an AWQ checkpoint"):
        _cpu_engine(quantization="awq")  # a preset is not one either


@pytest.mark.parametrize("mode", ["fp8", "int4"])
def test_other_modes_on_awq_checkpoint_raise(awq_dirs, mode):
    with pytest.raises(ValueError, match="AWQ checkpoint"):
        _cpu_engine(model_path=awq_dirs["awq"], quantization=mode)


def test_unknown_quantization_raises():
    with pytest.raises(ValueError, match="unknown quantization 'int3'"):
        EngineConfig(preset="tiny", quantization="int3")


def test_moe_awq_checkpoint_not_supported(tmp_path):
    path = str(tmp_path / "moe")
    save_random_checkpoint(PRESET_CONFIGS["tiny-moe"], path, seed=1)
    cfg_path = os.path.join(path, "config.json")
    with open(cfg_path) as f:
        cfg = json.load(f)
    cfg["num_local_experts"] = 4
    cfg["quantization_config"] = {"quant_method": "awq", "bits": 4,
                                  "group_size": 128, "zero_point": True,
                                  "version": "gemm"}
    with open(cfg_path, "w") as f:
        json.dump(cfg, f)
    with pytest.raises(ValueError, match="MoE.*not supported"):
        _cpu_engine(model_path=path)


# ------------------------------- LoRA --------------------------------------
def test_int4_with_lora_constructs_and_generates(tmp_path):
    from lora_testutil import engine_cfg, make_adapters

    adapters = make_adapters("tiny", tmp_path)
    sp = SamplingParams(max_tokens=5, ignore_eos=True)
    e = LLMEngine(engine_cfg("tiny", "cpu", enable_lora=True,
                             lora_modules=adapters, quantization="int4"))
    assert e.runner.model.layers[0].self_attn.qkv_proj.w4
    out = e.generate([[1, 5, 9, 20, 31, 7]] * 2, sp, lora=["a", None])
    assert all(len(o) == 5 for o in out)
    assert out[0] != out[1]  # the adapter's delta reaches the W4 layers


# ------------------------------ routing ------------------------------------
@pytest.mark.parametrize("m", [1, 16, 17, 33, 64])
@pytest.mark.parametrize("n,k", [(64, 128), (128, 384), (1024, 256),
                                 (4608, 3584), (3584, 3584), (37888, 3584),
                                 (3584, 18944), (192, 8192)])
def test_w4_plan_is_launchable(m, n, k):
    """Whatever numbers the routing rule holds, its plans must satisfy what
    the kernel requires: whole 128-groups per split, splits that cover K
    with none empty, a tile width that divides N."""
    import arks_amd.ops as ops

    nw, nsplits, kps, mrows = ops._w4_plan(m, n, k)
    assert nw in (1, 2) and n % (64 * nw) == 0
    assert kps % 128 == 0 and kps >= 128
    assert nsplits >= 1 and (nsplits - 1) * kps < k <= nsplits * kps
    assert mrows == 16 * min(-(-m // 16), 4)
