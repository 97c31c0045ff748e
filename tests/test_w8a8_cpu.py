"""W8A8 mode (EngineConfig.w8_activations="fp8") on the CPU: the activation
quantization rule, option validation, and the flag reaching the layers."""

import pytest
import torch

import arks_amd.ops as ops
from arks_amd.config import PRESET_CONFIGS, EngineConfig
from arks_amd.engine import LLMEngine, SamplingParams
from arks_amd.loader.safetensors_loader import save_fp8_checkpoint
from arks_amd.ops import ref


def test_rule_scales_codes_and_planted_cases():
    g = torch.Generator().manual_seed(0)
    mag = torch.randint(-6, 7, (5, 3, 1), generator=g).float()
    x = (torch.randn(5, 3, 128, generator=g) * torch.exp2(mag)).view(5, 384)
    x = x.to(torch.bfloat16)
    x[4, :128] = 0.0                      # block 0: all zero
    x[4, 128:256] = x[4, 128:256].clamp(-40, 40)
    x[4, 128] = 56.0                      # block 1: amax 56 -> s = 2^-3
    x[4, 129] = 17 * 0.125                # a tie between 16 and 18
    x[4, 130] = -3 * 2.0 ** -9 * 0.125    # an e4m3 denormal
    xq, xs = ref.w8_quantize_act(x)
    assert xq.dtype == torch.float8_e4m3fn and xq.shape == (5, 384)
    assert xs.dtype == torch.float32 and xs.shape == (5, 3)
    amax = x.float().view(5, 3, 128).abs().amax(dim=2)
    assert torch.equal(xs, torch.where(amax > 0, amax / 448.0,
                                       torch.ones_like(amax)))
    codes = xq.float()
    assert codes.abs().max() == 448.0  # every row's amax maps to it; no NaN
    assert xs[4, 0] == 1.0 and not codes[4, :128].any()
    assert xs[4, 1] == 0.125
    assert codes[4, 128:131].tolist() == [448.0, 16.0, -3 * 2.0 ** -9]
    assert torch.equal(ref.w8_dequant_act(xq, xs),
                       codes * xs.repeat_interleave(128, dim=1))
    assert torch.equal(ref.w8_qdq_act(x), ref.w8_dequant_act(xq, xs))
    # the layer emulation: both dequantized operands in f32, one bf16 rounding
    w8, blocks = ref.w8_quantize(torch.randn(64, 384, generator=g) * 0.05)
    scales = ref.w8_expand_scales(blocks, 64)
    bias = torch.randn(64, generator=g).to(torch.bfloat16)
    want = (ref.w8_qdq_act(x).double()
            @ ref.w8_dequant(w8, scales).double().t() + bias.double())
    got = ref.w8a8_linear(x, w8, scales, bias)
    assert got.dtype == torch.bfloat16
    assert ((got.double() - want).abs() <= 2.0 ** -8 * want.abs() + 1e-4).all()
    assert torch.equal(ops.w8a8_gemm(xq, xs, (w8, scales), bias), got)


def test_option_needs_w8_weights_and_defaults_to_bf16(tmp_path):
    assert EngineConfig(preset="tiny").w8_activations == "bf16"
    with pytest.raises(ValueError, match="w8_activations"):
        EngineConfig(preset="tiny", w8_activations="e4m3")
    with pytest.raises(ValueError, match="w8_activations.*quantization"):
        EngineConfig(preset="tiny", quantization="int4", w8_activations="fp8")
    # a bf16 model resolves to None, or to the load-time "fp8": refused too
    for quant in (None, "fp8"):
        cfg = EngineConfig(preset="tiny", quantization=quant,
                           w8_activations="fp8")
        with pytest.raises(ValueError, match="w8_activations.*quantization"):
            cfg.resolve_quantization(PRESET_CONFIGS["tiny"])
    path = str(tmp_path / "fp8")
    save_fp8_checkpoint(PRESET_CONFIGS["tiny"], path, seed=4)
    ok = EngineConfig(model_path=path, w8_activations="fp8")
    assert ok.resolve_quantization(ok.model_config()) == "fp8_block"


def test_flag_reaches_the_layers_of_a_cpu_engine(tmp_path):
    path = str(tmp_path / "fp8")
    save_fp8_checkpoint(PRESET_CONFIGS["tiny"], path, seed=4)
    prompt = [(7 * i) % 500 + 3 for i in range(ops.W8A8_MFMA_MIN_M + 5)]
    seen = {}
    for mode in ("bf16", "fp8"):
        e = LLMEngine(EngineConfig(model_path=path, device="cpu",
                                   kv_cache_blocks=128, max_model_len=256,
                                   seed=2, w8_activations=mode))
        model = e.runner.model
        for layer in model.layers:
            for mod in (layer.self_attn.qkv_proj, layer.self_attn.o_proj,
                        layer.mlp.gate_up_proj, layer.mlp.down_proj):
                assert mod.w8 and getattr(mod, "w8_act", "bf16") == mode
        assert not hasattr(model.lm_head, "w8_act")
        got = []
        hook = model.lm_head.register_forward_hook(
            lambda m, args, out: got.append(out))
        out = e.generate([prompt], SamplingParams(max_tokens=2,
                                                  ignore_eos=True))
        hook.remove()
        assert len(out[0]) == 2
        seen[mode] = got[0][-1]  # the first call: the prefill's logits
    assert not torch.equal(seen["bf16"], seen["fp8"])
