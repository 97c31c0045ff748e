"""W8A8 kernels on the GPU: the activation quantizer (w8_act_quant_kernel)
against the rule, the FP8 MFMA GEMM (w8_mfma_gemm_kernel) and the layer entry
against float64, and the engine with FP8 activations.

Tolerance of the GEMM checks, derived. With T = |x^| @ |w^|^T in float64:
  |out - y| <= 2^-8 |y| + (K + 256) 2^-23 T.
The products of two e4m3 codes are exact in f32 and each k-block sums 128 of
them; the scale product, the FMA and the K/128 outer additions round once
each, which the constant 256 covers with room to spare; the bf16 rounding
(2^-9) carries a factor two of slack."""

import functools

import pytest
import torch

import arks_amd.ops as ops
from arks_amd.config import PRESET_CONFIGS, EngineConfig
from arks_amd.engine import LLMEngine, SamplingParams
from arks_amd.ops import ref

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _blocks(rows, k, seed, scale=1.0):
    """bf16 [rows, k] on the CPU: normal noise times a power of two, 2^-6 to
    2^6, drawn per 128-block, so the scales vary along every row."""
    g = torch.Generator().manual_seed(seed)
    mag = torch.randint(-6, 7, (rows, k // 128, 1), generator=g).float()
    x = torch.randn(rows, k // 128, 128, generator=g) * torch.exp2(mag)
    return (x.view(rows, k) * scale).to(torch.bfloat16)


@pytest.mark.parametrize("m,k,strided", [
    (1, 128, False), (3, 384, False), (67, 128, False), (67, 384, False),
    (67, 384, True)])
def test_quantizer_follows_the_rule(m, k, strided):
    assert ops.native_available()
    x = _blocks(m, k + 128 if strided else k, 10 * m + k)
    r = m - 1  # planted in the last row
    x[r, :128] = x[r, :128].clamp(-40, 40)
    x[r, 0] = 56.0                      # amax 56 -> s = 2^-3, code 448
    x[r, 1] = 17 * 0.125                # a tie between 16 and 18
    x[r, 2] = -3 * 2.0 ** -9 * 0.125    # an e4m3 denormal
    if k > 128:
        x[r, 128:256] = 0.0             # an all-zero block
    x = x.to(DEV)
    if strided:
        x = x[:, :k]
        assert x.stride(0) > k
    q_ref, s_ref = ref.w8_quantize_act(x.cpu())
    assert s_ref[r, 0] == 0.125 and q_ref[r, :3].float().tolist() == [
        448.0, 16.0, -3 * 2.0 ** -9]
    assert k == 128 or s_ref[r, 1] == 1.0
    xq, xs = ops.w8_quantize_act(x)
    assert xq.shape == (m, k) and xq.dtype == torch.float8_e4m3fn
    assert xs.shape == (m, k // 128) and xs.dtype == torch.float32
    assert torch.equal(xs.cpu(), s_ref)
    assert torch.equal(ref.w8_dequant_act(xq.cpu(), xs.cpu()),
                       ref.w8_dequant_act(q_ref, s_ref))  # -0 == 0


@functools.lru_cache(maxsize=None)
def _problem(m, n, k, per_column=False):
    """CPU-quantized operands, bias, the float64 product and T = |x^| @
    |w^|^T. per_column: every (k-block, column) scale drawn on its own
    instead of expanded from 128 x 128 blocks."""
    xq, xs = ref.w8_quantize_act(_blocks(m, k, 7 * m + n + k))
    w8, blocks = ref.w8_quantize(_blocks(n, k, m + 3 * n + k + 1, 0.05))
    scales = ref.w8_expand_scales(blocks, n)
    if per_column:
        g = torch.Generator().manual_seed(n + k)
        scales = scales * (0.5 + torch.rand(scales.shape, generator=g))
    bias = _blocks(1, 128 * -(-n // 128), n)[0, :n].contiguous()
    xd = ref.w8_dequant_act(xq, xs).double()
    wd = ref.w8_dequant(w8, scales).double()
    return (xq, xs), (w8, scales), bias, xd @ wd.t(), xd.abs() @ wd.abs().t()


def _check(out, y, T, k):
    err = (out.double().cpu() - y).abs()
    tol = 2.0 ** -8 * y.abs() + (k + 256) * 2.0 ** -23 * T
    print("max err / tol:", (err / tol.clamp_min(1e-300)).max().item())
    assert (err <= tol).all(), (err - tol).max().item()


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("mtile", [64, 128])
@pytest.mark.parametrize("m,n,k,per_column", [
    (1, 64, 128, False), (17, 192, 384, False), (129, 128, 512, False),
    (200, 192, 640, False), (272, 256, 1024, False), (200, 192, 640, True)])
def test_mfma_gemm_against_float64(m, n, k, per_column, mtile, with_bias):
    assert ops.native_available()
    (xq, xs), weight, bias, y, T = _problem(m, n, k, per_column)
    if with_bias:
        y = y + bias.double()
    out = ops.w8a8_gemm(xq.to(DEV), xs.to(DEV),
                        tuple(t.to(DEV) for t in weight),
                        bias.to(DEV) if with_bias else None, mtile=mtile)
    assert out.shape == (m, n) and out.dtype == torch.bfloat16
    _check(out, y, T, k)


@pytest.mark.parametrize("m", [1, 64, 128, 129, 200])
def test_layer_entry_on_both_sides_of_the_routing_boundary(m):
    assert ops.native_available()
    ms = (1, 64, 128, 129, 200)
    assert min(ms) < ops.W8A8_MFMA_MIN_M <= max(ms)  # both routes run
    n, k = 192, 384
    _, weight, bias, _, _ = _problem(200, n, k)
    weight = tuple(t.to(DEV) for t in weight)
    x = _blocks(m, k, 50 + m)
    out = ops.w8a8_linear(x.to(DEV), weight, bias.to(DEV))
    assert out.shape == (m, n) and out.dtype == torch.bfloat16
    if m < ops.W8A8_MFMA_MIN_M:
        assert torch.equal(out, ops.w8_linear(x.to(DEV), weight,
                                              bias.to(DEV)))
        return
    xd = ref.w8_qdq_act(x).double()
    wd = ref.w8_dequant(*(t.cpu() for t in weight)).double()
    _check(out, xd @ wd.t() + bias.double(), xd.abs() @ wd.abs().t(), k)


def test_engine_with_fp8_activations_graph_equals_eager(tmp_path):
    from arks_amd.loader.safetensors_loader import save_fp8_checkpoint

    assert ops.native_available()
    path = str(tmp_path / "fp8")
    save_fp8_checkpoint(PRESET_CONFIGS["tiny-gpu"], path, seed=3)
    long = [(7 * i) % 2000 + 1 for i in range(ops.W8A8_MFMA_MIN_M + 11)]
    prompts = [long, [2, 4, 6], [11, 12, 13, 14]]
    sp = SamplingParams(max_tokens=4, ignore_eos=True)
    outs = []
    for eager in (False, True, False):
        e = LLMEngine(EngineConfig(model_path=path, device="cuda",
                                   kv_cache_blocks=512, max_model_len=1024,
                                   seed=5, enforce_eager=eager,
                                   w8_activations="fp8"))
        layer = e.runner.model.layers[0]
        for mod in (layer.self_attn.qkv_proj, layer.self_attn.o_proj,
                    layer.mlp.gate_up_proj, layer.mlp.down_proj):
            assert mod.w8 and mod.w8_act == "fp8"
        assert not hasattr(e.runner.model.lm_head, "w8_act")
        outs.append(e.generate(prompts, sp))
        del e
    assert all(len(o) == 4 for o in outs[0])
    assert outs[0] == outs[1] == outs[2]
