"""W4A4 MX kernels on the GPU: the activation quantizer (mx4_act_quant_kernel)
against the conversion rule, the scaled-MFMA GEMM (mx4_mfma_gemm_kernel) and
the layer entry against float64, and the engine with MX activations.

Tolerance of the GEMM checks, derived: the products of two e2m1 values times
powers of two are exact, the kernel sums K of them in f32 and rounds once to
bf16, so |y - ref| <= 2^-8 |y| (bf16 rounding, 2^-9, with a factor two of
slack) + K 2^-23 (|x^| @ |w^|^T) (f32 accumulation)."""

import functools

import pytest
import torch

import arks_amd.ops as ops
from arks_amd.config import PRESET_CONFIGS, EngineConfig
from arks_amd.engine import LLMEngine, SamplingParams
from arks_amd.ops import ref

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _blocks(rows, k, seed):
    """bf16 [rows, k] on the CPU: normal noise times a power of two, 2^-6 to
    2^6, drawn per MX block, so scale bytes vary along every row."""
    g = torch.Generator().manual_seed(seed)
    mag = torch.randint(-6, 7, (rows, k // 32, 1), generator=g).float()
    x = torch.randn(rows, k // 32, 32, generator=g) * torch.exp2(mag)
    return x.view(rows, k).to(torch.bfloat16)


@pytest.mark.parametrize("m,k,strided", [
    (1, 128, False), (1, 384, False), (3, 128, False), (3, 384, False),
    (67, 128, False), (67, 384, False), (67, 384, True)])
def test_quantizer_follows_the_rule(m, k, strided):
    assert ops.native_available()
    x = _blocks(m, k + 64 if strided else k, 10 * m + k)
    r = m - 1  # planted in the last row, blocks 0..3 of its first 128 k
    x[r, :32] = 0.0                                    # block 0: all zero
    x[r, 64:128] = 0.0
    x[r, 32:64] *= 2.0 ** -9
    x[r, 40], x[r, 41] = 8.0, -2.0 ** -20              # amax = 2^3; tiny < 0
    ties = torch.tensor([0.25, 0.75, 1.25, 2.5, 5.0])  # block 2: scale 2^-3
    x[r, 64:74] = (torch.cat([ties, -ties]) * 0.125).to(torch.bfloat16)
    x[r, 96:100] = torch.tensor([6.5, 7.0, -7.5, 6.25]).to(
        torch.bfloat16) * 4.0                          # block 3: (6, 8) * 2^2
    x = x.to(DEV)
    if strided:
        x = x[:, :k]
        assert x.stride(0) > k
    q_ref, s_ref = ref.mx4_quantize(x.cpu())
    want = ref.mx4_dequant(q_ref, s_ref)
    assert s_ref[r, :4].tolist() == [127, 128, 124, 129]
    xq, xs = ops.mx4_quantize_act(x)
    assert xq.shape == (m, k // 2) and xs.shape == (m, k // 32)
    assert torch.equal(xs.cpu(), s_ref)
    assert torch.equal(ref.mx4_dequant(xq.cpu(), xs.cpu()), want)  # -0 == 0
    xhat = ops.mx4_quantize_act(x, qdq=True)
    assert xhat.dtype == torch.bfloat16 and xhat.is_contiguous()
    assert torch.equal(xhat.float().cpu(), want)


@functools.lru_cache(maxsize=None)
def _problem(m, n, k):
    """CPU-quantized operands, bias, and the float64 product with its
    accumulation bound K 2^-23 |x^| @ |w^|^T."""
    xq, xs = ref.mx4_quantize(_blocks(m, k, 7 * m + n + k))
    weight = ref.mx4_quantize(_blocks(n, k, m + 3 * n + k + 1))
    bias = _blocks(1, n, n)[0]
    xd = ref.mx4_dequant(xq, xs).double()
    wd = ref.mx4_dequant(*weight).double()
    return ((xq, xs), weight, bias, xd @ wd.t(),
            k * 2.0 ** -23 * (xd.abs() @ wd.abs().t()))


def _check(out, y, acc_bound):
    err = (out.double().cpu() - y).abs()
    tol = 2.0 ** -8 * y.abs() + acc_bound
    assert (err <= tol).all(), (err - tol).max().item()


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("mtile", [64, 128])
@pytest.mark.parametrize("m,n,k", [
    (1, 64, 128), (17, 192, 384), (129, 128, 512), (200, 192, 640),
    (272, 256, 1024), (64, 64, 1536)])
def test_mfma_gemm_against_float64(m, n, k, mtile, with_bias):
    assert ops.native_available()
    (xq, xs), weight, bias, y, acc_bound = _problem(m, n, k)
    if with_bias:
        y = y + bias.double()
    out = ops.mx4a4_gemm(xq.to(DEV), xs.to(DEV),
                         tuple(t.to(DEV) for t in weight),
                         bias.to(DEV) if with_bias else None, mtile=mtile)
    assert out.shape == (m, n) and out.dtype == torch.bfloat16
    _check(out, y, acc_bound)


@pytest.mark.parametrize("m", [1, 16, 64, 100, 128, 129, 200])
def test_layer_entry_on_both_sides_of_the_routing_boundary(m):
    assert ops.native_available()
    ms = (1, 16, 64, 100, 128, 129, 200)
    assert min(ms) < ops.MX4A4_MFMA_MIN_M <= max(ms)  # both routes run
    n, k = 192, 384
    _, weight, bias, _, _ = _problem(200, n, k)
    x = _blocks(m, k, 50 + m)
    xd = ref.mx4_qdq(x).double()
    wd = ref.mx4_dequant(*weight).double()
    out = ops.mx4a4_linear(x.to(DEV), tuple(t.to(DEV) for t in weight),
                           bias.to(DEV))
    assert out.shape == (m, n) and out.dtype == torch.bfloat16
    _check(out, xd @ wd.t() + bias.double(),
           k * 2.0 ** -23 * (xd.abs() @ wd.abs().t()))


def test_engine_with_mx_activations_graph_equals_eager(tmp_path):
    from arks_amd.loader.safetensors_loader import save_mx4_checkpoint

    assert ops.native_available()
    path = str(tmp_path / "mx4")
    save_mx4_checkpoint(PRESET_CONFIGS["tiny-gpu"], path, seed=3)
    long = [(7 * i) % 2000 + 1 for i in range(ops.MX4A4_MFMA_MIN_M + 11)]
    prompts = [long, [2, 4, 6], [11, 12, 13, 14]]
    sp = SamplingParams(max_tokens=4, ignore_eos=True)
    outs = []
    for eager in (False, True, False):
        e = LLMEngine(EngineConfig(model_path=path, device="cuda",
                                   kv_cache_blocks=512, max_model_len=1024,
                                   seed=5, enforce_eager=eager,
                                   mx_activations="mxfp4"))
        layer = e.runner.model.layers[0]
        for mod in (layer.self_attn.qkv_proj, layer.self_attn.o_proj,
                    layer.mlp.gate_up_proj, layer.mlp.down_proj):
            assert mod.mx4 and mod.mx4_act == "mxfp4"
        assert not hasattr(e.runner.model.lm_head, "mx4_act")
        outs.append(e.generate(prompts, sp))
        del e
    assert all(len(o) == 4 for o in outs[0])
    assert outs[0] == outs[1] == outs[2]
