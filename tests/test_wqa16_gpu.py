"""Fused-dequant W4 / W8 / MX4 x bf16 MFMA GEMM (wqa16_mfma_gemm.hip) on the
GPU: the kernel against the dequantized weight in f32, the routing of the
*_linear ops above the slab limit, and the int4 engine through a prefill that
runs it."""

import pytest
import torch

import arks_amd.ops as ops
from arks_amd.config import EngineConfig
from arks_amd.engine import LLMEngine, SamplingParams
from arks_amd.ops import ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
FMTS = ("w4", "w8", "mx4")
MTILES = (64, 128)


def _weight(fmt, n, k, seed):
    """(weight tuple on the GPU, its dequantized bf16 [n, k] on the GPU) from
    random weights of std ~0.05 with ordinary scales."""
    g = torch.Generator().manual_seed(seed)
    if fmt == "w4":
        q = torch.randint(0, 16, (n, k), generator=g, dtype=torch.uint8)
        z = torch.randint(0, 16, (n, k // 128), generator=g, dtype=torch.uint8)
        s = (0.0077 * (0.5 + torch.rand(n, k // 128, generator=g))).half()
        weight, wd = ref.w4_pack(q, z, s.float()), ref.w4_dequant(q, z,
                                                                  s.float())
    elif fmt == "w8":
        w8, blocks = ref.w8_quantize(torch.randn(n, k, generator=g) * 0.05)
        weight = (w8, ref.w8_expand_scales(blocks, n))
        wd = ref.w8_dequant(*weight)
    else:
        weight = ref.mx4_quantize(torch.randn(n, k, generator=g) * 0.05)
        wd = ref.mx4_dequant(*weight)
    return (tuple(t.to(DEV) for t in weight),
            wd.to(torch.bfloat16).to(DEV))


def _gemm(fmt):
    return getattr(ops, fmt + "a16_gemm")


@pytest.mark.parametrize("mtile", MTILES)
@pytest.mark.parametrize("fmt", FMTS)
def test_exact_mapping(fmt, mtile):
    """One-hot activations leave one non-zero product per output, so every
    f32 sum is exact and row r must be column k of the bf16 dequantized
    weight bit for bit: nibble / byte order, scale and zero lanes, the LDS
    swizzle, the fragment mapping, the M tail (200 = 128 + 72), the wave past
    N = 192 and a three-stage K loop."""
    assert ops.native_available()
    m, n, k = 200, 192, 384
    weight, wd = _weight(fmt, n, k, 3)
    rows = torch.arange(m, device=DEV)
    for c in (0, 1):
        cols = (rows + 200 * c) % k
        x = torch.zeros(m, k, dtype=torch.bfloat16, device=DEV)
        x[rows, cols] = 1.0
        out = _gemm(fmt)(x, weight, mtile=mtile)
        assert out.dtype == torch.bfloat16 and out.shape == (m, n)
        assert torch.equal(out, wd[:, cols].t()), (fmt, mtile, c)


@pytest.mark.parametrize("mtile", MTILES)
@pytest.mark.parametrize("m,n,k", [(129, 128, 512), (200, 192, 640),
                                   (272, 256, 1024)])
@pytest.mark.parametrize("fmt", FMTS)
def test_numerics(fmt, m, n, k, mtile):
    """|out - y| <= 2^-8 |y| + K 2^-23 T against y = x @ Wd^T + bias in f32,
    T the same sum over magnitudes: bf16 products are exact in f32, K f32
    additions of either order each err by at most 2^-24 of the running
    magnitude, the final bf16 rounding by 2^-9 relative; a factor two of slack
    on each."""
    assert ops.native_available()
    weight, wd = _weight(fmt, n, k, 5)
    torch.manual_seed(7)
    x = torch.randn(m, k, dtype=torch.bfloat16, device=DEV) * 0.5
    bias = torch.randn(n, dtype=torch.bfloat16, device=DEV)
    wide = torch.zeros(m, k + 64, dtype=torch.bfloat16, device=DEV)
    wide[:, :k] = x  # a row-strided view of the same values
    for b in (None, bias):
        y = x.float() @ wd.float().t()
        t = x.float().abs() @ wd.float().abs().t()
        if b is not None:
            y, t = y + b.float(), t + b.float().abs()
        out = _gemm(fmt)(x, weight, b, mtile=mtile)
        tol = 2.0 ** -8 * y.abs() + k * 2.0 ** -23 * t
        err = (out.float() - y).abs()
        print(f"{fmt} {(m, n, k)} mtile={mtile} bias={b is not None}: "
              f"max err/tol = {(err / tol).max().item():.3f}")
        assert (err <= tol).all()
        assert torch.equal(_gemm(fmt)(wide[:, :k], weight, b, mtile=mtile),
                           out)


@pytest.mark.parametrize(
    "fmt", [f for f in FMTS if ops.wqa16_min_m(f, 256, 1024) is not None])
def test_route(fmt):
    """Above the slab limit {fmt}_linear is the new kernel from the M the
    rule names; at M = 64 it is still the skinny kernel with its own plan."""
    assert ops.native_available()
    n, k = 256, 1024
    m = ops.wqa16_min_m(fmt, n, k)
    assert m > 128
    weight, _ = _weight(fmt, n, k, 11)
    ops.reserve_dequant_workspace(n * k, DEV)
    torch.manual_seed(13)
    x = torch.randn(m, k, dtype=torch.bfloat16, device=DEV) * 0.5
    bias = torch.randn(n, dtype=torch.bfloat16, device=DEV)
    linear = getattr(ops, fmt + "_linear")
    assert torch.equal(linear(x, weight, bias), _gemm(fmt)(x, weight, bias))
    skinny = ops._wq_skinny(getattr(ops, "_" + fmt.upper()), x[:64], weight,
                            bias, False, None)
    assert torch.equal(linear(x[:64], weight, bias), skinny)


def test_engine_int4_long_prompt_graph_equals_eager_and_deterministic():
    """A 300-token prompt prefills through the new kernel; greedy outputs
    agree across fresh engines and between captured and eager decode."""
    assert ops.native_available()
    prompts = [[(5 * i) % 2000 + 1 for i in range(300)],
               [1, 5, 9, 20, 7, 3], [2, 4, 6], [11, 12, 13, 14]]
    sp = SamplingParams(max_tokens=8, ignore_eos=True)
    outs = []
    for eager in (False, True, False):
        e = LLMEngine(EngineConfig(
            device="cuda", kv_cache_blocks=512, max_model_len=1024, seed=5,
            preset="tiny-gpu", quantization="int4", enforce_eager=eager))
        outs.append(e.generate(prompts, sp))
        del e
    assert all(len(o) == 8 for o in outs[0])
    assert outs[0] == outs[1] == outs[2]
