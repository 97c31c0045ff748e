"""Routed fused-dequant W4 / W8 / MX4 x bf16 MFMA GEMM
(wqa16_moe_mfma_gemm_kernel) on the GPU: the kernel against the bf16
dequantized experts, the MoEMLP routing above DENSE_TOKENS and the int4 engine
through a prefill that runs it."""

import functools

import pytest
import torch
import torch.nn.functional as F

import arks_amd.ops as ops
from arks_amd.config import PRESET_CONFIGS, EngineConfig
from arks_amd.engine import LLMEngine, SamplingParams
from arks_amd.models.llama_family import MoEMLP
from arks_amd.ops import ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
FMTS = ("w4", "w8", "mx4")
MTILES = (64, 128)


def _one(fmt, n, k, g):
    """(weight tuple, f32 dequantized [n, k]) of one random expert."""
    if fmt == "w4":
        q = torch.randint(0, 16, (n, k), generator=g, dtype=torch.uint8)
        z = torch.randint(0, 16, (n, k // 128), generator=g, dtype=torch.uint8)
        s = (0.0077 * (0.5 + torch.rand(n, k // 128, generator=g))).half()
        return ref.w4_pack(q, z, s.float()), ref.w4_dequant(q, z, s.float())
    if fmt == "w8":
        w8, blocks = ref.w8_quantize(torch.randn(n, k, generator=g) * 0.05)
        sc = ref.w8_expand_scales(blocks, n) * (0.5 + torch.rand(
            k // 128, n, generator=g))       # per row and k-block
        return (w8.view(torch.uint8), sc), ref.w8_dequant(w8, sc)
    weight = ref.mx4_quantize(torch.randn(n, k, generator=g) * 0.05)
    return weight, ref.mx4_dequant(*weight)


@functools.lru_cache(maxsize=None)
def _experts(fmt, E, n, k):
    """(stacked experts on the GPU as MoEMLP holds them, their bf16
    dequantized weights [E, n, k] on the CPU), distinct per expert."""
    g = torch.Generator().manual_seed(3 + n + k)
    ws, wds = zip(*[_one(fmt, n, k, g) for _ in range(E)])
    weight = [torch.stack(t).to(DEV) for t in zip(*ws)]
    if fmt == "w8":
        weight[0] = weight[0].view(torch.float8_e4m3fn)
    return tuple(weight), torch.stack(wds).to(torch.bfloat16)


def _gemm(fmt):
    return getattr(ops, fmt + "a16_moe_gemm")


@pytest.mark.parametrize("src_div", [2, 1])
@pytest.mark.parametrize("mtile", MTILES)
@pytest.mark.parametrize("fmt", FMTS)
def test_exact_mapping_and_untouched_rows(fmt, mtile, src_div):
    """One-hot activations leave one non-zero product per output, so a
    written row is one column of ITS expert's bf16 dequantized weight, bit for
    bit. Lists of 0, 17 and 130 rows: empty, partial tile, a last slab of 2
    rows at both tile heights. K = 384: three stages; N = 192: a wave past N.
    The pairs of the non-local expert 0 keep the sentinel."""
    assert ops.native_available()
    E, k, base, T, N, K = 3, 2, 1, 130, 192, 384
    ids = torch.empty(T, k, dtype=torch.int32)
    for t in range(T):
        other = 2 if t < 17 else 0
        ids[t] = torch.tensor([3, other] if t % 2 else [other, 3])
    counts, pairs = ref.moe_route(ids, base, E)
    assert counts.tolist() == [0, 17, 130]
    weight, wd = _experts(fmt, E, N, K)
    assert not torch.equal(wd[1], wd[2])

    rows_a = T * k // src_div
    cols = (7 * torch.arange(rows_a) + 1) % K
    a = torch.zeros(rows_a, K, dtype=torch.bfloat16)
    a[torch.arange(rows_a), cols] = 1.0
    out = torch.full((T * k, N), -3.0, dtype=torch.bfloat16, device=DEV)
    got = _gemm(fmt)(a.to(DEV), weight, counts.to(DEV), pairs.to(DEV),
                     src_div, T, out=out, mtile=mtile)
    assert got is out
    out = out.cpu()
    for p, gid in enumerate(ids.reshape(-1).tolist()):
        if gid < base:
            assert (out[p] == -3.0).all(), p
        else:
            assert torch.equal(out[p], wd[gid - base][:, cols[p // src_div]]), p


@pytest.mark.parametrize("mtile", MTILES)
@pytest.mark.parametrize("T,N,K", [(70, 192, 384), (300, 256, 1024)])
@pytest.mark.parametrize("fmt", FMTS)
def test_numerics_against_float64(fmt, T, N, K, mtile):
    """|out - y| <= 2^-8 |y| + K 2^-23 (|a| @ |Wd|^T) against the float64
    product with the bf16 dequantized weights: bf16 products are exact in
    f32, K additions err by at most 2^-24 of the running magnitude each, the
    final rounding to bf16 by 2^-9 relative; a factor two of slack on each."""
    assert ops.native_available()
    E, k = 4, 2
    weight, wd = _experts(fmt, E, N, K)
    g = torch.Generator().manual_seed(31 + T)
    ids = torch.rand(T, E, generator=g).topk(k, dim=-1).indices.to(
        torch.int32)
    counts, pairs = ref.moe_route(ids, 0, E)
    flat, p = ids.reshape(-1).long(), torch.arange(T * k)
    for src_div in (k, 1):
        a = (torch.randn(T * k // src_div, K, generator=g) * 0.5).to(
            torch.bfloat16)
        out = _gemm(fmt)(a.to(DEV), weight, counts.to(DEV), pairs.to(DEV),
                         src_div, T, mtile=mtile)
        assert out.shape == (T * k, N) and out.dtype == torch.bfloat16
        ad = a.double()[p // src_div]
        y = torch.einsum("pk,enk->epn", ad, wd.double())[flat, p]
        tol = 2.0 ** -8 * y.abs() + K * 2.0 ** -23 * torch.einsum(
            "pk,enk->epn", ad.abs(), wd.double().abs())[flat, p]
        err = (out.double().cpu() - y).abs()
        print(f"{fmt} {(T, N, K)} mtile={mtile} src_div={src_div}: "
              f"max err/tol = {(err / tol).max().item():.3f}")
        assert (err <= tol).all()


def _block(fmt):
    """(quantized tiny-moe-gpu block, its streaming op and MIN_ROWS attribute,
    its f32 dequantized experts [E, in, out] on the GPU)."""
    torch.manual_seed(11)
    blk = MoEMLP(PRESET_CONFIGS["tiny-moe-gpu"]).to(DEV)
    blk.gate.data.normal_(0, 0.5)
    blk.w13.data.normal_(0, 0.05)
    blk.w2.data.normal_(0, 0.05)
    getattr(blk, "quantize_" + fmt)("test")
    f32 = {}
    for which in ("w13", "w2"):
        w = [t.cpu() for t in {"w4": blk.w4_packed, "w8": blk.w8_weight,
                               "mx4": blk.mx4_weight}[fmt](which)]
        deq = {"w4": lambda *p: ref.w4_dequant(*ref.w4_unpack(p)),
               "w8": ref.w8_dequant, "mx4": ref.mx4_dequant}[fmt]
        f32[which] = torch.stack([deq(*(t[e] for t in w)).t()
                                  for e in range(w[0].shape[0])]).to(DEV)
    return blk, f32


@pytest.mark.parametrize("fmt", FMTS)
def test_block_routes_above_dense_tokens_only(fmt):
    """T = 300: the block runs the new op (the counter advances; the rule's
    attribute is set on the instance where the measured rule does not route a
    list this short) and meets the rule of the format's own block test: its
    error against the f32 block is at most twice that of the bf16 block on
    the same dequantized weights. T = DENSE_TOKENS: the counter stays and the
    output is that of the streaming op."""
    assert ops.native_available()
    blk, f32 = _block(fmt)
    attr = fmt.upper() + "A16_MOE_MIN_ROWS"
    T = 300
    if getattr(blk, attr) is None or getattr(blk, attr) > T // 2:
        setattr(blk, attr, 128)
    bf16 = MoEMLP(PRESET_CONFIGS["tiny-moe-gpu"]).to(DEV)
    bf16.gate.data.copy_(blk.gate.data)
    bf16.w13.data.copy_(f32["w13"])
    bf16.w2.data.copy_(f32["w2"])
    torch.manual_seed(13 + T)
    x = torch.randn(T, blk.hidden, dtype=torch.bfloat16, device=DEV)
    with torch.no_grad():
        got = blk(x).float()
        assert blk.routed_wqa16_calls == 1
        plain = bf16(x).float()
        weights, sel = ops.moe_topk(F.linear(x, blk.gate).float(), blk.top_k,
                                    blk.norm_topk)
        expect = torch.zeros(T, blk.hidden, device=DEV)
        for j in range(blk.top_k):
            e = sel[:, j].long()
            g, u = torch.einsum("th,thn->tn", x.float(),
                                f32["w13"][e]).chunk(2, dim=-1)
            expect += weights[:, j, None] * torch.einsum(
                "ti,tih->th", F.silu(g) * u, f32["w2"][e])
        err = ((got - expect).norm() / expect.norm()).item()
        err_bf16 = ((plain - expect).norm() / expect.norm()).item()
        print(f"{fmt} T={T}: relative error {err:.3e}, bf16 {err_bf16:.3e}")
        assert torch.isfinite(got).all() and err <= 2 * err_bf16

        xd = x[:blk.DENSE_TOKENS]
        stream = getattr(ops, fmt + "_moe_gemm")
        w = {"w4": blk.w4_packed, "w8": blk.w8_weight,
             "mx4": blk.mx4_weight}[fmt]
        assert torch.equal(blk(xd), blk._forward_routed(xd, stream, w("w13"),
                                                        w("w2")))
        assert blk.routed_wqa16_calls == 1


def test_engine_int4_experts_long_prompt_graph_equals_eager(monkeypatch):
    """A 300-token prompt prefills the int4 experts through the new kernel
    (about 150 rows per expert; the rule is lowered to that where the
    measured one asks for more); greedy outputs agree across fresh engines
    and between captured and eager decode."""
    assert ops.native_available()
    if (MoEMLP.W4A16_MOE_MIN_ROWS or 10 ** 9) > 128:
        monkeypatch.setattr(MoEMLP, "W4A16_MOE_MIN_ROWS", 128)
    prompts = [[(5 * i) % 2000 + 1 for i in range(300)],
               [1, 5, 9, 20, 7, 3], [2, 4, 6], [11, 12, 13, 14]]
    sp = SamplingParams(max_tokens=8, ignore_eos=True)
    outs = []
    for eager in (False, True, False):
        e = LLMEngine(EngineConfig(
            device="cuda", kv_cache_blocks=512, max_model_len=1024, seed=5,
            preset="tiny-moe-gpu", quantization="int4", quantize_experts=True,
            enforce_eager=eager))
        outs.append(e.generate(prompts, sp))
        moe = e.runner.model.layers[0].mlp
        assert moe.w4 and moe.routed_wqa16_calls >= 1
        del e
    assert all(len(o) == 8 for o in outs[0])
    assert outs[0] == outs[1] == outs[2]
