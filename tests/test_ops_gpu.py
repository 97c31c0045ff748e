"""Numerics tests: every gfx950 HIP kernel vs the plain-PyTorch fp32 reference
(arks_amd/ops/ref.py). All tests here need the GPU."""

import math

import pytest
import torch

import arks_amd.ops as ops
from arks_amd.config import EngineConfig
from arks_amd.engine import LLMEngine, SamplingParams
from arks_amd.ops import ref

pytestmark = pytest.mark.gpu

DEV = "cuda"


def assert_native():
    assert ops.native_available(), "HIP extension must be built on a GPU box"


@pytest.mark.parametrize("rows,hidden", [(7, 128), (64, 3584), (3, 8192)])
def test_rmsnorm(rows, hidden):
    assert_native()
    torch.manual_seed(0)
    x = torch.randn(rows, hidden, dtype=torch.bfloat16, device=DEV)
    w = torch.randn(hidden, dtype=torch.bfloat16, device=DEV)
    out = ops.rmsnorm(x, w, 1e-6)
    expect = ref.rmsnorm(x.float().cpu(), w.float().cpu(), 1e-6)
    torch.testing.assert_close(out.float().cpu(), expect, atol=2e-2, rtol=2e-2)


@pytest.mark.parametrize("rows,hidden", [(64, 3584), (5, 256)])
def test_fused_add_rmsnorm(rows, hidden):
    assert_native()
    torch.manual_seed(1)
    x = torch.randn(rows, hidden, dtype=torch.bfloat16, device=DEV)
    res = torch.randn(rows, hidden, dtype=torch.bfloat16, device=DEV)
    w = torch.randn(hidden, dtype=torch.bfloat16, device=DEV)
    res_cpu = res.float().cpu().clone()
    out, new_res = ops.fused_add_rmsnorm(x, res, w, 1e-6)
    expect_out, expect_res = ref.fused_add_rmsnorm(
        x.float().cpu(), res_cpu, w.float().cpu(), 1e-6
    )
    torch.testing.assert_close(new_res.float().cpu(), expect_res, atol=2e-2, rtol=2e-2)
    torch.testing.assert_close(out.float().cpu(), expect_out, atol=3e-2, rtol=3e-2)


def test_silu_mul():
    assert_native()
    torch.manual_seed(2)
    x = torch.randn(33, 2 * 1024, dtype=torch.bfloat16, device=DEV)
    out = ops.silu_mul(x)
    expect = ref.silu_mul(x.float().cpu())
    torch.testing.assert_close(out.float().cpu(), expect, atol=2e-2, rtol=2e-2)


@pytest.mark.parametrize("hq,hkv,hd", [(8, 2, 128), (4, 4, 64)])
def test_rope(hq, hkv, hd):
    assert_native()
    torch.manual_seed(3)
    T = 50
    pos = torch.randint(0, 2000, (T,), dtype=torch.int64, device=DEV)
    q = torch.randn(T, hq * hd, dtype=torch.bfloat16, device=DEV)
    k = torch.randn(T, hkv * hd, dtype=torch.bfloat16, device=DEV)
    cs = ref.rope_cos_sin_cache(hd, 2048, 10000.0, device=DEV)
    q_ref, k_ref = ref.rope_apply(
        pos.cpu(), q.float().cpu(), k.float().cpu(), cs.cpu(), hd
    )
    q2, k2 = ops.rope_apply_inplace(pos, q, k, cs, hd)
    torch.testing.assert_close(q2.float().cpu(), q_ref, atol=2e-2, rtol=2e-2)
    torch.testing.assert_close(k2.float().cpu(), k_ref, atol=2e-2, rtol=2e-2)


def test_reshape_and_cache():
    assert_native()
    torch.manual_seed(4)
    T, hkv, hd, nb, bs = 37, 4, 128, 16, 16
    k = torch.randn(T, hkv, hd, dtype=torch.bfloat16, device=DEV)
    v = torch.randn(T, hkv, hd, dtype=torch.bfloat16, device=DEV)
    kc = torch.zeros(nb, hkv, bs, hd, dtype=torch.bfloat16, device=DEV)
    vc = torch.zeros_like(kc)
    slots = torch.randperm(nb * bs, device=DEV)[:T].to(torch.int64)
    kc_ref, vc_ref = kc.cpu().clone(), vc.cpu().clone()
    ref.reshape_and_cache(k.cpu(), v.cpu(), kc_ref, vc_ref, slots.cpu())
    ops.reshape_and_cache(k, v, kc, vc, slots)
    torch.testing.assert_close(kc.cpu(), kc_ref)
    torch.testing.assert_close(vc.cpu(), vc_ref)

    # a padding row (slot -1 writes nothing anywhere), bf16 and fp8 caches
    T, hkv, hd, nb = 5, 2, 64, 4
    k = torch.randn(T, hkv, hd, dtype=torch.bfloat16, device=DEV)
    v = torch.randn(T, hkv, hd, dtype=torch.bfloat16, device=DEV)
    slots = torch.tensor([17, 3, -1, 63, 32], dtype=torch.int64, device=DEV)
    keep = (slots >= 0).cpu()
    kc_ref = torch.zeros(nb, hkv, bs, hd, dtype=torch.float32)
    vc_ref = torch.zeros_like(kc_ref)
    ref.reshape_and_cache(k.float().cpu()[keep], v.float().cpu()[keep],
                          kc_ref, vc_ref, slots.cpu()[keep])
    assert kc_ref.count_nonzero() >= 4 * hkv * hd - 8
    for dt in (torch.bfloat16, torch.float8_e4m3fn):
        kc = torch.zeros(nb, hkv, bs, hd, dtype=dt, device=DEV)
        vc = torch.zeros_like(kc)
        ops.reshape_and_cache(k, v, kc, vc, slots)
        for got, want in ((kc, kc_ref), (vc, vc_ref)):
            err = (got.float().cpu() - want).abs()
            if dt == torch.bfloat16:
                assert err.max() == 0  # a copy
            else:
                # correctly rounded to e4m3 whichever way ties go: within
                # half an ulp, 2^(e-3) for |x| in [2^e, 2^(e+1)), e >= -6
                # (subnormals below); untouched bytes (want == 0) stay 0
                e = torch.frexp(want)[1] - 1
                half_ulp = 0.5 * torch.exp2((e.clamp(min=-6) - 3).float())
                assert (err <= half_ulp * (want != 0)).all()


def test_mfma_probe():
    """Verify the MFMA fragment-layout hypothesis vs torch.matmul.
    Asymmetric operands so a transpose cannot pass (guide §3)."""
    assert_native()
    torch.manual_seed(5)
    a = torch.randn(16, 32, dtype=torch.bfloat16, device=DEV)
    b = torch.randn(32, 16, dtype=torch.bfloat16, device=DEV)
    d = torch.zeros(16, 16, dtype=torch.float32, device=DEV)
    from arks_amd.ops import _load

    _load.C.mfma_probe(d, a, b)
    expect = a.float() @ b.float()
    torch.testing.assert_close(d.cpu(), expect.cpu(), atol=2e-2, rtol=2e-2)


@pytest.mark.parametrize(
    "hq,hkv,hd,seq_lens",
    [
        (28, 4, 128, [1, 16, 33, 256]),
        (8, 8, 128, [64, 127]),
        (8, 1, 128, [300]),
        (4, 2, 64, [17, 90]),
    ],
)
def test_attention_decode_paged(hq, hkv, hd, seq_lens):
    assert_native()
    torch.manual_seed(6)
    bs = 16
    S = len(seq_lens)
    max_blocks = (max(seq_lens) + bs - 1) // bs
    total_blocks = sum((n + bs - 1) // bs for n in seq_lens) + 2
    q = torch.randn(S, hq, hd, dtype=torch.bfloat16, device=DEV)
    kc = torch.randn(total_blocks, hkv, bs, hd, dtype=torch.bfloat16, device=DEV)
    vc = torch.randn_like(kc)
    # assign blocks sequentially
    bt = torch.zeros(S, max_blocks, dtype=torch.int32, device=DEV)
    nxt = 0
    for i, n in enumerate(seq_lens):
        nb = (n + bs - 1) // bs
        bt[i, :nb] = torch.arange(nxt, nxt + nb, dtype=torch.int32)
        nxt += nb
    sl = torch.tensor(seq_lens, dtype=torch.int32, device=DEV)
    scale = 1.0 / math.sqrt(hd)
    out = ops.attention_decode_paged(q, kc, vc, bt, sl, scale)
    expect = ref.attention_decode_paged(
        q.float().cpu(), kc.float().cpu(), vc.float().cpu(), bt.cpu(), sl.cpu(), scale
    )
    torch.testing.assert_close(out.float().cpu(), expect, atol=2e-2, rtol=2e-2)


@pytest.mark.parametrize(
    "hq,hkv,hd,seq_lens",
    [
        (28, 4, 128, [1, 5, 64, 200]),
        (8, 8, 128, [129]),
        (4, 1, 128, [64, 64]),
        (4, 2, 64, [100, 33]),
    ],
)
def test_attention_prefill_varlen(hq, hkv, hd, seq_lens):
    assert_native()
    torch.manual_seed(7)
    T = sum(seq_lens)
    q = torch.randn(T, hq, hd, dtype=torch.bfloat16, device=DEV)
    k = torch.randn(T, hkv, hd, dtype=torch.bfloat16, device=DEV)
    v = torch.randn(T, hkv, hd, dtype=torch.bfloat16, device=DEV)
    cu = torch.tensor(
        [0] + list(torch.tensor(seq_lens).cumsum(0)), dtype=torch.int32, device=DEV
    )
    scale = 1.0 / math.sqrt(hd)
    out = ops.attention_prefill_varlen(q, k, v, cu, seq_lens, scale)
    expect = ref.attention_prefill_varlen(
        q.float().cpu(), k.float().cpu(), v.float().cpu(), cu.cpu(), scale
    )
    torch.testing.assert_close(out.float().cpu(), expect, atol=3e-2, rtol=3e-2)


def test_attention_decode_partitions_agree():
    """Flash-decode split (nparts>1) must match the single-partition path."""
    assert_native()
    torch.manual_seed(11)
    hq, hkv, hd, bs = 8, 2, 128, 16
    seq_lens = [700, 123, 48]
    S = len(seq_lens)
    max_blocks = (max(seq_lens) + bs - 1) // bs
    total = sum((n + bs - 1) // bs for n in seq_lens)
    q = torch.randn(S, hq, hd, dtype=torch.bfloat16, device=DEV)
    kc = torch.randn(total, hkv, bs, hd, dtype=torch.bfloat16, device=DEV)
    vc = torch.randn_like(kc)
    bt = torch.zeros(S, max_blocks, dtype=torch.int32, device=DEV)
    nxt = 0
    for i, n in enumerate(seq_lens):
        nb = (n + bs - 1) // bs
        bt[i, :nb] = torch.arange(nxt, nxt + nb, dtype=torch.int32)
        nxt += nb
    sl = torch.tensor(seq_lens, dtype=torch.int32, device=DEV)
    scale = 1.0 / math.sqrt(hd)
    o1 = ops.attention_decode_paged(q, kc, vc, bt, sl, scale, num_partitions=1)
    o8 = ops.attention_decode_paged(q, kc, vc, bt, sl, scale, num_partitions=8)
    torch.testing.assert_close(o1.float(), o8.float(), atol=2e-2, rtol=2e-2)
    expect = ref.attention_decode_paged(
        q.float().cpu(), kc.float().cpu(), vc.float().cpu(), bt.cpu(), sl.cpu(), scale
    )
    torch.testing.assert_close(o8.float().cpu(), expect, atol=2e-2, rtol=2e-2)


def test_strided_qkv_views():
    """RoPE/cache/attention on strided views into a fused QKV buffer must
    match the contiguous path (the engine's no-copy hot path)."""
    assert_native()
    torch.manual_seed(12)
    hq, hkv, hd = 8, 2, 128
    T = 40
    qkv = torch.randn(T, (hq + 2 * hkv) * hd, dtype=torch.bfloat16, device=DEV)
    q = qkv[:, : hq * hd]
    k = qkv[:, hq * hd : (hq + hkv) * hd]
    v = qkv[:, (hq + hkv) * hd :]
    q_c, k_c, v_c = q.contiguous(), k.contiguous(), v.contiguous()
    pos = torch.randint(0, 1000, (T,), dtype=torch.int64, device=DEV)
    cs = ref.rope_cos_sin_cache(hd, 2048, 10000.0, device=DEV)
    ops.rope_apply_inplace(pos, q, k, cs, hd)  # strided in-place
    q2, k2 = ops.rope_apply_inplace(pos, q_c, k_c, cs, hd)
    torch.testing.assert_close(q.contiguous(), q2)
    torch.testing.assert_close(k.contiguous(), k2)

    # strided cache write
    nb = 4
    kc1 = torch.zeros(nb, hkv, 16, hd, dtype=torch.bfloat16, device=DEV)
    vc1 = torch.zeros_like(kc1)
    kc2, vc2 = kc1.clone(), vc1.clone()
    slots = torch.randperm(nb * 16, device=DEV)[:T].to(torch.int64)
    ops.reshape_and_cache(k.unflatten(-1, (hkv, hd)), v.unflatten(-1, (hkv, hd)),
                          kc1, vc1, slots)
    ops.reshape_and_cache(k2.view(T, hkv, hd), v_c.view(T, hkv, hd), kc2, vc2, slots)
    torch.testing.assert_close(kc1, kc2)
    torch.testing.assert_close(vc1, vc2)

    # strided prefill q/k/v
    cu = torch.tensor([0, T], dtype=torch.int32, device=DEV)
    scale = 1.0 / math.sqrt(hd)
    o_str = ops.attention_prefill_varlen(
        q.unflatten(-1, (hq, hd)), k.unflatten(-1, (hkv, hd)),
        v.unflatten(-1, (hkv, hd)), cu, [T], scale,
    )
    o_c = ops.attention_prefill_varlen(
        q.contiguous().view(T, hq, hd), k.contiguous().view(T, hkv, hd),
        v.contiguous().view(T, hkv, hd), cu, [T], scale,
    )
    torch.testing.assert_close(o_str, o_c)


def test_greedy_sample():
    assert_native()
    torch.manual_seed(8)
    logits = torch.randn(9, 32000, dtype=torch.bfloat16, device=DEV)
    out = ops.greedy_sample(logits)
    expect = logits.float().argmax(dim=-1).cpu()
    torch.testing.assert_close(out.cpu(), expect)


def test_gumbel_sample_greedy_rows():
    """Rows with temperature 0 must match argmax exactly."""
    assert_native()
    torch.manual_seed(9)
    logits = torch.randn(8, 5000, dtype=torch.bfloat16, device=DEV)
    temps = torch.zeros(8, dtype=torch.float32, device=DEV)
    u = torch.rand(8, 5000, dtype=torch.float32, device=DEV)
    out = ops.sample_tokens(logits, temps, u)
    expect = logits.float().argmax(dim=-1).cpu()
    torch.testing.assert_close(out.cpu(), expect)


def test_gumbel_sample_distribution():
    """Sampling a 4-token vocab many times approximates the softmax dist."""
    assert_native()
    torch.manual_seed(10)
    N = 20000
    logits = torch.tensor([[2.0, 1.0, 0.0, -1.0]], dtype=torch.bfloat16, device=DEV)
    logits = logits.expand(N, 4).contiguous()
    temps = torch.ones(N, dtype=torch.float32, device=DEV)
    u = torch.rand(N, 4, dtype=torch.float32, device=DEV)
    out = ops.sample_tokens(logits, temps, u)
    counts = torch.bincount(out, minlength=4).float() / N
    expect = torch.softmax(torch.tensor([2.0, 1.0, 0.0, -1.0]), dim=0)
    assert (counts.cpu() - expect).abs().max() < 0.02


@pytest.mark.parametrize(
    "hq,hkv,hd,spec",
    [
        # (kv_len, q_len) per seq; q_len < kv_len = cached prefix
        (8, 2, 128, [(80, 80), (45, 13), (200, 1)]),
        (28, 4, 128, [(512, 128), (100, 100)]),
        (4, 4, 64, [(33, 17), (16, 1), (64, 64)]),
    ],
)
def test_attention_extend_paged(hq, hkv, hd, spec):
    """Extend kernel (paged KV, cached prefixes) vs torch fp32 reference."""
    assert_native()
    torch.manual_seed(13)
    bs = 16
    kv_lens = [s[0] for s in spec]
    q_lens = [s[1] for s in spec]
    S = len(spec)
    Tq = sum(q_lens)
    nb = [(n + bs - 1) // bs for n in kv_lens]
    total_blocks = sum(nb) + 3
    q = torch.randn(Tq, hq, hd, dtype=torch.bfloat16, device=DEV)
    kc = torch.randn(total_blocks, hkv, bs, hd, dtype=torch.bfloat16, device=DEV)
    vc = torch.randn_like(kc)
    bt = torch.zeros(S, max(nb), dtype=torch.int32, device=DEV)
    # scrambled non-contiguous block ids
    perm = torch.randperm(total_blocks - 1) + 1
    idx = 0
    for i in range(S):
        for j in range(nb[i]):
            bt[i, j] = perm[idx]
            idx += 1
    cu_q = torch.tensor([0] + list(torch.tensor(q_lens).cumsum(0)),
                        dtype=torch.int32, device=DEV)
    kvl = torch.tensor(kv_lens, dtype=torch.int32, device=DEV)
    scale = 1.0 / math.sqrt(hd)
    out = ops.attention_extend_paged(q, kc, vc, bt, kvl, cu_q, q_lens, scale)
    expect = ref.attention_extend_paged(
        q.float().cpu(), kc.float().cpu(), vc.float().cpu(), bt.cpu(),
        kvl.cpu(), cu_q.cpu(), scale,
    )
    torch.testing.assert_close(out.float().cpu(), expect, atol=3e-2, rtol=3e-2)


def test_quant_fp8_rows_matches_torch_cast():
    """HW cvt (quant_fp8_rows kernel) vs torch's fp32->e4m3 cast."""
    assert_native()
    torch.manual_seed(17)
    x = torch.randn(33, 3584, dtype=torch.bfloat16, device=DEV) * 4
    q, inv_s = ops.quant_fp8_rows(x)
    qr, inv_sr = ref.quant_fp8_rows(x.cpu())
    torch.testing.assert_close(inv_s.cpu(), inv_sr.float(), atol=1e-6, rtol=1e-5)
    # bytes should agree except possibly ties at rounding boundaries
    # HW cvt vs torch cast may resolve rounding ties differently; require
    # byte agreement on ~all values and dequant closeness everywhere
    same = (q.cpu().view(torch.uint8) == qr.view(torch.uint8)).float().mean()
    assert same > 0.995, same.item()
    # and the differing bytes must still dequantize within one e4m3 ulp
    dq = q.cpu().float() * inv_s.cpu()[:, None]
    rel = (dq - x.cpu().float()).abs() / x.cpu().float().abs().clamp(min=1e-3)
    assert rel.max() < 0.13, rel.max().item()


def test_engine_fp8_gpu():
    """fp8 engine produces plausible deterministic output via _scaled_mm."""
    e1 = LLMEngine(EngineConfig(
        preset="tiny-gpu", device="cuda", kv_cache_blocks=256,
        max_model_len=512, quantization="fp8", seed=4,
    ))
    prompts = [[5, 2, 8] * 5, [1, 9, 9, 3]]
    sp = SamplingParams(max_tokens=6, ignore_eos=True)
    out1 = e1.generate(prompts, sp)
    out2 = e1.generate(prompts, sp)  # prefix-cache hit path + fp8
    assert out1 == out2 and all(len(o) == 6 for o in out1)


@pytest.mark.parametrize("m,k,n", [
    (1, 3584, 4608), (5, 96, 64), (17, 3584, 3584), (64, 18944, 3584),
    (37, 18944, 3584), (64, 3584, 37888), (33, 3584, 152064), (64, 128, 64),
])
def test_skinny_gemm(m, k, n):
    """Streaming decode GEMM vs hipBLASLt, both split and direct paths."""
    assert_native()
    torch.manual_seed(19)
    a = torch.randn(m, k, dtype=torch.bfloat16, device=DEV) * 0.5
    w = torch.randn(n, k, dtype=torch.bfloat16, device=DEV) * 0.05
    bias = torch.randn(n, dtype=torch.bfloat16, device=DEV)
    ref_out = torch.nn.functional.linear(a, w, bias).float()
    out = ops.skinny_gemm(a, w, bias).float()
    torch.testing.assert_close(out, ref_out, atol=5e-2, rtol=5e-2)
    # no-bias path
    out2 = ops.skinny_gemm(a, w).float()
    torch.testing.assert_close(
        out2, torch.nn.functional.linear(a, w).float(), atol=5e-2, rtol=5e-2
    )


def test_skinny_gemm_strided_input():
    """Row-strided activations (views into a fused buffer)."""
    assert_native()
    torch.manual_seed(23)
    buf = torch.randn(16, 512, dtype=torch.bfloat16, device=DEV)
    a = buf[:, 128:128 + 256]  # stride(0)=512
    w = torch.randn(128, 256, dtype=torch.bfloat16, device=DEV) * 0.1
    out = ops.skinny_gemm(a, w).float()
    torch.testing.assert_close(
        out, torch.nn.functional.linear(a, w).float(), atol=5e-2, rtol=5e-2
    )


def test_mfma_probe_32x32():
    """Verify the 32x32x16 bf16 MFMA fragment layout hypothesis on HW."""
    assert_native()
    torch.manual_seed(3)
    a = torch.randn(32, 16, dtype=torch.bfloat16, device=DEV)
    b = torch.randn(16, 32, dtype=torch.bfloat16, device=DEV)
    d = torch.zeros(32, 32, dtype=torch.float32, device=DEV)
    from arks_amd.ops import _native
    _native().mfma_probe32(d, a, b)
    ref_out = a.float() @ b.float()
    torch.testing.assert_close(d.cpu(), ref_out.cpu(), atol=2e-2, rtol=2e-2)


def test_rmsnorm_fp8_fused_matches_composed():
    assert_native()
    torch.manual_seed(31)
    x = torch.randn(17, 3584, dtype=torch.bfloat16, device=DEV)
    res = torch.randn_like(x)
    w = torch.randn(3584, dtype=torch.bfloat16, device=DEV)
    # no-residual variant
    q, s = ops.rmsnorm_fp8(x, w, 1e-6)
    y = ops.rmsnorm(x, w, 1e-6)
    qr, sr = ops.quant_fp8_rows(y)
    # fused quantizes the f32 normalized values; composed goes through a
    # bf16 round first -> scales/values differ by ~1 bf16 ulp
    torch.testing.assert_close(s, sr, atol=1e-4, rtol=1e-2)
    dq = q.float() * s[:, None]
    dqr = qr.float() * sr[:, None]
    torch.testing.assert_close(dq, dqr, atol=0.1, rtol=0.15)
    # fused-add variant mutates residual identically
    res2 = res.clone()
    q2, s2, r2 = ops.fused_add_rmsnorm_fp8(x, res, w, 1e-6)
    y2, r2b = ops.fused_add_rmsnorm(x, res2, w, 1e-6)
    torch.testing.assert_close(r2, r2b)
    dq2 = q2.float() * s2[:, None]
    torch.testing.assert_close(dq2, y2.float(), atol=0.1, rtol=0.15)


def test_silu_mul_fp8_fused_matches_composed():
    assert_native()
    torch.manual_seed(37)
    gu = torch.randn(9, 2 * 18944, dtype=torch.bfloat16, device=DEV)
    q, s = ops.silu_mul_fp8(gu)
    y = ops.silu_mul(gu)
    dq = q.float() * s[:, None]
    torch.testing.assert_close(dq, y.float(), atol=0.08, rtol=0.12)


def _mk_paged(spec, hq, hkv, hd, seed=13):
    """Build scrambled paged KV fixtures: (q, kc, vc, bt, kvl, cu_q, q_lens)."""
    torch.manual_seed(seed)
    bs = 16
    kv_lens = [s[0] for s in spec]
    q_lens = [s[1] for s in spec]
    S = len(spec)
    Tq = sum(q_lens)
    nb = [(n + bs - 1) // bs for n in kv_lens]
    total_blocks = sum(nb) + 3
    q = torch.randn(Tq, hq, hd, dtype=torch.bfloat16, device=DEV)
    kc = torch.randn(total_blocks, hkv, bs, hd, dtype=torch.bfloat16, device=DEV)
    vc = torch.randn_like(kc)
    bt = torch.zeros(S, max(nb), dtype=torch.int32, device=DEV)
    perm = torch.randperm(total_blocks - 1) + 1
    idx = 0
    for i in range(S):
        for j in range(nb[i]):
            bt[i, j] = perm[idx]
            idx += 1
    cu_q = torch.tensor([0] + list(torch.tensor(q_lens).cumsum(0)),
                        dtype=torch.int32, device=DEV)
    kvl = torch.tensor(kv_lens, dtype=torch.int32, device=DEV)
    return q, kc, vc, bt, kvl, cu_q, q_lens


@pytest.mark.parametrize(
    "hq,hkv,hd,spec",
    [
        # big q tiles: the 8-wave 32x32 ladder kernel (attn_extend2)
        (28, 4, 128, [(1024, 1024)]),
        (8, 2, 128, [(700, 300), (257, 257), (1030, 97)]),
        (4, 4, 64, [(600, 600), (300, 129)]),
        # mixed routing: one seq per kernel in the same call
        (8, 2, 128, [(512, 512), (40, 13)]),
        # deep KV behind a short chunk: the split+combine path (one
        # 256-row tile over 8k keys forces kv-partitioning)
        (28, 4, 128, [(8192, 256)]),
        (8, 2, 64, [(4096, 200), (4096, 256)]),
    ],
)
def test_attention_extend2_big_tiles(hq, hkv, hd, spec):
    """The 256-row ladder extend kernel vs the torch fp32 reference,
    including q lengths that straddle tile boundaries and calls that mix
    both kernels."""
    assert_native()
    q, kc, vc, bt, kvl, cu_q, q_lens = _mk_paged(spec, hq, hkv, hd)
    scale = 1.0 / math.sqrt(hd)
    out = ops.attention_extend_paged(q, kc, vc, bt, kvl, cu_q, q_lens, scale)
    expect = ref.attention_extend_paged(
        q.float().cpu(), kc.float().cpu(), vc.float().cpu(), bt.cpu(),
        kvl.cpu(), cu_q.cpu(), scale,
    )
    torch.testing.assert_close(out.float().cpu(), expect, atol=3e-2, rtol=3e-2)


@pytest.mark.parametrize(
    "hq,hkv,hd,spec,window",
    [
        (8, 2, 128, [(900, 800)], 128),     # ladder kernel, window binds
        (8, 2, 128, [(900, 80), (64, 64)], 100),  # 64-row kernel
        (4, 4, 64, [(512, 512)], 64),
        (28, 4, 128, [(1024, 512)], 4096),  # window larger than kv: no-op
    ],
)
def test_attention_extend_sliding_window(hq, hkv, hd, spec, window):
    """Sliding-window masking in both extend kernels vs the reference."""
    assert_native()
    q, kc, vc, bt, kvl, cu_q, q_lens = _mk_paged(spec, hq, hkv, hd, seed=7)
    scale = 1.0 / math.sqrt(hd)
    out = ops.attention_extend_paged(
        q, kc, vc, bt, kvl, cu_q, q_lens, scale, window=window
    )
    expect = ref.attention_extend_paged(
        q.float().cpu(), kc.float().cpu(), vc.float().cpu(), bt.cpu(),
        kvl.cpu(), cu_q.cpu(), scale, window=window,
    )
    torch.testing.assert_close(out.float().cpu(), expect, atol=3e-2, rtol=3e-2)


@pytest.mark.parametrize("drop_pages", [False, True])
def test_attention_decode_sliding_window(drop_pages):
    """Decode kernel with a sliding window; out-of-window pages may be
    dropped from the block table (-1) without changing the output."""
    assert_native()
    hq, hkv, hd = 8, 2, 128
    window = 96
    spec = [(400, 1), (97, 1), (64, 1)]
    torch.manual_seed(11)
    bs = 16
    kv_lens = [s[0] for s in spec]
    S = len(spec)
    nb = [(n + bs - 1) // bs for n in kv_lens]
    total_blocks = sum(nb) + 3
    q = torch.randn(S, hq, hd, dtype=torch.bfloat16, device=DEV)
    kc = torch.randn(total_blocks, hkv, bs, hd, dtype=torch.bfloat16, device=DEV)
    vc = torch.randn_like(kc)
    bt = torch.zeros(S, max(nb), dtype=torch.int32, device=DEV)
    perm = torch.randperm(total_blocks - 1) + 1
    idx = 0
    for i in range(S):
        for j in range(nb[i]):
            bt[i, j] = perm[idx]
            idx += 1
    sl = torch.tensor(kv_lens, dtype=torch.int32, device=DEV)
    scale = 1.0 / math.sqrt(hd)
    expect = ref.attention_decode_paged(
        q.float().cpu(), kc.float().cpu(), vc.float().cpu(), bt.cpu(),
        sl.cpu(), scale, window=window,
    )
    if drop_pages:
        # drop pages wholly below the window (allocator page-dropping)
        for i, L in enumerate(kv_lens):
            lo = max(0, L - window) // bs
            bt[i, :lo] = -1
    for nparts in (1, 4):
        out = ops.attention_decode_paged(
            q, kc, vc, bt, sl, scale, num_partitions=nparts, window=window
        )
        torch.testing.assert_close(out.float().cpu(), expect,
                                   atol=3e-2, rtol=3e-2)


@pytest.mark.parametrize("E,k,renorm", [(128, 8, True), (8, 2, True),
                                        (60, 4, False), (512, 16, True)])
def test_moe_topk_matches_torch(E, k, renorm):
    """Fused softmax+topk+renorm routing kernel vs the torch chain,
    including tie-free random logits and the id set equality."""
    assert_native()
    torch.manual_seed(5)
    T = 97
    logits = torch.randn(T, E, dtype=torch.float32, device=DEV)
    w, ids = ops.moe_topk(logits, k, renorm)
    wr, idr = ref.moe_topk(logits.cpu(), k, renorm)
    # same expert sets (order may differ only on exact ties — none here)
    assert torch.equal(ids.cpu().long().sort(dim=-1).values,
                       idr.long().sort(dim=-1).values)
    torch.testing.assert_close(
        w.cpu().sort(dim=-1).values, wr.sort(dim=-1).values,
        atol=1e-5, rtol=1e-5)


def test_moe_mix_matches_einsum():
    assert_native()
    torch.manual_seed(6)
    El, T, H, k = 16, 33, 2048, 8
    base = 16  # TP slice: rank 1 of 2
    y = torch.randn(El, T, H, dtype=torch.bfloat16, device=DEV)
    ids = torch.randint(0, 2 * El, (T, k), dtype=torch.int32, device=DEV)
    w = torch.rand(T, k, dtype=torch.float32, device=DEV)
    out = ops.moe_mix(y, w, ids, expert_base=base)
    expect = ref.moe_mix(y.float().cpu(), w.cpu(), ids.cpu(), base)
    torch.testing.assert_close(out.float().cpu(), expect.float(),
                               atol=2e-2, rtol=2e-2)


def test_one_shot_allreduce_single_device():
    """p2p all-reduce data path on one GPU: world=1 is identity; a
    simulated world=2 (two mailbox sets on one device, flags pre-armed so
    the sequential launches never spin) reduces both contributions."""
    assert_native()
    nat = ops._native()
    torch.manual_seed(3)
    n = 8192
    x0 = torch.randn(n, dtype=torch.bfloat16, device=DEV)
    x1 = torch.randn(n, dtype=torch.bfloat16, device=DEV)

    # world = 1: identity (ipc_alloc'd raw buffers, as production uses;
    # mailboxes sized like production: 2 parities x 8 slots x MAX_ELEMS)
    MAILBYTES = 2 * 8 * (1 << 19) * 2
    mail_ptr, mail_h = nat.ipc_alloc(MAILBYTES)
    flag_ptr, _ = nat.ipc_alloc(64 * 8)
    assert len(bytes(mail_h)) == 64
    seq = torch.zeros(1, dtype=torch.int64, device=DEV)
    out = torch.empty_like(x0)
    nat.one_shot_allreduce(out, x0, [mail_ptr], [flag_ptr], seq, 0)
    torch.cuda.synchronize()
    torch.testing.assert_close(out, x0)
    nat.ipc_alloc_free(mail_ptr)
    nat.ipc_alloc_free(flag_ptr)

    # world = 2 simulated on one device; flags pre-armed (0x7f bytes =
    # huge sequence values) so the two sequential launches never spin
    mails, flgs = [], []
    for _ in range(2):
        mp, _h = nat.ipc_alloc(MAILBYTES)
        fp, _h2 = nat.ipc_alloc(2 * 64 * 8)
        mails.append(mp)
        flgs.append(fp)
    seqs = [torch.zeros(1, dtype=torch.int64, device=DEV) for _ in range(2)]
    out0 = torch.empty_like(x0)
    out1 = torch.empty_like(x0)
    nat.arm_flags(flgs[0], 2 * 64)
    nat.arm_flags(flgs[1], 2 * 64)
    nat.one_shot_allreduce(out0, x0, mails, flgs, seqs[0], 0)
    nat.one_shot_allreduce(out1, x1, mails, flgs, seqs[1], 1)
    torch.cuda.synchronize()
    # the SECOND launch sees both mailbox slots populated
    torch.testing.assert_close(out1.float(), (x0.float() + x1.float()),
                               atol=2e-2, rtol=2e-2)
    for p in mails + flgs:
        nat.ipc_alloc_free(p)


@pytest.mark.parametrize("fp8", [False, True])
def test_rope_and_cache_fused_matches_two_step(fp8):
    """Fused RoPE+cache kernel vs the separate rope + reshape_and_cache
    pair, including padded rows (slot -1: rotate but skip the cache). Both
    rotate through rope_rotate and store through cache_store, so the results
    are the same bits. The last case is the Qwen2.5-7B batch-64 decode shape:
    a differently contracted fma shows about once in 1e5 elements, and this
    one rotates 262k."""
    assert_native()
    torch.manual_seed(21)
    bs = 16
    dt = torch.float8_e4m3fn if fp8 else torch.bfloat16
    for T, hq, hkv, hd, max_pos, base in [
        (9, 8, 2, 128, 64, 10000.0),
        (9, 2, 1, 64, 64, 10000.0),
        (64, 28, 4, 128, 2048, 1000000.0),
    ]:
        nblocks = (3 * T + bs - 1) // bs  # slots are i * 3
        qkv = torch.randn(T, (hq + 2 * hkv) * hd, dtype=torch.bfloat16,
                          device=DEV)
        q = qkv[:, : hq * hd]
        k = qkv[:, hq * hd: (hq + hkv) * hd]
        v = qkv[:, (hq + hkv) * hd:]
        q2, k2, v2 = (t.clone().contiguous() for t in (q, k, v))
        cos_sin = ref.rope_cos_sin_cache(hd, max_pos, base).cuda()
        pos = torch.randint(0, max_pos, (T,), dtype=torch.int64, device=DEV)
        slots = torch.tensor([i * 3 if i != 4 else -1 for i in range(T)],
                             dtype=torch.int64, device=DEV)
        kc_a = torch.zeros(nblocks, hkv, bs, hd, dtype=dt, device=DEV)
        vc_a = torch.zeros_like(kc_a)
        kc_b = torch.zeros_like(kc_a)
        vc_b = torch.zeros_like(kc_a)
        # fused
        ops.rope_and_cache(pos, q, k, v, kc_a, vc_a, slots, cos_sin, hd)
        # two-step
        ops.rope_apply_inplace(pos, q2, k2, cos_sin, hd)
        ops.reshape_and_cache(k2.view(T, hkv, hd), v2.view(T, hkv, hd),
                              kc_b, vc_b, slots)
        assert torch.equal(q, q2)
        assert torch.equal(k, k2)
        assert torch.equal(kc_a.view(torch.uint8), kc_b.view(torch.uint8))
        assert torch.equal(vc_a.view(torch.uint8), vc_b.view(torch.uint8))
        assert kc_a.view(torch.uint8).any()
        # slot 12 would have been row 4's: nothing was cached for it
        assert not kc_a.view(torch.uint8)[0, :, 12].any()


@pytest.mark.parametrize("with_bias", [False, True])
def test_skinny_gemm_tall_k_configs_agree(monkeypatch, with_bias):
    """The tall-K kernel and its non-temporal-load twin (launch configs 1 and
    2, ARKS_SKINNY_TALLK_V=7 / 8): the load hint changes no arithmetic, so
    the two results are the same bits."""
    assert_native()
    torch.manual_seed(29)
    m, n, k = 64, 256, 1024
    a = torch.randn(m, k, dtype=torch.bfloat16, device=DEV) * 0.5
    w = torch.randn(n, k, dtype=torch.bfloat16, device=DEV) * 0.05
    bias = (torch.randn(n, dtype=torch.bfloat16, device=DEV)
            if with_bias else None)
    outs = []
    for config in (1, 2):
        monkeypatch.setattr(ops, "_SKINNY_TALLK_CONFIG", config)
        assert ops._skinny_plan(m, n, k) == (config, 4, 256, 64)
        outs.append(ops.skinny_gemm(a, w, bias))
    expect = torch.nn.functional.linear(a, w, bias).float()
    for out in outs:
        torch.testing.assert_close(out.float(), expect, atol=5e-2, rtol=5e-2)
    assert torch.equal(outs[0], outs[1])
