"""Split-K partials consumed by the kernels that follow the skinny GEMM.

The reference in every fused case is the unfused composition of existing
ops (ops.skinny_gemm, then ops.fused_add_rmsnorm or ops.rope_and_cache); the
fused kernels must reproduce it bit for bit, so results are compared with
torch.equal, never a tolerance."""

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


def _split_rule(K, nsplits):
    """k_per_split as ops.skinny_gemm derives it for a wanted split count."""
    kps = -(-(-(-K // nsplits)) // 32) * 32
    assert -(-K // kps) == nsplits, (K, nsplits, kps)
    return kps


@pytest.mark.parametrize("m", [1, 17, 64])
@pytest.mark.parametrize("k,n", [(96, 64), (416, 128), (3584, 192)])
@pytest.mark.parametrize("nsplits", [2, 3])
def test_partials_layout_and_combine(m, k, n, nsplits):
    """Partials-only launch writes [split][m][n]; the combine fallback sums
    them. Covers a K tail shorter than one 128 chunk, an uneven last split
    and M that is no multiple of 16."""
    assert_native()
    nat = ops._native()
    torch.manual_seed(31)
    a = torch.randn(m, k, dtype=torch.bfloat16, device=DEV) * 0.5
    w = torch.randn(n, k, dtype=torch.bfloat16, device=DEV) * 0.05
    bias = torch.randn(n, dtype=torch.bfloat16, device=DEV)
    kps = _split_rule(k, nsplits)
    mrows = ((m + 15) // 16) * 16
    part = torch.full((nsplits * mrows * n,), float("nan"),
                      dtype=torch.float32, device=DEV)
    nat.skinny_gemm_partials(part, a, w, kps, nsplits)
    # layout: slab sp, row mi, column ni holds the K-range sp of C[mi, ni].
    # Tolerance: exact bf16 products accumulated in f32 over <= 1216 terms;
    # sum|terms| ~ 1216 * (2/pi) * 0.5 * 0.05 ~ 19, times f32 eps 6e-8 times
    # the <= 38 sequential 32-wide MFMA accumulations ~ 5e-5; 1e-3 leaves 20x.
    slabs = part.view(nsplits, mrows, n)[:, :m]
    for sp in range(nsplits):
        ks = slice(sp * kps, min(k, (sp + 1) * kps))
        expect = a[:, ks].double() @ w[:, ks].double().t()
        torch.testing.assert_close(slabs[sp].double(), expect,
                                   atol=1e-3, rtol=0)
    for b in (bias, None):
        out = torch.empty(m, n, dtype=torch.bfloat16, device=DEV)
        nat.skinny_combine(out, part, b, nsplits, mrows)
        torch.testing.assert_close(
            out.float(), torch.nn.functional.linear(a, w, b).float(),
            atol=5e-2, rtol=5e-2)
        # and it is the ordered f32 sum, biased, rounded once
        s = torch.zeros(m, n, dtype=torch.float32, device=DEV)
        for sp in range(nsplits):
            s = s + slabs[sp]
        if b is not None:
            s = s + b.float()
        assert torch.equal(out, s.to(torch.bfloat16))


@pytest.mark.parametrize("m,k,n", [
    (1, 96, 64), (17, 416, 128), (64, 3584, 192), (64, 3584, 3584),
])
def test_skinny_gemm_matches_linear(m, k, n):
    """ops.skinny_gemm through the new layout, at its own split rule."""
    assert_native()
    torch.manual_seed(37)
    a = torch.randn(m, k, dtype=torch.bfloat16, device=DEV) * 0.5
    w = torch.randn(n, k, dtype=torch.bfloat16, device=DEV) * 0.05
    bias = torch.randn(n, dtype=torch.bfloat16, device=DEV)
    for b in (bias, None):
        torch.testing.assert_close(
            ops.skinny_gemm(a, w, b).float(),
            torch.nn.functional.linear(a, w, b).float(),
            atol=5e-2, rtol=5e-2)


# The first three are the shapes that matter (a single split pair, M and N
# off the tile sizes, the o_proj decode shape with 10 splits); the last two
# add the tall-K variant kernel (64-row slabs) and more than 16 splits (a
# second pass of the reduction loop).
@pytest.mark.parametrize("m,n,k", [
    (1, 64, 512), (17, 192, 416), (64, 3584, 3584),
    (64, 256, 1024), (5, 64, 8192),
])
@pytest.mark.parametrize("with_bias", [False, True])
def test_fused_add_rmsnorm_bit_equal(m, n, k, with_bias):
    assert_native()
    torch.manual_seed(41)
    x = torch.randn(m, k, dtype=torch.bfloat16, device=DEV) * 0.5
    w = torch.randn(n, k, dtype=torch.bfloat16, device=DEV) * 0.05
    bias = (torch.randn(n, dtype=torch.bfloat16, device=DEV)
            if with_bias else None)
    res = torch.randn(m, n, dtype=torch.bfloat16, device=DEV)
    nw = torch.randn(n, dtype=torch.bfloat16, device=DEV)

    res_ref = res.clone()
    y = ops.skinny_gemm(x, w, bias)
    out_ref, _ = ops.fused_add_rmsnorm(y, res_ref, nw, 1e-6)

    res_new = res.clone()
    h = ops.skinny_gemm(x, w, bias, defer=True)
    assert isinstance(h, ops.SplitKPending) and h.nsplits > 1
    out_new, _ = ops.fused_add_rmsnorm(h, res_new, nw, 1e-6)
    assert torch.equal(res_new, res_ref)
    assert torch.equal(out_new, out_ref)
    # the handle is still live: the fallback gives the plain GEMM result
    assert torch.equal(h.materialize(), y)


@pytest.mark.parametrize("hq,hkv,hd", [(4, 2, 128), (2, 1, 64)])
@pytest.mark.parametrize("T", [1, 5, 64])
@pytest.mark.parametrize("fp8", [False, True])
def test_fused_rope_cache_bit_equal(hq, hkv, hd, T, fp8):
    assert_native()
    torch.manual_seed(43)
    hidden, bs, nblocks = 512, 16, 16
    n = (hq + 2 * hkv) * hd
    dt = torch.float8_e4m3fn if fp8 else torch.bfloat16
    x = torch.randn(T, hidden, dtype=torch.bfloat16, device=DEV) * 0.5
    w = torch.randn(n, hidden, dtype=torch.bfloat16, device=DEV) * 0.05
    bias = torch.randn(n, dtype=torch.bfloat16, device=DEV)
    cos_sin = ref.rope_cos_sin_cache(hd, 64, 10000.0).cuda()
    pos = torch.randint(0, 64, (T,), dtype=torch.int64, device=DEV)
    # one padding row (slot -1); for T == 1 also the all-valid mapping
    masks = [T // 2] + ([None] if T == 1 else [])
    for skip in masks:
        slots = torch.tensor([-1 if i == skip else i * 3 for i in range(T)],
                             dtype=torch.int64, device=DEV)
        kc_ref = torch.zeros(nblocks, hkv, bs, hd, dtype=dt, device=DEV)
        vc_ref = torch.zeros_like(kc_ref)
        kc_new = torch.zeros_like(kc_ref)
        vc_new = torch.zeros_like(kc_ref)

        qkv = ops.skinny_gemm(x, w, bias)
        q, k, v = qkv.split([hq * hd, hkv * hd, hkv * hd], dim=-1)
        q_ref, _ = ops.rope_and_cache(pos, q, k, v, kc_ref, vc_ref, slots,
                                      cos_sin, hd)

        h = ops.skinny_gemm(x, w, bias, defer=True)
        assert isinstance(h, ops.SplitKPending) and h.nsplits > 1
        q_new = ops.rope_and_cache_splitk(pos, h, kc_new, vc_new, slots,
                                          cos_sin, hd, hq)
        assert q_new.is_contiguous() and q_new.shape == (T, hq * hd)
        assert torch.equal(q_new, q_ref)
        assert torch.equal(kc_new.view(torch.uint8), kc_ref.view(torch.uint8))
        assert torch.equal(vc_new.view(torch.uint8), vc_ref.view(torch.uint8))
        if skip is None:
            assert kc_ref.view(torch.uint8).any()  # something was cached


def test_bit_equal_at_qwen7b_decode_shapes():
    """The batch-64 Qwen2.5-7B decode shapes themselves. A last-bit drift
    (say, an fma contracted in one kernel and not in the other) shows up
    about once in 1e5 elements, so it needs this many to be seen: the small
    cases above passed with one present."""
    assert_native()
    torch.manual_seed(53)
    T, hq, hkv, hd, hidden, inter = 64, 28, 4, 128, 3584, 18944
    n = (hq + 2 * hkv) * hd
    x = torch.randn(T, hidden, dtype=torch.bfloat16, device=DEV) * 0.5
    w = torch.randn(n, hidden, dtype=torch.bfloat16, device=DEV) * 0.05
    bias = torch.randn(n, dtype=torch.bfloat16, device=DEV)
    cos_sin = ref.rope_cos_sin_cache(hd, 2048, 1000000.0).cuda()
    pos = torch.randint(0, 2048, (T,), dtype=torch.int64, device=DEV)
    slots = torch.arange(T, dtype=torch.int64, device=DEV) * 3
    for dt in (torch.bfloat16, torch.float8_e4m3fn):
        kc_ref = torch.zeros(16, hkv, 16, hd, dtype=dt, device=DEV)
        vc_ref, kc_new, vc_new = (torch.zeros_like(kc_ref) for _ in range(3))
        qkv = ops.skinny_gemm(x, w, bias)
        q, k, v = qkv.split([hq * hd, hkv * hd, hkv * hd], dim=-1)
        q_ref, _ = ops.rope_and_cache(pos, q, k, v, kc_ref, vc_ref, slots,
                                      cos_sin, hd)
        h = ops.skinny_gemm(x, w, bias, defer=True)
        q_new = ops.rope_and_cache_splitk(pos, h, kc_new, vc_new, slots,
                                          cos_sin, hd, hq)
        assert torch.equal(q_new, q_ref)
        assert torch.equal(kc_new.view(torch.uint8), kc_ref.view(torch.uint8))
        assert torch.equal(vc_new.view(torch.uint8), vc_ref.view(torch.uint8))

    # down_proj: the tall-K variant kernel, 8 splits of 64-row slabs
    a = torch.randn(T, inter, dtype=torch.bfloat16, device=DEV) * 0.5
    wd = torch.randn(hidden, inter, dtype=torch.bfloat16, device=DEV) * 0.02
    nw = torch.randn(hidden, dtype=torch.bfloat16, device=DEV)
    res = torch.randn(T, hidden, dtype=torch.bfloat16, device=DEV)
    res_ref, res_new = res.clone(), res.clone()
    out_ref, _ = ops.fused_add_rmsnorm(ops.skinny_gemm(a, wd), res_ref, nw)
    h = ops.skinny_gemm(a, wd, defer=True)
    assert isinstance(h, ops.SplitKPending) and h.mrows == 64
    out_new, _ = ops.fused_add_rmsnorm(h, res_new, nw)
    assert torch.equal(res_new, res_ref) and torch.equal(out_new, out_ref)


def test_stale_handle_raises_before_launch():
    assert_native()
    torch.manual_seed(47)
    x = torch.randn(4, 512, dtype=torch.bfloat16, device=DEV)
    w = torch.randn(64, 512, dtype=torch.bfloat16, device=DEV) * 0.05
    nw = torch.ones(64, dtype=torch.bfloat16, device=DEV)
    res = torch.randn(4, 64, dtype=torch.bfloat16, device=DEV)
    before = res.clone()
    h1 = ops.skinny_gemm(x, w, defer=True)
    h2 = ops.skinny_gemm(x, w, defer=True)
    with pytest.raises(RuntimeError, match="stale split-K handle"):
        ops.fused_add_rmsnorm(h1, res, nw, 1e-6)
    with pytest.raises(RuntimeError, match="stale split-K handle"):
        h1.materialize()
    torch.cuda.synchronize()
    assert torch.equal(res, before)  # nothing ran on the residual
    ops.fused_add_rmsnorm(h2, res, nw, 1e-6)  # the live one is fine
    assert not torch.equal(res, before)


def test_engine_greedy_tokens_equal_fused_and_unfused(monkeypatch):
    """tiny-gpu engine: the same greedy tokens with the fusion on and off,
    and the fused kernels really are on the decode path when it is on."""
    assert_native()
    prompts = [[1, 5, 9, 20, 7, 3], [2, 4, 6]]
    sp = SamplingParams(max_tokens=8, ignore_eos=True)
    calls = {"rope": 0, "norm": 0}
    real_rope, real_norm = ops.rope_and_cache_splitk, ops.fused_add_rmsnorm

    def rope(*a, **kw):
        calls["rope"] += 1
        return real_rope(*a, **kw)

    def norm(x, *a, **kw):
        calls["norm"] += isinstance(x, ops.SplitKPending)
        return real_norm(x, *a, **kw)

    monkeypatch.setattr(ops, "rope_and_cache_splitk", rope)
    monkeypatch.setattr(ops, "fused_add_rmsnorm", norm)
    outs = {}
    for fuse in (True, False):
        monkeypatch.setattr(ops, "_SPLITK_FUSE", fuse)
        calls["rope"] = calls["norm"] = 0
        engine = LLMEngine(EngineConfig(
            preset="tiny-gpu", device="cuda", kv_cache_blocks=256,
            max_model_len=1024, seed=5,
        ))
        outs[fuse] = engine.generate(prompts, sp)
        if fuse:
            assert calls["rope"] > 0 and calls["norm"] > 0
        else:
            assert calls["rope"] == 0 and calls["norm"] == 0
        del engine
    assert all(len(o) == 8 for o in outs[True])
    assert outs[True] == outs[False]
