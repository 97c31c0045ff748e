"""W4A16 kernels (w4_gemm.hip) and the int4 / AWQ engine modes on the GPU.

References: ops.ref.w4_dequant (f32) for the kernels, the unfused op
sequence for the split-K consumers (bit-equal), and the eager engine for the
captured one."""

import pytest
import torch

import arks_amd.ops as ops
from arks_amd.config import PRESET_CONFIGS, EngineConfig
from arks_amd.engine import LLMEngine, SamplingParams
from arks_amd.ops import ref

pytestmark = pytest.mark.gpu

DEV = "cuda"


def assert_native():
    assert ops.native_available(), "HIP extension must be built on a GPU box"


def _random_w4(n, k, seed, pow2_scales=False):
    """Random (q, z, s) on the CPU with weights of std ~0.05 (q - z is
    uniform-ish over +-15 with std ~6.5, s ~ 0.0077), or power-of-two scales
    for exact tests. q and z are forced to contain 0 and 15."""
    g = torch.Generator().manual_seed(seed)
    G = k // 128
    q = torch.randint(0, 16, (n, k), generator=g, dtype=torch.uint8)
    z = torch.randint(0, 16, (n, G), generator=g, dtype=torch.uint8)
    q[0, 0], q[0, 1], z[0, 0], z[-1, -1] = 0, 15, 0, 15
    if pow2_scales:
        e = torch.randint(1, 5, (n, G), generator=g)
        s = torch.pow(2.0, -e.float())
    else:
        s = (0.0077 * (0.5 + torch.rand(n, G, generator=g))).half().float()
    return q, z, s


def _to_dev(packed):
    return tuple(t.to(DEV) for t in packed)


def _mt_rows(m):
    return 16 * min(-(-m // 16), 4)


@pytest.mark.parametrize("nw", [1, 2])
@pytest.mark.parametrize("nsplits", [1, 2])
def test_exact_fragment_mapping(nw, nsplits):
    """One-hot activations and power-of-two scales make every step exact, so
    each output row must be one column of the dequantized weight, bit for
    bit: any slip in the nibble order, the k permutation of the A fragment,
    the C fragment rows or the scale/zero-point lanes shows."""
    assert_native()
    n, k, m = 128, 256, 64
    q, z, s = _random_w4(n, k, 3, pow2_scales=True)
    wd = ref.w4_dequant(q, z, s).to(DEV)
    packed = _to_dev(ref.w4_pack(q, z, s))
    plan = (nw, nsplits, k // nsplits, _mt_rows(m))
    for c in range(4):
        x = torch.zeros(m, k, dtype=torch.bfloat16, device=DEV)
        x[torch.arange(m), 64 * c + torch.arange(m)] = 1.0
        out = ops.w4_linear(x, packed, plan=plan)
        assert out.dtype == torch.bfloat16 and out.shape == (m, n)
        expect = wd[:, 64 * c: 64 * c + m].t()
        assert torch.equal(out.float(), expect), (c, nw, nsplits)


@pytest.mark.parametrize("m", [1, 16, 17, 48, 64])
@pytest.mark.parametrize("n,k", [(64, 128), (128, 384), (1024, 256),
                                 (256, 1024)])
def test_numerics_small_m(m, n, k):
    assert_native()
    q, z, s = _random_w4(n, k, 5)
    wd = ref.w4_dequant(q, z, s).to(DEV)
    packed = _to_dev(ref.w4_pack(q, z, s))
    torch.manual_seed(7)
    x = torch.randn(m, k, dtype=torch.bfloat16, device=DEV) * 0.5
    bias = torch.randn(n, dtype=torch.bfloat16, device=DEV)
    # row-strided view of the same values
    wide = torch.zeros(m, k + 64, dtype=torch.bfloat16, device=DEV)
    wide[:, :k] = x
    for b in (None, bias):
        expect = x.float() @ wd.t()
        if b is not None:
            expect = expect + b.float()
        out = ops.w4_linear(x, packed, b)
        torch.testing.assert_close(out.float(), expect, atol=5e-2, rtol=5e-2)
        assert torch.equal(ops.w4_linear(wide[:, :k], packed, b), out)
        # every split count the shape allows gives the same answer
        for nsplits in (2, 3):
            chunks = k // 128
            if chunks < nsplits:
                continue
            kps = -(-chunks // nsplits) * 128
            plan = (1, -(-k // kps), kps, _mt_rows(m))
            if plan[1] < 2:
                continue
            o2 = ops.w4_linear(x, packed, b, plan=plan)
            torch.testing.assert_close(o2.float(), expect, atol=5e-2,
                                       rtol=5e-2)


@pytest.mark.parametrize("m", [65, 200])
def test_numerics_large_m(m):
    """M > 64: 65 rows take the per-64-row-slab route (a full slab and a
    one-row slab), 200 rows w4_dequant_kernel into the reserved workspace and
    the library GEMM."""
    assert 65 <= ops.W4_SLAB_MAX_M < 200
    assert_native()
    n, k = 256, 1024
    q, z, s = _random_w4(n, k, 11)
    wd = ref.w4_dequant(q, z, s).to(DEV)
    packed = _to_dev(ref.w4_pack(q, z, s))
    ops.reserve_dequant_workspace(n * k, DEV)
    torch.manual_seed(13)
    x = torch.randn(m, k, dtype=torch.bfloat16, device=DEV) * 0.5
    bias = torch.randn(n, dtype=torch.bfloat16, device=DEV)
    for b in (None, bias):
        expect = x.float() @ wd.t()
        if b is not None:
            expect = expect + b.float()
        torch.testing.assert_close(ops.w4_linear(x, packed, b).float(),
                                   expect, atol=5e-2, rtol=5e-2)


def test_dequant_kernel_bit_equal():
    assert_native()
    n, k = 128, 384
    q, z, s = _random_w4(n, k, 17)
    packed = _to_dev(ref.w4_pack(q, z, s))
    out = ops.w4_dequant(packed)
    assert out.shape == (n, k) and out.dtype == torch.bfloat16
    assert torch.equal(out.cpu(), ref.w4_dequant(q, z, s).to(torch.bfloat16))


def test_gpu_rejects_what_it_cannot_run():
    """No silent fallback: shapes outside the kernels raise."""
    assert_native()
    q, z, s = _random_w4(96, 128, 19)  # N % 64 != 0
    packed = _to_dev(ref.w4_pack(q, z, s))
    x = torch.zeros(4, 128, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="N % 64"):
        ops.w4_linear(x, packed)


def _forced_plan(m, n, k):
    """The default plan, or a 2-way split where it would not split."""
    plan = ops._w4_plan(m, n, k)
    if plan[1] > 1:
        return plan
    assert k >= 256
    kps = -(-(k // 128) // 2) * 128
    return (plan[0], -(-k // kps), kps, plan[3])


# test_splitk_fused_gpu.py's shapes with K rounded to the 128 group.
@pytest.mark.parametrize("m,n,k", [
    (1, 64, 512), (17, 192, 384), (64, 3584, 3584),
    (64, 256, 1024), (5, 64, 8192),
])
@pytest.mark.parametrize("with_bias", [False, True])
def test_deferred_add_rmsnorm_bit_equal(m, n, k, with_bias):
    assert_native()
    q, z, s = _random_w4(n, k, 23)
    packed = _to_dev(ref.w4_pack(q, z, s))
    torch.manual_seed(41)
    x = torch.randn(m, k, dtype=torch.bfloat16, device=DEV) * 0.5
    bias = (torch.randn(n, dtype=torch.bfloat16, device=DEV)
            if with_bias else None)
    res = torch.randn(m, n, dtype=torch.bfloat16, device=DEV)
    nw = torch.randn(n, dtype=torch.bfloat16, device=DEV)
    plan = _forced_plan(m, n, k)

    res_ref = res.clone()
    y = ops.w4_linear(x, packed, bias, plan=plan)
    out_ref, _ = ops.fused_add_rmsnorm(y, res_ref, nw, 1e-6)

    res_new = res.clone()
    h = ops.w4_linear(x, packed, bias, defer=True, plan=plan)
    assert isinstance(h, ops.SplitKPending) and h.nsplits > 1
    assert torch.equal(h.materialize(), y)
    out_new, _ = ops.fused_add_rmsnorm(h, res_new, nw, 1e-6)
    assert torch.equal(res_new, res_ref)
    assert torch.equal(out_new, out_ref)


@pytest.mark.parametrize("hq,hkv,hd", [(4, 2, 128), (2, 1, 64)])
@pytest.mark.parametrize("T", [1, 5, 64])
@pytest.mark.parametrize("fp8", [False, True])
def test_deferred_rope_cache_bit_equal(hq, hkv, hd, T, fp8):
    assert_native()
    hidden, bs, nblocks = 512, 16, 16
    n = (hq + 2 * hkv) * hd
    dt = torch.float8_e4m3fn if fp8 else torch.bfloat16
    q4, z4, s4 = _random_w4(n, hidden, 29)
    packed = _to_dev(ref.w4_pack(q4, z4, s4))
    torch.manual_seed(43)
    x = torch.randn(T, hidden, dtype=torch.bfloat16, device=DEV) * 0.5
    bias = torch.randn(n, dtype=torch.bfloat16, device=DEV)
    cos_sin = ref.rope_cos_sin_cache(hd, 64, 10000.0).cuda()
    pos = torch.randint(0, 64, (T,), dtype=torch.int64, device=DEV)
    slots = torch.tensor([-1 if i == T // 2 and T > 1 else i * 3
                          for i in range(T)], dtype=torch.int64, device=DEV)
    plan = _forced_plan(T, n, hidden)
    kc_ref = torch.zeros(nblocks, hkv, bs, hd, dtype=dt, device=DEV)
    vc_ref, kc_new, vc_new = (torch.zeros_like(kc_ref) for _ in range(3))

    qkv = ops.w4_linear(x, packed, bias, plan=plan)
    q, k, v = qkv.split([hq * hd, hkv * hd, hkv * hd], dim=-1)
    q_ref, _ = ops.rope_and_cache(pos, q, k, v, kc_ref, vc_ref, slots,
                                  cos_sin, hd)
    h = ops.w4_linear(x, packed, bias, defer=True, plan=plan)
    assert isinstance(h, ops.SplitKPending) and h.nsplits > 1
    q_new = ops.rope_and_cache_splitk(pos, h, kc_new, vc_new, slots,
                                      cos_sin, hd, hq)
    assert torch.equal(q_new, q_ref)
    assert torch.equal(kc_new.view(torch.uint8), kc_ref.view(torch.uint8))
    assert torch.equal(vc_new.view(torch.uint8), vc_ref.view(torch.uint8))
    assert kc_ref.view(torch.uint8).any()


# ------------------------------ engine ------------------------------------
PROMPTS = [[1, 5, 9, 20, 7, 3], [2, 4, 6], [11, 12, 13, 14]]
SP = SamplingParams(max_tokens=8, ignore_eos=True)


def _engine(**kw):
    kw.setdefault("preset", "tiny-gpu")
    if kw.get("model_path"):
        kw.pop("preset")
    return LLMEngine(EngineConfig(device="cuda", kv_cache_blocks=512,
                                  max_model_len=1024, seed=5, **kw))


def test_engine_int4_graph_equals_eager_and_deterministic():
    assert_native()
    outs = []
    for eager in (False, True, False):
        e = _engine(quantization="int4", enforce_eager=eager)
        mod = e.runner.model.layers[0].mlp.down_proj
        assert mod.w4 and mod.weight is None and mod.w4_qweight.is_cuda
        outs.append(e.generate(PROMPTS, SP))
        del e
    assert all(len(o) == 8 for o in outs[0])
    assert outs[0] == outs[1] == outs[2]


@pytest.mark.parametrize("batch", [70, 130])
def test_engine_int4_large_batch_graph_equals_eager(batch):
    """Both M > 64 routes inside a captured decode step: 70 sequences pad to
    the 96-row graph (skinny kernel per 64-row slab), 130 to the 192-row one
    (dequant workspace + library GEMM; the workspace pointer is captured)."""
    assert_native()
    assert 96 <= ops.W4_SLAB_MAX_M < 192
    prompts = [[(7 * i + j) % 2000 + 1 for j in range(3 + i % 4)]
               for i in range(batch)]
    sp = SamplingParams(max_tokens=4, ignore_eos=True)
    outs = []
    for eager in (False, True):
        e = _engine(quantization="int4", enforce_eager=eager)
        outs.append(e.generate(prompts, sp))
        del e
    assert all(len(o) == 4 for o in outs[0])
    assert outs[0] == outs[1]


def test_engine_int4_with_fp8_kv_runs_and_is_deterministic():
    assert_native()
    outs = []
    for _ in range(2):
        e = _engine(quantization="int4", kv_cache_dtype="fp8")
        outs.append(e.generate(PROMPTS, SP))
        del e
    assert all(len(o) == 8 for o in outs[0])
    assert outs[0] == outs[1]


def test_engine_awq_checkpoint_agrees_with_dequantized_bf16(tmp_path):
    """The AWQ engine runs the W4 kernels (f32 dequant, group-wise
    accumulation); the bf16 engine runs the same weights rounded to bf16
    through other GEMMs. Reduction orders differ, so — as for the fp8 KV
    cache test — greedy tokens are required to agree on at least half of the
    generated positions, not everywhere."""
    assert_native()
    from arks_amd.loader.safetensors_loader import save_awq_checkpoint

    awq_dir, bf16_dir = str(tmp_path / "awq"), str(tmp_path / "bf16")
    save_awq_checkpoint(PRESET_CONFIGS["tiny-gpu"], awq_dir, seed=3,
                        dequantized_dir=bf16_dir)
    e = _engine(model_path=awq_dir)
    assert e.runner.model.layers[0].self_attn.qkv_proj.w4
    a = e.generate(PROMPTS, SP)
    del e
    e = _engine(model_path=bf16_dir)
    assert not e.runner.model.layers[0].self_attn.qkv_proj.w4
    b = e.generate(PROMPTS, SP)
    del e
    total = sum(len(o) for o in a)
    same = sum(x == y for oa, ob in zip(a, b) for x, y in zip(oa, ob))
    print(f"awq vs dequantized-bf16 token agreement: {same}/{total}")
    assert total == 8 * len(PROMPTS)
    assert same * 2 >= total
