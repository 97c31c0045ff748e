"""MX4 (MXFP4, W4A16) kernels (mx4_gemm.hip) and MXFP4 checkpoints on the GPU.

References: ops.ref.mx4_dequant (f32, exact) for the kernels, the unfused op
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


def _random_mx4(n, k, seed):
    """(packed u8 [n, k/2], scales u8 [n, k/32]) on the CPU from weights of
    std 0.05 through the MX quantizer."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(n, k, generator=g) * 0.05
    return ref.mx4_quantize(w)


def _to_dev(weight):
    return tuple(t.to(DEV) for t in weight)


def _mt_rows(m):
    return 16 * min(-(-m // 16), 4)


@pytest.mark.parametrize("nw", [1, 2])
@pytest.mark.parametrize("nsplits", [1, 2])
def test_exact_fragment_mapping_and_conversion(nw, nsplits):
    """One-hot activations make every step exact (an e2m1 value times a power
    of two is a bf16), so each output row must be one column of the
    dequantized weight, bit for bit: any slip in the nibble order, the byte
    select of the conversion, the k permutation of the A fragment, the C
    fragment rows or the lane that owns a scale byte shows. All 16 codes
    occur, and one block each sits at the two ends of the accepted scale
    range (2: 0.5 * 2^-125 is the smallest normal bf16; 252: 6 * 2^125 is
    finite)."""
    assert_native()
    n, k, m = 128, 256, 64
    g = torch.Generator().manual_seed(3)
    codes = torch.arange(16, dtype=torch.uint8).repeat(n * k // 16)
    codes = codes[torch.randperm(n * k, generator=g)].view(n, k)
    assert set(codes.flatten().tolist()) == set(range(16))
    packed = (codes[:, 0::2] | (codes[:, 1::2] << 4)).contiguous()
    scales = torch.randint(117, 138, (n, k // 32), generator=g,
                           dtype=torch.uint8)
    scales[5, 1] = ref.MX4_SCALE_MIN
    scales[70, 6] = ref.MX4_SCALE_MAX
    assert (scales.min(), scales.max()) == (2, 252)
    wd = ref.mx4_dequant(packed, scales)
    assert torch.isfinite(wd).all()
    assert torch.equal(wd.to(torch.bfloat16).float(), wd)
    wd = wd.to(DEV)
    weight = _to_dev((packed, scales))
    plan = (nw, nsplits, k // nsplits, _mt_rows(m))
    for c in range(4):
        x = torch.zeros(m, k, dtype=torch.bfloat16, device=DEV)
        x[torch.arange(m), 64 * c + torch.arange(m)] = 1.0
        out = ops.mx4_linear(x, weight, plan=plan)
        assert out.dtype == torch.bfloat16 and out.shape == (m, n)
        expect = wd[:, 64 * c: 64 * c + m].t()
        assert torch.equal(out.float(), expect), (c, nw, nsplits)


@pytest.mark.parametrize("m", [1, 16, 17, 48, 64])
@pytest.mark.parametrize("n,k", [(64, 128), (128, 384), (1024, 256),
                                 (256, 1024)])
def test_numerics_small_m(m, n, k):
    assert_native()
    packed, scales = _random_mx4(n, k, 5)
    wd = ref.mx4_dequant(packed, scales).to(DEV)
    weight = _to_dev((packed, scales))
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
        out = ops.mx4_linear(x, weight, b)
        torch.testing.assert_close(out.float(), expect, atol=5e-2, rtol=5e-2)
        assert torch.equal(ops.mx4_linear(wide[:, :k], weight, b), out)
        # every split count the shape allows gives the same answer
        for nsplits in (2, 3):
            chunks = k // 128
            if chunks < nsplits:
                continue
            kps = -(-chunks // nsplits) * 128
            plan = (1, -(-k // kps), kps, _mt_rows(m))
            if plan[1] < 2:
                continue
            o2 = ops.mx4_linear(x, weight, b, plan=plan)
            torch.testing.assert_close(o2.float(), expect, atol=5e-2,
                                       rtol=5e-2)


@pytest.mark.parametrize("m", [65, 200])
def test_numerics_large_m(m):
    """M > 64: 65 rows take the per-64-row-slab route (a full slab and a
    one-row slab), 200 rows mx4_dequant_kernel into the reserved workspace
    and the library GEMM."""
    assert 65 <= ops.MX4_SLAB_MAX_M < 200
    assert_native()
    n, k = 256, 1024
    packed, scales = _random_mx4(n, k, 11)
    wd = ref.mx4_dequant(packed, scales).to(DEV)
    weight = _to_dev((packed, scales))
    ops.reserve_dequant_workspace(n * k, DEV)
    torch.manual_seed(13)
    x = torch.randn(m, k, dtype=torch.bfloat16, device=DEV) * 0.5
    bias = torch.randn(n, dtype=torch.bfloat16, device=DEV)
    for b in (None, bias):
        expect = x.float() @ wd.t()
        if b is not None:
            expect = expect + b.float()
        torch.testing.assert_close(ops.mx4_linear(x, weight, b).float(),
                                   expect, atol=5e-2, rtol=5e-2)


def test_dequant_kernel_bit_equal():
    assert_native()
    n, k = 128, 384
    packed, scales = _random_mx4(n, k, 17)
    out = ops.mx4_dequant(_to_dev((packed, scales)))
    assert out.shape == (n, k) and out.dtype == torch.bfloat16
    expect = ref.mx4_dequant(packed, scales)
    assert torch.equal(out.cpu().float(), expect)


def test_gpu_rejects_what_it_cannot_run():
    """No silent fallback: shapes outside the kernels raise."""
    assert_native()
    packed, scales = _random_mx4(96, 128, 19)  # N % 64 != 0
    weight = _to_dev((packed, scales))
    x = torch.zeros(4, 128, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="N % 64"):
        ops.mx4_linear(x, weight)


def _forced_plan(m, n, k):
    """The default plan, or a 2-way split where it would not split."""
    plan = ops._mx4_plan(m, n, k)
    if plan[1] > 1:
        return plan
    assert k >= 256
    kps = -(-(k // 128) // 2) * 128
    return (plan[0], -(-k // kps), kps, plan[3])


# test_w8_gpu.py's shapes: MT = 2 with an N off the 128 tile pair, and the
# square decode shape at nw = 2
@pytest.mark.parametrize("m,n,k", [(17, 192, 384), (64, 3584, 3584)])
@pytest.mark.parametrize("with_bias", [False, True])
def test_deferred_add_rmsnorm_bit_equal(m, n, k, with_bias):
    assert_native()
    weight = _to_dev(_random_mx4(n, k, 23))
    torch.manual_seed(41)
    x = torch.randn(m, k, dtype=torch.bfloat16, device=DEV) * 0.5
    bias = (torch.randn(n, dtype=torch.bfloat16, device=DEV)
            if with_bias else None)
    res = torch.randn(m, n, dtype=torch.bfloat16, device=DEV)
    nw = torch.randn(n, dtype=torch.bfloat16, device=DEV)
    plan = _forced_plan(m, n, k)

    res_ref = res.clone()
    y = ops.mx4_linear(x, weight, bias, plan=plan)
    out_ref, _ = ops.fused_add_rmsnorm(y, res_ref, nw, 1e-6)

    res_new = res.clone()
    h = ops.mx4_linear(x, weight, bias, defer=True, plan=plan)
    assert isinstance(h, ops.SplitKPending) and h.nsplits > 1
    assert torch.equal(h.materialize(), y)
    out_new, _ = ops.fused_add_rmsnorm(h, res_new, nw, 1e-6)
    assert torch.equal(res_new, res_ref)
    assert torch.equal(out_new, out_ref)


@pytest.mark.parametrize("hq,hkv,hd", [(4, 2, 128), (2, 1, 64)])
@pytest.mark.parametrize("T", [5, 64])
@pytest.mark.parametrize("fp8", [False, True])
def test_deferred_rope_cache_bit_equal(hq, hkv, hd, T, fp8):
    assert_native()
    hidden, bs, nblocks = 512, 16, 16
    n = (hq + 2 * hkv) * hd
    dt = torch.float8_e4m3fn if fp8 else torch.bfloat16
    weight = _to_dev(_random_mx4(n, hidden, 29))
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

    qkv = ops.mx4_linear(x, weight, bias, plan=plan)
    q, k, v = qkv.split([hq * hd, hkv * hd, hkv * hd], dim=-1)
    q_ref, _ = ops.rope_and_cache(pos, q, k, v, kc_ref, vc_ref, slots,
                                  cos_sin, hd)
    h = ops.mx4_linear(x, weight, bias, defer=True, plan=plan)
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


@pytest.fixture(scope="module")
def mx4_dirs(tmp_path_factory):
    from arks_amd.loader.safetensors_loader import save_mx4_checkpoint

    root = tmp_path_factory.mktemp("mx4")
    dirs = {k: str(root / k) for k in ("mx4", "bf16")}
    save_mx4_checkpoint(PRESET_CONFIGS["tiny-gpu"], dirs["mx4"], seed=3,
                        dequantized_dir=dirs["bf16"])
    return dirs


def _engine(model_path, **kw):
    return LLMEngine(EngineConfig(model_path=model_path, device="cuda",
                                  kv_cache_blocks=512, max_model_len=1024,
                                  seed=5, **kw))


def test_engine_mx4_checkpoint_graph_equals_eager_and_deterministic(mx4_dirs):
    assert_native()
    outs = []
    for eager in (False, True, False):
        e = _engine(mx4_dirs["mx4"], enforce_eager=eager)
        assert e.runner.quantization == "mxfp4"
        layer = e.runner.model.layers[0]
        for mod in (layer.self_attn.qkv_proj, layer.self_attn.o_proj,
                    layer.mlp.gate_up_proj, layer.mlp.down_proj):
            assert mod.mx4 and mod.weight is None
            for t in (mod.mx4_weight, mod.mx4_scales):
                assert t.is_cuda and t.dtype == torch.uint8
            assert not hasattr(mod, "weight_qdq")
        outs.append(e.generate(PROMPTS, SP))
        del e
    assert all(len(o) == 8 for o in outs[0])
    assert outs[0] == outs[1] == outs[2]


@pytest.mark.parametrize("batch", [70, 130])
def test_engine_mx4_checkpoint_large_batch_graph_equals_eager(mx4_dirs, batch):
    """Both M > 64 routes inside a captured decode step: 70 sequences pad to
    the 96-row graph (skinny kernel per 64-row slab), 130 to the 192-row one
    (dequant workspace + library GEMM; the workspace pointer is captured)."""
    assert_native()
    assert 96 <= ops.MX4_SLAB_MAX_M < 192
    prompts = [[(7 * i + j) % 2000 + 1 for j in range(3 + i % 4)]
               for i in range(batch)]
    sp = SamplingParams(max_tokens=4, ignore_eos=True)
    outs = []
    for eager in (False, True):
        e = _engine(mx4_dirs["mx4"], enforce_eager=eager)
        outs.append(e.generate(prompts, sp))
        del e
    assert all(len(o) == 4 for o in outs[0])
    assert outs[0] == outs[1]


def test_engine_mx4_checkpoint_with_fp8_kv_runs_and_is_deterministic(mx4_dirs):
    assert_native()
    outs = []
    for _ in range(2):
        e = _engine(mx4_dirs["mx4"], kv_cache_dtype="fp8")
        outs.append(e.generate(PROMPTS, SP))
        del e
    assert all(len(o) == 8 for o in outs[0])
    assert outs[0] == outs[1]


def test_engine_mx4_checkpoint_agrees_with_dequantized_bf16(mx4_dirs):
    """The MX4 engine runs the MX4 kernels (exact scaled e2m1 -> bf16
    conversion, f32 chunk sums); the bf16 engine runs the same weights, which
    bf16 holds exactly, through other GEMMs. Reduction orders differ, so
    — the rule of test_engine_awq_checkpoint_agrees_with_dequantized_bf16 —
    greedy tokens are required to agree on at least half of the generated
    positions, not everywhere."""
    assert_native()
    e = _engine(mx4_dirs["mx4"])
    assert e.runner.model.layers[0].self_attn.qkv_proj.mx4
    a = e.generate(PROMPTS, SP)
    del e
    e = _engine(mx4_dirs["bf16"])
    assert not e.runner.model.layers[0].self_attn.qkv_proj.mx4
    b = e.generate(PROMPTS, SP)
    del e
    total = sum(len(o) for o in a)
    same = sum(x == y for oa, ob in zip(a, b) for x, y in zip(oa, ob))
    print(f"mxfp4 checkpoint vs dequantized-bf16 token agreement: "
          f"{same}/{total}")
    assert total == 8 * len(PROMPTS)
    assert same * 2 >= total


def test_engine_mx4_ngram_speculation_is_greedy_exact(mx4_dirs):
    assert_native()
    prompts = [[5, 6, 7, 5, 6, 7, 5, 6], [2, 4, 6]]
    sp = SamplingParams(max_tokens=10, ignore_eos=True)
    e = _engine(mx4_dirs["mx4"])
    base = e.generate(prompts, sp)
    del e
    e = _engine(mx4_dirs["mx4"], speculative="ngram")
    spec = e.generate(prompts, sp)
    del e
    assert all(len(o) == 10 for o in base)
    assert spec == base


def test_engine_mx4_embeddings_close_to_the_dequantized_twin(mx4_dirs):
    """Pooled, L2-normalised embeddings of the MX4 engine against the bf16
    engine on the same (exactly representable) weights: only the GEMM
    reduction orders differ, each output rounded to bf16 (relative 2^-8)
    through two layers, so the cosine of unit vectors stays within 1e-2 of
    1."""
    assert_native()
    prompts = [[1, 5, 9, 20, 7, 3, 11, 12], [2, 4, 6]]
    e = _engine(mx4_dirs["mx4"])
    a = e.embed(prompts, {"mode": "last"})
    del e
    e = _engine(mx4_dirs["bf16"])
    b = e.embed(prompts, {"mode": "last"})
    del e
    for x, y in zip(a, b):
        x, y = torch.as_tensor(x).float(), torch.as_tensor(y).float()
        assert x.shape == y.shape and torch.isfinite(x).all()
        cos = torch.dot(x, y) / (x.norm() * y.norm())
        print(f"mx4 vs bf16 embedding cosine: {cos.item():.6f}")
        assert cos > 0.99
