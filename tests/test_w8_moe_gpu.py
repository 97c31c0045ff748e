"""W8 MoE experts on the GPU: w8_moe_gemm_kernel, the W8 MoEMLP forward and
the engine on a block-scaled FP8 MoE checkpoint.

References: ops.ref.moe_route for the table, the f32 product with the
dequantized weights (ops.ref.w8_dequant) for the GEMM, an f32 evaluation of
the block for the layer, and the eager engine for the captured one."""

import pytest
import torch
import torch.nn.functional as F

import arks_amd.ops as ops
from arks_amd.config import PRESET_CONFIGS, EngineConfig
from arks_amd.engine import LLMEngine, SamplingParams
from arks_amd.ops import ref

pytestmark = pytest.mark.gpu

DEV = "cuda"


def assert_native():
    assert ops.native_available(), "HIP extension must be built on a GPU box"


def _distinct_ids(T, k, E, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(T, E, generator=g).topk(k, dim=-1).indices.to(
        torch.int32)


def _all_codes(n, k, g):
    """e4m3fn [n, k] holding all 254 non-NaN codes, shuffled."""
    codes = torch.arange(256, dtype=torch.int64).repeat(n * k // 256)
    codes = codes[torch.randperm(n * k, generator=g)]
    codes[codes == 0x7F] = 0x7E   # the two NaN codes -> +-448
    codes[codes == 0xFF] = 0xFE
    w8 = codes.to(torch.uint8).view(n, k).view(torch.float8_e4m3fn)
    assert (set(w8.view(torch.uint8).flatten().tolist())
            == set(range(256)) - {0x7F, 0xFF})
    return w8


# ------------------------------ exact mapping ------------------------------
@pytest.mark.parametrize("n", [64, 128])
@pytest.mark.parametrize("src_div", [2, 1])
def test_exact_mapping_and_untouched_rows(src_div, n):
    """One-hot activations and power-of-two scales make every step exact, so
    each written row must be one column of ITS expert's dequantized weight,
    bit for bit: a wrong expert offset in the weights or in the scales (both
    differ per expert, the scales per k-block too), a wrong byte order or a
    conversion that slips on a subnormal, on -0 or on +-448 shows. The three
    local experts get 0, 17 and 65 rows (an empty list, a partial tile, a
    second slab of one row); the pairs of a fourth, non-local expert must
    keep the sentinel `out` was filled with. N = 64 runs one sub-tile per
    workgroup, N = 128 at max_rows = 65 two."""
    assert_native()
    E, K, k, T = 3, 256, 2, 65
    base = 1  # local experts are global ids 1, 2, 3; id 0 is another rank's
    ids = torch.empty(T, k, dtype=torch.int32)
    for t in range(T):
        other = 2 if t < 17 else 0
        ids[t] = torch.tensor([3, other] if t % 2 else [other, 3])
    counts, pairs = ref.moe_route(ids, base, E)
    assert counts.tolist() == [0, 17, 65]
    g = torch.Generator().manual_seed(3 + n)
    w8 = torch.stack([_all_codes(n, K, g).view(torch.uint8)
                      for _ in range(E)]).view(torch.float8_e4m3fn)
    scales = torch.pow(
        2.0, -torch.randint(1, 5, (E, K // 128, n), generator=g).float())
    assert not torch.equal(w8[1].view(torch.uint8), w8[2].view(torch.uint8))
    assert not torch.equal(scales[1], scales[2])
    assert not torch.equal(scales[2, 0], scales[2, 1])
    wd = torch.stack([ref.w8_dequant(w8[e], scales[e]) for e in range(E)])

    n_pairs = T * k
    rows_a = T if src_div == k else n_pairs
    cols = (7 * torch.arange(rows_a) + 1) % K
    a = torch.zeros(rows_a, K, dtype=torch.bfloat16)
    a[torch.arange(rows_a), cols] = 1.0
    out = torch.full((n_pairs, n), -3.0, dtype=torch.bfloat16, device=DEV)
    got = ops.w8_moe_gemm(a.to(DEV), (w8.to(DEV), scales.to(DEV)),
                          counts.to(DEV), pairs.to(DEV), src_div, T, out=out)
    assert got is out
    out = out.cpu().float()
    flat = ids.reshape(-1)
    for p in range(n_pairs):
        le = int(flat[p]) - base
        if le < 0:
            assert (out[p] == -3.0).all(), p
        else:
            assert torch.equal(out[p], wd[le][:, cols[p // src_div]]), p


# ------------------------------- numerics ----------------------------------
def _random_experts(E, n, k, seed):
    """(stacked W8 pair on the GPU, f32 dequantized [E, n, k] on the CPU):
    weights of std 0.05 through the block quantizer, a seed per expert."""
    w8s, scs = [], []
    for e in range(E):
        g = torch.Generator().manual_seed(seed + e)
        w8, blocks = ref.w8_quantize(torch.randn(n, k, generator=g) * 0.05)
        w8s.append(w8.view(torch.uint8))
        scs.append(ref.w8_expand_scales(blocks, n))
    w8 = torch.stack(w8s).view(torch.float8_e4m3fn)
    sc = torch.stack(scs)
    wd = torch.stack([ref.w8_dequant(w8[e], sc[e]) for e in range(E)])
    return (w8.to(DEV), sc.to(DEV)), wd


@pytest.mark.parametrize("T", [1, 16, 70])
@pytest.mark.parametrize("n,k_dim", [(64, 128), (512, 512), (512, 256)])
def test_numerics(T, n, k_dim):
    """Against the f32 product with the dequantized weights, at the
    tolerance tests/test_w8_gpu.py and tests/test_w4_moe_gpu.py use for the
    same weight and activation scales."""
    assert_native()
    E, k = 4, 2
    weight, wd = _random_experts(E, n, k_dim, 5)
    ids = _distinct_ids(T, k, E, 31 + T)
    counts, pairs = ops.moe_route(ids.to(DEV), 0, E)
    flat = ids.reshape(-1).long()
    torch.manual_seed(7)
    for src_div in (k, 1):
        rows_a = T * k // src_div
        a = (torch.randn(rows_a, k_dim) * 0.5).to(torch.bfloat16)
        src = torch.arange(T * k) // src_div
        expect = torch.einsum("pk,pnk->pn", a[src].float(), wd[flat])
        out = ops.w8_moe_gemm(a.to(DEV), weight, counts, pairs, src_div, T)
        assert out.shape == (T * k, n) and out.dtype == torch.bfloat16
        torch.testing.assert_close(out.cpu().float(), expect, atol=5e-2,
                                   rtol=5e-2)


# ------------------------------ layer level --------------------------------
@pytest.fixture(scope="module")
def moe_layers():
    """(W8 block, bf16 block holding the same dequantized weights, their f32
    dequantized weights) of the tiny-moe-gpu shape."""
    from arks_amd.models.llama_family import MoEMLP

    cfg = PRESET_CONFIGS["tiny-moe-gpu"]
    torch.manual_seed(11)
    w8 = MoEMLP(cfg).to(DEV)
    w8.gate.data.normal_(0, 0.5)
    w8.w13.data.normal_(0, 0.05)
    w8.w2.data.normal_(0, 0.05)
    gate = w8.gate.data.clone()
    w8.quantize_w8("test")
    f32 = {}
    for which in ("w13", "w2"):
        q, sc = (t.cpu() for t in w8.w8_weight(which))
        f32[which] = torch.stack([
            ref.w8_dequant(q[e], sc[e]).t()
            for e in range(q.shape[0])]).to(DEV)            # [E, in, out]
    bf16 = MoEMLP(cfg).to(DEV)
    bf16.gate.data.copy_(gate)
    bf16.w13.data.copy_(f32["w13"])
    bf16.w2.data.copy_(f32["w2"])
    return w8, bf16, f32


def test_layer_holds_the_experts_in_w8_only(moe_layers):
    w8, _, _ = moe_layers
    assert w8.w8 and not w8.w4
    params = dict(w8.named_parameters())
    assert "w13" not in params and "w2" not in params
    assert not hasattr(w8, "w13") and not hasattr(w8, "w2")
    E, I, H = w8.local_experts, w8.inter, w8.hidden
    held = [t for which in ("w13", "w2") for t in w8.w8_weight(which)]
    assert all(t.is_cuda for t in held)
    assert w8.w13_w8.dtype == torch.float8_e4m3fn
    nbytes = sum(t.numel() * t.element_size() for t in held)
    assert nbytes * 128 == E * 3 * I * H * (128 + 4)
    expert_bytes = sum(
        t.numel() * t.element_size()
        for n, t in list(w8.named_buffers()) + list(w8.named_parameters())
        if n.startswith(("w13", "w2")))
    assert expert_bytes == nbytes


@pytest.mark.parametrize("T", [8, 300])
def test_layer_error_within_twice_the_bf16_path(moe_layers, T):
    """||got - ref|| / ||ref|| of the W8 block must not exceed twice that of
    the existing bf16 block run on the same (dequantized) weights and inputs;
    ref is the block evaluated in f32 with the routing both blocks compute.
    Both paths round gu, h, y and the output to bf16 once each; the factor 2
    covers the different reduction order. T = 300 is above DENSE_TOKENS."""
    assert_native()
    w8, bf16, f32 = moe_layers
    assert (T > w8.DENSE_TOKENS) == (T == 300)
    torch.manual_seed(13 + T)
    x = torch.randn(T, w8.hidden, dtype=torch.bfloat16, device=DEV)
    with torch.no_grad():
        got = w8(x).float()
        plain = bf16(x).float()
        weights, sel = ops.moe_topk(F.linear(x, w8.gate).float(), w8.top_k,
                                    w8.norm_topk)
        xf = x.float()
        expect = torch.zeros(T, w8.hidden, device=DEV)
        for j in range(w8.top_k):
            e = sel[:, j].long()
            gu = torch.einsum("th,thn->tn", xf, f32["w13"][e])
            g, u = gu.chunk(2, dim=-1)
            y = torch.einsum("ti,tih->th", F.silu(g) * u, f32["w2"][e])
            expect += weights[:, j, None] * y
    err_w8 = ((got - expect).norm() / expect.norm()).item()
    err_bf16 = ((plain - expect).norm() / expect.norm()).item()
    print(f"T={T}: relative error W8 {err_w8:.3e}, bf16 {err_bf16:.3e}")
    assert torch.isfinite(got).all()
    assert err_w8 <= 2 * err_bf16


# ------------------------------- bindings ----------------------------------
def test_bindings_reject_what_the_kernel_cannot_take():
    assert_native()
    E, T, k = 2, 4, 2
    ids = _distinct_ids(T, k, E, 1).to(DEV)
    counts, pairs = ops.moe_route(ids, 0, E)

    def call(n=64, kk=128, pairs_=pairs, out_rows=T * k, max_rows=T):
        w8 = torch.zeros(E, n, kk, dtype=torch.uint8, device=DEV).view(
            torch.float8_e4m3fn)
        sc = torch.zeros(E, max(kk // 128, 1), n, dtype=torch.float32,
                         device=DEV)
        a = torch.zeros(T, kk, dtype=torch.bfloat16, device=DEV)
        out = torch.zeros(out_rows, n, dtype=torch.bfloat16, device=DEV)
        return ops.w8_moe_gemm(a, (w8, sc), counts, pairs_, k, max_rows,
                               out=out)

    call()  # the valid call goes through
    with pytest.raises(RuntimeError, match="N % 64"):
        call(n=96)
    with pytest.raises(RuntimeError, match="K % 128"):
        call(kk=192)
    with pytest.raises(RuntimeError, match="pairs"):
        call(pairs_=pairs[:1].contiguous())
    with pytest.raises(RuntimeError, match="pairs"):
        call(pairs_=pairs.reshape(-1))
    with pytest.raises(RuntimeError, match="out must be"):
        call(out_rows=T * k - 1)
    with pytest.raises(RuntimeError, match="max_rows"):
        call(max_rows=0)


# ------------------------------- engine ------------------------------------
PROMPTS = [[1, 5, 9, 20, 7, 3], [2, 4, 6], [11, 12, 13, 14]]
SP = SamplingParams(max_tokens=8, ignore_eos=True)


@pytest.fixture(scope="module")
def fp8_dirs(tmp_path_factory):
    from arks_amd.loader.safetensors_loader import save_fp8_checkpoint

    root = tmp_path_factory.mktemp("w8moe")
    dirs = {"fp8": str(root / "fp8"), "bf16": str(root / "bf16")}
    save_fp8_checkpoint(PRESET_CONFIGS["tiny-moe-gpu"], dirs["fp8"], seed=3,
                        dequantized_dir=dirs["bf16"])
    return dirs


def _engine(path, **kw):
    return LLMEngine(EngineConfig(device="cuda", kv_cache_blocks=512,
                                  max_model_len=1024, seed=5, model_path=path,
                                  **kw))


def test_engine_fp8_experts_graph_equals_eager_and_deterministic(fp8_dirs):
    assert_native()
    outs = []
    for eager in (False, True, False):
        e = _engine(fp8_dirs["fp8"], enforce_eager=eager)
        assert e.runner.quantization == "fp8_block"
        moe = e.runner.model.layers[0].mlp
        assert moe.w8 and not moe.w4
        assert moe.w13_w8.is_cuda
        assert moe.w13_w8.dtype == torch.float8_e4m3fn
        params = dict(moe.named_parameters())
        assert "w13" not in params and "w2" not in params
        assert not hasattr(moe, "w13") and not hasattr(moe, "w2")
        outs.append(e.generate(PROMPTS, SP))
        del e
    assert all(len(o) == 8 for o in outs[0])
    assert outs[0] == outs[1] == outs[2]


def test_engine_fp8_experts_batch_70_graph_equals_eager(fp8_dirs):
    """70 sequences pad to the 96-row graph: max_rows = 96 gives two slabs
    per expert and the two-sub-tile kernel."""
    assert_native()
    prompts = [[(7 * i + j) % 2000 + 1 for j in range(3 + i % 4)]
               for i in range(70)]
    sp = SamplingParams(max_tokens=4, ignore_eos=True)
    outs = []
    for eager in (False, True):
        e = _engine(fp8_dirs["fp8"], enforce_eager=eager)
        outs.append(e.generate(prompts, sp))
        del e
    assert all(len(o) == 4 for o in outs[0])
    assert outs[0] == outs[1]


def test_engine_fp8_experts_with_fp8_kv_cache_is_deterministic(fp8_dirs):
    assert_native()
    outs = []
    for _ in range(2):
        e = _engine(fp8_dirs["fp8"], kv_cache_dtype="fp8")
        assert e.runner.model.layers[0].mlp.w8
        outs.append(e.generate(PROMPTS, SP))
        del e
    assert all(len(o) == 8 for o in outs[0])
    assert outs[0] == outs[1]


def test_engine_fp8_moe_checkpoint_agrees_with_dequantized_bf16(fp8_dirs):
    """The project's rule for a quantized engine against the bf16 engine on
    the dequantized weights (tests/test_w4_gpu.py): the two hold the same
    weights but reduce in different orders, so greedy tokens must agree on at
    least half of the generated positions."""
    assert_native()
    e = _engine(fp8_dirs["fp8"])
    assert e.runner.model.layers[0].mlp.w8
    a = e.generate(PROMPTS, SP)
    del e
    e = _engine(fp8_dirs["bf16"])
    assert not e.runner.model.layers[0].mlp.w8
    b = e.generate(PROMPTS, SP)
    del e
    total = sum(len(o) for o in a)
    same = sum(x == y for oa, ob in zip(a, b) for x, y in zip(oa, ob))
    print(f"MoE fp8 vs dequantized-bf16 token agreement: {same}/{total}")
    assert total == 8 * len(PROMPTS)
    assert same * 2 >= total
