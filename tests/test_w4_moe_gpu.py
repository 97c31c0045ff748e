"""W4 MoE experts on the GPU: moe_route_kernel, w4_moe_gemm_kernel, the W4
MoEMLP forward and the engine modes that use them.

References: ops.ref.moe_route for the table, the f32 product with the
dequantized weights (ops.ref.w4_dequant) for the GEMM, an f32 evaluation of
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


def _random_experts(E, n, k, seed, pow2_scales=False):
    """(stacked packed triple on the GPU, f32 dequantized [E, n, k] on the
    CPU)."""
    qzs = [_random_w4(n, k, seed + e, pow2_scales) for e in range(E)]
    packs = [ref.w4_pack(*t) for t in qzs]
    packed = tuple(torch.stack([p[i] for p in packs]).to(DEV)
                   for i in range(3))
    return packed, torch.stack([ref.w4_dequant(*t) for t in qzs])


def _distinct_ids(T, k, E, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(T, E, generator=g).topk(k, dim=-1).indices.to(
        torch.int32)


# ------------------------------ exact mapping ------------------------------
@pytest.mark.parametrize("src_div", [2, 1])
def test_exact_mapping_and_untouched_rows(src_div):
    """One-hot activations and power-of-two scales make every step exact, so
    each written row must be one column of its expert's dequantized weight,
    bit for bit. The three local experts get 0, 17 and 65 rows (an empty
    list, a partial tile, a second slab of one row); the pairs of a fourth,
    non-local expert must keep the sentinel `out` was filled with."""
    assert_native()
    E, N, K, k, T = 3, 128, 256, 2, 65
    base = 1  # local experts are global ids 1, 2, 3; id 0 is another rank's
    ids = torch.empty(T, k, dtype=torch.int32)
    for t in range(T):
        other = 2 if t < 17 else 0
        ids[t] = torch.tensor([3, other] if t % 2 else [other, 3])
    counts, pairs = ref.moe_route(ids, base, E)
    assert counts.tolist() == [0, 17, 65]
    packed, wd = _random_experts(E, N, K, 3, pow2_scales=True)

    n_pairs = T * k
    rows_a = T if src_div == k else n_pairs
    cols = (7 * torch.arange(rows_a) + 1) % K
    a = torch.zeros(rows_a, K, dtype=torch.bfloat16)
    a[torch.arange(rows_a), cols] = 1.0
    out = torch.full((n_pairs, N), -3.0, dtype=torch.bfloat16, device=DEV)
    got = ops.w4_moe_gemm(a.to(DEV), packed, counts.to(DEV), pairs.to(DEV),
                          src_div, T, out=out)
    assert got is out
    out = out.cpu().float()
    flat = ids.reshape(-1)
    for p in range(n_pairs):
        le = int(flat[p]) - base
        if le < 0:
            assert (out[p] == -3.0).all(), p
        else:
            assert torch.equal(out[p], wd[le][:, cols[p // src_div]]), p


# ------------------------------ routing table ------------------------------
@pytest.mark.parametrize("T", [1, 5, 64, 200])
@pytest.mark.parametrize("k", [2, 8])
@pytest.mark.parametrize("E", [4, 128])
def test_route_table_equals_reference(T, k, E):
    """expert_base > 0 and n_local < E, so ids of other ranks' experts are
    present. k = 8 of E = 4 cannot be distinct experts: those ids are drawn
    with repeats, which also drives an expert past T matches, where kernel
    and reference both keep the first T."""
    assert_native()
    if k <= E:
        ids = _distinct_ids(T, k, E, 100 * T + k)
    else:
        g = torch.Generator().manual_seed(100 * T + k)
        ids = torch.randint(0, E, (T, k), generator=g, dtype=torch.int32)
    base, n_local = (1, 2) if E == 4 else (32, 64)
    counts, pairs = ops.moe_route(ids.to(DEV), base, n_local)
    assert counts.shape == (n_local,) and counts.dtype == torch.int32
    assert pairs.shape == (n_local, T) and pairs.dtype == torch.int32
    rc, rp = ref.moe_route(ids, base, n_local)
    counts, pairs = counts.cpu(), pairs.cpu()
    assert torch.equal(counts, rc)
    for e in range(n_local):
        c = int(counts[e])
        assert 0 <= c <= T
        assert torch.equal(pairs[e, :c], rp[e, :c]), e
        assert (torch.diff(pairs[e, :c]) > 0).all()  # ascending
    local = (ids >= base) & (ids < base + n_local)
    if k <= E:
        assert int(counts.sum()) == int(local.sum())


# ------------------------------- numerics ----------------------------------
@pytest.mark.parametrize("T", [1, 16, 70])
@pytest.mark.parametrize("n,k_dim", [(64, 128), (512, 512), (512, 256)])
def test_numerics(T, n, k_dim):
    """Against the f32 product with the dequantized weights, at the
    tolerance tests/test_w4_gpu.py uses for w4_linear with the same weight
    and activation scales."""
    assert_native()
    E, k = 4, 2
    packed, wd = _random_experts(E, n, k_dim, 5)
    ids = _distinct_ids(T, k, E, 31 + T)
    counts, pairs = ops.moe_route(ids.to(DEV), 0, E)
    flat = ids.reshape(-1).long()
    torch.manual_seed(7)
    for src_div in (k, 1):
        rows_a = T * k // src_div
        a = (torch.randn(rows_a, k_dim) * 0.5).to(torch.bfloat16)
        src = torch.arange(T * k) // src_div
        expect = torch.einsum("pk,pnk->pn", a[src].float(), wd[flat])
        out = ops.w4_moe_gemm(a.to(DEV), packed, counts, pairs, src_div, T)
        assert out.shape == (T * k, n) and out.dtype == torch.bfloat16
        torch.testing.assert_close(out.cpu().float(), expect, atol=5e-2,
                                   rtol=5e-2)


# ------------------------------ layer level --------------------------------
@pytest.fixture(scope="module")
def moe_layers():
    """(W4 block, bf16 block holding the same dequantized weights, their f32
    dequantized weights) of the tiny-moe-gpu shape."""
    from arks_amd.models.llama_family import MoEMLP

    cfg = PRESET_CONFIGS["tiny-moe-gpu"]
    torch.manual_seed(11)
    w4 = MoEMLP(cfg).to(DEV)
    w4.gate.data.normal_(0, 0.5)
    w4.w13.data.normal_(0, 0.05)
    w4.w2.data.normal_(0, 0.05)
    gate = w4.gate.data.clone()
    w4.quantize_w4("test")
    assert w4.w4 and "w13" not in dict(w4.named_parameters())
    f32 = {}
    for which in ("w13", "w2"):
        qw, sc, zr = (t.cpu() for t in w4.w4_packed(which))
        f32[which] = torch.stack([
            ref.w4_dequant(*ref.w4_unpack((qw[e], sc[e], zr[e]))).t()
            for e in range(qw.shape[0])]).to(DEV)       # [E, in, out]
    bf16 = MoEMLP(cfg).to(DEV)
    bf16.gate.data.copy_(gate)
    bf16.w13.data.copy_(f32["w13"])
    bf16.w2.data.copy_(f32["w2"])
    return w4, bf16, f32


@pytest.mark.parametrize("T", [8, 300])
def test_layer_error_within_twice_the_bf16_path(moe_layers, T):
    """||got - ref|| / ||ref|| of the W4 block must not exceed twice that of
    the existing bf16 block run on the same (dequantized) weights and inputs;
    ref is the block evaluated in f32 with the routing both blocks compute.
    Both paths round gu, h, y and the output to bf16 once each; the factor 2
    covers the different reduction order. T = 300 is above DENSE_TOKENS."""
    assert_native()
    w4, bf16, f32 = moe_layers
    assert (T > w4.DENSE_TOKENS) == (T == 300)
    torch.manual_seed(13 + T)
    x = torch.randn(T, w4.hidden, dtype=torch.bfloat16, device=DEV)
    with torch.no_grad():
        got = w4(x).float()
        plain = bf16(x).float()
        weights, sel = ops.moe_topk(F.linear(x, w4.gate).float(), w4.top_k,
                                    w4.norm_topk)
        xf = x.float()
        expect = torch.zeros(T, w4.hidden, device=DEV)
        for j in range(w4.top_k):
            e = sel[:, j].long()
            gu = torch.einsum("th,thn->tn", xf, f32["w13"][e])
            g, u = gu.chunk(2, dim=-1)
            y = torch.einsum("ti,tih->th", F.silu(g) * u, f32["w2"][e])
            expect += weights[:, j, None] * y
    err_w4 = ((got - expect).norm() / expect.norm()).item()
    err_bf16 = ((plain - expect).norm() / expect.norm()).item()
    print(f"T={T}: relative error W4 {err_w4:.3e}, bf16 {err_bf16:.3e}")
    assert torch.isfinite(got).all()
    assert err_w4 <= 2 * err_bf16


# ------------------------------- bindings ----------------------------------
def test_bindings_reject_what_the_kernel_cannot_take():
    assert_native()
    E, T, k = 2, 4, 2
    ids = _distinct_ids(T, k, E, 1).to(DEV)
    counts, pairs = ops.moe_route(ids, 0, E)

    def call(n=64, kk=128, pairs_=pairs, out_rows=T * k):
        qw = torch.zeros(E, n, kk // 8, dtype=torch.int32, device=DEV)
        sc = torch.zeros(E, max(kk // 128, 1), n, dtype=torch.float16,
                         device=DEV)
        zr = torch.zeros(E, max(kk // 128, 1), n, dtype=torch.uint8,
                         device=DEV)
        a = torch.zeros(T, kk, dtype=torch.bfloat16, device=DEV)
        out = torch.zeros(out_rows, n, dtype=torch.bfloat16, device=DEV)
        return ops.w4_moe_gemm(a, (qw, sc, zr), counts, pairs_, k, T, out=out)

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
        ops.w4_moe_gemm(
            torch.zeros(T, 128, dtype=torch.bfloat16, device=DEV),
            (torch.zeros(E, 64, 16, dtype=torch.int32, device=DEV),
             torch.zeros(E, 1, 64, dtype=torch.float16, device=DEV),
             torch.zeros(E, 1, 64, dtype=torch.uint8, device=DEV)),
            counts, pairs, k, 0)


# ------------------------------- engine ------------------------------------
PROMPTS = [[1, 5, 9, 20, 7, 3], [2, 4, 6], [11, 12, 13, 14]]
SP = SamplingParams(max_tokens=8, ignore_eos=True)


def _engine(**kw):
    kw.setdefault("preset", "tiny-moe-gpu")
    if kw.get("model_path"):
        kw.pop("preset")
    return LLMEngine(EngineConfig(device="cuda", kv_cache_blocks=512,
                                  max_model_len=1024, seed=5, **kw))


def test_engine_int4_experts_graph_equals_eager_and_deterministic():
    assert_native()
    outs = []
    for eager in (False, True, False):
        e = _engine(quantization="int4", quantize_experts=True,
                    enforce_eager=eager)
        moe = e.runner.model.layers[0].mlp
        assert moe.w4 and moe.w13_qweight.is_cuda
        params = dict(moe.named_parameters())
        assert "w13" not in params and "w2" not in params
        assert not hasattr(moe, "w13")
        outs.append(e.generate(PROMPTS, SP))
        del e
    assert all(len(o) == 8 for o in outs[0])
    assert outs[0] == outs[1] == outs[2]


def test_engine_int4_experts_batch_70_graph_equals_eager():
    """70 sequences pad to the 96-row graph: max_rows = 96 gives two slabs
    per expert and the two-sub-tile kernel."""
    assert_native()
    prompts = [[(7 * i + j) % 2000 + 1 for j in range(3 + i % 4)]
               for i in range(70)]
    sp = SamplingParams(max_tokens=4, ignore_eos=True)
    outs = []
    for eager in (False, True):
        e = _engine(quantization="int4", quantize_experts=True,
                    enforce_eager=eager)
        outs.append(e.generate(prompts, sp))
        del e
    assert all(len(o) == 4 for o in outs[0])
    assert outs[0] == outs[1]


def test_qwen3_moe_single_sequence_decodes(tmp_path):
    """Batch-1 decode of a qk-norm MoE model (the shape class of the
    qwen3-30b-a3b measurements): v's one-row view of the fused qkv buffer
    must reach the cache kernel with k's row stride. Graph == eager."""
    assert_native()
    import dataclasses

    from arks_amd.loader.safetensors_loader import save_random_checkpoint

    cfg = dataclasses.replace(PRESET_CONFIGS["tiny-moe-gpu"],
                              architecture="Qwen3MoeForCausalLM",
                              qk_norm=True)
    path = str(tmp_path / "q3moe")
    save_random_checkpoint(cfg, path, seed=9)
    outs = []
    for eager in (False, True):
        e = _engine(model_path=path, enforce_eager=eager)
        assert e.model_cfg.qk_norm and e.model_cfg.num_local_experts == 4
        outs.append(e.generate(PROMPTS[:1], SP))
        del e
    assert len(outs[0][0]) == 8 and outs[0] == outs[1]


def test_engine_moe_awq_checkpoint_agrees_with_dequantized_bf16(tmp_path):
    """The rule and reasoning of tests/test_w4_gpu.py's
    test_engine_awq_checkpoint_agrees_with_dequantized_bf16: the two engines
    hold the same weights but reduce in different orders, so greedy tokens
    must agree on at least half of the generated positions."""
    assert_native()
    from arks_amd.loader.safetensors_loader import save_awq_checkpoint

    awq_dir, bf16_dir = str(tmp_path / "awq"), str(tmp_path / "bf16")
    save_awq_checkpoint(PRESET_CONFIGS["tiny-moe-gpu"], awq_dir, seed=3,
                        dequantized_dir=bf16_dir)
    e = _engine(model_path=awq_dir)
    assert e.runner.quantization == "awq"
    assert e.runner.model.layers[0].mlp.w4
    a = e.generate(PROMPTS, SP)
    del e
    e = _engine(model_path=bf16_dir)
    assert not e.runner.model.layers[0].mlp.w4
    b = e.generate(PROMPTS, SP)
    del e
    total = sum(len(o) for o in a)
    same = sum(x == y for oa, ob in zip(a, b) for x, y in zip(oa, ob))
    print(f"MoE awq vs dequantized-bf16 token agreement: {same}/{total}")
    assert total == 8 * len(PROMPTS)
    assert same * 2 >= total
