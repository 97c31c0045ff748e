"""Routed bf16 MoE experts on the GPU: moe_bf16_gemm_kernel, the routed bf16
MoEMLP forward and the engine on a bf16 MoE checkpoint.

References: ops.ref.moe_route for the table, an f64 einsum for the GEMM, an
f32 evaluation of the block against the library paths for the layer, and the
eager engine for the captured one."""

import pytest
import torch
import torch.nn.functional as F

import arks_amd.ops as ops
from arks_amd.config import PRESET_CONFIGS, EngineConfig
from arks_amd.engine import LLMEngine, SamplingParams
from arks_amd.ops import ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
SLAB = 64  # list rows per workgroup (moe_gemm.hip MG_SLAB)


def assert_native():
    assert ops.native_available(), "HIP extension must be built on a GPU box"


def _distinct_ids(T, k, E, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(T, E, generator=g).topk(k, dim=-1).indices.to(
        torch.int32)


# ------------------------------ exact mapping ------------------------------
@pytest.mark.parametrize("n", [128, 256])
@pytest.mark.parametrize("src_div", [2, 1])
def test_exact_mapping_and_untouched_rows(src_div, n):
    """One-hot activations make every step exact, so each written row must be
    one row of ITS expert's weight, bit for bit: a wrong expert offset, a
    wrong image mapping (k and n swapped or permuted inside a fragment), a
    wrong gather or scatter shows. The three local experts get 0, 17 and 65
    rows (an empty list, a partial tile pair, a second slab of one row); the
    pairs of a fourth, non-local expert keep the sentinel `out` held."""
    assert_native()
    E, K, k, T = 3, 256, 2, SLAB + 1
    base = 1  # local experts are global ids 1, 2, 3; id 0 is another rank's
    ids = torch.empty(T, k, dtype=torch.int32)
    for t in range(T):
        other = 2 if t < 17 else 0
        ids[t] = torch.tensor([3, other] if t % 2 else [other, 3])
    counts, pairs = ref.moe_route(ids, base, E)
    assert counts.tolist() == [0, 17, SLAB + 1]
    g = torch.Generator().manual_seed(3 + n)
    w = torch.randn(E, K, n, generator=g).to(torch.bfloat16)

    n_pairs = T * k
    rows_a = T if src_div == k else n_pairs
    cols = (7 * torch.arange(rows_a) + 1) % K
    a = torch.zeros(rows_a, K, dtype=torch.bfloat16)
    a[torch.arange(rows_a), cols] = 1.0
    out = torch.full((n_pairs, n), -3.0, dtype=torch.bfloat16, device=DEV)
    got = ops.moe_bf16_gemm(a.to(DEV), w.to(DEV), counts.to(DEV),
                            pairs.to(DEV), src_div, T, out=out)
    assert got is out
    out = out.cpu()
    flat = ids.reshape(-1)
    for p in range(n_pairs):
        le = int(flat[p]) - base
        if le < 0:
            assert (out[p] == -3.0).all(), p
        else:
            assert torch.equal(out[p], w[le][cols[p // src_div]]), p


# ------------------------------- numerics ----------------------------------
def _gemm_case(T, n, k_dim, src_div, E=4, k=2):
    """(a, w, ids) on the CPU, seeded by the shape."""
    g = torch.Generator().manual_seed(1000 * n + k_dim + T + src_div)
    w = (torch.randn(E, k_dim, n, generator=g) * 0.05).to(torch.bfloat16)
    a = (torch.randn(T * k // src_div, k_dim, generator=g) * 0.5).to(
        torch.bfloat16)
    return a, w, _distinct_ids(T, k, E, 31 + T)


@pytest.mark.parametrize("T", [1, 16, SLAB + 6])
@pytest.mark.parametrize("n,k_dim", [(128, 64), (256, 512), (384, 192)])
def test_numerics(T, n, k_dim):
    """Against an f64 einsum. The only rounding is one bf16 RNE (2^-9
    relative); f32 accumulation over K <= 512 of terms this size stays below
    1e-5: rtol = 2^-7 is four times the rounding bound, atol = 1e-3."""
    assert_native()
    k = 2
    for src_div in (k, 1):
        a, w, ids = _gemm_case(T, n, k_dim, src_div)
        counts, pairs = ops.moe_route(ids.to(DEV), 0, w.shape[0])
        src = torch.arange(T * k) // src_div
        expect = torch.einsum("pk,pkn->pn", a[src].double(),
                              w[ids.reshape(-1).long()].double())
        out = ops.moe_bf16_gemm(a.to(DEV), w.to(DEV), counts, pairs, src_div,
                                T)
        assert out.shape == (T * k, n) and out.dtype == torch.bfloat16
        torch.testing.assert_close(out.cpu().double(), expect, atol=1e-3,
                                   rtol=2 ** -7)


def test_row_results_do_not_depend_on_the_batch():
    """Token 0 inside a batch of SLAB + 6 and alone (T = 1, max_rows = 1):
    its k output rows must be bit-identical, whatever slab, tile count and
    list position they had in the batch."""
    assert_native()
    T, n, k_dim, k = SLAB + 6, 256, 512, 2
    a, w, ids = _gemm_case(T, n, k_dim, k)
    a, w = a.to(DEV), w.to(DEV)
    counts, pairs = ops.moe_route(ids.to(DEV), 0, w.shape[0])
    batch = ops.moe_bf16_gemm(a, w, counts, pairs, k, T)
    counts1, pairs1 = ops.moe_route(ids[:1].to(DEV), 0, w.shape[0])
    alone = ops.moe_bf16_gemm(a[:1], w, counts1, pairs1, k, 1)
    assert alone.shape == (k, n)
    assert torch.equal(alone, batch[:k])


# ------------------------------ layer level --------------------------------
@pytest.mark.parametrize("T", [8, 300])
def test_layer_error_within_twice_the_library_path(T):
    """||got - ref|| / ||ref|| of the routed block must not exceed twice that
    of the library path on the same module and input (the dense bmm for
    T = 8, the sparse path for T = 300); ref is the block evaluated in f32
    with the routing the block computes. Both round gu, h, y and the output
    to bf16 once each; the factor 2 covers the different reduction order."""
    assert_native()
    from arks_amd.models.llama_family import MoEMLP

    torch.manual_seed(11)
    moe = MoEMLP(PRESET_CONFIGS["tiny-moe-gpu"]).to(DEV)
    moe.gate.data.normal_(0, 0.5)
    moe.w13.data.normal_(0, 0.05)
    moe.w2.data.normal_(0, 0.05)
    assert moe.bf16_routed_supported()
    torch.manual_seed(13 + T)
    x = torch.randn(T, moe.hidden, dtype=torch.bfloat16, device=DEV)
    with torch.no_grad():
        got = moe._forward_routed(x, ops.moe_bf16_gemm, moe.w13,
                                  moe.w2).float()
        weights, sel = ops.moe_topk(F.linear(x, moe.gate).float(), moe.top_k,
                                    moe.norm_topk)
        parent = (moe._forward_bmm if T <= moe.DENSE_TOKENS
                  else moe._forward_sparse)(x, weights, sel).float()
        xf, w13, w2 = x.float(), moe.w13.float(), moe.w2.float()
        expect = torch.zeros(T, moe.hidden, device=DEV)
        for j in range(moe.top_k):
            e = sel[:, j].long()
            g, u = torch.einsum("th,thn->tn", xf, w13[e]).chunk(2, dim=-1)
            y = torch.einsum("ti,tih->th", F.silu(g) * u, w2[e])
            expect += weights[:, j, None] * y
    err = ((got - expect).norm() / expect.norm()).item()
    err_parent = ((parent - expect).norm() / expect.norm()).item()
    print(f"T={T}: relative error routed {err:.3e}, library {err_parent:.3e}")
    assert torch.isfinite(got).all()
    assert err <= 2 * err_parent


# ------------------------------- bindings ----------------------------------
def test_bindings_reject_what_the_kernel_cannot_take():
    assert_native()
    E, T, k = 2, 4, 2
    ids = _distinct_ids(T, k, E, 1).to(DEV)
    counts, pairs = ops.moe_route(ids, 0, E)

    def call(n=128, kk=64, pairs_=pairs, out_rows=T * k, max_rows=T):
        w = torch.zeros(E, kk, n, dtype=torch.bfloat16, device=DEV)
        a = torch.zeros(T, kk, dtype=torch.bfloat16, device=DEV)
        out = torch.zeros(out_rows, n, dtype=torch.bfloat16, device=DEV)
        return ops.moe_bf16_gemm(a, w, counts, pairs_, k, max_rows, out=out)

    call()  # the valid call goes through
    with pytest.raises(RuntimeError, match="N % 128"):
        call(n=192)
    with pytest.raises(RuntimeError, match="K % 64"):
        call(kk=96)
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


@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    from arks_amd.loader.safetensors_loader import save_random_checkpoint

    path = str(tmp_path_factory.mktemp("moebf16") / "ckpt")
    save_random_checkpoint(PRESET_CONFIGS["tiny-moe-gpu"], path, seed=3)
    return path


def _generate(path, prompts, max_tokens, eager):
    e = LLMEngine(EngineConfig(device="cuda", kv_cache_blocks=512,
                               max_model_len=1024, seed=5, model_path=path,
                               enforce_eager=eager))
    moe = e.runner.model.layers[0].mlp
    assert not moe.w4 and not moe.w8 and moe.routed_bf16_calls == 0
    out = e.generate(prompts, SamplingParams(max_tokens=max_tokens,
                                             ignore_eos=True))
    assert moe.routed_bf16_calls > 0  # the block took the routed path
    return out


def test_engine_bf16_experts_graph_equals_eager_and_deterministic(ckpt):
    assert_native()
    outs = [_generate(ckpt, PROMPTS, 8, eager)
            for eager in (False, True, False)]
    assert all(len(o) == 8 for o in outs[0])
    assert outs[0] == outs[1] == outs[2]


def test_engine_bf16_experts_batch_70_graph_equals_eager(ckpt):
    """70 sequences pad to the 96-row graph: max_rows = 96 gives two slabs
    per expert."""
    assert_native()
    prompts = [[(7 * i + j) % 2000 + 1 for j in range(3 + i % 4)]
               for i in range(70)]
    outs = [_generate(ckpt, prompts, 4, eager) for eager in (False, True)]
    assert all(len(o) == 4 for o in outs[0])
    assert outs[0] == outs[1]
