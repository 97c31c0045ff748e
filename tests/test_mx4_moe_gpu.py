"""MX4 MoE experts on the GPU: mx4_moe_gemm_kernel ("stream", W4A16),
mx4_moe_mfma_gemm_kernel ("mfma", W4A4), the MX4 MoEMLP forward and the engine
on an MXFP4 MoE checkpoint. GEMM tolerance as tests/test_mx4a4_gpu.py derives
it: exact products, K of them summed in f32, one rounding to bf16, so
|y - ref| <= 2^-8 |y| + K 2^-23 (|x^| @ |w^|^T)."""

import functools

import pytest
import torch
import torch.nn.functional as F

import arks_amd.ops as ops
from arks_amd.config import PRESET_CONFIGS, EngineConfig
from arks_amd.engine import LLMEngine, SamplingParams
from arks_amd.ops import ref

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _gemm(kernel, a, weight, counts, pairs, src_div, max_rows, out=None,
          mtile=None):
    """-> (out, the f32 activations the kernel multiplies): `a` itself, or
    for "mfma" its ref.mx4_quantize codes."""
    args = (tuple(t.to(DEV) for t in weight), counts.to(DEV), pairs.to(DEV),
            src_div, max_rows)
    if kernel == "stream":
        return ops.mx4_moe_gemm(a.to(DEV), *args, out=out), a.float()
    xq, xs = ref.mx4_quantize(a)
    got = ops.mx4a4_moe_gemm(xq.to(DEV), xs.to(DEV), *args, out=out,
                             mtile=mtile)
    return got, ref.mx4_dequant(xq, xs)


@pytest.mark.parametrize("src_div", [2, 1])
@pytest.mark.parametrize("kernel,K,n,T,mtile", [
    ("stream", 256, 64, 65, None), ("stream", 256, 128, 65, None),
    ("mfma", 640, 192, 130, 64), ("mfma", 640, 192, 130, 128)])
def test_exact_mapping_and_untouched_rows(kernel, K, n, T, mtile, src_div):
    """One-hot activations of 1.0 (exact in MXFP4): a written row is one
    column of ITS expert's dequantized weight, bit for bit. Lists of 0, 17
    and T rows: empty, partial tile, further slabs of one or two rows. K =
    640: quarter super-chunk; N = 192: a wave past N."""
    assert ops.native_available()
    E, k, base = 3, 2, 1   # local experts are global ids 1, 2, 3
    ids = torch.empty(T, k, dtype=torch.int32)
    for t in range(T):
        other = 2 if t < 17 else 0
        ids[t] = torch.tensor([3, other] if t % 2 else [other, 3])
    counts, pairs = ref.moe_route(ids, base, E)
    assert counts.tolist() == [0, 17, T]
    g = torch.Generator().manual_seed(3 + n)
    codes = torch.arange(16).repeat(E * n * K // 16)[
        torch.randperm(E * n * K, generator=g)].to(torch.uint8).view(E, n, K)
    w = codes[..., 0::2] | (codes[..., 1::2] << 4)
    scales = torch.randint(120, 135, (E, n, K // 32), generator=g).to(
        torch.uint8)
    assert all(len(codes[e].unique()) == 16 for e in range(E))
    wd = torch.stack([ref.mx4_dequant(w[e], scales[e]) for e in range(E)])

    rows_a = T * k // src_div
    cols = (7 * torch.arange(rows_a) + 1) % K
    a = torch.zeros(rows_a, K, dtype=torch.bfloat16)
    a[torch.arange(rows_a), cols] = 1.0
    out = torch.full((T * k, n), -3.0, dtype=torch.bfloat16, device=DEV)
    got, _ = _gemm(kernel, a, (w, scales), counts, pairs, src_div, T, out=out,
                   mtile=mtile)
    assert got is out
    out = out.cpu().float()
    for p, gid in enumerate(ids.reshape(-1).tolist()):
        if gid < base:
            assert (out[p] == -3.0).all(), p
        else:
            assert torch.equal(out[p],
                               wd[gid - base][:, cols[p // src_div]]), p


def _blocks(rows, k, seed):
    """bf16 [rows, k]: noise times 2^-6 .. 2^6 drawn per MX block."""
    g = torch.Generator().manual_seed(seed)
    mag = torch.randint(-6, 7, (rows, k // 32, 1), generator=g).float()
    x = torch.randn(rows, k // 32, 32, generator=g) * torch.exp2(mag)
    return x.view(rows, k).to(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def _experts(E, n, k):
    qs = [ref.mx4_quantize(_blocks(n, k, 5 + e + n + k)) for e in range(E)]
    weight = tuple(torch.stack(t) for t in zip(*qs))
    return weight, torch.stack([ref.mx4_dequant(*q) for q in qs]).double()


@pytest.mark.parametrize("kernel,T,n,k_dim,mtile", [
    *[("stream", T, n, kd, None) for T in (1, 16, 70)
      for n, kd in ((64, 128), (512, 512))],
    *[("mfma", T, n, kd, mt) for T in (70, 300)
      for n, kd in ((192, 640), (256, 1024)) for mt in (64, 128)]])
def test_numerics_against_float64(kernel, T, n, k_dim, mtile):
    assert ops.native_available()
    E, k = 4, 2
    weight, wd = _experts(E, n, k_dim)
    g = torch.Generator().manual_seed(31 + T)
    ids = torch.rand(T, E, generator=g).topk(k, dim=-1).indices.to(
        torch.int32)
    counts, pairs = ref.moe_route(ids, 0, E)
    flat = ids.reshape(-1).long()
    for src_div in (k, 1):
        a = _blocks(T * k // src_div, k_dim, 7 * T + src_div)
        out, xhat = _gemm(kernel, a, weight, counts, pairs, src_div, T,
                          mtile=mtile)
        assert out.shape == (T * k, n) and out.dtype == torch.bfloat16
        xd = xhat.double()[torch.arange(T * k) // src_div]
        y = torch.einsum("pk,pnk->pn", xd, wd[flat])
        acc = k_dim * 2.0 ** -23 * torch.einsum("pk,pnk->pn", xd.abs(),
                                                wd[flat].abs())
        err = (out.double().cpu() - y).abs()
        tol = 2.0 ** -8 * y.abs() + acc
        assert (err <= tol).all(), (err - tol).max().item()


@pytest.fixture(scope="module")
def moe_layers():
    """(MX4 block, bf16 block on the same dequantized weights, those in f32
    [E, in, out]) of the tiny-moe-gpu shape; the MX4 block holds no bf16
    expert and exactly E*3*I*H*(1/2 + 1/32) expert bytes."""
    from arks_amd.models.llama_family import MoEMLP

    cfg = PRESET_CONFIGS["tiny-moe-gpu"]
    torch.manual_seed(11)
    mx4 = MoEMLP(cfg).to(DEV)
    mx4.gate.data.normal_(0, 0.5)
    mx4.w13.data.normal_(0, 0.05)
    mx4.w2.data.normal_(0, 0.05)
    bf16 = MoEMLP(cfg).to(DEV)
    bf16.gate.data.copy_(mx4.gate.data)
    mx4.quantize_mx4("test")
    f32 = {}
    for which in ("w13", "w2"):
        q, sc = (t.cpu() for t in mx4.mx4_weight(which))
        f32[which] = torch.stack([ref.mx4_dequant(q[e], sc[e]).t()
                                  for e in range(q.shape[0])]).to(DEV)
        getattr(bf16, which).data.copy_(f32[which])
    assert mx4.mx4 and not hasattr(mx4, "w13") and not hasattr(mx4, "w2")
    E, I, H = mx4.local_experts, mx4.inter, mx4.hidden
    held = [t for n, t in (*mx4.named_buffers(), *mx4.named_parameters())
            if n.startswith(("w13", "w2"))]
    assert all(t.is_cuda and t.dtype == torch.uint8 for t in held)
    assert sum(t.numel() for t in held) * 32 == E * 3 * I * H * (16 + 1)
    return mx4, bf16, f32


def _f32_block(layer, f32, x, qdq):
    """The block in f32 with the layer's routing. qdq: both GEMMs take
    ref.mx4_qdq of their input, h as the bf16 tensor the block holds: the
    quantizer turns a 2^-9 rounding of h into a whole e2m1 step, so an
    unrounded h would measure those flips, not the kernels."""
    weights, sel = ops.moe_topk(F.linear(x, layer.gate).float(), layer.top_k,
                                layer.norm_topk)
    xf = ref.mx4_qdq(x).float() if qdq else x.float()
    expect = torch.zeros(x.shape[0], layer.hidden, device=DEV)
    for j in range(layer.top_k):
        e = sel[:, j].long()
        gu = torch.einsum("th,thn->tn", xf, f32["w13"][e])
        if qdq:
            g, u = gu.to(torch.bfloat16).float().chunk(2, dim=-1)
            h = ref.mx4_qdq((F.silu(g) * u).to(torch.bfloat16)).float()
        else:
            g, u = gu.chunk(2, dim=-1)
            h = F.silu(g) * u
        expect += weights[:, j, None] * torch.einsum("ti,tih->th", h,
                                                     f32["w2"][e])
    return expect


@pytest.mark.parametrize("mode,T", [("bf16", 8), ("bf16", 300), ("mxfp4", 8),
                                    ("mxfp4", 256), ("mxfp4", 257),
                                    ("mxfp4", 300)])
def test_layer_error_within_twice_the_bf16_path(moe_layers, mode, T):
    """The W8 test's rule (both blocks round gu, h, y and the output once; 2
    covers the reduction order). 256 / 257: both sides of MX4A4_MFMA_TOKENS."""
    assert ops.native_available()
    mx4, bf16, f32 = moe_layers
    assert mx4.MX4A4_MFMA_TOKENS == mx4.DENSE_TOKENS == 256
    torch.manual_seed(13 + T)
    x = torch.randn(T, mx4.hidden, dtype=torch.bfloat16, device=DEV)
    mx4.mx4_act = mode
    try:
        with torch.no_grad():
            got = mx4(x).float()
            plain = bf16(x).float()
            expect = _f32_block(mx4, f32, x, mode == "mxfp4")
            expect_bf16 = _f32_block(mx4, f32, x, False)
    finally:
        mx4.mx4_act = "bf16"
    err_mx4 = ((got - expect).norm() / expect.norm()).item()
    err_bf16 = ((plain - expect_bf16).norm() / expect_bf16.norm()).item()
    print(f"{mode} T={T}: relative error MX4 {err_mx4:.3e}, "
          f"bf16 {err_bf16:.3e}")
    assert torch.isfinite(got).all()
    assert err_mx4 <= 2 * err_bf16


@pytest.mark.parametrize("kernel", ["stream", "mfma"])
def test_bindings_reject_what_the_kernel_cannot_take(kernel):
    assert ops.native_available()
    E, T, k = 2, 4, 2
    ids = torch.rand(T, E).topk(k, dim=-1).indices.to(torch.int32).to(DEV)
    counts, pairs = ops.moe_route(ids, 0, E)

    def call(n=64, kk=128, pairs_=pairs, out_rows=T * k, max_rows=T):
        def z(*shape, dt=torch.uint8):
            return torch.zeros(*shape, dtype=dt, device=DEV)

        args = ((z(E, n, kk // 2), z(E, n, kk // 32)), counts, pairs_, k,
                max_rows)
        out = z(out_rows, n, dt=torch.bfloat16)
        if kernel == "stream":
            return ops.mx4_moe_gemm(z(T, kk, dt=torch.bfloat16), *args,
                                    out=out)
        return ops.mx4a4_moe_gemm(z(T, kk // 2), z(T, kk // 32), *args,
                                  out=out)

    assert (call().float() == 0).all()  # the valid call goes through
    for match, kw in (("N % 64", {"n": 96}), ("K % 128", {"kk": 192}),
                      ("pairs", {"pairs_": pairs[:1].contiguous()}),
                      ("pairs", {"pairs_": pairs.reshape(-1)}),
                      ("out must be", {"out_rows": T * k - 1}),
                      ("max_rows", {"max_rows": 0})):
        with pytest.raises(RuntimeError, match=match):
            call(**kw)


LONG = [(7 * i) % 2000 + 1 for i in range(300)]   # prefill > DENSE_TOKENS
PROMPTS = [[1, 5, 9, 20, 7, 3], [2, 4, 6], [11, 12, 13, 14]]
SP = SamplingParams(max_tokens=8, ignore_eos=True)


@pytest.fixture(scope="module")
def mx4_dirs(tmp_path_factory):
    from arks_amd.loader.safetensors_loader import save_mx4_checkpoint

    root = tmp_path_factory.mktemp("mx4moe")
    dirs = {"mx4": str(root / "mx4"), "bf16": str(root / "bf16")}
    save_mx4_checkpoint(PRESET_CONFIGS["tiny-moe-gpu"], dirs["mx4"], seed=3,
                        dequantized_dir=dirs["bf16"])
    return dirs


def _engine(path, **kw):
    return LLMEngine(EngineConfig(device="cuda", kv_cache_blocks=512,
                                  max_model_len=1024, seed=5, model_path=path,
                                  **kw))


@pytest.mark.parametrize("mode", ["bf16", "mxfp4"])
def test_engine_mx4_experts_graph_equals_eager_and_agrees_with_bf16(
        mx4_dirs, mode):
    """Graph = eager = second graph; in bf16-activation mode also the
    project's rule for a quantized engine against its dequantized bf16 twin:
    greedy tokens agree on at least half of the positions."""
    assert ops.native_available()
    outs = []
    for eager in (False, True, False):
        e = _engine(mx4_dirs["mx4"], enforce_eager=eager, mx_activations=mode)
        assert e.runner.quantization == "mxfp4"
        moe = e.runner.model.layers[0].mlp
        assert moe.mx4 and moe.mx4_act == mode and moe.w13_mx4.is_cuda
        assert not hasattr(moe, "w13") and not hasattr(moe, "w2")
        outs.append(e.generate(PROMPTS + [LONG], SP))
        del e
    assert all(len(o) == 8 for o in outs[0])
    assert outs[0] == outs[1] == outs[2]
    if mode == "bf16":
        e = _engine(mx4_dirs["bf16"])
        assert not e.runner.model.layers[0].mlp.mx4
        twin = e.generate(PROMPTS + [LONG], SP)
        same = sum(x == y for a, b in zip(outs[0], twin) for x, y in zip(a, b))
        print(f"MoE mxfp4 vs dequantized-bf16 token agreement: {same}/32")
        assert same * 2 >= 32
