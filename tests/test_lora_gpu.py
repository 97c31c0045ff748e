"""Multi-LoRA on the GPU: the lora_shrink / lora_expand HIP kernels against
the fp32 reference, and the engine through them (graphed decode, mixed
batches, wiring against merged weights)."""

import pytest
import torch

import arks_amd.ops as ops
from arks_amd.engine import LLMEngine, SamplingParams
from arks_amd.ops import ref
from lora_testutil import engine_cfg, make_adapters, run_mixed, wiring_distances

pytestmark = pytest.mark.gpu

TOL = dict(atol=2e-2, rtol=2e-2)  # the project's bf16-versus-fp32 convention
DEV = "cuda"


def _tiles(rows):
    return torch.tensor(rows, dtype=torch.int32, device=DEV).reshape(-1, 3)


def _covered(tiles, T):
    m = torch.zeros(T, dtype=torch.bool)
    for row0, nrows, slot in tiles.tolist():
        if slot >= 0:
            m[row0:row0 + nrows] = True
    return m.to(DEV)


def _shrink_case(T, K, S, R, tiles, L=2, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, K, generator=g).to(torch.bfloat16).to(DEV)
    A = (torch.randn(L, S * R, K, generator=g) / K ** 0.5).to(
        torch.bfloat16).to(DEV)
    tiles = _tiles(tiles)
    sentinel = 12345.0
    h = torch.full((T + 3, S * R), sentinel, device=DEV)
    want = h.clone()
    ops.lora_shrink(h, x, A, tiles)
    ref.lora_shrink(want, x, A, tiles)
    cov = _covered(tiles, T + 3)
    torch.testing.assert_close(h[cov], want[cov], **TOL)
    assert torch.equal(h[~cov], want[~cov])  # uncovered rows untouched
    assert cov.any()


def test_shrink_single_row_tile():
    _shrink_case(T=1, K=512, S=1, R=16, tiles=[(0, 1, 0)])


def test_shrink_partial_tiles_two_slots_uneven_k_split():
    # K/32 = 37 steps do not divide over the 4 waves; rows 21..29 uncovered
    _shrink_case(T=37, K=1184, S=3, R=16,
                 tiles=[(0, 16, 0), (16, 5, 1), (30, 7, 0)])


@pytest.mark.parametrize("K,R", [(3584, 64), (18944, 16)])
def test_shrink_deep_k(K, R):
    _shrink_case(T=16, K=K, S=1, R=R, tiles=[(0, 16, 1)])


def _expand_case(T, N, offs, R, tiles, L=2, seed=0, pad_rank=None):
    g = torch.Generator().manual_seed(seed)
    S = len(offs) - 1
    h = torch.randn(T, S * R, generator=g).to(DEV)
    B = (torch.randn(L, N, R, generator=g) / R ** 0.5).to(torch.bfloat16)
    if pad_rank is not None:  # a smaller-rank adapter zero-padded into R
        B[:, :, pad_rank:] = 0
        h.view(T, S, R)[:, :, pad_rank:] = 7.0  # must meet zeros in B
    B = B.to(DEV)
    y0 = torch.randn(T, N, generator=g).to(torch.bfloat16).to(DEV)
    tiles = _tiles(tiles)
    y = y0.clone()
    ops.lora_expand(y, h, B, tiles, offs)
    want = y0.float()
    ref.lora_expand(want, h, B, tiles, offs)
    cov = _covered(tiles, T)
    torch.testing.assert_close(y[cov].float(), want[cov], **TOL)
    assert torch.equal(y[~cov], y0[~cov])  # bit-identical uncovered rows
    assert not torch.equal(y[cov], y0[cov])
    return y


def test_expand_three_slices():
    _expand_case(T=37, N=1024, offs=(0, 512, 768, 1024), R=16,
                 tiles=[(0, 16, 0), (16, 5, 1), (30, 7, 0)])


def test_expand_column_tail():
    # N = 16 * 37: the last workgroup's column blocks run past N
    _expand_case(T=20, N=592, offs=(0, 592), R=32,
                 tiles=[(0, 16, 1), (16, 4, 0)])


def test_expand_rank64():
    _expand_case(T=18, N=512, offs=(0, 256, 512), R=64,
                 tiles=[(0, 16, 0), (16, 2, 1)])


def test_expand_rank8_padded_into_16():
    _expand_case(T=16, N=256, offs=(0, 256), R=16, tiles=[(0, 16, 0)],
                 pad_rank=8)


def test_skipped_middle_tile():
    tiles = [(0, 16, 0), (16, 16, -1), (32, 8, 1)]
    _shrink_case(T=40, K=512, S=2, R=16, tiles=tiles)
    _expand_case(T=40, N=512, offs=(0, 256, 512), R=16, tiles=tiles)


def _dense_apply(y0, x, A, B, row_slot, offs, R):
    out = y0.float().clone()
    for t, slot in enumerate(row_slot):
        if slot < 0:
            continue
        h = A[slot].float() @ x[t].float()
        for s in range(len(offs) - 1):
            cols = slice(offs[s], offs[s + 1])
            out[t, cols] += B[slot, cols].float() @ h[s * R:(s + 1) * R]
    return out


def test_lora_apply_slot_stride_against_dense_formula():
    """Shrink and expand chained, three slots with distinct weights, each
    used, against the dense fp32 formula."""
    g = torch.Generator().manual_seed(4)
    T, K, N, R, L = 45, 512, 768, 16, 3
    offs = (0, 512, 640, 768)
    x = torch.randn(T, K, generator=g).to(torch.bfloat16).to(DEV)
    A = (torch.randn(L, 3 * R, K, generator=g) / K ** 0.5).to(
        torch.bfloat16).to(DEV)
    B = (torch.randn(L, N, R, generator=g) / R ** 0.5).to(
        torch.bfloat16).to(DEV)
    y0 = torch.randn(T, N, generator=g).to(torch.bfloat16).to(DEV)
    q_lens = [10, 9, 7, 19]
    slots = [2, 0, -1, 1]
    tiles = ops.build_lora_tiles(q_lens, slots, DEV)
    row_slot = [s for n, s in zip(q_lens, slots) for _ in range(n)]
    y = y0.clone()
    h_ws = torch.zeros(64, 3 * R, device=DEV)
    ops.lora_apply(y, x, A, B, tiles, offs, h_ws)
    want = _dense_apply(y0, x, A, B, row_slot, offs, R)
    cov = torch.tensor([s >= 0 for s in row_slot], device=DEV)
    torch.testing.assert_close(y[cov].float(), want[cov], **TOL)
    assert torch.equal(y[~cov], y0[~cov])
    # every slot's rows differ from what another slot's weights would give
    wrong = _dense_apply(y0, x, A, B, [(s + 1) % L if s >= 0 else -1
                                       for s in row_slot], offs, R)
    assert (y[cov].float() - wrong[cov]).abs().max() > 0.5


def test_kernels_reject_bad_shapes():
    x = torch.zeros(4, 48, dtype=torch.bfloat16, device=DEV)
    A = torch.zeros(1, 16, 48, dtype=torch.bfloat16, device=DEV)
    h = torch.zeros(4, 16, device=DEV)
    with pytest.raises(RuntimeError, match="K % 32"):
        ops.lora_shrink(h, x, A, _tiles([(0, 4, 0)]))
    y = torch.zeros(4, 24, dtype=torch.bfloat16, device=DEV)
    B = torch.zeros(1, 24, 16, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="N % 16"):
        ops.lora_expand(y, h, B, _tiles([(0, 4, 0)]), (0, 24))


# ---------------- engine on tiny-gpu ----------------
PROMPTS = [[1, 5, 9, 20, 31, 7], [3, 3, 7, 90], [17] * 40]
LORAS = ["a", "b", None]


@pytest.fixture(scope="module")
def adapters(tmp_path_factory):
    return make_adapters("tiny-gpu", tmp_path_factory.mktemp("adapters"))


def _engine(adapters, **kw):
    return LLMEngine(engine_cfg("tiny-gpu", DEV, enable_lora=True,
                                lora_modules=adapters, **kw))


def test_graphed_decode_equals_eager_with_adapters(adapters):
    sp = SamplingParams(max_tokens=12, ignore_eos=True)
    eager = _engine(adapters, enforce_eager=True).generate(
        PROMPTS, sp, lora=LORAS)
    e = _engine(adapters)
    graphed = e.generate(PROMPTS, sp, lora=LORAS)
    assert graphed == eager
    assert e.runner._lora_graphs and not e.runner._graphs
    assert len({tuple(o) for o in graphed}) == 3


def test_base_requests_on_lora_engine_equal_plain_engine(adapters):
    sp = SamplingParams(max_tokens=12, ignore_eos=True)
    plain = LLMEngine(engine_cfg("tiny-gpu", DEV)).generate(PROMPTS, sp)
    e = _engine(adapters)
    assert e.generate(PROMPTS, sp) == plain
    # all-base steps replay graphs without LoRA launches in them
    assert e.runner._graphs and not e.runner._lora_graphs


def test_adapter_request_alone_equals_mixed_batch(adapters):
    sp = SamplingParams(max_tokens=10, ignore_eos=True)
    alone = _engine(adapters).generate([PROMPTS[0]], sp, lora=["a"])[0]
    reqs = [(PROMPTS[0], "a"), (PROMPTS[1], "b"), (PROMPTS[2], None)]
    out = run_mixed(_engine(adapters), reqs, late=1)
    assert out[0] == alone
    assert out[1] != out[0]


def test_wiring_against_merged_weights_gpu(adapters):
    """Same yardstick as the CPU suite, computed on the GPU: d_drop comes
    from merged models run by the LoRA-free kernels; the engine under "a"
    must sit within d_drop / 3 of merged-"a" and further than d_drop from
    merged-"b". Measured on an MI355X: see docs/kernels.md."""
    d, d_drop, d_neg = wiring_distances("tiny-gpu", DEV, adapters)
    assert d <= d_drop / 3, (d, d_drop)
    assert d_neg > d_drop, (d_neg, d_drop)
