"""Sort-free top-k / top-p / min-p cutoff (topk_topp.hip) against the float64
definition in ref.sample_cutoff, and its two consumers.

A cutoff pair always describes a prefix of the (value descending, index
ascending) order, so comparing kept sets comes down to comparing their
sizes. Rows limited by top_k must match exactly. For top_p / min_p the
kernel's fixed-point mass (error < 152k * 2^-41 of Z) and exp2 (a few ulp)
allow EPS = 1e-4 on the parameter, and the test checks that this band is at
most 4 tokens wide for every row it uses, so it cannot hide a wrong cutoff.
"""

import pytest
import torch

import arks_amd.ops as ops
from arks_amd.ops import ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS = 1e-4
ROWS = (1, 3, 64)
VOCABS = (8, 9, 1000, 4104, 4111)
TEMPS = (0.0, 0.3, 0.7, 1.5)
INF = float("inf")
KEEP_ALL = (-INF, ref.INT32_MAX)
# (top_k, top_p, min_p), cycled over the rows (15 is coprime to the 4
# temperatures); top_k "v" = vocab, "v+5" = vocab + 5, both off
FILTERS = (
    (0, 1.0, 0.0), (1, 1.0, 0.0), (20, 1.0, 0.0), ("v", 1.0, 0.0),
    ("v+5", 1.0, 0.0), (0, 1e-9, 0.0), (0, 0.5, 0.0), (0, 0.8, 0.0),
    (0, 0.95, 0.0), (0, 1.0, 0.05), (0, 1.0, 0.3), (20, 0.8, 0.0),
    (20, 0.95, 0.05), (0, 0.5, 0.3), ("v+5", 0.8, 0.05),
)


def _params(rows, vocab, shift=0):
    f = [FILTERS[(r + shift) % len(FILTERS)] for r in range(rows)]
    k = [{"v": vocab, "v+5": vocab + 5}.get(x[0], x[0]) for x in f]
    return (torch.tensor([TEMPS[(r + shift) % 4] for r in range(rows)]),
            torch.tensor(k, dtype=torch.int32),
            torch.tensor([x[1] for x in f], dtype=torch.float32),
            torch.tensor([x[2] for x in f], dtype=torch.float32))


def _gpu_cutoff(logits, t, k, p, m):
    cv, ci = ops.sample_cutoff(logits.to(DEV), t.to(DEV), k.to(DEV),
                               p.to(DEV), m.to(DEV))
    assert cv.dtype == torch.float32 and ci.dtype == torch.int32
    return cv.cpu(), ci.cpu()


def _kept(logits, pair):
    return ref.cutoff_keep(logits, *pair).sum(dim=1)


@pytest.mark.parametrize("vocab", VOCABS)
@pytest.mark.parametrize("rows", ROWS)
def test_cutoff_matches_reference(rows, vocab):
    gen = torch.Generator().manual_seed(1000 * rows + vocab)
    logits = (torch.randn(rows, vocab, generator=gen) * 2).to(torch.bfloat16)
    # rows = 64 sees every filter at every temperature over its two rounds
    for shift in (0, 1) if rows == 64 else (0,):
        t, k, p, m = _params(rows, vocab, shift)
        got = _gpu_cutoff(logits, t, k, p, m)
        again = _gpu_cutoff(logits, t, k, p, m)
        assert torch.equal(got[0], again[0]) and torch.equal(got[1], again[1])
        p64, m64 = p.double(), m.double()
        lo = _kept(logits, ref.sample_cutoff(
            logits, t, k, torch.where(p64 < 1, p64 - EPS, p64), m64 * (1 + EPS)))
        hi = _kept(logits, ref.sample_cutoff(
            logits, t, k, torch.where(p64 < 1, p64 + EPS, p64), m64 * (1 - EPS)))
        n_got = _kept(logits, got)
        print("band", int((hi - lo).max()), "above lo", int((n_got - lo).max()))
        assert int((hi - lo).max()) <= 4
        assert bool(((lo <= n_got) & (n_got <= hi)).all())
        off = (t <= 0) | (((k <= 0) | (k >= vocab)) & (p >= 1) & (m <= 0))
        for r in torch.nonzero(off).flatten().tolist():
            assert (float(got[0][r]), int(got[1][r])) == KEEP_ALL


def _adversarial():
    """(logits bf16 [9, 4111], params, kept indices per row; None = the
    keep-all pair)."""
    v = 4111
    x = torch.full((9, v), -1.0)
    rows = []  # (T, top_k, top_p, min_p, kept)
    x[0] = 0.5  # all equal: the lowest indices
    rows.append((1.0, 5, 1.0, 0.0, range(5)))
    # eight ties of the 4th value, across a 16-byte vector edge whatever the
    # row's alignment: the first three still fit
    x[1, 2000] = 3.0
    x[1, 5:13] = 2.0
    rows.append((0.7, 4, 1.0, 0.0, [5, 6, 7, 2000]))
    # ties in the scalar tail
    x[2, 50] = 3.0
    x[2, [100, v - 3, v - 2, v - 1]] = 2.0
    rows.append((1.5, 3, 1.0, 0.0, [50, 100, v - 3]))
    x[3] = -INF  # all -inf: equal weights
    rows.append((1.0, 5, 1.0, 0.0, range(5)))
    # NaN scattered and next to the maximum: never kept
    x[4, ::5] = float("nan")
    x[4, v // 2 + 1] = 2.0
    x[4, v // 2 + 2] = float("nan")
    rows.append((1.0, 3, 1.0, 0.0, [1, 2, v // 2 + 1]))
    x[5, v - 1] = 30.0  # the maximum as the last element takes all the mass
    rows.append((0.3, 0, 0.5, 0.0, [v - 1]))
    rows.append((0.0, 5, 0.5, 0.3, None))  # greedy row
    rows.append((1.0, 0, 1.0, 0.0, None))  # no filter
    # +-3e38 at T = 0.3: 2056 tokens of weight 1, the rest weigh 0;
    # 0.3 * 2056 = 616.8, so 617 of them
    x[8, 0::2] = 3e38
    x[8, 1::2] = -3e38
    rows.append((0.3, 0, 0.3, 0.0, range(0, 2 * 617, 2)))
    cols = list(zip(*rows))
    params = (torch.tensor(cols[0]), torch.tensor(cols[1], dtype=torch.int32),
              torch.tensor(cols[2]), torch.tensor(cols[3]))
    return x.to(torch.bfloat16), params, cols[4]


def test_adversarial_rows():
    logits, params, kept = _adversarial()
    for pair in (_gpu_cutoff(logits, *params),
                 ref.sample_cutoff(logits, *params)):
        keep = ref.cutoff_keep(logits, *pair)
        for r, want in enumerate(kept):
            if want is None:
                assert (float(pair[0][r]), int(pair[1][r])) == KEEP_ALL, r
            else:
                assert torch.nonzero(keep[r]).flatten().tolist() == sorted(want), r


@pytest.mark.parametrize("chunks", (1, 2, 3, 8))
def test_sampler_with_cutoff(chunks):
    """The sampler skipping past the cutoff = the sampler on logits the
    elementwise kernel masked, whatever the chunk count."""
    rows, vocab = 64, 4111
    gen = torch.Generator().manual_seed(77)
    cpu = (torch.randn(rows, vocab, generator=gen) * 2).to(torch.bfloat16)
    cpu[5, 7::3] = float("nan")
    logits = cpu.to(DEV)
    u = torch.rand(rows, vocab, generator=gen).to(DEV)
    t, k, p, m = (x.to(DEV) for x in _params(rows, vocab))
    cutoff = ops.sample_cutoff(logits, t, k, p, m)
    masked = ops.apply_sample_cutoff(logits.clone(), *cutoff)
    want = ref.apply_sample_cutoff(cpu.clone(), *(c.cpu() for c in cutoff))
    assert torch.equal(masked.cpu().view(torch.int16), want.view(torch.int16))
    got = ops.sample_tokens(logits, t, u, chunks=chunks, cutoff=cutoff)
    assert torch.equal(got, ops.sample_tokens(masked, t, u, chunks=chunks))
    # top_k = 1 leaves the argmax alone, at any temperature
    hot = torch.full((rows,), 1.5, device=DEV)
    one = ops.sample_cutoff(logits, hot, torch.ones_like(k),
                            torch.ones_like(p), torch.zeros_like(m))
    assert torch.equal(
        ops.sample_tokens(logits, hot, u, chunks=chunks, cutoff=one),
        ops.greedy_sample(logits))
