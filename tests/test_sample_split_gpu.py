"""Argmax / Gumbel sampling over rows x vocabulary chunks (sampling.hip).

Below one row per compute unit the samplers cut a row into chunks, one
workgroup each, and a second launch merges the chunk winners. The ids must
not depend on the chunk count: every forced count in {2, 3, 8} is compared
with chunks = 1 (one workgroup per row, the kernel as it was), greedy also
with torch.argmax of the float copy on the CPU. Gumbel is compared with
chunks = 1 only: __logf is not the CPU's log.
"""

import pytest
import torch

import arks_amd.ops as ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
CHUNKS = (2, 3, 8)
ROWS = (1, 3, 64)
# a tail (9, 1000 is whole vectors, 4111) and row strides that are no
# multiple of 8 (9, 4111)
VOCABS = (8, 9, 1000, 4104, 4111)


def _chunk_len(vocab, chunks):
    """The launcher's chunk length: ceil(vocab / chunks) rounded up to 8."""
    return -(-(-(-vocab // chunks)) // 8) * 8


@pytest.fixture(scope="module")
def gen():
    return torch.Generator(device="cpu").manual_seed(1234)


def _logits(gen, rows, vocab):
    # bf16 has 8 bits of mantissa: a row of 4111 normals has tied maxima
    # now and then, which is wanted
    return torch.randn(rows, vocab, generator=gen).to(torch.bfloat16)


@pytest.mark.parametrize("vocab", VOCABS)
@pytest.mark.parametrize("rows", ROWS)
def test_greedy_chunked(gen, rows, vocab):
    cpu = _logits(gen, rows, vocab)
    logits = cpu.to(DEV)
    want = torch.argmax(cpu.float(), dim=-1)
    one = ops.greedy_sample(logits, chunks=1)
    assert one.dtype == torch.int64
    assert torch.equal(one.cpu(), want)
    for chunks in CHUNKS:
        assert torch.equal(ops.greedy_sample(logits, chunks=chunks), one), chunks
    # the default pick of the wrapper
    assert torch.equal(ops.greedy_sample(logits), one)


@pytest.mark.parametrize("vocab", VOCABS)
@pytest.mark.parametrize("rows", ROWS)
def test_gumbel_chunked(gen, rows, vocab):
    logits = _logits(gen, rows, vocab).to(DEV)
    u = torch.rand(rows, vocab, generator=gen).to(DEV)
    temps = torch.tensor([0.0, 0.7, 1.0, 1.5], dtype=torch.float32)
    temps = temps.repeat(-(-rows // 4))[:rows].to(DEV)
    one = ops.sample_tokens(logits, temps, u, chunks=1)
    greedy = ops.greedy_sample(logits, chunks=1)
    assert torch.equal(one[temps == 0], greedy[temps == 0])
    for chunks in CHUNKS:
        got = ops.sample_tokens(logits, temps, u, chunks=chunks)
        assert torch.equal(got, one), chunks
    assert torch.equal(ops.sample_tokens(logits, temps, u), one)


def _adversarial(vocab, chunks):
    """(logits bf16 [7, vocab] on the CPU, expected ids)."""
    cl = _chunk_len(vocab, chunks)
    assert cl < vocab and vocab % 8 != 0
    lowest = torch.finfo(torch.bfloat16).min
    x = torch.full((7, vocab), -1.0)
    want = []
    # equal maxima, last element of one chunk and first of the next: the
    # lower index wins
    x[0, cl - 1] = x[0, cl] = 3.0
    want.append(cl - 1)
    # all equal
    x[1] = 0.5
    want.append(0)
    # all -inf: nothing beats the initial pair
    x[2] = float("-inf")
    want.append(0)
    # the lowest finite bf16 everywhere (-FLT_MAX itself is not a bf16)
    x[3] = lowest
    want.append(0)
    # NaN scattered through the row, never taken; one next to the maximum
    x[4, ::5] = float("nan")
    x[4, vocab // 2 + 1] = 2.0
    assert (vocab // 2 + 1) % 5 != 0
    x[4, vocab // 2 + 2] = float("nan")
    want.append(vocab // 2 + 1)
    # all NaN
    x[5] = float("nan")
    want.append(0)
    # the maximum in the scalar tail
    x[6, vocab - 1] = 1.0
    want.append(vocab - 1)
    return x.to(torch.bfloat16), torch.tensor(want, dtype=torch.int64)


@pytest.mark.parametrize("chunks", CHUNKS)
def test_adversarial_rows(chunks):
    vocab = 4111
    cpu, want = _adversarial(vocab, chunks)
    logits = cpu.to(DEV)
    one = ops.greedy_sample(logits, chunks=1)
    assert torch.equal(one.cpu(), want)
    assert torch.equal(ops.greedy_sample(logits, chunks=chunks), one)
    # temperature 0 rows of the Gumbel kernel are the same argmax
    u = torch.full((7, vocab), 0.5, device=DEV)
    zero = torch.zeros(7, device=DEV)
    assert torch.equal(ops.sample_tokens(logits, zero, u, chunks=chunks), one)


def test_default_chunk_count():
    """The wrapper's pick: a few workgroups per CU, chunks of at least 2048,
    one workgroup per row once the rows fill the chip."""
    pick = ops._sample_chunks
    assert pick(64, 152064, 256) == 16
    assert pick(256, 152064, 256) == 1
    assert pick(1000, 152064, 256) == 1
    assert pick(1, 152064, 256) == 152064 // 2048
    assert pick(64, 4111, 256) == 2
    assert pick(64, 1000, 256) == 1
