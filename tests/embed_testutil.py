"""Shared cases for the embedding-pooling tests: the packed inputs, the fp64
oracle written from the definition in ops.ref.pool_embed, and the chunking
of mean segments through the carry."""

import functools

import torch

SEG_LENS = [1, 2, 63, 64, 65, 600, 1100]
# non-pooled rows (generation sequences of the same batch) in front of each
# segment and behind the last one; filled with NaN, so reading one shows
GAPS = [3, 0, 5, 1, 0, 7, 2, 4]
HIDDENS = [896, 1024, 3584, 4096]
MODES = ["last", "mean", "cls"]
EPS = 1e-6

# engine tests on the tiny-gpu preset (vocabulary 2048): mixed lengths, one
# prompt longer than max_num_batched_tokens = 64, so that it chunks
ENGINE_PROMPTS = [
    [1, 5, 9, 20, 31, 7],
    [3, 3, 7, 90],
    [17] * 40,
    [11, 400, 23, 1999, 5, 5, 68],
    list(range(100, 148)),
    [7],
    [(13 * i + 5) % 2000 + 3 for i in range(150)],  # > 64: chunks
    [250, 251, 252, 900, 12],
]


def dims_for(H):
    return [H, 256, 33]


@functools.lru_cache(maxsize=None)
def make_inputs(H):
    """(x, residual, weight, starts): bf16 packed rows [T, H] as
    base + 0.5 * noise, so a mean keeps a common component instead of
    cancelling; starts[i] is the first row of segment i."""
    g = torch.Generator().manual_seed(4321 + H)
    starts, row = [], 0
    for gap, n in zip(GAPS, SEG_LENS):
        row += gap
        starts.append(row)
        row += n
    T = row + GAPS[-1]

    def rows():
        base = torch.randn(1, H, generator=g)
        return base + 0.5 * torch.randn(T, H, generator=g)

    x, residual = rows(), rows()
    keep = torch.zeros(T, dtype=torch.bool)
    for s, n in zip(starts, SEG_LENS):
        keep[s:s + n] = True
    x[~keep] = float("nan")
    residual[~keep] = float("nan")
    weight = 1.0 + 0.1 * torch.randn(H, generator=g)
    return (x.to(torch.bfloat16), residual.to(torch.bfloat16),
            weight.to(torch.bfloat16), tuple(starts))


def oracle(x, residual, weight, row0, nrows, mode, dims, normalize,
           eps=EPS):
    """fp64, from the definition: r = dtype(x + residual); y = r *
    rsqrt(mean(r^2) + eps) * w; last / cls / mean; truncate; normalise."""
    sl = slice(row0, row0 + nrows)
    r = (x[sl].float() + residual[sl].float()).to(x.dtype).double()
    y = r * torch.rsqrt(r.pow(2).mean(-1, keepdim=True) + eps) * weight.double()
    if mode == "last":
        v = y[-1]
    elif mode == "cls":
        v = y[0]
    else:
        v = y.sum(0) / nrows
    v = v[:dims]
    if normalize:
        v = v / v.norm().clamp_min(1e-12)
    return v


def oracle_all(H, mode, dims, normalize=True):
    x, residual, weight, starts = make_inputs(H)
    return torch.stack([
        oracle(x, residual, weight, s, n, mode, dims, normalize)
        for s, n in zip(starts, SEG_LENS)])


def whole_segments(H, mode):
    """One table entry per segment, each a single final chunk."""
    _, _, _, starts = make_inputs(H)
    return [(s, n, mode, -1, 0, 1) for s, n in zip(starts, SEG_LENS)]


def chunk_cuts(n):
    """Uneven cut points of an n-row segment: one chunk for n = 1, two for
    n = 2, three otherwise."""
    if n == 1:
        return [0, 1]
    if n == 2:
        return [0, 1, 2]
    return [0, n // 3, n // 3 + max(1, n // 2), n]


def mean_chunk_calls(H):
    """[(entries, owners)] per call: call j pools chunk j of every segment
    that has one, through carry slot = segment index; owners[k] is the
    segment whose final vector row k of that call's output holds (None for a
    non-final chunk)."""
    _, _, _, starts = make_inputs(H)
    calls = []
    for j in range(3):
        entries, owners = [], []
        for i, (s, n) in enumerate(zip(starts, SEG_LENS)):
            cuts = chunk_cuts(n)
            if j >= len(cuts) - 1:
                continue
            final = j == len(cuts) - 2
            slot = i if len(cuts) > 2 else -1
            entries.append((s + cuts[j], cuts[j + 1] - cuts[j], "mean", slot,
                            cuts[j], int(final)))
            owners.append(i if final else None)
        calls.append((entries, owners))
    return calls


def run_mean_chunked(pool, H, dims, device, normalize=True):
    """Mean over 2-3 pool_embed calls per segment; `pool(table_entries,
    carry)` runs one call. Returns [num_segments, dims] fp32 on the CPU."""
    carry = torch.full((len(SEG_LENS), H), float("nan"), dtype=torch.float32,
                       device=device)  # stale contents must never be read
    out = torch.zeros(len(SEG_LENS), dims, dtype=torch.float32)
    for entries, owners in mean_chunk_calls(H):
        got = pool(entries, carry).cpu()
        for k, i in enumerate(owners):
            if i is None:
                assert got[k].abs().max() == 0  # not due yet
            else:
                out[i] = got[k]
    return out
