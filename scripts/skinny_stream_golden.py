"""Bit-exact fixture of the skinny decode GEMM (skinny_gemm.hip).

The cases call the extension with an explicit (config, nsplits, k_per_split),
so small shapes reach the long K-ranges, tails and split layouts of the decode
plan. Inputs come from an integer formula that is exact in bf16 (no RNG), so
any build can be compared bit for bit with the recorded one.

    python scripts/skinny_stream_golden.py [OUT.npz]

writes the raw bits of every case (bf16 outputs as uint16, and for split cases
the f32 partial rows < M as uint32; every fourth row for the largest slab, see
RECORDED_ROWS) to tests/golden/skinny_stream/parent.npz.
It was run once, on an MI355X, at the commit before the W-ring rewrite of the
kernel; tests/test_skinny_stream_gpu.py asserts torch.equal against that file.
Re-record only when a change is meant to move the bits.
"""

from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "skinny_stream", "parent.npz")

# name: (M, N, K, config, nsplits, k_per_split, a_stride or None)
CASES = {
    # 9.25 chunks of 128 per split: the W ring wraps, 32-wide tail chunk
    "tallk_wrap": (64, 64, 2368, 1, 2, 1184, None),
    # direct epilogue with bias; the qkv K-range, the ring never refills
    "direct_448": (64, 128, 448, 0, 1, 448, None),
    # the qkv split
    "split_448": (64, 128, 896, 0, 2, 448, None),
    # MT = 3, 12 full chunks
    "mt3_long": (33, 64, 1536, 0, 1, 1536, None),
    # MT = 2, uneven splits (224 + 192)
    "mt2_uneven": (17, 192, 416, 0, 2, 224, None),
    # shorter than one chunk
    "short": (5, 64, 96, 0, 1, 96, None),
    # MT = 1, many splits
    "mt1_splits": (1, 64, 8192, 0, 32, 256, None),
    # row-strided A: a view into a wider buffer, 128 + 32 tail per split
    "strided": (16, 128, 320, 0, 2, 160, 512),
}
# part a only (no recorded bits). First: tall-K kernel, one chunk, unsplit
EXTRA_CASES = {
    "tallk_one_chunk": (49, 64, 128, 1, 1, 128, None),
    # tall-K tiles are 128 rows: one whole tile and one that hangs over N
    "tallk_n192": (64, 192, 384, 1, 2, 192, None),
    "tallk_n192_direct": (50, 192, 160, 1, 1, 160, None),
}


# Partial rows that are recorded (default: every row < M). The qkv split is
# the largest slab; every fourth row of it keeps the file small and still
# covers every lane group, wave and M tile of the store.
RECORDED_ROWS = {"split_448": slice(0, None, 4)}


def recorded_rows(name, rows):
    return rows[:, RECORDED_ROWS.get(name, slice(None)), :]


def make_inputs(case, device, unit=False):
    """(a, w, bias) for a case. Every value is an 8-bit integer times a power
    of two, so it is exact in bf16.

    unit=False (the recorded inputs): the exponent varies along K so that the
    f32 partial sums do round and their bits depend on the summation order;
    the products are small (|A @ W^T| < 0.1).
    unit=True (the tolerance check): the plain formula, A in [-0.5, 0.5] and
    W in [-0.49, 0.49], so that |A @ W^T| is of order sqrt(K) / 12, far above
    the tolerance, and a wrong or missing product cannot hide inside it."""
    M, N, K, _config, _nsplits, _kps, a_stride = case
    width = K if a_stride is None else a_stride
    i = torch.arange(M, dtype=torch.int64).view(-1, 1)
    j = torch.arange(width, dtype=torch.int64).view(1, -1)
    av = ((i * 131 + j * 71) % 257 - 128).double() / 256.0
    n = torch.arange(N, dtype=torch.int64).view(-1, 1)
    k = torch.arange(K, dtype=torch.int64).view(1, -1)
    wv = ((n * 89 + k * 113) % 251 - 125).double() / 256.0
    if not unit:
        av = av * torch.pow(2.0, -((i + j) % 7).double())
        wv = wv / 16.0 * torch.pow(2.0, -((3 * n + k) % 5).double())
    bv = ((torch.arange(N, dtype=torch.int64) * 37) % 129 - 64).double() / 64.0
    buf = av.to(torch.bfloat16)
    assert torch.equal(buf.double(), av), "A formula must be exact in bf16"
    w = wv.to(torch.bfloat16)
    assert torch.equal(w.double(), wv), "W formula must be exact in bf16"
    buf = buf.to(device)
    a = buf if a_stride is None else buf[:, 64:64 + K]
    return a, w.to(device), bv.to(torch.bfloat16).to(device)


def run_case(native, case, device, config=None, unit=False, groups=0):
    """Launch one case. Returns (out bf16 [M, N], partial rows f32
    [nsplits, M, N] or None when the case does not split). groups is the
    workgroups-per-split argument of config 3 (0 = auto)."""
    M, N, K, cfg, nsplits, kps, _ = case
    cfg = cfg if config is None else config
    a, w, bias = make_inputs(case, device, unit)
    # configs 0 and 3 (A-resident) take the slab height from M
    mrows = 16 * (min(-(-M // 16), 4) if cfg in (0, 3) else 4)
    out = torch.empty((M, N), dtype=torch.bfloat16, device=device)
    if nsplits == 1:
        part = torch.empty(0, dtype=torch.float32, device=device)
        native.skinny_gemm(out, part, a, w, bias, kps, nsplits, cfg)
        return out, None
    part = torch.full((nsplits * mrows * N,), float("nan"),
                      dtype=torch.float32, device=device)
    native.skinny_gemm_partials(part, a, w, kps, nsplits, cfg, groups)
    rows = part.view(nsplits, mrows, N)[:, :M, :].clone()
    native.skinny_gemm(out, part, a, w, bias, kps, nsplits, cfg, groups)
    return out, rows


def main(argv):
    path = argv[1] if len(argv) > 1 else GOLDEN
    import arks_amd.ops as ops

    assert torch.cuda.is_available() and ops.native_available()
    native = ops._native()
    blobs = {}
    for name, case in CASES.items():
        out, rows = run_case(native, case, "cuda")
        blobs[name + ".out"] = out.view(torch.int16).cpu().numpy().view(np.uint16)
        if rows is not None:
            rows = recorded_rows(name, rows).contiguous()
            blobs[name + ".part"] = (
                rows.view(torch.int32).cpu().numpy().view(np.uint32))
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez_compressed(path, **blobs)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(blobs)} arrays")


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    main(sys.argv)
