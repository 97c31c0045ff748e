"""Bit-exact fixture of the quantized streaming GEMMs (w4_gemm.hip,
w8_gemm.hip): the dense W4 and W8 skinny kernels and the routed W4 expert
kernel.

The dense cases call the extension with an explicit (nw, nsplits,
k_per_split), so toy shapes reach every MT, both N sub-tile counts, single
and odd chunk counts, unequal splits and a row-strided A. The routed cases
build their tables with ops.moe_route. Inputs come from a seeded CPU
generator, so any build can be compared bit for bit with the recorded one.

    python scripts/wq_stream_golden.py [OUT_DIR]

writes dense.npz and routed.npz to tests/golden/wq_stream/: the raw bits of
every bf16 output (uint16; for the routed cases the whole sentinel-filled
tensor) and, where K is split, of the f32 partial rows < M of each split
(uint32). It was run once, on an MI355X, at the commit before the three
kernel bodies were merged into one; tests/test_wq_stream_gpu.py asserts
torch.equal against those files. Re-record only when a change is meant to
move the bits.

    python scripts/wq_stream_golden.py --check-inputs

runs the inputs through ops.ref on the CPU and asserts that every output
stands well away from zero (see check_inputs).
"""

from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden", "wq_stream")
DENSE = os.path.join(GOLDEN_DIR, "dense.npz")
ROUTED = os.path.join(GOLDEN_DIR, "routed.npz")

FORMATS = ("w4", "w8")

# name: (M, N, K, nw, nsplits, k_per_split, bias, a_stride or None)
DENSE_CASES = {
    # single chunk: every prefetch clamps
    "one_chunk": (1, 64, 128, 1, 1, 128, False, None),
    # odd chunk count (the ring exits mid-unroll), MT = 2 with clamped rows
    "odd_chunks": (17, 128, 384, 2, 1, 384, True, 384 + 8),
    # unequal splits (3 and 2 chunks), MT = 3
    "uneven_splits": (33, 64, 640, 1, 2, 384, False, None),
    # one chunk per split, partial store across both N sub-tiles
    "chunk_splits": (16, 128, 256, 2, 2, 128, False, None),
    # MT = 4, direct epilogue over both sub-tiles
    "mt4_direct": (49, 128, 512, 2, 1, 512, True, None),
}

# name: (src_div, T, top_k, N, K, tokens of local experts 0 / 1)
# Three local experts (global ids 1..3) of five; the third gets no pair, and
# the pairs of global experts 0 and 4 belong to no local expert.
ROUTED_CASES = {
    # 67 pairs (two slabs, the second of 3 rows: mt = 1 there), 9 pairs, none
    "gather_two_slabs": (2, 70, 2, 64, 256, 67, 9),
    # a = h [T*k, K]: 40 rows, three chunks
    "rows_three_chunks": (1, 20, 2, 128, 384, 18, 5),
    # max_rows = 40 > 32 and N = 128: nw = 2; 35 pairs are MT = 3
    "gather_nw2": (2, 40, 2, 128, 256, 35, 7),
}
SENTINEL = -3.0
EXPERT_BASE, N_LOCAL = 1, 3


def _gen(name, tag):
    seed = sum((i + 1) * b for i, b in enumerate(f"{name}/{tag}".encode()))
    return torch.Generator().manual_seed(seed)


def make_w4(name, N, K, experts=None):
    """Packed (qweight, scales, zeros) on the CPU: random nibbles, zero-points
    in 1..15 that vary per (row, group), random f16 scales around 0.0077 (so
    weights of std ~0.05). experts = E stacks E such weights."""
    from arks_amd.ops import ref

    g = _gen(name, "w4")
    packs = []
    for _ in range(experts or 1):
        q = torch.randint(0, 16, (N, K), generator=g, dtype=torch.uint8)
        z = torch.randint(1, 16, (N, K // 128), generator=g, dtype=torch.uint8)
        s = (0.0077 * (0.5 + torch.rand(N, K // 128, generator=g))).half()
        packs.append(ref.w4_pack(q, z, s.float()))
    if experts is None:
        return packs[0]
    return tuple(torch.stack([p[i] for p in packs]) for i in range(3))


def make_w8(name, N, K):
    """(w8 e4m3fn [N, K], scales f32 [K/128, N]) on the CPU: normal weights
    scaled to the e4m3 range, one random scale per (k-block, row), dequantized
    std ~0.05."""
    g = _gen(name, "w8")
    w = (64.0 * torch.randn(N, K, generator=g)).clamp(-448.0, 448.0)
    scales = (0.05 / 64.0) * (0.5 + torch.rand(K // 128, N, generator=g))
    return w.to(torch.float8_e4m3fn), scales.float().contiguous()


def make_weight(fmt, name, N, K):
    return make_w4(name, N, K) if fmt == "w4" else make_w8(name, N, K)


def make_dense_inputs(fmt, name, device):
    """(a, weight tuple, bias or None) of a dense case. A is normal with std
    0.5; with a_stride it is a view into a wider buffer."""
    M, N, K, _nw, _ns, _kps, has_bias, a_stride = DENSE_CASES[name]
    g = _gen(name, "a")
    buf = (0.5 * torch.randn(M, a_stride or K, generator=g)).bfloat16()
    bias = torch.randn(N, generator=g).bfloat16() if has_bias else None
    buf = buf.to(device)
    a = buf if a_stride is None else buf[:, :K]
    weight = tuple(t.to(device) for t in make_weight(fmt, name, N, K))
    return a, weight, None if bias is None else bias.to(device)


def run_dense(native, fmt, name, device):
    """Launch one dense case. Returns (out bf16 [M, N], partial rows f32
    [nsplits, M, N] or None when the case does not split)."""
    M, N, _K, nw, nsplits, kps, _b, _s = DENSE_CASES[name]
    a, weight, bias = make_dense_inputs(fmt, name, device)
    gemm = getattr(native, fmt + "_skinny_gemm")
    partials = getattr(native, fmt + "_skinny_gemm_partials")
    mrows = 16 * min(-(-M // 16), 4)
    out = torch.empty((M, N), dtype=torch.bfloat16, device=device)
    if nsplits == 1:
        part = torch.empty(0, dtype=torch.float32, device=device)
        gemm(out, part, a, *weight, bias, kps, nsplits, nw)
        return out, None
    part = torch.full((nsplits * mrows * N,), float("nan"),
                      dtype=torch.float32, device=device)
    partials(part, a, *weight, kps, nsplits, nw)
    rows = part.view(nsplits, mrows, N)[:, :M, :].clone()
    gemm(out, part, a, *weight, bias, kps, nsplits, nw)
    return out, rows


def routed_ids(name):
    """ids int32 [T, top_k] (global expert ids, distinct per token): the
    first n0 tokens route to local expert 0, n1 evenly spread ones to local
    expert 1, the other slots to the non-local experts 0 and 4; the slot
    order alternates with t."""
    _sd, T, top_k, _N, _K, n0, n1 = ROUTED_CASES[name]
    assert top_k == 2
    step = T // n1
    ids = torch.empty(T, 2, dtype=torch.int32)
    for t in range(T):
        first = EXPERT_BASE if t < n0 else 0
        second = (EXPERT_BASE + 1 if t % step == 3 and t // step < n1
                  else EXPERT_BASE + N_LOCAL)
        ids[t] = torch.tensor([first, second] if t % 2 else [second, first])
    return ids


def make_routed_inputs(name, device):
    """(a, stacked packed triple, ids) of a routed case."""
    src_div, T, top_k, N, K, _n0, _n1 = ROUTED_CASES[name]
    g = _gen(name, "a")
    a = (0.5 * torch.randn(T * top_k // src_div, K, generator=g)).bfloat16()
    packed = tuple(t.to(device) for t in make_w4(name, N, K, experts=N_LOCAL))
    return a.to(device), packed, routed_ids(name).to(device)


def run_routed(ops, name, device):
    """Launch one routed case with max_rows = T into a sentinel-filled out.
    Returns (out bf16 [T*top_k, N], counts, pairs)."""
    src_div, T, top_k, N, _K, _n0, _n1 = ROUTED_CASES[name]
    a, packed, ids = make_routed_inputs(name, device)
    counts, pairs = ops.moe_route(ids, EXPERT_BASE, N_LOCAL)
    out = torch.full((T * top_k, N), SENTINEL, dtype=torch.bfloat16,
                     device=device)
    ops.w4_moe_gemm(a, packed, counts, pairs, src_div, T, out=out)
    return out, counts, pairs


def _bf16_step(v: float) -> float:
    """Spacing of bf16 at magnitude v (8 significand bits)."""
    return 2.0 ** (int(np.floor(np.log2(v))) - 7)


def check_inputs():
    """CPU check that no case can pass by accident: through ops.ref, mean
    |out| of every case (without the bias; for routed cases over the written
    rows) is at least ten times the bf16 rounding step at that magnitude, and
    the routed tables have the lists the cases are about."""
    import arks_amd.ops as ops
    from arks_amd.ops import ref

    for fmt in FORMATS:
        for name, case in DENSE_CASES.items():
            a, weight, _bias = make_dense_inputs(fmt, name, "cpu")
            if fmt == "w4":
                zeros = weight[2]  # [K/128, N]
                assert int(zeros.min()) >= 1
                assert zeros.shape[0] == 1 or (zeros[0] != zeros[1]).any()
                out = ref.w4_linear(a, weight)
            else:
                out = ref.w8_linear(a, *weight)
            mean = float(out.float().abs().mean())
            print(f"{fmt} {name}: mean |out| = {mean:.4f}, "
                  f"bf16 step {_bf16_step(mean):.6f}")
            assert mean >= 10 * _bf16_step(mean)
            if case[7] is not None:
                assert a.stride(0) == case[7] and not a.is_contiguous()
    for name, case in ROUTED_CASES.items():
        src_div, T, top_k, N, _K, n0, n1 = case
        a, packed, ids = make_routed_inputs(name, "cpu")
        assert all(len(set(row.tolist())) == top_k for row in ids)
        counts, pairs = ops.moe_route(ids, EXPERT_BASE, N_LOCAL)
        assert counts.tolist() == [n0, n1, 0], counts
        assert int(packed[2].min()) >= 1
        out = torch.full((T * top_k, N), SENTINEL, dtype=torch.bfloat16)
        ref.w4_moe_gemm(a, packed, counts, pairs, src_div, out=out)
        local = (ids.reshape(-1) >= EXPERT_BASE) & (
            ids.reshape(-1) < EXPERT_BASE + N_LOCAL)
        assert int(local.sum()) == n0 + n1 < T * top_k
        assert (out[~local] == SENTINEL).all()
        mean = float(out[local].float().abs().mean())
        print(f"routed {name}: counts {counts.tolist()}, mean |out| = "
              f"{mean:.4f}, bf16 step {_bf16_step(mean):.6f}")
        assert mean >= 10 * _bf16_step(mean)
    print("inputs OK")


def _u16(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _u32(t):
    return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


def main(argv):
    if "--check-inputs" in argv:
        return check_inputs()
    out_dir = argv[1] if len(argv) > 1 else GOLDEN_DIR
    import arks_amd.ops as ops

    assert torch.cuda.is_available() and ops.native_available()
    native = ops._native()
    dense, routed = {}, {}
    for fmt in FORMATS:
        for name in DENSE_CASES:
            out, rows = run_dense(native, fmt, name, "cuda")
            dense[f"{fmt}.{name}.out"] = _u16(out)
            if rows is not None:
                dense[f"{fmt}.{name}.part"] = _u32(rows)
    for name in ROUTED_CASES:
        out, _counts, _pairs = run_routed(ops, name, "cuda")
        routed[name + ".out"] = _u16(out)
    torch.cuda.synchronize()
    os.makedirs(out_dir, exist_ok=True)
    for fname, blobs in (("dense.npz", dense), ("routed.npz", routed)):
        path = os.path.join(out_dir, fname)
        np.savez_compressed(path, **blobs)
        print(f"wrote {path}: {os.path.getsize(path)} bytes, "
              f"{len(blobs)} arrays")


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    main(sys.argv)
