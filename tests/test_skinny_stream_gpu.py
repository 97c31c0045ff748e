"""Skinny decode GEMM with the statically unrolled W ring (skinny_gemm.hip).

The extension is called with an explicit (config, nsplits, k_per_split), so
small shapes reach what the decode plan reaches only at 7B sizes: K-ranges
longer than the ring (it wraps and refills), ranges it holds whole, short
tail chunks, every MT and the tall-K configs (eight waves, 128-row tiles,
with N = 64 and 192 leaving the last tile half empty).

Part a compares with F.linear in fp32 at the tolerance of
test_ops_gpu.py::test_skinny_gemm, on inputs of order 1 so that the product
stands far above that tolerance. Part b asserts bit-equality with outputs
recorded from the kernel before the rewrite (scripts/skinny_stream_golden.py,
tests/golden/skinny_stream/parent.npz): every accumulator must still see the
same MFMA sequence over ascending k within the same split boundaries.
"""

import importlib.util
import os

import numpy as np
import pytest
import torch

import arks_amd.ops as ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load_golden_script():
    path = os.path.join(ROOT, "scripts", "skinny_stream_golden.py")
    spec = importlib.util.spec_from_file_location("skinny_stream_golden", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _load_golden_script()
ALL_CASES = dict(G.CASES, **G.EXTRA_CASES)
# (case name, config override): the tall-K case also runs as config 2
RUNS = [(name, None) for name in ALL_CASES] + [("tallk_wrap", 2)]
GOLDEN_RUNS = [(name, None) for name in G.CASES] + [("tallk_wrap", 2)]


def _id(run):
    return run[0] if run[1] is None else f"{run[0]}-config{run[1]}"


@pytest.fixture(scope="module")
def native():
    assert ops.native_available(), "HIP extension must be built on a GPU box"
    return ops._native()


@pytest.fixture(scope="module")
def results(native):
    """Every run once: {(name, config): (out, partial rows or None)}."""
    res = {}
    for name, config in RUNS:
        res[(name, config)] = G.run_case(native, ALL_CASES[name], DEV, config)
    torch.cuda.synchronize()
    return res


@pytest.fixture(scope="module")
def golden():
    return np.load(G.GOLDEN)


@pytest.fixture(scope="module")
def unit_results(native):
    """Every run once more, on the order-1 inputs of part a."""
    res = {}
    for name, config in RUNS:
        res[(name, config)] = G.run_case(native, ALL_CASES[name], DEV, config,
                                         unit=True)
    torch.cuda.synchronize()
    return res


ATOL = RTOL = 5e-2


@pytest.mark.parametrize("run", RUNS, ids=_id)
def test_skinny_stream_matches_linear(unit_results, run):
    """Part a: fp32 F.linear reference, atol = rtol = 5e-2.

    The inputs are make_inputs(unit=True): the recorded inputs of part b give
    |A @ W^T| < 0.1, which the tolerance would swallow whole. With these the
    product has mean magnitude 0.4-1.9 and the test first asserts that a
    missing product (zeros, or the bias alone) would fail on over 90 % of the
    elements."""
    case = ALL_CASES[run[0]]
    M, N, K, _config, nsplits, kps, a_stride = case
    out, rows = unit_results[run]
    a, w, bias = G.make_inputs(case, DEV, unit=True)
    if a_stride is not None:
        assert a.stride(0) == a_stride > K
    ref_nb = torch.nn.functional.linear(a.float(), w.float())
    assert ref_nb.abs().mean() > 5 * ATOL
    assert (ref_nb.abs() > ATOL + RTOL * ref_nb.abs()).float().mean() > 0.9
    ref = torch.nn.functional.linear(a.float(), w.float(), bias.float())
    torch.testing.assert_close(out.float(), ref, atol=ATOL, rtol=RTOL)
    if nsplits > 1:
        assert rows.shape == (nsplits, M, N) and not torch.isnan(rows).any()
        # each split's rows are the product over its own K-range ...
        for s in range(nsplits):
            ks = slice(s * kps, min(K, (s + 1) * kps))
            ref_s = torch.nn.functional.linear(a[:, ks].float(),
                                               w[:, ks].float())
            torch.testing.assert_close(rows[s], ref_s, atol=ATOL, rtol=RTOL)
        # ... and summed in split order they are the whole product
        torch.testing.assert_close(rows.sum(0), ref_nb, atol=ATOL, rtol=RTOL)
    else:
        assert rows is None


@pytest.mark.parametrize("run", GOLDEN_RUNS, ids=_id)
def test_skinny_stream_bits_match_parent(results, golden, run):
    """Part b: bit-equal to the kernel before the rewrite. Config 2 is held
    to the config 1 record (the two are bit-equal by contract)."""
    name = run[0]
    out, rows = results[run]
    want = torch.from_numpy(golden[name + ".out"].view(np.int16))
    assert torch.equal(out.view(torch.int16).cpu(), want)
    if rows is not None:
        want = torch.from_numpy(golden[name + ".part"].view(np.int32))
        rows = G.recorded_rows(name, rows).contiguous()
        assert torch.equal(rows.view(torch.int32).cpu(), want)
    else:
        assert name + ".part" not in golden.files
