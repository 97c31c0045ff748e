"""The shared streaming chunk loop of the quantized GEMMs (wq_stream.h):
dense W4, dense W8 and the routed W4 expert kernel.

Every case of scripts/wq_stream_golden.py is launched once and its bits are
compared with the ones recorded from the three separate kernel bodies that
the shared loop replaced (tests/golden/wq_stream/): each accumulator must
still see the same MFMA sequence over ascending k within a chunk, the same
FMA nesting in the scale step and the same split boundaries. The routed
outputs are recorded whole over a sentinel fill, so rows of no local expert
are held to "not written". Tolerance tests of the same kernels are in
test_w4_gpu.py, test_w8_gpu.py and test_w4_moe_gpu.py.
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
    path = os.path.join(ROOT, "scripts", "wq_stream_golden.py")
    spec = importlib.util.spec_from_file_location("wq_stream_golden", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _load_golden_script()
DENSE_RUNS = [(fmt, name) for fmt in G.FORMATS for name in G.DENSE_CASES]


@pytest.fixture(scope="module")
def native():
    assert ops.native_available(), "HIP extension must be built on a GPU box"
    return ops._native()


@pytest.fixture(scope="module")
def dense_results(native):
    """Every dense run once: {(fmt, name): (out, partial rows or None)}."""
    res = {run: G.run_dense(native, *run, DEV) for run in DENSE_RUNS}
    torch.cuda.synchronize()
    return res


@pytest.fixture(scope="module")
def routed_results(native):
    res = {name: G.run_routed(ops, name, DEV) for name in G.ROUTED_CASES}
    torch.cuda.synchronize()
    return res


@pytest.fixture(scope="module")
def golden_dense():
    return np.load(G.DENSE)


@pytest.fixture(scope="module")
def golden_routed():
    return np.load(G.ROUTED)


def test_every_recorded_array_is_checked(golden_dense, golden_routed):
    want = {f"{fmt}.{name}.out" for fmt, name in DENSE_RUNS}
    want |= {f"{fmt}.{name}.part" for fmt, name in DENSE_RUNS
             if G.DENSE_CASES[name][4] > 1}
    assert set(golden_dense.files) == want
    assert set(golden_routed.files) == {n + ".out" for n in G.ROUTED_CASES}


@pytest.mark.parametrize("run", DENSE_RUNS, ids="-".join)
def test_dense_bits_match_parent(dense_results, golden_dense, run):
    fmt, name = run
    M, N, _K, _nw, nsplits, _kps, _bias, _stride = G.DENSE_CASES[name]
    out, rows = dense_results[run]
    want = torch.from_numpy(golden_dense[f"{fmt}.{name}.out"].view(np.int16))
    assert want.shape == (M, N)
    assert torch.equal(out.view(torch.int16).cpu(), want)
    if nsplits > 1:
        want = torch.from_numpy(
            golden_dense[f"{fmt}.{name}.part"].view(np.int32))
        assert want.shape == (nsplits, M, N)
        assert torch.equal(rows.contiguous().view(torch.int32).cpu(), want)
    else:
        assert rows is None


@pytest.mark.parametrize("name", list(G.ROUTED_CASES))
def test_routed_bits_match_parent(routed_results, golden_routed, name):
    _sd, T, top_k, N, _K, n0, n1 = G.ROUTED_CASES[name]
    out, counts, _pairs = routed_results[name]
    assert counts.tolist() == [n0, n1, 0]
    want = torch.from_numpy(golden_routed[name + ".out"].view(np.int16))
    assert want.shape == (T * top_k, N)
    # the record itself keeps the sentinel in the rows of no local expert
    ids = G.routed_ids(name).reshape(-1)
    foreign = (ids < G.EXPERT_BASE) | (ids >= G.EXPERT_BASE + G.N_LOCAL)
    sentinel = torch.tensor(G.SENTINEL, dtype=torch.bfloat16).view(torch.int16)
    assert foreign.any() and (want[foreign] == sentinel).all()
    assert not (want[~foreign] == sentinel).all(dim=1).any()
    assert torch.equal(out.view(torch.int16).cpu(), want)
