"""Tall-K skinny GEMM on 112-row tiles (launch config 4, skinny_gemm.hip).

Config 4 runs skinny_gemm_kernel<4, false, 7>: seven waves per workgroup, so
the cooperative A staging takes three passes of 28 rows and the third runs
past row 63. A wave's MFMA sequence does not depend on the number of waves,
so partials and outputs must be bit-equal to config 1's (eight waves, 128-row
tiles) in the same build; config 1 itself is pinned to recorded bits by
test_skinny_stream_gpu.py. The cases also compare with F.linear in fp32 at
that file's tolerance, on its order-1 inputs.

Cases go through scripts/skinny_stream_golden.py::run_case with an explicit
config, like test_skinny_stream_gpu.py.
"""

import importlib.util
import os

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

# name: (M, N, K, config, nsplits, k_per_split, a_stride or None); the config
# field is overridden per run
CASES = {
    # 9.25 chunks per split: the ring wraps, short tail chunk
    "wrap": (64, 112, 2368, 1, 2, 1184, None),
    # one chunk, two tiles, direct epilogue
    "one_chunk_direct": (64, 224, 128, 1, 1, 128, None),
    # 192 = 112 + 80: the last tile hangs over, 5 of its 7 waves live
    "overhang": (49, 192, 384, 1, 2, 192, None),
    # the tile is wider than N
    "wide_tile": (50, 64, 160, 1, 1, 160, None),
    # M = 1: every staging pass clamps its rows
    "m1": (1, 112, 256, 1, 2, 128, None),
    # row-strided A
    "strided": (64, 112, 512, 1, 1, 512, 640),
}
# every tail count of the drain switch: t chunks, the last one 96 wide
for _t in range(1, 8):
    CASES[f"tail{_t}"] = (64, 112, 128 * _t - 32, 1, 1, 128 * _t - 32, None)

ATOL = RTOL = 5e-2  # test_skinny_stream_gpu.py


@pytest.fixture(scope="module")
def native():
    assert ops.native_available(), "HIP extension must be built on a GPU box"
    return ops._native()


@pytest.fixture(scope="module")
def results(native):
    """{(name, config, unit): (out, partial rows or None)}, every run once."""
    res = {}
    for name, case in CASES.items():
        for config in (1, 4):
            res[(name, config, False)] = G.run_case(native, case, DEV, config)
        res[(name, 4, True)] = G.run_case(native, case, DEV, 4, unit=True)
    torch.cuda.synchronize()
    return res


@pytest.mark.parametrize("name", list(CASES))
def test_tallk7_bits_match_config1(results, name):
    out1, rows1 = results[(name, 1, False)]
    out4, rows4 = results[(name, 4, False)]
    assert torch.equal(out4.view(torch.int16), out1.view(torch.int16))
    if CASES[name][4] > 1:
        assert not torch.isnan(rows4).any()
        assert torch.equal(rows4.view(torch.int32), rows1.view(torch.int32))
    else:
        assert rows1 is None and rows4 is None


@pytest.mark.parametrize("name", list(CASES))
def test_tallk7_matches_linear(results, name):
    case = CASES[name]
    M, N, K, _config, nsplits, kps, a_stride = case
    out, rows = results[(name, 4, True)]
    a, w, bias = G.make_inputs(case, DEV, unit=True)
    if a_stride is not None:
        assert a.stride(0) == a_stride > K
    ref_nb = torch.nn.functional.linear(a.float(), w.float())
    # a missing product would not hide inside the tolerance
    assert ref_nb.abs().mean() > 5 * ATOL
    ref = torch.nn.functional.linear(a.float(), w.float(), bias.float())
    torch.testing.assert_close(out.float(), ref, atol=ATOL, rtol=RTOL)
    if nsplits > 1:
        assert rows.shape == (nsplits, M, N)
        for s in range(nsplits):
            ks = slice(s * kps, min(K, (s + 1) * kps))
            ref_s = torch.nn.functional.linear(a[:, ks].float(),
                                               w[:, ks].float())
            torch.testing.assert_close(rows[s], ref_s, atol=ATOL, rtol=RTOL)
