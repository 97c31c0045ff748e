"""A-resident skinny GEMM (skinny_gemm.hip, launch config 3).

The kernel keeps a workgroup's whole A slice in LDS and streams several
16-row slabs of W per wave, but an accumulator must still see the MFMA
sequence of config 0 for the same split boundaries. So every check but the
last is bit-equality: the split cases of scripts/skinny_stream_golden.py
against the bits recorded before the W-ring rewrite, and further shapes
against config 0 of the same build at the same (nsplits, k_per_split). The
`groups` argument (workgroups per split) lets small shapes reach what the
decode plan reaches at 7B sizes: several slabs per wave, every tail count of
the slab ring, uneven groups, waves and workgroups without a slab.

The last check compares with F.linear in fp32 on inputs of order 1, at the
tolerance and with the guard of test_skinny_stream_gpu.py.
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

# recorded split cases that fit config 3 (K-range <= 512)
GOLDEN_NAMES = ["split_448", "mt2_uneven", "mt1_splits", "strided"]

# name: ((M, N, K, 0, nsplits, k_per_split, a_stride or None), groups)
CASES = {
    # 36 slabs: nine per wave in one workgroup (the ring turns twice), two
    # workgroups of 18 (waves with 5 and 4), and groups of 8, 8, 8, 8, 4
    "n576_g1": ((64, 576, 896, 0, 2, 448, None), 1),
    "n576_g2": ((64, 576, 896, 0, 2, 448, None), 2),
    "n576_g5": ((64, 576, 896, 0, 2, 448, None), 5),
    # four slabs over eight workgroups: four of them have none, and in the
    # others three waves have none
    "n64_g8": ((17, 64, 512, 0, 2, 256, None), 8),
    # splits of 3, 3 and 1 chunks (the o_proj pattern)
    "k896_331": ((64, 128, 896, 0, 3, 384, None), 0),
    # the longest K-range (LDS above 64 KB at MT = 4) and the shortest
    "krange_512": ((64, 128, 1024, 0, 2, 512, None), 0),
    "krange_32": ((64, 64, 64, 0, 2, 32, None), 0),
    # every MT, M off the tile size
    "m1": ((1, 192, 896, 0, 2, 448, None), 0),
    "m17": ((17, 192, 896, 0, 2, 448, None), 0),
    "m33": ((33, 192, 896, 0, 2, 448, None), 0),
    "m49": ((49, 192, 896, 0, 2, 448, None), 0),
    "m64": ((64, 192, 896, 0, 2, 448, None), 0),
    # row-strided A
    "strided_a": ((64, 128, 768, 0, 2, 384, 1024), 0),
}
# One workgroup per split, N / 64 slabs per wave: every count of slabs left
# after the last full turn of the ring, for the ring of two slabs (K-ranges
# of 3-4 chunks) and of three (1-2 chunks; 160 ends in a 32-wide chunk).
for _kps in (448, 160):
    for _nsl in range(1, 8):
        CASES[f"tail_k{_kps}_s{_nsl}"] = (
            (16, 64 * _nsl, 2 * _kps, 0, 2, _kps, None), 1)


@pytest.fixture(scope="module")
def native():
    assert ops.native_available(), "HIP extension must be built on a GPU box"
    return ops._native()


@pytest.fixture(scope="module")
def golden():
    return np.load(G.GOLDEN)


@pytest.fixture(scope="module")
def golden_results(native):
    res = {name: G.run_case(native, G.CASES[name], DEV, 3)
           for name in GOLDEN_NAMES}
    torch.cuda.synchronize()
    return res


@pytest.fixture(scope="module")
def pair_results(native):
    """{name: (config 0 result, config 3 result)}, each (out, rows)."""
    res = {}
    for name, (case, groups) in CASES.items():
        res[name] = (G.run_case(native, case, DEV, 0),
                     G.run_case(native, case, DEV, 3, groups=groups))
    torch.cuda.synchronize()
    return res


@pytest.fixture(scope="module")
def unit_results(native):
    res = {name: G.run_case(native, case, DEV, 3, unit=True, groups=groups)
           for name, (case, groups) in CASES.items()}
    torch.cuda.synchronize()
    return res


@pytest.mark.parametrize("name", GOLDEN_NAMES)
def test_resident_bits_match_recorded(golden_results, golden, name):
    M, _N, _K, _cfg, _nsplits, kps, _ = G.CASES[name]
    assert kps <= ops._SKINNY_RESIDENT_KMAX
    out, rows = golden_results[name]
    want = torch.from_numpy(golden[name + ".out"].view(np.int16))
    assert torch.equal(out.view(torch.int16).cpu(), want)
    want = torch.from_numpy(golden[name + ".part"].view(np.int32))
    rows = G.recorded_rows(name, rows).contiguous()
    assert torch.equal(rows.view(torch.int32).cpu(), want)


@pytest.mark.parametrize("name", list(CASES))
def test_resident_bits_match_config0(pair_results, name):
    (out0, rows0), (out3, rows3) = pair_results[name]
    M, N, _K, _cfg, nsplits, _kps, _ = CASES[name][0]
    assert rows0.shape == rows3.shape == (nsplits, M, N)
    assert not torch.isnan(rows3).any()
    assert torch.equal(rows3.view(torch.int32), rows0.view(torch.int32))
    assert torch.equal(out3.view(torch.int16), out0.view(torch.int16))


ATOL = RTOL = 5e-2


@pytest.mark.parametrize("name", list(CASES))
def test_resident_matches_linear(unit_results, name):
    """fp32 F.linear on make_inputs(unit=True); the guard asserts first that
    a missing product would fail on over 90 % of the elements."""
    case = CASES[name][0]
    M, N, K, _cfg, nsplits, kps, a_stride = case
    out, rows = unit_results[name]
    a, w, bias = G.make_inputs(case, DEV, unit=True)
    if a_stride is not None:
        assert a.stride(0) == a_stride > K
    ref_nb = torch.nn.functional.linear(a.float(), w.float())
    assert ref_nb.abs().mean() > 5 * ATOL
    assert (ref_nb.abs() > ATOL + RTOL * ref_nb.abs()).float().mean() > 0.9
    ref = torch.nn.functional.linear(a.float(), w.float(), bias.float())
    torch.testing.assert_close(out.float(), ref, atol=ATOL, rtol=RTOL)
    assert rows.shape == (nsplits, M, N) and not torch.isnan(rows).any()
    for s in range(nsplits):
        ks = slice(s * kps, min(K, (s + 1) * kps))
        ref_s = torch.nn.functional.linear(a[:, ks].float(), w[:, ks].float())
        torch.testing.assert_close(rows[s], ref_s, atol=ATOL, rtol=RTOL)
    torch.testing.assert_close(rows.sum(0), ref_nb, atol=ATOL, rtol=RTOL)

