"""Split-K RoPE + cache consumer over (token, group) (kvcache.hip).

splitk_rope_cache_kernel spreads a token's rotation and v items over several
workgroups when the tokens alone leave compute units idle. No item needs
another, so q and the written K and V cache slots must be bit-equal to the
one-workgroup-per-token launch (groups = 1), which stays reachable through
the groups argument. The partials are synthetic: the kernel only sums them in
split order, so any f32 values do.
"""

import pytest
import torch

import arks_amd.ops as ops
from arks_amd.ops import ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
MROWS = 16
GROUPS = (2, 4, 7, 64)  # 64 is past what the launcher grants: it clamps


def _run(native, groups, T, hq, hkv, hd, nsplits, bias, fp8, part, pos, slots,
         cos_sin):
    dt = torch.float8_e4m3fn if fp8 else torch.bfloat16
    kc = torch.zeros(8, hkv, 16, hd, dtype=dt, device=DEV)
    vc = torch.zeros_like(kc)
    # NaN bits: an element the launch does not write stays visible
    q = torch.full((T, hq * hd), float("nan"), dtype=torch.bfloat16, device=DEV)
    native.splitk_rope_and_cache(pos, part, bias, q, kc, vc, slots, cos_sin,
                                 hd, nsplits, MROWS, groups)
    return q.view(torch.int16), kc.view(torch.uint8), vc.view(torch.uint8)


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("nsplits", [1, 8, 10])
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("hq,hkv", [(28, 4), (4, 4)])
def test_groups_bit_equal(hq, hkv, hd, nsplits, with_bias, fp8):
    assert ops.native_available(), "HIP extension must be built on a GPU box"
    native = ops._native()
    torch.manual_seed(7)
    n = (hq + 2 * hkv) * hd
    cos_sin = ref.rope_cos_sin_cache(hd, 64, 10000.0).to(DEV)
    bias = (torch.randn(n, dtype=torch.bfloat16, device=DEV)
            if with_bias else None)
    for T in (1, 5):
        part = torch.randn(nsplits, MROWS, n, dtype=torch.float32, device=DEV)
        pos = torch.randint(0, 64, (T,), dtype=torch.int64, device=DEV)
        # T = 5: token 2 has no cache slot
        slots = torch.tensor([-1 if (T > 1 and i == 2) else 5 + i * 3
                              for i in range(T)], dtype=torch.int64, device=DEV)
        args = (T, hq, hkv, hd, nsplits, bias, fp8, part, pos, slots, cos_sin)
        q1, k1, v1 = _run(native, 1, *args)
        assert k1.any() and v1.any()
        for groups in GROUPS:
            q, k, v = _run(native, groups, *args)
            assert torch.equal(q, q1), (T, groups)
            assert torch.equal(k, k1), (T, groups)
            assert torch.equal(v, v1), (T, groups)


def test_default_group_count():
    assert ops._rope_splitk_groups(64, 256) == 4
    assert ops._rope_splitk_groups(1, 256) == 256
    assert ops._rope_splitk_groups(256, 256) == 1
    assert ops._rope_splitk_groups(1000, 256) == 1
