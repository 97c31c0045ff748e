"""One-round add-RMSNorm consumer of split-K partials (elementwise.hip).

Rows of up to 4096 columns take splitk_add_rmsnorm_wide_kernel (one 8-column
vector per thread, every load up front, the row kept in registers); wider
rows stay on splitk_add_rmsnorm_kernel. Either way the output and the new
residual must be the bits of the unfused pair: materialize() (the combine
kernel) followed by fused_add_rmsnorm. hidden 8192 is here because the wide
kernel, taken by mistake, would leave the upper half of such a row unwritten.

The partials are made up (no GEMM runs), so that the split count is free:
2, 8 and 10 are one round of splitk_reduce's loads, 17 is a second round.
Partial rows past M are NaN; no kernel may read them.
"""

import pytest
import torch

import arks_amd.ops as ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS = 1e-6


def _pending(part, nsplits, mrows, rows, hidden, bias):
    """A live SplitKPending over hand-made partials."""
    key = (torch.cuda.current_device(),)
    ops._SKINNY_WS_GEN[key] = ops._SKINNY_WS_GEN.get(key, 0) + 1
    return ops.SplitKPending(part, nsplits, mrows, rows, hidden, bias, key)


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("rows", [1, 5, 64])
@pytest.mark.parametrize("nsplits", [2, 8, 10, 17])
@pytest.mark.parametrize("hidden", [64, 2048, 3584, 4096, 8192])
def test_splitk_norm_bit_equal_to_unfused(hidden, nsplits, rows, with_bias):
    assert ops.native_available(), "HIP extension must be built on a GPU box"
    gen = torch.Generator(device=DEV)
    gen.manual_seed(hidden * 131 + nsplits * 17 + rows)
    mrows = -(-rows // 16) * 16
    part = torch.randn(nsplits, mrows, hidden, dtype=torch.float32,
                       device=DEV, generator=gen)
    part[:, rows:, :] = float("nan")
    part = part.reshape(-1)
    bias = (torch.randn(hidden, device=DEV, generator=gen).to(torch.bfloat16)
            if with_bias else None)
    res = torch.randn(rows, hidden, device=DEV,
                      generator=gen).to(torch.bfloat16)
    weight = torch.randn(hidden, device=DEV, generator=gen).to(torch.bfloat16)

    res_ref = res.clone()
    y = _pending(part, nsplits, mrows, rows, hidden, bias).materialize()
    out_ref, _ = ops.fused_add_rmsnorm(y, res_ref, weight, EPS)

    res_new = res.clone()
    h = _pending(part, nsplits, mrows, rows, hidden, bias)
    out_new, res_out = ops.fused_add_rmsnorm(h, res_new, weight, EPS)
    assert res_out is res_new
    assert not torch.isnan(out_new.float()).any()
    assert torch.equal(res_new.view(torch.int16), res_ref.view(torch.int16))
    assert torch.equal(out_new.view(torch.int16), out_ref.view(torch.int16))
