"""Routing of the tall-K plan to 112-row tiles (ops._skinny_tallk7_config).

_skinny_plan is pinned by test_skinny_plan_cpu.py; this step only moves a
config-1 plan to launch config 4, and only where 112-row tiles put work on
more compute units than 128-row tiles without exceeding one workgroup each.
"""

import arks_amd.ops as ops

CUS = 256


def _route(M, N, K, cus=CUS):
    config, nsplits, kps, mrows = ops._skinny_plan(M, N, K)
    config = ops._skinny_resident_config(config, M, nsplits, kps)
    return ops._skinny_tallk7_config(config, N, nsplits, cus), nsplits, kps, mrows


def test_down_proj_takes_112_row_tiles():
    # 3584 / 112 * 8 = 256 workgroups, against 28 * 8 = 224
    assert _route(64, 3584, 18944) == (4, 8, 2368, 64)


def test_switch_restores_128_row_tiles(monkeypatch):
    monkeypatch.setattr(ops, "_TALLK_WAVES", "8")
    assert _route(64, 3584, 18944) == (1, 8, 2368, 64)


def test_unchanged_plans():
    # M <= 48 is not a tall-K plan
    plan = ops._skinny_plan(48, 3584, 18944)
    assert plan[0] == 0
    assert _route(48, 3584, 18944) == plan
    # a multiple of 64 that is not a multiple of 112
    plan = ops._skinny_plan(64, 3520, 18944)
    assert plan[0] == 1
    assert _route(64, 3520, 18944) == plan
    # config-0 plans, with and without the A-resident step
    assert _route(64, 4608, 3584)[0] == 3
    assert _route(64, 152064, 3584)[0] == 0
    # more workgroups than compute units
    assert _route(64, 3584, 18944, cus=255)[0] == 1
    # config 2 (non-temporal) stays
    assert ops._skinny_tallk7_config(2, 3584, 8, CUS) == 2
