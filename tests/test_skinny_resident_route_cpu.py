"""Second routing step of the skinny GEMM (ops._skinny_resident_config):
short-K split-K plans of config 0 go to the A-resident kernel, launch
config 3, with _skinny_plan's split and slab height unchanged. No GPU and no
extension needed."""

import arks_amd.ops as ops


def test_decode_shapes_route_to_config3(monkeypatch):
    """The second routing step keeps _skinny_plan's split and slab height."""
    monkeypatch.setattr(ops, "_SKINNY_RESIDENT", True)
    for shape in [(64, 4608, 3584), (64, 3584, 3584)]:
        config, nsplits, kps, _mrows = ops._skinny_plan(*shape)
        assert config == 0
        assert ops._skinny_resident_config(config, shape[0], nsplits, kps) == 3
    # unsplit, long K-ranges and the tall-K plan stay where they were
    assert ops._skinny_resident_config(0, 64, 1, 448) == 0
    assert ops._skinny_resident_config(0, 64, 4, 7168) == 0
    assert ops._skinny_resident_config(1, 64, 8, 2368) == 1
    monkeypatch.setattr(ops, "_SKINNY_RESIDENT", False)
    assert ops._skinny_resident_config(0, 64, 8, 448) == 0
