"""ref.sample_cutoff is the old filter wherever the old one was defined: on
tie-free rows away from a nucleus boundary its kept set equals the finite
mask of ModelRunner._apply_top_p_top_k."""

import pytest
import torch

from arks_amd.engine.model_runner import ModelRunner
from arks_amd.engine.sequence import SamplingParams, Sequence
from arks_amd.ops import ref

_RANDOM = (torch.randn(6, 257, generator=torch.Generator().manual_seed(5)) * 3)

CASES = [
    # test_min_p_filter
    ([[10.0, 9.9, 5.0, 1.0], [10.0, 9.9, 9.8, 9.7]],
     [dict(temperature=1.0, min_p=0.5),
      dict(temperature=1.0, min_p=0.5, top_k=2)]),
    # test_temperature_scales_top_p_nucleus
    ([[4.0, 2.0, 0.0, -2.0]] * 4,
     [dict(temperature=1.0, top_p=0.9), dict(temperature=5.0, top_p=0.9),
      dict(temperature=1.0, min_p=0.3), dict(temperature=8.0, min_p=0.3)]),
    (_RANDOM.tolist(),
     [dict(temperature=0.7, top_p=0.8, top_k=20), dict(temperature=1.5, top_p=0.5),
      dict(temperature=0.3, top_k=1000), dict(temperature=1.0, top_k=7, min_p=0.01),
      dict(temperature=0.0, top_p=0.5), dict(temperature=1.0)]),
]


@pytest.mark.parametrize("rows,params", CASES)
def test_cutoff_is_the_old_filter(rows, params):
    logits = torch.tensor(rows)
    sps = [SamplingParams(**p) for p in params]
    old = ModelRunner._apply_top_p_top_k(
        logits.clone(), [Sequence([1], sp) for sp in sps])
    pair = ref.sample_cutoff(
        logits, torch.tensor([sp.temperature for sp in sps]),
        torch.tensor([sp.top_k for sp in sps], dtype=torch.int32),
        torch.tensor([sp.top_p for sp in sps]),
        torch.tensor([sp.min_p for sp in sps]))
    assert pair[0].dtype == torch.float32 and pair[1].dtype == torch.int32
    keep = ref.cutoff_keep(logits, *pair)
    assert torch.equal(keep, torch.isfinite(old))
    assert torch.equal(ref.apply_sample_cutoff(logits.clone(), *pair), old)
