#!/usr/bin/env python
"""Time of the filter-plus-sample part of ModelRunner.sample for a batch of
top-k / top-p requests ("Sampling filters"): the torch filter
(_apply_top_p_top_k: sort, softmax, cumsum, a host loop over rows, scatter)
followed by the Gumbel sampler, against the cutoff kernel (topk_topp.hip)
followed by the sampler that consumes the cutoff.

Both variants start from the same bf16 logits, build their per-row tensors,
draw the noise and end in the .tolist() that synchronises the device, as
sample() does. They alternate inside one process, each warmed up and then
timed over a window of at least --window seconds, --repeats times. One JSON
line. Fails without a GPU; it never falls back.
"""

from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--vocab", type=int, default=152064)
    p.add_argument("--rows", type=int, nargs="+", default=[64, 256])
    p.add_argument("--temperature", type=float, default=0.7)
    p.add_argument("--top-p", type=float, default=0.8)
    p.add_argument("--top-k", type=int, default=20)
    p.add_argument("--window", type=float, default=1.0)
    p.add_argument("--repeats", type=int, default=3)
    args = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("this measurement needs a GPU")

    import arks_amd.ops as ops
    from arks_amd.engine.model_runner import ModelRunner
    from arks_amd.engine.sequence import SamplingParams, Sequence

    assert ops.native_available()
    sp = SamplingParams(temperature=args.temperature, top_p=args.top_p,
                        top_k=args.top_k)
    res = {"vocab": args.vocab, "temperature": sp.temperature,
           "top_p": sp.top_p, "top_k": sp.top_k, "window_s": args.window,
           "shapes": {}}
    for rows in args.rows:
        g = torch.Generator(device="cuda").manual_seed(rows)
        logits = (torch.randn(rows, args.vocab, device="cuda", generator=g)
                  * 3).bfloat16()
        seqs = [Sequence([1], sp) for _ in range(rows)]
        temps = [s.sampling.temperature for s in seqs]

        def old():
            lg = ModelRunner._apply_top_p_top_k(logits, seqs)
            t = torch.tensor(temps, dtype=torch.float32, device=lg.device)
            u = torch.rand(lg.shape, dtype=torch.float32, device=lg.device)
            return ops.sample_tokens(lg.contiguous(), t, u).tolist()

        def new():
            t = torch.tensor(temps, dtype=torch.float32, device=logits.device)
            cutoff = ops.sample_cutoff(logits, t, *ModelRunner._filter_tensors(
                [s.sampling for s in seqs], logits.device))
            u = torch.rand(logits.shape, dtype=torch.float32,
                           device=logits.device)
            return ops.sample_tokens(logits, t, u, cutoff=cutoff).tolist()

        def window(fn):
            n = 0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            while True:
                fn()  # ends in a device synchronise
                n += 1
                dt = time.perf_counter() - t0
                if dt >= args.window:
                    return dt / n * 1000.0

        fns = {"torch_filter": old, "cutoff_kernel": new}
        for fn in fns.values():
            for _ in range(3):
                fn()
        runs = {k: [] for k in fns}
        for _ in range(args.repeats):
            for k, fn in fns.items():
                runs[k].append(window(fn))
        res["shapes"][f"{rows}x{args.vocab}"] = {
            k: {"median_ms": round(statistics.median(v), 4),
                "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
            for k, v in runs.items()}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
