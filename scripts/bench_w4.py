"""Time ops.w4_linear against ops.linear_bf16 on the Qwen2.5-7B decode shapes.

Same process, same activations, alternating the two paths in every round so
that drift of the machine hits both. Each path cycles through enough copies
of its weight to exceed the 256 MB LLC, so a call streams its weight from HBM
as a decode step does. Times are device-event times over a window of many
calls, eager and inside one captured graph; the table shows the median of the
rounds and their min..max spread, and the effective weight bandwidth (bytes
of the weight as stored, over the median time).

For M > 64 both W4 routes are timed next to the one w4_linear ships for that
M: the skinny kernel once per 64-row slab (w4_slab) and dequantize into the
workspace + library GEMM (w4_deq).

    python scripts/bench_w4.py [--rounds 5] [--out results.json]
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import arks_amd.ops as ops  # noqa: E402

SHAPES = {  # name: (N, K)
    "qkv": (4608, 3584),
    "o": (3584, 3584),
    "gate_up": (37888, 3584),
    "down": (3584, 18944),
}
MS = (1, 16, 64, 128, 256)
LLC_BYTES = 256 << 20


def w4_bytes(n, k):
    return n * k // 2 + (k // 128) * n * 3


def make_w4(n, k, gen):
    """Random packed weight straight in the storage format (values are what
    a quantizer of std-0.05 weights would give; no quantization pass)."""
    qw = torch.randint(-2**31, 2**31 - 1, (n, k // 8), dtype=torch.int32,
                       device="cuda", generator=gen)
    scales = torch.full((k // 128, n), 0.0077, dtype=torch.float16,
                        device="cuda")
    zeros = torch.randint(0, 16, (k // 128, n), dtype=torch.uint8,
                          device="cuda", generator=gen)
    return qw, scales, zeros



def time_eager(fn, weights, calls):
    for w in weights:  # warm every copy
        fn(w)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(
        enable_timing=True)
    t0.record()
    for i in range(calls):
        fn(weights[i % len(weights)])
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3 / calls  # us per call


def capture(fn, weights):
    for w in weights:
        fn(w)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for w in weights:
            fn(w)
    return g


def time_graph(g, ncalls, replays):
    g.replay()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(
        enable_timing=True)
    t0.record()
    for _ in range(replays):
        g.replay()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3 / (replays * ncalls)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--ms", default=",".join(map(str, MS)))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available() or not ops.native_available():
        sys.exit("bench_w4 needs a GPU and the built extension")
    gen = torch.Generator(device="cuda").manual_seed(0)
    rows = []
    print(f"{'shape':8} {'M':>4} {'mode':6} {'path':8} {'us':>9} "
          f"{'min..max':>19} {'GB/s':>8}")
    for name in args.shapes.split(","):
        n, k = SHAPES[name]
        ncopy16 = -(-2 * LLC_BYTES // (n * k * 2))
        ncopy4 = -(-2 * LLC_BYTES // w4_bytes(n, k))
        w16 = [torch.randn(n, k, dtype=torch.bfloat16, device="cuda",
                           generator=gen) * 0.05 for _ in range(ncopy16)]
        w4 = [make_w4(n, k, gen) for _ in range(ncopy4)]
        ops.reserve_dequant_workspace(n * k, "cuda")
        for m in map(int, args.ms.split(",")):
            x = torch.randn(m, k, dtype=torch.bfloat16, device="cuda",
                            generator=gen) * 0.5
            paths = {
                "bf16": (lambda w: ops.linear_bf16(x, w), w16, n * k * 2),
                "w4": (lambda w: ops.w4_linear(x, w), w4, w4_bytes(n, k)),
            }
            if m > 64:  # both routes, whichever w4_linear ships for this M
                paths["w4_slab"] = (
                    lambda w: ops._wq_slabs(ops._W4, x, w, None), w4,
                                    w4_bytes(n, k))
                paths["w4_deq"] = (
                    lambda w: ops._wq_dequant_linear(ops._W4, x, w, None), w4,
                    w4_bytes(n, k))
            graphs = {p: capture(fn, ws) for p, (fn, ws, _) in paths.items()}
            res = {(mode, p): [] for mode in ("eager", "graph")
                   for p in paths}
            for _ in range(args.rounds):  # alternate the paths every round
                for p, (fn, ws, _) in paths.items():
                    calls = max(3 * len(ws), 60)
                    res[("eager", p)].append(time_eager(fn, ws, calls))
                    res[("graph", p)].append(
                        time_graph(graphs[p], len(ws),
                                   max(3, 60 // len(ws))))
            for (mode, p), ts in res.items():
                med = statistics.median(ts)
                gbs = paths[p][2] / med / 1e3
                print(f"{name:8} {m:4d} {mode:6} {p:8} {med:9.1f} "
                      f"{min(ts):9.1f}..{max(ts):<9.1f}{gbs:8.0f}",
                      flush=True)
                rows.append({"shape": name, "N": n, "K": k, "M": m,
                             "mode": mode, "path": p, "us_median": med,
                             "us_min": min(ts), "us_max": max(ts),
                             "weight_gbs": gbs, "rounds": len(ts)})
            del graphs
        del w16, w4
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
