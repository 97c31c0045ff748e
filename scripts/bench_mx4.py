"""Time ops.mx4_linear against ops.w4_linear and ops.linear_bf16 on the
Qwen2.5-7B decode shapes.

The W4 (AWQ-style) kernel is the yardstick: both stream half a byte per weight
through the same chunk loop, MX4 with 1/32 B of scale per weight against
3/128 B of scale and zero-point, so at M <= 64 an MX4 GEMM is expected to take
at most 1.03x the W4 time (the byte ratio 0.53125 / 0.5156) plus the W4
run-to-run spread. linear_bf16 is what the same model costs unquantized.

Same process, same activations, the paths alternating in every round so that
drift of the machine hits all of them. Each path cycles through enough copies
of its weight to exceed the 256 MB LLC, so a call streams its weight from HBM
as a decode step does. Times are device-event times over a window of many
calls inside one captured graph (--eager adds the eager times); the table
shows the median of the rounds, their min..max spread, and the effective
weight bandwidth (bytes of the weight as stored, over the median time). For
M <= 64 the last column checks the expectation above against the measured W4
spread (max - min over the rounds).

For M > 64 both MX4 routes are timed next to the one mx4_linear ships for
that M: the skinny kernel once per 64-row slab (mx4_slab) and dequantize into
the workspace + library GEMM (mx4_deq).

    python scripts/bench_mx4.py [--rounds 5] [--out results.json]
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
MS = (1, 8, 16, 32, 64, 128, 256)
LLC_BYTES = 256 << 20
BYTE_RATIO = 1.03  # (0.5 + 1/32) / (0.5 + 3/128)


def mx4_bytes(n, k):
    return n * k // 2 + n * (k // 32)


def w4_bytes(n, k):
    return n * k // 2 + (k // 128) * n * 3


def make_mx4(n, k, gen):
    """Random weight straight in the storage format: every nibble code, scale
    bytes around what the quantizer gives std-0.05 weights (amax of a block
    of 32 near 0.1: floor(log2 0.1) - 2 + 127 = 121); no quantization pass."""
    w = torch.randint(0, 256, (n, k // 2), dtype=torch.uint8, device="cuda",
                      generator=gen)
    scales = torch.randint(120, 123, (n, k // 32), dtype=torch.uint8,
                           device="cuda", generator=gen)
    return w, scales


def make_w4(n, k, gen):
    """As scripts/bench_w4.py: random packed W4 in the storage format."""
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
    ap.add_argument("--eager", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available() or not ops.native_available():
        sys.exit("bench_mx4 needs a GPU and the built extension")
    if args.rounds < 3:
        sys.exit("the W4 spread needs at least three rounds")
    gen = torch.Generator(device="cuda").manual_seed(0)
    modes = ("eager", "graph") if args.eager else ("graph",)
    rows = []
    print(f"{'shape':8} {'M':>4} {'mode':6} {'path':8} {'us':>9} "
          f"{'min..max':>19} {'GB/s':>8}  vs W4")
    for name in args.shapes.split(","):
        n, k = SHAPES[name]
        ncopy16 = -(-2 * LLC_BYTES // (n * k * 2))
        ncopy4 = -(-2 * LLC_BYTES // w4_bytes(n, k))
        w16 = [torch.randn(n, k, dtype=torch.bfloat16, device="cuda",
                           generator=gen) * 0.05 for _ in range(ncopy16)]
        w4 = [make_w4(n, k, gen) for _ in range(ncopy4)]
        mx4 = [make_mx4(n, k, gen) for _ in range(ncopy4)]
        ops.reserve_dequant_workspace(n * k, "cuda")
        for m in map(int, args.ms.split(",")):
            x = torch.randn(m, k, dtype=torch.bfloat16, device="cuda",
                            generator=gen) * 0.5
            paths = {
                "bf16": (lambda w: ops.linear_bf16(x, w), w16, n * k * 2),
                "w4": (lambda w: ops.w4_linear(x, w), w4, w4_bytes(n, k)),
                "mx4": (lambda w: ops.mx4_linear(x, w), mx4,
                        mx4_bytes(n, k)),
            }
            if m > 64:  # both routes, whichever mx4_linear ships for this M
                paths["mx4_slab"] = (
                    lambda w: ops._wq_slabs(ops._MX4, x, w, None), mx4,
                    mx4_bytes(n, k))
                paths["mx4_deq"] = (
                    lambda w: ops._wq_dequant_linear(ops._MX4, x, w, None),
                    mx4, mx4_bytes(n, k))
            graphs = {p: capture(fn, ws) for p, (fn, ws, _) in paths.items()}
            res = {(mode, p): [] for mode in modes for p in paths}
            for _ in range(args.rounds):  # alternate the paths every round
                for p, (fn, ws, _) in paths.items():
                    if args.eager:
                        calls = max(3 * len(ws), 60)
                        res[("eager", p)].append(time_eager(fn, ws, calls))
                    res[("graph", p)].append(
                        time_graph(graphs[p], len(ws),
                                   max(3, 60 // len(ws))))
            w4_ts = res[("graph", "w4")]
            bound = (statistics.median(w4_ts) * BYTE_RATIO
                     + max(w4_ts) - min(w4_ts))
            for (mode, p), ts in res.items():
                med = statistics.median(ts)
                gbs = paths[p][2] / med / 1e3
                verdict = ""
                if p == "mx4" and mode == "graph" and m <= 64:
                    verdict = (f"{'ok' if med <= bound else 'MISS'} "
                               f"(<= {bound:.1f})")
                print(f"{name:8} {m:4d} {mode:6} {p:8} {med:9.1f} "
                      f"{min(ts):9.1f}..{max(ts):<9.1f}{gbs:8.0f}  {verdict}",
                      flush=True)
                rows.append({"shape": name, "N": n, "K": k, "M": m,
                             "mode": mode, "path": p, "us_median": med,
                             "us_min": min(ts), "us_max": max(ts),
                             "weight_gbs": gbs, "rounds": len(ts),
                             "w4_bound_us": bound if verdict else None})
            del graphs
        del w16, w4, mx4
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
