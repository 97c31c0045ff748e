"""Time ops.w8_linear against ops.linear_bf16 on the Qwen2.5-7B decode shapes.

linear_bf16 on the dequantized weight is the route the engine took for a
block-scaled FP8 model before it could read the format (the bf16 release of
the same model), so it is the baseline.

Same process, same activations, alternating the two paths in every round so
that drift of the machine hits both. Each path cycles through enough copies
of its weight to exceed the 256 MB LLC, so a call streams its weight from HBM
as a decode step does. Times are device-event times over a window of many
calls, eager and inside one captured graph; the table shows the median of the
rounds and their min..max spread, and the effective weight bandwidth (bytes
of the weight as stored, over the median time).

For M > 64 both W8 routes are timed next to the one w8_linear ships for that
M: the skinny kernel once per 64-row slab (w8_slab) and dequantize into the
workspace + library GEMM (w8_deq), next to the fused-dequant MFMA GEMM with
64- and 128-row workgroup tiles (w8_a16t64 / w8_a16t128; TF/s = 2 M N K over
the median), whose output is first compared with w8_deq's on the same inputs
against the bound of tests/test_wqa16_gpu.py.

--a8 times the W8A8 mode instead, at prefill sizes (A8_MS rows): (a) w8 =
ops.w8_linear, the route a W8A16 layer takes at that M (slabs up to
W8_SLAB_MAX_M rows, dequantize + library GEMM above); (b) bf16 = the library
GEMM on bf16 weights; (c) quant = the activation quantizer alone; (d) gemm64 /
gemm128 = the FP8 MFMA GEMM alone on quantized activations with either tile
height, with the achieved FLOP/s (2 M N K over the time) and their share of
PEAK_FP8; (e) a8 = quantizer + MFMA GEMM with the shipped tile rule, what
ops.w8a8_linear runs from W8A8_MFMA_MIN_M rows. Same method: in-graph times,
weights cycled past the LLC, paths alternating every round.

    python scripts/bench_w8.py [--rounds 5] [--out results.json] [--a8]
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
MS = (1, 8, 32, 64, 96, 128, 256)
A8_MS = (64, 128, 129, 192, 256, 512, 2048, 8192)
LLC_BYTES = 256 << 20
# MI355X peak dense FP8 matrix rate, from AMD's published product
# specification of the Instinct MI355X (5.0 PFLOP/s)
PEAK_FP8 = 5.0e15


def w8_bytes(n, k):
    return n * k + (k // 128) * n * 4


def make_w8(n, k, gen):
    """Random weight straight in the storage format: every byte a finite
    e4m3 code (the two NaN codes are remapped), scales of the size a
    quantizer of std-0.05 weights would give; no quantization pass."""
    b = torch.randint(0, 256, (n, k), dtype=torch.uint8, device="cuda",
                      generator=gen)
    b[(b & 0x7F) == 0x7F] = 0x38
    scales = torch.full((k // 128, n), 0.2 / 448, dtype=torch.float32,
                        device="cuda")
    return b.view(torch.float8_e4m3fn), scales


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


def main_a8(args):
    gen = torch.Generator(device="cuda").manual_seed(0)
    rows = []
    print(f"{'shape':8} {'M':>5} {'path':8} {'us':>10} {'min..max':>21} "
          f"{'TFLOP/s':>8} {'of peak':>8}")
    for name in args.shapes.split(","):
        n, k = SHAPES[name]
        ncopy16 = -(-2 * LLC_BYTES // (n * k * 2))
        ncopy8 = -(-2 * LLC_BYTES // w8_bytes(n, k))
        w16 = [torch.randn(n, k, dtype=torch.bfloat16, device="cuda",
                           generator=gen) * 0.05 for _ in range(ncopy16)]
        w8 = [make_w8(n, k, gen) for _ in range(ncopy8)]
        ops.reserve_dequant_workspace(n * k, "cuda")
        for m in map(int, args.ms.split(",")):
            x = torch.randn(m, k, dtype=torch.bfloat16, device="cuda",
                            generator=gen) * 0.5
            xq, xs = ops.w8_quantize_act(x)
            paths = {
                "w8": (lambda w: ops.w8_linear(x, w), w8),
                "bf16": (lambda w: ops.linear_bf16(x, w), w16),
                "quant": (lambda w: ops.w8_quantize_act(x), w8[:1] * 8),
                "gemm64": (lambda w: ops.w8a8_gemm(xq, xs, w, mtile=64), w8),
                "gemm128": (lambda w: ops.w8a8_gemm(xq, xs, w, mtile=128),
                            w8),
                "a8": (lambda w: ops.w8a8_gemm(*ops.w8_quantize_act(x), w),
                       w8),
            }
            # every path once before the first capture: the split-K workspace
            # that w8_linear and linear_bf16 share grows to the larger of
            # their needs here, so no graph keeps a pointer that a later
            # path's warm-up would have freed
            for fn, ws in paths.values():
                fn(ws[0])
            torch.cuda.synchronize()
            graphs = {p: capture(fn, ws) for p, (fn, ws) in paths.items()}
            res = {p: [] for p in paths}
            for _ in range(args.rounds):  # alternate the paths every round
                for p, (fn, ws) in paths.items():
                    res[p].append(time_graph(graphs[p], len(ws),
                                             max(3, 60 // len(ws))))
            for p, ts in res.items():
                med = statistics.median(ts)
                flops = (2 * m * n * k / (med * 1e-6)
                         if p.startswith("gemm") else None)
                tail = (f"{flops / 1e12:8.0f} {flops / PEAK_FP8:8.1%}"
                        if flops else "")
                print(f"{name:8} {m:5d} {p:8} {med:10.1f} "
                      f"{min(ts):10.1f}..{max(ts):<10.1f}{tail}", flush=True)
                rows.append({"shape": name, "N": n, "K": k, "M": m, "path": p,
                             "us_median": med, "us_min": min(ts),
                             "us_max": max(ts), "flops": flops,
                             "rounds": len(ts)})
            del graphs
        del w16, w8
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


def check_a16(name, m, x, wd, y_old, *ys_new):
    """Old route (dequant + library) against the fused GEMM on the same
    inputs: max |new - old| over the bound of two f32 summation orders."""
    y, t = y_old.float(), x.float().abs() @ wd.float().abs().t()
    tol = 2.0 ** -8 * y.abs() + x.shape[1] * 2.0 ** -23 * t
    worst = max(((o.float() - y).abs() / tol).max().item() for o in ys_new)
    print(f"{name:8} {m:4d} a16 vs deq: max |diff| / bound = {worst:.3f}",
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--ms", default=None)
    ap.add_argument("--a8", action="store_true",
                    help="time the W8A8 mode at prefill sizes instead")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available() or not ops.native_available():
        sys.exit("bench_w8 needs a GPU and the built extension")
    args.ms = args.ms or ",".join(map(str, A8_MS if args.a8 else MS))
    if args.a8:
        return main_a8(args)
    gen = torch.Generator(device="cuda").manual_seed(0)
    rows = []
    print(f"{'shape':8} {'M':>4} {'mode':6} {'path':10} {'us':>9} "
          f"{'min..max':>19} {'GB/s':>8} {'TF/s':>7}")
    for name in args.shapes.split(","):
        n, k = SHAPES[name]
        ncopy16 = -(-2 * LLC_BYTES // (n * k * 2))
        ncopy8 = -(-2 * LLC_BYTES // w8_bytes(n, k))
        w16 = [torch.randn(n, k, dtype=torch.bfloat16, device="cuda",
                           generator=gen) * 0.05 for _ in range(ncopy16)]
        w8 = [make_w8(n, k, gen) for _ in range(ncopy8)]
        ops.reserve_dequant_workspace(n * k, "cuda")
        for m in map(int, args.ms.split(",")):
            x = torch.randn(m, k, dtype=torch.bfloat16, device="cuda",
                            generator=gen) * 0.5
            paths = {
                "bf16": (lambda w: ops.linear_bf16(x, w), w16, n * k * 2),
                "w8": (lambda w: ops.w8_linear(x, w), w8, w8_bytes(n, k)),
            }
            if m > 64:  # both routes, whichever w8_linear ships for this M
                paths["w8_slab"] = (
                    lambda w: ops._wq_slabs(ops._W8, x, w, None), w8,
                                    w8_bytes(n, k))
                paths["w8_deq"] = (
                    lambda w: ops._wq_dequant_linear(ops._W8, x, w, None), w8,
                    w8_bytes(n, k))
                for mt in (64, 128):
                    paths[f"w8_a16t{mt}"] = (
                        lambda w, mt=mt: ops.w8a16_gemm(x, w, mtile=mt), w8,
                        w8_bytes(n, k))
                check_a16(name, m, x, ops.w8_dequant(w8[0]),
                          paths["w8_deq"][0](w8[0]),
                          paths["w8_a16t64"][0](w8[0]),
                          paths["w8_a16t128"][0](w8[0]))
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
                tfs = 2 * m * n * k / med / 1e6
                print(f"{name:8} {m:4d} {mode:6} {p:10} {med:9.1f} "
                      f"{min(ts):9.1f}..{max(ts):<9.1f}{gbs:8.0f} {tfs:7.1f}",
                      flush=True)
                rows.append({"shape": name, "N": n, "K": k, "M": m,
                             "mode": mode, "path": p, "us_median": med,
                             "us_min": min(ts), "us_max": max(ts),
                             "weight_gbs": gbs, "tflops": tfs,
                             "rounds": len(ts)})
            del graphs
        del w16, w8
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
