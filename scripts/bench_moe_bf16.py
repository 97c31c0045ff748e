"""Measure the routed bf16 MoE block against the library paths it replaces.

    python scripts/bench_moe_bf16.py [--rounds 5] [--ts 1,8,64,256,2048]
                                     [--out k.json]

One MoE block (router, experts, mix) of the qwen3-30b-a3b and mixtral-8x7b
shapes: MoEMLP._forward_routed over ops.moe_bf16_gemm against the parent path
on the SAME modules (MoEMLP._forward_bmm up to DENSE_TOKENS, _forward_sparse
above), inside one captured graph (T above DENSE_TOKENS syncs with the host
once per call on both paths and is timed eagerly). The method is
scripts/bench_w8_moe.py's: the paths cycle through enough copies of the block
that the bytes the ROUTED call touches exceed the 256 MB LLC twice over, they
alternate within each round, and the table shows the median and min..max of
the rounds (device-event times), the bytes of expert weights a call has to
read and the rate that makes.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import arks_amd.ops as ops  # noqa: E402
from arks_amd.config import PRESET_CONFIGS  # noqa: E402
from bench_w4 import LLC_BYTES, time_eager, time_graph  # noqa: E402
from bench_w4_moe import BLOCKS, make_block  # noqa: E402


def routed(blk, x):
    return blk._forward_routed(x, ops.moe_bf16_gemm, blk.w13, blk.w2)


def parent(blk, x):
    logits = torch.nn.functional.linear(x, blk.gate).float()
    weights, selected = ops.moe_topk(logits, blk.top_k, blk.norm_topk)
    if x.shape[0] <= blk.DENSE_TOKENS:
        return blk._forward_bmm(x, weights, selected)
    return blk._forward_sparse(x, weights, selected)


PATHS = {"parent": parent, "routed": routed}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--blocks", default=",".join(BLOCKS))
    ap.add_argument("--ts", default="1,8,64,256,2048")
    ap.add_argument("--max-copies", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available() or not ops.native_available():
        sys.exit("bench_moe_bf16 needs a GPU and the built extension")
    gen = torch.Generator(device="cuda").manual_seed(0)
    rows = []
    print(f"{'block':14} {'T':>5} {'path':7} {'copies':>6} {'us':>9} "
          f"{'min..max':>21} {'MB':>8} {'TB/s':>6}")
    for name in args.blocks.split(","):
        cfg = PRESET_CONFIGS[name]
        E, k = cfg.num_local_experts, cfg.num_experts_per_tok
        I = cfg.moe_intermediate_size or cfg.intermediate_size
        per_expert = 3 * I * cfg.hidden_size * 2
        blocks = []
        for T in map(int, args.ts.split(",")):
            x = torch.randn(T, cfg.hidden_size, dtype=torch.bfloat16,
                            device="cuda", generator=gen)
            # the parent streams every expert; the routed path at most the
            # T*k selected ones
            touched = {"parent": E * per_expert,
                       "routed": min(E, T * k) * per_expert}
            n = min(args.max_copies,
                    max(1, -(-2 * LLC_BYTES // touched["routed"])))
            while len(blocks) < n:
                blocks.append(make_block(cfg, False, gen))
            use = blocks[:n]
            assert use[0].bf16_routed_supported()
            graphs = {}
            if T <= use[0].DENSE_TOKENS:
                for path, fn in PATHS.items():
                    with torch.no_grad():
                        for b in use:
                            fn(b, x)
                        torch.cuda.synchronize()
                        g = torch.cuda.CUDAGraph()
                        with torch.cuda.graph(g):
                            for b in use:
                                fn(b, x)
                    graphs[path] = g
            res = {path: [] for path in PATHS}
            for _ in range(args.rounds):  # alternate the paths every round
                for path, fn in PATHS.items():
                    if path in graphs:
                        t = time_graph(graphs[path], n, max(3, 40 // n))
                    else:
                        with torch.no_grad():
                            t = time_eager(lambda b: fn(b, x), use,
                                           max(3 * n, 20))
                    res[path].append(t)
            for path, ts in res.items():
                med = statistics.median(ts)
                print(f"{name:14} {T:5d} {path:7} {n:6d} {med:9.1f} "
                      f"{min(ts):10.1f}..{max(ts):<10.1f}"
                      f"{touched[path] / 1e6:8.1f} "
                      f"{touched[path] / med / 1e6:6.2f}", flush=True)
                rows.append({"block": name, "T": T, "path": path,
                             "mode": "graph" if path in graphs else "eager",
                             "copies": n, "us_median": med,
                             "us_min": min(ts), "us_max": max(ts),
                             "touched_bytes": touched[path],
                             "rounds": len(ts)})
            del graphs
        del blocks
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
