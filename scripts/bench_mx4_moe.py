"""Measure MX4 (MXFP4) MoE experts against the bf16 MoE block.

    python scripts/bench_mx4_moe.py [--rounds 5] [--ts 1,8,64,256,512,2048]
                                    [--out rows.json]

One MoE block (MoEMLP.forward: router, experts, mix) of the qwen3-30b-a3b and
mixtral-8x7b shapes. Paths:
  bf16     the block as an MXFP4 checkpoint's experts were held before MX4
           storage: dequantized to bf16 at load
  mx4      MX4 experts, bf16 activations (mx4_moe_gemm_kernel at every T,
           as before the fused-dequant MFMA kernel existed)
  mx4-64   the same above MoEMLP.DENSE_TOKENS on wqa16_moe_mfma_gemm_kernel
  mx4-128  forced to 64- / 128-row workgroups (with --grid-orders also
           mx4-64s / mx4-128s: the grid order (slabs, N tiles, experts))
  a4       MX4 experts, MXFP4 activations, T <= MoEMLP.MX4A4_MFMA_TOKENS
           (quantize-expand, then mx4_moe_gemm_kernel)
  a4-64    the same above it: mx4_moe_mfma_gemm_kernel forced to 64-row
  a4-128   and to 128-row workgroups
The method is scripts/bench_w8_moe.py's: inside one captured graph up to
MoEMLP.DENSE_TOKENS (above it every path syncs with the host once per call
and is timed eagerly), each path cycling through enough copies of the block
that the bytes a call touches exceed the 256 MB LLC twice over, the paths
alternating within each round, median and min..max of the rounds
(device-event times).
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
from bench_w4_moe import BLOCKS, quant_paths, run_path  # noqa: E402
from bench_w4_moe import make_block as make_bf16_block  # noqa: E402

TS = (1, 8, 64, 256, 512, 2048)


def expert_bytes(cfg, mx4: bool) -> int:
    """Stored bytes of ONE expert (w13 + w2): a nibble per weight plus one
    scale byte per 32, or bf16."""
    H = cfg.hidden_size
    I = cfg.moe_intermediate_size or cfg.intermediate_size
    return 3 * I * H * 17 // 32 if mx4 else 3 * I * H * 2


def make_block(cfg, mx4: bool, gen):
    """A MoEMLP built on the GPU with random weights; the MX4 one is filled
    straight in the storage format (random codes and scale bytes, no
    quantization pass)."""
    if not mx4:
        return make_bf16_block(cfg, False, gen)
    from arks_amd.models.llama_family import MoEMLP

    with torch.device("cuda"):
        blk = MoEMLP(cfg)
    blk.gate.data.normal_(0, 0.5, generator=gen)
    if blk.shared is not None:
        raise SystemExit("the bench covers blocks without a shared expert")
    blk.init_mx4("bench")
    for which in ("w13", "w2"):
        q, sc = blk.mx4_weight(which)
        q.random_(0, 256, generator=gen)
        sc.random_(118, 122, generator=gen)
    blk._mx4_got = None  # filled here, nothing streams in
    return blk


def paths_for(T: int, boundary: int, dense_tokens: int, grid_orders: bool):
    return (("bf16",) + quant_paths("mx4", T, dense_tokens, grid_orders)
            + (("a4",) if T <= boundary else ("a4-64", "a4-128")))


def run(blk, x, path):
    """One forward of blk on the given path (the tile height is forced
    through the rule's constant, the block's only way to the MFMA kernel)."""
    if path.startswith("a4"):
        blk.mx4_act = "mxfp4"
        ops._MX4A4_TILE128_MIN_WGS = 1 << 30 if path == "a4-64" else 0
        return blk(x)
    blk.mx4_act = "bf16"
    return run_path(blk, x, path)


def bench(args):
    from arks_amd.models.llama_family import MoEMLP

    rule = ops._MX4A4_TILE128_MIN_WGS
    rules = ops._WQA16_MOE_TILE128_MIN_WGS, ops._WQA16_MOE_SLAB_MAJOR
    gen = torch.Generator(device="cuda").manual_seed(0)
    rows = []
    print(f"{'block':14} {'T':>4} {'path':8} {'mode':5} {'copies':>6} "
          f"{'us':>9} {'min..max':>21} {'touched MB':>10}")
    for name in args.blocks.split(","):
        cfg = PRESET_CONFIGS[name]
        E, k = cfg.num_local_experts, cfg.num_experts_per_tok
        for T in map(int, args.ts.split(",")):
            x = torch.randn(T, cfg.hidden_size, dtype=torch.bfloat16,
                            device="cuda", generator=gen)
            paths = paths_for(T, MoEMLP.MX4A4_MFMA_TOKENS,
                              MoEMLP.DENSE_TOKENS, args.grid_orders)
            # the routed kernels read at most the T*k selected experts
            touched = {p: min(E, T * k) * expert_bytes(cfg, p != "bf16")
                       for p in paths}
            ncopy = {p: min(args.max_copies,
                            max(1, -(-2 * LLC_BYTES // touched[p])))
                     for p in paths}
            blocks = {"bf16": [make_block(cfg, False, gen)
                               for _ in range(ncopy["bf16"])]}
            blocks["mx4"] = [make_block(cfg, True, gen)
                             for _ in range(ncopy["mx4"])]
            for p in paths[2:]:
                blocks[p] = blocks["mx4"]
            graphs = {}
            if T <= MoEMLP.DENSE_TOKENS:
                for p in paths:
                    with torch.no_grad():
                        for b in blocks[p]:
                            run(b, x, p)
                        torch.cuda.synchronize()
                        g = torch.cuda.CUDAGraph()
                        with torch.cuda.graph(g):
                            for b in blocks[p]:
                                run(b, x, p)
                    graphs[p] = g
            res = {p: [] for p in paths}
            for _ in range(args.rounds):  # alternate the paths every round
                for p in paths:
                    if p in graphs:
                        t = time_graph(graphs[p], ncopy[p],
                                       max(3, 40 // ncopy[p]))
                    else:
                        with torch.no_grad():
                            t = time_eager(lambda b: run(b, x, p), blocks[p],
                                           max(3 * ncopy[p], 20))
                    res[p].append(t)
            for p, ts in res.items():
                med = statistics.median(ts)
                mode = "graph" if p in graphs else "eager"
                print(f"{name:14} {T:4d} {p:8} {mode:5} {ncopy[p]:6d} "
                      f"{med:9.1f} {min(ts):10.1f}..{max(ts):<10.1f}"
                      f"{touched[p] / 1e6:10.1f}", flush=True)
                rows.append({"block": name, "T": T, "path": p, "mode": mode,
                             "copies": ncopy[p], "us_median": med,
                             "us_min": min(ts), "us_max": max(ts),
                             "touched_bytes": touched[p], "rounds": len(ts)})
            del graphs, blocks
            torch.cuda.empty_cache()
    ops._MX4A4_TILE128_MIN_WGS = rule
    ops._WQA16_MOE_TILE128_MIN_WGS, ops._WQA16_MOE_SLAB_MAJOR = rules
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--blocks", default=",".join(BLOCKS))
    ap.add_argument("--ts", default=",".join(map(str, TS)))
    ap.add_argument("--max-copies", type=int, default=32)
    ap.add_argument("--grid-orders", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available() or not ops.native_available():
        sys.exit("bench_mx4_moe needs a GPU and the built extension")
    rows = bench(args)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
