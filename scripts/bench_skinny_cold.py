"""Per-shape time of the skinny GEMM with cold weights: the extension is
called at the decode plan's launch parameters while W rotates through
copies larger in total than the 256 MB last-level cache, as in a real decode
step, where 15 GB of other weights pass between two calls.

    PYTHONPATH=. python scripts/bench_skinny_cold.py [LABEL] [--config C]
        [--groups G[,G...]] [--shapes NAME[,NAME...]]
        [--down-config C[,C...]]

--config overrides the launch config of the split-K qkv/o shapes (0 = the
chunk-ring kernel, 3 = the A-resident kernel; default: what ops.skinny_gemm
routes to). --groups times config 3 once per value (workgroups per split,
0 = auto). --down-config times the down-proj shape once per value (1 =
128-row tiles, 4 = 112-row tiles; default: what ops.skinny_gemm routes to).

Companion of scripts/bench_membw_cold.hip (the raw-read floor of the same
pattern and grid); results in profiles/r05_skinny_stream.md and
profiles/r07_resident_a.md and profiles/r08_all_cus.md.
"""
import argparse

import torch

import arks_amd.ops as ops

ap = argparse.ArgumentParser()
ap.add_argument("label", nargs="?", default="build")
ap.add_argument("--config", type=int, default=None)
ap.add_argument("--groups", default="0")
ap.add_argument("--shapes", default=None)
ap.add_argument("--down-config", default=None)
args = ap.parse_args()
label = args.label
native = ops._native()
dev = "cuda"
torch.manual_seed(0)
# name, M, N, K
shapes = [("down", 64, 3584, 18944), ("down_nt", 64, 3584, 18944),
          ("qkv", 64, 4608, 3584), ("o", 64, 3584, 3584),
          ("qkv_m16", 16, 4608, 3584), ("o_m16", 16, 3584, 3584)]
if args.shapes:
    shapes = [s for s in shapes if s[0] in args.shapes.split(",")]
for name, M, N, K in shapes:
    config, nsplits, kps, mrows = ops._skinny_plan(M, N, K)
    config = ops._skinny_resident_config(config, M, nsplits, kps)
    config = ops._skinny_tallk7_config(config, N, nsplits, ops._cu_count(
        torch.device(dev, torch.cuda.current_device())))
    if name == "down_nt":
        config = 2
    elif args.config is not None and not name.startswith("down"):
        config = args.config
    wbytes = N * K * 2
    nbuf = max(2, -(-640 * 2**20 // wbytes))
    ws = [torch.randn(N, K, dtype=torch.bfloat16, device=dev) * 0.05 for _ in range(nbuf)]
    a = torch.randn(M, K, dtype=torch.bfloat16, device=dev) * 0.5
    part = torch.empty(nsplits * mrows * N, dtype=torch.float32, device=dev)
    configs = ([int(c) for c in args.down_config.split(",")]
               if name == "down" and args.down_config else [config])
    runs = [(c, g) for c in configs
            for g in ([int(g) for g in args.groups.split(",")]
                      if c == 3 else [0])]
    for config, groups in runs:
        def rot(n):
            for _ in range(n):
                for w in ws:
                    native.skinny_gemm_partials(part, a, w, kps, nsplits,
                                                config, groups)
        rot(2)
        torch.cuda.synchronize()
        res = []
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rot(3)
            e1.record()
            torch.cuda.synchronize()
            res.append(e0.elapsed_time(e1) * 1000 / (3 * nbuf))
        us = sorted(res)[1]
        print(f"{label:10s} {name:8s} cfg={config} g={groups} ns={nsplits} kps={kps} nbuf={nbuf} "
              f"{us:7.2f} us  {wbytes / us / 1e6:5.2f} TB/s   (runs {[round(r, 2) for r in res]})",
              flush=True)
    del ws
