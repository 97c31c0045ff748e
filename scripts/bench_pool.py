#!/usr/bin/env python3
"""Embedding pooling: ops.pool_embed against the composition it replaces.

T = 16384 packed rows of H = 4096 (bf16), cut into 16 and into 256 equal
segments. Per shape and per mode (last, mean), alternated within one
invocation so drift hits both alike:

  pool   ops.pool_embed: add + final norm + pooling + L2 normalisation
  comp   ops.fused_add_rmsnorm over all T rows, then torch pooling (the last
         row of each segment / the per-segment mean in fp32) and F.normalize

The composition gets its best case: equal-length segments, so its mean is one
reshaped reduction with no gather. Both read two alternating (x, residual)
sets (2 x 256 MiB) so neither is served from the 256 MiB last-level cache.
x flips sign between the composition's calls, which add it into residual in
place, so the data stays in range however long the run.

Times are device-event times over --iters back-to-back calls. Bytes are what
each algorithm must move, from shapes: pool/mean reads x and residual once,
pool/last reads one row pair per segment; the composition reads x and
residual, writes residual and the normed rows, and reads the latter again.

    python scripts/bench_pool.py [--rounds 5] [--iters 300] [--json out.json]
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import arks_amd.ops as ops  # noqa: E402

EPS = 1e-6
HBM_TBPS = 6.3  # streaming ceiling (docs/kernels.md)


def timed(fn, iters: int) -> float:
    """Mean microseconds per call over `iters` calls, by device events."""
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    for i in range(iters):
        fn(i)
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / iters


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=16384)
    p.add_argument("--hidden", type=int, default=4096)
    p.add_argument("--segments", type=int, nargs="+", default=[16, 256])
    p.add_argument("--iters", type=int, default=300)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--json", default=None)
    args = p.parse_args()
    assert torch.cuda.is_available(), "bench_pool.py needs a GPU"
    assert ops.native_available(), "build the extension first"
    T, H = args.rows, args.hidden
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)

    def rows():
        base = torch.randn(1, H, device=dev, generator=g)
        return (base + 0.5 * torch.randn(T, H, device=dev, generator=g)
                ).to(torch.bfloat16)

    sets = [(rows(), rows()) for _ in range(2)]
    negs = [-x for x, _ in sets]
    weight = (1 + 0.1 * torch.randn(H, device=dev, generator=g)
              ).to(torch.bfloat16)

    out = {"rows": T, "hidden": H, "iters": args.iters, "rounds": args.rounds,
           "shapes": {}}
    rowpair = 2 * H * 2  # one row of x and of residual, bf16
    for S in args.segments:
        assert T % S == 0
        L = T // S
        tables = {
            m: ops.build_pool_table(
                [(i * L, L, m, -1, 0, 1) for i in range(S)], dev)
            for m in ("last", "mean")}
        last_idx = torch.arange(S, device=dev) * L + (L - 1)

        def pool(mode):
            def fn(i):
                x, r = sets[i & 1]
                return ops.pool_embed(x, r, weight, EPS, tables[mode], None)
            return fn

        def comp(mode):
            def fn(i):
                x, r = sets[i & 1]
                # +x, -x, +x ... into each residual: it stays bounded
                xi = x if (i >> 1) & 1 == 0 else negs[i & 1]
                y, _ = ops.fused_add_rmsnorm(xi, r, weight, EPS)
                if mode == "last":
                    v = y[last_idx].float()
                else:
                    v = y.view(S, L, H).mean(1, dtype=torch.float32)
                return F.normalize(v, dim=-1)
            return fn

        # the two must agree before either is timed (same inputs, residual
        # untouched by pool and restored for the check)
        for mode in ("last", "mean"):
            x, r = sets[0]
            a = pool(mode)(0)
            b = comp(mode)(0)
            r.copy_((r.float() - x.float()).to(torch.bfloat16))
            diff = (a - b).abs().max().item()
            # comp rounds the normed rows to bf16 first: half an ulp, up to
            # 2^-8 of a component, and components stay below 0.25 here
            assert diff < 1e-3, (S, mode, diff)

        variants = {"pool/last": pool("last"), "comp/last": comp("last"),
                    "pool/mean": pool("mean"), "comp/mean": comp("mean")}
        bytes_ = {
            "pool/last": S * rowpair,
            "pool/mean": T * rowpair,
            "comp/last": T * rowpair + 2 * T * H * 2 + S * H * 2,
            "comp/mean": T * rowpair + 2 * T * H * 2 + T * H * 2,
        }
        for fn in variants.values():  # warm every shape, untimed
            timed(fn, 8)
        us = {k: [] for k in variants}
        for _ in range(args.rounds):
            for k, fn in variants.items():
                us[k].append(timed(fn, args.iters))
        shape = out["shapes"][str(S)] = {}
        print(f"\nT={T} H={H} segments={S} (x {L} rows)")
        print("| variant | us/call (median, min-max) | bytes moved | TB/s | "
              "of 6.3 TB/s |")
        print("|---|---|---|---|---|")
        for k in variants:
            med = statistics.median(us[k])
            tbps = bytes_[k] / (med * 1e-6) / 1e12
            shape[k] = {"us": us[k], "bytes": bytes_[k], "tbps": tbps}
            print(f"| {k} | {med:.1f} ({min(us[k]):.1f}-{max(us[k]):.1f}) | "
                  f"{bytes_[k] / 1e6:.1f} MB | {tbps:.2f} | "
                  f"{100 * tbps / HBM_TBPS:.0f}% |")
    print(json.dumps(out))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
