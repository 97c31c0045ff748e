#!/usr/bin/env python
"""ops.attention_mla_paged (attn_mla.hip) against ops.ref's torch
implementation run on the GPU: the parent of this kernel has no MLA path, so
the torch reference is the baseline.

Decode at batch 1 / 8 / 64 over contexts 1k / 4k / 16k with H = 16 and 128,
prefill of 512 / 2048 new tokens with H = 16. Times are device events around
ITERS back-to-back calls (after a warm-up of every shape), median of ROUNDS
rounds with the kernel and the reference alternating; min..max are printed.
"latent GB/s" is the bytes the algorithm needs, every live cache row once per
sequence (decode) or once per query token's head tile (what this kernel
streams in prefill), over the kernel's time: a whole-call rate, not a share
of peak. One JSON line per case.

  python scripts/bench_mla.py [--quick] [--parts N]
"""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import arks_amd.ops as ops  # noqa: E402
from arks_amd.ops import ref  # noqa: E402

ROW_BYTES = 576 * 2


def make_case(S, ctx, q_len, H, dev):
    nb = -(-ctx // 16)
    cache = torch.randn(S * nb + 1, 16, 576, dtype=torch.bfloat16, device=dev)
    bt = torch.randperm(S * nb, device=dev).to(torch.int32).view(S, nb)
    sl = torch.full((S,), ctx, dtype=torch.int32, device=dev)
    T = S * q_len
    q_lat = torch.randn(T, H, 512, dtype=torch.bfloat16, device=dev)
    q_pe = torch.randn(T, H, 64, dtype=torch.bfloat16, device=dev)
    cu = None
    if q_len > 1:
        cu = torch.arange(0, T + 1, q_len, dtype=torch.int32, device=dev)
    return q_lat, q_pe, cache, bt, sl, cu


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters  # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true",
                    help="fewer rounds and iterations")
    ap.add_argument("--parts", type=int, default=None,
                    help="num_partitions (default: the heuristic)")
    args = ap.parse_args()
    assert torch.cuda.is_available() and ops.native_available(), \
        "needs the GPU and the built extension"
    dev = torch.device("cuda")
    rounds, iters = (3, 5) if args.quick else (5, 20)
    scale = 192 ** -0.5
    cases = [("decode", S, ctx, 1, H) for H in (16, 128)
             for S in (1, 8, 64) for ctx in (1024, 4096, 16384)]
    cases += [("prefill", 1, n, n, 16) for n in (512, 2048)]
    for kind, S, ctx, q_len, H in cases:
        q_lat, q_pe, cache, bt, sl, cu = make_case(S, ctx, q_len, H, dev)
        T = S * q_len
        parts = args.parts or ops.mla_num_partitions(T, H, bt.shape[1])

        def kernel():
            return ops.attention_mla_paged(q_lat, q_pe, cache, bt, sl, scale,
                                           cu_seqlens=cu, num_partitions=parts)

        def baseline():
            return ref.attention_mla_paged(q_lat, q_pe, cache, bt, sl, scale, cu)

        got, want = kernel(), baseline()  # warm-up of both, and a check
        err = (got.float() - want.float()).abs().max().item()
        ref_iters = max(1, iters // 5)
        k_us, r_us = [], []
        for _ in range(rounds):
            k_us.append(timed(kernel, iters))
            r_us.append(timed(baseline, ref_iters))
        if q_len == 1:
            stream = S * ctx * ROW_BYTES
        else:  # every query token's head tile streams its causal prefix
            stream = S * -(-H // 16) * ROW_BYTES * sum(
                ctx - q_len + i + 1 for i in range(q_len))
        k_med = statistics.median(k_us)
        print(json.dumps({
            "case": kind, "batch": S, "context": ctx, "q_len": q_len,
            "heads": H, "partitions": parts,
            "kernel_us": round(k_med, 1),
            "kernel_us_min_max": [round(min(k_us), 1), round(max(k_us), 1)],
            "torch_ref_us": round(statistics.median(r_us), 1),
            "torch_ref_us_min_max": [round(min(r_us), 1), round(max(r_us), 1)],
            "latent_GBps": round(stream / k_med / 1e3, 1),
            "max_abs_diff_vs_ref": round(err, 4),
        }), flush=True)


if __name__ == "__main__":
    main()
