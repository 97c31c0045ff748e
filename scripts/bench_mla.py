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

--prefill-layer times the whole attention-side work of a layer for a prefill
chunk on both paths instead: non-absorbed (gather + up-projection GEMMs +
attn_mla_prefill.hip, 128- and 256-row tiles) against absorbed (two bmms +
attn_mla.hip), fresh and over 4k / 32k prefixes, H = 16 and 128.

  python scripts/bench_mla.py [--quick] [--parts N] [--prefill-layer]
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


def prefill_layer_case(new, prefix, H, dev, rounds):
    """The attention-side work of one layer for a chunk of `new` tokens over
    a `prefix`, on both paths: non-absorbed (gather + the two up-projection
    GEMMs + attn_mla_prefill.hip, with 128- and 256-row tiles) and absorbed
    (the two bmms + attn_mla.hip, what every prefill ran before)."""
    ctx = prefix + new
    scale = 192 ** -0.5
    _, _, cache, bt, sl, _ = make_case(1, ctx, 1, 1, dev)
    q = torch.randn(new, H, 192, dtype=torch.bfloat16, device=dev)
    w_uk = torch.randn(H, 128, 512, dtype=torch.bfloat16, device=dev) * 0.05
    w_uv = torch.randn(H, 512, 128, dtype=torch.bfloat16, device=dev) * 0.05
    cu = torch.tensor([0, new], dtype=torch.int32, device=dev)
    plans = {t: ops.build_mla_prefill_plan([new], [ctx], H, dev, 1, 10**9, t)
             for t in (128, 256)}

    def non_absorbed(plan):
        c_kv, k_pe = ops.mla_gather_rows(cache, bt, plan.cu_seqlens_kv, ctx)
        k_nope = ops.linear_bf16(c_kv, w_uk.view(H * 128, 512))
        v = torch.matmul(c_kv, w_uv)
        return ops.attention_mla_prefill(q, k_nope.view(ctx, H, 128), k_pe,
                                         v.transpose(0, 1), cu, plan, scale)

    def absorbed():
        q_nope = q[..., :128].transpose(0, 1).contiguous()
        q_lat = torch.bmm(q_nope, w_uk).transpose(0, 1).contiguous()
        o_lat = ops.attention_mla_paged(q_lat, q[..., 128:], cache, bt, sl,
                                        scale, cu_seqlens=cu)
        return torch.bmm(o_lat.transpose(0, 1).contiguous(),
                         w_uv).transpose(0, 1)

    fns = {"tile128": lambda: non_absorbed(plans[128]),
           "tile256": lambda: non_absorbed(plans[256]), "absorbed": absorbed}
    outs = {k: f().float() for k, f in fns.items()}       # warm-up, check
    iters = {k: max(1, min(20, int(2e4 / max(timed(f, 1), 1.0))))
             for k, f in fns.items()}
    us = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():                          # alternating
            us[k].append(timed(f, iters[k]))
    med = {k: statistics.median(t) for k, t in us.items()}
    print(json.dumps({
        "case": "prefill_layer", "new_tokens": new, "prefix": prefix,
        "heads": H, "workspace_MiB": round(ctx * H * 512 / 2**20, 1),
        **{f"{k}_us": round(med[k], 1) for k in fns},
        **{f"{k}_us_min_max": [round(min(us[k]), 1), round(max(us[k]), 1)]
           for k in fns},
        "absorbed_over_tile128": round(med["absorbed"] / med["tile128"], 2),
        "absorbed_over_tile256": round(med["absorbed"] / med["tile256"], 2),
        "max_abs_diff_128_vs_absorbed": round(
            (outs["tile128"] - outs["absorbed"]).abs().max().item(), 4),
        "max_abs_diff_256_vs_128": round(
            (outs["tile256"] - outs["tile128"]).abs().max().item(), 4),
    }), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true",
                    help="fewer rounds and iterations")
    ap.add_argument("--prefill-layer", action="store_true",
                    help="only the prefill cases that time a layer's whole "
                         "attention-side work on both paths")
    ap.add_argument("--parts", type=int, default=None,
                    help="num_partitions (default: the heuristic)")
    args = ap.parse_args()
    assert torch.cuda.is_available() and ops.native_available(), \
        "needs the GPU and the built extension"
    dev = torch.device("cuda")
    rounds, iters = (3, 5) if args.quick else (5, 20)
    scale = 192 ** -0.5
    if args.prefill_layer:
        for H in (16, 128):
            for new in (128, 256, 512, 2048, 8192):
                prefill_layer_case(new, 0, H, dev, rounds)
            for prefix in (4096, 32768):
                for new in (256, 1024, 2048):
                    prefill_layer_case(new, prefix, H, dev, rounds)
        return
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
