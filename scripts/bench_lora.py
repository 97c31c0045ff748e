#!/usr/bin/env python3
"""Multi-LoRA serving cost: decode ms/step and TTFT with LoRA off and on.

Qwen2.5-7B random-init, batch 64 x input 1024, rank-16 random adapters
(save_random_adapter). Four configurations, alternated within one
invocation so drift hits all of them alike; (a) is repeated every round, its
spread is the run-to-run noise the others are read against:

  a  LoRA disabled
  b  LoRA enabled, every request on the base model (replays the same graphs)
  c  every request on one adapter
  d  four adapters round-robin

Each measurement: fresh requests, all prefills (TTFT p50), warm-up decode
steps (graph capture included), then >= 200 timed decode steps.

    python scripts/bench_lora.py [--rounds 3] [--steps 200] [--json out.json]
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from arks_amd.config import PRESET_CONFIGS, EngineConfig  # noqa: E402
from arks_amd.engine import LLMEngine, SamplingParams  # noqa: E402
from arks_amd.loader.lora_loader import save_random_adapter  # noqa: E402


def adapter_bytes_per_step(mc, rank: int, n_active: int) -> int:
    """Adapter weight bytes one decode step reads, from shapes: per layer
    A [S*R, K] + B [N, R] bf16 of qkv, o, gate_up and down, once per
    distinct active adapter (the tiles of one slot hit the same lines in L2)."""
    H, I, hd = mc.hidden_size, mc.intermediate_size, mc.head_dim
    nq, nkv = mc.num_attention_heads, mc.num_key_value_heads
    layers = [  # (S, K, N)
        (3, H, (nq + 2 * nkv) * hd), (1, nq * hd, H), (2, H, 2 * I), (1, I, H),
    ]
    per_layer = sum(S * rank * K + N * rank for S, K, N in layers) * 2
    return per_layer * mc.num_hidden_layers * n_active


def measure(engine: LLMEngine, prompts, loras, steps: int, warmup: int):
    sp = SamplingParams(max_tokens=warmup + steps + 64, ignore_eos=True)
    seqs = [engine.add_request(p, sp, lora=l) for p, l in zip(prompts, loras)]
    while engine.scheduler.num_waiting > 0:
        engine.step()
    torch.cuda.synchronize()
    ttfts = sorted((s.first_token_time - s.arrival_time) * 1e3 for s in seqs)
    for _ in range(warmup):
        engine.step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 0
    for _ in range(steps):
        n += len(engine.step())
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    assert n == steps * len(seqs), "a sequence left the batch while timed"
    for s in seqs:
        engine.abort_request(s.request_id)
    return ms, ttfts[len(ttfts) // 2]


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--model", default="qwen2.5-7b")
    p.add_argument("--batch", type=int, default=64)
    p.add_argument("--input-len", type=int, default=1024)
    p.add_argument("--rank", type=int, default=16)
    p.add_argument("--steps", type=int, default=200)
    p.add_argument("--warmup", type=int, default=16)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--json", default=None)
    args = p.parse_args()
    assert torch.cuda.is_available(), "bench_lora.py needs a GPU"

    mc = PRESET_CONFIGS[args.model]
    tmp = tempfile.mkdtemp(prefix="arks_lora_")
    mods = {}
    for i in range(4):
        mods[f"ad{i}"] = os.path.join(tmp, f"ad{i}")
        save_random_adapter(mc, mods[f"ad{i}"], rank=args.rank,
                            alpha=2 * args.rank, seed=i + 1, std=0.02)

    horizon = args.input_len + args.warmup + args.steps + 128
    common = dict(
        preset=args.model, device="cuda", max_num_seqs=max(args.batch, 256),
        max_num_batched_tokens=max(8192, args.input_len * 2),
        max_model_len=horizon,
        kv_cache_blocks=(args.batch * horizon + 15) // 16 + 64,
        # every round re-sends the same prompts: TTFT must not be a cache hit
        enable_prefix_caching=False,
    )
    off = LLMEngine(EngineConfig(**common))
    on = LLMEngine(EngineConfig(**common, enable_lora=True, max_loras=4,
                                max_lora_rank=args.rank, lora_modules=mods))

    g = torch.Generator().manual_seed(0)
    prompts = [torch.randint(0, mc.vocab_size - 1, (args.input_len,),
                             generator=g).tolist() for _ in range(args.batch)]
    B = args.batch
    configs = {
        "a": (off, [None] * B, 0),
        "b": (on, [None] * B, 0),
        "c": (on, ["ad0"] * B, 1),
        "d": (on, [f"ad{i % 4}" for i in range(B)], 4),
    }
    # warm up every shape (kernels, workspaces, both graph sets) untimed
    for eng, loras, _ in configs.values():
        measure(eng, prompts, loras, steps=4, warmup=4)

    res = {k: {"ms": [], "ttft": []} for k in configs}
    for _ in range(args.rounds):
        for k, (eng, loras, _) in configs.items():
            ms, ttft = measure(eng, prompts, loras, args.steps, args.warmup)
            res[k]["ms"].append(ms)
            res[k]["ttft"].append(ttft)

    out = {"model": args.model, "batch": B, "input_len": args.input_len,
           "rank": args.rank, "steps": args.steps, "rounds": args.rounds,
           "configs": {}}
    print("| config | decode ms/step (median, min-max) | TTFT p50 ms "
          "(median, min-max) | adapter MB read/step |")
    print("|---|---|---|---|")
    for k, (_, _, n_active) in configs.items():
        ms, tt = res[k]["ms"], res[k]["ttft"]
        mb = adapter_bytes_per_step(mc, args.rank, n_active) / 1e6
        out["configs"][k] = {"decode_ms": ms, "ttft_ms": tt,
                             "adapter_mb_per_step": mb}
        print(f"| {k} | {statistics.median(ms):.3f} "
              f"({min(ms):.3f}-{max(ms):.3f}) | {statistics.median(tt):.1f} "
              f"({min(tt):.1f}-{max(tt):.1f}) | {mb:.1f} |")
    print(json.dumps(out))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
