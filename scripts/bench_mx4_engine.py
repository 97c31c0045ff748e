"""Engine-level MXFP4 measurement: decode ms/step, weight bytes and KV blocks
against bf16.

Builds the random-init preset once per mode (bf16, and quantization="mxfp4",
which converts the dense projections by the OCP rule right after the weights
exist, i.e. before the KV pool is sized and the decode graphs are captured),
and for each of `--batches` runs that many requests of `--input-len` tokens
through prefill, then times `--steps` decode steps over the full batch after
`--warmup` untimed ones (host clock around a device synchronise, as bench.py
does). hipGraph decode. Random weights through the quantizer: this measures
speed and memory only.

kv_blocks_at_0.90 is the pool the engine would size by itself at the default
gpu_memory_utilization: the run's own (small, fixed) pool is added back to
the free memory that profile_num_blocks sees.

    python scripts/bench_mx4_engine.py [--model qwen2.5-7b] [--out r.json]
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from arks_amd.config import EngineConfig  # noqa: E402
from arks_amd.engine import LLMEngine, SamplingParams  # noqa: E402
from arks_amd.engine.kv_cache import kv_cache_block_bytes  # noqa: E402


def weight_bytes(mc, mx4: bool) -> int:
    """Bytes of weights one decode step streams (dense layers + lm_head)."""
    H, I = mc.hidden_size, mc.intermediate_size
    qkv = (mc.num_attention_heads + 2 * mc.num_key_value_heads) * mc.head_dim
    shapes = [(qkv, H), (H, mc.num_attention_heads * mc.head_dim),
              (2 * I, H), (H, I)]
    if mx4:
        per_layer = sum(n * k // 2 + n * (k // 32) for n, k in shapes)
    else:
        per_layer = sum(n * k * 2 for n, k in shapes)
    return mc.num_hidden_layers * per_layer + mc.vocab_size * H * 2


def build(args, mx4: bool):
    horizon = args.input_len + args.warmup + args.steps + 128
    top = max(args.batches)
    return LLMEngine(EngineConfig(
        preset=args.model, device=args.device, max_num_seqs=max(top, 256),
        max_num_batched_tokens=max(8192, args.input_len * 2),
        max_model_len=horizon,
        kv_cache_blocks=(top * horizon + 15) // 16 + 64, seed=args.seed,
        quantization="mxfp4" if mx4 else None,
    ))


def kv_blocks_at_default(engine) -> int | None:
    r = engine.runner
    if r.device.type != "cuda":
        return None
    mc = r.model_cfg
    block_bytes = kv_cache_block_bytes(
        mc.num_hidden_layers, mc.num_key_value_heads, mc.head_dim,
        r.cfg.block_size, dtype_bytes=2)
    free, total = torch.cuda.mem_get_info(r.device)
    used = (total - free) - r.num_blocks * block_bytes
    return int(total * 0.90 - used) // block_bytes


def decode_ms(engine, args, batch: int) -> float:
    g = torch.Generator().manual_seed(args.seed)
    prompts = [torch.randint(0, engine.model_cfg.vocab_size - 1,
                             (args.input_len,), generator=g).tolist()
               for _ in range(batch)]
    sp = SamplingParams(max_tokens=args.warmup + args.steps, ignore_eos=True)
    for i, pr in enumerate(prompts):
        engine.add_request(pr, sp, request_id=f"b{batch}-{i}")
    while engine.scheduler.num_waiting > 0:
        engine.step()
    for _ in range(args.warmup):
        engine.step()
    sync = torch.cuda.synchronize if args.device == "cuda" else (lambda: None)
    sync()
    t0 = time.time()
    tokens = 0
    for _ in range(args.steps - 1):
        tokens += len(engine.step())
    sync()
    ms = (time.time() - t0) * 1e3 / (args.steps - 1)
    assert tokens == batch * (args.steps - 1), tokens
    while engine.has_work():  # drain the last token of every request
        engine.step()
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="qwen2.5-7b")
    ap.add_argument("--batches", default="1,8,64")
    ap.add_argument("--input-len", type=int, default=128)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--device", default="cuda",
                    help="cpu only rehearses the script; its times mean nothing")
    args = ap.parse_args()
    args.batches = [int(b) for b in args.batches.split(",")]
    if args.device == "cuda" and not torch.cuda.is_available():
        sys.exit("bench_mx4_engine needs a GPU")
    result = {"model": args.model, "input_len": args.input_len,
              "steps": args.steps, "runs": []}
    for mx4 in (False, True):
        engine = build(args, mx4)
        mod = engine.runner.model.layers[0].mlp.down_proj
        assert bool(getattr(mod, "mx4", False)) == mx4
        engine.generate([[1, 2, 3] * 16, [4, 5] * 8],
                        SamplingParams(max_tokens=4, ignore_eos=True))
        blocks = kv_blocks_at_default(engine)
        for batch in args.batches:
            ms = decode_ms(engine, args, batch)
            wb = weight_bytes(engine.model_cfg, mx4)
            row = {"weights": "mxfp4" if mx4 else "bf16", "batch": batch,
                   "decode_ms_per_step": round(ms, 3),
                   "weight_gb_per_step": round(wb / 1e9, 3),
                   "whole_step_weight_gbs": round(wb / ms / 1e6, 1),
                   "kv_blocks_at_0.90": blocks}
            print(json.dumps(row), flush=True)
            result["runs"].append(row)
        del engine
        if args.device == "cuda":
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
