"""Engine-level int4 measurement: decode ms/step and logit drift against bf16.

Builds the random-init preset twice per mode (quantization None and "int4";
hipGraph decode and eager), runs `--batch` requests of `--input-len` tokens
through prefill, then times `--steps` decode steps over the full batch after
`--warmup` untimed ones (host clock around a device synchronise, as bench.py
does). Both configurations run in this one process, alternating.

It also reports the mean and max absolute difference of the last-position
prefill logits, int4 against bf16, on the same random weights and prompts.
That is round-to-nearest on RANDOM weights, not an AWQ-calibrated model: it
bounds nothing about a real checkpoint's quality.

    python scripts/bench_w4_engine.py [--model qwen2.5-7b] [--out r.json]
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


def weight_bytes(mc, int4: bool) -> int:
    """Bytes of weights one decode step streams (dense layers + lm_head)."""
    H, I = mc.hidden_size, mc.intermediate_size
    qkv = (mc.num_attention_heads + 2 * mc.num_key_value_heads) * mc.head_dim
    shapes = [(qkv, H), (H, mc.num_attention_heads * mc.head_dim),
              (2 * I, H), (H, I)]
    if int4:
        per_layer = sum(n * k // 2 + (k // 128) * n * 3 for n, k in shapes)
    else:
        per_layer = sum(n * k * 2 for n, k in shapes)
    return mc.num_hidden_layers * per_layer + mc.vocab_size * H * 2


def run(args, quantization, eager):
    horizon = args.input_len + args.warmup + args.steps + 128
    engine = LLMEngine(EngineConfig(
        preset=args.model, device=args.device, max_num_seqs=max(args.batch, 256),
        max_num_batched_tokens=max(8192, args.input_len * 2),
        max_model_len=horizon,
        kv_cache_blocks=(args.batch * horizon + 15) // 16 + 64,
        seed=args.seed, quantization=quantization, enforce_eager=eager,
    ))
    engine.generate([[1, 2, 3] * 16, [4, 5] * 8],
                    SamplingParams(max_tokens=4, ignore_eos=True))
    g = torch.Generator().manual_seed(args.seed)
    prompts = [torch.randint(0, engine.model_cfg.vocab_size - 1,
                             (args.input_len,), generator=g).tolist()
               for _ in range(args.batch)]
    sp = SamplingParams(max_tokens=args.warmup + args.steps + 64,
                        ignore_eos=True)

    # accuracy probe: one prefill step of 8 x 256 tokens, its logits kept
    logits = []
    real = engine.runner.model.forward

    def spy(batch, kv):
        out = real(batch, kv)
        logits.append(out.detach().float().cpu())
        return out

    engine.runner.model.forward = spy
    engine.generate([p[:256] for p in prompts[:8]],
                    SamplingParams(max_tokens=1, ignore_eos=True))
    engine.runner.model.forward = real
    logits = logits[:1]

    for i, pr in enumerate(prompts):
        engine.add_request(pr, sp, request_id=f"b-{i}")
    while engine.scheduler.num_waiting > 0:
        engine.step()
    for _ in range(args.warmup):
        engine.step()
    sync = torch.cuda.synchronize if args.device == "cuda" else (lambda: None)
    sync()
    t0 = time.time()
    tokens = 0
    for _ in range(args.steps):
        tokens += len(engine.step())
    sync()
    ms = (time.time() - t0) * 1e3 / args.steps
    assert tokens == args.batch * args.steps, tokens
    mc = engine.model_cfg
    del engine
    if args.device == "cuda":
        torch.cuda.empty_cache()
    return ms, torch.cat(logits), mc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="qwen2.5-7b")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--input-len", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--modes", default="graph,eager")
    ap.add_argument("--out", default=None)
    ap.add_argument("--device", default="cuda",
                    help="cpu only rehearses the script; its times mean nothing")
    args = ap.parse_args()
    if args.device == "cuda" and not torch.cuda.is_available():
        sys.exit("bench_w4_engine needs a GPU")
    result = {"model": args.model, "batch": args.batch,
              "input_len": args.input_len, "steps": args.steps, "runs": []}
    ref_logits = {}
    for mode in args.modes.split(","):
        for quant in (None, "int4"):
            ms, logits, mc = run(args, quant, eager=(mode == "eager"))
            wb = weight_bytes(mc, quant == "int4")
            row = {"mode": mode, "quantization": quant,
                   "decode_ms_per_step": round(ms, 3),
                   "weight_gb_per_step": round(wb / 1e9, 3),
                   "whole_step_weight_gbs": round(wb / ms / 1e6, 1)}
            if quant is None:
                ref_logits[mode] = logits
            else:
                d = (logits - ref_logits[mode]).abs()
                row["logit_absdiff_mean"] = float(d.mean())
                row["logit_absdiff_max"] = float(d.max())
                row["logit_abs_mean_bf16"] = float(
                    ref_logits[mode].abs().mean())
            print(json.dumps(row), flush=True)
            result["runs"].append(row)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
