#!/usr/bin/env python
"""Measurements of the structured-output path (docs/kernels.md, "Masked
sampling"). Three independent parts, each prints one JSON line:

  --kernels   masked vs unmasked sampling kernels at (64, V) and (256, V),
              V = 151936, every row constrained; device events, the two
              variants alternated inside one process
  --step      decode ms/step at batch 64 on a preset with random weights,
              all rows under one JSON-schema grammar against none; the
              host share (mask lookup + upload) and the sampling-kernel
              share are timed inside the same steps
  --compile   grammar compile time and DFA state counts (CPU only)

The GPU parts fail without a GPU; they never fall back.
"""

from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402

TEST_SCHEMA = {
    "type": "object",
    "properties": {
        "ok": {"type": "boolean"},
        "color": {"enum": ["red", "green", "blue"]},
        "code": {"type": "string", "pattern": "[A-Z]{3}"},
        "tags": {"type": "array", "items": {"enum": ["a", "b", "c"]},
                 "maxItems": 3},
    },
    "required": ["ok", "code"],
}


def need_gpu():
    if not torch.cuda.is_available():
        sys.exit("this measurement needs a GPU")


def _events(fn, iters):
    start = [torch.cuda.Event(enable_timing=True) for _ in range(iters)]
    stop = [torch.cuda.Event(enable_timing=True) for _ in range(iters)]
    for i in range(iters):
        start[i].record()
        fn()
        stop[i].record()
    torch.cuda.synchronize()
    return [s.elapsed_time(e) * 1000.0 for s, e in zip(start, stop)]  # us


def bench_kernels(args):
    need_gpu()
    import arks_amd.ops as ops

    V = args.vocab
    W = (V + 31) // 32
    res = {"part": "kernels", "vocab": V, "iters": args.iters, "shapes": {}}
    for rows in (64, 256):
        g = torch.Generator(device="cuda").manual_seed(rows)
        logits = torch.randn(rows, V, device="cuda", generator=g).bfloat16()
        u = torch.rand(rows, V, device="cuda", generator=g)
        temps = torch.full((rows,), 0.8, device="cuda")
        # 16 distinct half-dense masks shared by the rows, like a batch
        # spread over a few grammar states
        masks = torch.randint(-2 ** 31, 2 ** 31 - 1, (16, W), device="cuda",
                              generator=g, dtype=torch.int64).to(torch.int32)
        mr = (torch.arange(rows, device="cuda") % 16).to(torch.int32)
        fns = {
            "greedy": lambda: ops.greedy_sample(logits),
            "greedy_masked": lambda: ops.greedy_sample_masked(logits, masks, mr),
            "gumbel": lambda: ops.sample_tokens(logits, temps, u),
            "gumbel_masked": lambda: ops.sample_tokens_masked(logits, temps, u, masks, mr),
        }
        for fn in fns.values():  # warm every variant at this shape
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        runs = {k: [] for k in fns}
        for _ in range(args.repeats):  # alternate variants: shared machine
            for k, fn in fns.items():
                runs[k].append(statistics.median(_events(fn, args.iters)))
        shape = {k: {"median_us": round(statistics.median(v), 2),
                     "min_us": round(min(v), 2), "max_us": round(max(v), 2)}
                 for k, v in runs.items()}
        shape["ratio_greedy"] = round(
            shape["greedy_masked"]["median_us"] / shape["greedy"]["median_us"], 3)
        shape["ratio_gumbel"] = round(
            shape["gumbel_masked"]["median_us"] / shape["gumbel"]["median_us"], 3)
        # bytes the algorithm needs: 2V (+4V noise) per row, + V/8 mask
        shape["expected_ratio_greedy"] = round((2 * V + V / 8) / (2 * V), 3)
        shape["expected_ratio_gumbel"] = round((6 * V + V / 8) / (6 * V), 3)
        res["shapes"][f"{rows}x{V}"] = shape
    print(json.dumps(res))


def bench_step(args):
    need_gpu()
    from arks_amd.config import EngineConfig
    from arks_amd.engine import LLMEngine, SamplingParams
    from arks_amd.server.tokenizer import ByteTokenizer

    horizon = args.input_len + 2 * (args.warmup + args.steps) + 192
    cfg = EngineConfig(
        preset=args.model, device="cuda", max_num_seqs=max(args.batch, 256),
        max_num_batched_tokens=max(8192, args.input_len * 2),
        max_model_len=horizon,
        kv_cache_blocks=(args.batch * horizon + 15) // 16 + 64, seed=args.seed,
    )
    engine = LLMEngine(cfg)
    mc = engine.model_cfg
    engine.set_tokenizer(ByteTokenizer(mc.vocab_size, mc.eos_token_id))
    engine.generate([[1, 2, 3] * 16, [4, 5] * 8],
                    SamplingParams(max_tokens=4, ignore_eos=True))
    n = args.warmup + args.steps + 16
    # a schema whose shortest document outlasts the timed window, so every
    # row stays constrained and in decode throughout
    schema = {"type": "array", "items": {"enum": ["alpha", "beta"]}, "minItems": n}
    runner = engine.runner
    host_s = [0.0]
    samp_us: list = []
    inner_masks, inner_sample = runner._structured_masks, runner.sample

    def timed_masks(logits, seqs):
        t0 = time.perf_counter()
        out = inner_masks(logits, seqs)
        host_s[0] += time.perf_counter() - t0
        return out

    def timed_sample(logits, seqs):
        a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
        a.record()
        out = inner_sample(logits, seqs)
        b.record()
        samp_us.append((a, b))
        return out

    runner._structured_masks, runner.sample = timed_masks, timed_sample
    g = torch.Generator().manual_seed(args.seed)
    res = {"part": "step", "model": args.model, "batch": args.batch,
           "steps": args.steps, "input_len": args.input_len}
    for name, structured in (("plain", None), ("structured", {"kind": "json_schema", "value": schema}),
                             ("plain_again", None)):
        prompts = [torch.randint(4, 260, (args.input_len,), generator=g).tolist()
                   for _ in range(args.batch)]
        sp = SamplingParams(max_tokens=n + 48, structured=structured,
                            ignore_eos=structured is None, temperature=args.temperature)
        seqs = [engine.add_request(p, sp) for p in prompts]
        while engine.scheduler.num_waiting > 0:
            engine.step()
        for _ in range(args.warmup):
            engine.step()
        torch.cuda.synchronize()
        host_s[0] = 0.0
        samp_us.clear()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            out = engine.step()
            assert len(out) == args.batch
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        res[name] = {
            "ms_per_step": round(dt / args.steps * 1000, 3),
            "host_mask_ms_per_step": round(host_s[0] / args.steps * 1000, 3),
            # device time from entering sample() to its last kernel
            "sample_device_ms_per_step": round(
                sum(a.elapsed_time(b) for a, b in samp_us) / args.steps, 3),
        }
        for s in seqs:
            engine.abort_request(s.request_id)
        while engine.has_work():
            engine.step()
    pool = runner._mask_pool
    res["pool_states"] = len(pool["lru"]) if pool else 0
    print(json.dumps(res))


def bench_compile(args):
    from arks_amd.server.tokenizer import ByteTokenizer
    from arks_amd.structured import (CompiledGrammar, TokenTable, any_object,
                                     compile_regex, schema_to_regex)

    V = args.vocab
    t0 = time.perf_counter()
    table = TokenTable.from_tokenizer(ByteTokenizer(V, V - 1), V, V - 1)
    res = {"part": "compile", "vocab": V,
           "token_table_s": round(time.perf_counter() - t0, 4)}
    for name, rx in (("test_schema", schema_to_regex(TEST_SCHEMA)),
                     ("json_object_depth5", any_object())):
        t0 = time.perf_counter()
        dfa = compile_regex(rx)
        t1 = time.perf_counter()
        g = CompiledGrammar(dfa, table)
        for s in range(dfa.num_states):
            g.state(s)
        t2 = time.perf_counter()
        res[name] = {"regex_chars": len(rx), "dfa_states": dfa.num_states,
                     "compile_s": round(t1 - t0, 4),
                     "all_state_masks_s": round(t2 - t1, 4)}
    print(json.dumps(res))


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--kernels", action="store_true")
    p.add_argument("--step", action="store_true")
    p.add_argument("--compile", action="store_true")
    p.add_argument("--vocab", type=int, default=151936)
    p.add_argument("--iters", type=int, default=200)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--model", default="qwen2.5-7b")
    p.add_argument("--batch", type=int, default=64)
    p.add_argument("--input-len", type=int, default=128)
    p.add_argument("--steps", type=int, default=64)
    p.add_argument("--warmup", type=int, default=8)
    p.add_argument("--temperature", type=float, default=0.0)
    p.add_argument("--seed", type=int, default=0)
    args = p.parse_args()
    if not (args.kernels or args.step or args.compile):
        p.error("pick at least one of --kernels, --step, --compile")
    if args.compile:
        bench_compile(args)
    if args.kernels:
        bench_kernels(args)
    if args.step:
        bench_step(args)


if __name__ == "__main__":
    main()
