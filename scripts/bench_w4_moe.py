"""Measure W4 MoE experts against the bf16 MoE block.

    python scripts/bench_w4_moe.py kernel [--rounds 5] [--out k.json]
    python scripts/bench_w4_moe.py engine [--model qwen3-30b-a3b] [--out e.json]
    python scripts/bench_w4_moe.py awq-load [--layers 2] [--out a.json]

kernel: one MoE block (MoEMLP.forward: router, experts, mix) of the
qwen3-30b-a3b and mixtral-8x7b shapes at T = 1, 8, 64, 256 tokens, the bf16
block as it stands against the W4 block, inside one captured graph (T above
MoEMLP.DENSE_TOKENS, e.g. --ts 2048, syncs with the host once per call on
both paths and is timed eagerly instead). Each path
cycles through enough copies of the block that the bytes a call touches
exceed the 256 MB LLC twice over, so every call streams its weights from HBM
as a decode step does; the two paths alternate within each round and the
table shows the median and min..max of the rounds (device-event times).

engine: decode ms/step of a random-init preset at batch 1, 8, 64, 256, bf16
against int4 + quantize_experts, one engine per configuration, with the
number of KV blocks each configuration gets from the memory left.

awq-load: writes an MoE AWQ checkpoint of the preset (optionally cut to
--layers layers, the full model takes the host a long time to quantize) with
save_awq_checkpoint and times the engine's load of it.
"""

from __future__ import annotations

import argparse
import dataclasses
import json
import os
import statistics
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import arks_amd.ops as ops  # noqa: E402
from arks_amd.config import PRESET_CONFIGS, EngineConfig  # noqa: E402
from bench_w4 import LLC_BYTES, time_eager, time_graph, w4_bytes  # noqa: E402

BLOCKS = ("qwen3-30b-a3b", "mixtral-8x7b")
TS = (1, 8, 64, 256)


def expert_bytes(cfg, w4: bool) -> int:
    """Stored bytes of ONE expert (w13 + w2)."""
    H = cfg.hidden_size
    I = cfg.moe_intermediate_size or cfg.intermediate_size
    if w4:
        return w4_bytes(2 * I, H) + w4_bytes(H, I)
    return 3 * I * H * 2


def make_block(cfg, w4: bool, gen):
    """A MoEMLP built on the GPU with random weights; the W4 one is filled
    straight in the storage format (no quantization pass)."""
    from arks_amd.models.llama_family import MoEMLP

    with torch.device("cuda"):
        blk = MoEMLP(cfg)
    blk.gate.data.normal_(0, 0.5, generator=gen)
    if blk.shared is not None:
        raise SystemExit("kernel bench covers blocks without a shared expert")
    if not w4:
        blk.w13.data.normal_(0, 0.05, generator=gen)
        blk.w2.data.normal_(0, 0.05, generator=gen)
        return blk
    blk.init_w4("bench")
    for which in ("w13", "w2"):
        qw, sc, zr = blk.w4_packed(which)
        qw.random_(-2**31, 2**31 - 1, generator=gen)
        sc.fill_(0.0077)
        zr.random_(0, 16, generator=gen)
    return blk


def bench_kernel(args):
    gen = torch.Generator(device="cuda").manual_seed(0)
    rows = []
    print(f"{'block':14} {'T':>4} {'path':5} {'copies':>6} {'us':>9} "
          f"{'min..max':>21} {'touched MB':>10}")
    for name in args.blocks.split(","):
        cfg = PRESET_CONFIGS[name]
        E, k = cfg.num_local_experts, cfg.num_experts_per_tok
        for T in map(int, args.ts.split(",")):
            x = torch.randn(T, cfg.hidden_size, dtype=torch.bfloat16,
                            device="cuda", generator=gen)
            # the bf16 decode path streams every expert; the routed W4 path
            # at most the T*k selected ones
            touched = {"bf16": E * expert_bytes(cfg, False),
                       "w4": min(E, T * k) * expert_bytes(cfg, True)}
            graphs, ncopy = {}, {}
            blocks = {}
            for path in ("bf16", "w4"):
                n = min(args.max_copies,
                        max(1, -(-2 * LLC_BYTES // touched[path])))
                blocks[path] = [make_block(cfg, path == "w4", gen)
                                for _ in range(n)]
                ncopy[path] = n
                if T > blocks[path][0].DENSE_TOKENS:
                    continue  # one host sync per call: timed eagerly
                with torch.no_grad():
                    for b in blocks[path]:
                        b(x)
                    torch.cuda.synchronize()
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g):
                        for b in blocks[path]:
                            b(x)
                graphs[path] = g
            res = {"bf16": [], "w4": []}
            for _ in range(args.rounds):  # alternate the paths every round
                for path in ("bf16", "w4"):
                    if path in graphs:
                        t = time_graph(graphs[path], ncopy[path],
                                       max(3, 40 // ncopy[path]))
                    else:
                        with torch.no_grad():
                            t = time_eager(lambda b: b(x), blocks[path],
                                           max(3 * ncopy[path], 20))
                    res[path].append(t)
            for path, ts in res.items():
                med = statistics.median(ts)
                print(f"{name:14} {T:4d} {path:5} {ncopy[path]:6d} {med:9.1f} "
                      f"{min(ts):10.1f}..{max(ts):<10.1f}"
                      f"{touched[path] / 1e6:10.1f}", flush=True)
                rows.append({"block": name, "T": T, "path": path,
                             "mode": "graph" if path in graphs else "eager",
                             "copies": ncopy[path], "us_median": med,
                             "us_min": min(ts), "us_max": max(ts),
                             "touched_bytes": touched[path],
                             "rounds": len(ts)})
            del graphs, blocks
            torch.cuda.empty_cache()
    return rows


def bench_engine(args):
    from arks_amd.engine import LLMEngine, SamplingParams

    rows = []
    batches = list(map(int, args.batches.split(",")))
    for quant in (None, "int4"):
        horizon = args.input_len + args.warmup + args.steps + 80
        t0 = time.time()
        engine = LLMEngine(EngineConfig(
            preset=args.model, device="cuda", max_num_seqs=max(batches),
            max_model_len=horizon, seed=args.seed, quantization=quant,
            quantize_experts=quant == "int4"))
        build_s = time.time() - t0
        g = torch.Generator().manual_seed(args.seed)
        for batch in batches:
            prompts = [torch.randint(0, engine.model_cfg.vocab_size - 1,
                                     (args.input_len,), generator=g).tolist()
                       for _ in range(batch)]
            # slack: with mixed batching the first sequences decode while
            # the last still prefill, and must not finish inside the window
            sp = SamplingParams(max_tokens=args.warmup + args.steps + 64,
                                ignore_eos=True)
            for i, pr in enumerate(prompts):
                engine.add_request(pr, sp, request_id=f"b{batch}-{i}")
            while engine.scheduler.num_waiting > 0:
                engine.step()
            for _ in range(args.warmup):
                engine.step()
            torch.cuda.synchronize()
            t0 = time.time()
            tokens = 0
            for _ in range(args.steps):
                tokens += len(engine.step())
            torch.cuda.synchronize()
            ms = (time.time() - t0) * 1e3 / args.steps
            assert tokens == batch * args.steps, tokens
            while engine.has_work():
                engine.step()
            row = {"model": args.model, "quantization": quant,
                   "quantize_experts": quant == "int4", "batch": batch,
                   "decode_ms_per_step": round(ms, 3),
                   "kv_blocks": engine.runner.num_blocks,
                   "engine_build_s": round(build_s, 1)}
            print(json.dumps(row), flush=True)
            rows.append(row)
        del engine
        torch.cuda.empty_cache()
    return rows


def bench_awq_load(args):
    from arks_amd.engine import LLMEngine
    from arks_amd.loader.safetensors_loader import save_awq_checkpoint

    cfg = PRESET_CONFIGS[args.model]
    if args.layers:
        cfg = dataclasses.replace(cfg, num_hidden_layers=args.layers)
    with tempfile.TemporaryDirectory(dir=args.tmp) as d:
        t0 = time.time()
        save_awq_checkpoint(cfg, d, seed=args.seed)
        write_s = time.time() - t0
        size = sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))
        t0 = time.time()
        engine = LLMEngine(EngineConfig(
            model_path=d, device="cuda", max_model_len=1024,
            kv_cache_blocks=256, enforce_eager=True))
        torch.cuda.synchronize()
        load_s = time.time() - t0
        assert engine.runner.model.layers[0].mlp.w4
    row = {"model": args.model, "layers": cfg.num_hidden_layers,
           "expert_tensors": cfg.num_hidden_layers * cfg.num_local_experts * 9,
           "checkpoint_gb": round(size / 1e9, 3),
           "write_s": round(write_s, 1), "engine_load_s": round(load_s, 1)}
    print(json.dumps(row), flush=True)
    return [row]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernel", "engine", "awq-load"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--blocks", default=",".join(BLOCKS))
    ap.add_argument("--ts", default=",".join(map(str, TS)))
    ap.add_argument("--max-copies", type=int, default=32)
    ap.add_argument("--model", default="qwen3-30b-a3b")
    ap.add_argument("--batches", default="1,8,64,256")
    ap.add_argument("--input-len", type=int, default=128)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--layers", type=int, default=0)
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available() or not ops.native_available():
        sys.exit("bench_w4_moe needs a GPU and the built extension")
    rows = {"kernel": bench_kernel, "engine": bench_engine,
            "awq-load": bench_awq_load}[args.what](args)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
