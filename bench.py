#!/usr/bin/env python3
"""Serving benchmark for the arks_amd engine (driver contract).

Measures the BASELINE.json headline: output tok/s (whole node) for
Qwen2.5-7B, bf16, synthetic data, random-init weights, plus p50 TTFT
(reported inside config). A "step" is one continuous-batching engine step
(decode over the full in-flight batch during the timed region).

Modes:
  --parallel dp  (default): each rank is an independent engine replica
                 (TP=1) — weak scaling, the reference's replica-scaling shape
                 (ArksApplication.spec.replicas).
  --parallel tp : all ranks form one tensor-parallel engine over RCCL/xGMI.

Launch (driver): python -m torch.distributed.run --nnodes=1 --nproc-per-node N
  --master-addr 127.0.0.1 bench.py --gpus N --steps K --warmup W

A plain run sets up, warms up, times the K steps and prints one JSON line.
  --dump-outputs DIR  also writes the last timed step's outputs as .npy
  --full              adds the secondary measurements (none at present)
"""

from __future__ import annotations

import argparse
import json
import os
import time

import torch


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=32)
    p.add_argument("--warmup", type=int, default=8)
    p.add_argument("--model", type=str, default="qwen2.5-7b")
    p.add_argument("--parallel", choices=["dp", "tp"], default="dp")
    p.add_argument("--batch", type=int, default=64, help="in-flight requests per engine")
    p.add_argument("--input-len", type=int, default=1024)
    p.add_argument("--seed", type=int, default=0)
    # NOT the headline config (BASELINE dtype is bf16): opt-in fp8 W8A8 run,
    # reported with dtype="fp8" so it is never mistaken for the bf16 number.
    p.add_argument("--quantization", choices=["fp8"], default=None)
    p.add_argument("--kv-cache-dtype", choices=["auto", "fp8"], default="auto")
    # opt-in: prompt-lookup speculative decoding (random-token synthetic
    # prompts rarely repeat, so this mostly measures the no-draft overhead;
    # acceptance-driven wins need repetitive real text)
    p.add_argument("--speculative", choices=["ngram", "draft"], default=None)
    p.add_argument("--draft-model", default=None,
                   help="draft checkpoint/preset for --speculative draft")
    # BASELINE's "model cold-start sec": write a random-init safetensors
    # checkpoint to disk once, drop the page cache, and time disk -> HBM
    # through the pinned double-buffer loader (not the synthetic
    # random-init path the serving bench uses).
    p.add_argument("--cold-start", action="store_true")
    p.add_argument("--ckpt-dir", default="/tmp/arks_ckpt")
    # After the timed steps, write what the last timed engine step returned
    # (and the logits it sampled from) as DIR/<name>.npy, so two builds can
    # be compared output for output. Inputs depend only on the arguments.
    p.add_argument("--dump-outputs", metavar="DIR", default=None)
    # A plain run does only what the headline figure needs. Secondary
    # measurements that would take runs of their own belong behind --full;
    # today there are none inside a plain run (cold start, fp8 and
    # speculation are separate invocations selected by their own options),
    # so --full currently adds nothing.
    p.add_argument("--full", action="store_true")
    return p.parse_args()


def run_cold_start(args):
    import glob
    import subprocess

    from arks_amd.config import EngineConfig, PRESET_CONFIGS
    from arks_amd.engine import LLMEngine
    from arks_amd.loader.safetensors_loader import save_random_checkpoint

    mcfg = PRESET_CONFIGS[args.model]
    ckpt = os.path.join(args.ckpt_dir, args.model)
    if not os.path.exists(os.path.join(ckpt, "config.json")):
        print(f"# writing random-init checkpoint to {ckpt} ...",
              file=os.sys.stderr)
        save_random_checkpoint(mcfg, ckpt, seed=args.seed)
    nbytes = sum(os.path.getsize(f)
                 for f in glob.glob(os.path.join(ckpt, "*.safetensors")))
    # evict the checkpoint's pages from the page cache so the read really
    # comes from disk (per file: needs no privilege, touches no host setting)
    try:
        subprocess.run(["sync"], check=False)
        for path in glob.glob(os.path.join(ckpt, "*.safetensors")):
            fd = os.open(path, os.O_RDONLY)
            try:
                os.posix_fadvise(fd, 0, 0, os.POSIX_FADV_DONTNEED)
            finally:
                os.close(fd)
        cache_dropped = True
    except (OSError, AttributeError):
        cache_dropped = False
    cfg = EngineConfig(
        model_path=ckpt,
        device="cuda" if torch.cuda.is_available() else "cpu",
        kv_cache_blocks=256,
        max_model_len=2048,
        max_num_seqs=8,
    )
    t0 = time.time()
    engine = LLMEngine(cfg)
    total_s = time.time() - t0
    load_s = engine.load_seconds
    result = {
        "metric": "model_cold_start_s",
        "value": round(total_s, 3),
        "unit": "s",
        "n_gpus": 1,
        "steps": 1,
        "warmup": 0,
        "ms_per_step": round(total_s * 1000.0, 1),
        "higher_is_better": False,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "bf16",
        "data": "random-init safetensors on disk",
        "config": {
            "model": args.model,
            "checkpoint_gb": round(nbytes / 1e9, 2),
            "weight_load_s": round(load_s, 3),
            "disk_to_hbm_gbps": round(nbytes / 1e9 / load_s, 2),
            "page_cache_dropped": cache_dropped,
        },
    }
    print(json.dumps(result))


# --dump-outputs stays well under 64 MB in all: logits above this many
# float32 bytes are cut to a fixed, seeded sample of vocabulary columns.
DUMP_LOGITS_MAX_BYTES = 48 * 1024 * 1024


def dump_outputs(args, engine, out):
    """Write the last timed step's results as DIR/<name>.npy (float64 ids,
    float32 logits), rows ordered by request so runs compare row for row."""
    import numpy as np

    os.makedirs(args.dump_outputs, exist_ok=True)
    # request ids are "bench-<i>"; a step returns them in scheduling order
    req = [int(o.request_id.rsplit("-", 1)[1]) for o in out]
    order = sorted(range(len(out)), key=lambda j: req[j])  # stable
    arrays = {
        "request_index": np.array([req[j] for j in order], dtype=np.float64),
        "new_token_ids": np.array(
            [out[j].new_token_id for j in order], dtype=np.float64),
    }
    # The logits the step sampled those tokens from are still in the decode
    # graph's output buffer (one row per sequence, in scheduling order).
    graphs = getattr(engine.runner, "_graphs", None) or {}
    sizes = [s for s in sorted(graphs) if s >= len(out)]
    if sizes and not args.speculative and len(set(req)) == len(out):
        logits = graphs[sizes[0]].logits[: len(out)].float().cpu()
        logits = logits[torch.tensor(order)]
        vocab = logits.shape[1]
        keep = DUMP_LOGITS_MAX_BYTES // (4 * max(len(out), 1))
        if keep < vocab:
            g = torch.Generator().manual_seed(args.seed)
            cols = torch.randperm(vocab, generator=g)[:keep].sort().values
            logits = logits[:, cols]
            arrays["logits_columns"] = cols.numpy().astype(np.float64)
        arrays["logits"] = logits.numpy().astype(np.float32)
    for name, arr in arrays.items():
        np.save(os.path.join(args.dump_outputs, name + ".npy"), arr)


def main():
    args = parse_args()
    if args.cold_start:
        run_cold_start(args)
        return
    rank = int(os.environ.get("RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    local_rank = int(os.environ.get("LOCAL_RANK", rank))
    use_gpu = torch.cuda.is_available()
    if use_gpu:
        torch.cuda.set_device(local_rank)

    import torch.distributed as dist

    from arks_amd.config import EngineConfig
    from arks_amd.engine import LLMEngine, SamplingParams
    from arks_amd.parallel import comm as tp_comm

    if args.parallel == "tp" and world > 1:
        tp_comm.init_tp()  # process group == TP group
    elif world > 1:
        dist.init_process_group(
            backend="nccl" if use_gpu else "gloo", rank=rank, world_size=world
        )

    def barrier():
        if world > 1:
            dist.barrier()
        if use_gpu:
            torch.cuda.synchronize()

    # KV pool sized for this run (keeps init fast; cache could hold far more
    # of the 288 GB).
    horizon = args.input_len + args.warmup + args.steps + 128
    blocks = (args.batch * horizon + 15) // 16 + 64
    cfg = EngineConfig(
        preset=args.model,
        device="cuda" if use_gpu else "cpu",
        max_num_seqs=max(args.batch, 256),
        max_num_batched_tokens=max(8192, args.input_len * 2),
        max_model_len=horizon,
        kv_cache_blocks=blocks,
        seed=args.seed,
        quantization=args.quantization,
        kv_cache_dtype=args.kv_cache_dtype,
        speculative=args.speculative,
        draft_model=args.draft_model,
    )
    t_load0 = time.time()
    engine = LLMEngine(cfg)
    load_s = time.time() - t_load0

    # One-time warmup outside any measurement: first-kernel compilation,
    # hipGraph captures and GEMM workspace allocation all happen here.
    engine.generate(
        [[1, 2, 3] * 16, [4, 5] * 8], SamplingParams(max_tokens=4, ignore_eos=True)
    )

    # Synthetic requests: random token ids, long enough to stay in decode
    # through the whole timed region.
    g = torch.Generator().manual_seed(args.seed + (0 if args.parallel == "tp" else rank))
    prompts = [
        torch.randint(0, engine.model_cfg.vocab_size - 1, (args.input_len,), generator=g).tolist()
        for _ in range(args.batch)
    ]
    sp = SamplingParams(max_tokens=args.warmup + args.steps + 64, ignore_eos=True)
    for i, pr in enumerate(prompts):
        engine.add_request(pr, sp, request_id=f"bench-{i}")

    # Run all prefills, then W untimed decode steps. TTFT = per-request
    # first-token latency from admission (p50 over the batch).
    while engine.scheduler.num_waiting > 0:
        engine.step()
    if use_gpu:
        torch.cuda.synchronize()
    ttfts = sorted(
        (s.first_token_time - s.arrival_time) * 1000.0
        for s in engine.scheduler.running
        if s.first_token_time is not None
    )
    ttft_ms = ttfts[len(ttfts) // 2] if ttfts else None
    out = []
    for _ in range(args.warmup):
        out = engine.step()
    barrier()

    # Timed region: exactly K decode steps over the full batch.
    t_start = time.time()
    tokens = 0
    for _ in range(args.steps):
        out = engine.step()
        tokens += len(out)
    if use_gpu:
        torch.cuda.synchronize()
    elapsed = time.time() - t_start
    barrier()

    # MAX elapsed across ranks; tokens aggregate over the job.
    if world > 1:
        te = torch.tensor([elapsed], dtype=torch.float64)
        tk = torch.tensor([tokens], dtype=torch.float64)
        if use_gpu:
            te, tk = te.cuda(), tk.cuda()
        dist.all_reduce(te, op=dist.ReduceOp.MAX)
        if args.parallel == "dp":
            dist.all_reduce(tk, op=dist.ReduceOp.SUM)  # replicas add up
        elapsed = float(te.item())
        tokens = int(tk.item())

    expect = args.batch * args.steps * (world if args.parallel == "dp" else 1)
    if args.speculative:
        # accepted drafts emit extra tokens per step
        assert tokens >= expect, "a sequence finished inside the timed region"
    else:
        assert tokens == expect, (
            "a sequence finished or was preempted inside the timed region"
        )

    if rank == 0 and args.dump_outputs:
        dump_outputs(args, engine, out)

    if rank == 0:
        n_gpus = world if use_gpu else args.gpus
        value = tokens / elapsed
        result = {
            "metric": "output_tok_s",
            "value": round(value, 2),
            "unit": "tok/s",
            "n_gpus": n_gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1000.0, 3),
            "higher_is_better": True,
            "scaling": "weak" if args.parallel == "dp" else "strong",
            "vs_baseline": None,
            "dtype": (args.quantization or "bf16")
            + ("+kv8" if args.kv_cache_dtype == "fp8" else ""),
            "data": "synthetic",
            "config": {
                "model": args.model,
                "global_batch": args.batch * (world if args.parallel == "dp" else 1),
                "seq_len": args.input_len,
                "parallelism": f"{args.parallel}{world}",
                "ttft_ms_p50": round(ttft_ms, 2) if ttft_ms is not None else None,
                "weight_load_s": round(load_s, 2),
                **({"spec_drafted": engine.spec_drafted_tokens,
                    "spec_accepted": engine.spec_accepted_tokens}
                   if args.speculative else {}),
            },
        }
        print(json.dumps(result))

    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
