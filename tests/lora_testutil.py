"""Shared helpers of the LoRA tests: the standard test adapters, a model
with an adapter MERGED into its weights (the yardstick the unmerged LoRA path
is measured against — it runs only code that knows nothing about LoRA), and
the prompt-logprob distance."""

from __future__ import annotations

import os

import torch

from arks_amd.config import PRESET_CONFIGS, EngineConfig
from arks_amd.engine import LLMEngine, SamplingParams
from arks_amd.loader.lora_loader import LORA_TARGETS, save_random_adapter

RANK, ALPHA, STD = 8, 16, 0.05
SEEDS = {"a": 1, "b": 2}
# wiring prompts: 12, 8 and 40 tokens
WIRING_PROMPTS = [
    [(7 * i + 3) % 500 + 1 for i in range(12)],
    [(11 * i + 5) % 500 + 1 for i in range(8)],
    [(13 * i + 2) % 500 + 1 for i in range(40)],
]
FUSED = {
    "qkv": ("q_proj", "k_proj", "v_proj"),
    "o": ("o_proj",),
    "gate_up": ("gate_proj", "up_proj"),
    "down": ("down_proj",),
}


def make_adapters(preset: str, root) -> dict[str, str]:
    """Write adapters "a" (seed 1) and "b" (seed 2) for `preset`."""
    out = {}
    for name, seed in SEEDS.items():
        path = os.path.join(str(root), f"{preset}-{name}")
        if not os.path.isdir(path):
            save_random_adapter(PRESET_CONFIGS[preset], path, rank=RANK,
                                alpha=ALPHA, targets=LORA_TARGETS, seed=seed,
                                std=STD)
        out[name] = path
    return out


def engine_cfg(preset: str, device: str, **kw) -> EngineConfig:
    base = dict(preset=preset, device=device, kv_cache_blocks=256,
                max_model_len=512, max_num_seqs=16)
    base.update(kw)
    return EngineConfig(**base)


class MergedModel:
    """One LoRA-less engine whose weights are rewritten in place to
    W + scale * B A for a chosen adapter, optionally leaving out one fused
    projection's delta."""

    def __init__(self, preset: str, device: str):
        self.engine = LLMEngine(engine_cfg(preset, device,
                                           enable_prefix_caching=False))
        self.layers = self.engine.runner.model.layers
        self.base = [self._weights(l) for l in self.layers]
        self.base = [{k: v.clone() for k, v in d.items()} for d in self.base]

    @staticmethod
    def _weights(layer) -> dict[str, torch.Tensor]:
        return {
            "qkv": layer.self_attn.qkv_proj.weight.data,
            "o": layer.self_attn.o_proj.weight.data,
            "gate_up": layer.mlp.gate_up_proj.weight.data,
            "down": layer.mlp.down_proj.weight.data,
        }

    def set(self, adapter_path: str | None, drop: tuple[int, str] | None = None):
        from safetensors.torch import load_file

        tensors = (load_file(os.path.join(adapter_path,
                                          "adapter_model.safetensors"))
                   if adapter_path else {})
        scale = ALPHA / RANK
        for li, layer in enumerate(self.layers):
            for fused, w in self._weights(layer).items():
                w.copy_(self.base[li][fused])
                if not adapter_path or drop == (li, fused):
                    continue
                deltas = []
                for t in FUSED[fused]:
                    block = "self_attn" if fused in ("qkv", "o") else "mlp"
                    pre = f"base_model.model.model.layers.{li}.{block}.{t}"
                    A = tensors[f"{pre}.lora_A.weight"].float()
                    B = tensors[f"{pre}.lora_B.weight"].float()
                    deltas.append(scale * (B @ A))
                delta = torch.cat(deltas, dim=0).to(w.device)
                w.copy_((self.base[li][fused].float() + delta).to(w.dtype))
        return self

    def logprobs(self, prompts=WIRING_PROMPTS):
        return prompt_logprobs(self.engine, prompts)


def prompt_logprobs(engine: LLMEngine, prompts, lora: str | None = None):
    sp = SamplingParams(max_tokens=1, ignore_eos=True, prompt_logprobs=True)
    seqs = [engine.add_request(list(p), sp, lora=lora) for p in prompts]
    while engine.has_work():
        engine.step()
    return [list(s.prompt_logprob_values) for s in seqs]


def dist(x, y) -> float:
    """Max absolute difference of two prompt_logprob_values sets."""
    assert [len(a) for a in x] == [len(b) for b in y]
    return max(abs(p - q) for a, b in zip(x, y) for p, q in zip(a, b))


def wiring_distances(preset: str, device: str, adapters: dict[str, str]):
    """-> (d, d_drop, d_neg): the LoRA engine under "a" against the merged-a
    model; the smallest distance any single left-out fused projection causes
    (merged-a against merged-a-minus-one, LoRA-free code only); the LoRA
    engine under "a" against the merged-b model (negative control)."""
    mm = MergedModel(preset, device)
    merged_a = mm.set(adapters["a"]).logprobs()
    drops = {}
    for li in range(len(mm.layers)):
        for fused in FUSED:
            drops[(li, fused)] = dist(
                merged_a, mm.set(adapters["a"], drop=(li, fused)).logprobs())
    merged_b = mm.set(adapters["b"]).logprobs()
    del mm
    eng = LLMEngine(engine_cfg(preset, device, enable_lora=True,
                               lora_modules=adapters))
    got = prompt_logprobs(eng, WIRING_PROMPTS, lora="a")
    d, d_drop, d_neg = dist(got, merged_a), min(drops.values()), dist(got, merged_b)
    print(f"[lora wiring {preset}/{device}] d={d:.5f} d_drop={d_drop:.5f} "
          f"(per projection: "
          + ", ".join(f"L{k[0]}.{k[1]}={v:.4f}" for k, v in drops.items())
          + f") d_neg={d_neg:.5f}")
    return d, d_drop, d_neg


def run_mixed(engine: LLMEngine, reqs, late: int, late_steps: int = 5,
              max_tokens: int = 10):
    """Run (prompt, lora) requests in one engine; request `late` is added
    after `late_steps` steps, so its prefill shares a step with decodes."""
    sp = SamplingParams(max_tokens=max_tokens, ignore_eos=True)
    seqs = {}
    for i, (p, l) in enumerate(reqs):
        if i != late:
            seqs[i] = engine.add_request(list(p), sp, lora=l)
    for _ in range(late_steps):
        engine.step()
    p, l = reqs[late]
    seqs[late] = engine.add_request(list(p), sp, lora=l)
    while engine.has_work():
        engine.step()
    return [seqs[i].output_token_ids for i in range(len(reqs))]
