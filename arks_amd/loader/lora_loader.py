"""PEFT-format LoRA adapters -> fixed GPU slots of the fused, TP-sharded
linear layers.

An adapter directory holds adapter_config.json + adapter_model.safetensors
with keys
``base_model.model.model.layers.{i}.{self_attn|mlp}.{proj}.lora_{A|B}.weight``
(A is [r, in], B is [out, r]). `peft` itself is not needed.

Slot layout per adapted layer (arks_amd/parallel/layers.py LoRAState):
A [max_loras, S*R, K] and B [max_loras, N, R] bf16 over the layer's LOCAL
widths, R = max_lora_rank, S fused slices (3 qkv, 2 gate_up, 1 o/down).
Slice s uses rows [s*R, (s+1)*R) of A; smaller ranks are zero-padded; the
LoRA scale (alpha/r, or alpha/sqrt(r) with rsLoRA) is folded into B in fp32
before the bf16 cast. Column-parallel layers replicate A and shard B as the
base weight; row-parallel layers shard A along K and keep B whole (the delta
joins the local partial sum before the all-reduce).
"""

from __future__ import annotations

import json
import math
import os
import re

import torch

from ..parallel.layers import LoRAState

ATTN_TARGETS = ("q_proj", "k_proj", "v_proj", "o_proj")
MLP_TARGETS = ("gate_proj", "up_proj", "down_proj")
LORA_TARGETS = ATTN_TARGETS + MLP_TARGETS

_KEY_RE = re.compile(
    r"^base_model\.model\.model\.layers\.(\d+)\.(self_attn|mlp)\."
    r"(\w+)\.lora_([AB])\.weight$"
)


def _fused_layers(layer) -> dict[str, tuple]:
    """fused layer name -> (module, per-projection target names)."""
    out = {
        "qkv_proj": (layer.self_attn.qkv_proj, ("q_proj", "k_proj", "v_proj")),
        "o_proj": (layer.self_attn.o_proj, ("o_proj",)),
    }
    if getattr(layer, "_dense_mlp", False):
        out["gate_up_proj"] = (layer.mlp.gate_up_proj, ("gate_proj", "up_proj"))
        out["down_proj"] = (layer.mlp.down_proj, ("down_proj",))
    return out


def _local_shape(mod) -> tuple[int, int]:
    """(N, K) of a linear layer's local weight, W4/W8-quantized or not."""
    if getattr(mod, "w8", False):
        return mod.w8_shape
    if getattr(mod, "mx4", False):
        return mod.mx4_shape
    return mod.w4_shape if getattr(mod, "w4", False) else tuple(mod.weight.shape)


def _slice_offsets(name: str, mod) -> tuple[int, ...]:
    if name == "qkv_proj":
        q = mod.nq_local * mod.head_dim
        kv = mod.nkv_local * mod.head_dim
        return (0, q, q + kv, q + 2 * kv)
    if name == "gate_up_proj":
        n = _local_shape(mod)[0]
        return (0, n // 2, n)
    return (0, _local_shape(mod)[0])


def allocate_lora_slots(model, max_loras: int, max_rank: int, device,
                        workspace_rows: int) -> int:
    """Attach zeroed slot tensors (LoRAState) to every adaptable linear layer
    and one shared f32 shrink workspace. Returns the bytes allocated. Fails
    when a layer's local shape does not meet the kernels' requirements —
    there is no fallback path."""
    R = max_rank
    h_ws = torch.zeros(workspace_rows * 3 * R, dtype=torch.float32,
                       device=device)
    total = h_ws.numel() * 4
    for li, layer in enumerate(model.layers):
        for name, (mod, targets) in _fused_layers(layer).items():
            N, K = _local_shape(mod)
            offs = _slice_offsets(name, mod)
            if K % 32 != 0 or N % 16 != 0 or any(o % 16 for o in offs):
                raise ValueError(
                    f"LoRA cannot adapt layers.{li}.{name}: the kernels need "
                    f"local K % 32 == 0, N % 16 == 0 and slice offsets in "
                    f"multiples of 16 (K={K}, N={N}, offsets={offs})"
                )
            S = len(targets)
            A = torch.zeros(max_loras, S * R, K, dtype=torch.bfloat16,
                            device=device)
            B = torch.zeros(max_loras, N, R, dtype=torch.bfloat16,
                            device=device)
            mod.lora = LoRAState(A, B, offs, h_ws)
            total += (A.numel() + B.numel()) * 2
    return total


def read_adapter_config(path: str, max_rank: int, model_cfg) -> dict:
    """Read and validate adapter_config.json; ValueError names the reason."""
    cfg_path = os.path.join(path, "adapter_config.json")
    if not os.path.isfile(cfg_path):
        raise ValueError(f"no adapter_config.json in {path!r}")
    with open(cfg_path) as f:
        cfg = json.load(f)
    r = cfg.get("r")
    if not isinstance(r, int) or r < 1:
        raise ValueError(f"adapter {path!r}: bad rank r={r!r}")
    if r > max_rank:
        raise ValueError(
            f"adapter {path!r}: rank r={r} exceeds max_lora_rank={max_rank}"
        )
    if cfg.get("use_dora"):
        raise ValueError(f"adapter {path!r}: use_dora (DoRA) is not supported")
    for field in ("modules_to_save", "rank_pattern", "alpha_pattern"):
        if cfg.get(field):
            raise ValueError(
                f"adapter {path!r}: non-empty {field} is not supported"
            )
    if cfg.get("bias", "none") != "none":
        raise ValueError(
            f"adapter {path!r}: bias={cfg['bias']!r} is not supported "
            "(only bias='none')"
        )
    targets = cfg.get("target_modules") or []
    if isinstance(targets, str):
        targets = [targets]
    for t in targets:
        if t in ("embed_tokens", "lm_head"):
            raise ValueError(
                f"adapter {path!r}: embedding / lm_head adapters "
                f"({t}) are not supported"
            )
        if t not in LORA_TARGETS:
            raise ValueError(
                f"adapter {path!r}: target module {t!r} is not one of "
                f"{', '.join(LORA_TARGETS)}"
            )
        if model_cfg.num_local_experts > 0 and t in MLP_TARGETS:
            raise ValueError(
                f"adapter {path!r}: MLP/expert target {t!r} on an MoE model "
                "(MoE models take attention-projection adapters only)"
            )
    return cfg


def lora_scale(cfg: dict) -> float:
    r = cfg["r"]
    alpha = cfg.get("lora_alpha", r)
    return alpha / math.sqrt(r) if cfg.get("use_rslora") else alpha / r


def _full_shapes(model_cfg) -> dict[str, tuple[int, int]]:
    """target -> (out, in) of the unsharded projection."""
    H, I, hd = (model_cfg.hidden_size, model_cfg.intermediate_size,
                model_cfg.head_dim)
    nq, nkv = model_cfg.num_attention_heads, model_cfg.num_key_value_heads
    return {
        "q_proj": (nq * hd, H), "k_proj": (nkv * hd, H),
        "v_proj": (nkv * hd, H), "o_proj": (H, nq * hd),
        "gate_proj": (I, H), "up_proj": (I, H), "down_proj": (H, I),
    }


def read_adapter(path: str, max_rank: int, model_cfg):
    """-> (config, {(layer, target): (A [r, in], B [out, r])}) validated
    against the model's shapes."""
    from safetensors.torch import load_file

    cfg = read_adapter_config(path, max_rank, model_cfg)
    st_path = os.path.join(path, "adapter_model.safetensors")
    if not os.path.isfile(st_path):
        raise ValueError(f"no adapter_model.safetensors in {path!r}")
    tensors = load_file(st_path)
    r = cfg["r"]
    shapes = _full_shapes(model_cfg)
    pairs: dict[tuple[int, str], dict[str, torch.Tensor]] = {}
    for key, t in tensors.items():
        m = _KEY_RE.match(key)
        if m is None:
            if "embed_tokens" in key or "lm_head" in key:
                raise ValueError(
                    f"adapter {path!r}: embedding / lm_head adapter tensor "
                    f"{key!r} is not supported"
                )
            raise ValueError(f"adapter {path!r}: unexpected tensor {key!r}")
        li, block, proj, ab = int(m[1]), m[2], m[3], m[4]
        want_block = "self_attn" if proj in ATTN_TARGETS else "mlp"
        if proj not in LORA_TARGETS or block != want_block:
            raise ValueError(
                f"adapter {path!r}: target {block}.{proj} is not one of "
                f"{', '.join(LORA_TARGETS)}"
            )
        if model_cfg.num_local_experts > 0 and proj in MLP_TARGETS:
            raise ValueError(
                f"adapter {path!r}: MLP/expert target {proj!r} on an MoE "
                "model (attention-projection adapters only)"
            )
        if li >= model_cfg.num_hidden_layers:
            raise ValueError(
                f"adapter {path!r}: layer {li} beyond the model's "
                f"{model_cfg.num_hidden_layers} layers"
            )
        out_f, in_f = shapes[proj]
        want = (r, in_f) if ab == "A" else (out_f, r)
        if tuple(t.shape) != want:
            raise ValueError(
                f"adapter {path!r}: shape mismatch for {key}: "
                f"{tuple(t.shape)} != {want}"
            )
        pairs.setdefault((li, proj), {})[ab] = t
    out = {}
    for (li, proj), d in pairs.items():
        if set(d) != {"A", "B"}:
            raise ValueError(
                f"adapter {path!r}: layers.{li}.{proj} lacks lora_A or lora_B"
            )
        out[(li, proj)] = (d["A"], d["B"])
    return cfg, out


def _pad_rows(t: torch.Tensor, rows: int) -> torch.Tensor:
    out = torch.zeros(rows, t.shape[1], dtype=t.dtype)
    out[: t.shape[0]] = t
    return out


def load_adapter_into_slot(model, model_cfg, path: str, slot: int,
                           max_rank: int) -> None:
    """Copy one PEFT adapter into slot `slot` of every adapted layer, in
    place (pointers stay put after graph capture). Targets the adapter
    lacks leave zeros in their slice."""
    cfg, pairs = read_adapter(path, max_rank, model_cfg)
    scale = lora_scale(cfg)
    R = max_rank
    r = cfg["r"]
    shapes = _full_shapes(model_cfg)
    for li, layer in enumerate(model.layers):
        for name, (mod, targets) in _fused_layers(layer).items():
            st: LoRAState | None = mod.lora
            if st is None:
                raise ValueError("LoRA slots are not allocated (enable_lora)")
            a_rows, b_full = [], []
            for t in targets:
                if (li, t) in pairs:
                    A, B = pairs[(li, t)]
                    A = A.float()
                    # fold the scale in fp32, then one cast to bf16
                    B = B.float() * scale
                else:
                    out_f, in_f = shapes[t]
                    A = torch.zeros(r, in_f)
                    B = torch.zeros(out_f, r)
                a_rows.append(_pad_rows(A, R))                    # [R, in]
                b_full.append(_pad_rows(B.t().contiguous(), R).t())  # [out, R]
            if name == "qkv_proj":
                b_parts = mod.shard_qkv_parts(*b_full)
            elif name == "gate_up_proj":
                b_parts = mod.shard_merged_parts(*b_full)
            else:  # row-parallel: A sharded along K, B whole
                a_rows = [mod.shard(a_rows[0])]
                b_parts = b_full
            A_slot = torch.cat(a_rows, dim=0)
            B_slot = torch.cat(list(b_parts), dim=0)
            assert A_slot.shape == st.A.shape[1:], (A_slot.shape, st.A.shape)
            assert B_slot.shape == st.B.shape[1:], (B_slot.shape, st.B.shape)
            st.A[slot].copy_(A_slot.to(torch.bfloat16))
            st.B[slot].copy_(B_slot.to(torch.bfloat16))


def save_random_adapter(model_cfg, out_dir: str, rank: int = 8,
                        alpha: float = 16, targets=LORA_TARGETS,
                        seed: int = 0, std: float = 0.05,
                        use_rslora: bool = False) -> None:
    """Write a random PEFT-layout adapter (adapter_config.json +
    adapter_model.safetensors) for tests and benchmarks. Both A and B are
    random, so the adapter changes the model's outputs."""
    from safetensors.torch import save_file

    g = torch.Generator().manual_seed(seed)
    shapes = _full_shapes(model_cfg)
    out: dict[str, torch.Tensor] = {}
    for li in range(model_cfg.num_hidden_layers):
        for t in targets:
            block = "self_attn" if t in ATTN_TARGETS else "mlp"
            out_f, in_f = shapes[t]
            pre = f"base_model.model.model.layers.{li}.{block}.{t}"
            out[f"{pre}.lora_A.weight"] = (
                torch.randn(rank, in_f, generator=g) * std).to(torch.bfloat16)
            out[f"{pre}.lora_B.weight"] = (
                torch.randn(out_f, rank, generator=g) * std).to(torch.bfloat16)
    os.makedirs(out_dir, exist_ok=True)
    save_file(out, os.path.join(out_dir, "adapter_model.safetensors"))
    with open(os.path.join(out_dir, "adapter_config.json"), "w") as f:
        json.dump({
            "peft_type": "LORA",
            "r": rank,
            "lora_alpha": alpha,
            "target_modules": list(targets),
            "bias": "none",
            "use_rslora": use_rslora,
            "use_dora": False,
            "modules_to_save": None,
            "rank_pattern": {},
            "alpha_pattern": {},
        }, f, indent=1)
