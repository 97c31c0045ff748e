"""Model and engine configuration.

ModelConfig is HF-config-driven: it reads the same config.json fields the
reference's delegated runtimes (vLLM/SGLang at reference
arksapplication_controller.go:941-1014) consume, so any Qwen2/Llama-family
checkpoint directory works unchanged.
"""

from __future__ import annotations

import json
import os
from dataclasses import dataclass


_BASE_MODEL_ARCHS = {
    "Qwen3Model": "Qwen3ForCausalLM",
    "Qwen2Model": "Qwen2ForCausalLM",
    "MistralModel": "MistralForCausalLM",
    "LlamaModel": "LlamaForCausalLM",
}


@dataclass
class ModelConfig:
    architecture: str = "Qwen2ForCausalLM"
    vocab_size: int = 151936
    hidden_size: int = 3584
    intermediate_size: int = 18944
    num_hidden_layers: int = 28
    num_attention_heads: int = 28
    num_key_value_heads: int = 4
    head_dim: int = 128
    rms_norm_eps: float = 1e-6
    rope_theta: float = 1000000.0
    max_position_embeddings: int = 32768
    # HF rope_scaling dict: {"rope_type": "llama3"|"yarn"|"linear", ...}
    rope_scaling: dict | None = None
    # Mixtral-style sparse MoE (0 experts = dense MLP)
    num_local_experts: int = 0
    num_experts_per_tok: int = 2
    moe_intermediate_size: int | None = None  # per-expert FFN width (MoE)
    shared_expert_intermediate_size: int | None = None  # Qwen2-MoE
    norm_topk_prob: bool = True  # renormalize top-k routing weights
    sliding_window: int | None = None  # sliding-window attention size
    # Qwen2-style per-layer mixing: layers >= max_window_layers slide,
    # lower layers use full attention (HF layer_types overrides when set)
    max_window_layers: int | None = None
    layer_types: list | None = None
    qk_norm: bool = False  # Qwen3: per-head RMSNorm on q/k before RoPE
    # SmolLM3 NoPE: no_rope_layers[i] == 1 -> layer i USES RoPE, 0 -> the
    # layer attends without positional encoding (HF configuration_smollm3
    # semantics; default = one NoPE layer every no_rope_layer_interval)
    no_rope_layers: list | None = None
    tie_word_embeddings: bool = False
    attention_bias: bool = True  # qwen2 has qkv bias; llama does not
    eos_token_id: int = 151645
    bos_token_id: int = 151643
    torch_dtype: str = "bfloat16"
    # "awq" when the checkpoint's quantization_config declares 4-bit AWQ,
    # "fp8_block" when it declares block-scaled FP8 (e4m3, 128x128 blocks,
    # f32 scales, dynamic activations), "mxfp4" when it declares a Quark
    # MXFP4 export (e2m1 weights, e8m0 scale per 32); None for plain
    # checkpoints
    quant_method: str | None = None
    # fp8_block: module-name fragments the checkpoint left unquantized
    # (modules_to_not_convert / ignored_layers); mxfp4: the export's
    # `exclude` list (module names, fnmatch patterns allowed)
    quant_skip_modules: tuple = ()

    def __post_init__(self):
        # Sliding-window attention is implemented end to end: the
        # attention kernels mask keys outside each query's per-layer
        # window (layer_window: Mistral = all layers; Qwen2
        # max_window_layers / layer_types mixing honored) and the engine
        # drops out-of-window KV pages when EVERY layer slides
        # (uniform_window).
        if self.sliding_window is not None and self.sliding_window <= 0:
            raise ValueError(
                f"invalid sliding_window={self.sliding_window}"
            )

    def layer_uses_rope(self, layer_idx: int) -> bool:
        if self.no_rope_layers is None:
            return True
        return bool(self.no_rope_layers[layer_idx])

    def layer_window(self, layer_idx: int) -> int:
        """Effective attention window for one layer (0 = full attention).
        HF Qwen2 semantics: layer_types wins when present; otherwise
        layers >= max_window_layers slide and lower layers are full."""
        if self.sliding_window is None:
            return 0
        if self.layer_types is not None:
            return (self.sliding_window
                    if self.layer_types[layer_idx] == "sliding_attention"
                    else 0)
        if self.max_window_layers is not None:
            return self.sliding_window if layer_idx >= self.max_window_layers else 0
        return self.sliding_window

    def uniform_window(self) -> int:
        """The window when EVERY layer slides (else 0): KV page dropping
        and the prefix-cache gate need all layers windowed — a single
        full-attention layer keeps the whole history live."""
        ws = [self.layer_window(i) for i in range(self.num_hidden_layers)]
        return ws[0] if ws and all(w == ws[0] and w > 0 for w in ws) else 0

    @staticmethod
    def _check_quantization_config(qc: dict | None) -> str | None:
        """Accepts exactly AutoAWQ 4-bit, group 128, zero-point, "GEMM"
        layout; anything else raises naming the offending field."""
        if not qc:
            return None
        if str(qc.get("quant_method")).lower() == "fp8":
            return ModelConfig._check_fp8_config(qc)
        if str(qc.get("quant_method")).lower() == "quark":
            return ModelConfig._check_quark_config(qc)
        want = {"quant_method": "awq", "bits": 4, "group_size": 128,
                "zero_point": True, "version": "gemm"}
        for field, ok in want.items():
            got = qc.get(field)
            if isinstance(got, str):
                got = got.lower()
            if got != ok or (field == "zero_point" and got is not True):
                raise ValueError(
                    f"unsupported quantization_config: {field}="
                    f"{qc.get(field)!r} (only {field}={ok!r} is supported; "
                    "the engine reads 4-bit AWQ, group size 128, with "
                    "zero-points, GEMM layout)"
                )
        return "awq"

    @staticmethod
    def _check_fp8_config(qc: dict) -> str:
        """Accepts exactly the block-scaled FP8 format transformers writes
        ("fine-grained FP8": Qwen3-*-FP8, DeepSeek-V3 style): e4m3 weights,
        128x128 blocks with f32 scales, dynamic activation scheme; anything
        else raises naming the offending field."""
        want = {"fmt": "e4m3", "weight_block_size": [128, 128],
                "activation_scheme": "dynamic"}
        for field, ok in want.items():
            got = qc.get(field)
            if isinstance(got, str):
                got = got.lower()
            if isinstance(got, tuple):
                got = list(got)
            if got != ok:
                raise ValueError(
                    f"unsupported quantization_config: {field}="
                    f"{qc.get(field)!r} (only {field}={ok!r} is supported; "
                    "the engine reads block-scaled FP8 with e4m3 weights, "
                    "128x128 blocks, f32 scales and dynamic activations)"
                )
        scale_fmt = qc.get("scale_fmt")
        if scale_fmt is not None and str(scale_fmt).lower() != "float":
            raise ValueError(
                f"unsupported quantization_config: scale_fmt={scale_fmt!r} "
                "(only scale_fmt='float' or none is supported; the engine "
                "reads block-scaled FP8 with f32 scales)"
            )
        return "fp8_block"

    @staticmethod
    def _check_quark_config(qc: dict) -> str:
        """Accepts exactly the MXFP4 weight-only reading of a Quark export
        (the amd/*-MXFP4 checkpoints): global_quant_config.weight is static
        fp4, per group of 32 with e8m0 scales, stored real_quantized; no
        per-layer overrides, no quantized outputs, bias or KV cache; anything
        else raises naming the offending field. input_tensors may be null or
        a DYNAMIC spec, which is accepted and ignored: the activations stay
        bf16 here, more precise than the checkpoint asks for. Static input
        scales are refused (they would be tensors the engine never reads)."""
        tail = ("the engine reads Quark MXFP4 with static fp4 weights, "
                "per_group scales of group size 32 in e8m0, weights only")

        def bad(field, got, ok):
            return ValueError(
                f"unsupported quantization_config: {field}={got!r} (only "
                f"{field}={ok} is supported; {tail})")

        glob = qc.get("global_quant_config")
        if not isinstance(glob, dict):
            raise bad("global_quant_config", glob, "{weight: ...}")
        weight = glob.get("weight")
        if not isinstance(weight, dict):
            raise bad("global_quant_config.weight", weight, "an fp4 spec")
        want = {"dtype": "fp4", "qscheme": "per_group", "group_size": 32,
                "scale_format": "e8m0", "is_dynamic": False}
        for field, ok in want.items():
            got = weight.get(field)
            if isinstance(got, str):
                got = got.lower()
            if got != ok or isinstance(got, bool) != isinstance(ok, bool):
                raise bad(f"global_quant_config.weight.{field}",
                          weight.get(field), repr(ok))
        inp = glob.get("input_tensors")
        if inp is not None:
            if not isinstance(inp, dict) or inp.get("is_dynamic") is not True:
                raise bad("global_quant_config.input_tensors", inp,
                          "null or a dynamic spec (is_dynamic=true)")
        for field in ("output_tensors", "bias"):
            if glob.get(field) is not None:
                raise bad(f"global_quant_config.{field}", glob.get(field),
                          "null")
        for field in ("layer_quant_config", "layer_type_quant_config"):
            if qc.get(field):
                raise bad(field, qc.get(field), "{}")
        export = qc.get("export") or {}
        if not isinstance(export, dict):
            raise bad("export", export, "{...}")
        if export.get("kv_cache_group"):
            raise bad("export.kv_cache_group", export.get("kv_cache_group"),
                      "[]")
        wf = export.get("weight_format", "real_quantized")
        if str(wf).lower() != "real_quantized":
            raise bad("export.weight_format", wf, "'real_quantized'")
        return "mxfp4"

    @staticmethod
    def _fp8_skip_modules(qc: dict | None) -> tuple:
        """modules_to_not_convert and its alias ignored_layers, merged; for
        a Quark MXFP4 checkpoint its `exclude` list (module names, fnmatch
        patterns allowed)."""
        if qc and str(qc.get("quant_method")).lower() == "quark":
            val = qc.get("exclude") or []
            if isinstance(val, str) or not all(isinstance(v, str)
                                               for v in val):
                raise ValueError(
                    f"unsupported quantization_config: exclude={val!r} "
                    "(expected a list of module names)")
            return tuple(dict.fromkeys(val))
        if not qc or str(qc.get("quant_method")).lower() != "fp8":
            return ()
        out: list[str] = []
        for key in ("modules_to_not_convert", "ignored_layers"):
            val = qc.get(key) or []
            if isinstance(val, str) or not all(isinstance(v, str)
                                               for v in val):
                raise ValueError(
                    f"unsupported quantization_config: {key}={val!r} "
                    "(expected a list of module names)")
            out.extend(v for v in val if v not in out)
        return tuple(out)

    @classmethod
    def from_hf_config(cls, cfg: dict) -> "ModelConfig":
        arch = (cfg.get("architectures") or ["Qwen2ForCausalLM"])[0]
        # base-model checkpoints (embedding models: Qwen3-Embedding ships as
        # Qwen3Model, e5-mistral as MistralModel) are the same decoder stack
        # without the lm_head
        arch = _BASE_MODEL_ARCHS.get(arch, arch)
        num_heads = cfg.get("num_attention_heads", 28)
        hidden = cfg.get("hidden_size", 3584)
        eos = cfg.get("eos_token_id", 151645)
        if isinstance(eos, list):
            eos = eos[0]
        return cls(
            architecture=arch,
            vocab_size=cfg.get("vocab_size", 151936),
            hidden_size=hidden,
            intermediate_size=cfg.get("intermediate_size", 18944),
            num_hidden_layers=cfg.get("num_hidden_layers", 28),
            num_attention_heads=num_heads,
            num_key_value_heads=cfg.get("num_key_value_heads", num_heads),
            head_dim=cfg.get("head_dim", hidden // num_heads),
            rms_norm_eps=cfg.get("rms_norm_eps", 1e-6),
            rope_theta=cfg.get("rope_theta", 10000.0),
            max_position_embeddings=cfg.get("max_position_embeddings", 32768),
            rope_scaling=cfg.get("rope_scaling"),
            qk_norm=arch.startswith("Qwen3"),
            no_rope_layers=(
                cfg["no_rope_layers"] if cfg.get("no_rope_layers") is not None
                else [int((i + 1) % cfg.get("no_rope_layer_interval", 4) != 0)
                      for i in range(cfg.get("num_hidden_layers", 28))]
                if arch == "SmolLM3ForCausalLM" else None),
            num_local_experts=cfg.get("num_local_experts",
                                      cfg.get("num_experts", 0)),
            # Qwen2-family configs declare a window but disable it
            sliding_window=(cfg.get("sliding_window")
                            if cfg.get("use_sliding_window", True) else None),
            max_window_layers=cfg.get("max_window_layers"),
            layer_types=cfg.get("layer_types"),
            num_experts_per_tok=cfg.get("num_experts_per_tok", 2),
            moe_intermediate_size=cfg.get("moe_intermediate_size"),
            shared_expert_intermediate_size=cfg.get(
                "shared_expert_intermediate_size"),
            norm_topk_prob=cfg.get("norm_topk_prob", "num_local_experts" in cfg),
            tie_word_embeddings=cfg.get("tie_word_embeddings", False),
            attention_bias=cfg.get("attention_bias", arch == "Qwen2ForCausalLM"
                                   or arch == "Qwen2MoeForCausalLM"),
            eos_token_id=eos,
            bos_token_id=cfg.get("bos_token_id", 1),
            torch_dtype=cfg.get("torch_dtype", "bfloat16"),
            quant_method=cls._check_quantization_config(
                cfg.get("quantization_config")),
            quant_skip_modules=cls._fp8_skip_modules(
                cfg.get("quantization_config")),
        )

    @classmethod
    def from_pretrained(cls, model_path: str) -> "ModelConfig":
        with open(os.path.join(model_path, "config.json")) as f:
            return cls.from_hf_config(json.load(f))

    @property
    def num_qo_heads(self) -> int:
        return self.num_attention_heads


# Named synthetic configs for benchmarks / tests (random-init weights; no
# network access for real checkpoints — BASELINE.json's models by shape).
PRESET_CONFIGS: dict[str, ModelConfig] = {
    "qwen2.5-0.5b": ModelConfig(
        architecture="Qwen2ForCausalLM",
        vocab_size=151936,
        hidden_size=896,
        intermediate_size=4864,
        num_hidden_layers=24,
        num_attention_heads=14,
        num_key_value_heads=2,
        head_dim=64,
        rope_theta=1000000.0,
        tie_word_embeddings=True,
    ),
    "qwen2.5-7b": ModelConfig(
        architecture="Qwen2ForCausalLM",
        vocab_size=152064,
        hidden_size=3584,
        intermediate_size=18944,
        num_hidden_layers=28,
        num_attention_heads=28,
        num_key_value_heads=4,
        head_dim=128,
        rope_theta=1000000.0,
    ),
    "qwen2.5-32b": ModelConfig(
        architecture="Qwen2ForCausalLM",
        vocab_size=152064,
        hidden_size=5120,
        intermediate_size=27648,
        num_hidden_layers=64,
        num_attention_heads=40,
        num_key_value_heads=8,
        head_dim=128,
        rope_theta=1000000.0,
    ),
    "llama-3-8b": ModelConfig(
        architecture="LlamaForCausalLM",
        vocab_size=128256,
        hidden_size=4096,
        intermediate_size=14336,
        num_hidden_layers=32,
        num_attention_heads=32,
        num_key_value_heads=8,
        head_dim=128,
        rms_norm_eps=1e-5,
        rope_theta=500000.0,
        attention_bias=False,
        eos_token_id=128001,
        bos_token_id=128000,
    ),
    "llama-3-70b": ModelConfig(
        architecture="LlamaForCausalLM",
        vocab_size=128256,
        hidden_size=8192,
        intermediate_size=28672,
        num_hidden_layers=80,
        num_attention_heads=64,
        num_key_value_heads=8,
        head_dim=128,
        rms_norm_eps=1e-5,
        rope_theta=500000.0,
        attention_bias=False,
        eos_token_id=128001,
        bos_token_id=128000,
    ),
    "mistral-7b": ModelConfig(  # v0.1: global sliding window 4096
        architecture="MistralForCausalLM",
        vocab_size=32000,
        hidden_size=4096,
        intermediate_size=14336,
        num_hidden_layers=32,
        num_attention_heads=32,
        num_key_value_heads=8,
        head_dim=128,
        rms_norm_eps=1e-5,
        rope_theta=10000.0,
        attention_bias=False,
        sliding_window=4096,
        eos_token_id=2,
        bos_token_id=1,
    ),
    "mixtral-8x7b": ModelConfig(
        architecture="MixtralForCausalLM",
        vocab_size=32000,
        hidden_size=4096,
        intermediate_size=14336,  # per expert
        num_hidden_layers=32,
        num_attention_heads=32,
        num_key_value_heads=8,
        head_dim=128,
        rms_norm_eps=1e-5,
        rope_theta=1000000.0,
        attention_bias=False,
        num_local_experts=8,
        num_experts_per_tok=2,
        eos_token_id=2,
        bos_token_id=1,
    ),
    "tiny-moe": ModelConfig(  # CPU-test-sized sparse MoE
        architecture="MixtralForCausalLM",
        vocab_size=512,
        hidden_size=128,
        intermediate_size=192,
        num_hidden_layers=2,
        num_attention_heads=4,
        num_key_value_heads=2,
        head_dim=32,
        rope_theta=10000.0,
        max_position_embeddings=2048,
        attention_bias=False,
        num_local_experts=4,
        num_experts_per_tok=2,
        eos_token_id=2,
        bos_token_id=1,
    ),
    "qwen3-8b": ModelConfig(
        architecture="Qwen3ForCausalLM",
        vocab_size=151936,
        hidden_size=4096,
        intermediate_size=12288,
        num_hidden_layers=36,
        num_attention_heads=32,
        num_key_value_heads=8,
        head_dim=128,
        rope_theta=1000000.0,
        attention_bias=False,
        qk_norm=True,
    ),
    "tiny-qwen3": ModelConfig(  # CPU-test-sized qk-norm arch
        architecture="Qwen3ForCausalLM",
        vocab_size=512,
        hidden_size=128,
        intermediate_size=256,
        num_hidden_layers=2,
        num_attention_heads=4,
        num_key_value_heads=2,
        head_dim=32,
        rope_theta=10000.0,
        max_position_embeddings=2048,
        attention_bias=False,
        qk_norm=True,
        eos_token_id=2,
        bos_token_id=1,
    ),
    "tiny-qwen2moe": ModelConfig(  # CPU-test-sized Qwen2-MoE (shared expert)
        architecture="Qwen2MoeForCausalLM",
        vocab_size=512,
        hidden_size=128,
        intermediate_size=256,
        moe_intermediate_size=96,
        shared_expert_intermediate_size=160,
        num_hidden_layers=2,
        num_attention_heads=4,
        num_key_value_heads=2,
        head_dim=32,
        rope_theta=10000.0,
        max_position_embeddings=2048,
        attention_bias=True,
        num_local_experts=4,
        num_experts_per_tok=2,
        norm_topk_prob=False,
        eos_token_id=2,
        bos_token_id=1,
    ),
    "tiny-qwen3moe": ModelConfig(  # CPU-test-sized Qwen3-MoE
        architecture="Qwen3MoeForCausalLM",
        vocab_size=512,
        hidden_size=128,
        intermediate_size=256,
        moe_intermediate_size=96,
        num_hidden_layers=2,
        num_attention_heads=4,
        num_key_value_heads=2,
        head_dim=32,
        rope_theta=10000.0,
        max_position_embeddings=2048,
        attention_bias=False,
        qk_norm=True,
        num_local_experts=4,
        num_experts_per_tok=2,
        norm_topk_prob=False,
        eos_token_id=2,
        bos_token_id=1,
    ),
    # The two below have widths the W4 expert kernels take (multiples of the
    # 128 group, also per rank at TP=2: 8 heads x 32 and a shared width of
    # 256 leave 128 each).
    "tiny-qwen2moe-w4": ModelConfig(  # Qwen2-MoE naming + shared expert
        architecture="Qwen2MoeForCausalLM",
        vocab_size=512,
        hidden_size=128,
        intermediate_size=256,
        moe_intermediate_size=128,
        shared_expert_intermediate_size=256,
        num_hidden_layers=2,
        num_attention_heads=8,
        num_key_value_heads=2,
        head_dim=32,
        rope_theta=10000.0,
        max_position_embeddings=2048,
        attention_bias=True,
        num_local_experts=4,
        num_experts_per_tok=2,
        norm_topk_prob=False,
        eos_token_id=2,
        bos_token_id=1,
    ),
    "tiny-qwen3moe-w4": ModelConfig(  # Qwen3-MoE naming
        architecture="Qwen3MoeForCausalLM",
        vocab_size=512,
        hidden_size=128,
        intermediate_size=256,
        moe_intermediate_size=128,
        num_hidden_layers=2,
        num_attention_heads=8,
        num_key_value_heads=2,
        head_dim=32,
        rope_theta=10000.0,
        max_position_embeddings=2048,
        attention_bias=False,
        qk_norm=True,
        num_local_experts=4,
        num_experts_per_tok=2,
        norm_topk_prob=True,
        eos_token_id=2,
        bos_token_id=1,
    ),
    "qwen3-30b-a3b": ModelConfig(  # Qwen3-30B-A3B MoE shape
        architecture="Qwen3MoeForCausalLM",
        vocab_size=151936,
        hidden_size=2048,
        intermediate_size=6144,
        moe_intermediate_size=768,
        num_hidden_layers=48,
        num_attention_heads=32,
        num_key_value_heads=4,
        head_dim=128,
        rope_theta=1000000.0,
        attention_bias=False,
        qk_norm=True,
        num_local_experts=128,
        num_experts_per_tok=8,
        norm_topk_prob=True,
    ),
    "tiny-moe-gpu": ModelConfig(  # GPU-test-sized sparse MoE (head_dim 128)
        architecture="MixtralForCausalLM",
        vocab_size=2048,
        hidden_size=512,
        intermediate_size=256,
        num_hidden_layers=2,
        num_attention_heads=4,
        num_key_value_heads=2,
        head_dim=128,
        rope_theta=10000.0,
        max_position_embeddings=4096,
        attention_bias=False,
        num_local_experts=4,
        num_experts_per_tok=2,
        eos_token_id=2,
        bos_token_id=1,
    ),
    "smollm3-3b": ModelConfig(
        architecture="SmolLM3ForCausalLM",
        vocab_size=128256,
        hidden_size=2048,
        intermediate_size=11008,
        num_hidden_layers=36,
        num_attention_heads=16,
        num_key_value_heads=4,
        head_dim=128,
        rms_norm_eps=1e-6,
        rope_theta=5000000.0,
        max_position_embeddings=65536,
        tie_word_embeddings=True,
        attention_bias=False,
        no_rope_layers=[int((i + 1) % 4 != 0) for i in range(36)],
        eos_token_id=128012,
        bos_token_id=128000,
    ),
    "tiny-smollm3": ModelConfig(  # CPU-test-sized, NoPE on odd layers
        architecture="SmolLM3ForCausalLM",
        vocab_size=512,
        hidden_size=128,
        intermediate_size=256,
        num_hidden_layers=2,
        num_attention_heads=4,
        num_key_value_heads=2,
        head_dim=32,
        rope_theta=10000.0,
        max_position_embeddings=2048,
        tie_word_embeddings=True,
        attention_bias=False,
        no_rope_layers=[1, 0],
        eos_token_id=2,
        bos_token_id=1,
    ),
    "tiny": ModelConfig(  # CPU-test-sized
        architecture="Qwen2ForCausalLM",
        vocab_size=512,
        hidden_size=128,
        intermediate_size=256,
        num_hidden_layers=2,
        num_attention_heads=4,
        num_key_value_heads=2,
        head_dim=32,
        rope_theta=10000.0,
        max_position_embeddings=2048,
        eos_token_id=2,
        bos_token_id=1,
    ),
    "tiny-gpu": ModelConfig(  # GPU-test-sized (head_dim 128 kernels)
        architecture="Qwen2ForCausalLM",
        vocab_size=2048,
        hidden_size=512,
        intermediate_size=1024,
        num_hidden_layers=2,
        num_attention_heads=4,
        num_key_value_heads=2,
        head_dim=128,
        rope_theta=10000.0,
        max_position_embeddings=4096,
        eos_token_id=2,
        bos_token_id=1,
    ),
}


@dataclass
class EngineConfig:
    model_path: str | None = None  # dir with config.json + *.safetensors
    preset: str | None = None  # or a PRESET_CONFIGS key (random-init)
    served_model_name: str = "model"
    tensor_parallel_size: int = 1
    block_size: int = 16  # KV page size (tokens) — fixed by the decode kernel
    gpu_memory_utilization: float = 0.90
    max_num_seqs: int = 256
    max_num_batched_tokens: int = 8192
    max_model_len: int = 8192
    kv_cache_blocks: int | None = None  # override (else sized from free HBM)
    enforce_eager: bool = False  # disable hipGraph decode capture
    enable_prefix_caching: bool = True  # content-addressed KV block reuse
    # mixed batching: prefill chunks share a step with in-flight decodes so
    # long prompts never stall token streams (vLLM-v1-style scheduling)
    enable_mixed_batching: bool = True
    # None | "fp8": W8A8 OCP-e4m3 for qkv/gate_up/down/lm_head GEMMs
    # (dynamic per-token activation scales; o_proj and KV stay bf16)
    # "int4": W4A16, round-to-nearest at load, group size 128, for the dense
    # qkv/o/gate_up/down GEMMs (lm_head, embeddings and router gates stay
    # bf16; MoE experts stay bf16 unless quantize_experts is set)
    # "awq": a 4-bit AWQ checkpoint, dense or MoE (auto-detected from its
    # config.json; giving it for any other checkpoint is an error)
    # "mxfp4": OCP MXFP4 weights (e2m1, one e8m0 scale per 32 along K), W4A16
    # for the dense qkv/o/gate_up/down GEMMs: a Quark MXFP4 checkpoint
    # (auto-detected, excludes every other mode) or, on a bf16 checkpoint,
    # the OCP conversion at load (the counterpart of "int4"; MoE experts
    # stay bf16)
    quantization: str | None = None
    # with quantization="int4" on an MoE model: also quantize the routed
    # experts and the shared expert at load (routed grouped W4 GEMM)
    quantize_experts: bool = False
    # "auto" (bf16) | "fp8": e4m3 KV pages (halves the decode KV stream;
    # scale 1.0, opt-in like vLLM's --kv-cache-dtype fp8)
    kv_cache_dtype: str = "auto"
    # None | "ngram": prompt-lookup speculative decoding (draft tokens from
    # n-gram matches in the sequence's own history, verified in one extend
    # forward; greedy-exact, applied only to temperature-0 requests without
    # penalties/logprobs — same surface as vLLM's ngram speculator)
    speculative: str | None = None
    num_speculative_tokens: int = 4  # max draft length per step
    # speculative="draft": the draft model ("preset:<name>" or a checkpoint
    # path; must share the target's tokenizer/vocab)
    draft_model: str | None = None
    device: str = "cuda"
    # "float32" runs the CPU reference path in fp32 (device="cpu" only: the
    # kernels are bf16); anything else is bf16
    dtype: str = "bfloat16"
    seed: int = 0
    # multi-LoRA serving (off by default): PEFT adapters of the base model
    # loaded at start-up into max_loras fixed GPU slots, zero-padded to
    # max_lora_rank (16, 32 or 64), selected per request by model name.
    # lora_modules maps adapter name -> PEFT directory.
    enable_lora: bool = False
    max_loras: int = 4
    max_lora_rank: int = 16
    lora_modules: dict[str, str] | None = None
    # structured outputs (arks_amd.structured): cap on a grammar's DFA
    # states, and rows of the device-resident mask pool ([slots, V/32])
    structured_max_states: int = 20000
    structured_mask_slots: int = 512
    # embedding requests: default pooling ("auto" | "last" | "mean" | "cls")
    # and L2 normalisation ("auto" | "true" | "false"); auto reads the
    # checkpoint's sentence-transformers settings, else last + normalise
    pooling: str = "auto"
    embedding_normalize: str = "auto"

    def __post_init__(self):
        if self.quantization not in (None, "fp8", "int4", "awq", "mxfp4"):
            raise ValueError(
                f"unknown quantization {self.quantization!r}: expected "
                "None, 'fp8', 'int4' or 'awq', or 'mxfp4'"
            )
        if self.quantize_experts and self.quantization != "int4":
            raise ValueError(
                "quantize_experts needs quantization='int4', got "
                f"quantization={self.quantization!r} (an AWQ checkpoint's "
                "experts are 4-bit already)"
            )
        if not self.enable_lora:
            if self.lora_modules:
                raise ValueError("lora_modules given without enable_lora")
            return
        if self.quantization == "fp8":
            raise ValueError(
                "enable_lora with quantization='fp8' is not supported: the "
                "fp8 layers receive pre-quantised activations"
            )
        if self.speculative == "draft":
            raise ValueError(
                "enable_lora with speculative='draft' is not supported "
                "(n-gram speculation is)"
            )
        if self.max_lora_rank not in (16, 32, 64):
            raise ValueError(
                f"max_lora_rank must be 16, 32 or 64, got {self.max_lora_rank}"
            )
        if self.max_loras < 1:
            raise ValueError(f"max_loras must be >= 1, got {self.max_loras}")
        mods = self.lora_modules or {}
        if self.served_model_name in mods:
            raise ValueError(
                f"LoRA adapter name {self.served_model_name!r} clashes with "
                "served_model_name"
            )
        if len(mods) > self.max_loras:
            raise ValueError(
                f"{len(mods)} lora_modules exceed max_loras={self.max_loras}"
            )

    def resolve_quantization(self, model_cfg: ModelConfig) -> str | None:
        """The mode the engine runs: an AWQ checkpoint selects "awq" on its
        own and excludes every other mode; "awq" needs such a checkpoint. A
        block-scaled FP8 checkpoint selects "fp8_block" on its own; "fp8"
        on it is accepted and means the same, on any other checkpoint it is
        the W8A8 path. An MXFP4 checkpoint selects "mxfp4" on its own and
        excludes every other mode; on a bf16 checkpoint "mxfp4" quantizes
        the dense layers at load."""
        if self.quantize_experts and model_cfg.num_local_experts == 0:
            raise ValueError(
                "quantize_experts needs an MoE model, "
                f"{model_cfg.architecture} has no experts"
            )
        if model_cfg.quant_method == "fp8_block":
            # the checkpoint's own format: "fp8" on it means exactly that,
            # not the load-time W8A8 re-quantization of a bf16 checkpoint
            if self.quantization not in (None, "fp8"):
                raise ValueError(
                    f"quantization={self.quantization!r} cannot be applied "
                    "to a block-scaled FP8 checkpoint: its weights are "
                    "already e4m3 (leave quantization unset or give 'fp8')"
                )
            return "fp8_block"
        if model_cfg.quant_method == "mxfp4":
            if self.quantization not in (None, "mxfp4"):
                raise ValueError(
                    f"quantization={self.quantization!r} cannot be applied "
                    "to an MXFP4 checkpoint: its weights are already 4-bit "
                    "(leave quantization unset or give 'mxfp4')"
                )
            return "mxfp4"
        if model_cfg.quant_method == "awq":
            if self.quantization not in (None, "awq"):
                raise ValueError(
                    f"quantization={self.quantization!r} cannot be applied "
                    "to an AWQ checkpoint: its weights are already 4-bit "
                    "(leave quantization unset or give 'awq')"
                )
            return "awq"
        if self.quantization == "awq":
            raise ValueError(
                "quantization='awq' needs an AWQ checkpoint, but the model's "
                "config.json has no AWQ quantization_config (use 'int4' to "
                "quantize a bf16 checkpoint at load)"
            )
        return self.quantization

    def model_config(self) -> ModelConfig:
        if self.model_path:
            return ModelConfig.from_pretrained(self.model_path)
        if self.preset:
            return PRESET_CONFIGS[self.preset]
        raise ValueError("EngineConfig needs model_path or preset")
