"""Qwen2 / Llama decoder family for the arks_amd engine.

One implementation covers both architectures (Qwen2 = Llama + QKV bias +
different rope_theta/vocab). HF-config-driven (arks_amd.config.ModelConfig);
weight names follow the HF checkpoint layout so safetensors load directly.

Compute path: F.linear GEMMs (hipBLASLt) + arks_amd.ops HIP kernels for
RMSNorm / RoPE / paged attention / SwiGLU; TP via column/row-parallel shards
with one RCCL all-reduce per attention and per MLP block.
"""

from __future__ import annotations

import math

import torch
import torch.nn as nn

from .. import ops
from ..config import ModelConfig
from ..engine.forward_batch import ForwardBatch
from ..parallel.comm import get_tp_rank, get_tp_world_size
from ..parallel.layers import (
    MergedColumnParallelLinear,
    ParallelLMHead,
    QKVParallelLinear,
    RowParallelLinear,
)


# tensor suffixes of an AutoAWQ "GEMM" projection
_AWQ_KINDS = ("qweight", "qzeros", "scales")


class RMSNorm(nn.Module):
    fp8_out = False  # emit (fp8, scales) for a W8A8 consumer GEMM

    def __init__(self, hidden: int, eps: float, dtype=torch.bfloat16):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(hidden, dtype=dtype), requires_grad=False)
        self.eps = eps

    def forward(self, x, residual=None):
        if isinstance(x, ops.SplitKPending) and (self.fp8_out
                                                 or residual is None):
            x = x.materialize()  # no fused consumer for these forms
        if self.fp8_out:
            if residual is None:
                return ops.rmsnorm_fp8(x, self.weight, self.eps)
            q, s, res = ops.fused_add_rmsnorm_fp8(x, residual, self.weight, self.eps)
            return (q, s), res
        if residual is None:
            return ops.rmsnorm(x, self.weight, self.eps)
        return ops.fused_add_rmsnorm(x, residual, self.weight, self.eps)


class Attention(nn.Module):
    def __init__(self, cfg: ModelConfig, dtype=torch.bfloat16,
                 layer_idx: int = 0):
        super().__init__()
        tp = get_tp_world_size()
        self.head_dim = cfg.head_dim
        self.nq_local = cfg.num_attention_heads // tp
        self.nkv_local = cfg.num_key_value_heads // tp
        self.scale = 1.0 / math.sqrt(cfg.head_dim)
        # per-layer sliding window (HF Qwen2 max_window_layers/layer_types
        # semantics; Mistral = every layer; 0 = full attention). Masking
        # happens inside the kernels.
        self.window = cfg.layer_window(layer_idx)
        # SmolLM3 NoPE layers attend without positional encoding: k/v are
        # cached unrotated (HF modeling_smollm3.py:200-226 semantics)
        self.use_rope = cfg.layer_uses_rope(layer_idx)
        self.qkv_proj = QKVParallelLinear(
            cfg.hidden_size, cfg.head_dim, cfg.num_attention_heads,
            cfg.num_key_value_heads, bias=cfg.attention_bias, dtype=dtype,
        )
        self.o_proj = RowParallelLinear(
            cfg.num_attention_heads * cfg.head_dim, cfg.hidden_size, bias=False,
            dtype=dtype,
        )
        # Qwen3: per-head RMSNorm on q and k before RoPE
        self.q_norm = (
            RMSNorm(cfg.head_dim, cfg.rms_norm_eps, dtype) if cfg.qk_norm else None
        )
        self.k_norm = (
            RMSNorm(cfg.head_dim, cfg.rms_norm_eps, dtype) if cfg.qk_norm else None
        )

    def forward(self, x, batch: ForwardBatch, kv_cache, defer: bool = False):
        """defer=True: the caller's next op is a fused add-RMSNorm that can
        take o_proj's result as an ops.SplitKPending."""
        T = (x[0] if isinstance(x, tuple) else x).shape[0]
        # Decode with plain RoPE: let the RoPE+cache kernel reduce the qkv
        # split-K partials itself (decode attention reads k/v from the cache,
        # so they are never materialised).
        qkv = self.qkv_proj(
            x, batch.lora_tiles,
            defer=(not batch.is_prefill and self.use_rope
                   and self.q_norm is None),
        )
        if isinstance(qkv, ops.SplitKPending):
            k_cache, v_cache = kv_cache
            q = ops.rope_and_cache_splitk(
                batch.positions, qkv, k_cache, v_cache, batch.slot_mapping,
                self._cos_sin, self.head_dim, self.nq_local,
            )
            out = ops.attention_decode_paged(
                q.unflatten(-1, (self.nq_local, self.head_dim)), k_cache,
                v_cache, batch.block_tables, batch.seq_lens, self.scale,
                window=self.window,
            )
            return self.o_proj(out.view(T, -1), batch.lora_tiles, defer=defer)
        # Strided views into the fused QKV buffer — RoPE/cache/attention
        # kernels take row strides, so no .contiguous() copies on the hot path.
        q, k, v = self.qkv_proj.split_qkv(qkv)
        if self.q_norm is not None:
            hd = self.head_dim
            q = self.q_norm(
                q.contiguous().view(-1, hd)).view(T, self.nq_local * hd)
            k = self.k_norm(
                k.contiguous().view(-1, hd)).view(T, self.nkv_local * hd)
            # reshape_and_cache wants one shared kv stride. clone, not
            # contiguous(): a one-row view counts as contiguous and would
            # keep the fused buffer's row stride (batch-1 decode)
            v = v.clone(memory_format=torch.contiguous_format)
        k_cache, v_cache = kv_cache
        if self.use_rope:
            q, k = ops.rope_and_cache(
                batch.positions, q, k, v, k_cache, v_cache,
                batch.slot_mapping, self._cos_sin, self.head_dim,
            )
        else:
            # NoPE layer: cache k/v as-is, q unrotated
            ops.reshape_and_cache(
                k.unflatten(-1, (self.nkv_local, self.head_dim)),
                v.unflatten(-1, (self.nkv_local, self.head_dim)),
                k_cache, v_cache, batch.slot_mapping,
            )
        k = k.unflatten(-1, (self.nkv_local, self.head_dim))
        v = v.unflatten(-1, (self.nkv_local, self.head_dim))
        q = q.unflatten(-1, (self.nq_local, self.head_dim))
        if batch.is_prefill:
            if batch.block_tables is not None:
                # Prefix-cache hit in the batch: new tokens attend over the
                # full paged KV (cached prefix + the rows just written above).
                out = ops.attention_extend_paged(
                    q, k_cache, v_cache, batch.block_tables, batch.seq_lens,
                    batch.cu_seqlens, batch.seq_lens_list, self.scale,
                    window=self.window, tiles=batch.ext_tiles,
                )
            else:
                out = ops.attention_prefill_varlen(
                    q, k, v, batch.cu_seqlens, batch.seq_lens_list, self.scale,
                    window=self.window,
                )
        else:
            out = ops.attention_decode_paged(
                q, k_cache, v_cache, batch.block_tables, batch.seq_lens,
                self.scale, window=self.window,
            )
        return self.o_proj(out.view(T, -1), batch.lora_tiles, defer=defer)


class MLP(nn.Module):
    def __init__(self, cfg: ModelConfig, dtype=torch.bfloat16):
        super().__init__()
        self.gate_up_proj = MergedColumnParallelLinear(
            cfg.hidden_size, cfg.intermediate_size, bias=False, dtype=dtype
        )
        self.down_proj = RowParallelLinear(
            cfg.intermediate_size, cfg.hidden_size, bias=False, dtype=dtype
        )

    fp8 = False

    def forward(self, x, batch: ForwardBatch | None = None,
                defer: bool = False):
        """defer=True: the caller's next op is a fused add-RMSNorm that can
        take down_proj's result as an ops.SplitKPending."""
        tiles = batch.lora_tiles if batch is not None else None
        gate_up = self.gate_up_proj(x, tiles)
        if self.fp8:
            return self.down_proj(ops.silu_mul_fp8(gate_up))
        return self.down_proj(ops.silu_mul(gate_up), tiles, defer=defer)


_ARANGE_CACHE: dict[tuple[int, int, str], torch.Tensor] = {}


def _arange_interleave(T: int, k: int, device) -> torch.Tensor:
    """Cached [0,0,..,1,1,..] token-index vector — identical for every MoE
    layer of a forward, so build it once per (T, k) instead of 48 times."""
    key = (T, k, str(device))
    t = _ARANGE_CACHE.get(key)
    if t is None:
        if len(_ARANGE_CACHE) > 256:
            _ARANGE_CACHE.clear()
        t = torch.arange(T, device=device).repeat_interleave(k)
        _ARANGE_CACHE[key] = t
    return t


class MoEMLP(nn.Module):
    """Mixtral-style sparse MoE block, expert-parallel over the TP group:
    each rank owns num_local_experts/tp whole experts (an expert's FFN is
    never split), computes its experts' contributions for the tokens routed
    to them, and one all-reduce sums the partial outputs — the same single
    collective per block as the dense RowParallel MLP. The router (gate) is
    replicated so every rank routes identically."""

    fp8 = False  # MoE experts stay bf16 (v1)

    def __init__(self, cfg: ModelConfig, dtype=torch.bfloat16):
        super().__init__()
        tp = get_tp_world_size()
        E = cfg.num_local_experts
        assert E % tp == 0, (E, tp)
        self.num_experts = E
        self.top_k = cfg.num_experts_per_tok
        self.local_experts = E // tp
        self.expert_base = get_tp_rank() * self.local_experts
        self.hidden = cfg.hidden_size
        self.inter = cfg.moe_intermediate_size or cfg.intermediate_size
        self.norm_topk = cfg.norm_topk_prob
        self.gate = nn.Parameter(
            torch.empty(E, cfg.hidden_size, dtype=dtype), requires_grad=False
        )
        # fused [gate|up] and down per local expert, stored PRE-TRANSPOSED
        # ([in, out] per expert) so every MoE GEMM is an NN strided bmm /
        # mm with contiguous operands: strided bmm with a transposed-VIEW B
        # memory-faults on this ROCm stack at prefill shapes
        # (scripts/probe_bmm_fault.py — all tb=True variants die, contiguous
        # B passes), and NN needs no per-call transpose copies.
        self.w13 = nn.Parameter(
            torch.empty(self.local_experts, self.hidden, 2 * self.inter,
                        dtype=dtype), requires_grad=False,
        )
        self.w2 = nn.Parameter(
            torch.empty(self.local_experts, self.inter, self.hidden,
                        dtype=dtype), requires_grad=False,
        )
        # Qwen2-MoE shared expert (dense, TP-sharded like a normal MLP) with
        # a sigmoid scalar gate
        self.shared = None
        self.shared_gate = None
        if cfg.shared_expert_intermediate_size:
            import dataclasses

            dense_cfg = dataclasses.replace(
                cfg, intermediate_size=cfg.shared_expert_intermediate_size
            )
            self.shared = MLP(dense_cfg, dtype)
            self.shared_gate = nn.Parameter(
                torch.zeros(1, cfg.hidden_size, dtype=dtype),
                requires_grad=False,
            )

    # Below this many tokens the dense path wins: every expert's weights
    # are streamed from HBM regardless (tokens scatter over all experts),
    # so decode is weight-bandwidth-bound and the extra MFMA work of
    # computing all tokens per expert stays at or under the HBM floor up
    # to ~256 tokens (E*T*3*I*H*2 flops vs E*3*I*H*2 bytes: the crossover
    # at ~1.5 PF effective and ~6 TB/s is T ~ 250). Data-independent
    # shapes make every decode batch size hipGraph-capturable.
    DENSE_TOKENS = 256

    # ---- W4 experts (int4 + quantize_experts, AWQ checkpoints) ----
    # Stacked packed buffers per local expert, ops.ref.w4_pack's format with
    # a leading expert dimension: w13 is [gate | up] along N (N = 2I, K = H),
    # w2 has N = H, K = I. The bf16 w13 / w2 parameters are dropped. On CPU
    # bf16-rounded dequantized [E, in, out] buffers named w13 / w2 stand in
    # for them and the bf16 forward runs unchanged (the weight_qdq
    # convention of the dense layers).
    w4 = False

    def w4_check_shapes(self, name: str) -> None:
        """What w4_moe_gemm_kernel needs of both expert GEMMs: K a multiple
        of the 128 group, N a multiple of the 64-row tile."""
        H, I = self.hidden, self.inter
        if H % 128 or I % 128 or (2 * I) % 64 or H % 64:
            raise ValueError(
                f"{name}: MoE expert width {I} is not supported: W4 experts "
                f"need hidden and expert widths that are multiples of the "
                f"group size 128, got hidden={H}, expert width={I}"
            )

    def w4_packed(self, which: str):
        return (getattr(self, f"{which}_qweight"),
                getattr(self, f"{which}_scales"),
                getattr(self, f"{which}_zeros"))

    def init_w4(self, name: str = "moe") -> None:
        """Switch to (empty) W4 storage; the bf16 parameters are dropped, so
        a block switched before its weights stream in never holds them."""
        from ..ops import ref

        self.w4_check_shapes(name)
        dev = self.w13.device
        E, H, I = self.local_experts, self.hidden, self.inter
        del self._parameters["w13"]
        del self._parameters["w2"]
        for which, (N, K) in (("w13", (2 * I, H)), ("w2", (H, I))):
            G = K // ref.W4_GROUP
            self.register_buffer(
                f"{which}_qweight",
                torch.zeros(E, N, K // 8, dtype=torch.int32, device=dev),
                persistent=False)
            self.register_buffer(
                f"{which}_scales",
                torch.zeros(E, G, N, dtype=torch.float16, device=dev),
                persistent=False)
            self.register_buffer(
                f"{which}_zeros",
                torch.zeros(E, G, N, dtype=torch.uint8, device=dev),
                persistent=False)
        self.w4 = True

    def finalize_w4(self) -> None:
        """After the packed buffers are filled: on CPU keep the bf16
        dequantized experts that emulate the GPU numerics."""
        from ..ops import ref

        if self.w13_qweight.is_cuda:
            return
        for which in ("w13", "w2"):
            qw, sc, zr = self.w4_packed(which)
            deq = torch.stack([
                ref.w4_dequant(*ref.w4_unpack((qw[e], sc[e], zr[e])))
                .to(torch.bfloat16).t() for e in range(self.local_experts)
            ]).contiguous()
            if which in self._buffers:
                del self._buffers[which]
            self.register_buffer(which, deq, persistent=False)

    def quantize_w4(self, name: str = "moe") -> None:
        """Round-to-nearest W4 of loaded bf16 experts, one expert at a time
        (ops.ref.w4_quantize), so the transient memory is one expert's."""
        from ..ops import ref

        self.w4_check_shapes(name)
        bf16 = {"w13": self.w13.data, "w2": self.w2.data}
        self.init_w4(name)
        for which, w in bf16.items():
            qw, sc, zr = self.w4_packed(which)
            for e in range(self.local_experts):
                # stored [in, out]; the quantizer takes [N, K] = [out, in]
                packed = ref.w4_pack(*ref.w4_quantize(w[e].t()))
                qw[e].copy_(packed[0])
                sc[e].copy_(packed[1])
                zr[e].copy_(packed[2])
        del bf16
        self.finalize_w4()

    def load_awq_expert(self, name: str, le: int, proj: str, kind: str,
                        t: torch.Tensor) -> None:
        """One AWQ tensor (kind: qweight / qzeros / scales) of local expert
        le's gate / up / down projection into the stacked buffers: gate
        fills rows [0, I) of w13, up rows [I, 2I). The packed format is
        row-major over N, so each tensor lands on its own."""
        from ..ops import ref

        if not self.w4:
            raise ValueError(
                f"{name}: AWQ tensor in the checkpoint but the model was not "
                "prepared for AWQ (config.json lacks quantization_config?)"
            )
        H, I = self.hidden, self.inter
        which, r0, N, K = {"gate": ("w13", 0, I, H), "up": ("w13", I, I, H),
                           "down": ("w2", 0, H, I)}[proj]
        G = K // ref.W4_GROUP
        want = {"qweight": (K, N // 8), "qzeros": (G, N // 8),
                "scales": (G, N)}[kind]
        if tuple(t.shape) != want:
            raise ValueError(
                f"{name}: shape {tuple(t.shape)}, expected {want} for a "
                f"{N}x{K} projection at group size {ref.W4_GROUP}"
            )
        qw, sc, zr = self.w4_packed(which)
        t = t.cpu()
        if kind == "scales":    # on disk [K/128, N]: our layout already
            sc[le, :, r0:r0 + N].copy_(t.to(torch.float16))
        elif kind == "qzeros":
            zr[le, :, r0:r0 + N].copy_(ref._unpack_nibbles(t))
        else:
            rows = ref._unpack_nibbles(t).t().contiguous()  # [N, K]
            qw[le, r0:r0 + N].copy_(ref._pack_nibbles(rows))

    # ---- W8 experts (block-scaled FP8 checkpoints, quantize_w8) ----
    # The checkpoint's e4m3 bytes stacked per local expert, ops/ref.py's W8
    # format with a leading expert dimension: w13_w8 [E, 2I, H] is
    # [gate | up] along N with scales [E, H/128, 2I]; w2_w8 [E, H, I] with
    # scales [E, I/128, H]. The bf16 w13 / w2 parameters are dropped. On CPU
    # the W4 convention holds: bf16 [E, in, out] buffers named w13 / w2
    # (dequantized in f32, rounded once) stand in and the bf16 forward runs
    # on them; on GPU a W8 block has no bf16 copy of its experts.
    w8 = False

    _W8_PROJS = {"gate": ("gate_proj", "w1"), "up": ("up_proj", "w3"),
                 "down": ("down_proj", "w2")}

    def w8_supported(self) -> bool:
        """What w8_moe_gemm_kernel needs of both expert GEMMs: K a multiple
        of the 128 scale block (N = 2I and H are then multiples of 64)."""
        return self.hidden % 128 == 0 and self.inter % 128 == 0

    def w8_check_shapes(self, name: str) -> None:
        if not self.w8_supported():
            raise ValueError(
                f"{name}: MoE expert width {self.inter} is not supported: W8 "
                f"experts need hidden and expert widths that are multiples "
                f"of the scale block 128, got hidden={self.hidden}, expert "
                f"width={self.inter}"
            )

    def w8_weight(self, which: str):
        return (getattr(self, f"{which}_w8"),
                getattr(self, f"{which}_w8_scales"))

    def init_w8(self, name: str = "moe") -> None:
        """Switch to (empty) W8 storage; the bf16 parameters are dropped, so
        a block switched before its weights stream in never holds them."""
        from ..ops import ref

        self.w8_check_shapes(name)
        dev = self.w13.device
        E, H, I = self.local_experts, self.hidden, self.inter
        del self._parameters["w13"]
        del self._parameters["w2"]
        for which, (N, K) in (("w13", (2 * I, H)), ("w2", (H, I))):
            self.register_buffer(
                f"{which}_w8",
                torch.zeros(E, N, K, dtype=torch.float8_e4m3fn, device=dev),
                persistent=False)
            self.register_buffer(
                f"{which}_w8_scales",
                torch.zeros(E, K // ref.W8_BLOCK, N, dtype=torch.float32,
                            device=dev),
                persistent=False)
        self.w8 = True
        self._w8_got = set()    # (local expert, projection, kind) arrived
        self._w8_names = {}     # projection -> (checkpoint prefix, leaf)

    def load_fp8_expert(self, name: str, le: int, proj: str, kind: str,
                        t: torch.Tensor) -> None:
        """One FP8 tensor (kind: weight / weight_scale_inv) of local expert
        le's gate / up / down projection into the stacked buffers: gate
        fills rows [0, I) of w13, up rows [I, 2I). The weight is stored as it
        is; the block scales are expanded to one row per output channel, cut
        to N and transposed. Each tensor lands on its own."""
        from ..ops import ref

        if not self.w8:
            raise ValueError(
                f"{name}: FP8 expert tensor in the checkpoint but the block "
                "was not prepared for FP8 (config.json lacks "
                "quantization_config, or the experts are on its skip list?)"
            )
        H, I, B = self.hidden, self.inter, ref.W8_BLOCK
        which, r0, N, K = {"gate": ("w13", 0, I, H), "up": ("w13", I, I, H),
                           "down": ("w2", 0, H, I)}[proj]
        w8, sc = self.w8_weight(which)
        if kind == "weight":
            if t.dtype != torch.float8_e4m3fn:
                raise ValueError(
                    f"{name}: plain {t.dtype} weight of an MoE expert, but "
                    "the block was prepared for FP8 (mixed-precision expert "
                    "checkpoints are not supported)")
            want = (N, K)
        elif kind == "weight_scale_inv":
            want = (-(-N // B), K // B)
        else:
            raise ValueError(f"{name}: unexpected tensor kind {kind!r} for "
                             "an FP8 expert")
        if tuple(t.shape) != want:
            raise ValueError(
                f"{name}: shape {tuple(t.shape)}, expected {want} for a "
                f"{N}x{K} projection at block size {B}"
            )
        if kind == "weight":
            # byte copy: no conversion may touch the checkpoint's codes
            w8[le, r0:r0 + N].view(torch.uint8).copy_(t.view(torch.uint8))
        else:
            rows = t.float().repeat_interleave(B, dim=0)[:N]     # [N, K/128]
            sc[le, :, r0:r0 + N].copy_(rows.t())
        self._w8_got.add((le, proj, kind))
        head, sep, _ = name.rpartition(".experts.")
        if sep and proj not in self._w8_names:
            self._w8_names[proj] = (head, name.split(".")[-2])

    def finalize_w8(self, name: str = "moe") -> None:
        """After loading: every (local expert, projection, kind) must have
        arrived. On CPU keep the bf16 dequantized experts that the bf16
        forward runs on."""
        from ..ops import ref

        got = getattr(self, "_w8_got", None)
        if got is not None:
            style = 0
            if self._w8_names:
                style = 1 if next(iter(self._w8_names.values()))[1] in (
                    "w1", "w2", "w3") else 0
            for le in range(self.local_experts):
                for proj, leaves in self._W8_PROJS.items():
                    for kind in ("weight", "weight_scale_inv"):
                        if (le, proj, kind) in got:
                            continue
                        head, leaf = self._w8_names.get(
                            proj, (f"{name}", leaves[style]))
                        raise ValueError(
                            f"{head}.experts.{self.expert_base + le}.{leaf}."
                            f"{kind}: missing from the checkpoint for the "
                            f"FP8 experts of {name}")
            self._w8_got = None
        if self.w13_w8.is_cuda:
            return
        for which in ("w13", "w2"):
            w8, sc = self.w8_weight(which)
            deq = torch.stack([
                ref.w8_dequant(w8[e], sc[e]).to(torch.bfloat16).t()
                for e in range(self.local_experts)
            ]).contiguous()
            if which in self._buffers:
                del self._buffers[which]
            self.register_buffer(which, deq, persistent=False)

    def quantize_w8(self, name: str = "moe") -> None:
        """Block-scaled W8 of loaded bf16 experts, one expert at a time
        (ops.ref.w8_quantize), so the transient memory is one expert's."""
        from ..ops import ref

        self.w8_check_shapes(name)
        bf16 = {"w13": self.w13.data, "w2": self.w2.data}
        self.init_w8(name)
        self._w8_got = None     # filled here, nothing streams in
        I = self.inter
        for which, w in bf16.items():
            w8, sc = self.w8_weight(which)
            for e in range(self.local_experts):
                # stored [in, out]; the quantizer takes [N, K] = [out, in].
                # gate and up are separate tensors in a checkpoint, each
                # with its own blocks along N.
                full = w[e].t()
                parts = ((0, full[:I]), (I, full[I:])) if which == "w13" \
                    else ((0, full),)
                for r0, part in parts:
                    q, blocks = ref.w8_quantize(part)
                    n = part.shape[0]
                    w8[e, r0:r0 + n].view(torch.uint8).copy_(
                        q.view(torch.uint8))
                    sc[e, :, r0:r0 + n].copy_(
                        ref.w8_expand_scales(blocks, n))
        del bf16
        self.finalize_w8(name)

    def _forward_routed(self, x, gemm, w13, w2):
        """GPU forward over quantized experts (gemm = ops.w4_moe_gemm on the
        packed W4 triples, ops.w8_moe_gemm on the W8 pairs), the same for
        every T: route once, then two routed grouped GEMMs that stream only
        the experts the batch selected. Up to DENSE_TOKENS the launch shapes depend on T alone (no
        host sync; the decode graphs capture it); above it one sync per layer
        fetches the longest expert list to size the grid."""
        from ..parallel.comm import tp_all_reduce

        T, k = x.shape[0], self.top_k
        router_logits = torch.nn.functional.linear(x, self.gate).float()
        weights, selected = ops.moe_topk(router_logits, k, self.norm_topk)
        counts, pairs = ops.moe_route(selected, self.expert_base,
                                      self.local_experts)
        max_rows = (T if T <= self.DENSE_TOKENS
                    else max(1, int(counts.max().item())))
        gu = gemm(x, w13, counts, pairs, k, max_rows)      # [T*k, 2I]
        h = ops.silu_mul(gu)                               # [T*k, I]
        # y row 0 is a zero row: the pairs of experts other ranks own are
        # never written, and the mix multiplies whatever it reads (0 * NaN
        # is NaN), so their slots read row 0 at weight 0.
        y = x.new_empty(T * k + 1, self.hidden)
        gemm(h, w2, counts, pairs, 1, max_rows, out=y[1:])
        rows = torch.arange(1, T * k + 1, dtype=torch.int32,
                            device=x.device).view(T, k)
        if self.local_experts != self.num_experts:
            y[0].zero_()
            le = selected - self.expert_base
            mine = (le >= 0) & (le < self.local_experts)
            rows = torch.where(mine, rows, torch.zeros_like(rows))
            weights = torch.where(mine, weights, torch.zeros_like(weights))
        out = tp_all_reduce(ops.moe_mix_rows(y, weights, rows))
        if self.shared is not None:
            gate = torch.sigmoid(
                torch.nn.functional.linear(x, self.shared_gate).float()
            ).to(x.dtype)
            out = out + gate * self.shared(x)
        return out

    def forward(self, x):
        from ..parallel.comm import tp_all_reduce

        if self.w4 and x.is_cuda:
            return self._forward_routed(x, ops.w4_moe_gemm,
                                        self.w4_packed("w13"),
                                        self.w4_packed("w2"))
        if self.w8 and x.is_cuda:
            return self._forward_routed(x, ops.w8_moe_gemm,
                                        self.w8_weight("w13"),
                                        self.w8_weight("w2"))
        T = x.shape[0]
        router_logits = torch.nn.functional.linear(x, self.gate).float()
        # fused softmax+topk+renorm routing kernel (ops.moe_topk) replaces
        # a 5-kernel torch chain per layer
        weights, selected = ops.moe_topk(router_logits, self.top_k,
                                         self.norm_topk)
        out = torch.zeros_like(x)
        if T <= self.DENSE_TOKENS:
            # Batched over experts: two strided-batch GEMMs (bmm) instead of
            # a per-expert loop — one launch pair regardless of E (Qwen3-MoE
            # has 128 experts), and every expert's weights stream once. The
            # weighted mix over experts is one gather kernel (ops.moe_mix).
            E = self.local_experts
            xb = x.unsqueeze(0).expand(E, T, self.hidden)
            gu = torch.bmm(xb, self.w13)  # [E, T, 2I]
            h = ops.silu_mul(gu.reshape(E * T, 2 * self.inter))
            y = torch.bmm(h.view(E, T, self.inter), self.w2)  # [E, T, H]
            out = ops.moe_mix(y, weights, selected, self.expert_base)
            out = tp_all_reduce(out)
            if self.shared is not None:
                gate = torch.sigmoid(
                    torch.nn.functional.linear(x, self.shared_gate).float()
                ).to(x.dtype)
                out = out + gate * self.shared(x)
            return out
        # Sparse path (prefill-sized T): sort token-expert pairs once so
        # each expert sees a contiguous segment (one host sync per layer
        # for the segment table), run the expert FFNs into ONE flat output
        # buffer — a capacity-clamped grouped bmm plus large-M overflow
        # GEMMs for heavily-routed experts — and combine with the
        # moe_mix_rows gather kernel. No index_add_ scatters anywhere:
        # torch's indexFuncLargeIndex was 36% of Qwen3-30B prefill GPU
        # time (profiles/r02_final.md).
        k = self.top_k
        flat_sel = selected.reshape(-1).long()
        flat_tok = _arange_interleave(T, k, x.device)
        order = torch.argsort(flat_sel, stable=True)
        tok_sorted = flat_tok[order]
        counts = torch.bincount(flat_sel, minlength=self.num_experts)
        offs = torch.cumsum(counts, 0)
        seg = torch.stack((counts, offs)).cpu()  # ONE host sync per layer
        counts_h = seg[0].tolist()
        offs_h = seg[1].tolist()
        El = self.local_experts
        base = self.expert_base
        local_counts_h = counts_h[base:base + El]
        cap = max(local_counts_h or [0])
        cap_lim = max(1, (512 * 1024 * 1024) // (El * 2 * self.inter * 2))
        # clamp the grouped capacity near 2x the mean load: under skewed
        # routing, padding the whole block to the heaviest expert wastes
        # multiples of the useful FLOPs, while spilled experts finish in
        # efficient large-M overflow GEMMs below
        mean2 = 2 * ((sum(local_counts_h) + El - 1) // El) if El else 0
        cap_eff = min(cap, cap_lim, max(128, mean2))
        ovf = [(le, c - cap_eff) for le, c in enumerate(local_counts_h)
               if c > cap_eff]
        n_of = sum(o for _, o in ovf)
        if cap_eff == 0:
            out = tp_all_reduce(out)  # no pairs routed to this rank
            if self.shared is not None:
                gate = torch.sigmoid(
                    torch.nn.functional.linear(x, self.shared_gate).float()
                ).to(x.dtype)
                out = out + gate * self.shared(x)
            return out

        y_all = x.new_empty(El * cap_eff + n_of, self.hidden)
        # grouped part: pad each local expert's segment to cap_eff rows
        # (two strided-batch GEMMs for the whole block; padding rows index
        # row 0 and are never gathered)
        local_counts = counts[base:base + El, None]        # [El, 1]
        local_starts = (offs[base:base + El] -
                        counts[base:base + El])[:, None]   # [El, 1]
        capped = torch.clamp(local_counts, max=cap_eff)
        ar = torch.arange(cap_eff, device=x.device)[None, :]  # [1, cap]
        flat = torch.where(ar < capped, local_starts + ar,
                           torch.zeros_like(ar)).reshape(-1)
        # single fused gather x[tok_sorted[flat]] — materializing an
        # intermediate x_g[T*k, H] costs a full extra round trip per layer
        xp = x[tok_sorted[flat]].view(El, cap_eff, self.hidden)
        gu = torch.bmm(xp, self.w13)
        h = ops.silu_mul(gu.reshape(El * cap_eff, 2 * self.inter))
        torch.bmm(h.view(El, cap_eff, self.inter), self.w2,
                  out=y_all[:El * cap_eff].view(El, cap_eff, self.hidden))
        # overflow part: experts past cap_eff finish with plain large-M
        # GEMMs appended to the same buffer
        p0 = El * cap_eff
        of_base_h = []
        acc = 0
        for le, o in ovf:
            of_base_h.append((le, acc))
            ge = base + le
            sl = slice(offs_h[ge] - counts_h[ge] + cap_eff, offs_h[ge])
            h2 = ops.silu_mul(x[tok_sorted[sl]] @ self.w13[le])
            torch.mm(h2, self.w2[le], out=y_all[p0 + acc:p0 + acc + o])
            acc += o

        # row map [T, k]: each pair's position in y_all
        inv = torch.empty_like(order)
        inv[order] = torch.arange(T * k, device=x.device)
        inv = inv.view(T, k)
        sel = selected.long().view(T, k)
        sel_local = sel - base
        mine = (sel_local >= 0) & (sel_local < El)
        seg_start = offs - counts  # [E] global segment starts
        local_idx = inv - seg_start[sel]
        in_cap = local_idx < cap_eff
        sl_safe = sel_local.clamp(0, El - 1)
        if ovf:
            of_base_t = torch.zeros(El, dtype=torch.long, device=x.device)
            of_base_t[torch.tensor([le for le, _ in of_base_h],
                                   device=x.device)] = torch.tensor(
                [a for _, a in of_base_h], device=x.device)
            rows_of = p0 + of_base_t[sl_safe] + (local_idx - cap_eff)
        else:
            rows_of = torch.zeros_like(local_idx)
        rows = torch.where(in_cap, sl_safe * cap_eff + local_idx, rows_of)
        rows = torch.where(mine, rows, torch.zeros_like(rows))
        w_masked = torch.where(mine, weights,
                               torch.zeros_like(weights))
        out = ops.moe_mix_rows(y_all, w_masked, rows.to(torch.int32))
        out = tp_all_reduce(out)
        if self.shared is not None:
            gate = torch.sigmoid(
                torch.nn.functional.linear(x, self.shared_gate).float()
            ).to(x.dtype)
            out = out + gate * self.shared(x)
        return out


class DecoderLayer(nn.Module):
    def __init__(self, cfg: ModelConfig, dtype=torch.bfloat16,
                 layer_idx: int = 0):
        super().__init__()
        self.input_layernorm = RMSNorm(cfg.hidden_size, cfg.rms_norm_eps, dtype)
        self.self_attn = Attention(cfg, dtype, layer_idx=layer_idx)
        self.post_attention_layernorm = RMSNorm(cfg.hidden_size, cfg.rms_norm_eps, dtype)
        self.mlp = (
            MoEMLP(cfg, dtype) if cfg.num_local_experts > 0 else MLP(cfg, dtype)
        )
        # MoE blocks take no adapters (attention-projection LoRA only)
        self._dense_mlp = isinstance(self.mlp, MLP)

    def forward(self, x, residual, batch: ForwardBatch, kv_cache):
        if residual is None:
            residual = x
            x = self.input_layernorm(x)
        else:
            x, residual = self.input_layernorm(x, residual)
        # o_proj and down_proj may come back as ops.SplitKPending: each is
        # consumed by the very next fused add-RMSNorm (post_attention here;
        # the next layer's input_layernorm or the model's final norm for
        # down_proj) before another skinny GEMM reuses the workspace.
        x = self.self_attn(x, batch, kv_cache, defer=True)
        x, residual = self.post_attention_layernorm(x, residual)
        x = (self.mlp(x, batch, defer=True) if self._dense_mlp
             else self.mlp(x))
        return x, residual


class LlamaFamilyForCausalLM(nn.Module):
    """Covers Qwen2ForCausalLM and LlamaForCausalLM."""

    def __init__(self, cfg: ModelConfig, dtype=torch.bfloat16):
        super().__init__()
        self.cfg = cfg
        self.dtype = dtype
        self.embed_tokens = nn.Embedding(
            cfg.vocab_size, cfg.hidden_size, dtype=dtype
        )
        self.embed_tokens.weight.requires_grad_(False)
        self.layers = nn.ModuleList(
            DecoderLayer(cfg, dtype, layer_idx=i)
            for i in range(cfg.num_hidden_layers)
        )
        self.norm = RMSNorm(cfg.hidden_size, cfg.rms_norm_eps, dtype)
        self.lm_head = ParallelLMHead(cfg.hidden_size, cfg.vocab_size, dtype)
        # False once a checkpoint turned out to carry no lm_head.weight and
        # no tied embeddings (an embedding model): pooling only
        self.has_lm_head = True
        self._lm_head_loaded = False
        cos_sin = self._build_cos_sin()
        self.register_buffer("rope_cos_sin", cos_sin, persistent=False)
        for layer in self.layers:
            layer.self_attn._cos_sin = cos_sin

    def quantize_fp8(self) -> None:
        """W8A8 fp8 for the weight-bandwidth-bound GEMMs (profiles/r01_p2:
        gate_up/down/lm_head dominate the decode step; o_proj is left bf16 —
        no gain at its size and its input is the attention output, which
        has no producing kernel to fuse a quant into)."""
        from ..parallel.layers import quantize_module_fp8

        for layer in self.layers:
            quantize_module_fp8(layer.self_attn.qkv_proj)
            layer.input_layernorm.fp8_out = True
            if isinstance(layer.mlp, MoEMLP):
                continue  # MoE experts stay bf16 (v1)
            quantize_module_fp8(layer.mlp.gate_up_proj)
            quantize_module_fp8(layer.mlp.down_proj)
            # producing kernels emit fp8 directly (fused activation quant)
            layer.post_attention_layernorm.fp8_out = True
            layer.mlp.fp8 = True
        quantize_module_fp8(self.lm_head)
        self.norm.fp8_out = True

    # the MoE blocks are W4 too (AWQ checkpoint, or int4 + quantize_experts)
    _w4_experts = False

    def _w4_targets(self, experts: bool = False):
        """(name, module) of the linear layers int4 / AWQ quantize: the
        dense qkv/o/gate_up/down projections and, with experts=True, the
        Qwen2-MoE shared expert (an ordinary MLP). lm_head, the embeddings
        and the router gates stay bf16 (as in AWQ checkpoints); the routed
        experts are not linear layers, see _moe_blocks."""
        for i, layer in enumerate(self.layers):
            yield f"layers.{i}.self_attn.qkv_proj", layer.self_attn.qkv_proj
            yield f"layers.{i}.self_attn.o_proj", layer.self_attn.o_proj
            mlp = layer.mlp
            if isinstance(mlp, MoEMLP):
                if not experts or mlp.shared is None:
                    continue
                mlp = mlp.shared
                pre = f"layers.{i}.mlp.shared_expert"
            else:
                pre = f"layers.{i}.mlp"
            yield f"{pre}.gate_up_proj", mlp.gate_up_proj
            yield f"{pre}.down_proj", mlp.down_proj

    def _moe_blocks(self):
        for i, layer in enumerate(self.layers):
            if isinstance(layer.mlp, MoEMLP):
                yield f"layers.{i}.mlp", layer.mlp

    def quantize_int4(self, quantize_experts: bool = False) -> None:
        """W4A16 round-to-nearest (group 128) over a loaded bf16 model; the
        activations stay bf16, so the norms and SwiGLU are unchanged.
        quantize_experts also quantizes the routed experts and the shared
        expert of an MoE model; a width the grouped kernel cannot take
        raises naming the layer."""
        from ..parallel.layers import quantize_module_w4

        if quantize_experts:
            if self.cfg.num_local_experts == 0:
                raise ValueError(
                    "quantize_experts needs an MoE model, "
                    f"{self.cfg.architecture} has no experts")
            for name, moe in self._moe_blocks():
                moe.w4_check_shapes(name)
            self._w4_experts = True
        for name, mod in self._w4_targets(quantize_experts):
            quantize_module_w4(mod, name)
        if quantize_experts:
            for name, moe in self._moe_blocks():
                moe.quantize_w4(name)

    def prepare_awq(self) -> None:
        """Switch the quantized layers to (empty) W4 storage BEFORE an AWQ
        checkpoint streams in, so their bf16 weights (the experts' above
        all) are never allocated on the device; finalize_w4() completes the
        switch after loading."""
        from ..parallel.layers import init_module_w4

        for name, moe in self._moe_blocks():
            moe.w4_check_shapes(name)
        self._w4_experts = self.cfg.num_local_experts > 0
        for name, mod in self._w4_targets(self._w4_experts):
            init_module_w4(mod, name)
        for name, moe in self._moe_blocks():
            moe.init_w4(name)

    def finalize_w4(self) -> None:
        from ..parallel.layers import finalize_module_w4

        for _, mod in self._w4_targets(self._w4_experts):
            finalize_module_w4(mod)
        if self._w4_experts:
            for _, moe in self._moe_blocks():
                moe.finalize_w4()

    # ---- block-scaled FP8 checkpoints (W8A16; format in ops/ref.py) ----
    # X.weight e4m3fn [N, K] + X.weight_scale_inv f32 [ceil(N/128),
    # ceil(K/128)] per quantized projection. The candidate layers are
    # _w4_targets(experts=True) plus the routed experts of every MoE block,
    # which keep their e4m3 bytes stacked for the grouped W8 kernel (MoEMLP
    # init_w8). A block whose widths that kernel cannot take is dequantized
    # to bf16 at load, as is a quantized lm_head.
    _W8_KINDS = ("weight", "weight_scale_inv")

    @staticmethod
    def _w8_hf_parts(name: str) -> list[str]:
        """HF module names behind one of our (possibly fused) layers."""
        pre, _, leaf = name.rpartition(".")
        group = {"qkv_proj": ("q_proj", "k_proj", "v_proj"),
                 "gate_up_proj": ("gate_proj", "up_proj")}.get(leaf, (leaf,))
        return [f"model.{pre}.{p}" for p in group]

    def _w8_skipped(self, hf_name: str) -> bool:
        """modules_to_not_convert semantics: an entry names a module when its
        dotted components occur in a row in the module's name."""
        comps = hf_name.split(".")
        for entry in self.cfg.quant_skip_modules:
            e = entry.split(".")
            if any(comps[i:i + len(e)] == e
                   for i in range(len(comps) - len(e) + 1)):
                return True
        return False

    def quantize_w8(self, experts: bool = False) -> None:
        """Block-scaled W8A16 of a loaded bf16 model in memory
        (quantize_module_w8 over the linear layers an FP8 checkpoint
        quantizes; with experts=True the routed experts of every MoE block
        too, otherwise they stay bf16). For tests and benchmarks: serving
        reads the format from a checkpoint, there is no --quantization
        value."""
        from ..parallel.layers import quantize_module_w8

        if experts:
            if self.cfg.num_local_experts == 0:
                raise ValueError(
                    "experts=True needs an MoE model, "
                    f"{self.cfg.architecture} has no experts")
            for name, moe in self._moe_blocks():
                moe.w8_check_shapes(name)
        for name, mod in self._w4_targets(experts=True):
            quantize_module_w8(mod, name)
        if experts:
            for name, moe in self._moe_blocks():
                moe.quantize_w8(name)

    def _w8_expert_hf_names(self, name: str, moe) -> list[str]:
        """HF module names of every routed expert projection of a block
        (all ranks' experts, so that every rank decides alike)."""
        if self.cfg.architecture.startswith("MixtralFor"):
            sub, leaves = "block_sparse_moe", ("w1", "w3", "w2")
        else:
            sub, leaves = "mlp", ("gate_proj", "up_proj", "down_proj")
        pre = name.rpartition(".")[0]
        return [f"model.{pre}.{sub}.experts.{e}.{p}"
                for e in range(moe.num_experts) for p in leaves]

    def prepare_fp8_checkpoint(self) -> None:
        """Switch the quantized layers to (empty) W8 storage BEFORE a
        block-scaled FP8 checkpoint streams in, so their bf16 weights are
        never allocated on the device; finalize_w8() completes the switch
        after loading. The parts of a fused projection must all be quantized
        or all be on the checkpoint's skip list, and so must the routed
        experts of an MoE block; a block whose widths the grouped kernel
        cannot take stays bf16 and is dequantized as its tensors arrive."""
        from ..parallel.layers import init_module_w8

        self._w8_pending = {}
        self._w8_experts_logged = False
        for name, mod in self._w4_targets(experts=True):
            skipped = [self._w8_skipped(p) for p in self._w8_hf_parts(name)]
            if all(skipped):
                continue
            if any(skipped):
                raise ValueError(
                    f"{name}: the checkpoint quantizes only some parts of "
                    "this fused projection "
                    f"({dict(zip(self._w8_hf_parts(name), skipped))}: True = "
                    "left in bf16); they must all be FP8 or all plain")
            init_module_w8(mod, name)
            mod._w8_got = set()
        for name, moe in self._moe_blocks():
            names = self._w8_expert_hf_names(name, moe)
            skipped = [self._w8_skipped(p) for p in names]
            if all(skipped):
                continue
            if any(skipped):
                plain = [p for p, s in zip(names, skipped) if s]
                raise ValueError(
                    f"{name}: the checkpoint quantizes only some parts of "
                    f"this block's routed experts ({len(plain)} of "
                    f"{len(names)} projections left in bf16, the first "
                    f"{plain[0]}); they must all be FP8 or all plain")
            if moe.w8_supported():
                moe.init_w8(name)

    def finalize_w8(self) -> None:
        from ..parallel.layers import finalize_module_w8

        for key, held in getattr(self, "_w8_pending", {}).items():
            for stem, kinds in held.items():
                if key[0] != "dequant":
                    raise ValueError(
                        f"{stem}.{key[1]}: the fused partners of this FP8 "
                        f"tensor ({key[0]}) are missing from the checkpoint")
                if "weight" not in kinds:
                    raise ValueError(
                        f"{stem}.weight_scale_inv: a scale without its "
                        "weight in the checkpoint")
                raise ValueError(
                    f"{stem}.weight: an FP8 weight without its "
                    "weight_scale_inv in the checkpoint")
        for name, mod in self._w4_targets(experts=True):
            if not getattr(mod, "w8", False):
                continue
            missing = set(self._W8_KINDS) - mod._w8_got
            if missing == {"weight"}:
                raise ValueError(
                    f"{name}: a scale without its weight in the checkpoint")
            if missing:
                raise ValueError(
                    f"{name}: the checkpoint has no {sorted(missing)} for "
                    "this FP8 layer")
            finalize_module_w8(mod)
        dropped = False
        for name, moe in self._moe_blocks():
            if not moe.w8:
                continue
            moe.finalize_w8(name)
            dropped = True
            if (not moe.w13_w8.is_cuda
                    and not getattr(self, "_w8_experts_logged", False)):
                import logging

                self._w8_experts_logged = True
                logging.getLogger(__name__).warning(
                    "FP8 routed experts are dequantized to bf16 on this "
                    "device (the grouped W8 kernel runs on the GPU only): "
                    "the model holds its experts at bf16 size")
        if dropped and torch.cuda.is_available() and any(
                moe.w13_w8.is_cuda for _, moe in self._moe_blocks()
                if moe.w8):
            # the dropped bf16 experts sit in the caching allocator; hand
            # them back so profile_num_blocks sees them as free
            torch.cuda.empty_cache()

    def _w8_target(self, stem: str):
        """(module, our name, fused HF partner stems or None, how) of the HF
        module `stem` (no "model." prefix) for an FP8 tensor; how is "col"
        (column-parallel, maybe fused), "row", "dequant" (dequantize to bf16
        and load as a plain weight), "expert" (a local routed expert of a W8
        MoE block: module is the block) or "skip" (another rank's expert).
        None for a module that never holds FP8."""
        if stem == "lm_head":
            return None, "lm_head", None, "dequant"
        parts = stem.split(".")
        if parts[0] != "layers" or len(parts) < 4:
            return None
        li = int(parts[1])
        if li >= len(self.layers):
            return None
        layer = self.layers[li]
        pre = f"layers.{li}"
        sub = ".".join(parts[2:])
        if parts[2] == "self_attn":
            attn = layer.self_attn
            if parts[3] in ("q_proj", "k_proj", "v_proj") and len(parts) == 4:
                return (attn.qkv_proj, f"{pre}.self_attn.qkv_proj",
                        [f"{pre}.self_attn.{p}"
                         for p in ("q_proj", "k_proj", "v_proj")], "col")
            if sub == "self_attn.o_proj":
                return attn.o_proj, f"{pre}.self_attn.o_proj", None, "row"
            return None
        if sub.startswith(("mlp.experts.", "block_sparse_moe.experts.")):
            if not isinstance(layer.mlp, MoEMLP) or len(parts) != 6:
                return None
            le = int(parts[4]) - layer.mlp.expert_base
            if not 0 <= le < layer.mlp.local_experts:
                return None, stem, None, "skip"
            if layer.mlp.w8 and parts[5] in (
                    "gate_proj", "up_proj", "down_proj", "w1", "w3", "w2"):
                return layer.mlp, stem, None, "expert"
            return None, stem, None, "dequant"
        if sub.startswith("mlp.shared_expert."):
            if not isinstance(layer.mlp, MoEMLP) or layer.mlp.shared is None:
                return None
            mlp, mpre = layer.mlp.shared, f"{pre}.mlp.shared_expert"
        elif parts[2] == "mlp" and isinstance(layer.mlp, MLP):
            mlp, mpre = layer.mlp, f"{pre}.mlp"
        else:
            return None
        leaf = parts[-1]
        if stem != f"{mpre}.{leaf}":
            return None
        if leaf in ("gate_proj", "up_proj"):
            return (mlp.gate_up_proj, f"{mpre}.gate_up_proj",
                    [f"{mpre}.gate_proj", f"{mpre}.up_proj"], "col")
        if leaf == "down_proj":
            return mlp.down_proj, f"{mpre}.down_proj", None, "row"
        return None

    def _route_w8(self, full_name: str, w: torch.Tensor) -> bool:
        """Takes the tensors of a block-scaled FP8 checkpoint (e4m3 weights
        and their weight_scale_inv) out of load_hf_state_dict's stream; True
        when the tensor was consumed here."""
        name = full_name.removeprefix("model.")
        stem, _, kind = name.rpartition(".")
        is_fp8 = w.dtype == torch.float8_e4m3fn
        if not is_fp8 and kind != "weight_scale_inv":
            if kind == "weight":
                tgt = self._w8_target(stem)
                if (tgt is not None and tgt[0] is not None
                        and getattr(tgt[0], "w8", False)):
                    raise ValueError(
                        f"{full_name}: plain {w.dtype} weight, but "
                        f"{tgt[1]} was prepared for FP8 (the checkpoint's "
                        "quantization_config does not list it under "
                        "modules_to_not_convert)")
            return False
        if is_fp8 and kind != "weight":
            raise ValueError(f"{full_name}: unexpected FP8 tensor (only "
                             "linear weights are read in FP8)")
        tgt = self._w8_target(stem)
        if tgt is None:
            raise ValueError(
                f"{full_name}: FP8 tensor for a module that is never "
                "quantized (embeddings, norms and router gates are read "
                "in bf16)")
        mod, modname, group, how = tgt
        if how == "skip":
            return True
        if not hasattr(self, "_w8_pending"):
            raise ValueError(
                f"{full_name}: FP8 tensor in the checkpoint but the model "
                "was not prepared for FP8 (config.json lacks "
                "quantization_config?)")
        if how == "dequant":
            self._w8_dequant_load(full_name, stem, kind, w)
            return True
        if how == "expert":
            parts = stem.split(".")
            proj = {"gate_proj": "gate", "up_proj": "up", "down_proj": "down",
                    "w1": "gate", "w3": "up", "w2": "down"}[parts[5]]
            mod.load_fp8_expert(full_name, int(parts[4]) - mod.expert_base,
                                proj, kind, w)
            return True
        if not getattr(mod, "w8", False):
            raise ValueError(
                f"{full_name}: FP8 tensor in the checkpoint but {modname} "
                "was not prepared for FP8 (it is on the checkpoint's skip "
                "list)")
        if group is None:
            self._load_w8(mod, modname, kind, [w], how)
            return True
        held = self._w8_pending.setdefault((modname, kind), {})
        held[stem] = {kind: w}
        if all(g in held for g in group):
            fulls = [held[g][kind] for g in group]
            del self._w8_pending[(modname, kind)]
            self._load_w8(mod, modname, kind, fulls, how)
        return True

    def _load_w8(self, mod, name: str, kind: str, fulls, how: str) -> None:
        """One tensor kind (weight / weight_scale_inv) of a projection, or
        of the fused partners `fulls`, into the module's W8 buffers. The
        block scales are expanded to one row per output channel first, so a
        column-parallel shard slices rows like the weight does and fused
        parts concatenate along N; a row-parallel shard slices K in whole
        128-blocks. The two kinds are independent, so they may arrive in
        different chunks."""
        from ..ops import ref

        B = ref.W8_BLOCK
        r = get_tp_rank()
        if kind == "weight":
            rows = list(fulls)
        else:
            rows = []
            for t in fulls:
                if t.dim() != 2:
                    raise ValueError(
                        f"{name}: weight_scale_inv {tuple(t.shape)} is not "
                        "a 2-D block scale")
                rows.append(t.float().repeat_interleave(B, dim=0))
        N, K = mod.w8_shape
        if how == "row":
            per = mod.in_per_rank if kind == "weight" else mod.in_per_rank // B
            # [:N]: the expanded scale rows run to the end of the last block
            parts = [rows[0][:N, r * per:(r + 1) * per]]
        elif len(rows) == 3:
            parts = mod.shard_qkv_parts(*rows)
        elif len(rows) == 2:
            parts = mod.shard_merged_parts(*rows)
        else:
            parts = [mod.shard(rows[0])]
        cols = K if kind == "weight" else K // B
        off = 0
        for part in parts:
            n = part.shape[0]
            if part.shape[1] != cols or off + n > N:
                raise ValueError(
                    f"{name}: FP8 {kind} part {tuple(part.shape)} does not "
                    f"fit the layer's {N}x{K} at block size {B}")
            if kind == "weight":
                mod.w8_weight[off:off + n].copy_(part)
            else:
                mod.w8_scales[:, off:off + n].copy_(part.t())
            off += n
        if off != N:
            raise ValueError(f"{name}: FP8 {kind} covers {off} of {N} rows")
        mod._w8_got.add(kind)

    def _w8_dequant_load(self, full_name: str, stem: str, kind: str,
                         w: torch.Tensor) -> None:
        """A routed expert or lm_head that arrives in FP8: hold the tensor
        until its partner is here, then dequantize to bf16 on the model's
        device and load it as the plain weight it replaces. One projection
        at a time, so the transient memory is one expert's."""
        import logging

        from ..ops import ref

        held = self._w8_pending.setdefault(("dequant", stem), {})
        pair = held.setdefault(stem, {})
        # the partner may come with a later chunk, after the staging buffer
        # this view points into has been recycled
        pair[kind] = w.clone()
        if len(pair) < 2:
            return
        del self._w8_pending[("dequant", stem)]
        if stem != "lm_head" and not self._w8_experts_logged:
            self._w8_experts_logged = True
            mlp = self.layers[int(stem.split(".")[1])].mlp
            why = ("the block was not prepared for FP8 experts"
                   if mlp.w8_supported() else
                   f"hidden={mlp.hidden}, expert width={mlp.inter}: the "
                   "grouped W8 kernel needs multiples of 128")
            logging.getLogger(__name__).warning(
                "FP8 routed experts are dequantized to bf16 at load (%s): "
                "the model holds these experts at bf16 size", why)
        dev = self.embed_tokens.weight.device
        w8 = pair["weight"].to(dev)
        scales = ref.w8_expand_scales(pair["weight_scale_inv"].to(dev),
                                      w8.shape[0])
        plain = ref.w8_dequant(w8, scales).to(self.dtype)
        pre = "" if stem == "lm_head" else "model."
        self.load_hf_state_dict({f"{pre}{stem}.weight": plain})

    # ---- MXFP4 checkpoints (MX4, W4A16; format in ops/ref.py) ----
    # X.weight u8 [N, K/2] + X.weight_scale u8 [N, K/32] per quantized
    # projection, as a Quark MXFP4 export stores them. The candidate layers
    # are _w4_targets(experts=True); routed experts (no grouped MX4 kernel)
    # and a quantized lm_head are dequantized to bf16 at load.
    _MX4_KINDS = ("weight", "weight_scale")

    def _mx4_skipped(self, hf_name: str) -> bool:
        """The export's `exclude` list: an entry names a module by its full
        name, by an fnmatch pattern over it, or (as for FP8 checkpoints) by
        dotted components that occur in a row in it."""
        import fnmatch

        return (self._w8_skipped(hf_name)
                or any(fnmatch.fnmatchcase(hf_name, e)
                       or fnmatch.fnmatchcase(hf_name.removeprefix("model."),
                                              e)
                       for e in self.cfg.quant_skip_modules))

    def quantize_mx4(self) -> None:
        """MX4 of a loaded bf16 model in memory by the OCP conversion rule
        (quantize_module_mx4 over the dense qkv/o/gate_up/down projections;
        lm_head, embeddings, router gates and every MoE expert stay bf16):
        --quantization mxfp4 on a bf16 checkpoint."""
        from ..parallel.layers import quantize_module_mx4

        for name, mod in self._w4_targets():
            quantize_module_mx4(mod, name)

    def prepare_mxfp4_checkpoint(self) -> None:
        """Switch the quantized layers to (empty) MX4 storage BEFORE an MXFP4
        checkpoint streams in, so their bf16 weights are never allocated on
        the device; finalize_mx4() completes the switch after loading. The
        parts of a fused projection must all be quantized or all be on the
        checkpoint's exclude list."""
        from ..parallel.layers import init_module_mx4

        self._mx4_pending = {}
        self._mx4_experts_logged = False
        for name, mod in self._w4_targets(experts=True):
            parts = self._w8_hf_parts(name)
            skipped = [self._mx4_skipped(p) for p in parts]
            if all(skipped):
                continue
            if any(skipped):
                raise ValueError(
                    f"{name}: the checkpoint quantizes only some parts of "
                    "this fused projection "
                    f"({dict(zip(parts, skipped))}: True = excluded, left "
                    "in bf16); they must all be MXFP4 or all excluded")
            init_module_mx4(mod, name)
            mod._mx4_got = set()

    def finalize_mx4(self) -> None:
        from ..parallel.layers import finalize_module_mx4

        for key, held in getattr(self, "_mx4_pending", {}).items():
            for stem, kinds in held.items():
                if key[0] != "dequant":
                    raise ValueError(
                        f"{stem}.{key[1]}: the fused partners of this MXFP4 "
                        f"tensor ({key[0]}) are missing from the checkpoint")
                if "weight" not in kinds:
                    raise ValueError(
                        f"{stem}.weight_scale: a scale without its weight "
                        "in the checkpoint")
                raise ValueError(
                    f"{stem}.weight: an MXFP4 weight without its "
                    "weight_scale in the checkpoint")
        for name, mod in self._w4_targets(experts=True):
            if not getattr(mod, "mx4", False):
                continue
            missing = set(self._MX4_KINDS) - mod._mx4_got
            if missing:
                raise ValueError(
                    f"{name}: the checkpoint has no {sorted(missing)} for "
                    "this MXFP4 layer")
            finalize_module_mx4(mod)

    def _route_mx4(self, full_name: str, w: torch.Tensor) -> bool:
        """Takes the tensors of an MXFP4 checkpoint (uint8 weights and their
        weight_scale) out of load_hf_state_dict's stream; True when the
        tensor was consumed here."""
        from ..ops import ref

        name = full_name.removeprefix("model.")
        stem, _, kind = name.rpartition(".")
        is_mx4 = w.dtype == torch.uint8 and kind == "weight"
        if not is_mx4 and kind != "weight_scale":
            if kind == "weight":
                tgt = self._w8_target(stem)
                if (tgt is not None and tgt[0] is not None
                        and getattr(tgt[0], "mx4", False)):
                    raise ValueError(
                        f"{full_name}: plain {w.dtype} weight, but "
                        f"{tgt[1]} was prepared for MXFP4 (the checkpoint's "
                        "quantization_config does not list it under "
                        "exclude)")
            return False
        tgt = self._w8_target(stem)
        if tgt is None:
            raise ValueError(
                f"{full_name}: MXFP4 tensor for a module that is never "
                "quantized (embeddings, norms and router gates are read "
                "in bf16)")
        mod, modname, group, how = tgt
        if how == "skip":
            return True
        if not hasattr(self, "_mx4_pending"):
            raise ValueError(
                f"{full_name}: MXFP4 tensor in the checkpoint but the model "
                "was not prepared for MXFP4 (config.json lacks "
                "quantization_config?)")
        if w.dtype != torch.uint8 or w.dim() != 2:
            raise ValueError(
                f"{full_name}: expected a 2-D uint8 tensor, got "
                f"{tuple(w.shape)} {w.dtype}")
        if kind == "weight_scale":
            # on the host, before anything is uploaded: outside this range a
            # scaled e2m1 value is not a normal finite bf16 (255 is NaN)
            lo, hi = int(w.min()), int(w.max())
            if lo < ref.MX4_SCALE_MIN or hi > ref.MX4_SCALE_MAX:
                raise ValueError(
                    f"{full_name}: e8m0 scale bytes span [{lo}, {hi}], "
                    f"outside the supported [{ref.MX4_SCALE_MIN}, "
                    f"{ref.MX4_SCALE_MAX}] (0.5 * 2^(s-127) must be a normal "
                    "bf16 and 6 * 2^(s-127) finite; 255 is NaN)")
        if how in ("dequant", "expert"):
            self._mx4_dequant_load(full_name, stem, kind, w)
            return True
        if not getattr(mod, "mx4", False):
            raise ValueError(
                f"{full_name}: MXFP4 tensor in the checkpoint but {modname} "
                "was not prepared for MXFP4 (it is on the checkpoint's "
                "exclude list)")
        if group is None:
            self._load_mx4(mod, modname, kind, [w], how)
            return True
        held = self._mx4_pending.setdefault((modname, kind), {})
        held[stem] = {kind: w}
        if all(g in held for g in group):
            fulls = [held[g][kind] for g in group]
            del self._mx4_pending[(modname, kind)]
            self._load_mx4(mod, modname, kind, fulls, how)
        return True

    def _load_mx4(self, mod, name: str, kind: str, fulls, how: str) -> None:
        """One tensor kind (weight / weight_scale) of a projection, or of
        the fused partners `fulls`, into the module's MX4 buffers, sharded on
        the host slice. Both kinds have one row per output channel, so a
        column-parallel shard slices rows of both and fused parts concatenate
        along N; a row-parallel shard slices K as K/2 bytes of nibbles and
        K/32 scale bytes. The two kinds are independent, so they may arrive
        in different chunks."""
        from ..ops import ref

        div = 2 if kind == "weight" else ref.MX4_BLOCK
        r = get_tp_rank()
        N, K = mod.mx4_shape
        if how == "row":
            per = mod.in_per_rank // div
            parts = [fulls[0][:, r * per:(r + 1) * per]]
        elif len(fulls) == 3:
            parts = mod.shard_qkv_parts(*fulls)
        elif len(fulls) == 2:
            parts = mod.shard_merged_parts(*fulls)
        else:
            parts = [mod.shard(fulls[0])]
        dst = mod.mx4_weight if kind == "weight" else mod.mx4_scales
        off = 0
        for part in parts:
            n = part.shape[0]
            if part.shape[1] != K // div or off + n > N:
                raise ValueError(
                    f"{name}: MXFP4 {kind} part {tuple(part.shape)} does "
                    f"not fit the layer's {N}x{K} ([N, K/{div}] bytes)")
            dst[off:off + n].copy_(part)
            off += n
        if off != N:
            raise ValueError(f"{name}: MXFP4 {kind} covers {off} of {N} rows")
        mod._mx4_got.add(kind)

    def _mx4_dequant_load(self, full_name: str, stem: str, kind: str,
                          w: torch.Tensor) -> None:
        """A routed expert or lm_head that arrives in MXFP4: hold the tensor
        until its partner is here, then dequantize to bf16 (exact) on the
        model's device and load it as the plain weight it replaces. One
        projection at a time, so the transient memory is one expert's."""
        import logging

        from ..ops import ref

        held = self._mx4_pending.setdefault(("dequant", stem), {})
        pair = held.setdefault(stem, {})
        # the partner may come with a later chunk, after the staging buffer
        # this view points into has been recycled
        pair[kind] = w.clone()
        if len(pair) < 2:
            return
        del self._mx4_pending[("dequant", stem)]
        if stem != "lm_head" and not self._mx4_experts_logged:
            self._mx4_experts_logged = True
            logging.getLogger(__name__).warning(
                "MXFP4 routed experts are dequantized to bf16 at load (no "
                "grouped MX4 kernel): the model holds its experts at bf16 "
                "size")
        dev = self.embed_tokens.weight.device
        plain = ref.mx4_dequant(pair["weight"].to(dev),
                                pair["weight_scale"].to(dev)).to(self.dtype)
        pre = "" if stem == "lm_head" else "model."
        self.load_hf_state_dict({f"{pre}{stem}.weight": plain})

    def _load_awq(self, mod, name: str, kind: str, fulls, shard_parts) -> None:
        """One AWQ tensor kind (qweight / qzeros / scales) of a projection,
        or of the fused partners `fulls`: unpack on the host to row form
        [N, K] or [N, K/128], shard with `shard_parts`, fuse along N and
        store in the module's packed buffers. The three kinds are
        independent, so they may arrive in different chunks."""
        from ..ops import ref

        if not getattr(mod, "w4", False):
            raise ValueError(
                f"{name}: AWQ tensor in the checkpoint but the model was not "
                "prepared for AWQ (config.json lacks quantization_config?)"
            )
        rows = []
        for t in fulls:
            t = t.cpu()
            if kind == "scales":
                rows.append(t.t())
            else:
                rows.append(ref._unpack_nibbles(t).t())
        fused = torch.cat([p for p in shard_parts(*rows)], dim=0).contiguous()
        if kind == "qweight":
            mod.w4_qweight.copy_(ref._pack_nibbles(fused))
        elif kind == "qzeros":
            mod.w4_zeros.copy_(fused.t().contiguous())
        else:
            mod.w4_scales.copy_(fused.t().contiguous().to(torch.float16))

    def _build_cos_sin(self, min_len: int | None = None):
        from ..ops import ref

        return ref.rope_cos_sin_cache(
            self.cfg.head_dim,
            max(self.cfg.max_position_embeddings, min_len or 0),
            self.cfg.rope_theta, rope_scaling=self.cfg.rope_scaling,
        )

    def extend_rope_table(self, min_len: int) -> None:
        """Grow the RoPE cos/sin table to at least `min_len` positions
        (serving past max_position_embeddings would otherwise read out of
        bounds in the rope kernel; plain RoPE extrapolates)."""
        if self.rope_cos_sin.shape[0] >= min_len:
            return
        cache = self._build_cos_sin(min_len).to(
            device=self.rope_cos_sin.device, dtype=self.rope_cos_sin.dtype
        )
        self.register_buffer("rope_cos_sin", cache, persistent=False)
        for layer in self.layers:
            layer.self_attn._cos_sin = cache

    def _apply(self, fn, recurse=True):  # keep the shared cos_sin in sync
        out = super()._apply(fn, recurse)
        for layer in self.layers:
            layer.self_attn._cos_sin = self.rope_cos_sin
        return out

    def forward(self, batch: ForwardBatch, kv_caches: list) -> torch.Tensor:
        """Returns logits for batch.logits_indices rows."""
        x, residual = self.forward_hidden(batch, kv_caches)
        return self.compute_logits(x, residual, batch)

    def forward_hidden(self, batch: ForwardBatch, kv_caches: list):
        """The decoder stack: (x, residual) of the last layer, before the
        final norm (x may still be an ops.SplitKPending)."""
        x = self.embed_tokens(batch.input_ids)
        residual = None
        for i, layer in enumerate(self.layers):
            x, residual = layer(x, residual, batch, kv_caches[i])
        return x, residual

    def pool(self, x, residual, table, carry, dims, normalize):
        """Embeddings of the pooled segments of `table` from forward_hidden's
        output, which it leaves untouched: call it before compute_logits,
        whose fused norm adds x into residual in place."""
        return ops.pool_embed(x, residual, self.norm.weight, self.norm.eps,
                              table, carry, dims=dims, normalize=normalize)

    def compute_logits(self, x, residual, batch: ForwardBatch) -> torch.Tensor:
        """Final norm and lm_head over batch.logits_indices rows."""
        if not self.has_lm_head:
            raise RuntimeError(
                "this checkpoint has no lm_head (an embedding model): it "
                "cannot produce logits")
        x, _ = self.norm(x, residual)
        if isinstance(x, tuple):  # fp8: (values, per-token scales)
            q8, sc = x
            if batch.logits_indices is not None:
                q8 = q8[batch.logits_indices]
                sc = sc[batch.logits_indices]
            return self.lm_head((q8, sc))
        if batch.logits_indices is not None:
            x = x[batch.logits_indices]
        return self.lm_head(x)

    # ------------------------- weight loading -------------------------
    def load_hf_state_dict(self, tensors: dict[str, torch.Tensor]) -> None:
        """Load an HF-layout state dict (full tensors; sharded here)."""
        pending_qkv: dict[int, dict] = {}
        pending_mlp: dict[int, dict] = {}
        own = dict(self.named_parameters())

        def put(name, value):
            p = own[name]
            assert p.shape == value.shape, (name, p.shape, value.shape)
            p.data.copy_(value.to(p.dtype))

        def put_cat(name, parts):
            # fused params load piecewise: each (pinned) slice goes straight
            # into its span of the parameter — no host-side torch.cat copy
            p = own[name]
            off = 0
            for part in parts:
                n = part.shape[0]
                p.data[off:off + n].copy_(part.to(p.dtype))
                off += n
            assert off == p.shape[0], (name, off, p.shape)

        for name, w in tensors.items():
            if self._route_w8(name, w) or self._route_mx4(name, w):
                continue
            name = name.removeprefix("model.")
            if name == "embed_tokens.weight":
                put("embed_tokens.weight", w)
                if self.cfg.tie_word_embeddings:
                    put("lm_head.weight", self.lm_head.shard(w))
                    self._lm_head_loaded = True
            elif name in ("lm_head.weight",):
                put("lm_head.weight", self.lm_head.shard(w))
                self._lm_head_loaded = True
            elif name == "norm.weight":
                put("norm.weight", w)
            elif name.startswith("layers."):
                parts = name.split(".")
                li = int(parts[1])
                sub = ".".join(parts[2:])
                layer = self.layers[li]
                if sub in ("input_layernorm.weight", "post_attention_layernorm.weight"):
                    put(f"layers.{li}.{sub}", w)
                elif sub in ("self_attn.q_norm.weight", "self_attn.k_norm.weight"):
                    put(f"layers.{li}.{sub}", w)
                elif sub.startswith("self_attn.") and sub.split(".")[1] in (
                    "q_proj", "k_proj", "v_proj",
                ):
                    proj, param = sub.split(".")[1], sub.split(".")[2]
                    pending_qkv.setdefault(li, {})[f"{proj}.{param}"] = w
                    d = pending_qkv[li]
                    keys_a = [f"{p}.{param}"
                              for p in ("q_proj", "k_proj", "v_proj")]
                    if param in _AWQ_KINDS and all(k in d for k in keys_a):
                        qkv = layer.self_attn.qkv_proj
                        self._load_awq(
                            qkv, f"layers.{li}.self_attn.qkv_proj", param,
                            [d.pop(k) for k in keys_a], qkv.shard_qkv_parts)
                    keys_w = {"q_proj.weight", "k_proj.weight", "v_proj.weight"}
                    keys_b = {"q_proj.bias", "k_proj.bias", "v_proj.bias"}
                    if keys_w <= d.keys():
                        parts = layer.self_attn.qkv_proj.shard_qkv_parts(
                            d["q_proj.weight"], d["k_proj.weight"], d["v_proj.weight"]
                        )
                        put_cat(f"layers.{li}.self_attn.qkv_proj.weight", parts)
                        for kk in keys_w:
                            del d[kk]
                    if layer.self_attn.qkv_proj.bias is not None and keys_b <= d.keys():
                        parts = layer.self_attn.qkv_proj.shard_qkv_parts(
                            d["q_proj.bias"], d["k_proj.bias"], d["v_proj.bias"]
                        )
                        put_cat(f"layers.{li}.self_attn.qkv_proj.bias", parts)
                        for kk in keys_b:
                            del d[kk]
                elif (parts[-1] in _AWQ_KINDS and ".".join(parts[2:-1]) in (
                        "mlp.gate", "block_sparse_moe.gate",
                        "mlp.shared_expert_gate")):
                    raise ValueError(
                        f"{name}: a quantized router gate is not supported "
                        "(AWQ checkpoints keep the MoE gates in f16)")
                elif (parts[-1] == "weight" and getattr(layer.mlp, "w4", False)
                      and sub.startswith(("mlp.experts.",
                                          "block_sparse_moe.experts."))):
                    raise ValueError(
                        f"{name}: plain weight of an MoE expert in an AWQ "
                        "checkpoint (mixed-precision expert checkpoints are "
                        "not supported)")
                elif (parts[-1] == "weight"
                      and sub.startswith("mlp.shared_expert.")
                      and getattr(layer.mlp.shared.down_proj, "w4", False)):
                    raise ValueError(
                        f"{name}: plain weight of the shared expert in an "
                        "AWQ checkpoint (mixed-precision expert checkpoints "
                        "are not supported)")
                elif (parts[-1] in _AWQ_KINDS and sub.startswith(
                        ("mlp.experts.", "block_sparse_moe.experts."))):
                    # experts.N.{gate,up,down}_proj.* (Qwen-MoE) or
                    # experts.N.{w1,w3,w2}.* (Mixtral); other ranks' experts
                    # are skipped
                    moe = layer.mlp
                    le = int(parts[4]) - moe.expert_base
                    proj = {"gate_proj": "gate", "up_proj": "up",
                            "down_proj": "down", "w1": "gate", "w3": "up",
                            "w2": "down"}.get(parts[5])
                    if proj is not None and 0 <= le < moe.local_experts:
                        moe.load_awq_expert(name, le, proj, parts[-1], w)
                elif (parts[-1] in _AWQ_KINDS
                      and sub.startswith("mlp.shared_expert.down_proj.")):
                    mod = layer.mlp.shared.down_proj
                    kind = parts[-1]
                    per = mod.in_per_rank // (1 if kind == "qweight" else 128)
                    r = get_tp_rank()
                    self._load_awq(
                        mod, f"layers.{li}.mlp.shared_expert.down_proj", kind,
                        [w], lambda full: [full[:, r * per:(r + 1) * per]])
                elif (parts[-1] in _AWQ_KINDS and sub.startswith(
                        ("mlp.shared_expert.gate_proj.",
                         "mlp.shared_expert.up_proj."))):
                    kind = parts[-1]
                    d = pending_mlp.setdefault((li, "se", kind), {})
                    d[sub] = w
                    keys_a = [f"mlp.shared_expert.{p}.{kind}"
                              for p in ("gate_proj", "up_proj")]
                    if all(k in d for k in keys_a):
                        gu = layer.mlp.shared.gate_up_proj
                        self._load_awq(
                            gu, f"layers.{li}.mlp.shared_expert.gate_up_proj",
                            kind, [d.pop(k) for k in keys_a],
                            gu.shard_merged_parts)
                elif sub == "self_attn.o_proj.weight":
                    put(
                        f"layers.{li}.self_attn.o_proj.weight",
                        layer.self_attn.o_proj.shard(w),
                    )
                elif (sub.startswith(("self_attn.o_proj.", "mlp.down_proj."))
                      and sub.split(".")[2] in _AWQ_KINDS):
                    mod = (layer.self_attn.o_proj if "o_proj" in sub
                           else layer.mlp.down_proj)
                    kind = sub.split(".")[2]
                    per = mod.in_per_rank // (1 if kind == "qweight" else 128)
                    r = get_tp_rank()
                    self._load_awq(
                        mod, f"layers.{li}.{sub.rsplit('.', 1)[0]}", kind, [w],
                        lambda full: [full[:, r * per:(r + 1) * per]])
                elif (sub.startswith(("mlp.gate_proj.", "mlp.up_proj."))
                      and sub.split(".")[2] in _AWQ_KINDS):
                    kind = sub.split(".")[2]
                    d = pending_mlp.setdefault((li, kind), {})
                    d[sub] = w
                    keys_a = [f"mlp.{p}.{kind}" for p in ("gate_proj", "up_proj")]
                    if all(k in d for k in keys_a):
                        gu = layer.mlp.gate_up_proj
                        self._load_awq(
                            gu, f"layers.{li}.mlp.gate_up_proj", kind,
                            [d.pop(k) for k in keys_a], gu.shard_merged_parts)
                elif sub in ("mlp.gate_proj.weight", "mlp.up_proj.weight"):
                    pending_mlp.setdefault(li, {})[sub] = w
                    d = pending_mlp[li]
                    if {"mlp.gate_proj.weight", "mlp.up_proj.weight"} <= d.keys():
                        parts = layer.mlp.gate_up_proj.shard_merged_parts(
                            d["mlp.gate_proj.weight"], d["mlp.up_proj.weight"]
                        )
                        put_cat(f"layers.{li}.mlp.gate_up_proj.weight", parts)
                        d.clear()
                elif sub == "mlp.down_proj.weight":
                    put(f"layers.{li}.mlp.down_proj.weight", layer.mlp.down_proj.shard(w))
                elif sub == "mlp.shared_expert_gate.weight":
                    layer.mlp.shared_gate.data.copy_(
                        w.to(layer.mlp.shared_gate.dtype))
                elif sub in ("mlp.shared_expert.gate_proj.weight",
                             "mlp.shared_expert.up_proj.weight"):
                    pending_mlp.setdefault((li, "se"), {})[sub] = w
                    d = pending_mlp[(li, "se")]
                    if len(d) == 2:
                        fused = layer.mlp.shared.gate_up_proj.shard_merged(
                            d["mlp.shared_expert.gate_proj.weight"],
                            d["mlp.shared_expert.up_proj.weight"],
                        )
                        layer.mlp.shared.gate_up_proj.weight.data.copy_(
                            fused.to(layer.mlp.shared.gate_up_proj.weight.dtype))
                        d.clear()
                elif sub == "mlp.shared_expert.down_proj.weight":
                    layer.mlp.shared.down_proj.weight.data.copy_(
                        layer.mlp.shared.down_proj.shard(w).to(
                            layer.mlp.shared.down_proj.weight.dtype))
                elif sub in ("block_sparse_moe.gate.weight", "mlp.gate.weight"):
                    layer.mlp.gate.data.copy_(w.to(layer.mlp.gate.dtype))
                elif sub.startswith("mlp.experts."):
                    # Qwen3-MoE naming: experts.N.{gate,up,down}_proj.weight
                    moe = layer.mlp
                    e = int(sub.split(".")[2])
                    which = sub.split(".")[3]
                    le = e - moe.expert_base
                    if 0 <= le < moe.local_experts:
                        # HF [out, in] -> our pre-transposed [in, out]
                        I = moe.inter
                        if which == "gate_proj":
                            moe.w13.data[le, :, :I].copy_(w.t().to(moe.w13.dtype))
                        elif which == "up_proj":
                            moe.w13.data[le, :, I:].copy_(w.t().to(moe.w13.dtype))
                        elif which == "down_proj":
                            moe.w2.data[le].copy_(w.t().to(moe.w2.dtype))
                elif sub.startswith("block_sparse_moe.experts."):
                    # Mixtral expert naming: w1=gate, w3=up, w2=down.
                    # EP-sharded: only this rank's experts are kept.
                    moe = layer.mlp
                    e = int(sub.split(".")[2])
                    which = sub.split(".")[3]
                    le = e - moe.expert_base
                    if 0 <= le < moe.local_experts:
                        # HF [out, in] -> our pre-transposed [in, out]
                        I = moe.inter
                        if which == "w1":
                            moe.w13.data[le, :, :I].copy_(w.t().to(moe.w13.dtype))
                        elif which == "w3":
                            moe.w13.data[le, :, I:].copy_(w.t().to(moe.w13.dtype))
                        elif which == "w2":
                            moe.w2.data[le].copy_(w.t().to(moe.w2.dtype))
                # rotary_emb.inv_freq etc. are ignored (recomputed)

    @torch.no_grad()
    def random_init(self, seed: int = 0) -> None:
        """Random-init with TP-consistent semantics: full HF-layout tensors
        are generated deterministically per name (so every TP rank sees
        slices of the SAME logical weights) and routed through the normal
        shard-aware loader. Generates on the model's device when possible."""
        import zlib

        cfg = self.cfg
        dev = self.embed_tokens.weight.device

        def gen(name: str, *shape, std: float = 0.02) -> torch.Tensor:
            s = (seed * 1000003 + zlib.crc32(name.encode())) % (2**63 - 1)
            if dev.type == "cuda":
                g = torch.Generator(device=dev).manual_seed(s)
                t = torch.randn(shape, generator=g, dtype=torch.float32, device=dev)
            else:
                g = torch.Generator().manual_seed(s)
                t = torch.randn(shape, generator=g, dtype=torch.float32)
            return t.mul_(std)

        H, I, hd = cfg.hidden_size, cfg.intermediate_size, cfg.head_dim
        nq, nkv = cfg.num_attention_heads, cfg.num_key_value_heads
        glob: dict[str, torch.Tensor] = {
            "model.embed_tokens.weight": gen("embed", cfg.vocab_size, H),
            "model.norm.weight": torch.ones(H),
        }
        if not cfg.tie_word_embeddings:
            glob["lm_head.weight"] = gen("lm_head", cfg.vocab_size, H)
        self.load_hf_state_dict(glob)
        del glob
        for i in range(cfg.num_hidden_layers):
            pre = f"model.layers.{i}"
            tensors = {
                f"{pre}.self_attn.q_proj.weight": gen(f"{pre}.q", nq * hd, H),
                f"{pre}.self_attn.k_proj.weight": gen(f"{pre}.k", nkv * hd, H),
                f"{pre}.self_attn.v_proj.weight": gen(f"{pre}.v", nkv * hd, H),
                f"{pre}.self_attn.o_proj.weight": gen(f"{pre}.o", H, nq * hd),
                f"{pre}.input_layernorm.weight": torch.ones(H),
                f"{pre}.post_attention_layernorm.weight": torch.ones(H),
            }
            if cfg.num_local_experts > 0:
                Ie = cfg.moe_intermediate_size or I
                if cfg.shared_expert_intermediate_size:
                    Is = cfg.shared_expert_intermediate_size
                    sp = f"{pre}.mlp.shared_expert"
                    tensors[f"{sp}.gate_proj.weight"] = gen(f"{sp}.g", Is, H)
                    tensors[f"{sp}.up_proj.weight"] = gen(f"{sp}.u", Is, H)
                    tensors[f"{sp}.down_proj.weight"] = gen(f"{sp}.d", H, Is)
                    tensors[f"{pre}.mlp.shared_expert_gate.weight"] = gen(
                        f"{sp}.sg", 1, H
                    )
                qstyle = not cfg.architecture.startswith("MixtralFor")
                gname = "mlp.gate" if qstyle else "block_sparse_moe.gate"
                tensors[f"{pre}.{gname}.weight"] = gen(
                    f"{pre}.moe.gate", cfg.num_local_experts, H
                )
                for e in range(cfg.num_local_experts):
                    if qstyle:
                        ep = f"{pre}.mlp.experts.{e}"
                        tensors[f"{ep}.gate_proj.weight"] = gen(f"{ep}.w1", Ie, H)
                        tensors[f"{ep}.up_proj.weight"] = gen(f"{ep}.w3", Ie, H)
                        tensors[f"{ep}.down_proj.weight"] = gen(f"{ep}.w2", H, Ie)
                    else:
                        ep = f"{pre}.block_sparse_moe.experts.{e}"
                        tensors[f"{ep}.w1.weight"] = gen(f"{ep}.w1", Ie, H)
                        tensors[f"{ep}.w3.weight"] = gen(f"{ep}.w3", Ie, H)
                        tensors[f"{ep}.w2.weight"] = gen(f"{ep}.w2", H, Ie)
            else:
                tensors[f"{pre}.mlp.gate_proj.weight"] = gen(f"{pre}.gate", I, H)
                tensors[f"{pre}.mlp.up_proj.weight"] = gen(f"{pre}.up", I, H)
                tensors[f"{pre}.mlp.down_proj.weight"] = gen(f"{pre}.down", H, I)
            if cfg.qk_norm:
                tensors[f"{pre}.self_attn.q_norm.weight"] = torch.ones(hd)
                tensors[f"{pre}.self_attn.k_norm.weight"] = torch.ones(hd)
            if cfg.attention_bias:
                tensors[f"{pre}.self_attn.q_proj.bias"] = torch.zeros(nq * hd)
                tensors[f"{pre}.self_attn.k_proj.bias"] = torch.zeros(nkv * hd)
                tensors[f"{pre}.self_attn.v_proj.bias"] = torch.zeros(nkv * hd)
            # load layer-by-layer to bound peak memory
            self.load_hf_state_dict(tensors)
