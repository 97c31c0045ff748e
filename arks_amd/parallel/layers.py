"""Tensor-parallel linear layers (Megatron-style column/row split).

GEMMs go through F.linear (hipBLASLt on ROCm — the guide's 'plain library
GEMM' path); the fused hot ops around them are the hand-written kernels in
arks_amd.ops. Weight loading maps full HF tensors to local shards via each
layer's `shard()`.
"""

from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from .comm import get_tp_rank, get_tp_world_size, tp_all_gather, tp_all_reduce


def quantize_module_fp8(mod: nn.Module) -> None:
    """Switch a linear layer to W8A8 fp8 (OCP e4m3, per-output-channel weight
    scales, dynamic per-token activation scales — ops.quant_fp8_rows).
    The bf16 weight parameter is dropped on CUDA to free HBM; on CPU a
    quant-dequant copy emulates the GPU numerics for tests."""
    w = mod.weight.data
    amax = w.float().abs().amax(dim=1).clamp(min=1e-6)
    scale = 448.0 / amax
    w8 = (w.float() * scale[:, None]).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)
    mod.register_buffer("weight_fp8", w8, persistent=False)
    mod.register_buffer(
        "w_inv_scale", (1.0 / scale).float()[None, :], persistent=False
    )
    if w.is_cuda:
        del mod._parameters["weight"]
        mod.weight = None
    else:
        mod.register_buffer(
            "weight_qdq",
            (w8.float() * (1.0 / scale)[:, None]).to(w.dtype),
            persistent=False,
        )
    mod.fp8 = True


def _fp8_linear_prequant(mod: nn.Module, x8, sa) -> torch.Tensor:
    """fp8 GEMM on an already-quantized activation (the producing kernel —
    rmsnorm_fp8 / silu_mul_fp8 — emitted x8 + per-token scales)."""
    if x8.is_cuda:
        return torch._scaled_mm(
            x8, mod.weight_fp8.t(), scale_a=sa[:, None], scale_b=mod.w_inv_scale,
            bias=mod.bias, out_dtype=torch.bfloat16,
        )
    xd = (x8.float() * sa[:, None]).to(torch.bfloat16)
    return F.linear(xd, mod.weight_qdq, mod.bias)


def _fp8_linear(mod: nn.Module, x: torch.Tensor) -> torch.Tensor:
    from .. import ops

    if x.is_cuda:
        x8, sa = ops.quant_fp8_rows(x)
        return torch._scaled_mm(
            x8, mod.weight_fp8.t(), scale_a=sa[:, None], scale_b=mod.w_inv_scale,
            bias=mod.bias, out_dtype=x.dtype,
        )
    # CPU emulation: quant-dequant both operands, accumulate in f32
    x8, sa = ops.quant_fp8_rows(x)
    xd = (x8.float() * sa[:, None]).to(x.dtype)
    return F.linear(xd, mod.weight_qdq, mod.bias)


def _w4_check_shape(mod: nn.Module, name: str) -> tuple[int, int]:
    from ..ops import ref

    N, K = mod.weight.shape
    if K % ref.W4_GROUP != 0:
        raise ValueError(
            f"{name}: int4 needs the per-rank input width to be a multiple "
            f"of the group size {ref.W4_GROUP}, got K={K} at TP="
            f"{get_tp_world_size()}"
        )
    if N % 8 != 0:
        raise ValueError(f"{name}: int4 needs N % 8 == 0, got N={N}")
    return N, K


def _w4_set_storage(mod: nn.Module, name: str) -> tuple[int, int]:
    """Replace mod.weight [N, K] by (empty) packed W4 buffers; returns (N, K).
    The bf16 parameter is dropped, so a model switched before its weights
    stream in never holds them."""
    from .. import ops
    from ..ops import ref

    N, K = _w4_check_shape(mod, name)
    dev = mod.weight.device
    G = K // ref.W4_GROUP
    del mod._parameters["weight"]
    mod.weight = None
    mod.register_buffer(
        "w4_qweight", torch.zeros(N, K // 8, dtype=torch.int32, device=dev),
        persistent=False)
    mod.register_buffer(
        "w4_scales", torch.zeros(G, N, dtype=torch.float16, device=dev),
        persistent=False)
    mod.register_buffer(
        "w4_zeros", torch.zeros(G, N, dtype=torch.uint8, device=dev),
        persistent=False)
    mod.w4 = True
    mod.w4_shape = (N, K)
    ops.reserve_dequant_workspace(N * K, dev)
    return N, K


def init_module_w4(mod: nn.Module, name: str = "linear") -> None:
    """Switch a linear layer to W4 storage with nothing in it yet (an AWQ
    checkpoint is about to stream into the packed buffers)."""
    _w4_set_storage(mod, name)


def finalize_module_w4(mod: nn.Module) -> None:
    """After the packed buffers are filled: reserve the device's dequant
    workspace (the module may have moved since it was switched) and, on CPU,
    keep the bf16 dequantized weight that emulates the GPU numerics."""
    from .. import ops
    from ..ops import ref

    dev = mod.w4_qweight.device
    if dev.type == "cuda":
        ops.reserve_dequant_workspace(mod.w4_shape[0] * mod.w4_shape[1], dev)
        return
    packed = (mod.w4_qweight, mod.w4_scales, mod.w4_zeros)
    mod.register_buffer(
        "weight_qdq",
        ref.w4_dequant(*ref.w4_unpack(packed)).to(torch.bfloat16),
        persistent=False,
    )


def quantize_module_w4(mod: nn.Module, name: str = "linear") -> None:
    """Switch a linear layer to W4A16: round-to-nearest 4-bit asymmetric
    weights, group size 128 along K (ops.ref.w4_quantize), packed for
    ops.w4_linear. The bf16 parameter is dropped; on CPU a bf16 dequantized
    copy emulates the GPU numerics for tests."""
    from ..ops import ref

    _w4_check_shape(mod, name)
    w = mod.weight.data
    packed = ref.w4_pack(*ref.w4_quantize(w))
    _w4_set_storage(mod, name)
    mod.w4_qweight.copy_(packed[0])
    mod.w4_scales.copy_(packed[1])
    mod.w4_zeros.copy_(packed[2])
    finalize_module_w4(mod)


def _w4_linear(mod: nn.Module, x, bias, defer: bool):
    if not x.is_cuda:
        return F.linear(x, mod.weight_qdq, bias)
    from .. import ops

    return ops.w4_linear(x, (mod.w4_qweight, mod.w4_scales, mod.w4_zeros),
                         bias, defer=defer)


def _w8_check_shape(mod: nn.Module, name: str) -> tuple[int, int]:
    from ..ops import ref

    N, K = mod.weight.shape
    if K % ref.W8_BLOCK != 0:
        raise ValueError(
            f"{name}: block-scaled fp8 needs the per-rank input width to be "
            f"a multiple of the block size {ref.W8_BLOCK}, got K={K} at TP="
            f"{get_tp_world_size()}"
        )
    if N % 64 != 0:
        raise ValueError(
            f"{name}: block-scaled fp8 needs the per-rank output width to "
            f"be a multiple of 64, got N={N} at TP={get_tp_world_size()}"
        )
    return N, K


def init_module_w8(mod: nn.Module, name: str = "linear") -> None:
    """Switch a linear layer to (empty) W8 storage: w8_weight e4m3fn [N, K]
    exactly as a block-scaled FP8 checkpoint stores it, w8_scales f32
    [K/128, N]. The bf16 parameter is dropped, so a model switched before
    its weights stream in never holds it."""
    from .. import ops
    from ..ops import ref

    N, K = _w8_check_shape(mod, name)
    dev = mod.weight.device
    mod.w8_dtype = mod.weight.dtype
    del mod._parameters["weight"]
    mod.weight = None
    mod.register_buffer(
        "w8_weight", torch.zeros(N, K, dtype=torch.float8_e4m3fn, device=dev),
        persistent=False)
    mod.register_buffer(
        "w8_scales",
        torch.ones(K // ref.W8_BLOCK, N, dtype=torch.float32, device=dev),
        persistent=False)
    mod.w8 = True
    mod.w8_shape = (N, K)
    ops.reserve_dequant_workspace(N * K, dev)


def finalize_module_w8(mod: nn.Module) -> None:
    """After the W8 buffers are filled: reserve the device's dequant
    workspace (the module may have moved since it was switched) and, on CPU,
    keep the dequantized weight in the layer's dtype so that the CPU path is
    F.linear on it."""
    from .. import ops
    from ..ops import ref

    dev = mod.w8_weight.device
    if dev.type == "cuda":
        ops.reserve_dequant_workspace(mod.w8_shape[0] * mod.w8_shape[1], dev)
        return
    mod.register_buffer(
        "weight_qdq",
        ref.w8_dequant(mod.w8_weight, mod.w8_scales).to(mod.w8_dtype),
        persistent=False,
    )


def quantize_module_w8(mod: nn.Module, name: str = "linear") -> None:
    """Switch a loaded linear layer to W8A16 in memory: block-wise amax/448
    e4m3 weights (ops.ref.w8_quantize). For tests and benchmarks; serving
    reads the format from a checkpoint."""
    from ..ops import ref

    N, _ = _w8_check_shape(mod, name)
    w8, blocks = ref.w8_quantize(mod.weight.data)
    init_module_w8(mod, name)
    mod.w8_weight.copy_(w8)
    mod.w8_scales.copy_(ref.w8_expand_scales(blocks, N))
    finalize_module_w8(mod)


def _w8_linear(mod: nn.Module, x, bias, defer: bool):
    if not x.is_cuda:
        return F.linear(x, mod.weight_qdq, bias)
    from .. import ops

    return ops.w8_linear(x, (mod.w8_weight, mod.w8_scales), bias, defer=defer)


def _mx4_check_shape(mod: nn.Module, name: str) -> tuple[int, int]:
    N, K = mod.weight.shape
    if K % 128 != 0:
        raise ValueError(
            f"{name}: mxfp4 needs the per-rank input width to be a multiple "
            f"of 128 (four MX blocks, one chunk of the kernel), got K={K} at "
            f"TP={get_tp_world_size()}"
        )
    if N % 64 != 0:
        raise ValueError(
            f"{name}: mxfp4 needs the per-rank output width to be a multiple "
            f"of 64, got N={N} at TP={get_tp_world_size()}"
        )
    return N, K


def init_module_mx4(mod: nn.Module, name: str = "linear") -> None:
    """Switch a linear layer to (empty) MX4 storage: mx4_weight u8 [N, K/2]
    and mx4_scales u8 [N, K/32] exactly as an MXFP4 checkpoint stores them
    (format in ops/ref.py). The bf16 parameter is dropped, so a model
    switched before its weights stream in never holds it."""
    from .. import ops
    from ..ops import ref

    N, K = _mx4_check_shape(mod, name)
    dev = mod.weight.device
    mod.mx4_dtype = mod.weight.dtype
    del mod._parameters["weight"]
    mod.weight = None
    mod.register_buffer(
        "mx4_weight", torch.zeros(N, K // 2, dtype=torch.uint8, device=dev),
        persistent=False)
    mod.register_buffer(
        "mx4_scales",
        torch.full((N, K // ref.MX4_BLOCK), 127, dtype=torch.uint8,
                   device=dev),
        persistent=False)
    mod.mx4 = True
    mod.mx4_shape = (N, K)
    ops.reserve_dequant_workspace(N * K, dev)


def finalize_module_mx4(mod: nn.Module) -> None:
    """After the MX4 buffers are filled: reserve the device's dequant
    workspace (the module may have moved since it was switched) and, on CPU,
    keep the dequantized weight in the layer's dtype so that the CPU path is
    F.linear on it."""
    from .. import ops
    from ..ops import ref

    dev = mod.mx4_weight.device
    if dev.type == "cuda":
        ops.reserve_dequant_workspace(mod.mx4_shape[0] * mod.mx4_shape[1],
                                      dev)
        return
    mod.register_buffer(
        "weight_qdq",
        ref.mx4_dequant(mod.mx4_weight, mod.mx4_scales).to(mod.mx4_dtype),
        persistent=False,
    )


def quantize_module_mx4(mod: nn.Module, name: str = "linear") -> None:
    """Switch a loaded linear layer to MX4 in memory by the OCP MX conversion
    rule (ops.ref.mx4_quantize): what --quantization mxfp4 does to a bf16
    checkpoint."""
    from ..ops import ref

    _mx4_check_shape(mod, name)
    packed, scales = ref.mx4_quantize(mod.weight.data)
    init_module_mx4(mod, name)
    mod.mx4_weight.copy_(packed)
    mod.mx4_scales.copy_(scales)
    finalize_module_mx4(mod)


def _mx4_linear(mod: nn.Module, x, bias, defer: bool):
    if not x.is_cuda:
        return F.linear(x, mod.weight_qdq, bias)
    from .. import ops

    return ops.mx4_linear(x, (mod.mx4_weight, mod.mx4_scales), bias,
                          defer=defer)


class LoRAState:
    """Per-layer multi-LoRA slot tensors (arks_amd/loader/lora_loader.py):
    A [max_loras, S*R, K] and B [max_loras, N, R] bf16 over the layer's LOCAL
    widths, the fused-slice column offsets, and the runner-wide f32 shrink
    workspace. Allocated once; adapters are copied into their slot in place,
    so the pointers captured into decode graphs never change."""

    def __init__(self, A: torch.Tensor, B: torch.Tensor,
                 slice_offsets: tuple[int, ...], h_ws: torch.Tensor):
        self.A = A
        self.B = B
        self.slice_offsets = slice_offsets
        # this layer's [rows, S*R] view of the shared flat workspace
        sr = A.shape[1]
        rows = h_ws.numel() // sr
        self.h_ws = h_ws[: rows * sr].view(rows, sr)

    def apply(self, y: torch.Tensor, x: torch.Tensor, tiles: torch.Tensor):
        from .. import ops

        ops.lora_apply(y, x, self.A, self.B, tiles, self.slice_offsets,
                       self.h_ws)
        return y


class ColumnParallelLinear(nn.Module):
    """Y = X W^T with W row-sharded over TP ranks (output features split).
    Output stays sharded (gather_output=False semantics)."""

    def __init__(self, in_features: int, out_features: int, bias: bool,
                 dtype: torch.dtype = torch.bfloat16):
        super().__init__()
        tp = get_tp_world_size()
        assert out_features % tp == 0, (out_features, tp)
        self.in_features = in_features
        self.out_features = out_features
        self.out_per_rank = out_features // tp
        self.weight = nn.Parameter(
            torch.empty(self.out_per_rank, in_features, dtype=dtype),
            requires_grad=False,
        )
        self.bias = (
            nn.Parameter(torch.empty(self.out_per_rank, dtype=dtype), requires_grad=False)
            if bias
            else None
        )

    def shard(self, full: torch.Tensor, param: str = "weight") -> torch.Tensor:
        r = get_tp_rank()
        return full[r * self.out_per_rank : (r + 1) * self.out_per_rank]

    fp8 = False
    w4 = False
    w8 = False  # block-scaled e4m3 weights (init_module_w8)
    mx4 = False  # MXFP4 weights (init_module_mx4)
    lora: LoRAState | None = None  # set when the engine runs enable_lora

    def forward(self, x, lora_tiles=None, defer: bool = False):
        """defer=True: the caller can consume an ops.SplitKPending in place
        of the tensor (see ops.skinny_gemm). Granted only where the fused
        consumers are valid: bf16, W4, W8 or MX4 GEMM, TP world size 1, no LoRA
        delta."""
        if isinstance(x, tuple):  # pre-quantized by the producing kernel
            return _fp8_linear_prequant(self, *x)
        if self.fp8:
            return _fp8_linear(self, x)
        from .. import ops

        use_lora = lora_tiles is not None and self.lora is not None
        defer = defer and not use_lora and get_tp_world_size() == 1
        if self.w4:
            y = _w4_linear(self, x, self.bias, defer)
        elif self.w8:
            y = _w8_linear(self, x, self.bias, defer)
        elif self.mx4:
            y = _mx4_linear(self, x, self.bias, defer)
        else:
            y = ops.linear_bf16(x, self.weight, self.bias, defer=defer)
        if use_lora:
            self.lora.apply(y, x, lora_tiles)
        return y


class QKVParallelLinear(ColumnParallelLinear):
    """Fused QKV projection; q/k/v head groups are sharded per rank.
    Weight layout per rank: [q_shard | k_shard | v_shard]."""

    def __init__(self, hidden: int, head_dim: int, num_q_heads: int,
                 num_kv_heads: int, bias: bool, dtype=torch.bfloat16):
        tp = get_tp_world_size()
        assert num_q_heads % tp == 0 and num_kv_heads % tp == 0
        self.head_dim = head_dim
        self.nq, self.nkv = num_q_heads, num_kv_heads
        self.nq_local = num_q_heads // tp
        self.nkv_local = num_kv_heads // tp
        out = (self.nq_local + 2 * self.nkv_local) * head_dim * tp  # per-rank x tp
        super().__init__(hidden, out, bias, dtype)

    def shard_qkv_parts(self, q_full, k_full, v_full) -> list[torch.Tensor]:
        """This rank's q/k/v slices in fused order (views — callers copy
        each part straight into the fused parameter, no host-side cat)."""
        r = get_tp_rank()
        hd = self.head_dim
        return [
            q_full[r * self.nq_local * hd: (r + 1) * self.nq_local * hd],
            k_full[r * self.nkv_local * hd: (r + 1) * self.nkv_local * hd],
            v_full[r * self.nkv_local * hd: (r + 1) * self.nkv_local * hd],
        ]

    def shard_qkv(self, q_full, k_full, v_full) -> torch.Tensor:
        """Build this rank's fused weight (or bias) from full q/k/v tensors."""
        return torch.cat(self.shard_qkv_parts(q_full, k_full, v_full), dim=0)

    def split_qkv(self, qkv: torch.Tensor):
        hd = self.head_dim
        q, k, v = qkv.split(
            [self.nq_local * hd, self.nkv_local * hd, self.nkv_local * hd], dim=-1
        )
        return q, k, v


class MergedColumnParallelLinear(ColumnParallelLinear):
    """Two column-parallel projections fused (gate_proj|up_proj)."""

    def __init__(self, in_features: int, each_out: int, bias: bool,
                 dtype=torch.bfloat16):
        self.each_out = each_out
        super().__init__(in_features, 2 * each_out, bias, dtype)

    def shard_merged_parts(self, gate_full, up_full) -> list[torch.Tensor]:
        r = get_tp_rank()
        tp = get_tp_world_size()
        per = self.each_out // tp
        return [gate_full[r * per: (r + 1) * per],
                up_full[r * per: (r + 1) * per]]

    def shard_merged(self, gate_full: torch.Tensor, up_full: torch.Tensor) -> torch.Tensor:
        return torch.cat(self.shard_merged_parts(gate_full, up_full), dim=0)


class RowParallelLinear(nn.Module):
    """Y = sum_ranks X_shard W_shard^T, W column-sharded (input features
    split); all-reduce over the TP group after the local GEMM."""

    def __init__(self, in_features: int, out_features: int, bias: bool,
                 dtype: torch.dtype = torch.bfloat16):
        super().__init__()
        tp = get_tp_world_size()
        assert in_features % tp == 0, (in_features, tp)
        self.in_per_rank = in_features // tp
        self.weight = nn.Parameter(
            torch.empty(out_features, self.in_per_rank, dtype=dtype),
            requires_grad=False,
        )
        # bias applied once (post-reduce) on every rank identically
        self.bias = (
            nn.Parameter(torch.empty(out_features, dtype=dtype), requires_grad=False)
            if bias
            else None
        )

    def shard(self, full: torch.Tensor, param: str = "weight") -> torch.Tensor:
        if param == "bias":
            return full
        r = get_tp_rank()
        return full[:, r * self.in_per_rank : (r + 1) * self.in_per_rank]

    fp8 = False
    w4 = False
    w8 = False  # block-scaled e4m3 weights (init_module_w8)
    mx4 = False  # MXFP4 weights (init_module_mx4)
    lora: LoRAState | None = None  # set when the engine runs enable_lora

    def forward(self, x, lora_tiles=None, defer: bool = False):
        """defer=True: the caller can consume an ops.SplitKPending in place
        of the tensor. Granted only with TP world size 1, no bias and no LoRA
        delta; the all-reduce and bias paths below are otherwise unchanged."""
        if isinstance(x, tuple) or self.fp8:
            bias = self.bias
            self.bias = None  # bias must be applied post-reduce, once
            try:
                y = (_fp8_linear_prequant(self, *x) if isinstance(x, tuple)
                     else _fp8_linear(self, x))
            finally:
                self.bias = bias
        else:
            from .. import ops

            use_lora = lora_tiles is not None and self.lora is not None
            defer = (defer and not use_lora and self.bias is None
                     and get_tp_world_size() == 1)
            if self.w4:
                y = _w4_linear(self, x, None, defer)
            elif self.w8:
                y = _w8_linear(self, x, None, defer)
            elif self.mx4:
                y = _mx4_linear(self, x, None, defer)
            else:
                y = ops.linear_bf16(x, self.weight, defer=defer)
            if isinstance(y, ops.SplitKPending):
                return y  # single rank, no bias: nothing left to apply
            if use_lora:
                # the delta joins the local partial sum: linear, so the one
                # all-reduce below covers it
                self.lora.apply(y, x, lora_tiles)
        y = tp_all_reduce(y)
        if self.bias is not None:
            y = y + self.bias
        return y


class ParallelLMHead(nn.Module):
    """Vocab-sharded output projection; logits are all-gathered so every rank
    samples identically."""

    def __init__(self, hidden: int, vocab: int, dtype=torch.bfloat16):
        super().__init__()
        tp = get_tp_world_size()
        # pad vocab shard up so it divides evenly
        self.vocab = vocab
        self.vocab_padded = ((vocab + tp - 1) // tp) * tp
        self.per_rank = self.vocab_padded // tp
        self.weight = nn.Parameter(
            torch.empty(self.per_rank, hidden, dtype=dtype), requires_grad=False
        )

    def shard(self, full: torch.Tensor, param: str = "weight") -> torch.Tensor:
        r = get_tp_rank()
        lo, hi = r * self.per_rank, (r + 1) * self.per_rank
        if hi <= full.shape[0]:
            return full[lo:hi]
        pad = torch.full(
            (hi - min(hi, full.shape[0]), full.shape[1]), 0, dtype=full.dtype
        )
        return torch.cat([full[lo:], pad], dim=0)

    fp8 = False

    def forward(self, x) -> torch.Tensor:
        if isinstance(x, tuple) or self.fp8:
            self.bias = None
            logits = (_fp8_linear_prequant(self, *x) if isinstance(x, tuple)
                      else _fp8_linear(self, x))
        else:
            from .. import ops

            logits = ops.linear_bf16(x, self.weight)
        logits = tp_all_gather(logits, dim=-1)
        return logits[..., : self.vocab]
