"""Op dispatch for arks_amd.

On GPU tensors every op runs the in-tree gfx950 HIP extension
(``arks_amd._C``) — there is no eager fallback: if the extension is missing
on a CUDA/ROCm device we raise immediately so a silently-slow PyTorch path
can never masquerade as the native one. On CPU tensors ops run the plain
PyTorch reference (arks_amd/ops/ref.py) so the engine/scheduler/model layers
are unit-testable without a GPU.
"""

from __future__ import annotations

import os
from typing import Callable, NamedTuple

import torch

from . import ref

_C = None
_C_ERR: str | None = None


def _load_extension():
    global _C, _C_ERR
    if _C is not None or _C_ERR is not None:
        return _C
    try:
        from . import _load  # noqa: F401  (imports the built .so in-tree)

        _C = _load.C
    except Exception as e:  # pragma: no cover - exercised only when unbuilt
        _C_ERR = f"{type(e).__name__}: {e}"
    return _C


def native_available() -> bool:
    return _load_extension() is not None


def _native():
    c = _load_extension()
    if c is None:
        raise RuntimeError(
            "arks_amd HIP extension (arks_amd._C) is not built but a GPU op was "
            "requested. Build it with `python -m arks_amd.ops.build` "
            f"(import error: {_C_ERR})"
        )
    return c


def rmsnorm(x: torch.Tensor, weight: torch.Tensor, eps: float = 1e-6) -> torch.Tensor:
    if x.is_cuda:
        out = torch.empty_like(x)
        _native().rmsnorm(out, x, weight, eps)
        return out
    return ref.rmsnorm(x, weight, eps)


def fused_add_rmsnorm(x, residual, weight, eps: float = 1e-6):
    """In-place on GPU: residual += x (written to residual), out = norm(residual).
    x may be a SplitKPending handle: the kernel then reduces the producing
    GEMM's split-K partials itself (bit-identical to materialising first)."""
    if isinstance(x, SplitKPending):
        x.check_live()
        if tuple(residual.shape) != x.shape:
            raise ValueError(f"residual {tuple(residual.shape)} vs {x.shape}")
        out = torch.empty_like(residual)
        _native().splitk_add_rmsnorm(out, x.ws, x.bias, residual, weight, eps,
                                     x.nsplits, x.mrows)
        return out, residual
    if x.is_cuda:
        out = torch.empty_like(x)
        _native().fused_add_rmsnorm(out, x, residual, weight, eps)
        return out, residual
    return ref.fused_add_rmsnorm(x, residual, weight, eps)


def silu_mul(gate_up: torch.Tensor) -> torch.Tensor:
    if gate_up.is_cuda:
        shape = list(gate_up.shape)
        shape[-1] //= 2
        out = gate_up.new_empty(shape)
        _native().silu_mul(out, gate_up)
        return out
    return ref.silu_mul(gate_up)


def rope_apply_inplace(positions, q, k, cos_sin, head_dim: int):
    """Rotates q and k in place (GPU). CPU path returns new tensors."""
    if q.is_cuda:
        _native().rope_inplace(positions, q, k, cos_sin, head_dim)
        return q, k
    return ref.rope_apply(positions, q, k, cos_sin, head_dim)


def rope_and_cache(positions, q, k, v, k_cache, v_cache, slot_mapping,
                   cos_sin, head_dim: int):
    """Fused RoPE + paged-cache write (GPU): rotates q/k in place and
    scatters rotated k + v into the cache in one launch. CPU path runs the
    two reference steps."""
    if q.is_cuda:
        _native().rope_and_cache(positions, q, k, v, k_cache, v_cache,
                                 slot_mapping, cos_sin, head_dim)
        return q, k
    q2, k2 = ref.rope_apply(positions, q, k, cos_sin, head_dim)
    T = q.shape[0]
    nkv = k.numel() // max(T, 1) // head_dim
    ref.reshape_and_cache(
        k2.reshape(T, nkv, head_dim), v.reshape(T, nkv, head_dim),
        k_cache, v_cache, slot_mapping,
    )
    return q2, k2


# ARKS_ROPE_SPLITK_GROUPS=1 keeps the RoPE + cache consumer of the split-K
# qkv GEMM at one workgroup per token for A/B runs (0 = spread the tokens
# over the compute units); the results are bit-identical either way.
_ROPE_SPLITK_GROUPS = int(os.environ.get("ARKS_ROPE_SPLITK_GROUPS", "0"))


def _rope_splitk_groups(tokens: int, cus: int) -> int:
    """Workgroups per token of the split-K RoPE + cache consumer: enough to
    put work on every compute unit when the tokens alone do not (decode: 64
    tokens on 256 CUs run as 4 groups each). The launcher keeps a group at
    64 items or more."""
    if _ROPE_SPLITK_GROUPS > 0:
        return _ROPE_SPLITK_GROUPS
    return max(1, -(-cus // max(tokens, 1)))


def rope_and_cache_splitk(positions, qkv, k_cache, v_cache, slot_mapping,
                          cos_sin, head_dim: int, num_q_heads: int,
                          groups: int | None = None):
    """rope_and_cache for a qkv projection that is still a SplitKPending
    handle: reduces the split-K partials, rotates, writes rotated k and v
    into the paged cache and returns rotated q [T, Hq*D]. k and v are not
    materialised (the decode attention kernel reads them from the cache).
    groups = workgroups per token (default: _rope_splitk_groups)."""
    qkv.check_live()
    if qkv.shape[1] != (num_q_heads + 2 * k_cache.shape[1]) * head_dim:
        raise ValueError(f"qkv width {qkv.shape[1]} does not match the heads")
    q = torch.empty((qkv.shape[0], num_q_heads * head_dim),
                    dtype=torch.bfloat16, device=qkv.ws.device)
    if groups is None:
        groups = _rope_splitk_groups(qkv.shape[0], _cu_count(qkv.ws.device))
    _native().splitk_rope_and_cache(positions, qkv.ws, qkv.bias, q, k_cache,
                                    v_cache, slot_mapping, cos_sin, head_dim,
                                    qkv.nsplits, qkv.mrows, groups)
    return q


def reshape_and_cache(k, v, k_cache, v_cache, slot_mapping):
    if k.is_cuda:
        _native().reshape_and_cache(k, v, k_cache, v_cache, slot_mapping)
        return
    ref.reshape_and_cache(k, v, k_cache, v_cache, slot_mapping)


PREFILL_QTILE = 64  # q rows per workgroup in the prefill kernel


def build_prefill_tiles(seq_lens: list[int], device) -> torch.Tensor:
    """int32 [ntiles, 2] of (seq_idx, q0) covering every sequence in 64-row
    tiles — the prefill kernel's grid."""
    tiles = []
    for i, n in enumerate(seq_lens):
        for q0 in range(0, n, PREFILL_QTILE):
            tiles.append((i, q0))
    return torch.tensor(tiles, dtype=torch.int32, device=device).reshape(-1, 2)


def attention_prefill_varlen(q, k, v, cu_seqlens, seq_lens: list[int],
                             scale: float, window: int = 0):
    """Causal varlen prefill attention. seq_lens is the host-side list of
    per-sequence lengths (used to build the q-tile grid without a D2H sync).
    window > 0 = sliding-window attention."""
    if q.is_cuda:
        out = torch.empty_like(q)
        tile_info = build_prefill_tiles(seq_lens, q.device)
        _native().attention_prefill_varlen(out, q, k, v, cu_seqlens, tile_info,
                                           scale, window)
        return out
    return ref.attention_prefill_varlen(q, k, v, cu_seqlens, scale, window)


EXTEND2_QTILE = 256  # q rows per workgroup in the 8-wave ladder kernel
E2_KVBLK = 64        # keys per LDS tile in the ladder kernel
# Sequences with at least this many new q tokens go to the 256-row ladder
# kernel; shorter ones (decode-adjacent chunks, prefix-cache hits) stay on
# the 64-row kernel where a mostly-empty 256-row tile would waste waves.
EXTEND2_MIN_QLEN = 97


def build_extend_tiles(q_lens: list[int], kv_lens: list[int] | None,
                       kv_fp8: bool, device, num_q_heads: int = 32):
    """Per-seq routing for the extend dispatcher:
    (tiles64, tiles256 [n,4], decode_rows, combine_table, ws_rows).

    q_len == 1 sequences (decode steps mixed into a prefill batch) go to
    the flash-decode kernel — an extend q-tile for one query scans the
    full KV with 255 masked rows (~6x slower than the decode kernel's
    partitioned scan). Remaining sequences split between the 64-row and
    256-row extend kernels; tiles are sorted by DESCENDING key depth
    (causal q-tiles differ up to 4x in KV work and the dispatcher issues
    blocks in order — deep tiles first removes the straggler tail). When
    the batch is too small to fill the chip, deep 256-row tiles are
    additionally SPLIT over their KV range flash-decode-style (part rows
    + a combine pass over f32 partials); split parts sort first so the
    partial workspace only covers them. Build once per batch and reuse
    across all layers."""
    t64, t256, dec = [], [], []
    kvl = kv_lens if kv_lens is not None else q_lens
    for i, n in enumerate(q_lens):
        off = kvl[i] - n
        if n == 1:
            dec.append(i)
        elif kv_fp8 or n < EXTEND2_MIN_QLEN:
            for q0 in range(0, n, PREFILL_QTILE):
                t64.append((i, q0, min(kvl[i], off + q0 + PREFILL_QTILE)))
        else:
            for q0 in range(0, n, EXTEND2_QTILE):
                t256.append((i, q0, min(kvl[i], off + q0 + EXTEND2_QTILE)))
    t64.sort(key=lambda t: -t[2])
    t256.sort(key=lambda t: -t[2])
    mk64 = lambda t: torch.tensor(
        [x[:2] for x in t], dtype=torch.int32, device=device
    ).reshape(-1, 2)

    # KV-split policy for the 256-row kernel: when tiles x heads cannot
    # fill ~2 workgroups per CU, split the deepest tiles' key ranges.
    base_wgs = len(t256) * max(num_q_heads, 1)
    factor = 1
    if t256 and base_wgs < 256:
        # truly starved launches only (256 CUs, 1 block/CU kernel): the
        # partial slabs + combine cost ~2x slab traffic, so marginal
        # shortfalls are better left unsplit
        factor = min(8, -(-512 // base_wgs))
    rows, combine = [], []
    ws_rows = 0
    if factor > 1:
        split, plain = [], []
        for (i, q0, kmax) in t256:
            span = (kmax + E2_KVBLK - 1) // E2_KVBLK
            p = min(factor, max(1, span // 4))
            (split if p > 1 else plain).append((i, q0, p))
        # cap the f32 partial workspace at ~512 MB
        slab = num_q_heads * EXTEND2_QTILE * 130 * 4
        if sum(p for _, _, p in split) * slab > 512 * 1024 * 1024:
            split, plain = [], split + plain
        for (i, q0, p) in split:
            combine.append((len(rows), p, i, q0))
            for part in range(p):
                rows.append((i, q0, part, p))
        ws_rows = len(rows)
        for (i, q0, p) in plain:
            rows.append((i, q0, 0, 1))
    else:
        rows = [(i, q0, 0, 1) for (i, q0, _) in t256]
    t256_t = torch.tensor(rows, dtype=torch.int32,
                          device=device).reshape(-1, 4)
    ctab = torch.tensor(combine, dtype=torch.int32,
                        device=device).reshape(-1, 4)

    if dec:
        # gather indices: the single q row of each decode seq sits at
        # cu_seqlens_q[i]; seq-level metadata indexes with `dec` itself
        cu = [0]
        for n in q_lens:
            cu.append(cu[-1] + n)
        drows = torch.tensor([cu[i] for i in dec], dtype=torch.long,
                             device=device)
        dseqs = torch.tensor(dec, dtype=torch.long, device=device)
    else:
        drows = dseqs = None
    return mk64(t64), t256_t, (drows, dseqs), ctab, ws_rows


def attention_extend_paged(
    q, k_cache, v_cache, block_tables, kv_lens, cu_seqlens_q,
    q_lens: list[int], scale: float, window: int = 0, tiles=None,
):
    """Causal attention of packed NEW tokens over each sequence's full paged
    KV history (cached prefix + new tokens already written by
    reshape_and_cache). The prefix-caching / chunked-prefill attention path.
    q_lens is the host-side per-seq new-token count (tile grid without a
    D2H sync); kv_lens is the device int32 total kv length per seq.
    window > 0 = sliding-window attention.

    Dispatch: big chunks run the 8-wave 32x32-MFMA ladder kernel
    (attn_extend2.hip, 256-row q tiles); small chunks and fp8-KV runs use
    the 4-wave 64-row kernel."""
    if q.is_cuda:
        out = torch.empty(
            (q.shape[0], q.shape[1], q.shape[2]), dtype=q.dtype, device=q.device
        )
        kv_fp8 = k_cache.dtype != torch.bfloat16
        t64, t256, (drows, dseqs), ctab, ws_rows = (
            tiles if tiles is not None
            else build_extend_tiles(q_lens, None, kv_fp8, q.device,
                                    num_q_heads=q.shape[1])
        )
        if t256.numel():
            if ws_rows:
                ws = _extend_ws(
                    ws_rows * q.shape[1] * EXTEND2_QTILE * (q.shape[2] + 2),
                    q.device,
                )
            else:
                ws = q.new_empty(0, dtype=torch.float32)
            _native().attention_extend_paged2(
                out, q, k_cache, v_cache, block_tables, kv_lens, cu_seqlens_q,
                t256, ws, scale, window,
            )
            if ctab.numel():
                _native().attention_extend2_combine(
                    out, ws, ctab, cu_seqlens_q, scale,
                )
        if t64.numel():
            _native().attention_extend_paged(
                out, q, k_cache, v_cache, block_tables, kv_lens, cu_seqlens_q,
                t64, scale, window,
            )
        if drows is not None:
            dq = q[drows].contiguous()
            dout = attention_decode_paged(
                dq, k_cache, v_cache,
                block_tables[dseqs].contiguous(),
                kv_lens[dseqs].contiguous(), scale, window=window,
            )
            out[drows] = dout
        return out
    return ref.attention_extend_paged(
        q, k_cache, v_cache, block_tables, kv_lens, cu_seqlens_q, scale,
        window,
    )


def decode_num_partitions(num_seqs: int, num_kv_heads: int, max_blocks: int) -> int:
    """Flash-decode split factor: fill the 256 CUs (target ~2 workgroups/CU)
    when batch x kv_heads alone cannot. Each partition keeps >= 8 pages so
    all 4 waves of a workgroup get a 2-page chunk and the K-prefetch
    software pipeline has depth (bench_decode2: starved waves at <8
    pages/partition cap short-seq shapes)."""
    base = num_seqs * num_kv_heads
    target = 512
    nparts = max(1, -(-target // base))
    nparts = min(nparts, max(1, max_blocks // 8), 64)
    return nparts


def attention_decode_paged(
    q, k_cache, v_cache, block_tables, seq_lens, scale: float,
    num_partitions: int | None = None, part_out=None, window: int = 0,
):
    if q.is_cuda:
        out = torch.empty(
            (q.shape[0], q.shape[1], q.shape[2]), dtype=q.dtype, device=q.device
        )
        num_kv_heads = k_cache.shape[1]
        if num_partitions is None:
            num_partitions = decode_num_partitions(
                q.shape[0], num_kv_heads, block_tables.shape[1]
            )
        if num_partitions > 1 and part_out is None:
            gq = q.shape[1] // num_kv_heads
            part_out = torch.empty(
                q.shape[0] * num_kv_heads * num_partitions * gq * (q.shape[2] + 2),
                dtype=torch.float32, device=q.device,
            )
        elif part_out is None:
            part_out = q.new_empty(0, dtype=torch.float32)
        _native().attention_decode_paged(
            out, q, k_cache, v_cache, block_tables, seq_lens, scale,
            part_out, num_partitions, window,
        )
        return out
    return ref.attention_decode_paged(
        q, k_cache, v_cache, block_tables, seq_lens, scale, window
    )


_EXTEND_WS: dict = {}


def _extend_ws(need: int, device):
    key = (device.index,)
    ws = _EXTEND_WS.get(key)
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=torch.float32, device=device)
        _EXTEND_WS[key] = ws
    return ws


_SKINNY_WS: dict = {}
# Bumped every time a split-K GEMM overwrites the shared workspace of a
# device; a SplitKPending remembers the value it was created under.
_SKINNY_WS_GEN: dict = {}


class SplitKPending:
    """Result of a split-K skinny GEMM that has not been reduced yet: the
    f32 partials [nsplits, mrows, N] sit in the shared workspace and the
    consumer kernel (fused_add_rmsnorm / rope_and_cache_splitk) sums them,
    adds the bias and rounds to bf16 on the fly. materialize() runs the
    combine kernel for anything that needs the plain [M, N] tensor.

    The workspace is shared by every skinny GEMM of the device, so a handle
    is only valid until the next one runs; consuming a stale handle raises
    here, before any kernel is launched."""

    __slots__ = ("ws", "nsplits", "mrows", "shape", "bias", "_key", "_gen")

    def __init__(self, ws, nsplits, mrows, M, N, bias, key):
        self.ws = ws
        self.nsplits = nsplits
        self.mrows = mrows
        self.shape = (M, N)
        self.bias = bias
        self._key = key
        self._gen = _SKINNY_WS_GEN[key]

    def check_live(self) -> None:
        if _SKINNY_WS_GEN.get(self._key) != self._gen:
            raise RuntimeError(
                "stale split-K handle: another skinny GEMM has overwritten "
                "the shared workspace since this result was produced"
            )

    def materialize(self) -> torch.Tensor:
        self.check_live()
        out = torch.empty(self.shape, dtype=torch.bfloat16,
                          device=self.ws.device)
        _native().skinny_combine(out, self.ws, self.bias, self.nsplits,
                                 self.mrows)
        return out


def skinny_gemm(x, weight, bias=None, defer: bool = False):
    """C = x @ weight^T for decode-sized M (<=64) via the split-K streaming
    MFMA kernel. Beats hipBLASLt's ~19 us latency floor on the small
    qkv/o_proj shapes and its ~46 us in-graph down-proj algo (bench_skinny /
    bench_down logs, r2); the dispatcher keeps the wide streaming shapes
    (gate_up, lm_head: N >> K) on the tuned library algos. Deterministic
    split-K (fixed-order combine, no atomics).

    defer=True returns a SplitKPending instead of the tensor whenever the
    GEMM splits K (nsplits > 1): the caller hands it to a consumer that
    reduces the partials itself, saving the combine launch."""
    M, K = x.shape
    N = weight.shape[0]
    config, nsplits, k_per_split, mrows = _skinny_plan(M, N, K)
    config = _skinny_resident_config(config, M, nsplits, k_per_split)
    if config == 1:  # the only plan the step moves; the rest need no device
        config = _skinny_tallk7_config(config, N, nsplits,
                                       _cu_count(x.device))
    part = (_skinny_ws(nsplits, N, mrows, x.device) if nsplits > 1
            else x.new_empty(0, dtype=torch.float32))
    if defer and nsplits > 1:
        _native().skinny_gemm_partials(part, x, weight, k_per_split, nsplits,
                                       config)
        return SplitKPending(part, nsplits, mrows, M, N, bias,
                             (x.device.index,))
    out = torch.empty((M, N), dtype=x.dtype, device=x.device)
    _native().skinny_gemm(out, part, x, weight, bias, k_per_split, nsplits,
                          config)
    return out


def _skinny_plan(M: int, N: int, K: int):
    """Routing rule of the skinny GEMM: (config, nsplits, k_per_split, mrows).
    config is the kernel the extension launches (0 = default ring with MT
    from M, 1 = tall-K, 2 = tall-K with non-temporal W loads); mrows is the
    slab height of its split-K partials, 16 * MT. _skinny_resident_config
    then moves short-K split plans of config 0 to config 3, and
    _skinny_tallk7_config tall-K plans to config 4, without touching the
    other three values."""
    ntiles = N // 64
    if K > N and ntiles < 128 and M > 48:
        # tall-K (down-proj shape): few N tiles, parallelism comes from
        # K-splits; the deeper-staged AB=3 kernel at nsplits ~= 448/ntiles
        # measured fastest (34.6 us vs hipBLASLt's 46.4 in-graph, r2).
        # M-gated: that kernel is fixed at MT=4 (full 64-row cost) while
        # hipBLASLt switches to a faster algo below M~48 — routing small-M
        # down-proj here regressed b16x8k decode by 4% (r2)
        config, mt = _SKINNY_TALLK_CONFIG, 4
        nsplits = min(-(-448 // ntiles), -(-K // 256))
    else:
        config, mt = 0, min(-(-M // 16), 4)
        nsplits = 1 if ntiles >= 384 else min(-(-512 // ntiles), -(-K // 256))
    k_per_split = -(-(-(-K // nsplits)) // 32) * 32
    nsplits = -(-K // k_per_split)
    return config, nsplits, k_per_split, 16 * mt


# Longest K-range whose A slice the A-resident kernel keeps in LDS.
_SKINNY_RESIDENT_KMAX = 512
# ARKS_SKINNY_RESIDENT=0 keeps the short-K split-K GEMMs (qkv, o_proj) on
# launch config 0 for A/B runs; the partials are bit-identical either way.
_SKINNY_RESIDENT = os.environ.get("ARKS_SKINNY_RESIDENT", "1") == "1"
# Smallest M that takes it (see profiles/r07_resident_a.md).
_SKINNY_RESIDENT_MIN_M = 1


def _skinny_resident_config(config: int, M: int, nsplits: int,
                            k_per_split: int) -> int:
    """Second routing step, after _skinny_plan: a config-0 plan that splits K
    into ranges short enough for a workgroup's A slice to stay in LDS runs
    the A-resident kernel (launch config 3) at the same nsplits, k_per_split
    and slab height. Everything else, the tall-K plan included, is left as
    planned."""
    if (_SKINNY_RESIDENT and config == 0 and nsplits > 1
            and k_per_split <= _SKINNY_RESIDENT_KMAX
            and M >= _SKINNY_RESIDENT_MIN_M):
        return 3
    return config


# ARKS_SKINNY_TALLK_WAVES=8 keeps the tall-K plan on 128-row tiles (launch
# config 1) for A/B runs; the partials are bit-identical either way.
_TALLK_WAVES = os.environ.get("ARKS_SKINNY_TALLK_WAVES", "7").strip()
if _TALLK_WAVES not in ("7", "8"):
    raise ValueError(
        f"ARKS_SKINNY_TALLK_WAVES={_TALLK_WAVES!r}: accepted values are 7 "
        "(112-row tiles where they fill more CUs) and 8 (128-row tiles)"
    )


def _skinny_tallk7_config(config: int, N: int, nsplits: int, cus: int) -> int:
    """Third routing step: a tall-K plan (config 1) runs on 112-row tiles
    (launch config 4, seven waves) when those put workgroups on more of the
    device's `cus` compute units than 128-row tiles do without exceeding one
    per CU: N a multiple of 112, N/112 * nsplits <= cus, and that more than
    ceil(N/128) * nsplits. The down-proj of a 7B model (N = 3584, 8 splits)
    goes from 224 workgroups to 256. nsplits, k_per_split and the slab height
    are untouched; config 2 (non-temporal) stays as it is."""
    if _TALLK_WAVES != "7" or config != 1 or N % 112 != 0:
        return config
    wgs = N // 112 * nsplits
    if wgs <= cus and wgs > -(-N // 128) * nsplits:
        return 4
    return config


def _skinny_ws(nsplits: int, N: int, mrows: int, device):
    """The device's shared split-K workspace, grown to fit. Every call is
    about to overwrite it, so it also retires outstanding handles."""
    key = (device.index,)
    need = nsplits * N * mrows
    ws = _SKINNY_WS.get(key)
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=torch.float32, device=device)
        _SKINNY_WS[key] = ws
    _SKINNY_WS_GEN[key] = _SKINNY_WS_GEN.get(key, 0) + 1
    return ws


_USE_SKINNY = os.environ.get("ARKS_SKINNY_GEMM", "1") == "1"
# Let the consumers of a split-K skinny GEMM (fused add-RMSNorm, RoPE+cache)
# reduce its partials instead of launching the combine kernel. 0 = always
# materialise (the unfused sequence; results are bit-identical either way).
_SPLITK_FUSE = os.environ.get("ARKS_SPLITK_FUSE", "1") == "1"
# Weight-elements threshold: the split-K streaming kernel beats hipBLASLt's
# ~19 us latency floor on the small decode shapes (qkv/o: 1.0-1.6x,
# bench_skinny v3); the big streaming shapes (gate_up/down/lm_head) stay on
# the tuned hipBLASLt algos which reach 5.4-6.4 TB/s there.
_SKINNY_MAX_ELEMS = 34_000_000
# tall-K decode shapes (down-proj: K > N) stream W near-HBM-rate through the
# split-K kernel and beat the library's in-graph algo (r2); wide-N shapes
# (gate_up/lm_head) stay on hipBLASLt which reaches ~6 TB/s there.
_SKINNY_TALLK_MAX_ELEMS = 80_000_000
# ARKS_SKINNY_TALLK_V picks the tall-K kernel: 7 = AB=3 deep-staged (launch
# config 1), 8 = same + non-temporal W loads (config 2). The numbers are the
# variant ids of the r2 experiments; only these two kernels are built.
_TALLK_V = os.environ.get("ARKS_SKINNY_TALLK_V", "7").strip()
if _TALLK_V not in ("7", "8"):
    raise ValueError(
        f"ARKS_SKINNY_TALLK_V={_TALLK_V!r}: accepted values are 7 (tall-K "
        "kernel) and 8 (tall-K kernel with non-temporal W loads)"
    )
_SKINNY_TALLK_CONFIG = {"7": 1, "8": 2}[_TALLK_V]


def linear_bf16(x, weight, bias=None, defer: bool = False):
    """Linear dispatch: the skinny split-K kernel for small decode-shaped
    GEMMs on GPU, hipBLASLt (F.linear) otherwise. defer=True lets the skinny
    path return a SplitKPending (see skinny_gemm); every other path returns
    the tensor as usual, so callers must accept both."""
    if (
        _USE_SKINNY
        and x.is_cuda
        and x.dim() == 2
        and 1 <= x.shape[0] <= 64
        and x.dtype == torch.bfloat16
        and weight.shape[0] % 64 == 0
        and weight.shape[1] % 32 == 0
        and (weight.numel() <= _SKINNY_MAX_ELEMS
             or (weight.shape[1] > weight.shape[0]
                 and x.shape[0] > 48
                 and weight.numel() <= _SKINNY_TALLK_MAX_ELEMS))
        and weight.is_contiguous()
        and native_available()
    ):
        return skinny_gemm(x, weight, bias, defer=defer and _SPLITK_FUSE)
    import torch.nn.functional as F

    return F.linear(x, weight, bias)


# ---------------------------------------------------------------------------
# Quantized weights, group / block size 128 along K (formats in ops/ref.py):
#   W4A16  4-bit AWQ-style, packed (qweight, scales, zeros)
#   W8A16  block-scaled e4m3fn, (w8_weight [N, K], w8_scales f32 [K/128, N])
#   MX4    OCP MXFP4 (W4A16): e2m1 nibbles with one e8m0 scale per 32 k,
#          (mx4_weight u8 [N, K/2], mx4_scales u8 [N, K/32]); a 128-wide
#          chunk holds four of its blocks, one per lane group
# All run the streaming chunk loop of csrc/wq_stream.h, so one path serves
# them, driven by a format descriptor.
# ---------------------------------------------------------------------------
# Rows one launch of the shared skinny kernel takes (MT <= 4 tiles of 16).
W4_SKINNY_MAX_M = W8_SKINNY_MAX_M = _WQ_SKINNY_MAX_M = 64
# 64 < M <= this: the skinny kernel once per 64-row slab; above it the
# weight is dequantized into the workspace for the library GEMM. Measured
# separately per format: crossovers and numbers in w4_linear's and
# w8_linear's docstrings (W8: the M = 96 / 128 / 256 rows of
# profiles/w8_gemm.md).
W4_SLAB_MAX_M = 128
W8_SLAB_MAX_M = 128
# MX4 starts from the W8 value: it moves only on a measurement recorded in
# profiles/mx4_gemm.md.
MX4_SLAB_MAX_M = W8_SLAB_MAX_M
# bf16 [N*K] scratch per device for the path above the slab limit
# (dequantize, then the library GEMM): a model is W4 or W8, never both at
# once, and either way the scratch is one bf16 [N*K] of its largest layer.
# Reserved when a layer is quantized and never grown inside w4_linear /
# w8_linear, so the pointer captured into decode graphs stays valid.
_DEQUANT_WS: dict = {}


def reserve_dequant_workspace(numel: int, device) -> None:
    """Make the device's dequant workspace hold at least `numel` bf16
    elements (the largest quantized layer). Call before capturing graphs."""
    device = torch.device(device)
    if device.type != "cuda":
        return
    key = (device.index if device.index is not None
           else torch.cuda.current_device(),)
    ws = _DEQUANT_WS.get(key)
    if ws is None or ws.numel() < numel:
        _DEQUANT_WS[key] = torch.empty(numel, dtype=torch.bfloat16,
                                       device=device)


class _WqFormat(NamedTuple):
    """What the shared path needs to know about a weight format. The native
    entry points are {name}_skinny_gemm, {name}_skinny_gemm_partials and
    {name}_dequant, each taking the weight's tensors in place of one."""
    name: str
    shape: Callable        # weight tuple -> (N, K)
    ref_linear: Callable   # CPU reference: (x, weight tuple, bias) -> y
    ref_dequant: Callable  # CPU reference: weight tuple -> f32 [N, K]
    slab_max_m: int        # W4_SLAB_MAX_M / W8_SLAB_MAX_M


_W4 = _WqFormat(
    "w4", lambda w: (w[0].shape[0], w[0].shape[1] * 8), ref.w4_linear,
    lambda w: ref.w4_dequant(*ref.w4_unpack(w)), W4_SLAB_MAX_M)
_W8 = _WqFormat(
    "w8", lambda w: tuple(w[0].shape),
    lambda x, w, bias: ref.w8_linear(x, *w, bias),
    lambda w: ref.w8_dequant(*w), W8_SLAB_MAX_M)
_MX4 = _WqFormat(
    "mx4", lambda w: (w[0].shape[0], w[0].shape[1] * 2),
    lambda x, w, bias: ref.mx4_linear(x, *w, bias),
    lambda w: ref.mx4_dequant(*w), MX4_SLAB_MAX_M)


def _wq_plan(M: int, N: int, K: int):
    """Routing rule of the W4 and W8 skinny GEMMs: (nw, nsplits, k_per_split,
    mrows). nw = 64-row N sub-tiles per workgroup, mrows = 16 * MT the slab
    height of the split-K partials, k_per_split a multiple of the 128 group /
    scale block.

    MEASURED for W4 on an MI355X (in-graph, weights cycled past the LLC;
    sweep over nw x nsplits at M = 1/16/32/64 on the Qwen2.5-7B shapes,
    tables in profiles/w4_gemm.md):
    - nw = 2 pays only above M = 32, where the activation re-read per tile
      outweighs the halved workgroup count (down-proj M=64: 27.8 us vs 30.6;
      M=16: 19.5 vs 17.5; qkv/o/gate_up within 0.6 us of each other at 32).
    - K-splits: fastest around 800 workgroups at nw = 1 and 450 at nw = 2,
      with at least 4 chunks (512 k) per split: qkv/o 7 splits (M=64 16 us vs
      32-38 unsplit), down-proj 14-15 (28 us vs 150-180 unsplit).
    - once the N tiles alone reach 256 workgroups a split's partials cost
      more than they hide (gate_up at nw=1, M=16: 26.4 us unsplit, 32.4 with
      2 splits, 28.8 with 3; at M=64/nw=2 3 splits would gain 7%).

    The W8 kernel shares the W4 kernel's staging, grid and partial layout, so
    it takes the W4 rule; it was not swept again cell by cell for W8.
    MEASURED as a whole on an MI355X with scripts/bench_w8.py (in-graph,
    weights cycled past the LLC; profiles/w8_gemm.md): with this plan every
    M <= 64 row of the Qwen2.5-7B shapes beats bf16 (qkv 10.1-16.5 us vs
    14.1-19.3, o 9.9-14.7 vs 12.1-15.9, gate_up 34.0-51.7 vs 56.8-63.1, down
    22.3-29.5 vs 42.4-110.9), gate_up unsplit at 4.1 TB/s of weight bytes
    at M = 1."""
    nw = 2 if (M > 32 and N % 128 == 0) else 1
    ntiles = N // (64 * nw)
    chunks = K // 128
    if ntiles >= 256:
        nsplits = 1
    else:
        target = 800 if nw == 1 else 448
        nsplits = max(1, min(-(-target // ntiles), chunks // 4))
    k_per_split = -(-chunks // nsplits) * 128
    nsplits = -(-K // k_per_split)
    return nw, nsplits, k_per_split, 16 * min(-(-M // 16), 4)


_w4_plan = _w8_plan = _mx4_plan = _wq_plan


def _wq_dequant(fmt: _WqFormat, weight, out=None):
    N, K = fmt.shape(weight)
    if not weight[0].is_cuda:
        return fmt.ref_dequant(weight).to(torch.bfloat16)
    if out is None:
        out = torch.empty(N * K, dtype=torch.bfloat16,
                          device=weight[0].device)
    getattr(_native(), fmt.name + "_dequant")(out, *weight)
    return out[: N * K].view(N, K)


def w4_dequant(packed, out=None):
    """bf16 [N, K] from a packed W4 weight, via w4_dequant_kernel on GPU."""
    return _wq_dequant(_W4, packed, out)


def w8_dequant(weight, out=None):
    """bf16 [N, K] from a W8 weight (w8_weight, w8_scales), via
    w8_dequant_kernel on GPU."""
    return _wq_dequant(_W8, weight, out)


def mx4_dequant(weight, out=None):
    """bf16 [N, K] from an MX4 weight (mx4_weight, mx4_scales), via
    mx4_dequant_kernel on GPU. Exact: every e2m1 value times a power of two
    is a bf16 for the scale bytes a layer accepts."""
    return _wq_dequant(_MX4, weight, out)


def _wq_skinny(fmt: _WqFormat, x, weight, bias, defer: bool, plan, out=None):
    """One launch of the format's skinny kernel for M <= 64 rows (plus the
    combine when it splits K and the result is not deferred)."""
    M, K = x.shape
    N = fmt.shape(weight)[0]
    if x.stride(1) != 1 or x.stride(0) % 8 != 0 or x.data_ptr() % 16 != 0:
        x = x.contiguous()
    nw, nsplits, k_per_split, mrows = plan or _wq_plan(M, N, K)
    part = (_skinny_ws(nsplits, N, mrows, x.device) if nsplits > 1
            else x.new_empty(0, dtype=torch.float32))
    if defer and nsplits > 1 and _SPLITK_FUSE:
        getattr(_native(), fmt.name + "_skinny_gemm_partials")(
            part, x, *weight, k_per_split, nsplits, nw)
        return SplitKPending(part, nsplits, mrows, M, N, bias,
                             (x.device.index,))
    if out is None:
        out = torch.empty((M, N), dtype=x.dtype, device=x.device)
    getattr(_native(), fmt.name + "_skinny_gemm")(
        out, part, x, *weight, bias, k_per_split, nsplits, nw)
    return out


def _wq_slabs(fmt: _WqFormat, x, weight, bias):
    """M > 64 through the skinny kernel, 64 rows at a time, each slab
    written straight into its rows of the output."""
    M = x.shape[0]
    out = torch.empty((M, fmt.shape(weight)[0]), dtype=x.dtype,
                      device=x.device)
    for r in range(0, M, _WQ_SKINNY_MAX_M):
        _wq_skinny(fmt, x[r:r + _WQ_SKINNY_MAX_M], weight, bias, False, None,
                   out=out[r:r + _WQ_SKINNY_MAX_M])
    return out


def _wq_dequant_linear(fmt: _WqFormat, x, weight, bias):
    """M above the slab limit through the library GEMM on the weight
    expanded to bf16 in the device's reserved dequant workspace."""
    N, K = fmt.shape(weight)
    ws = _DEQUANT_WS.get((x.device.index,))
    if ws is None or ws.numel() < N * K:
        raise RuntimeError(
            f"dequant workspace missing or smaller than {N}x{K}: "
            "call ops.reserve_dequant_workspace when the layer is quantized"
        )
    import torch.nn.functional as F

    return F.linear(x, _wq_dequant(fmt, weight, ws), bias)


def _wq_linear(fmt: _WqFormat, x, weight, bias, defer: bool, plan):
    if not x.is_cuda:
        return fmt.ref_linear(x, weight, bias)
    if x.dim() != 2 or x.dtype != torch.bfloat16:
        raise ValueError(f"{fmt.name}_linear needs a 2-D bf16 input, got "
                         f"{tuple(x.shape)} {x.dtype}")
    M, K = x.shape
    N, wk = fmt.shape(weight)
    if wk != K:
        raise ValueError(f"{fmt.name}_linear: x has K={K}, weight K={wk}")
    if M == 0:
        return x.new_empty((0, N))
    if M <= _WQ_SKINNY_MAX_M:
        return _wq_skinny(fmt, x, weight, bias, defer, plan)
    if M <= fmt.slab_max_m:
        return _wq_slabs(fmt, x, weight, bias)
    return _wq_dequant_linear(fmt, x, weight, bias)


def w4_linear(x, packed, bias=None, defer: bool = False, plan=None):
    """y = x @ dequant(packed)^T + bias for a packed W4 weight
    (qweight, scales, zeros). On GPU: the W4 streaming kernel for M <= 64
    (defer=True returns a SplitKPending when it splits K, as skinny_gemm
    does); M up to W4_SLAB_MAX_M runs that kernel per 64-row slab; above it
    the weight is expanded to bf16 in the preallocated workspace and the
    library GEMM runs on it. No eager fallback: a shape the kernels cannot
    take raises. On CPU: the reference emulation.
    plan overrides _w4_plan for M <= 64 (tests force a split count with it).

    M > 64 crossover, MEASURED with scripts/bench_w4.py on an MI355X
    (in-graph us, slabs vs dequant+library; profiles/w4_gemm.md):
    M=128: qkv 31.0 vs 37.0, o 28.2 vs 34.2, gate_up 100 vs 151, down 55 vs
    109 — slabs win everywhere. M=256: qkv 61.6 vs 47.9, o 55.4 vs 30.5,
    gate_up 197 vs 157 — the library GEMM wins (down alone still favours
    slabs, 108 vs 138). 192 was not measured; the threshold sits at the last
    size where slabs were seen to win. Above M = 64 bf16 weights are faster
    than either route on qkv/o/gate_up (23 / 23 / 70 us at 128): int4 trades
    large-batch and prefill speed for decode speed and memory."""
    return _wq_linear(_W4, x, packed, bias, defer, plan)


def w8_linear(x, weight, bias=None, defer: bool = False, plan=None):
    """y = x @ dequant(weight)^T + bias for a W8 weight (w8_weight e4m3fn
    [N, K], w8_scales f32 [K/128, N]). On GPU: the W8 streaming kernel for
    M <= 64 (defer=True returns a SplitKPending when it splits K, as
    skinny_gemm does); M up to W8_SLAB_MAX_M runs that kernel per 64-row
    slab; above it the weight is expanded to bf16 in the preallocated
    workspace and the library GEMM runs on it. No eager fallback: a shape the
    kernels cannot take raises. On CPU: the reference emulation.
    plan overrides _w8_plan for M <= 64 (tests force a split count with it).

    M > 64 crossover, MEASURED with scripts/bench_w8.py on an MI355X
    (in-graph us, slabs vs dequant+library; profiles/w8_gemm.md):
    M=96: qkv 25.9 vs 32.1, o 24.3 vs 30.9, gate_up 85.5 vs 147, down 52.1
    vs 102; M=128: qkv 31.3 vs 33.7, o 28.3 vs 32.4, gate_up 96.5 vs 151,
    down 55.0 vs 110 — slabs win everywhere. M=256: qkv 61.4 vs 45.3, o 55.6
    vs 28.8, gate_up 181 vs 156 — the library GEMM wins (down alone still
    favours slabs, 106 vs 140). 192 was not measured; W8_SLAB_MAX_M sits at
    the last size where slabs were seen to win. Above M = 64 bf16 weights are
    faster than either route on qkv/o/gate_up (23 / 23 / 70 us at 128); down
    stays faster in W8 up to 128 rows."""
    return _wq_linear(_W8, x, weight, bias, defer, plan)


def mx4_linear(x, weight, bias=None, defer: bool = False, plan=None):
    """y = x @ dequant(weight)^T + bias for an MX4 weight (mx4_weight u8
    [N, K/2] of e2m1 nibble pairs, mx4_scales u8 [N, K/32] e8m0; the
    tensors of an MXFP4 checkpoint). On GPU: the MX4 streaming kernel for
    M <= 64 (defer=True returns a SplitKPending when it splits K, as
    skinny_gemm does); M up to MX4_SLAB_MAX_M runs that kernel per 64-row
    slab; above it the weight is expanded to bf16 in the preallocated
    workspace and the library GEMM runs on it. No eager fallback: a shape the
    kernels cannot take (N % 64, K % 128) raises. On CPU: the reference
    emulation.
    plan overrides _mx4_plan for M <= 64 (tests force a split count with it).

    _mx4_plan is _wq_plan: the kernel shares the W4 and W8 kernels' staging,
    grid and partial layout, so it takes their rule; the plan was not swept
    again for MX4. MEASURED as a whole on an MI355X with scripts/bench_mx4.py
    (in-graph us, weights cycled past the LLC; profiles/mx4_gemm.md): with
    this plan every M <= 64 row of the Qwen2.5-7B shapes beats bf16 (qkv
    8.9-15.3 vs 11.2-16.8, o 8.6-13.7 vs 10.6-15.1, gate_up 28.8-47.8 vs
    55.8-63.0, down 21.0-27.9 vs 34.3-111); against w4_linear in the same
    session it is within 4% on qkv / o, 4-9% faster at M = 64, and 10-23%
    SLOWER on gate_up / down at M <= 32 (cause not established).
    M > 64: slabs vs dequant+library at M=128: qkv 29.8 vs 37.9, o 26.7 vs
    36.6, gate_up 85.2 vs 165.5, down 52.1 vs 118.9 — slabs win everywhere;
    M=256: qkv 59.0 vs 49.1, o 53.1 vs 33.7 — the library wins; gate_up 160.6
    vs 172.5, down 101.1 vs 148.4 — slabs win. MX4_SLAB_MAX_M stays at the W8
    value, the last measured size where slabs win on every shape."""
    return _wq_linear(_MX4, x, weight, bias, defer, plan)


def w4_moe_gemm(a, packed, counts, pairs, src_div: int, max_rows: int,
                out=None):
    """Routed grouped W4A16 GEMM over the stacked local experts of an MoE
    block (w4_moe_gemm_kernel): for every local expert e and every
    p in pairs[e][:counts[e]], out[p] = a[p // src_div] @ dequant(W[e])^T.
    packed = (qweight [E, N, K/8], scales [E, K/128, N], zeros [E, K/128, N]);
    counts, pairs come from moe_route. src_div = k gathers token rows for the
    w13 GEMM (a = hidden states [T, K]), src_div = 1 reads a = h [T*k, K].
    max_rows bounds the longest expert list (T is always enough); the launch
    shape depends on it and on the weight's shape only, so with max_rows = T
    the call is hipGraph-capturable. Rows of `out` [T*k, N] that belong to no
    local expert are not written. `out` and everything else allocated here
    come from the caching allocator, i.e. from the graph's own pool under
    capture, so no pointer a captured graph holds is ever reallocated.
    No eager fallback on GPU: a shape the kernel cannot take raises."""
    if not a.is_cuda:
        return ref.w4_moe_gemm(a, packed, counts, pairs, src_div, out=out)
    qweight, scales, zeros = packed
    T = pairs.shape[1] if pairs.dim() == 2 else 0
    top_k = a.shape[0] * src_div // max(T, 1)
    if out is None:
        out = torch.empty((T * top_k, qweight.shape[1]), dtype=a.dtype,
                          device=a.device)
    if not a.is_contiguous() or a.data_ptr() % 16 != 0:
        a = a.contiguous()
    _native().w4_moe_gemm(out, a, qweight, scales, zeros, counts, pairs,
                          top_k, src_div, max_rows)
    return out


def w8_moe_gemm(a, weight, counts, pairs, src_div: int, max_rows: int,
                out=None):
    """Routed grouped W8A16 GEMM over the stacked local experts of an MoE
    block (w8_moe_gemm_kernel): w4_moe_gemm for weight = (w8 e4m3fn
    [E, N, K], scales f32 [E, K/128, N]), the checkpoint's bytes and its
    block scales expanded per output row:
    out[p] = a[p // src_div] @ (float(w8[e]) * scales[e])^T for every local
    expert e and p in pairs[e][:counts[e]]. Same arguments, same capture
    rules, and no eager fallback on GPU either."""
    if not a.is_cuda:
        return ref.w8_moe_gemm(a, weight, counts, pairs, src_div, out=out)
    w8, scales = weight
    T = pairs.shape[1] if pairs.dim() == 2 else 0
    top_k = a.shape[0] * src_div // max(T, 1)
    if out is None:
        out = torch.empty((T * top_k, w8.shape[1]), dtype=a.dtype,
                          device=a.device)
    if not a.is_contiguous() or a.data_ptr() % 16 != 0:
        a = a.contiguous()
    _native().w8_moe_gemm(out, a, w8, scales, counts, pairs, top_k, src_div,
                          max_rows)
    return out


def rmsnorm_fp8(x, weight, eps: float = 1e-6):
    """Fused RMSNorm -> per-token fp8 e4m3: (out8, inv_scale). GPU-only
    fast path (hidden <= 8192); otherwise compose the unfused ops."""
    if x.is_cuda and x.shape[-1] <= 8192:
        out = torch.empty(x.shape, dtype=torch.float8_e4m3fn, device=x.device)
        inv_scale = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
        _native().rmsnorm_fp8(out, inv_scale, x, None, weight, eps)
        return out, inv_scale
    return quant_fp8_rows(rmsnorm(x, weight, eps))


def fused_add_rmsnorm_fp8(x, residual, weight, eps: float = 1e-6):
    """Fused residual-add + RMSNorm -> fp8: (out8, inv_scale, residual)."""
    if x.is_cuda and x.shape[-1] <= 8192:
        out = torch.empty(x.shape, dtype=torch.float8_e4m3fn, device=x.device)
        inv_scale = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
        _native().rmsnorm_fp8(out, inv_scale, x, residual, weight, eps)
        return out, inv_scale, residual
    y, res = fused_add_rmsnorm(x, residual, weight, eps)
    q, s = quant_fp8_rows(y)
    return q, s, res


def silu_mul_fp8(gate_up):
    """Fused SwiGLU -> per-token fp8: (out8, inv_scale)."""
    d = gate_up.shape[-1] // 2
    # dynamic-LDS default cap is 64 KiB; stay under it (d*2 bytes staged)
    if gate_up.is_cuda and d % 8 == 0 and d * 2 <= 60 * 1024:
        out = torch.empty((gate_up.shape[0], d), dtype=torch.float8_e4m3fn,
                          device=gate_up.device)
        inv_scale = torch.empty(gate_up.shape[0], dtype=torch.float32,
                                device=gate_up.device)
        _native().silu_mul_fp8(out, inv_scale, gate_up.contiguous())
        return out, inv_scale
    return quant_fp8_rows(silu_mul(gate_up))


def quant_fp8_rows(x):
    """Dynamic per-token fp8 e4m3 quantization: [M, K] bf16 ->
    ([M, K] float8_e4m3fn, [M] fp32 dequant scales) for W8A8 GEMMs
    (torch._scaled_mm rowwise)."""
    if x.is_cuda:
        out = torch.empty(x.shape, dtype=torch.float8_e4m3fn, device=x.device)
        inv_scale = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
        _native().quant_fp8_rows(out, inv_scale, x.contiguous())
        return out, inv_scale
    return ref.quant_fp8_rows(x)


LORA_TILE_ROWS = 16  # token rows per LoRA tile (one MFMA M tile)


def build_lora_tiles(q_lens: list[int], slots: list[int],
                     device=None) -> torch.Tensor:
    """int32 [ntiles, 3] of (row0, nrows, slot) for the LoRA kernels: runs of
    consecutive packed rows on one adapter slot, cut into tiles of at most 16
    rows. Neighbouring sequences on the same slot share tiles; rows of
    slot -1 (base-model requests) are covered by no tile. Build once per
    batch and reuse across all layers."""
    tiles: list[tuple[int, int, int]] = []
    row = 0
    run_start, run_slot = 0, -1
    for n, slot in list(zip(q_lens, slots)) + [(0, -2)]:
        if slot != run_slot:
            if run_slot >= 0:
                for r0 in range(run_start, row, LORA_TILE_ROWS):
                    tiles.append((r0, min(LORA_TILE_ROWS, row - r0), run_slot))
            run_start, run_slot = row, slot
        row += n
    return torch.tensor(tiles, dtype=torch.int32, device=device).reshape(-1, 3)


def lora_shrink(h, x, A, tiles) -> None:
    """h[row] = x[row] . A[slot]^T into the caller's f32 workspace."""
    if x.is_cuda:
        _native().lora_shrink(h, x, A, tiles)
        return
    ref.lora_shrink(h, x, A, tiles)


def lora_expand(y, h, B, tiles, slice_offsets) -> None:
    """y[row, n] += h[row, slice(n)] . B[slot][n] in place."""
    if y.is_cuda:
        _native().lora_expand(y, h, B, tiles, list(slice_offsets))
        return
    ref.lora_expand(y, h, B, tiles, slice_offsets)


def lora_apply(y, x, A, B, tiles, slice_offsets, h_ws) -> None:
    """y[t] += B[a(t)] . (A[a(t)] . x[t]) for the rows covered by `tiles`
    (shrink into the f32 workspace h_ws [>=T, S*R], then expand into y in
    place). Allocates and synchronises nothing: safe under graph capture."""
    if h_ws.shape[0] < x.shape[0]:
        raise ValueError(
            f"LoRA workspace holds {h_ws.shape[0]} rows, batch has {x.shape[0]}"
        )
    lora_shrink(h_ws, x, A, tiles)
    lora_expand(y, h_ws, B, tiles, slice_offsets)


def moe_topk(router_logits, k: int, renorm: bool):
    """softmax + top-k + optional renorm in one kernel:
    (weights [T,k] f32, ids [T,k] i32). torch.topk tie-breaking (lower
    expert id wins)."""
    if router_logits.is_cuda:
        T = router_logits.shape[0]
        weights = torch.empty(T, k, dtype=torch.float32,
                              device=router_logits.device)
        ids = torch.empty(T, k, dtype=torch.int32,
                          device=router_logits.device)
        _native().moe_topk(weights, ids, router_logits.contiguous(), k,
                           1 if renorm else 0)
        return weights, ids
    return ref.moe_topk(router_logits, k, renorm)


def moe_route(ids, expert_base: int, n_local: int):
    """Routing table of the W4 expert GEMM from moe_topk's ids [T, k]:
    (counts int32 [n_local], pairs int32 [n_local, T]); local expert e's
    first counts[e] entries of pairs[e] are the pair indices p = t*k + j
    routed to it, ascending (the rest is unspecified). One launch, no atomics
    and no host sync, so it is hipGraph-capturable."""
    if not ids.is_cuda:
        return ref.moe_route(ids, expert_base, n_local)
    T = ids.shape[0]
    counts = torch.empty(n_local, dtype=torch.int32, device=ids.device)
    pairs = torch.empty(n_local, T, dtype=torch.int32, device=ids.device)
    _native().moe_route(counts, pairs, ids.contiguous(), expert_base)
    return counts, pairs


def moe_mix(y, weights, ids, expert_base: int = 0):
    """out[t] = sum_i weights[t,i] * y[ids[t,i]-expert_base, t] with
    out-of-slice experts contributing 0 (TP expert parallelism)."""
    if y.is_cuda:
        El, T, H = y.shape
        out = torch.empty(T, H, dtype=y.dtype, device=y.device)
        _native().moe_mix(out, y.contiguous(), weights, ids, expert_base, El)
        return out
    return ref.moe_mix(y, weights, ids, expert_base)


def moe_mix_rows(y, weights, rows):
    """out[t] = sum_j weights[t,j] * y[rows[t,j]] — the gather-side mix
    over a flat per-pair expert-output buffer (zero-weight slots point at
    row 0)."""
    if y.is_cuda:
        T, k = weights.shape
        out = torch.empty(T, y.shape[1], dtype=y.dtype, device=y.device)
        _native().moe_mix_rows(out, y.contiguous(), weights, rows)
        return out
    return ref.moe_mix_rows(y, weights, rows)


_CU_COUNT: dict = {}


def _cu_count(device) -> int:
    """Compute units of a GPU, queried once per device."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    n = _CU_COUNT.get(idx)
    if n is None:
        n = _CU_COUNT[idx] = torch.cuda.get_device_properties(idx).multi_processor_count
    return n


# Shortest vocabulary chunk a sampling workgroup is given (one trip of its
# 256 threads x 8 tokens), and the workgroups per CU the chunking aims for.
_SAMPLE_MIN_CHUNK = 2048
_SAMPLE_WGS_PER_CU = 4


def _sample_chunks(rows: int, vocab: int, cus: int) -> int:
    """Workgroups per row of the unmasked samplers. The kernels scan a row
    with one workgroup; below one row per CU most of the chip would idle
    (decode: 64 rows of 152k logits on 256 CUs), so a row is cut into chunks,
    about _SAMPLE_WGS_PER_CU workgroups per CU in all, none shorter than
    _SAMPLE_MIN_CHUNK. The ids do not depend on the count."""
    if rows >= cus:
        return 1
    want = -(-_SAMPLE_WGS_PER_CU * cus // max(rows, 1))
    return max(1, min(want, vocab // _SAMPLE_MIN_CHUNK))


def _sample_launch(fn, logits, args, chunks):
    rows, vocab = logits.shape
    if chunks is None:
        chunks = _sample_chunks(rows, vocab, _cu_count(logits.device))
    out = torch.empty(rows, dtype=torch.int64, device=logits.device)
    pairs = (torch.empty((rows, chunks, 2), dtype=torch.int32,
                         device=logits.device) if chunks > 1 else None)
    fn(out, logits, *args, pairs, chunks)
    return out


def sample_tokens(logits, temperatures, uniform, chunks=None):
    """Gumbel-max categorical sampling; rows with temperature 0 are greedy.
    chunks forces the workgroups per row (default: _sample_chunks)."""
    if logits.is_cuda:
        return _sample_launch(_native().gumbel_sample, logits,
                              (temperatures, uniform), chunks)
    return ref.gumbel_sample(logits, temperatures, uniform)


def greedy_sample(logits, chunks=None):
    """Argmax per row, lowest index on ties. chunks forces the workgroups
    per row (default: _sample_chunks)."""
    if logits.is_cuda:
        return _sample_launch(_native().greedy_sample, logits, (), chunks)
    return ref.greedy_sample(logits)


def greedy_sample_masked(logits, masks, mask_row):
    """Argmax over the tokens whose bit is set in masks[mask_row[r]]
    (mask_row -1 = unconstrained row); -1 for a row with no bit set."""
    if logits.is_cuda:
        out = torch.empty(logits.shape[0], dtype=torch.int64, device=logits.device)
        _native().greedy_sample_masked(out, logits, masks, mask_row)
        return out
    return ref.greedy_sample_masked(logits, masks, mask_row)


def sample_tokens_masked(logits, temperatures, uniform, masks, mask_row):
    """Gumbel-max sampling restricted to each row's allowed tokens."""
    if logits.is_cuda:
        out = torch.empty(logits.shape[0], dtype=torch.int64, device=logits.device)
        _native().gumbel_sample_masked(out, logits, temperatures, uniform,
                                       masks, mask_row)
        return out
    return ref.gumbel_sample_masked(logits, temperatures, uniform, masks,
                                    mask_row)


gumbel_sample_masked = sample_tokens_masked


def apply_token_bitmask(logits, masks, mask_row):
    """In place: logits[r, t] = -inf where token t's bit is clear in
    masks[mask_row[r]]; rows with mask_row -1 are left alone."""
    if logits.is_cuda:
        _native().apply_token_bitmask(logits, masks, mask_row)
        return logits
    return ref.apply_token_bitmask(logits, masks, mask_row)


# ---------------------------------------------------------------------------
# Embedding pooling (pooling.hip; definition in ref.pool_embed)
# ---------------------------------------------------------------------------
POOL_MODES = {"last": ref.POOL_LAST, "mean": ref.POOL_MEAN,
              "cls": ref.POOL_CLS}
POOL_SLAB_ROWS = 32  # rows per workgroup of the mean kernel (pooling.hip)
_POOL_WS: dict = {}


class PoolTable:
    """Work table of one pool_embed call: the host list of segments, and on
    GPU the int32 segment table [S, 8] (row0, nrows, mode, slot, counted,
    final, first slab, slab count) with the slab table [NS, 4] (row0, nrows,
    partial row, 0) that cuts every mean segment into POOL_SLAB_ROWS-row
    slabs at fixed offsets from its first row."""

    __slots__ = ("segments", "segs", "slabs", "max_row", "max_slot")

    def __init__(self, segments, segs, slabs, max_row, max_slot):
        self.segments = segments
        self.segs = segs
        self.slabs = slabs
        self.max_row = max_row
        self.max_slot = max_slot

    def __len__(self) -> int:
        return len(self.segments)


def build_pool_table(segments, device=None) -> PoolTable:
    """Segment table for pool_embed from (row0, nrows, mode, slot, counted,
    final) entries; mode is "last" / "mean" / "cls". slot is the row of the
    fp32 carry a mean-pooled sequence accumulates in across prefill chunks
    (-1 when it needs none: a single final chunk), counted the tokens pooled
    by its earlier chunks. Packed rows covered by no entry are never read.
    Build once per batch, on the host, like build_lora_tiles."""
    host, segs, slabs = [], [], []
    max_row, max_slot, used = 0, -1, set()
    for row0, nrows, mode, slot, counted, final in segments:
        m = POOL_MODES[mode] if isinstance(mode, str) else int(mode)
        if m not in (ref.POOL_LAST, ref.POOL_MEAN, ref.POOL_CLS):
            raise ValueError(f"unknown pooling mode {mode!r}")
        if row0 < 0 or nrows < 1 or counted < 0:
            raise ValueError(f"bad pooling segment {(row0, nrows, counted)}")
        final = 1 if final else 0
        part0 = len(slabs)
        if m == ref.POOL_MEAN:
            if counted > 0 or not final:
                if slot < 0 or slot in used:
                    raise ValueError(
                        f"mean segment needs its own carry slot, got {slot}")
                used.add(slot)
                max_slot = max(max_slot, slot)
            for r in range(0, nrows, POOL_SLAB_ROWS):
                slabs.append((row0 + r, min(POOL_SLAB_ROWS, nrows - r),
                              len(slabs), 0))
        elif counted or not final:
            raise ValueError("last/cls segments are single final chunks")
        max_row = max(max_row, row0 + nrows)
        host.append((row0, nrows, m, slot, counted, final))
        segs.append((row0, nrows, m, slot, counted, final, part0,
                     len(slabs) - part0))
    dev = torch.device(device) if device is not None else None
    if dev is None or dev.type != "cuda":
        return PoolTable(host, None, None, max_row, max_slot)
    # one H2D copy for both tables
    flat = torch.tensor([v for e in segs for v in e]
                        + [v for e in slabs for v in e],
                        dtype=torch.int32).to(dev)
    n = len(segs) * 8
    return PoolTable(host, flat[:n].view(-1, 8), flat[n:].view(-1, 4),
                     max_row, max_slot)


def pool_embed(x, residual, weight, eps: float, table: PoolTable, carry=None,
               dims: int | None = None, normalize: bool = True):
    """Final-norm + pooling + truncation + L2 normalisation of the decoder
    stack's (x, residual) output, packed rows [T, H]: fp32
    [num_segments, dims], one vector per entry of `table` (a non-final mean
    chunk's row is zero; it only updates carry [slots, H] fp32 in place).
    x and residual are not modified. x may be a SplitKPending (small
    prefills take the skinny split-K path): it is materialised first.
    Native on GPU, no fallback; ref.pool_embed on CPU."""
    if isinstance(x, SplitKPending):
        x = x.materialize()
    T, H = x.shape
    if tuple(residual.shape) != (T, H):
        raise ValueError(f"residual {tuple(residual.shape)} vs x {(T, H)}")
    if H % 8 != 0:
        raise ValueError(f"pool_embed requires H % 8 == 0, got {H}")
    dims = H if dims is None else int(dims)
    if not 1 <= dims <= H:
        raise ValueError(f"dims must be in [1, {H}], got {dims}")
    if len(table) == 0:
        raise ValueError("empty pooling table")
    if table.max_row > T:
        raise ValueError(f"pooling table covers row {table.max_row}, batch "
                         f"has {T}")
    if table.max_slot >= 0 and (carry is None
                                or table.max_slot >= carry.shape[0]
                                or carry.shape[1] != H):
        raise ValueError(f"carry must be fp32 [> {table.max_slot}, {H}]")
    if not x.is_cuda:
        return ref.pool_embed(x, residual, weight, eps, table.segments, carry,
                              dims, normalize)
    if table.segs is None:
        raise ValueError("pooling table was built for the CPU")
    if carry is None:
        carry = torch.empty((0, H), dtype=torch.float32, device=x.device)
    need = table.slabs.shape[0] * H
    key = (x.device.index,)
    ws = _POOL_WS.get(key)
    if ws is None or ws.numel() < need:
        ws = torch.empty(max(need, 1), dtype=torch.float32, device=x.device)
        _POOL_WS[key] = ws
    out = torch.empty((len(table), dims), dtype=torch.float32, device=x.device)
    _native().pool_embed(out, carry, ws, x, residual, weight, table.segs,
                         table.slabs, eps, dims, bool(normalize))
    return out
