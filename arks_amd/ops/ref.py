"""Reference implementations of every arks_amd custom op, in plain PyTorch.

These are the numerics oracle for the HIP kernels (tests compare the gfx950
kernels against these run in fp32) and the compute path for CPU-only unit
tests of the engine/scheduler/model layers. They are NOT a runtime fallback:
on a GPU box the HIP extension is required and ops fail loudly without it
(see arks_amd/ops/__init__.py).

Conventions shared with the kernels:
- KV cache layout: [num_blocks, num_kv_heads, block_size, head_dim]
- block_tables: int32 [num_seqs, max_blocks_per_seq]
- slot_mapping: int64 flat slot index = block_id * block_size + offset
"""

from __future__ import annotations

import math

import torch


def rmsnorm(x: torch.Tensor, weight: torch.Tensor, eps: float = 1e-6) -> torch.Tensor:
    """RMSNorm over the last dim. Accumulates in fp32 like the kernel."""
    dtype = x.dtype
    xf = x.float()
    var = xf.pow(2).mean(dim=-1, keepdim=True)
    out = xf * torch.rsqrt(var + eps) * weight.float()
    return out.to(dtype)


def fused_add_rmsnorm(
    x: torch.Tensor, residual: torch.Tensor, weight: torch.Tensor, eps: float = 1e-6
) -> tuple[torch.Tensor, torch.Tensor]:
    """residual += x; out = rmsnorm(residual). Returns (out, new_residual)."""
    new_residual = (residual.float() + x.float()).to(x.dtype)
    return rmsnorm(new_residual, weight, eps), new_residual


def silu_mul(gate_up: torch.Tensor) -> torch.Tensor:
    """SwiGLU activation: input [..., 2*d] as [gate | up] -> silu(gate) * up."""
    d = gate_up.shape[-1] // 2
    gate = gate_up[..., :d].float()
    up = gate_up[..., d:].float()
    return (torch.nn.functional.silu(gate) * up).to(gate_up.dtype)


def _scaled_inv_freq(inv_freq: torch.Tensor, rope_scaling: dict | None,
                     base: float, head_dim: int) -> tuple[torch.Tensor, float]:
    """Apply an HF rope_scaling config; returns (inv_freq, mscale).
    Supports the llama3 ramp, YaRN (NTK-by-parts + attention scaling) and
    plain linear scaling — matching transformers' rope_utils semantics."""
    if not rope_scaling:
        return inv_freq, 1.0
    rtype = rope_scaling.get("rope_type") or rope_scaling.get("type")
    factor = float(rope_scaling.get("factor", 1.0))
    if rtype == "linear":
        return inv_freq / factor, 1.0
    if rtype == "llama3":
        lo = float(rope_scaling.get("low_freq_factor", 1.0))
        hi = float(rope_scaling.get("high_freq_factor", 4.0))
        orig = float(rope_scaling.get("original_max_position_embeddings", 8192))
        wavelen = 2 * math.pi / inv_freq
        scaled = torch.where(wavelen > orig / lo, inv_freq / factor, inv_freq)
        smooth = (orig / wavelen - lo) / (hi - lo)
        mid = (1 - smooth) * inv_freq / factor + smooth * inv_freq
        is_mid = (wavelen <= orig / lo) & (wavelen >= orig / hi)
        return torch.where(is_mid, mid, scaled), 1.0
    if rtype == "yarn":
        orig = float(rope_scaling.get("original_max_position_embeddings", 4096))
        beta_fast = float(rope_scaling.get("beta_fast", 32.0))
        beta_slow = float(rope_scaling.get("beta_slow", 1.0))

        def corr_dim(num_rot: float) -> float:
            return (head_dim * math.log(orig / (num_rot * 2 * math.pi))) / (
                2 * math.log(base))

        low = max(math.floor(corr_dim(beta_fast)), 0)
        high = min(math.ceil(corr_dim(beta_slow)), head_dim // 2 - 1)
        ramp = torch.clamp(
            (torch.arange(head_dim // 2, dtype=torch.float64,
                          device=inv_freq.device) - low) / max(high - low, 1),
            0, 1,
        )
        # ramp==0 (high-freq dims) -> extrapolate (keep original);
        # ramp==1 (long wavelengths) -> interpolate (divide by factor)
        out = (inv_freq / factor) * ramp + inv_freq * (1 - ramp)
        mscale = float(rope_scaling.get("attention_factor") or
                       (0.1 * math.log(factor) + 1.0))
        return out, mscale
    return inv_freq, 1.0


def rope_cos_sin_cache(
    head_dim: int,
    max_positions: int,
    base: float = 10000.0,
    dtype: torch.dtype = torch.float32,
    device=None,
    rope_scaling: dict | None = None,
) -> torch.Tensor:
    """Precomputed [max_positions, head_dim] cache: first half cos, second half sin
    (per rotary pair), matching HF neox-style RoPE (incl. llama3 / yarn /
    linear rope_scaling)."""
    inv_freq = 1.0 / (
        base ** (torch.arange(0, head_dim, 2, dtype=torch.float64, device=device) / head_dim)
    )
    inv_freq, mscale = _scaled_inv_freq(inv_freq, rope_scaling, base, head_dim)
    t = torch.arange(max_positions, dtype=torch.float64, device=device)
    freqs = torch.outer(t, inv_freq)  # [P, head_dim/2]
    cache = torch.cat([freqs.cos() * mscale, freqs.sin() * mscale], dim=-1)
    return cache.to(dtype)


def rope_apply(
    positions: torch.Tensor,  # [num_tokens] int
    q: torch.Tensor,  # [num_tokens, num_q_heads * head_dim]
    k: torch.Tensor,  # [num_tokens, num_kv_heads * head_dim]
    cos_sin: torch.Tensor,  # [max_pos, head_dim]
    head_dim: int,
) -> tuple[torch.Tensor, torch.Tensor]:
    """Neox-style (rotate-half) RoPE applied out-of-place to q and k."""

    def _rot(x: torch.Tensor) -> torch.Tensor:
        n = x.shape[0]
        xf = x.float().view(n, -1, head_dim)
        half = head_dim // 2
        cs = cos_sin.float()[positions]  # [n, head_dim]
        cos = cs[:, :half].unsqueeze(1)  # [n, 1, half]
        sin = cs[:, half:].unsqueeze(1)
        x1 = xf[..., :half]
        x2 = xf[..., half:]
        o1 = x1 * cos - x2 * sin
        o2 = x2 * cos + x1 * sin
        return torch.cat([o1, o2], dim=-1).view(n, -1).to(x.dtype)

    return _rot(q), _rot(k)


def reshape_and_cache(
    k: torch.Tensor,  # [num_tokens, num_kv_heads, head_dim]
    v: torch.Tensor,
    k_cache: torch.Tensor,  # [num_blocks, num_kv_heads, block_size, head_dim]
    v_cache: torch.Tensor,
    slot_mapping: torch.Tensor,  # [num_tokens] int64
) -> None:
    block_size = k_cache.shape[2]
    block_ids = slot_mapping // block_size
    offsets = slot_mapping % block_size
    k_cache[block_ids, :, offsets] = k.to(k_cache.dtype)
    v_cache[block_ids, :, offsets] = v.to(v_cache.dtype)


def attention_prefill_varlen(
    q: torch.Tensor,  # [total_tokens, num_q_heads, head_dim]
    k: torch.Tensor,  # [total_tokens, num_kv_heads, head_dim]
    v: torch.Tensor,
    cu_seqlens: torch.Tensor,  # [num_seqs + 1] int32
    scale: float,
    window: int = 0,
) -> torch.Tensor:
    """Causal attention over packed variable-length sequences (full prefill:
    keys == the packed k/v of the same forward). GQA by head repetition.
    window > 0 = sliding-window attention."""
    num_q_heads = q.shape[1]
    num_kv_heads = k.shape[1]
    rep = num_q_heads // num_kv_heads
    out = torch.empty_like(q)
    for i in range(cu_seqlens.numel() - 1):
        s, e = int(cu_seqlens[i]), int(cu_seqlens[i + 1])
        qi = q[s:e].float().transpose(0, 1)  # [H, L, D]
        ki = k[s:e].float().repeat_interleave(rep, dim=1).transpose(0, 1)
        vi = v[s:e].float().repeat_interleave(rep, dim=1).transpose(0, 1)
        L = e - s
        scores = torch.matmul(qi, ki.transpose(-1, -2)) * scale  # [H, L, L]
        mask = torch.triu(
            torch.full((L, L), float("-inf"), device=q.device), diagonal=1
        )
        if window > 0:
            mask = mask + torch.tril(
                torch.full((L, L), float("-inf"), device=q.device),
                diagonal=-window,
            )
        scores = scores + mask
        p = torch.softmax(scores, dim=-1)
        o = torch.matmul(p, vi)  # [H, L, D]
        out[s:e] = o.transpose(0, 1).to(q.dtype)
    return out


def attention_decode_paged(
    q: torch.Tensor,  # [num_seqs, num_q_heads, head_dim]
    k_cache: torch.Tensor,  # [num_blocks, num_kv_heads, block_size, head_dim]
    v_cache: torch.Tensor,
    block_tables: torch.Tensor,  # [num_seqs, max_blocks] int32
    seq_lens: torch.Tensor,  # [num_seqs] int32 (length INCLUDING current token)
    scale: float,
    window: int = 0,
) -> torch.Tensor:
    """Single-token decode attention against the paged KV cache.
    window > 0 = sliding-window (the query sees the last `window` keys)."""
    num_seqs, num_q_heads, head_dim = q.shape
    num_kv_heads = k_cache.shape[1]
    block_size = k_cache.shape[2]
    rep = num_q_heads // num_kv_heads
    out = torch.empty_like(q)
    for i in range(num_seqs):
        L = int(seq_lens[i])
        nblocks = (L + block_size - 1) // block_size
        bt = block_tables[i, :nblocks].long()
        # gather [L, num_kv_heads, head_dim]
        ks = k_cache[bt].permute(0, 2, 1, 3).reshape(nblocks * block_size, num_kv_heads, head_dim)[:L]
        vs = v_cache[bt].permute(0, 2, 1, 3).reshape(nblocks * block_size, num_kv_heads, head_dim)[:L]
        kf = ks.float().repeat_interleave(rep, dim=1)  # [L, H, D]
        vf = vs.float().repeat_interleave(rep, dim=1)
        qi = q[i].float()  # [H, D]
        scores = torch.einsum("hd,lhd->hl", qi, kf) * scale
        if window > 0 and L > window:
            scores[:, : L - window] = float("-inf")
        p = torch.softmax(scores, dim=-1)
        o = torch.einsum("hl,lhd->hd", p, vf)
        out[i] = o.to(q.dtype)
    return out


def attention_extend_paged(
    q: torch.Tensor,  # [total_new_tokens, num_q_heads, head_dim]
    k_cache: torch.Tensor,  # [num_blocks, num_kv_heads, block_size, head_dim]
    v_cache: torch.Tensor,
    block_tables: torch.Tensor,  # [num_seqs, max_blocks] int32
    kv_lens: torch.Tensor,  # [num_seqs] int32 total kv length per seq
    cu_seqlens_q: torch.Tensor,  # [num_seqs + 1] int32 (packed new tokens)
    scale: float,
    window: int = 0,
) -> torch.Tensor:
    """Causal attention of each sequence's new tokens over its full paged KV
    (prefix caching / chunked prefill). New token j of seq i sits at global
    position kv_len - q_len + j. window > 0 = sliding-window attention
    (each query sees only the last `window` key positions)."""
    num_q_heads, head_dim = q.shape[1], q.shape[2]
    num_kv_heads = k_cache.shape[1]
    block_size = k_cache.shape[2]
    rep = num_q_heads // num_kv_heads
    out = torch.empty_like(q)
    for i in range(cu_seqlens_q.numel() - 1):
        s, e = int(cu_seqlens_q[i]), int(cu_seqlens_q[i + 1])
        qn = e - s
        L = int(kv_lens[i])
        off = L - qn
        nblocks = (L + block_size - 1) // block_size
        bt = block_tables[i, :nblocks].long()
        ks = k_cache[bt].permute(0, 2, 1, 3).reshape(nblocks * block_size, num_kv_heads, head_dim)[:L]
        vs = v_cache[bt].permute(0, 2, 1, 3).reshape(nblocks * block_size, num_kv_heads, head_dim)[:L]
        kf = ks.float().repeat_interleave(rep, dim=1).transpose(0, 1)  # [H, L, D]
        vf = vs.float().repeat_interleave(rep, dim=1).transpose(0, 1)
        qi = q[s:e].float().transpose(0, 1)  # [H, qn, D]
        scores = torch.matmul(qi, kf.transpose(-1, -2)) * scale  # [H, qn, L]
        kpos = torch.arange(L, device=q.device)
        qpos = torch.arange(off, L, device=q.device)
        mask = kpos[None, :] > qpos[:, None]  # [qn, L] True = hidden
        if window > 0:
            mask |= kpos[None, :] <= qpos[:, None] - window
        scores = scores.masked_fill(mask, float("-inf"))
        p = torch.softmax(scores, dim=-1)
        o = torch.matmul(p, vf)  # [H, qn, D]
        out[s:e] = o.transpose(0, 1).to(q.dtype)
    return out


def moe_topk(router_logits: torch.Tensor, k: int, renorm: bool):
    """softmax + top-k (+ renorm): (weights [T,k] f32, ids [T,k] i32)."""
    probs = torch.softmax(router_logits.float(), dim=-1)
    weights, selected = probs.topk(k, dim=-1)
    if renorm:
        weights = weights / weights.sum(dim=-1, keepdim=True)
    return weights, selected.to(torch.int32)


def moe_mix(y: torch.Tensor, weights: torch.Tensor, ids: torch.Tensor,
            expert_base: int = 0) -> torch.Tensor:
    """Weighted mix of per-(local-)expert dense outputs y [El, T, H]."""
    El, T, H = y.shape
    le = ids.long() - expert_base
    mine = (le >= 0) & (le < El)
    le = le.clamp(0, El - 1)
    t_idx = torch.arange(T, device=y.device)[:, None].expand_as(le)
    gathered = y[le, t_idx].float()  # [T, k, H]
    w = torch.where(mine, weights, torch.zeros_like(weights))
    return torch.einsum("tkh,tk->th", gathered, w.float()).to(y.dtype)


def moe_mix_rows(y: torch.Tensor, weights: torch.Tensor,
                 rows: torch.Tensor) -> torch.Tensor:
    """out[t] = sum_j weights[t,j] * y[rows[t,j]] over a flat [R, H]
    expert-output buffer."""
    gathered = y[rows.long()].float()  # [T, k, H]
    return torch.einsum("tkh,tk->th", gathered, weights.float()).to(y.dtype)


def lora_shrink(h: torch.Tensor, x: torch.Tensor, A: torch.Tensor,
                tiles: torch.Tensor) -> None:
    """h[row, :] = x[row, :] . A[slot]^T (fp32) for the rows covered by the
    (row0, nrows, slot) tile table; slot < 0 tiles are skipped."""
    for row0, nrows, slot in tiles.tolist():
        if slot < 0:
            continue
        rows = slice(row0, row0 + nrows)
        h[rows] = x[rows].float() @ A[slot].float().t()


def lora_expand(y: torch.Tensor, h: torch.Tensor, B: torch.Tensor,
                tiles: torch.Tensor, slice_offsets) -> None:
    """y[row, n] += sum_j h[row, s(n) R + j] B[slot][n, j] in place (fp32
    accumulate, one rounding to y's dtype); uncovered rows are untouched."""
    R = B.shape[2]
    for row0, nrows, slot in tiles.tolist():
        if slot < 0:
            continue
        rows = slice(row0, row0 + nrows)
        for s in range(len(slice_offsets) - 1):
            cols = slice(slice_offsets[s], slice_offsets[s + 1])
            delta = h[rows, s * R:(s + 1) * R].float() @ B[slot, cols].float().t()
            y[rows, cols] = (y[rows, cols].float() + delta).to(y.dtype)


def quant_fp8_rows(x: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """Per-row symmetric quantization to OCP e4m3 (range +-448)."""
    amax = x.float().abs().amax(dim=1).clamp(min=1e-6)
    scale = 448.0 / amax
    q = (x.float() * scale[:, None]).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)
    return q, (1.0 / scale)


def greedy_sample(logits: torch.Tensor) -> torch.Tensor:
    """[num_seqs, vocab] -> [num_seqs] int64 argmax."""
    return logits.float().argmax(dim=-1)


def gumbel_sample(
    logits: torch.Tensor,  # [num_seqs, vocab]
    temperatures: torch.Tensor,  # [num_seqs] float; 0 => greedy
    uniform: torch.Tensor,  # [num_seqs, vocab] uniform(0,1) noise
) -> torch.Tensor:
    """Exact categorical sampling via the Gumbel-max trick:
    argmax(logits/T + Gumbel) ~ softmax(logits/T). T==0 rows are greedy."""
    lf = logits.float()
    t = temperatures.float().clamp(min=0.0).unsqueeze(1)
    gumbel = -torch.log(-torch.log(uniform.float().clamp(1e-20, 1.0)))
    scaled = torch.where(t > 0, lf / t.clamp(min=1e-8) + gumbel, lf)
    return scaled.argmax(dim=-1)


def bitmask_allowed(masks: torch.Tensor, mask_row: torch.Tensor,
                    vocab: int) -> torch.Tensor:
    """[rows, vocab] bool from packed masks: bit (t % 32) of int32 word
    (t // 32) of masks[mask_row[r]] allows token t. Rows with mask_row -1
    allow everything; bits at positions >= vocab are ignored."""
    t = torch.arange(vocab, device=masks.device)
    mr = mask_row.long()
    words = masks[mr.clamp(min=0)][:, t // 32].long()
    allowed = ((words >> (t % 32)) & 1).bool()
    return allowed | (mr < 0).unsqueeze(1)


def apply_token_bitmask(logits: torch.Tensor, masks: torch.Tensor,
                        mask_row: torch.Tensor) -> torch.Tensor:
    """In place: -inf where the token's bit is clear."""
    allowed = bitmask_allowed(masks, mask_row, logits.shape[1])
    logits.masked_fill_(~allowed, float("-inf"))
    return logits


def _pick_allowed(scores: torch.Tensor, allowed: torch.Tensor) -> torch.Tensor:
    ids = scores.argmax(dim=-1)
    # every allowed score is -inf: argmax may sit on a masked index; the
    # lowest allowed index wins then, and a row with no bit set gives -1
    bad = ~allowed.gather(1, ids.unsqueeze(1)).squeeze(1)
    first = allowed.int().argmax(dim=-1)
    first = torch.where(allowed.any(dim=-1), first, torch.full_like(first, -1))
    return torch.where(bad, first, ids)


def greedy_sample_masked(logits: torch.Tensor, masks: torch.Tensor,
                         mask_row: torch.Tensor) -> torch.Tensor:
    """greedy_sample over the allowed tokens only (NaN/+inf on a masked
    token never win); [rows] int64, -1 for an empty mask."""
    allowed = bitmask_allowed(masks, mask_row, logits.shape[1])
    lf = torch.where(allowed, logits.float(), float("-inf"))
    return _pick_allowed(lf, allowed)


def gumbel_sample_masked(logits, temperatures, uniform, masks,
                         mask_row) -> torch.Tensor:
    """gumbel_sample over the allowed tokens only."""
    allowed = bitmask_allowed(masks, mask_row, logits.shape[1])
    lf = torch.where(allowed, logits.float(), float("-inf"))
    t = temperatures.float().clamp(min=0.0).unsqueeze(1)
    gumbel = -torch.log(-torch.log(uniform.float().clamp(1e-20, 1.0)))
    scaled = torch.where(t > 0, lf / t.clamp(min=1e-8) + gumbel, lf)
    scaled = torch.where(allowed, scaled, float("-inf"))
    return _pick_allowed(scaled, allowed)


def softmax_scale(head_dim: int) -> float:
    return 1.0 / math.sqrt(head_dim)


# ---------------------------------------------------------------------------
# W4A16: 4-bit unsigned asymmetric weights, group size 128 along K.
#   w[n, k] = (q[n, k] - z[n, k // 128]) * s[n, k // 128]
# q, z are uint8 in 0..15; s is f32 holding f16-representable values (the
# stored precision). The packed form the GPU kernels read (w4_gemm.hip):
#   qweight int32 [N, K/8]  nibble i of word c of row n = q[n, 8c + order[i]]
#   scales  f16   [K/128, N]
#   zeros   uint8 [K/128, N]
# order = [0,2,4,6,1,3,5,7] puts elements 2p and 2p+1 in nibbles p and p+4,
# i.e. 16 bits apart, so one shift+mask yields a bf16 pair in the kernel.
# ---------------------------------------------------------------------------
W4_GROUP = 128
_W4_ORDER = (0, 2, 4, 6, 1, 3, 5, 7)


def _pack_nibbles(x: torch.Tensor) -> torch.Tensor:
    """[..., L] values 0..15 -> int32 [..., L/8]; nibble i of word c holds
    x[..., 8c + order[i]]."""
    assert x.shape[-1] % 8 == 0, x.shape
    v = x.reshape(*x.shape[:-1], -1, 8).to(torch.int64)
    v = v[..., list(_W4_ORDER)]
    shifts = torch.arange(0, 32, 4, dtype=torch.int64, device=x.device)
    return (v << shifts).sum(dim=-1).to(torch.int32)  # wraps to two's compl.


def _unpack_nibbles(p: torch.Tensor) -> torch.Tensor:
    """Inverse of _pack_nibbles: int32 [..., C] -> uint8 [..., 8C]."""
    shifts = torch.arange(0, 32, 4, dtype=torch.int32, device=p.device)
    nib = ((p.unsqueeze(-1) >> shifts) & 0xF).to(torch.uint8)
    out = torch.empty_like(nib)
    out[..., list(_W4_ORDER)] = nib
    return out.reshape(*p.shape[:-1], -1)


def w4_check_k(K: int, what: str = "weight") -> None:
    if K % W4_GROUP != 0:
        raise ValueError(
            f"{what}: int4 needs the input width to be a multiple of the "
            f"group size {W4_GROUP}, got K={K}"
        )


def w4_quantize(w: torch.Tensor):
    """Round-to-nearest per (row, 128-group) over the group's min/max range
    (widened to include 0 so the zero-point fits 0..15): (q, z, s) with
    q uint8 [N, K], z uint8 [N, K/128], s f32 [N, K/128]. s is rounded UP to
    f16 so the stored scale still spans the range; a constant group gets the
    smallest scale instead of dividing by zero."""
    N, K = w.shape
    w4_check_k(K)
    G = K // W4_GROUP
    wf = w.float().reshape(N, G, W4_GROUP)
    lo = wf.amin(dim=-1).clamp(max=0.0)
    hi = wf.amax(dim=-1).clamp(min=0.0)
    s = ((hi - lo) / 15.0).clamp(min=2.0 ** -14)
    s16 = s.to(torch.float16)
    # next f16 up (positive values: the bit pattern plus one)
    s16 = torch.where(s16.float() < s,
                      (s16.view(torch.int16) + 1).view(torch.float16), s16)
    s = s16.float()
    z = torch.round(-lo / s).clamp(0, 15)
    q = (torch.round(wf / s[..., None]) + z[..., None]).clamp(0, 15)
    return (q.reshape(N, K).to(torch.uint8), z.to(torch.uint8), s)


def w4_dequant(q: torch.Tensor, z: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """f32 [N, K] = (q - z) * s."""
    N, K = q.shape
    G = K // W4_GROUP
    d = q.float().reshape(N, G, W4_GROUP) - z.float()[..., None]
    return (d * s.float()[..., None]).reshape(N, K)


def w4_pack(q: torch.Tensor, z: torch.Tensor, s: torch.Tensor):
    """(q, z, s) -> the packed triple (qweight, scales, zeros) above."""
    w4_check_k(q.shape[1])
    return (_pack_nibbles(q), s.t().contiguous().to(torch.float16),
            z.t().contiguous().to(torch.uint8))


def w4_unpack(packed):
    """Inverse of w4_pack: (q, z, s)."""
    qweight, scales, zeros = packed
    return (_unpack_nibbles(qweight), zeros.t().contiguous(),
            scales.t().float().contiguous())


def w4_linear(x: torch.Tensor, packed, bias=None) -> torch.Tensor:
    """The CPU emulation of a W4 layer: a bf16 GEMM on the bf16-rounded
    dequantized weight."""
    w = w4_dequant(*w4_unpack(packed)).to(torch.bfloat16)
    return torch.nn.functional.linear(x, w, bias)


def moe_route(ids: torch.Tensor, expert_base: int, n_local: int):
    """Routing table of the W4 expert GEMM from ids [T, k] (global expert
    ids): counts int32 [n_local] and pairs int32 [n_local, T], where expert
    e's first counts[e] entries are the pair indices p = t*k + j routed to
    expert_base + e, ascending. Entries past counts[e] are 0 here and
    unspecified in general."""
    T = ids.shape[0]
    flat = ids.reshape(-1)
    counts = torch.zeros(n_local, dtype=torch.int32, device=ids.device)
    pairs = torch.zeros(n_local, T, dtype=torch.int32, device=ids.device)
    for e in range(n_local):
        p = torch.nonzero(flat == expert_base + e).reshape(-1)[:T]
        counts[e] = p.numel()
        pairs[e, :p.numel()] = p.to(torch.int32)
    return counts, pairs


def w4_moe_gemm(a: torch.Tensor, packed, counts: torch.Tensor,
                pairs: torch.Tensor, src_div: int, out=None) -> torch.Tensor:
    """out[p] = a[p // src_div] @ dequant(W[e])^T for every local expert e
    and p in pairs[e][:counts[e]]: a plain loop over experts on the
    dequantized weights (f32 accumulate, one rounding to a's dtype). packed
    is the stacked triple (qweight [E, N, K/8], scales [E, K/128, N], zeros
    [E, K/128, N]). Rows of `out` that no local expert owns are left as they
    are (zeros when out is None)."""
    qweight, scales, zeros = packed
    E, N = qweight.shape[0], qweight.shape[1]
    T = pairs.shape[1]
    n_pairs = T * (a.shape[0] * src_div // T)
    if out is None:
        out = torch.zeros(n_pairs, N, dtype=a.dtype, device=a.device)
    for e in range(E):
        p = pairs[e, :int(counts[e])].long()
        if p.numel() == 0:
            continue
        w = w4_dequant(*w4_unpack((qweight[e], scales[e], zeros[e])))
        src = torch.div(p, src_div, rounding_mode="floor")
        out[p] = (a[src].float() @ w.t()).to(out.dtype)
    return out


def awq_unpack(qweight: torch.Tensor, qzeros: torch.Tensor,
               scales: torch.Tensor):
    """AutoAWQ "GEMM" on-disk layout -> (q [N, K], z [N, K/128], s [N, K/128]).
    qweight int32 [K, N/8], qzeros int32 [K/128, N/8], scales f16 [K/128, N];
    nibble i of packed column c holds logical column 8c + order[i]."""
    K = qweight.shape[0]
    w4_check_k(K, "AWQ qweight")
    if qzeros.shape[0] * W4_GROUP != K or scales.shape[0] * W4_GROUP != K:
        raise ValueError(
            f"AWQ tensors disagree on group size {W4_GROUP}: qweight K={K}, "
            f"qzeros {tuple(qzeros.shape)}, scales {tuple(scales.shape)}"
        )
    q = _unpack_nibbles(qweight).t().contiguous()
    z = _unpack_nibbles(qzeros).t().contiguous()
    return q, z, scales.t().float().contiguous()


def awq_pack(q: torch.Tensor, z: torch.Tensor, s: torch.Tensor):
    """Inverse of awq_unpack: (qweight, qzeros, scales)."""
    return (_pack_nibbles(q.t().contiguous()),
            _pack_nibbles(z.t().contiguous()),
            s.t().contiguous().to(torch.float16))


# ---------------------------------------------------------------------------
# W8A16: OCP e4m3fn weights scaled per 128x128 block (the "fine-grained FP8"
# checkpoint format of transformers):
#   w[n, k] = float(w8[n, k]) * block_scale[n // 128, k // 128]
# On disk: weight e4m3fn [N, K] and weight_scale_inv f32
# [ceil(N/128), ceil(K/128)]. In a layer the weight is kept as it is and the
# scales are expanded to one value per (k-block, output row), f32
# [ceil(K/128), N]: the orientation of the W4 scales, so that fused
# projections concatenate along N and a shard can cut at any row.
# ---------------------------------------------------------------------------
W8_BLOCK = 128
W8_MAX = 448.0  # largest e4m3fn value


def w8_quantize(w: torch.Tensor):
    """Block-wise amax / 448 scaling with round-to-nearest-even:
    (w8 e4m3fn [N, K], block scales f32 [ceil(N/128), ceil(K/128)]), the two
    tensors a checkpoint stores as weight / weight_scale_inv. An all-zero
    block gets scale 1."""
    N, K = w.shape
    B = W8_BLOCK
    nb, kb = -(-N // B), -(-K // B)
    wf = torch.zeros(nb * B, kb * B, dtype=torch.float32, device=w.device)
    wf[:N, :K] = w.float()
    blocks = wf.view(nb, B, kb, B)
    amax = blocks.abs().amax(dim=(1, 3))
    s = torch.where(amax > 0, amax / W8_MAX, torch.ones_like(amax))
    q = (blocks / s[:, None, :, None]).clamp(-W8_MAX, W8_MAX)
    w8 = q.reshape(nb * B, kb * B)[:N, :K].contiguous().to(torch.float8_e4m3fn)
    return w8, s


def w8_expand_scales(block_scales: torch.Tensor, N: int) -> torch.Tensor:
    """Block scales [ceil(N/128), ceil(K/128)] -> per-row f32
    [ceil(K/128), N]: out[kb, n] = block_scales[n // 128, kb]."""
    if block_scales.dim() != 2 or block_scales.shape[0] != -(-N // W8_BLOCK):
        raise ValueError(
            f"block scales {tuple(block_scales.shape)} do not cover N={N} "
            f"at block size {W8_BLOCK}")
    rows = block_scales.float().repeat_interleave(W8_BLOCK, dim=0)[:N]
    return rows.t().contiguous()


def w8_dequant(w8: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """f32 [N, K] = float(w8) * scales[k // 128, n] for the expanded scales
    [ceil(K/128), N] of a layer."""
    N, K = w8.shape
    if tuple(scales.shape) != (-(-K // W8_BLOCK), N):
        raise ValueError(
            f"scales {tuple(scales.shape)} do not match a {N}x{K} weight: "
            f"expected [{-(-K // W8_BLOCK)}, {N}]")
    per_k = scales.float().t().repeat_interleave(W8_BLOCK, dim=1)[:, :K]
    return w8.float() * per_k


def w8_linear(x: torch.Tensor, w8: torch.Tensor, scales: torch.Tensor,
              bias=None) -> torch.Tensor:
    """The CPU emulation of a W8 layer: a GEMM on the dequantized weight
    rounded to the activation dtype."""
    return torch.nn.functional.linear(
        x, w8_dequant(w8, scales).to(x.dtype), bias)


def w8_moe_gemm(a: torch.Tensor, weight, counts: torch.Tensor,
                pairs: torch.Tensor, src_div: int, out=None) -> torch.Tensor:
    """out[p] = a[p // src_div] @ (float(w8[e]) * scales[e])^T for every
    local expert e and p in pairs[e][:counts[e]]: a plain loop over experts
    on w8_dequant (f32 accumulate, one rounding to a's dtype). weight is the
    stacked pair (w8 e4m3fn [E, N, K], scales f32 [E, K/128, N]). Rows of
    `out` that no local expert owns are left as they are (zeros when out is
    None)."""
    w8, scales = weight
    E, N = w8.shape[0], w8.shape[1]
    T = pairs.shape[1]
    n_pairs = T * (a.shape[0] * src_div // T)
    if out is None:
        out = torch.zeros(n_pairs, N, dtype=a.dtype, device=a.device)
    for e in range(E):
        p = pairs[e, :int(counts[e])].long()
        if p.numel() == 0:
            continue
        w = w8_dequant(w8[e], scales[e])
        src = torch.div(p, src_div, rounding_mode="floor")
        out[p] = (a[src].float() @ w.t()).to(out.dtype)
    return out


# ---------------------------------------------------------------------------
# MX4 (W4A16): OCP microscaling FP4 (MXFP4). e2m1 elements, one shared e8m0
# scale per block of 32 along K:
#   w[n, k] = e2m1(code[n, k]) * 2^(scales[n, k // 32] - 127)
# On disk and in a layer alike: weight u8 [N, K/2], byte b of a row holding
# k = 2b in its low nibble and k = 2b+1 in its high nibble, and scales u8
# [N, K/32]. A code is a sign (bit 3) and an index into MX4_VALUES.
# ---------------------------------------------------------------------------
MX4_BLOCK = 32
MX4_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
# Scale bytes a layer accepts: 0.5 * 2^(s-127) must be a normal bf16 and
# 6 * 2^(s-127) finite, so that scaling before the MFMA is exact. 255 is NaN.
MX4_SCALE_MIN, MX4_SCALE_MAX = 2, 252


def mx4_quantize(w: torch.Tensor):
    """The OCP MX conversion rule: per block of 32 along K the shared
    exponent is floor(log2(amax)) - 2 (2 = the exponent of e2m1's largest
    value), the elements are divided by it, rounded to the nearest e2m1 value
    (ties to the even code) and saturated at +-6. Returns (packed u8
    [N, K/2], scales u8 [N, K/32]). An all-zero block gets scale byte 127;
    the byte is kept inside [MX4_SCALE_MIN, MX4_SCALE_MAX], the range a
    layer accepts (elements of a block below it round towards zero, above it
    they saturate)."""
    N, K = w.shape
    if K % MX4_BLOCK != 0:
        raise ValueError(f"mx4_quantize needs K % {MX4_BLOCK} == 0, got K={K}")
    blocks = w.float().view(N, K // MX4_BLOCK, MX4_BLOCK)
    amax = blocks.abs().amax(dim=2)
    # amax = m * 2^ex with m in [0.5, 1): floor(log2(amax)) = ex - 1, exactly
    _, ex = torch.frexp(amax)
    s = torch.where(amax > 0, ex.to(torch.int32) - 3 + 127,
                    torch.full_like(ex, 127, dtype=torch.int32))
    s = s.clamp(MX4_SCALE_MIN, MX4_SCALE_MAX)
    q = torch.ldexp(blocks, (127 - s)[:, :, None])
    a = q.abs().clamp(max=6.0)
    step = torch.where(a < 2.0, 0.5, torch.where(a < 4.0, 1.0, 2.0))
    v = torch.round(a / step) * step  # half to even = ties to the even code
    table = torch.tensor(MX4_VALUES, dtype=torch.float32, device=w.device)
    code = torch.searchsorted(table, v.contiguous()).to(torch.uint8)
    code = code | (((q < 0) & (v > 0)).to(torch.uint8) << 3)
    code = code.view(N, K)
    packed = code[:, 0::2] | (code[:, 1::2] << 4)
    return packed.contiguous(), s.to(torch.uint8)


def mx4_dequant(packed: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """f32 [N, K] = e2m1(code) * 2^(scales[n, k // 32] - 127), exactly (a
    scale byte of 255 is NaN)."""
    N, K = packed.shape[0], packed.shape[1] * 2
    if (packed.dtype != torch.uint8 or scales.dtype != torch.uint8
            or K % MX4_BLOCK != 0
            or tuple(scales.shape) != (N, K // MX4_BLOCK)):
        raise ValueError(
            f"mx4 weight {tuple(packed.shape)} {packed.dtype} / scales "
            f"{tuple(scales.shape)} {scales.dtype}: expected uint8 [N, K/2] "
            f"and uint8 [N, K/{MX4_BLOCK}]")
    mags = torch.tensor(MX4_VALUES, dtype=torch.float32, device=packed.device)
    lut = torch.cat([mags, -mags])
    code = torch.stack([packed & 0xF, packed >> 4], dim=2).view(N, K)
    vals = lut[code.long()]
    s = scales.to(torch.int32)
    p2 = torch.ldexp(torch.ones_like(s, dtype=torch.float32), s - 127)
    p2 = torch.where(s == 255, torch.full_like(p2, float("nan")), p2)
    return vals * p2.repeat_interleave(MX4_BLOCK, dim=1)


def mx4_linear(x: torch.Tensor, packed: torch.Tensor, scales: torch.Tensor,
               bias=None) -> torch.Tensor:
    """The CPU emulation of an MX4 layer: a GEMM on the dequantized weight
    rounded to the activation dtype (exact for bf16 and wider)."""
    return torch.nn.functional.linear(
        x, mx4_dequant(packed, scales).to(x.dtype), bias)


POOL_LAST, POOL_MEAN, POOL_CLS = 0, 1, 2


def pool_embed(x, residual, weight, eps, segments, carry=None,
               dims: int | None = None, normalize: bool = True):
    """Embedding pooling over packed rows [T, H]: one fp32 vector per entry
    of `segments`, a list of (row0, nrows, mode, slot, counted, final).
    For a segment of rows [a, b):
      r_i = (x_i + residual_i) rounded to the input dtype (the rounding
            fused_add_rmsnorm gives the residual stream);
      y_i = r_i * rsqrt(mean(r_i^2) + eps) * w, in fp32, never rounded;
      last: v = y_{b-1}; cls: v = y_a; mean: v = (carry + sum y_i) / count,
      where carry [slots, H] fp32 holds the sum over the `counted` tokens of
      earlier prefill chunks (ignored when counted == 0) and count =
      counted + nrows. A non-final mean chunk only writes the updated carry
      (its output row is zero).
    v is cut to v[:dims] and, with normalize, divided by max(|v|_2, 1e-12).
    Returns fp32 [num_segments, dims]; x and residual are not modified."""
    H = x.shape[-1]
    dims = H if dims is None else dims
    if not 1 <= dims <= H:
        raise ValueError(f"dims must be in [1, {H}], got {dims}")
    wf = weight.float()
    out = torch.zeros((len(segments), dims), dtype=torch.float32,
                      device=x.device)

    def normed(rows):
        r = (x[rows].float() + residual[rows].float()).to(x.dtype).float()
        var = r.pow(2).mean(dim=-1, keepdim=True)
        return r * torch.rsqrt(var + eps) * wf

    for s, (row0, nrows, mode, slot, counted, final) in enumerate(segments):
        if mode == POOL_MEAN:
            v = normed(slice(row0, row0 + nrows)).sum(dim=0)
            if counted > 0:
                v = carry[slot] + v
            if not final:
                carry[slot] = v
                continue
            v = v / float(counted + nrows)
        else:
            row = row0 + nrows - 1 if mode == POOL_LAST else row0
            v = normed(slice(row, row + 1))[0]
        v = v[:dims]
        if normalize:
            v = v / v.norm().clamp_min(1e-12)
        out[s] = v
    return out
