// Multi-head latent attention (DeepSeek-V2/V3 MLA) for CDNA4 (gfx950):
// the kernel that writes the paged latent cache and absorbed-query attention
// over it, for decode and for query lengths above 1.
//
// Latent cache: one tensor per layer, [num_blocks, 16, 576] bf16, no head
// axis and no separate V. Columns 0..511 of a row are the RMS-normalised
// compressed KV (kv_lora_rank), columns 512..575 the rotated shared rope key
// (qk_rope_head_dim). All heads read the same row, as key (576 wide) and as
// value (the first 512 columns).
//
// attn_mla_kernel. Grid (ceil(H/16), T, partitions), 256 threads = 4 waves.
// A tile of 16 heads of ONE query token is the MFMA M/N axis; rows >= H are
// zero and never stored. Each wave keeps Q^T as B-operand fragments (18
// contraction steps of 32 = 72 VGPRs) and 32 f32x4 output chunks (128
// accumulator registers), and strides over the partition's pages, one
// 16-token page per iteration. A page is contiguous in the cache (18 KB): it
// is fetched ONCE with coalesced 16 B loads (18 per lane), the loads of page
// i+1 ride in registers during page i's MFMAs, and it is staged row-major in
// the wave's LDS region, from which BOTH operand views are built:
//   S = K Q^T   A-operand rows straight from the image (b128 per lane), all
//               576 columns: 18 mfma_f32_16x16x32_bf16 per page;
//   O += P V    B-operand through ds_read_tr16_b64 on the same image (lane
//               i of a 16-lane group addresses token i/4, columns 4*(i%4)..),
//               one 16-token 16x16x16 MFMA per 16 output columns. Its
//               A-operand layout (head = lane%16, tokens 4*(lane/16)..+3) is
//               exactly the layout S comes out of the first MFMA in, so P
//               goes from the softmax registers into the second MFMA with no
//               LDS round trip.
// Token rows at or beyond the causal limit are never loaded: their LDS rows
// are zero (the row is also V, and 0 x NaN is NaN). Column-wise online
// softmax as in attn_decode.hip (lane lq owns head lq); waves merge
// flash-style in LDS; with more than one partition every workgroup emits an
// f32 partial (acc[512], m, l) per head and attn_mla_combine_kernel reduces
// them. The sequence of a query token is found from cu_seqlens in the kernel,
// so the launch needs no host-built table and no synchronisation.
#include "common.h"

#include <cfloat>

namespace arks {

constexpr int MLA_PAGE = 16;       // tokens per page (matches the engine)
constexpr int MLA_LAT = 512;       // kv_lora_rank
constexpr int MLA_ROPE = 64;       // qk_rope_head_dim
constexpr int MLA_ROW = MLA_LAT + MLA_ROPE;
constexpr int MLA_LDS_ROW = 584;   // padded LDS row (1168 B: 16 B aligned,
                                   // 16 rows x b128 hit 64 distinct banks)
constexpr int MLA_STEPS = MLA_ROW / 32;    // QK^T contraction steps
constexpr int MLA_CHUNKS = MLA_LAT / 16;   // PV output column chunks
constexpr int MLA_PAGE_LOADS = MLA_PAGE * MLA_ROW / 8 / WAVE_SIZE;  // 18
constexpr int MLA_MROW = MLA_LAT + 4;  // merge / partial row: acc, m, l, pad

typedef __attribute__((ext_vector_type(8))) __bf16 mla_bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 mla_bf16x4;
typedef __attribute__((ext_vector_type(4))) float mla_f32x4;

__global__ __launch_bounds__(256) void attn_mla_kernel(
    bf16* __restrict__ out,        // [T, H, 512] (used when gridDim.z == 1)
    float* __restrict__ part_out,  // [T, HT, P, 16, MLA_MROW] (gridDim.z > 1)
    const bf16* __restrict__ q_lat,  // [T, H, 512] contiguous
    const bf16* __restrict__ q_pe,   // [T, H, 64], strides qpe_ts / qpe_hs
    const bf16* __restrict__ cache,  // [num_blocks, 16, 576]
    const int* __restrict__ block_tables,  // [S, max_blocks]
    const int* __restrict__ seq_lens,      // [S] total KV length
    const int* __restrict__ cu_seqlens,    // [S + 1] or null (T == S)
    const float scale, const int H, const int num_seqs, const int max_blocks,
    const int num_blocks, const int64_t qpe_ts, const int64_t qpe_hs) {
  constexpr int NUM_WAVES = 4;
  const int ht = blockIdx.x;
  const int tok = blockIdx.y;
  const int part = blockIdx.z;
  const int nparts = gridDim.z;
  const int tid = threadIdx.x;
  const int wave = tid / WAVE_SIZE;
  const int lane = tid % WAVE_SIZE;
  const int lq = lane % 16;
  const int la = lane / 16;

  // The sequence of this query token and how many positions it sees:
  // token i of a sequence with q_len new tokens sees < seq_len - q_len + i + 1.
  int seq = tok;
  int L;
  if (cu_seqlens != nullptr) {
    int lo = 0, hi = num_seqs - 1;  // the last s with cu_seqlens[s] <= tok
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (cu_seqlens[mid] <= tok) lo = mid; else hi = mid - 1;
    }
    seq = lo;
    L = seq_lens[seq] - cu_seqlens[seq + 1] + tok + 1;
  } else {
    L = seq_lens[seq];
  }
  L = max(0, min(L, max_blocks * MLA_PAGE));
  const int nblocks = (L + MLA_PAGE - 1) / MLA_PAGE;
  const int chunk = (nblocks + nparts - 1) / nparts;  // pages per partition
  const int pb_lo = part * chunk;
  const int pb_hi = min(pb_lo + chunk, nblocks);

  // Per-wave LDS region: the page image during the main loop, the merge
  // buffer afterwards (a wave touches only its own region between the loop
  // and the barrier).
  constexpr int TILE_BYTES = MLA_PAGE * MLA_LDS_ROW * 2;
  constexpr int MERGE_BYTES = 16 * MLA_MROW * 4;
  constexpr int WAVE_BYTES = TILE_BYTES > MERGE_BYTES ? TILE_BYTES : MERGE_BYTES;
  __shared__ __attribute__((aligned(16))) char smem[NUM_WAVES][WAVE_BYTES];
  bf16* tile = reinterpret_cast<bf16*>(smem[wave]);       // [16][584]
  float* merge_lds = reinterpret_cast<float*>(smem[wave]);  // [16][516]

  // Q fragments: B-operand [32 k x 16 heads] per step; steps 0..15 come from
  // q_lat, 16..17 from q_pe; rows >= H are zero.
  mla_bf16x8 qfrag[MLA_STEPS];
  {
    const int head = ht * 16 + lq;
    const bool valid = head < H;
    const bf16* ql = q_lat + ((int64_t)tok * H + (valid ? head : 0)) * MLA_LAT;
    const bf16* qp = q_pe + (int64_t)tok * qpe_ts +
                     (int64_t)(valid ? head : 0) * qpe_hs;
#pragma unroll
    for (int st = 0; st < MLA_STEPS; ++st) {
      ushort8 u{};
      if (valid) {
        const bf16* src = st < MLA_LAT / 32 ? ql + st * 32 + 8 * la
                                            : qp + (st - MLA_LAT / 32) * 32 + 8 * la;
        u = *reinterpret_cast<const ushort8*>(src);
      }
      qfrag[st] = *reinterpret_cast<mla_bf16x8*>(&u);
    }
  }

  float m_run = -FLT_MAX;  // per head lq (replicated over la)
  float l_run = 0.f;
  mla_f32x4 oacc[MLA_CHUNKS];
#pragma unroll
  for (int c = 0; c < MLA_CHUNKS; ++c) oacc[c] = {0.f, 0.f, 0.f, 0.f};

  const int* bt = block_tables + (int64_t)seq * max_blocks;
  // Block-table ids run two iterations ahead of their use, so the page
  // loads never wait on a dependent id load (as in attn_decode.hip).
  auto raw_bt = [&](int pb_) { return pb_ < pb_hi ? bt[pb_] : 0; };
  // One page into registers: lane + 64 j is the 16 B piece index of the
  // contiguous page, piece / 72 its token row. Rows at or beyond L are not
  // read and stay zero.
  auto load_page = [&](int id, int pb_, ushort8 (&dst)[MLA_PAGE_LOADS]) {
    id = min(max(id, 0), num_blocks - 1);
    const bf16* base = cache + (int64_t)id * (MLA_PAGE * MLA_ROW);
    const int rows = L - pb_ * MLA_PAGE;
#pragma unroll
    for (int j = 0; j < MLA_PAGE_LOADS; ++j) {
      const int piece = lane + WAVE_SIZE * j;
      ushort8 u{};
      if (piece / (MLA_ROW / 8) < rows)
        u = *reinterpret_cast<const ushort8*>(base + piece * 8);
      dst[j] = u;
    }
  };

  ushort8 pre[MLA_PAGE_LOADS];
  const int pb_w0 = pb_lo + wave;
  int nid = raw_bt(pb_w0 + NUM_WAVES);
  if (pb_w0 < pb_hi) load_page(raw_bt(pb_w0), pb_w0, pre);

  for (int pb = pb_w0; pb < pb_hi; pb += NUM_WAVES) {
    const int nnid = raw_bt(pb + 2 * NUM_WAVES);
    const int tok0 = pb * MLA_PAGE;

    // ---- stage the page row-major in LDS (behind the previous page's
    // reads: LDS is in order within the wave), then start the next page.
#pragma unroll
    for (int j = 0; j < MLA_PAGE_LOADS; ++j) {
      const int piece = lane + WAVE_SIZE * j;
      *reinterpret_cast<ushort8*>(
          &tile[(piece / (MLA_ROW / 8)) * MLA_LDS_ROW +
                (piece % (MLA_ROW / 8)) * 8]) = pre[j];
    }
    if (pb + NUM_WAVES < pb_hi) load_page(nid, pb + NUM_WAVES, pre);
    // Intra-wave LDS producer->consumer: wait on the LDS counter ONLY, the
    // next page's global loads stay outstanding.
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

    // ---- S = K Q^T over all 576 columns: A = image rows, B = Q registers.
    mla_f32x4 sc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int st = 0; st < MLA_STEPS; ++st) {
      ushort8 ka = *reinterpret_cast<const ushort8*>(
          &tile[lq * MLA_LDS_ROW + st * 32 + 8 * la]);
      sc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          *reinterpret_cast<mla_bf16x8*>(&ka), qfrag[st], sc, 0, 0, 0);
    }

    // Phase fence for the scheduler: left free it hoists the next phase's
    // LDS reads over this one and spills (59 VGPRs, 104 B of scratch a lane).
    __builtin_amdgcn_sched_barrier(0);
    // ---- masked column-wise online softmax: sc[r] is token 4 la + r of
    // head lq.
    float p[4];
    float tile_max = -FLT_MAX;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool vis = tok0 + 4 * la + r < L;
      p[r] = vis ? sc[r] * scale : -FLT_MAX;
      tile_max = fmaxf(tile_max, p[r]);
    }
    tile_max = fmaxf(tile_max, __shfl_xor(tile_max, 16, WAVE_SIZE));
    tile_max = fmaxf(tile_max, __shfl_xor(tile_max, 32, WAVE_SIZE));
    const float m_new = fmaxf(m_run, tile_max);
    float alpha = 1.f;
    float psum = 0.f;
    if (m_new > -FLT_MAX) {
      alpha = __expf(m_run - m_new);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        p[r] = (p[r] > -FLT_MAX) ? __expf(p[r] - m_new) : 0.f;
        psum += p[r];
      }
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) p[r] = 0.f;
    }
    psum += __shfl_xor(psum, 16, WAVE_SIZE);
    psum += __shfl_xor(psum, 32, WAVE_SIZE);
    l_run = l_run * alpha + psum;
    m_run = m_new;

    // rescale O rows (head = 4 la + r in the PV fragment).
    float row_alpha[4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
      row_alpha[r] = __shfl(alpha, 4 * la + r, WAVE_SIZE);
#pragma unroll
    for (int c = 0; c < MLA_CHUNKS; ++c) {
#pragma unroll
      for (int r = 0; r < 4; ++r) oacc[c][r] *= row_alpha[r];
    }

    __builtin_amdgcn_sched_barrier(0);
    // ---- O += P V: P (head lq, tokens 4 la..+3) is already an A fragment;
    // V^T comes out of the same image through the transposing read.
    mla_bf16x4 pa;
    {
      ushort4v pk;
#pragma unroll
      for (int r = 0; r < 4; ++r) pk[r] = float_to_bf16_bits(p[r]);
      pa = *reinterpret_cast<mla_bf16x4*>(&pk);
    }
    const bf16* vrow = &tile[(4 * la + (lq >> 2)) * MLA_LDS_ROW + 4 * (lq & 3)];
#pragma unroll
    for (int c = 0; c < MLA_CHUNKS; ++c) {
      mla_bf16x4 vb = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
          (__attribute__((address_space(3))) mla_bf16x4*)(vrow + c * 16));
      oacc[c] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(pa, vb, oacc[c], 0,
                                                          0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
    nid = nnid;
  }

  // ---- merge the 4 wave partials (flash-style) and emit.
  __syncthreads();  // everyone done with the page image before the union flips
#pragma unroll
  for (int c = 0; c < MLA_CHUNKS; ++c) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      merge_lds[(4 * la + r) * MLA_MROW + c * 16 + lq] = oacc[c][r];
  }
  if (la == 0) {
    merge_lds[lq * MLA_MROW + MLA_LAT] = m_run;
    merge_lds[lq * MLA_MROW + MLA_LAT + 1] = l_run;
  }
  __syncthreads();

  // 256 threads = 16 heads x 16 column slices; a thread owns columns
  // 4 l16 + 64 e .. +3 (e = 0..7) of head g, merged over the 4 waves.
  const int g = tid / 16;
  const int l16 = tid % 16;
  const int head = ht * 16 + g;
  if (head >= H) return;
  float mf = -FLT_MAX, lf = 0.f;
  float4v af[MLA_LAT / 64];
#pragma unroll
  for (int e = 0; e < MLA_LAT / 64; ++e) af[e] = float4v{0.f, 0.f, 0.f, 0.f};
  for (int w = 0; w < NUM_WAVES; ++w) {
    const float* wl = reinterpret_cast<const float*>(smem[w]) + g * MLA_MROW;
    const float mw = wl[MLA_LAT];
    const float lw = wl[MLA_LAT + 1];
    const float mn = fmaxf(mf, mw);
    const float a1 = __expf(mf - mn);
    const float a2 = __expf(mw - mn);
    lf = lf * a1 + lw * a2;
#pragma unroll
    for (int e = 0; e < MLA_LAT / 64; ++e)
      af[e] = af[e] * a1 +
              *reinterpret_cast<const float4v*>(wl + 4 * l16 + 64 * e) * a2;
    mf = mn;
  }
  if (nparts == 1) {
    const float inv = lf > 0.f ? 1.f / lf : 0.f;
    bf16* op = out + ((int64_t)tok * H + head) * MLA_LAT + 4 * l16;
#pragma unroll
    for (int e = 0; e < MLA_LAT / 64; ++e) {
      ushort4v o4;
#pragma unroll
      for (int i = 0; i < 4; ++i) o4[i] = float_to_bf16_bits(af[e][i] * inv);
      *reinterpret_cast<ushort4v*>(op + 64 * e) = o4;
    }
  } else {
    float* pp = part_out +
                ((((int64_t)tok * gridDim.x + ht) * nparts + part) * 16 + g) *
                    MLA_MROW;
#pragma unroll
    for (int e = 0; e < MLA_LAT / 64; ++e)
      *reinterpret_cast<float4v*>(pp + 4 * l16 + 64 * e) = af[e];
    if (l16 == 0) {
      pp[MLA_LAT] = mf;
      pp[MLA_LAT + 1] = lf;
    }
  }
}

// Combine the partition partials: one workgroup of 128 threads per
// (query token, head), 4 output columns per thread. Every partition writes
// its partial, empty ones as (m = -FLT_MAX, l = 0, acc = 0).
__global__ __launch_bounds__(128) void attn_mla_combine_kernel(
    bf16* __restrict__ out,              // [T, H, 512]
    const float* __restrict__ part_out,  // [T, HT, P, 16, MLA_MROW]
    const int H, const int nparts) {
  const int tok = blockIdx.x;
  const int h = blockIdx.y;
  const int num_ht = (H + 15) / 16;
  const int d = 4 * threadIdx.x;
  const float* pp = part_out +
                    (((int64_t)tok * num_ht + h / 16) * nparts * 16 + h % 16) *
                        MLA_MROW;
  float mf = -FLT_MAX, lf = 0.f;
  float4v af = {0.f, 0.f, 0.f, 0.f};
  for (int p = 0; p < nparts; ++p, pp += 16 * MLA_MROW) {
    const float mw = pp[MLA_LAT];
    const float lw = pp[MLA_LAT + 1];
    const float mn = fmaxf(mf, mw);
    const float a1 = __expf(mf - mn);
    const float a2 = __expf(mw - mn);
    lf = lf * a1 + lw * a2;
    af = af * a1 + *reinterpret_cast<const float4v*>(pp + d) * a2;
    mf = mn;
  }
  const float inv = lf > 0.f ? 1.f / lf : 0.f;
  ushort4v o4;
#pragma unroll
  for (int i = 0; i < 4; ++i) o4[i] = float_to_bf16_bits(af[i] * inv);
  *reinterpret_cast<ushort4v*>(out + ((int64_t)tok * H + h) * MLA_LAT + d) = o4;
}

// One pass over a token's kv_a_proj_with_mqa row and its q_pe heads: wave 0
// RMS-normalises columns 0..511 (f32 accumulation) into the token's cache
// slot; all threads rotate the 32 pairs of the shared rope key (into the
// slot) and of every head's q_pe (in place). DeepSeek's rotation is over
// interleaved pairs: (2i, 2i+1) turns with frequency i, the pair stays where
// it is. A negative slot is a padding row: nothing is written to the cache.
__global__ __launch_bounds__(256) void mla_rope_cache_kernel(
    const int64_t* __restrict__ positions,  // [T]
    const bf16* __restrict__ kv_a,          // [T, 576], row stride kv_stride
    const bf16* __restrict__ norm_weight,   // [512]
    bf16* __restrict__ q_pe,                // [T, H, 64], strides
    const float* __restrict__ cos_sin,      // [max_pos, 64]: cos | sin
    bf16* __restrict__ cache,               // [num_blocks, 16, 576]
    const int64_t* __restrict__ slot_mapping,  // [T] (< 0 = no cache write)
    const float eps, const int H, const int64_t kv_stride,
    const int64_t qpe_ts, const int64_t qpe_hs) {
  const int token = blockIdx.x;
  const int tid = threadIdx.x;
  const int64_t slot = slot_mapping[token];
  const bf16* row = kv_a + (int64_t)token * kv_stride;
  bf16* dst = cache + (slot < 0 ? 0 : slot) * MLA_ROW;

  if (tid < WAVE_SIZE && slot >= 0) {
    const ushort8 x = *reinterpret_cast<const ushort8*>(row + 8 * tid);
    const ushort8 w = *reinterpret_cast<const ushort8*>(norm_weight + 8 * tid);
    float xf[8];
    float ss = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      xf[e] = bf16_bits_to_float(x[e]);
      ss += xf[e] * xf[e];
    }
    ss = wave_reduce_sum(ss);
    const float inv = rsqrtf(ss / MLA_LAT + eps);
    ushort8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e)
      o[e] = float_to_bf16_bits(xf[e] * inv * bf16_bits_to_float(w[e]));
    *reinterpret_cast<ushort8*>(dst + 8 * tid) = o;
  }

  const float* cs = cos_sin + positions[token] * MLA_ROPE;
  // item = head * 32 + pair; head H is the shared key
  for (int item = tid; item < (H + 1) * (MLA_ROPE / 2); item += blockDim.x) {
    const int head = item / (MLA_ROPE / 2);
    const int i = item % (MLA_ROPE / 2);
    const bool is_k = head == H;
    if (is_k && slot < 0) continue;
    const bf16* src = is_k ? row + MLA_LAT + 2 * i
                           : q_pe + (int64_t)token * qpe_ts +
                                 (int64_t)head * qpe_hs + 2 * i;
    const ushort2v ab = *reinterpret_cast<const ushort2v*>(src);
    ushort2v o;
    uint16_t o1, o2;
    rope_rotate(bf16_bits_to_float(ab[0]), bf16_bits_to_float(ab[1]), cs[i],
                cs[MLA_ROPE / 2 + i], o1, o2);
    o[0] = o1;
    o[1] = o2;
    bf16* d = is_k ? dst + MLA_LAT + 2 * i
                   : q_pe + (int64_t)token * qpe_ts + (int64_t)head * qpe_hs +
                         2 * i;
    *reinterpret_cast<ushort2v*>(d) = o;
  }
}

}  // namespace arks

using namespace arks;

extern "C" void arks_attn_mla_paged(
    void* out, void* part_out, const void* q_lat, const void* q_pe,
    const void* cache, const void* block_tables, const void* seq_lens,
    const void* cu_seqlens, float scale, int num_tokens, int num_heads,
    int num_seqs, int max_blocks, int num_blocks, int nparts, int64_t qpe_ts,
    int64_t qpe_hs, hipStream_t stream) {
  if (num_tokens == 0) return;
  dim3 grid((num_heads + 15) / 16, num_tokens, nparts), block(256);
  hipLaunchKernelGGL(attn_mla_kernel, grid, block, 0, stream, (bf16*)out,
                     (float*)part_out, (const bf16*)q_lat, (const bf16*)q_pe,
                     (const bf16*)cache, (const int*)block_tables,
                     (const int*)seq_lens, (const int*)cu_seqlens, scale,
                     num_heads, num_seqs, max_blocks, num_blocks, qpe_ts,
                     qpe_hs);
  if (nparts > 1) {
    dim3 cgrid(num_tokens, num_heads), cblock(128);
    hipLaunchKernelGGL(attn_mla_combine_kernel, cgrid, cblock, 0, stream,
                       (bf16*)out, (const float*)part_out, num_heads, nparts);
  }
}

extern "C" void arks_mla_rope_cache(
    const void* positions, const void* kv_a, const void* norm_weight,
    void* q_pe, const void* cos_sin, void* cache, const void* slot_mapping,
    float eps, int num_tokens, int num_heads, int64_t kv_stride,
    int64_t qpe_ts, int64_t qpe_hs, hipStream_t stream) {
  if (num_tokens == 0) return;
  hipLaunchKernelGGL(mla_rope_cache_kernel, dim3(num_tokens), dim3(256), 0,
                     stream, (const int64_t*)positions, (const bf16*)kv_a,
                     (const bf16*)norm_weight, (bf16*)q_pe,
                     (const float*)cos_sin, (bf16*)cache,
                     (const int64_t*)slot_mapping, eps, num_heads, kv_stride,
                     qpe_ts, qpe_hs);
}
