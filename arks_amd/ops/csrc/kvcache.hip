// Paged KV-cache writers: scatter the new tokens' K/V into their assigned
// slots, alone or fused with RoPE (and with the split-K reduction of the qkv
// GEMM). Cache layout, slot addressing and the bf16 / e4m3 stores are in
// kv_store.h; the rotation is rope_rotate (common.h).
#include "kv_store.h"

#include <type_traits>

namespace arks {

template <bool FP8>
__global__ void reshape_and_cache_kernel(
    const bf16* __restrict__ k,  // [T, Hkv, D], token rows strided
    const bf16* __restrict__ v,
    void* __restrict__ k_cache,  // [B, Hkv, block_size, D] bf16 or e4m3
    void* __restrict__ v_cache,
    const int64_t* __restrict__ slot_mapping,  // [T]
    const int num_kv_heads, const int head_dim, const int block_size,
    const int64_t kv_stride) {
  const int token = blockIdx.x;
  const CachePage pg =
      cache_page(slot_mapping[token], num_kv_heads, block_size, head_dim);
  if (!pg.valid) return;  // padding slot
  const int nvec = num_kv_heads * head_dim / 8;
  const bf16* k_src = k + (int64_t)token * kv_stride;
  const bf16* v_src = v + (int64_t)token * kv_stride;
  for (int i = threadIdx.x; i < nvec; i += blockDim.x) {
    const int h = (i * 8) / head_dim;
    const int d = (i * 8) % head_dim;
    const int64_t dst = pg.base + (int64_t)h * pg.hstride + d;
    cache_store<FP8>(k_cache, dst,
                     *reinterpret_cast<const ushort8*>(k_src + i * 8));
    cache_store<FP8>(v_cache, dst,
                     *reinterpret_cast<const ushort8*>(v_src + i * 8));
  }
}

// ---------------------------------------------------------------------------
// Fused RoPE + cache write: rotate q/k in place AND scatter the rotated k
// (plus v) into the paged cache in one launch — the separate
// rope_kernel + reshape_and_cache pair cost a kernel boundary and a full
// re-read of k every layer on the decode path. The rotating thread already
// holds the rotated k values in registers, so the cache store is free.
// Thread space: [q heads | kv heads] x pair-couples for the rotation, then
// the v copy strided over the same block.
// ---------------------------------------------------------------------------
template <bool FP8>
__global__ void rope_cache_kernel(
    const int64_t* __restrict__ positions,
    bf16* __restrict__ q,        // [T, Hq*D] rows strided
    bf16* __restrict__ k,        // [T, Hkv*D] rows strided
    const bf16* __restrict__ v,  // [T, Hkv*D] rows strided (k_stride)
    void* __restrict__ k_cache,  // [B, Hkv, block_size, D] bf16 or e4m3
    void* __restrict__ v_cache,
    const int64_t* __restrict__ slot_mapping,  // [T] (-1 = no cache write)
    const float* __restrict__ cos_sin,         // [max_pos, D]
    const int head_dim, const int num_q_heads, const int num_kv_heads,
    const int block_size, const int64_t q_stride, const int64_t k_stride) {
  const int token = blockIdx.x;
  const int half = head_dim / 2;
  const int64_t pos = positions[token];
  const float* cs = cos_sin + pos * head_dim;
  const CachePage pg =
      cache_page(slot_mapping[token], num_kv_heads, block_size, head_dim);

  const int total_heads = num_q_heads + num_kv_heads;
  const int pairs2 = half / 2;
  for (int idx = threadIdx.x; idx < total_heads * pairs2; idx += blockDim.x) {
    const int h = idx / pairs2;
    const int p2 = (idx % pairs2) * 2;
    const bool is_q = h < num_q_heads;
    bf16* base = is_q
                     ? q + (int64_t)token * q_stride + (int64_t)h * head_dim
                     : k + (int64_t)token * k_stride +
                           (int64_t)(h - num_q_heads) * head_dim;
    ushort2v x1 = *reinterpret_cast<const ushort2v*>(base + p2);
    ushort2v x2 = *reinterpret_cast<const ushort2v*>(base + half + p2);
    ushort2v o1, o2;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      uint16_t r1, r2;
      rope_rotate(bf16_bits_to_float(x1[j]), bf16_bits_to_float(x2[j]),
                  cs[p2 + j], cs[half + p2 + j], r1, r2);
      o1[j] = r1;
      o2[j] = r2;
    }
    *reinterpret_cast<ushort2v*>(base + p2) = o1;
    *reinterpret_cast<ushort2v*>(base + half + p2) = o2;
    if (!is_q && pg.valid) {
      const int64_t dst = pg.base + (int64_t)(h - num_q_heads) * pg.hstride;
      cache_store<FP8>(k_cache, dst + p2, o1);
      cache_store<FP8>(k_cache, dst + half + p2, o2);
    }
  }
  if (!pg.valid) return;
  // v: plain copy into the page (vectorized 8)
  const bf16* v_src = v + (int64_t)token * k_stride;
  const int nvec = num_kv_heads * head_dim / 8;
  for (int i = threadIdx.x; i < nvec; i += blockDim.x) {
    const int h = (i * 8) / head_dim;
    const int d = (i * 8) % head_dim;
    cache_store<FP8>(v_cache, pg.base + (int64_t)h * pg.hstride + d,
                     *reinterpret_cast<const ushort8*>(v_src + i * 8));
  }
}

// ---------------------------------------------------------------------------
// rope_cache_kernel whose q/k/v input is still the split-K partials of the
// qkv skinny GEMM (skinny_gemm.hip, layout [split][m][n], n over the fused
// [q | k | v] columns): every element is reduced in split order, biased and
// rounded to bf16 exactly as skinny_combine_kernel would, then rotated and
// cached with rope_cache_kernel's arithmetic — bit-identical outputs without
// the combine launch or the bf16 qkv round trip. Rotated q goes to a dense
// [T, Hq*D] buffer; k and v go ONLY to the paged cache (the decode attention
// kernel reads them from there). The kernel is bound by the latency of the
// partial reads (nsplits x 18 KB per token at Qwen2.5-7B), so (a) a thread
// covers four rotary pairs, making the loads 16 B, and (b) rotation items and
// v items share one index space that the launcher covers with up to 1024
// threads per token: every thread then makes one memory round trip instead
// of three dependent ones. grid = (tokens, groups): the groups of a token
// share its index space (no item needs another, so any grouping gives the
// same bits), which spreads a decode batch of fewer tokens than compute
// units over the chip instead of pulling a token's partials through one CU.
// ---------------------------------------------------------------------------
template <bool FP8>
__global__ __launch_bounds__(1024) void splitk_rope_cache_kernel(
    const int64_t* __restrict__ positions,
    const float* __restrict__ part,  // [nsplits][mrows][(Hq + 2*Hkv) * D]
    const bf16* __restrict__ bias,   // [(Hq + 2*Hkv) * D] or null
    bf16* __restrict__ q_out,        // [T, Hq*D]
    void* __restrict__ k_cache,      // [B, Hkv, block_size, D] bf16 or e4m3
    void* __restrict__ v_cache,
    const int64_t* __restrict__ slot_mapping,  // [T] (-1 = no cache write)
    const float* __restrict__ cos_sin,         // [max_pos, D]
    const int head_dim, const int num_q_heads, const int num_kv_heads,
    const int block_size, const int nsplits, const int64_t split_stride) {
  const int token = blockIdx.x;
  const int half = head_dim / 2;
  const int n_total = (num_q_heads + 2 * num_kv_heads) * head_dim;
  const int64_t pos = positions[token];
  const float* cs = cos_sin + pos * head_dim;
  const CachePage pg =
      cache_page(slot_mapping[token], num_kv_heads, block_size, head_dim);
  const float* part_row = part + (int64_t)token * n_total;

  // q and k heads are consecutive column blocks of the fused row, so head h
  // of the [q | k] space starts at column h * head_dim; v follows.
  const int quads = half / 4;  // pair-quads per head
  const int nrot_q = num_q_heads * quads;
  // without a cache slot neither k nor v is needed by anyone
  const int nrot = pg.valid ? nrot_q + num_kv_heads * quads : nrot_q;
  const int nvec = pg.valid ? num_kv_heads * head_dim / 8 : 0;
  const int v_col0 = (num_q_heads + num_kv_heads) * head_dim;
  for (int idx = blockIdx.y * blockDim.x + threadIdx.x; idx < nrot + nvec;
       idx += blockDim.x * gridDim.y) {
    if (idx < nrot) {
      const int h = idx / quads;
      const int p4 = (idx % quads) * 4;
      const int col = h * head_dim + p4;
      const float* const p[2] = {part_row + col, part_row + col + half};
      float4v acc[2];
      splitk_reduce<2, 1>(p, split_stride, nsplits, acc);
      ushort4v o1, o2;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float af = acc[0][j];
        float bf = acc[1][j];
        if (bias != nullptr) {
          af += bf16_bits_to_float(bias[col + j]);
          bf += bf16_bits_to_float(bias[col + half + j]);
        }
        // the combine's bf16 rounding, then rope_cache_kernel's rotation
        const float a = bf16_bits_to_float(float_to_bf16_bits(af));
        const float b = bf16_bits_to_float(float_to_bf16_bits(bf));
        uint16_t r1, r2;
        rope_rotate(a, b, cs[p4 + j], cs[half + p4 + j], r1, r2);
        o1[j] = r1;
        o2[j] = r2;
      }
      if (h < num_q_heads) {
        bf16* base = q_out + ((int64_t)token * num_q_heads + h) * head_dim;
        *reinterpret_cast<ushort4v*>(base + p4) = o1;
        *reinterpret_cast<ushort4v*>(base + half + p4) = o2;
      } else {
        const int64_t dst = pg.base + (int64_t)(h - num_q_heads) * pg.hstride;
        cache_store<FP8>(k_cache, dst + p4, o1);
        cache_store<FP8>(k_cache, dst + half + p4, o2);
      }
    } else {
      // v: reduce + round, straight into the page (vectorized 8)
      const int i = idx - nrot;
      const int h = (i * 8) / head_dim;
      const int d = (i * 8) % head_dim;
      const int col = v_col0 + i * 8;
      const float* const p[2] = {part_row + col, part_row + col + 4};
      float4v acc[2];
      splitk_reduce<2, 1>(p, split_stride, nsplits, acc);
      ushort8 vv8;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float vf = acc[e / 4][e % 4];
        if (bias != nullptr) vf += bf16_bits_to_float(bias[col + e]);
        vv8[e] = float_to_bf16_bits(vf);
      }
      cache_store<FP8>(v_cache, pg.base + (int64_t)h * pg.hstride + d, vv8);
    }
  }
}

}  // namespace arks

using namespace arks;

// Calls f(std::true_type) for an e4m3 cache, f(std::false_type) for bf16, so
// a launcher names its kernel template once.
template <typename F>
static void dispatch_kv_fp8(int kv_fp8, F&& f) {
  if (kv_fp8)
    f(std::true_type{});
  else
    f(std::false_type{});
}

extern "C" void arks_reshape_and_cache(const void* k, const void* v,
                                       void* k_cache, void* v_cache,
                                       const void* slot_mapping, int num_tokens,
                                       int num_kv_heads, int head_dim,
                                       int block_size, int64_t kv_stride,
                                       int kv_fp8, hipStream_t stream) {
  if (num_tokens == 0) return;
  int threads = std::min(256, num_kv_heads * head_dim / 8);
  dispatch_kv_fp8(kv_fp8, [&](auto fp8) {
    hipLaunchKernelGGL((reshape_and_cache_kernel<decltype(fp8)::value>),
                       dim3(num_tokens), dim3(threads), 0, stream,
                       (const bf16*)k, (const bf16*)v, k_cache, v_cache,
                       (const int64_t*)slot_mapping, num_kv_heads, head_dim,
                       block_size, kv_stride);
  });
}

extern "C" void arks_splitk_rope_and_cache(
    const void* positions, const void* part, const void* bias, void* q_out,
    void* k_cache, void* v_cache, const void* slot_mapping,
    const void* cos_sin, int num_tokens, int head_dim, int num_q_heads,
    int num_kv_heads, int block_size, int nsplits, int mrows_pad, int kv_fp8,
    int groups, hipStream_t stream) {
  if (num_tokens == 0) return;
  // one item per thread where the token's work fits (see the kernel
  // comment), over `groups` workgroups per token
  const int items = (num_q_heads + num_kv_heads) * (head_dim / 8) +
                    num_kv_heads * head_dim / 8;
  groups = std::max(1, std::min(groups, (items + 63) / 64));
  const int per_group = (items + groups - 1) / groups;
  dim3 grid(num_tokens, groups);
  dim3 block(std::min(1024, (per_group + 63) / 64 * 64));
  const int64_t split_stride =
      (int64_t)mrows_pad * (num_q_heads + 2 * num_kv_heads) * head_dim;
  dispatch_kv_fp8(kv_fp8, [&](auto fp8) {
    hipLaunchKernelGGL((splitk_rope_cache_kernel<decltype(fp8)::value>), grid,
                       block, 0, stream, (const int64_t*)positions,
                       (const float*)part, (const bf16*)bias, (bf16*)q_out,
                       k_cache, v_cache, (const int64_t*)slot_mapping,
                       (const float*)cos_sin, head_dim, num_q_heads,
                       num_kv_heads, block_size, nsplits, split_stride);
  });
}

extern "C" void arks_rope_and_cache(
    const void* positions, void* q, void* k, const void* v, void* k_cache,
    void* v_cache, const void* slot_mapping, const void* cos_sin,
    int num_tokens, int head_dim, int num_q_heads, int num_kv_heads,
    int block_size, int64_t q_stride, int64_t k_stride, int kv_fp8,
    hipStream_t stream) {
  if (num_tokens == 0) return;
  dim3 grid(num_tokens), block(256);
  dispatch_kv_fp8(kv_fp8, [&](auto fp8) {
    hipLaunchKernelGGL((rope_cache_kernel<decltype(fp8)::value>), grid, block,
                       0, stream, (const int64_t*)positions, (bf16*)q,
                       (bf16*)k, (const bf16*)v, k_cache, v_cache,
                       (const int64_t*)slot_mapping, (const float*)cos_sin,
                       head_dim, num_q_heads, num_kv_heads, block_size,
                       q_stride, k_stride);
  });
}
