// Paged KV-cache scatter: write the new tokens' K/V into their assigned slots.
// Cache layout: [num_blocks, num_kv_heads, block_size, head_dim] bf16
// slot = block_id * block_size + offset  (flat, per token)
#include "common.h"

#include <hip/hip_fp8.h>

namespace arks {

__global__ void reshape_and_cache_kernel(
    const bf16* __restrict__ k,  // [T, Hkv, D], token rows strided
    const bf16* __restrict__ v,
    bf16* __restrict__ k_cache,  // [B, Hkv, block_size, D]
    bf16* __restrict__ v_cache,
    const int64_t* __restrict__ slot_mapping,  // [T]
    const int num_kv_heads, const int head_dim, const int block_size,
    const int64_t kv_stride) {
  const int token = blockIdx.x;
  const int64_t slot = slot_mapping[token];
  if (slot < 0) return;  // padding slot
  const int64_t block_id = slot / block_size;
  const int offset = (int)(slot % block_size);
  const int nvec = num_kv_heads * head_dim / 8;
  const bf16* k_src = k + (int64_t)token * kv_stride;
  const bf16* v_src = v + (int64_t)token * kv_stride;
  for (int i = threadIdx.x; i < nvec; i += blockDim.x) {
    const int h = (i * 8) / head_dim;
    const int d = (i * 8) % head_dim;
    const int64_t dst = ((block_id * num_kv_heads + h) * block_size + offset) *
                            head_dim + d;
    *reinterpret_cast<ushort8*>(k_cache + dst) =
        *reinterpret_cast<const ushort8*>(k_src + i * 8);
    *reinterpret_cast<ushort8*>(v_cache + dst) =
        *reinterpret_cast<const ushort8*>(v_src + i * 8);
  }
}

__global__ void reshape_and_cache_fp8_kernel(
    const bf16* __restrict__ k,  // [T, Hkv, D], token rows strided
    const bf16* __restrict__ v,
    uint8_t* __restrict__ k_cache,  // [B, Hkv, block_size, D] e4m3
    uint8_t* __restrict__ v_cache,
    const int64_t* __restrict__ slot_mapping,  // [T]
    const int num_kv_heads, const int head_dim, const int block_size,
    const int64_t kv_stride) {
  const int token = blockIdx.x;
  const int64_t slot = slot_mapping[token];
  if (slot < 0) return;  // padding slot
  const int64_t block_id = slot / block_size;
  const int offset = (int)(slot % block_size);
  const int nvec = num_kv_heads * head_dim / 8;
  const bf16* k_src = k + (int64_t)token * kv_stride;
  const bf16* v_src = v + (int64_t)token * kv_stride;
  for (int i = threadIdx.x; i < nvec; i += blockDim.x) {
    const int h = (i * 8) / head_dim;
    const int d = (i * 8) % head_dim;
    const int64_t dst = ((block_id * num_kv_heads + h) * block_size + offset) *
                            head_dim + d;
    ushort8 kv8 = *reinterpret_cast<const ushort8*>(k_src + i * 8);
    ushort8 vv8 = *reinterpret_cast<const ushort8*>(v_src + i * 8);
    uchar8 ko, vo;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      __hip_fp8_e4m3 kq(bf16_bits_to_float(kv8[e]));
      __hip_fp8_e4m3 vq(bf16_bits_to_float(vv8[e]));
      ko[e] = kq.__x;
      vo[e] = vq.__x;
    }
    *reinterpret_cast<uchar8*>(k_cache + dst) = ko;
    *reinterpret_cast<uchar8*>(v_cache + dst) = vo;
  }
}

}  // namespace arks

using namespace arks;

extern "C" void arks_reshape_and_cache_fp8(
    const void* k, const void* v, void* k_cache, void* v_cache,
    const void* slot_mapping, int num_tokens, int num_kv_heads, int head_dim,
    int block_size, int64_t kv_stride, hipStream_t stream) {
  if (num_tokens == 0) return;
  int threads = std::min(256, num_kv_heads * head_dim / 8);
  hipLaunchKernelGGL(reshape_and_cache_fp8_kernel, dim3(num_tokens),
                     dim3(threads), 0, stream, (const bf16*)k, (const bf16*)v,
                     (uint8_t*)k_cache, (uint8_t*)v_cache,
                     (const int64_t*)slot_mapping, num_kv_heads, head_dim,
                     block_size, kv_stride);
}

extern "C" void arks_reshape_and_cache(const void* k, const void* v,
                                       void* k_cache, void* v_cache,
                                       const void* slot_mapping, int num_tokens,
                                       int num_kv_heads, int head_dim,
                                       int block_size, int64_t kv_stride,
                                       hipStream_t stream) {
  if (num_tokens == 0) return;
  int threads = std::min(256, num_kv_heads * head_dim / 8);
  hipLaunchKernelGGL(reshape_and_cache_kernel, dim3(num_tokens), dim3(threads),
                     0, stream, (const bf16*)k, (const bf16*)v, (bf16*)k_cache,
                     (bf16*)v_cache, (const int64_t*)slot_mapping, num_kv_heads,
                     head_dim, block_size, kv_stride);
}

namespace arks {

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
  const int64_t slot = slot_mapping[token];
  const bool cache = slot >= 0;
  const int64_t block_id = cache ? slot / block_size : 0;
  const int offset = cache ? (int)(slot % block_size) : 0;
  const int64_t cbase =
      (block_id * num_kv_heads) * (int64_t)block_size * head_dim +
      (int64_t)offset * head_dim;
  const int64_t hstride = (int64_t)block_size * head_dim;

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
      const float c = cs[p2 + j];
      const float s = cs[half + p2 + j];
      const float a = bf16_bits_to_float(x1[j]);
      const float b = bf16_bits_to_float(x2[j]);
      o1[j] = float_to_bf16_bits(a * c - b * s);
      o2[j] = float_to_bf16_bits(b * c + a * s);
    }
    *reinterpret_cast<ushort2v*>(base + p2) = o1;
    *reinterpret_cast<ushort2v*>(base + half + p2) = o2;
    if (!is_q && cache) {
      const int64_t dst = cbase + (int64_t)(h - num_q_heads) * hstride;
      if constexpr (FP8) {
        uint8_t* kc = reinterpret_cast<uint8_t*>(k_cache);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          // convert from the bf16-ROUNDED values so the cache is
          // bit-identical to the separate rope + reshape_and_cache path
          __hip_fp8_e4m3 a(bf16_bits_to_float(o1[j]));
          __hip_fp8_e4m3 b(bf16_bits_to_float(o2[j]));
          kc[dst + p2 + j] = a.__x;
          kc[dst + half + p2 + j] = b.__x;
        }
      } else {
        bf16* kc = reinterpret_cast<bf16*>(k_cache);
        *reinterpret_cast<ushort2v*>(kc + dst + p2) = o1;
        *reinterpret_cast<ushort2v*>(kc + dst + half + p2) = o2;
      }
    }
  }
  if (!cache) return;
  // v: plain copy into the page (vectorized 8)
  const bf16* v_src = v + (int64_t)token * k_stride;
  const int nvec = num_kv_heads * head_dim / 8;
  for (int i = threadIdx.x; i < nvec; i += blockDim.x) {
    const int h = (i * 8) / head_dim;
    const int d = (i * 8) % head_dim;
    const int64_t dst = cbase + (int64_t)h * hstride + d;
    ushort8 vv8 = *reinterpret_cast<const ushort8*>(v_src + i * 8);
    if constexpr (FP8) {
      uchar8 vo;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        __hip_fp8_e4m3 vq(bf16_bits_to_float(vv8[e]));
        vo[e] = vq.__x;
      }
      *reinterpret_cast<uchar8*>(reinterpret_cast<uint8_t*>(v_cache) + dst) = vo;
    } else {
      *reinterpret_cast<ushort8*>(reinterpret_cast<bf16*>(v_cache) + dst) = vv8;
    }
  }
}

// One rotary pair (a, b) by (c, s), rounded to bf16, with the contraction
// written out: o1 = fma(a, c, -(b*s)), o2 = fma(b, c, a*s). That is the form
// the compiler gives rope_cache_kernel's `a*c - b*s` / `b*c + a*s` (read off
// its ISA); the same expressions inside the partials-reading kernel below
// were contracted the other way round for o2 and then differed from
// rope_cache_kernel in the last bf16 bit about once in 1e5 elements. The
// bit-equality tests at the full decode shapes guard the pairing.
__device__ __forceinline__ void rope_rotate(const float a, const float b,
                                            const float c, const float s,
                                            uint16_t& o1, uint16_t& o2) {
  o1 = float_to_bf16_bits(__builtin_fmaf(a, c, -(b * s)));
  o2 = float_to_bf16_bits(__builtin_fmaf(b, c, a * s));
}

// ---------------------------------------------------------------------------
// rope_cache_kernel whose q/k/v input is still the split-K partials of the
// qkv skinny GEMM (skinny_gemm.hip, layout [split][m][n], n over the fused
// [q | k | v] columns): every element is reduced in split order, biased and
// rounded to bf16 exactly as skinny_combine_kernel would, then rotated and
// cached with rope_cache_kernel's arithmetic — bit-identical outputs without
// the combine launch or the bf16 qkv round trip. Rotated q goes to a dense
// [T, Hq*D] buffer; k and v go ONLY to the paged cache (the decode attention
// kernel reads them from there). One workgroup per token as before, but the
// kernel is bound by the latency of the partial reads (nsplits x 18 KB per
// token at Qwen2.5-7B), so (a) a thread covers four rotary pairs, making the
// loads 16 B, and (b) rotation items and v items share one index space that
// the launcher covers with up to 1024 threads: every thread then makes one
// memory round trip instead of three dependent ones.
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
  const int64_t slot = slot_mapping[token];
  const bool cache = slot >= 0;
  const int64_t block_id = cache ? slot / block_size : 0;
  const int offset = cache ? (int)(slot % block_size) : 0;
  const int64_t cbase =
      (block_id * num_kv_heads) * (int64_t)block_size * head_dim +
      (int64_t)offset * head_dim;
  const int64_t hstride = (int64_t)block_size * head_dim;
  const float* part_row = part + (int64_t)token * n_total;

  // q and k heads are consecutive column blocks of the fused row, so head h
  // of the [q | k] space starts at column h * head_dim; v follows.
  const int quads = half / 4;  // pair-quads per head
  const int nrot_q = num_q_heads * quads;
  // without a cache slot neither k nor v is needed by anyone
  const int nrot = cache ? nrot_q + num_kv_heads * quads : nrot_q;
  const int nvec = cache ? num_kv_heads * head_dim / 8 : 0;
  const int v_col0 = (num_q_heads + num_kv_heads) * head_dim;
  for (int idx = threadIdx.x; idx < nrot + nvec; idx += blockDim.x) {
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
        const int64_t dst = cbase + (int64_t)(h - num_q_heads) * hstride;
        if constexpr (FP8) {
          uint8_t* kc = reinterpret_cast<uint8_t*>(k_cache);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            __hip_fp8_e4m3 a(bf16_bits_to_float(o1[j]));
            __hip_fp8_e4m3 b(bf16_bits_to_float(o2[j]));
            kc[dst + p4 + j] = a.__x;
            kc[dst + half + p4 + j] = b.__x;
          }
        } else {
          bf16* kc = reinterpret_cast<bf16*>(k_cache);
          *reinterpret_cast<ushort4v*>(kc + dst + p4) = o1;
          *reinterpret_cast<ushort4v*>(kc + dst + half + p4) = o2;
        }
      }
    } else {
      // v: reduce + round, straight into the page (vectorized 8)
      const int i = idx - nrot;
      const int h = (i * 8) / head_dim;
      const int d = (i * 8) % head_dim;
      const int64_t dst = cbase + (int64_t)h * hstride + d;
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
      if constexpr (FP8) {
        uchar8 vo;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          __hip_fp8_e4m3 vq(bf16_bits_to_float(vv8[e]));
          vo[e] = vq.__x;
        }
        *reinterpret_cast<uchar8*>(reinterpret_cast<uint8_t*>(v_cache) + dst) =
            vo;
      } else {
        *reinterpret_cast<ushort8*>(reinterpret_cast<bf16*>(v_cache) + dst) =
            vv8;
      }
    }
  }
}

}  // namespace arks

extern "C" void arks_splitk_rope_and_cache(
    const void* positions, const void* part, const void* bias, void* q_out,
    void* k_cache, void* v_cache, const void* slot_mapping,
    const void* cos_sin, int num_tokens, int head_dim, int num_q_heads,
    int num_kv_heads, int block_size, int nsplits, int mrows_pad, int kv_fp8,
    hipStream_t stream) {
  if (num_tokens == 0) return;
  // one item per thread where the token's work fits (see the kernel comment)
  const int items = (num_q_heads + num_kv_heads) * (head_dim / 8) +
                    num_kv_heads * head_dim / 8;
  dim3 grid(num_tokens), block(std::min(1024, (items + 63) / 64 * 64));
  const int64_t split_stride =
      (int64_t)mrows_pad * (num_q_heads + 2 * num_kv_heads) * head_dim;
  if (kv_fp8) {
    hipLaunchKernelGGL((splitk_rope_cache_kernel<true>), grid, block, 0, stream,
                       (const int64_t*)positions, (const float*)part,
                       (const bf16*)bias, (bf16*)q_out, k_cache, v_cache,
                       (const int64_t*)slot_mapping, (const float*)cos_sin,
                       head_dim, num_q_heads, num_kv_heads, block_size,
                       nsplits, split_stride);
  } else {
    hipLaunchKernelGGL((splitk_rope_cache_kernel<false>), grid, block, 0,
                       stream, (const int64_t*)positions, (const float*)part,
                       (const bf16*)bias, (bf16*)q_out, k_cache, v_cache,
                       (const int64_t*)slot_mapping, (const float*)cos_sin,
                       head_dim, num_q_heads, num_kv_heads, block_size,
                       nsplits, split_stride);
  }
}

extern "C" void arks_rope_and_cache(
    const void* positions, void* q, void* k, const void* v, void* k_cache,
    void* v_cache, const void* slot_mapping, const void* cos_sin,
    int num_tokens, int head_dim, int num_q_heads, int num_kv_heads,
    int block_size, int64_t q_stride, int64_t k_stride, int kv_fp8,
    hipStream_t stream) {
  if (num_tokens == 0) return;
  dim3 grid(num_tokens), block(256);
  if (kv_fp8) {
    hipLaunchKernelGGL((rope_cache_kernel<true>), grid, block, 0, stream,
                       (const int64_t*)positions, (bf16*)q, (bf16*)k,
                       (const bf16*)v, k_cache, v_cache,
                       (const int64_t*)slot_mapping, (const float*)cos_sin,
                       head_dim, num_q_heads, num_kv_heads, block_size,
                       q_stride, k_stride);
  } else {
    hipLaunchKernelGGL((rope_cache_kernel<false>), grid, block, 0, stream,
                       (const int64_t*)positions, (bf16*)q, (bf16*)k,
                       (const bf16*)v, k_cache, v_cache,
                       (const int64_t*)slot_mapping, (const float*)cos_sin,
                       head_dim, num_q_heads, num_kv_heads, block_size,
                       q_stride, k_stride);
  }
}
