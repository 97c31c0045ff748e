// Paged KV-cache addressing and stores shared by every cache writer
// (kvcache.hip). Cache layout: [num_blocks, num_kv_heads, block_size,
// head_dim], bf16 or OCP e4m3 (scale 1.0);
// slot = block_id * block_size + offset (flat, per token).
#pragma once

#include "common.h"

#include <hip/hip_fp8.h>

namespace arks {

// Where a token's slot lives in the cache: element (h, d) of the token is at
// base + h * hstride + d. slot < 0 is a padding row: valid is false and the
// page is block 0 / offset 0, which the caller must not write.
struct CachePage {
  bool valid;
  int64_t base;
  int64_t hstride;
};

__device__ __forceinline__ CachePage cache_page(const int64_t slot,
                                                const int num_kv_heads,
                                                const int block_size,
                                                const int head_dim) {
  CachePage pg;
  pg.valid = slot >= 0;
  const int64_t block_id = pg.valid ? slot / block_size : 0;
  const int offset = pg.valid ? (int)(slot % block_size) : 0;
  pg.base = (block_id * num_kv_heads) * (int64_t)block_size * head_dim +
            (int64_t)offset * head_dim;
  pg.hstride = (int64_t)block_size * head_dim;
  return pg;
}

// Store a vector V of 2, 4 or 8 bf16 values (ushort2v / ushort4v / ushort8)
// at element idx of a cache: as they are into a bf16 cache, converted to
// e4m3 (hardware cvt) into an fp8 one — one vector store either way. The
// conversion starts from the bf16-ROUNDED value, so a writer that has just
// rounded its result caches the same byte as one that re-reads the bf16
// tensor. idx must be a multiple of the vector length.
template <bool FP8, typename V>
__device__ __forceinline__ void cache_store(void* __restrict__ cache,
                                            const int64_t idx, const V v) {
  constexpr int N = sizeof(V) / sizeof(uint16_t);
  if constexpr (FP8) {
    typedef __attribute__((ext_vector_type(N))) uint8_t U;
    U o;
#pragma unroll
    for (int e = 0; e < N; ++e) {
      __hip_fp8_e4m3 q(bf16_bits_to_float(v[e]));
      o[e] = q.__x;
    }
    *reinterpret_cast<U*>(reinterpret_cast<uint8_t*>(cache) + idx) = o;
  } else {
    *reinterpret_cast<V*>(reinterpret_cast<bf16*>(cache) + idx) = v;
  }
}

}  // namespace arks
