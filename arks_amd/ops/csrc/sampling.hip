// Sampling kernels: greedy argmax and Gumbel-max categorical sampling.
//
// Gumbel-max: argmax(logits/T + G) with G ~ Gumbel(0,1) is an exact sample
// from softmax(logits/T) — one memory-bound pass over the logits, no
// normalization, no sort. Rows with T == 0 fall back to plain argmax.
// uniform noise is supplied by the caller (torch.rand on the same stream) so
// sampling stays reproducible under torch.manual_seed.
#include "common.h"

#include <algorithm>
#include <cfloat>

namespace arks {

constexpr int SAMPLE_BLOCK = 256;

// One candidate against the running best: higher value wins, equal values go
// to the lower index (matches torch argmax), NaN is never taken. A strict
// order on (value descending, index ascending), so the winner of a row does
// not depend on how the row is cut up or in which order pieces are merged.
__device__ __forceinline__ void sample_take(float v, int idx, float& best,
                                            int& best_idx) {
  if (v > best || (v == best && idx < best_idx)) {
    best = v;
    best_idx = idx;
  }
}

// The best (value, index) of lrow[begin, end) over the workgroup's 256
// threads; thread 0 returns true and holds the result. begin is a multiple
// of 8. Each thread scans a strided slice, 8-wide where whole vectors are
// left (neither end nor the row stride need be a multiple of 8: the tail is
// handled scalar), then wave shuffles + LDS. Starts from (-FLT_MAX, 0), so
// a slice where nothing is taken (all NaN, all -inf, ...) reports index 0.
template <bool GUMBEL>
__device__ __forceinline__ bool sample_scan(const bf16* __restrict__ lrow,
                                            const float* __restrict__ urow,
                                            const bool greedy,
                                            const float inv_t, const int begin,
                                            const int end, float& best,
                                            int& best_idx) {
  constexpr int BLOCK = SAMPLE_BLOCK;
  best = -FLT_MAX;
  best_idx = 0;
  const int vec0 = begin / 8;
  const int nvec = end / 8;
  for (int i = vec0 + threadIdx.x; i < nvec; i += BLOCK) {
    ushort8 x = *reinterpret_cast<const ushort8*>(lrow + i * 8);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float v = bf16_bits_to_float(x[j]);
      if constexpr (GUMBEL) {
        if (!greedy) {
          float u = urow[i * 8 + j];
          u = fmaxf(u, 1e-20f);
          v = v * inv_t - __logf(-__logf(u));
        }
      }
      sample_take(v, i * 8 + j, best, best_idx);
    }
  }
  for (int idx = nvec * 8 + threadIdx.x; idx < end; idx += BLOCK) {
    float v = bf16_bits_to_float(lrow[idx]);
    if constexpr (GUMBEL) {
      if (!greedy) {
        float u = fmaxf(urow[idx], 1e-20f);
        v = v * inv_t - __logf(-__logf(u));
      }
    }
    sample_take(v, idx, best, best_idx);
  }

#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    float ov = __shfl_xor(best, off, WAVE_SIZE);
    int oi = __shfl_xor(best_idx, off, WAVE_SIZE);
    sample_take(ov, oi, best, best_idx);
  }
  __shared__ float sval[BLOCK / WAVE_SIZE];
  __shared__ int sidx[BLOCK / WAVE_SIZE];
  const int wave = threadIdx.x / WAVE_SIZE;
  if (threadIdx.x % WAVE_SIZE == 0) {
    sval[wave] = best;
    sidx[wave] = best_idx;
  }
  __syncthreads();
  if (threadIdx.x != 0) return false;
  best = sval[0];
  best_idx = sidx[0];
#pragma unroll
  for (int w = 1; w < BLOCK / WAVE_SIZE; ++w)
    sample_take(sval[w], sidx[w], best, best_idx);
  return true;
}

// grid = (rows, chunks): workgroup (row, c) scans tokens [c * chunk_len,
// (c + 1) * chunk_len) of its row (chunk_len a multiple of 8). With one
// chunk it writes out[row]; otherwise its (value, index) pair goes to
// pairs[row][c] and sample_merge_kernel picks the row's winner. One
// workgroup per row leaves most of the chip idle at decode batch sizes
// (64 rows of 304 KB on 256 CUs); rows x chunks covers it.
template <bool GUMBEL>
__global__ __launch_bounds__(SAMPLE_BLOCK) void sample_kernel(
    int64_t* __restrict__ out,
    int2* __restrict__ pairs,  // [rows, chunks] (chunks > 1)
    const bf16* __restrict__ logits,  // [rows, vocab]
    const float* __restrict__ temperatures,  // null if !GUMBEL
    const float* __restrict__ uniform,  // [rows, vocab]
    const int vocab, const int chunk_len) {
  const int row = blockIdx.x;
  const bf16* lrow = logits + (int64_t)row * vocab;
  float inv_t = 0.f;
  bool greedy = true;
  if constexpr (GUMBEL) {
    const float t = temperatures[row];
    greedy = (t <= 0.f);
    inv_t = greedy ? 1.f : 1.f / t;
  }
  const float* urow = GUMBEL ? uniform + (int64_t)row * vocab : nullptr;

  // chunks * chunk_len may overshoot vocab by a chunk or more: such a chunk
  // is empty and reports the initial pair
  const int begin =
      (int)std::min<int64_t>((int64_t)blockIdx.y * chunk_len, vocab);
  const int end = (int)std::min<int64_t>((int64_t)begin + chunk_len, vocab);
  float best;
  int best_idx;
  if (!sample_scan<GUMBEL>(lrow, urow, greedy, inv_t, begin, end, best,
                           best_idx))
    return;
  if (gridDim.y == 1)
    out[row] = best_idx;
  else
    pairs[(int64_t)row * gridDim.y + blockIdx.y] =
        make_int2(__float_as_int(best), best_idx);
}

// Second stage of a chunked launch: one thread per row folds the row's
// pairs in chunk order with the same predicate, from the same initial pair.
// A launch of its own, not a last-arriver counter in the first stage: it
// needs no cross-workgroup ordering. The pairs are loaded sixteen at a time
// ahead of the fold (one memory round trip at the decode chunk count, not
// one per pair); a batch that runs past the row takes its last pair again,
// which the strict predicate ignores.
__global__ __launch_bounds__(64) void sample_merge_kernel(
    int64_t* __restrict__ out, const int2* __restrict__ pairs, const int rows,
    const int chunks) {
  const int row = blockIdx.x * 64 + threadIdx.x;
  if (row >= rows) return;
  float best = -FLT_MAX;
  int best_idx = 0;
  constexpr int BATCH = 16;
  const int2* prow = pairs + (int64_t)row * chunks;
  for (int c = 0; c < chunks; c += BATCH) {
    int2 p[BATCH];
#pragma unroll
    for (int j = 0; j < BATCH; ++j) p[j] = prow[min(c + j, chunks - 1)];
#pragma unroll
    for (int j = 0; j < BATCH; ++j)
      sample_take(__int_as_float(p[j].x), p[j].y, best, best_idx);
  }
  out[row] = best_idx;
}

// ---------------------------------------------------------------------------
// Masked variants (structured outputs). masks is [slots, words] with
// words = ceil(vocab / 32); bit (t % 32) of word (t / 32) is 1 when token t
// is allowed. mask_row[row] picks the mask of a row; -1 = unconstrained.
//
// The launch shape of sample_kernel at one chunk (one 256-thread workgroup per
// row; the masked kernels are not chunked), but
// each wave owns tiles of 64 mask words = 256 logit vectors: lane L loads
// word L of the tile once, then the wave issues four fully coalesced 16-byte
// logit loads and fetches the word of each from lane k*16 + L/4 by shuffle.
// So one mask load per four logit loads and no per-token mask traffic.
// Tokens are only ever visited at idx < vocab, so the unused high bits of
// the last word are never looked at.
// ---------------------------------------------------------------------------
constexpr int NO_TOKEN = 0x7fffffff;

__device__ __forceinline__ void masked_take(float v, int idx, float& best,
                                            int& best_idx, bool allowed = true) {
  // best starts at -inf / NO_TOKEN, so an allowed -inf logit still wins
  // over "nothing"; NaN never compares true, like sample_kernel. Written
  // as selects: a branch per token costs more than the scan itself.
  const bool take =
      allowed & ((v > best) | ((v == best) & (idx < best_idx)));
  best = take ? v : best;
  best_idx = take ? idx : best_idx;
}

template <bool GUMBEL>
__global__ void sample_masked_kernel(int64_t* __restrict__ out,
                                     const bf16* __restrict__ logits,
                                     const float* __restrict__ temperatures,
                                     const float* __restrict__ uniform,
                                     const uint32_t* __restrict__ masks,
                                     const int* __restrict__ mask_row,
                                     const int vocab, const int words,
                                     const int slots) {
  constexpr int BLOCK = 256;
  constexpr int WAVES = BLOCK / WAVE_SIZE;
  const int row = blockIdx.x;
  const int mr = mask_row[row];
  if (mr >= slots) {  // never index outside the pool
    if (threadIdx.x == 0) out[row] = -1;
    return;
  }
  const bool constrained = mr >= 0;
  const uint32_t* mrow = constrained ? masks + (int64_t)mr * words : nullptr;
  const bf16* lrow = logits + (int64_t)row * vocab;
  float inv_t = 0.f;
  bool greedy = true;
  if constexpr (GUMBEL) {
    const float t = temperatures[row];
    greedy = (t <= 0.f);
    inv_t = greedy ? 1.f : 1.f / t;
  }
  const float* urow = GUMBEL ? uniform + (int64_t)row * vocab : nullptr;

  float best = -INFINITY;
  int best_idx = NO_TOKEN;
  const int lane = threadIdx.x % WAVE_SIZE;
  const int wave = threadIdx.x / WAVE_SIZE;
  // 16-byte loads need a 16-byte aligned row (vocab % 8 != 0 shifts later
  // rows); otherwise the whole row goes through the scalar loop.
  const bool aligned = (reinterpret_cast<uintptr_t>(lrow) & 15) == 0;
  const int nvec = aligned ? vocab / 8 : 0;
  const int ntiles = (nvec + 4 * WAVE_SIZE - 1) / (4 * WAVE_SIZE);
  // The mask word of the next tile is fetched while this one is scanned,
  // and the four logit loads are issued together before any is used, so a
  // tile costs one memory latency, not mask-then-logits back to back. A
  // vector whose eight bits are all clear is never loaded at all.
  auto load_mask = [&](int tile) -> uint32_t {
    if (!constrained) return 0xffffffffu;
    const int w = tile * WAVE_SIZE + lane;
    return (tile < ntiles && w < words) ? mrow[w] : 0u;
  };
  uint32_t next = load_mask(wave);
  for (int tile = wave; tile < ntiles; tile += WAVES) {
    const uint32_t mine = next;
    uint32_t bits[4];
    ushort8 x[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t word =
          (uint32_t)__shfl((int)mine, k * 16 + (lane >> 2), WAVE_SIZE);
      const int i = tile * 4 * WAVE_SIZE + k * WAVE_SIZE + lane;
      bits[k] = i < nvec ? (word >> ((lane & 3) * 8)) & 0xffu : 0u;
      if (bits[k] != 0u)
        x[k] = *reinterpret_cast<const ushort8*>(lrow + i * 8);
    }
    next = load_mask(tile + WAVES);  // in flight together with the logits
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (bits[k] == 0u) continue;
      const int i = tile * 4 * WAVE_SIZE + k * WAVE_SIZE + lane;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float v = bf16_bits_to_float(x[k][j]);
        if constexpr (GUMBEL) {
          if (!greedy) {
            float u = urow[i * 8 + j];
            u = fmaxf(u, 1e-20f);
            v = v * inv_t - __logf(-__logf(u));
          }
        }
        masked_take(v, i * 8 + j, best, best_idx, (bits[k] >> j) & 1u);
      }
    }
  }
  for (int idx = nvec * 8 + threadIdx.x; idx < vocab; idx += BLOCK) {
    if (constrained && !((mrow[idx >> 5] >> (idx & 31)) & 1u)) continue;
    float v = bf16_bits_to_float(lrow[idx]);
    if constexpr (GUMBEL) {
      if (!greedy) {
        float u = fmaxf(urow[idx], 1e-20f);
        v = v * inv_t - __logf(-__logf(u));
      }
    }
    masked_take(v, idx, best, best_idx);
  }

#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    float ov = __shfl_xor(best, off, WAVE_SIZE);
    int oi = __shfl_xor(best_idx, off, WAVE_SIZE);
    masked_take(ov, oi, best, best_idx);
  }
  __shared__ float sval[WAVES];
  __shared__ int sidx[WAVES];
  if (lane == 0) {
    sval[wave] = best;
    sidx[wave] = best_idx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float b = sval[0];
    int bi = sidx[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) masked_take(sval[w], sidx[w], b, bi);
    // nothing taken: an empty mask reports -1; an unconstrained row (all
    // NaN) reports 0 like sample_kernel
    out[row] = bi == NO_TOKEN ? (constrained ? -1 : 0) : bi;
  }
}

// In place: logits[row, t] = -inf where the bit of t is clear. grid =
// (rows, ceil(vocab / 2048)); a thread owns 8 consecutive tokens, which lie
// in one mask word. Rows with mask_row -1 are not touched at all.
template <typename T>
__global__ void apply_bitmask_kernel(T* __restrict__ logits,
                                     const uint32_t* __restrict__ masks,
                                     const int* __restrict__ mask_row,
                                     const int vocab, const int words,
                                     const int slots, const T neg_inf) {
  const int row = blockIdx.x;
  const int mr = mask_row[row];
  if (mr < 0 || mr >= slots) return;
  const int idx0 = (blockIdx.y * 256 + threadIdx.x) * 8;
  if (idx0 >= vocab) return;
  const uint32_t word = masks[(int64_t)mr * words + (idx0 >> 5)];
  const uint32_t bits = (word >> (idx0 & 31)) & 0xffu;
  if (bits == 0xffu) return;
  T* lrow = logits + (int64_t)row * vocab;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if (idx0 + j < vocab && !((bits >> j) & 1u)) lrow[idx0 + j] = neg_inf;
  }
}

}  // namespace arks

using namespace arks;

// chunks = workgroups per row (>= 1); pairs = workspace of rows * chunks
// (value, index) pairs, 8 bytes each, unused when chunks == 1.
template <bool GUMBEL>
static void launch_sample(void* out, void* pairs, const void* logits,
                          const void* temperatures, const void* uniform,
                          int rows, int vocab, int chunks,
                          hipStream_t stream) {
  chunks = std::max(chunks, 1);
  // a multiple of 8, so that every chunk starts on a vector of its row
  const int chunk_len =
      chunks == 1 ? vocab : ((vocab + chunks - 1) / chunks + 7) / 8 * 8;
  hipLaunchKernelGGL((sample_kernel<GUMBEL>), dim3(rows, chunks),
                     dim3(SAMPLE_BLOCK), 0, stream, (int64_t*)out,
                     (int2*)pairs, (const bf16*)logits,
                     (const float*)temperatures, (const float*)uniform, vocab,
                     chunk_len);
  if (chunks > 1)
    hipLaunchKernelGGL(sample_merge_kernel, dim3((rows + 63) / 64), dim3(64),
                       0, stream, (int64_t*)out, (const int2*)pairs, rows,
                       chunks);
}

extern "C" {

void arks_greedy_sample_masked(void* out, const void* logits,
                               const void* masks, const void* mask_row,
                               int rows, int vocab, int slots,
                               hipStream_t stream) {
  hipLaunchKernelGGL((sample_masked_kernel<false>), dim3(rows), dim3(256), 0,
                     stream, (int64_t*)out, (const bf16*)logits, nullptr,
                     nullptr, (const uint32_t*)masks, (const int*)mask_row,
                     vocab, (vocab + 31) / 32, slots);
}

void arks_gumbel_sample_masked(void* out, const void* logits,
                               const void* temperatures, const void* uniform,
                               const void* masks, const void* mask_row,
                               int rows, int vocab, int slots,
                               hipStream_t stream) {
  hipLaunchKernelGGL((sample_masked_kernel<true>), dim3(rows), dim3(256), 0,
                     stream, (int64_t*)out, (const bf16*)logits,
                     (const float*)temperatures, (const float*)uniform,
                     (const uint32_t*)masks, (const int*)mask_row, vocab,
                     (vocab + 31) / 32, slots);
}

void arks_apply_token_bitmask(void* logits, int is_fp32, const void* masks,
                              const void* mask_row, int rows, int vocab,
                              int slots, hipStream_t stream) {
  const dim3 grid(rows, (vocab + 2047) / 2048);
  const int words = (vocab + 31) / 32;
  if (is_fp32) {
    hipLaunchKernelGGL((apply_bitmask_kernel<float>), grid, dim3(256), 0,
                       stream, (float*)logits, (const uint32_t*)masks,
                       (const int*)mask_row, vocab, words, slots, -INFINITY);
  } else {
    // bf16 -inf is 0xff80
    hipLaunchKernelGGL((apply_bitmask_kernel<uint16_t>), grid, dim3(256), 0,
                       stream, (uint16_t*)logits, (const uint32_t*)masks,
                       (const int*)mask_row, vocab, words, slots,
                       (uint16_t)0xff80);
  }
}

void arks_greedy_sample(void* out, void* pairs, const void* logits, int rows,
                        int vocab, int chunks, hipStream_t stream) {
  launch_sample<false>(out, pairs, logits, nullptr, nullptr, rows, vocab,
                       chunks, stream);
}

void arks_gumbel_sample(void* out, void* pairs, const void* logits,
                        const void* temperatures, const void* uniform,
                        int rows, int vocab, int chunks, hipStream_t stream) {
  launch_sample<true>(out, pairs, logits, temperatures, uniform, rows, vocab,
                      chunks, stream);
}

}  // extern "C"
