// Batched multi-LoRA kernels for gfx950: y[t] += B[a(t)] . (A[a(t)] . x[t])
// with a different adapter slot a(t) per token of a continuous batch.
//
// Work is described by an int32 tile table [ntiles, 3] of (row0, nrows,
// slot): 1..16 consecutive rows of the packed token batch sharing one slot.
// A tile with slot < 0 (graphed decode keeps a fixed-shape table) or with
// out-of-range fields is skipped by the whole workgroup. Nothing here
// allocates or synchronises, so both launches capture into hipGraphs; there
// are no float atomics, split-K partials combine in wave order.
//
// Both kernels feed __builtin_amdgcn_mfma_f32_16x16x32_bf16 with the
// fragment mapping pinned by tests/test_ops_gpu.py::test_mfma_probe:
//   A operand: lane l holds A[row = l & 15][k = 8 (l >> 4) + j], j = 0..7
//   B operand: lane l holds B[k = 8 (l >> 4) + j][col = l & 15]
//   C/D:       lane l holds D[row = 4 (l >> 4) + reg][col = l & 15]
#include "common.h"

namespace arks {

typedef __attribute__((ext_vector_type(8))) __bf16 lora_bf16x8;
typedef __attribute__((ext_vector_type(4))) float lora_f32x4;

__device__ __forceinline__ lora_f32x4 lora_mfma(lora_bf16x8 a, lora_bf16x8 b,
                                                lora_f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ lora_bf16x8 lora_as_frag(ushort8 v) {
  union {
    ushort8 u;
    lora_bf16x8 b;
  } c;
  c.u = v;
  return c.b;
}

// Decodes and validates one tile; false = the workgroup has nothing to do.
__device__ __forceinline__ bool lora_tile(const int* __restrict__ tiles,
                                          int tile, int T, int max_loras,
                                          int& row0, int& nrows, int& slot) {
  row0 = tiles[tile * 3];
  nrows = tiles[tile * 3 + 1];
  slot = tiles[tile * 3 + 2];
  return slot >= 0 && slot < max_loras && nrows >= 1 && nrows <= 16 &&
         row0 >= 0 && row0 <= T - nrows;
}

constexpr int LORA_WAVES = 4;

// h[row, jb*16 .. jb*16+16) = x[row, :] . A[slot][jb*16 .., :]^T
// grid (ntiles, SR/16), 4 waves; wave w owns a contiguous quarter of the
// K/32 MFMA steps, partial accumulators are summed through LDS in wave order.
__global__ __launch_bounds__(LORA_WAVES* WAVE_SIZE) void lora_shrink_kernel(
    float* __restrict__ h,           // [>=T, SR] f32
    const bf16* __restrict__ x,      // [T, K]
    const bf16* __restrict__ a,      // [max_loras, SR, K]
    const int* __restrict__ tiles,   // [ntiles, 3]
    const int T, const int K, const int SR, const int max_loras) {
  int row0, nrows, slot;
  if (!lora_tile(tiles, blockIdx.x, T, max_loras, row0, nrows, slot)) return;
  const int jb = blockIdx.y;
  const int tid = threadIdx.x;
  const int wave = tid / WAVE_SIZE;
  const int lane = tid % WAVE_SIZE;
  const int lq = lane & 15;
  const int la = lane >> 4;

  const int nsteps = K / 32;
  const int per = (nsteps + LORA_WAVES - 1) / LORA_WAVES;
  const int s0 = wave * per;
  const int s1 = min(nsteps, s0 + per);

  const bool row_ok = lq < nrows;
  const bf16* xp = x + (int64_t)(row0 + (row_ok ? lq : 0)) * K + 8 * la;
  const bf16* ap = a + ((int64_t)slot * SR + jb * 16 + lq) * K + 8 * la;

  lora_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  const ushort8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll 4
  for (int s = s0; s < s1; ++s) {
    const ushort8 xv =
        row_ok ? *reinterpret_cast<const ushort8*>(xp + s * 32) : zero;
    const ushort8 av = *reinterpret_cast<const ushort8*>(ap + s * 32);
    acc = lora_mfma(lora_as_frag(xv), lora_as_frag(av), acc);
  }

  __shared__ float part[LORA_WAVES][256];
#pragma unroll
  for (int r = 0; r < 4; ++r) part[wave][(4 * la + r) * 16 + lq] = acc[r];
  __syncthreads();
  const int row = tid >> 4;
  const int col = tid & 15;
  if (row < nrows) {
    float sum = part[0][tid];
#pragma unroll
    for (int w = 1; w < LORA_WAVES; ++w) sum += part[w][tid];
    h[(int64_t)(row0 + row) * SR + jb * 16 + col] = sum;
  }
}

constexpr int LORA_EXP_CB_PER_WAVE = 4;  // 16-column blocks per wave
constexpr int LORA_EXP_COLS = LORA_WAVES * LORA_EXP_CB_PER_WAVE * 16;

// y[row, n] = bf16(float(y[row, n]) + sum_j h[row, s(n) R + j] B[slot][n, j])
// grid (ntiles, ceil(N / 256)), 4 waves x 4 column blocks of 16. Computed
// transposed (D = B . h^T) so a lane ends up with 4 consecutive columns of
// one token: the read-modify-write of y is one 8-byte load and store.
// h goes f32 -> (hi + lo) bf16 operands, two MFMAs per step, which keeps
// ~16 mantissa bits of the shrink result.
template <int R>
__global__ __launch_bounds__(LORA_WAVES* WAVE_SIZE) void lora_expand_kernel(
    bf16* __restrict__ y,            // [T, N]
    const float* __restrict__ h,     // [>=T, S*R] f32
    const bf16* __restrict__ b,      // [max_loras, N, R]
    const int* __restrict__ tiles,   // [ntiles, 3]
    const int T, const int N, const int S, const int off1, const int off2,
    const int max_loras) {
  int row0, nrows, slot;
  if (!lora_tile(tiles, blockIdx.x, T, max_loras, row0, nrows, slot)) return;
  const int tid = threadIdx.x;
  const int wave = tid / WAVE_SIZE;
  const int lane = tid % WAVE_SIZE;
  const int lq = lane & 15;
  const int la = lane >> 4;
  constexpr int KSTEPS = (R + 31) / 32;
  // R == 16 fills only k = 0..15 of the 32-deep MFMA: lanes with la >= 2
  // supply zeros and load nothing
  const bool k_ok = (R >= 32) || la < 2;
  const bool row_ok = lq < nrows;
  const int SR = S * R;
  const float* hp = h + (int64_t)(row0 + (row_ok ? lq : 0)) * SR + 8 * la;
  const bf16* bp = b + (int64_t)slot * N * R + 8 * la;
  const ushort8 zero = {0, 0, 0, 0, 0, 0, 0, 0};

  int cur_s = -1;
  ushort8 h_hi[KSTEPS], h_lo[KSTEPS];
#pragma unroll
  for (int c = 0; c < LORA_EXP_CB_PER_WAVE; ++c) {
    const int n0 = blockIdx.y * LORA_EXP_COLS +
                   (wave * LORA_EXP_CB_PER_WAVE + c) * 16;
    if (n0 >= N) break;
    const int s = (S > 1 && n0 >= off1) ? ((S > 2 && n0 >= off2) ? 2 : 1) : 0;
    if (s != cur_s) {
      cur_s = s;
#pragma unroll
      for (int ks = 0; ks < KSTEPS; ++ks) {
        h_hi[ks] = zero;
        h_lo[ks] = zero;
        if (k_ok && row_ok) {
          const float4v v0 =
              *reinterpret_cast<const float4v*>(hp + s * R + ks * 32);
          const float4v v1 =
              *reinterpret_cast<const float4v*>(hp + s * R + ks * 32 + 4);
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const float f = j < 4 ? v0[j] : v1[j - 4];
            const uint16_t hi = float_to_bf16_bits(f);
            h_hi[ks][j] = hi;
            h_lo[ks][j] = float_to_bf16_bits(f - bf16_bits_to_float(hi));
          }
        }
      }
    }
    lora_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KSTEPS; ++ks) {
      const ushort8 bv =
          k_ok ? *reinterpret_cast<const ushort8*>(
                     bp + (int64_t)(n0 + lq) * R + ks * 32)
               : zero;
      acc = lora_mfma(lora_as_frag(bv), lora_as_frag(h_lo[ks]), acc);
      acc = lora_mfma(lora_as_frag(bv), lora_as_frag(h_hi[ks]), acc);
    }
    // D[row = n0 + 4 la + r][col = token lq]
    if (row_ok) {
      bf16* yp = y + (int64_t)(row0 + lq) * N + n0 + 4 * la;
      ushort4v yv = *reinterpret_cast<const ushort4v*>(yp);
#pragma unroll
      for (int r = 0; r < 4; ++r)
        yv[r] = float_to_bf16_bits(bf16_bits_to_float(yv[r]) + acc[r]);
      *reinterpret_cast<ushort4v*>(yp) = yv;
    }
  }
}

}  // namespace arks

using namespace arks;

extern "C" void arks_lora_shrink(void* h, const void* x, const void* a,
                                 const void* tiles, int ntiles, int T, int K,
                                 int SR, int max_loras, hipStream_t stream) {
  if (ntiles <= 0) return;
  dim3 grid(ntiles, SR / 16);
  hipLaunchKernelGGL(lora_shrink_kernel, grid, dim3(LORA_WAVES * WAVE_SIZE), 0,
                     stream, (float*)h, (const bf16*)x, (const bf16*)a,
                     (const int*)tiles, T, K, SR, max_loras);
  HIP_CHECK_KERNEL();
}

extern "C" void arks_lora_expand(void* y, const void* h, const void* b,
                                 const void* tiles, int ntiles, int T, int N,
                                 int R, int S, int off1, int off2,
                                 int max_loras, hipStream_t stream) {
  if (ntiles <= 0) return;
  dim3 grid(ntiles, (N + LORA_EXP_COLS - 1) / LORA_EXP_COLS);
  dim3 block(LORA_WAVES * WAVE_SIZE);
#define ARKS_LORA_EXPAND(RANK)                                               \
  hipLaunchKernelGGL(lora_expand_kernel<RANK>, grid, block, 0, stream,       \
                     (bf16*)y, (const float*)h, (const bf16*)b,              \
                     (const int*)tiles, T, N, S, off1, off2, max_loras)
  if (R == 16) {
    ARKS_LORA_EXPAND(16);
  } else if (R == 32) {
    ARKS_LORA_EXPAND(32);
  } else {
    ARKS_LORA_EXPAND(64);
  }
#undef ARKS_LORA_EXPAND
  HIP_CHECK_KERNEL();
}
