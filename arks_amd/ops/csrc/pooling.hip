// Embedding pooling for gfx950: the tail of an embedding model's forward
// (residual add, final RMSNorm, pooling, truncation, L2 normalisation) over
// the packed rows [T, H] of a prefill batch, one f32 vector per segment.
//
// For a segment of rows [a, b):
//   r_i = bf16(x_i + residual_i)              (fused_add_rmsnorm's rounding)
//   y_i = r_i * (1 / sqrt(mean(r_i^2) + eps)) * w      in f32, never rounded
//   last: v = y_{b-1}    cls: v = y_a    mean: v = (carry + sum_i y_i) / count
//   v = v[:dims];  normalize: v /= max(|v|_2, 1e-12)
//
// Two kernels, no atomics, so a vector is bitwise reproducible and does not
// depend on where its rows sit in the packed batch:
//
// pool_slab_kernel (mean only): the host table (ops.build_pool_table) cuts a
//   segment into slabs of ops.POOL_SLAB_ROWS rows at fixed offsets from its
//   first row; one workgroup per slab, so a long sequence spreads over the
//   chip. Each wave owns whole rows (row w, w+4, ... of the slab): it loads
//   x and residual once with 16-byte loads, keeps the row in registers,
//   reduces the sum of squares with wave shuffles (no barrier per row) and
//   adds r * rrms into its f32 column accumulators. The four waves'
//   accumulators are then summed in wave order through LDS and stored as
//   one f32 partial row.
//
// pool_finish_kernel: one workgroup per segment. last/cls read the single
//   row they need (O(segments * H), not O(T * H)) and normalise it; mean
//   sums its slab partials in slab order, applies the norm weight once,
//   adds the carry of earlier prefill chunks and either stores the new carry
//   (non-final chunk) or divides by the token count. Truncation and the L2
//   normalisation happen in the same pass.
#include "common.h"

namespace arks {

constexpr int POOL_BLOCK = 256;
constexpr int POOL_WAVES = POOL_BLOCK / WAVE_SIZE;
// finish kernel: 8 columns x POOL_MAXV vectors per thread
constexpr int POOL_MAXV = 4;
constexpr int POOL_MAX_HIDDEN = POOL_BLOCK * 8 * POOL_MAXV;  // 8192

enum PoolMode { POOL_LAST = 0, POOL_MEAN = 1, POOL_CLS = 2 };
// segment table columns (int32 [S, 8])
enum PoolCol { PC_ROW0 = 0, PC_NROWS, PC_MODE, PC_SLOT, PC_COUNTED, PC_FINAL,
               PC_PART0, PC_NPARTS };

// Eight columns of one row: r = bf16(x + residual) as f32, and ss += r^2.
__device__ __forceinline__ float pool_add8(const ushort8 x, const ushort8 r,
                                           float (&out)[8], float ss) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float v = bf16_bits_to_float(float_to_bf16_bits(
        bf16_bits_to_float(x[j]) + bf16_bits_to_float(r[j])));
    out[j] = v;
    ss += v * v;
  }
  return ss;
}

__device__ __forceinline__ float pool_rrms(const float ss, const int hidden,
                                           const float eps) {
  return 1.0f / sqrtf(ss / (float)hidden + eps);
}

// NV = 16-byte vectors per lane per row: hidden <= 512 * NV.
template <int NV>
__global__ __launch_bounds__(POOL_BLOCK) void pool_slab_kernel(
    float* __restrict__ part,          // [nslabs, hidden]
    const bf16* __restrict__ x, const bf16* __restrict__ residual,
    const int* __restrict__ slabs,     // [nslabs, 4]: row0, nrows, part, -
    const float eps, const int hidden) {
  extern __shared__ float pool_lds[];  // [hidden]
  const int* sl = slabs + blockIdx.x * 4;
  const int row0 = sl[0], nrows = sl[1], pidx = sl[2];
  const int wave = threadIdx.x / WAVE_SIZE;
  const int lane = threadIdx.x % WAVE_SIZE;
  const int nvec = hidden / 8;

  float acc[NV][8];
#pragma unroll
  for (int k = 0; k < NV; ++k)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[k][j] = 0.f;

  for (int r = wave; r < nrows; r += POOL_WAVES) {
    const int64_t off = (int64_t)(row0 + r) * hidden;
    ushort8 xv[NV], rv[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const int i = k * WAVE_SIZE + lane;
      if (i < nvec) {
        xv[k] = *reinterpret_cast<const ushort8*>(x + off + i * 8);
        rv[k] = *reinterpret_cast<const ushort8*>(residual + off + i * 8);
      } else {
        xv[k] = ushort8{0, 0, 0, 0, 0, 0, 0, 0};
        rv[k] = ushort8{0, 0, 0, 0, 0, 0, 0, 0};
      }
    }
    float rf[NV][8];
    float ss = 0.f;
#pragma unroll
    for (int k = 0; k < NV; ++k) ss = pool_add8(xv[k], rv[k], rf[k], ss);
    ss = wave_reduce_sum(ss);  // every lane holds the same bits
    const float rrms = pool_rrms(ss, hidden, eps);
#pragma unroll
    for (int k = 0; k < NV; ++k)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[k][j] += rf[k][j] * rrms;
  }

  // ((w0 + w1) + w2) + w3, one wave's accumulators through LDS at a time
  for (int w = 1; w < POOL_WAVES; ++w) {
    if (wave == w) {
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        const int i = k * WAVE_SIZE + lane;
        if (i < nvec) {
          *reinterpret_cast<float4v*>(pool_lds + i * 8) =
              float4v{acc[k][0], acc[k][1], acc[k][2], acc[k][3]};
          *reinterpret_cast<float4v*>(pool_lds + i * 8 + 4) =
              float4v{acc[k][4], acc[k][5], acc[k][6], acc[k][7]};
        }
      }
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        const int i = k * WAVE_SIZE + lane;
        if (i < nvec) {
          const float4v a = *reinterpret_cast<const float4v*>(pool_lds + i * 8);
          const float4v b =
              *reinterpret_cast<const float4v*>(pool_lds + i * 8 + 4);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            acc[k][j] += a[j];
            acc[k][4 + j] += b[j];
          }
        }
      }
    }
    __syncthreads();
  }
  if (wave == 0) {
    float* dst = part + (int64_t)pidx * hidden;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const int i = k * WAVE_SIZE + lane;
      if (i < nvec) {
        *reinterpret_cast<float4v*>(dst + i * 8) =
            float4v{acc[k][0], acc[k][1], acc[k][2], acc[k][3]};
        *reinterpret_cast<float4v*>(dst + i * 8 + 4) =
            float4v{acc[k][4], acc[k][5], acc[k][6], acc[k][7]};
      }
    }
  }
}

__global__ __launch_bounds__(POOL_BLOCK) void pool_finish_kernel(
    float* __restrict__ out,           // [S, dims]
    float* __restrict__ carry,         // [slots, hidden]
    const float* __restrict__ part,    // [nslabs, hidden]
    const bf16* __restrict__ x, const bf16* __restrict__ residual,
    const bf16* __restrict__ weight,
    const int* __restrict__ segs,      // [S, 8]
    const float eps, const int hidden, const int dims, const int normalize) {
  __shared__ float red[2][POOL_WAVES];
  const int* sg = segs + blockIdx.x * 8;
  const int row0 = sg[PC_ROW0], nrows = sg[PC_NROWS], mode = sg[PC_MODE];
  const int nvec = hidden / 8;
  float* out_row = out + (int64_t)blockIdx.x * dims;

  float v[POOL_MAXV][8] = {};
  if (mode != POOL_MEAN) {
    const int64_t off =
        (int64_t)(mode == POOL_LAST ? row0 + nrows - 1 : row0) * hidden;
    float ss = 0.f;
#pragma unroll
    for (int k = 0; k < POOL_MAXV; ++k) {
      const int i = k * POOL_BLOCK + threadIdx.x;
      if (i < nvec) {
        const ushort8 xv = *reinterpret_cast<const ushort8*>(x + off + i * 8);
        const ushort8 rv =
            *reinterpret_cast<const ushort8*>(residual + off + i * 8);
        ss = pool_add8(xv, rv, v[k], ss);
      }
    }
    const float rrms =
        pool_rrms(block_reduce_sum<POOL_BLOCK>(ss, red[0]), hidden, eps);
#pragma unroll
    for (int k = 0; k < POOL_MAXV; ++k) {
      const int i = k * POOL_BLOCK + threadIdx.x;
      if (i < nvec) {
        const ushort8 w = *reinterpret_cast<const ushort8*>(weight + i * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j)
          v[k][j] = v[k][j] * rrms * bf16_bits_to_float(w[j]);
      }
    }
  } else {
    const int slot = sg[PC_SLOT], counted = sg[PC_COUNTED];
    const int part0 = sg[PC_PART0], nparts = sg[PC_NPARTS];
    const bool final_chunk = sg[PC_FINAL] != 0;
    const float inv_count = 1.0f / (float)(counted + nrows);
#pragma unroll
    for (int k = 0; k < POOL_MAXV; ++k) {
      const int i = k * POOL_BLOCK + threadIdx.x;
      if (i < nvec) {
        float4v a = float4v{0.f, 0.f, 0.f, 0.f}, b = a;
        // slab order; unrolled so that several slabs' loads are in flight
#pragma unroll 4
        for (int p = 0; p < nparts; ++p) {
          const float* src = part + (int64_t)(part0 + p) * hidden + i * 8;
          a += *reinterpret_cast<const float4v*>(src);
          b += *reinterpret_cast<const float4v*>(src + 4);
        }
        const ushort8 w = *reinterpret_cast<const ushort8*>(weight + i * 8);
        float4v ca = float4v{0.f, 0.f, 0.f, 0.f}, cb = ca;
        if (counted > 0) {
          const float* c = carry + (int64_t)slot * hidden + i * 8;
          ca = *reinterpret_cast<const float4v*>(c);
          cb = *reinterpret_cast<const float4v*>(c + 4);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          a[j] = ca[j] + a[j] * bf16_bits_to_float(w[j]);
          b[j] = cb[j] + b[j] * bf16_bits_to_float(w[4 + j]);
        }
        if (!final_chunk) {
          float* c = carry + (int64_t)slot * hidden + i * 8;
          *reinterpret_cast<float4v*>(c) = a;
          *reinterpret_cast<float4v*>(c + 4) = b;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          v[k][j] = a[j] * inv_count;
          v[k][4 + j] = b[j] * inv_count;
        }
      }
    }
    if (!final_chunk) {  // uniform: the vector is not due yet
      for (int c = threadIdx.x; c < dims; c += POOL_BLOCK) out_row[c] = 0.f;
      return;
    }
  }

  float scale = 1.f;
  if (normalize) {
    float ss = 0.f;
#pragma unroll
    for (int k = 0; k < POOL_MAXV; ++k) {
      const int c0 = (k * POOL_BLOCK + threadIdx.x) * 8;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (c0 + j < dims) ss += v[k][j] * v[k][j];
    }
    const float norm = sqrtf(block_reduce_sum<POOL_BLOCK>(ss, red[1]));
    scale = 1.0f / fmaxf(norm, 1e-12f);
  }
#pragma unroll
  for (int k = 0; k < POOL_MAXV; ++k) {
    const int c0 = (k * POOL_BLOCK + threadIdx.x) * 8;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (c0 + j < dims) out_row[c0 + j] = v[k][j] * scale;
  }
}

}  // namespace arks

using namespace arks;

extern "C" {

int arks_pool_max_hidden() { return POOL_MAX_HIDDEN; }

void arks_pool_embed(void* out, void* carry, void* part, const void* x,
                     const void* residual, const void* weight,
                     const void* segs, const void* slabs, int nsegs,
                     int nslabs, float eps, int hidden, int dims,
                     int normalize, hipStream_t stream) {
  if (nslabs > 0) {
    const int nv = ceil_div(hidden, 8 * WAVE_SIZE);
    const size_t lds = (size_t)hidden * sizeof(float);
#define POOL_SLAB_LAUNCH(NV)                                               \
  hipLaunchKernelGGL((pool_slab_kernel<NV>), dim3(nslabs),                 \
                     dim3(POOL_BLOCK), lds, stream, (float*)part,          \
                     (const bf16*)x, (const bf16*)residual,                \
                     (const int*)slabs, eps, hidden)
    if (nv <= 1) POOL_SLAB_LAUNCH(1);
    else if (nv <= 2) POOL_SLAB_LAUNCH(2);
    else if (nv <= 4) POOL_SLAB_LAUNCH(4);
    else if (nv <= 8) POOL_SLAB_LAUNCH(8);
    else POOL_SLAB_LAUNCH(16);
#undef POOL_SLAB_LAUNCH
  }
  hipLaunchKernelGGL(pool_finish_kernel, dim3(nsegs), dim3(POOL_BLOCK), 0,
                     stream, (float*)out, (float*)carry, (const float*)part,
                     (const bf16*)x, (const bf16*)residual,
                     (const bf16*)weight, (const int*)segs, eps, hidden, dims,
                     normalize);
}

}  // extern "C"
