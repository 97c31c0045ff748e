// Elementwise / normalization kernels for the decode hot path (bf16, gfx950).
// All memory-bound: vectorized 16 B/lane loads (guide G13), grid-stride, f32
// accumulation. Ops: rmsnorm, fused residual-add + rmsnorm, silu_mul (SwiGLU),
// neox-style RoPE (in-place on q and k).
#include "common.h"

namespace arks {

// ss + v*v as a rounded multiply followed by a rounded add, never an fma:
// the form rmsnorm_kernel<true> compiles to. Written out so that the
// partials-reading variant below accumulates the identical sum of squares
// (left to the compiler it contracted to fma there and not here).
__device__ __forceinline__ float add_square(const float ss, const float v) {
#pragma clang fp contract(off)
  return ss + v * v;
}

// The norm kernels below run one workgroup of NORM_BLOCK threads (4 waves)
// per row, 8 columns per thread per iteration; that map and
// block_reduce_sum<NORM_BLOCK> fix the summation order of the sum of squares.
constexpr int NORM_BLOCK = 256;

// Pass-1 step of the fused-add norms for eight columns: residual += x,
// rounded to bf16 and stored back; returns ss plus the squares of the
// ROUNDED sums, so that pass 2's re-read sees what was accumulated.
__device__ __forceinline__ float add_residual8(const ushort8 x,
                                               bf16* __restrict__ res,
                                               float ss) {
  ushort8 r = *reinterpret_cast<const ushort8*>(res);
  ushort8 s;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float v = bf16_bits_to_float(x[j]) + bf16_bits_to_float(r[j]);
    s[j] = float_to_bf16_bits(v);
    ss = add_square(ss, bf16_bits_to_float(s[j]));
  }
  *reinterpret_cast<ushort8*>(res) = s;
  return ss;
}

// Passes 1.5 and 2 of every norm: block-reduce the sum of squares, then
// normalize src_row (re-read from L1/L2), scale by weight, round.
__device__ __forceinline__ void rmsnorm_finish(bf16* __restrict__ out_row,
                                               const bf16* __restrict__ src_row,
                                               const bf16* __restrict__ weight,
                                               const float ss, const float eps,
                                               const int hidden) {
  __shared__ float red[NORM_BLOCK / WAVE_SIZE];
  float total = block_reduce_sum<NORM_BLOCK>(ss, red);
  const float rrms = rsqrtf(total / (float)hidden + eps);
  for (int i = threadIdx.x; i < hidden / 8; i += NORM_BLOCK) {
    ushort8 x = *reinterpret_cast<const ushort8*>(src_row + i * 8);
    ushort8 w = *reinterpret_cast<const ushort8*>(weight + i * 8);
    ushort8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float v = bf16_bits_to_float(x[j]) * rrms * bf16_bits_to_float(w[j]);
      o[j] = float_to_bf16_bits(v);
    }
    *reinterpret_cast<ushort8*>(out_row + i * 8) = o;
  }
}

// ---------------------------------------------------------------------------
// RMSNorm, optionally with the residual add fused in.
// hidden must be a multiple of 8 (bf16x8 vector loads).
// ---------------------------------------------------------------------------
template <bool FUSED_ADD>
__global__ void rmsnorm_kernel(bf16* __restrict__ out,
                               const bf16* __restrict__ input,
                               bf16* __restrict__ residual,  // null unless FUSED_ADD
                               const bf16* __restrict__ weight,
                               const float eps, const int hidden) {
  const int row = blockIdx.x;
  const bf16* in_row = input + (int64_t)row * hidden;
  bf16* res_row = FUSED_ADD ? residual + (int64_t)row * hidden : nullptr;

  const int nvec = hidden / 8;
  float ss = 0.f;
  // Pass 1: (optionally add residual and store it), accumulate sum of squares.
  for (int i = threadIdx.x; i < nvec; i += NORM_BLOCK) {
    ushort8 x = *reinterpret_cast<const ushort8*>(in_row + i * 8);
    if constexpr (FUSED_ADD) {
      ss = add_residual8(x, res_row + i * 8, ss);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float v = bf16_bits_to_float(x[j]);
        ss += v * v;
      }
    }
  }
  rmsnorm_finish(out + (int64_t)row * hidden, FUSED_ADD ? res_row : in_row,
                 weight, ss, eps, hidden);
}

// ---------------------------------------------------------------------------
// Fused residual-add + RMSNorm whose input is still the split-K partials of
// the producing skinny GEMM (skinny_gemm.hip, layout [split][m][n]): each
// element is reduced in split order, biased and rounded to bf16 exactly as
// skinny_combine_kernel would, then goes through the very helpers
// rmsnorm_kernel<true> uses, so the residual, the sum of squares and the
// output are bit-identical to the unfused pair; what goes away is the
// combine launch and its bf16 round trip.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void splitk_add_rmsnorm_kernel(
    bf16* __restrict__ out, const float* __restrict__ part,
    const bf16* __restrict__ bias,  // [hidden] or null
    bf16* __restrict__ residual, const bf16* __restrict__ weight,
    const float eps, const int hidden, const int nsplits,
    const int64_t split_stride) {
  const int row = blockIdx.x;
  const float* part_row = part + (int64_t)row * hidden;
  bf16* res_row = residual + (int64_t)row * hidden;

  const int nvec = hidden / 8;
  float ss = 0.f;
  for (int i = threadIdx.x; i < nvec; i += NORM_BLOCK) {
    const float* const p[2] = {part_row + i * 8, part_row + i * 8 + 4};
    float4v acc[2];
    splitk_reduce<2, 2>(p, split_stride, nsplits, acc);
    ushort8 x;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float xf = acc[j / 4][j % 4];
      if (bias != nullptr) xf += bf16_bits_to_float(bias[i * 8 + j]);
      x[j] = float_to_bf16_bits(xf);  // the combine's rounding
    }
    ss = add_residual8(x, res_row + i * 8, ss);
  }
  rmsnorm_finish(out + (int64_t)row * hidden, res_row, weight, ss, eps,
                 hidden);
}

// ---------------------------------------------------------------------------
// The same op in one round of loads, for rows of at most NORM_WIDE_BLOCK
// vectors (hidden <= 4096): one thread per 8-column vector, so every load of
// a row — partials, residual, weight, bias — is issued before the first
// add, and the rounded sums stay in registers for the normalisation (the
// kernel above needs two dependent rounds at hidden 3584 and re-reads the
// row for pass 2).
// The bits are those of the kernel above because its summation order is
// rebuilt exactly: there, lane t of 256 chains add_square over vector t and
// then over vector t + 256; here the upper 256 threads publish their
// rounded sums to LDS and lane t continues its chain over them, and
// block_reduce_sum<NORM_BLOCK>'s order (wave shuffle tree, then the four
// wave sums added 0..3) runs over the lower four waves only.
// ---------------------------------------------------------------------------
constexpr int NORM_WIDE_BLOCK = 512;

__global__ __launch_bounds__(NORM_WIDE_BLOCK) void splitk_add_rmsnorm_wide_kernel(
    bf16* __restrict__ out, const float* __restrict__ part,
    const bf16* __restrict__ bias,  // [hidden] or null
    bf16* __restrict__ residual, const bf16* __restrict__ weight,
    const float eps, const int hidden, const int nsplits,
    const int64_t split_stride) {
  // One LDS object: a second one can cost extra waits on the first.
  __shared__ struct {
    ushort8 hi[NORM_WIDE_BLOCK - NORM_BLOCK];  // rounded sums of vector t+256
    float red[NORM_BLOCK / WAVE_SIZE];
  } lds;
  const int row = blockIdx.x;
  const int tid = threadIdx.x;
  const int nvec = hidden / 8;
  const bool live = tid < nvec;
  // Idle threads load vector 0 (in bounds) and store nothing.
  const int col = live ? tid * 8 : 0;
  const float* part_row = part + (int64_t)row * hidden;
  bf16* res = residual + (int64_t)row * hidden + col;

  // Every load of the row, up front.
  const ushort8 r = *reinterpret_cast<const ushort8*>(res);
  const ushort8 w = *reinterpret_cast<const ushort8*>(weight + col);
  ushort8 b = {0, 0, 0, 0, 0, 0, 0, 0};
  if (bias != nullptr) b = *reinterpret_cast<const ushort8*>(bias + col);
  const float* const p[2] = {part_row + col, part_row + col + 4};
  float4v acc[2];
  splitk_reduce<2, 2>(p, split_stride, nsplits, acc);

  ushort8 s;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float xf = acc[j / 4][j % 4];
    if (bias != nullptr) xf += bf16_bits_to_float(b[j]);
    const uint16_t x = float_to_bf16_bits(xf);  // the combine's rounding
    // add_residual8's arithmetic
    s[j] = float_to_bf16_bits(bf16_bits_to_float(x) +
                              bf16_bits_to_float(r[j]));
  }
  if (live) *reinterpret_cast<ushort8*>(res) = s;
  if (tid >= NORM_BLOCK) lds.hi[tid - NORM_BLOCK] = s;
  __syncthreads();

  if (tid < NORM_BLOCK) {  // whole waves 0..3
    float ss = 0.f;
    if (live) {
#pragma unroll
      for (int j = 0; j < 8; ++j) ss = add_square(ss, bf16_bits_to_float(s[j]));
    }
    if (tid + NORM_BLOCK < nvec) {
      const ushort8 h = lds.hi[tid];
#pragma unroll
      for (int j = 0; j < 8; ++j) ss = add_square(ss, bf16_bits_to_float(h[j]));
    }
    ss = wave_reduce_sum(ss);
    if (tid % WAVE_SIZE == 0) lds.red[tid / WAVE_SIZE] = ss;
  }
  __syncthreads();
  float total = 0.f;
#pragma unroll
  for (int wv = 0; wv < NORM_BLOCK / WAVE_SIZE; ++wv) total += lds.red[wv];
  const float rrms = rsqrtf(total / (float)hidden + eps);
  if (!live) return;
  ushort8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float v = bf16_bits_to_float(s[j]) * rrms * bf16_bits_to_float(w[j]);
    o[j] = float_to_bf16_bits(v);
  }
  *reinterpret_cast<ushort8*>(out + (int64_t)row * hidden + col) = o;
}

// ---------------------------------------------------------------------------
// SiLU-mul: input [rows, 2*d] = [gate | up], output [rows, d].
// ---------------------------------------------------------------------------
__global__ void silu_mul_kernel(bf16* __restrict__ out,
                                const bf16* __restrict__ gate_up,
                                const int d, const int64_t total_vec) {
  // Grid-stride over row-major output in 8-element vectors.
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       idx < total_vec; idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = idx / (d / 8);
    const int col8 = (int)(idx % (d / 8)) * 8;
    const bf16* g = gate_up + row * (2 * (int64_t)d) + col8;
    const bf16* u = g + d;
    ushort8 gv = *reinterpret_cast<const ushort8*>(g);
    ushort8 uv = *reinterpret_cast<const ushort8*>(u);
    ushort8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float x = bf16_bits_to_float(gv[j]);
      float silu = x / (1.f + __expf(-x));
      o[j] = float_to_bf16_bits(silu * bf16_bits_to_float(uv[j]));
    }
    *reinterpret_cast<ushort8*>(out + row * d + col8) = o;
  }
}

// ---------------------------------------------------------------------------
// RoPE (neox / rotate-half), in place on q [T, Hq*D] and k [T, Hkv*D].
// cos_sin: [max_pos, D] f32, first half cos, second half sin (host-precomputed
// — guide App. B: never sinf/cosf on device for RoPE).
// One workgroup per token; threads cover (head, pair) space, 2 pairs each.
// ---------------------------------------------------------------------------
__global__ void rope_kernel(const int64_t* __restrict__ positions,
                            bf16* __restrict__ q, bf16* __restrict__ k,
                            const float* __restrict__ cos_sin,
                            const int head_dim, const int num_q_heads,
                            const int num_kv_heads, const int64_t q_stride,
                            const int64_t k_stride) {
  const int token = blockIdx.x;
  const int half = head_dim / 2;
  const int64_t pos = positions[token];
  const float* cs = cos_sin + pos * head_dim;
  const int total_heads = num_q_heads + num_kv_heads;
  // Each thread handles 2 consecutive rotary pairs (4 bf16 values).
  const int pairs2 = half / 2;  // pair-couples per head
  for (int idx = threadIdx.x; idx < total_heads * pairs2; idx += blockDim.x) {
    const int h = idx / pairs2;
    const int p2 = (idx % pairs2) * 2;  // first pair index of the couple
    bf16* base = (h < num_q_heads)
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
  }
}

}  // namespace arks

// ------------------------------- launchers ---------------------------------
using namespace arks;

extern "C" {

void arks_rmsnorm(void* out, const void* input, const void* weight, float eps,
                  int rows, int hidden, hipStream_t stream) {
  dim3 grid(rows), block(256);
  hipLaunchKernelGGL((rmsnorm_kernel<false>), grid, block, 0, stream,
                     (bf16*)out, (const bf16*)input, nullptr,
                     (const bf16*)weight, eps, hidden);
}

void arks_fused_add_rmsnorm(void* out, const void* input, void* residual,
                            const void* weight, float eps, int rows, int hidden,
                            hipStream_t stream) {
  dim3 grid(rows), block(256);
  hipLaunchKernelGGL((rmsnorm_kernel<true>), grid, block, 0, stream, (bf16*)out,
                     (const bf16*)input, (bf16*)residual, (const bf16*)weight,
                     eps, hidden);
}

void arks_splitk_add_rmsnorm(void* out, const void* part, const void* bias,
                             void* residual, const void* weight, float eps,
                             int rows, int hidden, int nsplits, int mrows_pad,
                             hipStream_t stream) {
  // One vector per thread where the row fits; wider rows loop.
  const bool wide = hidden <= 8 * NORM_WIDE_BLOCK;
  dim3 grid(rows), block(wide ? NORM_WIDE_BLOCK : NORM_BLOCK);
  hipLaunchKernelGGL(
      wide ? splitk_add_rmsnorm_wide_kernel : splitk_add_rmsnorm_kernel, grid,
      block, 0, stream, (bf16*)out, (const float*)part, (const bf16*)bias,
      (bf16*)residual, (const bf16*)weight, eps, hidden, nsplits,
      (int64_t)mrows_pad * hidden);
}

void arks_silu_mul(void* out, const void* gate_up, int64_t rows, int d,
                   hipStream_t stream) {
  int64_t total_vec = rows * (d / 8);
  int blocks = (int)std::min<int64_t>((total_vec + 255) / 256, 2048);
  if (blocks == 0) blocks = 1;
  hipLaunchKernelGGL(silu_mul_kernel, dim3(blocks), dim3(256), 0, stream,
                     (bf16*)out, (const bf16*)gate_up, d, total_vec);
}

void arks_rope_inplace(const void* positions, void* q, void* k,
                       const void* cos_sin, int num_tokens, int head_dim,
                       int num_q_heads, int num_kv_heads, int64_t q_stride,
                       int64_t k_stride, hipStream_t stream) {
  dim3 grid(num_tokens), block(256);
  hipLaunchKernelGGL(rope_kernel, grid, block, 0, stream,
                     (const int64_t*)positions, (bf16*)q, (bf16*)k,
                     (const float*)cos_sin, head_dim, num_q_heads,
                     num_kv_heads, q_stride, k_stride);
}

}  // extern "C"
