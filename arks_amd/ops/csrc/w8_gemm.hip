// W8A16 GEMMs for gfx950: C[M,N] = A[M,K] @ dequant(W8)[N,K]^T with OCP
// e4m3fn weights scaled per 128x128 block (the published "fine-grained FP8"
// checkpoint format):
//   w[n,k] = float(w8[n,k]) * s[k/128, n].
//
// Format (no repack; ops/ref.py w8_quantize / w8_expand_scales):
//   w8     e4m3fn [N, K]     row-major as in the checkpoint: 16 consecutive
//                            bytes of a row are 16 consecutive k
//   scales f32    [K/128, N] the checkpoint's [N/128, K/128] block scales
//                            expanded to one value per (k-block, output row),
//                            the orientation of the W4 scales
// gfx950 FP8 is OCP e4m3fn, so the checkpoint's bytes are the device format.
//
// Conversion: v_cvt_pk_f32_fp8 turns two e4m3 bytes into two f32, exactly
// (subnormals and signed zero included). Every e4m3 value has 3 mantissa
// bits and an exponent inside bf16's range, so the low 16 bits of that f32
// are zero and its high half IS the bf16 value: one v_perm_b32 packs the two
// high halves into a bf16 pair. 8 VALU ops per 8 weights, no rounding
// anywhere.
//
// w8_skinny_gemm_kernel (M <= 64) is the streaming chunk loop of wq_stream.h
// (design, staging and issue order are described there) fed by bytes:
//   grid = (N/(64*NW), nsplits). A lane's chunk of W is two 16 B loads per
//   sub-tile, the 32 bytes k = 32*la .. 32*la + 31 of its row, two dwords
//   per k-step, plus the f32 scales of its four C-fragment rows.
//   KC = 128 = one scale block along K, so a chunk's scale is constant per n
//   row: the chunk accumulates into its own f32 fragment and contributes
//       s[n] * acc_chunk.
//   No zero-point, hence no activation sums (the W4 format's asum) and no
//   LDS for them.
//
// w8_moe_gemm_kernel is the same chunk loop over the stacked experts of an
// MoE block ([E, N, K] / [E, K/128, N]), its rows gathered and scattered
// through the routing table that moe_route_kernel (moe.hip) writes; comment
// at the kernel.
//
// w8_dequant_kernel expands the weight to bf16 [N, K] for the library GEMM
// (M above the slab limit).
#include "wq_stream.h"

namespace arks {

typedef __attribute__((ext_vector_type(2))) float f32x2;

// Two e4m3 bytes (the low or the high half of `w`) as a bf16 pair, exact.
template <bool HI>
__device__ __forceinline__ uint32_t w8_pair(const uint32_t w) {
  union {
    f32x2 f;
    uint32_t u[2];
  } c;
  c.f = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, HI);
  // bytes 3,2 of u[1] over bytes 3,2 of u[0]: the two f32 high halves
  return __builtin_amdgcn_perm(c.u[1], c.u[0], 0x07060302u);
}

// Eight consecutive weights (two dwords of a row) as the bf16 fragment.
__device__ __forceinline__ bf16x8 w8_frag(const uint32_t d0,
                                          const uint32_t d1) {
  union {
    u32x4 u;
    bf16x8 b;
  } c;
  c.u[0] = w8_pair<false>(d0);
  c.u[1] = w8_pair<true>(d0);
  c.u[2] = w8_pair<false>(d1);
  c.u[3] = w8_pair<true>(d1);
  return c.b;
}

// The W8 weight format of wq_stream: one [N, K] weight as a lane sees it.
template <int NW_>
struct W8Weights {
  static constexpr int NW = NW_;
  static constexpr bool ASUM = false;

  // One chunk of W for a lane: per N sub-tile the 32 bytes of its A-fragment
  // row, plus the scales of the four C-fragment rows it accumulates.
  struct Chunk {
    u32x4 q[NW][2];
    f32x4 sc[NW];
  };

  const uint8_t* wrow;  // this lane's 32 B of chunk 0 in sub-tile 0
  const float* scales;  // [K/128, N]
  int nc, n_total, k_total;

  __device__ __forceinline__ W8Weights(const WqLane& ln, const uint8_t* w8,
                                       const float* scales, const int n_total,
                                       const int k_total)
      : wrow(w8 + (int64_t)(ln.n0 + ln.wave * 16 + ln.lq) * k_total +
             32 * ln.la),
        scales(scales),
        nc(ln.nc),
        n_total(n_total),
        k_total(k_total) {}

  __device__ __forceinline__ void load(const int kc, Chunk& dst) const {
    const int64_t g = (int64_t)(kc / WQ_KC) * n_total;
#pragma unroll
    for (int j = 0; j < NW; ++j) {
      const uint8_t* p = wrow + (int64_t)j * 64 * k_total + kc;
      dst.q[j][0] = *reinterpret_cast<const u32x4*>(p);
      dst.q[j][1] = *reinterpret_cast<const u32x4*>(p + 16);
      dst.sc[j] = *reinterpret_cast<const f32x4*>(scales + g + nc + j * 64);
    }
  }

  static __device__ __forceinline__ bf16x8 frag(const Chunk& c, const int j,
                                                const int s) {
    return w8_frag(c.q[j][s / 2][2 * (s % 2)], c.q[j][s / 2][2 * (s % 2) + 1]);
  }

  // acc += s * cacc
  template <int MT, typename Lds>
  static __device__ __forceinline__ void scale(f32x4 (&acc)[NW][MT],
                                               const f32x4 (&cacc)[NW][MT],
                                               const Chunk& c, const Lds&,
                                               const int, const int) {
#pragma unroll
    for (int j = 0; j < NW; ++j)
#pragma unroll
      for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          acc[j][t][r] =
              __builtin_fmaf(c.sc[j][r], cacc[j][t][r], acc[j][t][r]);
  }
};

template <int MT, int NW, int PF>
__global__ __launch_bounds__(256) void w8_skinny_gemm_kernel(
    float* __restrict__ part,        // [nsplits, 16*MT, N] (nsplits > 1)
    bf16* __restrict__ out,          // [M, N] (nsplits == 1)
    const bf16* __restrict__ a,      // [M, K] (row stride a_stride)
    const uint8_t* __restrict__ w8,  // [N, K] e4m3fn
    const float* __restrict__ scales,  // [K/128, N]
    const bf16* __restrict__ bias,   // [N] or null (applied when nsplits==1)
    const int m_rows, const int n_total, const int k_total,
    const int k_per_split, const int nsplits, const int64_t a_stride) {
  const WqLane ln(64 * NW);
  wq_dense_gemm<MT, PF>(
      ln, W8Weights<NW>(ln, w8, scales, n_total, k_total),
      WqDenseRows<MT>{part, out, a, bias, m_rows, nsplits, a_stride}, n_total,
      k_total, k_per_split);
}

// Routed grouped W8A16 GEMM over the local experts of an MoE block:
//   for e < E_local, i < counts[e], p = pairs[e][i]:
//     out[p, :] = a[p / src_div, :] @ (float(w8[e]) * scales[e])^T
// w4_moe_gemm_kernel (w4_gemm.hip, read the notes there) with W8Weights: the
// same grid = (N/(64*NW), E_local, slabs), a function of (N, E_local,
// max_rows) only; the same uniform early return for a list shorter than the
// slab, the same prow table and clamps, the same MT = 1..4 bodies picked once
// by ceil(rows / 16). The expert's weight and scales are reached by 64-bit
// offsets (e * N * K bytes, e * (K/128) * N floats); inside an expert the
// dense format's addressing is unchanged. No zero-point, so no activation
// sums in LDS.
template <int NW, int PF>
__global__ __launch_bounds__(256) void w8_moe_gemm_kernel(
    bf16* __restrict__ out,             // [n_pairs, N]
    const bf16* __restrict__ a,         // [>= ceil(n_pairs / src_div), K]
    const uint8_t* __restrict__ w8,     // [E, N, K] e4m3fn
    const float* __restrict__ scales,   // [E, K/128, N]
    const int* __restrict__ counts,     // [E]
    const int* __restrict__ pairs,      // [E, t_cols]
    const int t_cols, const int n_pairs, const int src_div,
    const int n_total, const int k_total) {
  const int e = blockIdx.y;
  const int cnt = min(max(counts[e], 0), t_cols);
  const int r0 = blockIdx.z * 64;
  if (r0 >= cnt) return;  // uniform
  const int rows = min(cnt - r0, 64);

  __shared__ __attribute__((aligned(16))) WqLds<NW, false> lds;
  __shared__ int prow[64];
  if (threadIdx.x < 64) {
    const int p = pairs[(int64_t)e * t_cols + r0 + min((int)threadIdx.x,
                                                       rows - 1)];
    prow[threadIdx.x] = min(max(p, 0), n_pairs - 1);
  }
  __syncthreads();

  const int64_t ww = (int64_t)e * n_total * k_total;
  const int64_t wg = (int64_t)e * (k_total / WQ_KC) * n_total;
  const WqLane ln(64 * NW);
#define ARKS_W8_MOE_SLAB(MT)                                              \
  wq_stream<MT, PF>(                                                      \
      lds, ln, W8Weights<NW>(ln, w8 + ww, scales + wg, n_total, k_total), \
      WqRoutedRows<MT>(out, a, prow, rows, src_div, k_total), 0, k_total, \
      n_total)
  switch ((rows + 15) / 16) {
    case 1: ARKS_W8_MOE_SLAB(1); break;
    case 2: ARKS_W8_MOE_SLAB(2); break;
    case 3: ARKS_W8_MOE_SLAB(3); break;
    default: ARKS_W8_MOE_SLAB(4); break;
  }
#undef ARKS_W8_MOE_SLAB
}

// out[n][16c..16c+15] = bf16(float(w8) * s): 16 weights per thread, two 16 B
// stores. One f32 multiply and one round-to-nearest-even per weight.
__global__ __launch_bounds__(256) void w8_dequant_kernel(
    bf16* __restrict__ out, const uint8_t* __restrict__ w8,
    const float* __restrict__ scales, const int n_total, const int k_total) {
  const int kvecs = k_total / 16;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)n_total * kvecs) return;
  const int n = (int)(idx / kvecs);
  const int c = (int)(idx % kvecs);
  const float s = scales[(int64_t)(c / 8) * n_total + n];
  const u32x4 w = *reinterpret_cast<const u32x4*>(w8 + idx * 16);
  bf16* o = out + (int64_t)n * k_total + 16 * c;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    ushort8 v;
#pragma unroll
    for (int d = 0; d < 2; ++d) {
      const f32x2 lo =
          __builtin_amdgcn_cvt_pk_f32_fp8((int)w[2 * h + d], false);
      const f32x2 hi =
          __builtin_amdgcn_cvt_pk_f32_fp8((int)w[2 * h + d], true);
      v[4 * d + 0] = float_to_bf16_bits(lo[0] * s);
      v[4 * d + 1] = float_to_bf16_bits(lo[1] * s);
      v[4 * d + 2] = float_to_bf16_bits(hi[0] * s);
      v[4 * d + 3] = float_to_bf16_bits(hi[1] * s);
    }
    *reinterpret_cast<ushort8*>(o + 8 * h) = v;
  }
}

}  // namespace arks

using namespace arks;

extern "C" void arks_w8_skinny_gemm(void* part, void* out, const void* a,
                                    const void* w8, const void* scales,
                                    const void* bias, int m_rows, int n_total,
                                    int k_total, int k_per_split, int nsplits,
                                    int64_t a_stride, int nw, bool combine,
                                    hipStream_t stream) {
  wq_launch_dense(
      out, part, bias, m_rows, n_total, nsplits, nw, combine, stream,
      [&](auto MT, auto NW, dim3 grid, dim3 block) {
        hipLaunchKernelGGL((w8_skinny_gemm_kernel<MT(), NW(), 1>), grid,
                           block, 0, stream, (float*)part, (bf16*)out,
                           (const bf16*)a, (const uint8_t*)w8,
                           (const float*)scales, (const bf16*)bias, m_rows,
                           n_total, k_total, k_per_split, nsplits, a_stride);
      });
}

// nw = 64-row N sub-tiles per workgroup (1 or 2); slabs = ceil(max_rows/64).
extern "C" void arks_w8_moe_gemm(void* out, const void* a, const void* w8,
                                 const void* scales, const void* counts,
                                 const void* pairs, int n_experts, int t_cols,
                                 int n_pairs, int src_div, int slabs,
                                 int n_total, int k_total, int nw,
                                 hipStream_t stream) {
  dim3 grid(n_total / (64 * nw), n_experts, slabs), block(256);
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, block, 0, stream, (bf16*)out,
                       (const bf16*)a, (const uint8_t*)w8,
                       (const float*)scales, (const int*)counts,
                       (const int*)pairs, t_cols, n_pairs, src_div, n_total,
                       k_total);
  };
  if (nw == 2)
    launch(w8_moe_gemm_kernel<2, 1>);
  else
    launch(w8_moe_gemm_kernel<1, 1>);
}

extern "C" void arks_w8_dequant(void* out, const void* w8, const void* scales,
                                int n_total, int k_total, hipStream_t stream) {
  const int64_t vecs = (int64_t)n_total * (k_total / 16);
  dim3 grid((unsigned)((vecs + 255) / 256)), block(256);
  hipLaunchKernelGGL(w8_dequant_kernel, grid, block, 0, stream, (bf16*)out,
                     (const uint8_t*)w8, (const float*)scales, n_total,
                     k_total);
}
