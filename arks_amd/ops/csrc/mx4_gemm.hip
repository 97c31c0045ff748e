// W4A16 MX GEMMs for gfx950: C[M,N] = A[M,K] @ dequant(MX4)[N,K]^T with OCP
// microscaling FP4 weights (MXFP4): e2m1 elements sharing one e8m0 scale per
// block of 32 along K,
//   w[n,k] = e2m1(code[n,k]) * 2^(s[n, k/32] - 127).
//
// Format (no repack; ops/ref.py mx4_quantize / mx4_dequant), the tensors of
// the checkpoint:
//   mx4_weight u8 [N, K/2]   byte b of a row holds k = 2b in its low nibble
//                            and k = 2b+1 in its high nibble. A code is sign
//                            (bit 3) and a magnitude index into
//                            0, 0.5, 1, 1.5, 2, 3, 4, 6
//   mx4_scales u8 [N, K/32]  e8m0: the biased exponent of a power of two
//
// Conversion: v_cvt_scalef32_pk_bf16_fp4 turns the two nibbles of one byte
// of a dword (low nibble to the low half) into a bf16 pair multiplied by an
// f32 scale: four of them per eight weights. The scale is a power of two,
// built as the f32 bit pattern s << 23, and an e2m1 value has one mantissa
// bit, so the product is exact in bf16 as long as it is a normal number: the
// loader admits scale bytes 2..252 only (0.5 * 2^(2-127) is the smallest
// normal bf16, 6 * 2^(252-127) is finite). Applying the scale before the MFMA
// therefore loses nothing, and the chunk's f32 fragment is added to the
// accumulator as it is.
//
// mx4_skinny_gemm_kernel (M <= 64) is the streaming chunk loop of wq_stream.h
// (design, staging and issue order are described there) fed by nibbles:
//   grid = (N/(64*NW), nsplits). A lane's W of a 128-wide chunk are the 32
//   consecutive k = 32*la .. 32*la + 31 of its row, which is exactly one MX
//   block: one 16 B load per sub-tile, one dword per k-step, and one scale
//   byte, taken out of the aligned dword that holds the chunk's four scales
//   of the row. No zero-point, hence no activation sums and no LDS for them.
//
// mx4_dequant_kernel expands the weight to bf16 [N, K] for the library GEMM
// (M above the slab limit).
//
// mx4_act_quant_kernel turns bf16 activations into MXFP4 (packed, or
// quantized and expanded again) for the W4A4 mode; the GEMM on the
// mfma_scale_f32_16x16x128_f8f6f4 instruction that takes both operands as
// FP4 is mx4_mfma_gemm.hip. The kernels of this file keep bf16 activations:
// decode is bound by the weight bytes.
//
// mx4_moe_gemm_kernel is the same chunk loop over the stacked experts of an
// MoE block ([E, N, K/2] / [E, N, K/32]), its rows gathered and scattered
// through the routing table that moe_route_kernel (moe.hip) writes; comment
// at the kernel. Its prefill-sized W4A4 counterpart on the scaled MFMA is
// mx4_moe_mfma_gemm_kernel (mx4_mfma_gemm.hip).
//
// Not here: the W4A16 MFMA kernel for prefill-sized batches of the dense
// layers with bf16 activations is wqa16_mfma_gemm.hip; the routed kernel
// still runs such batches slab by slab.
#include "wq_stream.h"

namespace arks {

typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;

// f32 2^(s - 127) of an e8m0 byte s in 1..254.
__device__ __forceinline__ float mx4_scale(const uint32_t s) {
  union {
    uint32_t u;
    float f;
  } c;
  c.u = s << 23;
  return c.f;
}

// Eight consecutive weights (one dword of a row) as the scaled bf16 fragment.
__device__ __forceinline__ bf16x8 mx4_frag(const uint32_t d, const float sc) {
  union {
    bf16x2 p[4];
    bf16x8 b;
  } c;
  c.p[0] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, sc, 0);
  c.p[1] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, sc, 1);
  c.p[2] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, sc, 2);
  c.p[3] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, sc, 3);
  return c.b;
}

// The MX4 weight format of wq_stream: one [N, K] weight as a lane sees it.
template <int NW_>
struct Mx4Weights {
  static constexpr int NW = NW_;
  static constexpr bool ASUM = false;

  // One chunk of W for a lane: per N sub-tile the 16 B of nibbles of its
  // A-fragment row (one MX block) and the dword holding the row's four
  // scale bytes of the chunk; the lane's own is byte la.
  struct Chunk {
    u32x4 q[NW];
    uint32_t sc[NW];
  };

  const uint8_t* wrow;  // this lane's 16 B of chunk 0 in sub-tile 0
  const uint8_t* srow;  // its row's scale bytes
  int k_total;

  __device__ __forceinline__ Mx4Weights(const WqLane& ln, const uint8_t* w,
                                        const uint8_t* scales,
                                        const int k_total)
      : wrow(w + (int64_t)(ln.n0 + ln.wave * 16 + ln.lq) * (k_total / 2) +
             16 * ln.la),
        srow(scales + (int64_t)(ln.n0 + ln.wave * 16 + ln.lq) * (k_total / 32)),
        k_total(k_total) {}

  __device__ __forceinline__ void load(const int kc, Chunk& dst) const {
#pragma unroll
    for (int j = 0; j < NW; ++j) {
      dst.q[j] = *reinterpret_cast<const u32x4*>(
          wrow + (int64_t)j * 64 * (k_total / 2) + kc / 2);
      dst.sc[j] = *reinterpret_cast<const uint32_t*>(
          srow + (int64_t)j * 64 * (k_total / 32) + kc / 32);
    }
  }

  static __device__ __forceinline__ bf16x8 frag(const Chunk& c, const int j,
                                                const int s) {
    const uint32_t la = threadIdx.x % WAVE_SIZE / 16;
    return mx4_frag(c.q[j][s],
                    mx4_scale(__builtin_amdgcn_ubfe(c.sc[j], 8 * la, 8)));
  }

  // acc += cacc: the scale went into the fragment
  template <int MT, typename Lds>
  static __device__ __forceinline__ void scale(f32x4 (&acc)[NW][MT],
                                               const f32x4 (&cacc)[NW][MT],
                                               const Chunk&, const Lds&,
                                               const int, const int) {
#pragma unroll
    for (int j = 0; j < NW; ++j)
#pragma unroll
      for (int t = 0; t < MT; ++t) acc[j][t] += cacc[j][t];
  }
};

template <int MT, int NW, int PF>
__global__ __launch_bounds__(256) void mx4_skinny_gemm_kernel(
    float* __restrict__ part,            // [nsplits, 16*MT, N] (nsplits > 1)
    bf16* __restrict__ out,              // [M, N] (nsplits == 1)
    const bf16* __restrict__ a,          // [M, K] (row stride a_stride)
    const uint8_t* __restrict__ w,       // [N, K/2] e2m1 pairs
    const uint8_t* __restrict__ scales,  // [N, K/32] e8m0
    const bf16* __restrict__ bias,  // [N] or null (applied when nsplits==1)
    const int m_rows, const int n_total, const int k_total,
    const int k_per_split, const int nsplits, const int64_t a_stride) {
  const WqLane ln(64 * NW);
  wq_dense_gemm<MT, PF>(
      ln, Mx4Weights<NW>(ln, w, scales, k_total),
      WqDenseRows<MT>{part, out, a, bias, m_rows, nsplits, a_stride}, n_total,
      k_total, k_per_split);
}

// Routed grouped W4A16 MX GEMM over the local experts of an MoE block:
//   for e < E_local, i < counts[e], p = pairs[e][i]:
//     out[p, :] = a[p / src_div, :] @ dequant(w[e], scales[e])^T
// w8_moe_gemm_kernel (w8_gemm.hip; the notes are at w4_moe_gemm_kernel) with
// Mx4Weights: the same grid = (N/(64*NW), E_local, slabs), a function of (N,
// E_local, max_rows) only, so a decode batch captures into a graph; the same
// uniform early return for a list shorter than the slab, the same prow table
// and clamps, the same MT = 1..4 bodies picked once by ceil(rows / 16). The
// expert's nibbles and scale bytes are reached by 64-bit offsets (e * N *
// K/2 and e * N * K/32 bytes, multiples of 16 and 4: the loads of Mx4Weights
// stay aligned); inside an expert the dense format's addressing is
// unchanged. No zero-point, so no activation sums in LDS.
template <int NW, int PF>
__global__ __launch_bounds__(256) void mx4_moe_gemm_kernel(
    bf16* __restrict__ out,              // [n_pairs, N]
    const bf16* __restrict__ a,          // [>= ceil(n_pairs / src_div), K]
    const uint8_t* __restrict__ w,       // [E, N, K/2] e2m1 pairs
    const uint8_t* __restrict__ scales,  // [E, N, K/32] e8m0
    const int* __restrict__ counts,      // [E]
    const int* __restrict__ pairs,       // [E, t_cols]
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

  const int64_t ww = (int64_t)e * n_total * (k_total / 2);
  const int64_t ws = (int64_t)e * n_total * (k_total / 32);
  const WqLane ln(64 * NW);
#define ARKS_MX4_MOE_SLAB(MT)                                             \
  wq_stream<MT, PF>(                                                      \
      lds, ln, Mx4Weights<NW>(ln, w + ww, scales + ws, k_total),          \
      WqRoutedRows<MT>(out, a, prow, rows, src_div, k_total), 0, k_total, \
      n_total)
  switch ((rows + 15) / 16) {
    case 1: ARKS_MX4_MOE_SLAB(1); break;
    case 2: ARKS_MX4_MOE_SLAB(2); break;
    case 3: ARKS_MX4_MOE_SLAB(3); break;
    default: ARKS_MX4_MOE_SLAB(4); break;
  }
#undef ARKS_MX4_MOE_SLAB
}

// out[n][32c..32c+31] = bf16(e2m1 * 2^(s-127)): one MX block per thread, a
// 16 B load, one scale byte, four 16 B stores. Exact, as in the GEMM.
__global__ __launch_bounds__(256) void mx4_dequant_kernel(
    bf16* __restrict__ out, const uint8_t* __restrict__ w,
    const uint8_t* __restrict__ scales, const int n_total,
    const int k_total) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)n_total * (k_total / 32)) return;
  // [N, K/32] blocks in row-major order are the scale tensor's own order
  const float sc = mx4_scale(scales[idx]);
  const u32x4 q = *reinterpret_cast<const u32x4*>(w + idx * 16);
  bf16* o = out + idx * 32;
#pragma unroll
  for (int s = 0; s < 4; ++s)
    *reinterpret_cast<bf16x8*>(o + 8 * s) = mx4_frag(q[s], sc);
}

// bf16 activations [M, K] (row stride x_stride) to MXFP4 by the conversion
// rule of ops/ref.py mx4_quantize, for the W4A4 GEMM (mx4_mfma_gemm.hip).
// A lane owns 8 consecutive elements (one 16 B load) and four adjacent lanes
// one MX block. The block's amax is the maximum of the integer magnitude
// bits (order-preserving for finite bf16), two quad-permute steps wide; its
// exponent field e gives the scale byte clamp(e - 2), i.e. a shared exponent
// of floor(log2(amax)) - 2, or 127 for an all-zero block. Four
// v_cvt_scalef32_pk_fp4_bf16 (round to nearest even, saturating, dividing by
// the scale) make the lane's dword of eight nibbles.
//   QDQ = false: xq u8 [M, K/2] (one coalesced dword per lane) and xs u8
//                [M, K/32] (lane 0 of the quad), the layout of the weights
//   QDQ = true:  the same codes expanded again by mx4_frag into bf16 [M, K],
//                exactly: the input of the W4A16 kernels below the MFMA
//                threshold, which then see the same activations
// Compiled without the packed f32 VALU forms, as mx4_mfma_gemm.hip explains
// (the kernel has no f32 arithmetic, so this costs nothing).
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push( \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif
template <bool QDQ>
__global__ __launch_bounds__(256) void mx4_act_quant_kernel(
    uint32_t* __restrict__ xq,  // [M, K/8] dwords of nibbles (!QDQ)
    uint8_t* __restrict__ xs,   // [M, K/32] (!QDQ)
    bf16* __restrict__ xhat,    // [M, K] (QDQ)
    const bf16* __restrict__ x, const int m_rows, const int k_total,
    const int64_t x_stride) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int per_row = k_total / 8;  // a multiple of 4: quads never straddle
  const bool in = idx < (int64_t)m_rows * per_row;
  const int64_t row = in ? idx / per_row : 0;
  const int c = in ? (int)(idx % per_row) : 0;
  union {
    u32x4 u;
    bf16x2 p[4];
  } v;
  v.u = u32x4{0u, 0u, 0u, 0u};
  if (in) v.u = *reinterpret_cast<const u32x4*>(x + row * x_stride + 8 * c);

  uint32_t amax = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t d = v.u[i] & 0x7fff7fffu;
    amax = max(amax, max(d & 0xffffu, d >> 16));
  }
  // quad_perm [1,0,3,2] then [2,3,0,1]: every lane of the quad gets the max
  amax = max(amax, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)amax, 0xB1,
                                                         0xf, 0xf, true));
  amax = max(amax, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)amax, 0x4E,
                                                         0xf, 0xf, true));
  const int e = (int)(amax >> 7);
  const uint32_t s = amax == 0 ? 127u : (uint32_t)min(max(e - 2, 2), 252);
  const float sc = mx4_scale(s);
  uint32_t q = 0;
  q = __builtin_amdgcn_cvt_scalef32_pk_fp4_bf16(q, v.p[0], sc, 0);
  q = __builtin_amdgcn_cvt_scalef32_pk_fp4_bf16(q, v.p[1], sc, 1);
  q = __builtin_amdgcn_cvt_scalef32_pk_fp4_bf16(q, v.p[2], sc, 2);
  q = __builtin_amdgcn_cvt_scalef32_pk_fp4_bf16(q, v.p[3], sc, 3);
  if (!in) return;
  if constexpr (QDQ) {
    *reinterpret_cast<bf16x8*>(xhat + row * k_total + 8 * c) =
        mx4_frag(q, sc);
  } else {
    xq[idx] = q;
    if (c % 4 == 0) xs[row * (k_total / 32) + c / 4] = (uint8_t)s;
  }
}
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

}  // namespace arks

using namespace arks;

// qdq: write bf16 xhat [M, K]; else xq u8 [M, K/2] and xs u8 [M, K/32].
extern "C" void arks_mx4_act_quant(void* xq, void* xs, void* xhat,
                                   const void* x, int m_rows, int k_total,
                                   int64_t x_stride, bool qdq,
                                   hipStream_t stream) {
  const int64_t lanes = (int64_t)m_rows * (k_total / 8);
  dim3 grid((unsigned)((lanes + 255) / 256)), block(256);
  if (qdq)
    hipLaunchKernelGGL(mx4_act_quant_kernel<true>, grid, block, 0, stream,
                       (uint32_t*)nullptr, (uint8_t*)nullptr, (bf16*)xhat,
                       (const bf16*)x, m_rows, k_total, x_stride);
  else
    hipLaunchKernelGGL(mx4_act_quant_kernel<false>, grid, block, 0, stream,
                       (uint32_t*)xq, (uint8_t*)xs, (bf16*)nullptr,
                       (const bf16*)x, m_rows, k_total, x_stride);
}

extern "C" void arks_mx4_skinny_gemm(void* part, void* out, const void* a,
                                     const void* w, const void* scales,
                                     const void* bias, int m_rows,
                                     int n_total, int k_total,
                                     int k_per_split, int nsplits,
                                     int64_t a_stride, int nw, bool combine,
                                     hipStream_t stream) {
  wq_launch_dense(
      out, part, bias, m_rows, n_total, nsplits, nw, combine, stream,
      [&](auto MT, auto NW, dim3 grid, dim3 block) {
        hipLaunchKernelGGL((mx4_skinny_gemm_kernel<MT(), NW(), 1>), grid,
                           block, 0, stream, (float*)part, (bf16*)out,
                           (const bf16*)a, (const uint8_t*)w,
                           (const uint8_t*)scales, (const bf16*)bias, m_rows,
                           n_total, k_total, k_per_split, nsplits, a_stride);
      });
}

// nw = 64-row N sub-tiles per workgroup (1 or 2); slabs = ceil(max_rows/64).
extern "C" void arks_mx4_moe_gemm(void* out, const void* a, const void* w,
                                  const void* scales, const void* counts,
                                  const void* pairs, int n_experts,
                                  int t_cols, int n_pairs, int src_div,
                                  int slabs, int n_total, int k_total, int nw,
                                  hipStream_t stream) {
  dim3 grid(n_total / (64 * nw), n_experts, slabs), block(256);
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, block, 0, stream, (bf16*)out,
                       (const bf16*)a, (const uint8_t*)w,
                       (const uint8_t*)scales, (const int*)counts,
                       (const int*)pairs, t_cols, n_pairs, src_div, n_total,
                       k_total);
  };
  if (nw == 2)
    launch(mx4_moe_gemm_kernel<2, 1>);
  else
    launch(mx4_moe_gemm_kernel<1, 1>);
}

extern "C" void arks_mx4_dequant(void* out, const void* w, const void* scales,
                                 int n_total, int k_total,
                                 hipStream_t stream) {
  const int64_t blocks = (int64_t)n_total * (k_total / 32);
  dim3 grid((unsigned)((blocks + 255) / 256)), block(256);
  hipLaunchKernelGGL(mx4_dequant_kernel, grid, block, 0, stream, (bf16*)out,
                     (const uint8_t*)w, (const uint8_t*)scales, n_total,
                     k_total);
}
