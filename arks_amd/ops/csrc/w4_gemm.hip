// W4A16 GEMMs for gfx950: C[M,N] = A[M,K] @ dequant(Wq)[N,K]^T with 4-bit
// unsigned asymmetric weights, group size 128 along K:
//   w[n,k] = (q[n,k] - z[n,k/128]) * s[n,k/128].
//
// Packed format (written by ops/ref.py w4_pack):
//   qweight u32 [N, K/8]   row-major over N; word c of row n holds k = 8c..8c+7,
//                          nibble i = q[n, 8c + order[i]], order = 0,2,4,6,1,3,5,7
//   scales  f16 [K/128, N]
//   zeros   u8  [K/128, N]
// With that nibble order elements 2p and 2p+1 sit 16 bits apart, so
// ((word >> 4p) & 0x000F000F) | 0x43004300 is the bf16 PAIR (128+q[2p],
// 128+q[2p+1]): 0x4300 is bf16 128.0, whose ulp is 1, so or-ing a nibble into
// the mantissa adds it exactly. One shift+and+or per two weights, no cvt.
//
// w4_skinny_gemm_kernel (M <= 64) is the streaming chunk loop of wq_stream.h
// (design, staging and issue order are described there) fed by nibbles:
//   grid = (N/(64*NW), nsplits). A lane's chunk of W is 16 B per sub-tile,
//   the 32 nibbles k = 32*la .. 32*la + 31 of its row, one packed word per
//   k-step, plus scale and zero-point of its four C-fragment rows.
//   KC = 128 = the group size, so a chunk's scale and zero-point are constant
//   per n row and are applied to the chunk's f32 accumulator, not per weight.
//   Zero-point: FOLDED. The MFMA runs on the raw 128+q; per (m, chunk) the
//   staging threads also sum the activations (asum, one 16-lane reduce per
//   row, cheap next to a per-weight subtract: there is no packed bf16 add to
//   do it in two-wide, and 32 cvt+sub per lane per chunk would outweigh the
//   16 MFMAs), and the chunk contributes
//       s * (acc_chunk - (128 + z) * asum).
//   Cancellation: acc_chunk and (128+z)*asum are each ~128*|sum a| and are
//   f32-rounded separately, so their difference carries an absolute error of
//   about 2^-23 * 143 * sum|a_k| over the chunk (~1e-3 for |a| ~ 0.5), which
//   the scale (~0.02 for weights of std 0.05) brings to ~2e-5 per chunk —
//   two orders below the bf16 rounding of the output. With exact data
//   (one-hot activations, power-of-two scales) every step is exact.
//   NW = 64-row N sub-tiles per workgroup (1 or 2). At 4 bits the weights of
//   a 64-row tile are 4 KB per chunk but the activations staged for them are
//   16 KB at M = 64; NW = 2 halves that re-read.
//
// w4_moe_gemm_kernel is the same chunk loop over the stacked experts of an
// MoE block ([E, N, K/8] / [E, K/128, N]), its rows gathered and scattered
// through the routing table that moe_route_kernel (moe.hip) writes; comment
// at the kernel.
//
// w4_dequant_kernel expands the packed weight to bf16 [N, K] for the library
// GEMM (M > 64).
#include "wq_stream.h"

namespace arks {

__device__ __forceinline__ float f16_bits_to_float(uint16_t u) {
  union {
    uint16_t u;
    _Float16 h;
  } c;
  c.u = u;
  return static_cast<float>(c.h);
}

// Eight weights of one packed word as the bf16 fragment (128 + q), in k order.
__device__ __forceinline__ bf16x8 w4_frag(const uint32_t w) {
  union {
    u32x4 u;
    bf16x8 b;
  } c;
#pragma unroll
  for (int p = 0; p < 4; ++p)
    c.u[p] = ((w >> (4 * p)) & 0x000F000Fu) | 0x43004300u;
  return c.b;
}

// The W4 weight format of wq_stream: one [N, K/8] weight as a lane sees it.
template <int NW_>
struct W4Weights {
  static constexpr int NW = NW_;
  static constexpr bool ASUM = true;  // the folded zero-point needs sum(a)

  // One chunk of W for a lane: per N sub-tile 32 nibbles of its A-fragment
  // row, plus scale / zero-point of the four C-fragment rows it accumulates.
  struct Chunk {
    u32x4 q[NW];
    ushort4v sc[NW];   // f16 bits
    uint32_t zr[NW];   // four u8
  };

  const uint32_t* qrow;    // this lane's 16 B of chunk 0 in sub-tile 0
  const uint16_t* scales;  // [K/128, N] f16
  const uint8_t* zeros;    // [K/128, N]
  int nc, kwords, n_total;

  __device__ __forceinline__ W4Weights(const WqLane& ln, const uint32_t* qw,
                                       const uint16_t* scales,
                                       const uint8_t* zeros, const int n_total,
                                       const int k_total)
      : qrow(qw + (int64_t)(ln.n0 + ln.wave * 16 + ln.lq) * (k_total / 8) +
             4 * ln.la),
        scales(scales),
        zeros(zeros),
        nc(ln.nc),
        kwords(k_total / 8),
        n_total(n_total) {}

  __device__ __forceinline__ void load(const int kc, Chunk& dst) const {
    const int64_t g = (int64_t)(kc / WQ_KC) * n_total;
#pragma unroll
    for (int j = 0; j < NW; ++j) {
      dst.q[j] = *reinterpret_cast<const u32x4*>(
          qrow + (int64_t)j * 64 * kwords + kc / 8);
      dst.sc[j] = *reinterpret_cast<const ushort4v*>(scales + g + nc + j * 64);
      dst.zr[j] = *reinterpret_cast<const uint32_t*>(zeros + g + nc + j * 64);
    }
  }

  static __device__ __forceinline__ bf16x8 frag(const Chunk& c, const int j,
                                                const int s) {
    return w4_frag(c.q[j][s]);
  }

  // acc += s * (cacc - (128 + z) * asum), contraction written out.
  template <int MT, typename Lds>
  static __device__ __forceinline__ void scale(f32x4 (&acc)[NW][MT],
                                               const f32x4 (&cacc)[NW][MT],
                                               const Chunk& c, const Lds& lds,
                                               const int buf, const int lq) {
#pragma unroll
    for (int j = 0; j < NW; ++j) {
      float sf[4], zf[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        sf[r] = f16_bits_to_float(c.sc[j][r]);
        zf[r] = -(128.f + (float)((c.zr[j] >> (8 * r)) & 0xFFu));
      }
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        const float as = lds.s.asum[buf][t * 16 + lq];
#pragma unroll
        for (int r = 0; r < 4; ++r)
          acc[j][t][r] = __builtin_fmaf(
              sf[r], __builtin_fmaf(zf[r], as, cacc[j][t][r]), acc[j][t][r]);
      }
    }
  }
};

template <int MT, int NW, int PF>
__global__ __launch_bounds__(256) void w4_skinny_gemm_kernel(
    float* __restrict__ part,        // [nsplits, 16*MT, N] (nsplits > 1)
    bf16* __restrict__ out,          // [M, N] (nsplits == 1)
    const bf16* __restrict__ a,      // [M, K] (row stride a_stride)
    const uint32_t* __restrict__ qw,     // [N, K/8]
    const uint16_t* __restrict__ scales, // [K/128, N] f16
    const uint8_t* __restrict__ zeros,   // [K/128, N]
    const bf16* __restrict__ bias,   // [N] or null (applied when nsplits==1)
    const int m_rows, const int n_total, const int k_total,
    const int k_per_split, const int nsplits, const int64_t a_stride) {
  const WqLane ln(64 * NW);
  wq_dense_gemm<MT, PF>(
      ln, W4Weights<NW>(ln, qw, scales, zeros, n_total, k_total),
      WqDenseRows<MT>{part, out, a, bias, m_rows, nsplits, a_stride}, n_total,
      k_total, k_per_split);
}

// Routed grouped W4A16 GEMM over the local experts of an MoE block:
//   for e < E_local, i < counts[e], p = pairs[e][i]:
//     out[p, :] = a[p / src_div, :] @ dequant(W[e])^T
// grid = (N/(64*NW), E_local, slabs); a workgroup takes entries
// [64*z, 64*z + 64) of its expert's list and returns before any other load
// when the list is shorter. The grid depends on (N, E_local, max_rows) only,
// never on the routing, so the launch is capturable.
// A slab is the dense kernel's chunk loop with the activation rows GATHERED
// through the list and the result rows SCATTERED to out[p] (WqRoutedRows).
// The live rows of a slab are a run-time number (1..8 per expert at decode
// while max_rows is the batch size), so the body is instantiated for
// MT = 1..4 and picked once at the top by mt = ceil(rows / 16), uniform over
// the workgroup: an expert with 4 rows pays for one tile, not four, and
// nothing inside the chunk loop branches (a branch around the W loads breaks
// the vmcnt counting, profiles/w4_gemm.md section 2). The register
// allocation is that of MT = 4 for every mt.
// Every index read from memory is clamped to the extents the host passed
// (counts to t_cols, pair indices to n_pairs), so no table content can send a
// load or a store out of bounds.
template <int NW, int PF>
__global__ __launch_bounds__(256) void w4_moe_gemm_kernel(
    bf16* __restrict__ out,              // [n_pairs, N]
    const bf16* __restrict__ a,          // [>= ceil(n_pairs / src_div), K]
    const uint32_t* __restrict__ qw,     // [E, N, K/8]
    const uint16_t* __restrict__ scales, // [E, K/128, N] f16
    const uint8_t* __restrict__ zeros,   // [E, K/128, N]
    const int* __restrict__ counts,      // [E]
    const int* __restrict__ pairs,       // [E, t_cols]
    const int t_cols, const int n_pairs, const int src_div,
    const int n_total, const int k_total) {
  const int e = blockIdx.y;
  const int cnt = min(max(counts[e], 0), t_cols);
  const int r0 = blockIdx.z * 64;
  if (r0 >= cnt) return;  // uniform
  const int rows = min(cnt - r0, 64);

  __shared__ __attribute__((aligned(16))) WqLds<NW, true> lds;
  __shared__ int prow[64];
  if (threadIdx.x < 64) {
    const int p = pairs[(int64_t)e * t_cols + r0 + min((int)threadIdx.x,
                                                       rows - 1)];
    prow[threadIdx.x] = min(max(p, 0), n_pairs - 1);
  }
  __syncthreads();

  const int64_t wq = (int64_t)e * n_total * (k_total / 8);
  const int64_t wg = (int64_t)e * (k_total / WQ_KC) * n_total;
  const WqLane ln(64 * NW);
#define ARKS_W4_MOE_SLAB(MT)                                                 \
  wq_stream<MT, PF>(                                                         \
      lds, ln,                                                               \
      W4Weights<NW>(ln, qw + wq, scales + wg, zeros + wg, n_total, k_total), \
      WqRoutedRows<MT>(out, a, prow, rows, src_div, k_total), 0, k_total,    \
      n_total)
  switch ((rows + 15) / 16) {
    case 1: ARKS_W4_MOE_SLAB(1); break;
    case 2: ARKS_W4_MOE_SLAB(2); break;
    case 3: ARKS_W4_MOE_SLAB(3); break;
    default: ARKS_W4_MOE_SLAB(4); break;
  }
#undef ARKS_W4_MOE_SLAB
}

// out[n][8c..8c+7] = bf16((q - z) * s): one packed word per thread, one 16 B
// store. (q - z) * s is exact in f32 (5-bit integer times an 11-bit
// mantissa), so the result is the RNE bf16 rounding of the true value.
__global__ __launch_bounds__(256) void w4_dequant_kernel(
    bf16* __restrict__ out, const uint32_t* __restrict__ qw,
    const uint16_t* __restrict__ scales, const uint8_t* __restrict__ zeros,
    const int n_total, const int k_total) {
  const int kwords = k_total / 8;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)n_total * kwords) return;
  const int n = (int)(idx / kwords);
  const int c = (int)(idx % kwords);
  const int64_t g = (int64_t)(c / 16) * n_total + n;
  const float s = f16_bits_to_float(scales[g]);
  const float z = (float)zeros[g];
  const uint32_t w = qw[idx];
  ushort8 o;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int nib = (e & 1) * 4 + (e >> 1);  // inverse of order[]
    o[e] = float_to_bf16_bits(((float)((w >> (4 * nib)) & 0xFu) - z) * s);
  }
  *reinterpret_cast<ushort8*>(out + (int64_t)n * k_total + 8 * c) = o;
}

}  // namespace arks

using namespace arks;

extern "C" int arks_wq_slab_rows(int m_rows) { return 16 * wq_mt(m_rows); }

extern "C" void arks_w4_skinny_gemm(void* part, void* out, const void* a,
                                    const void* qw, const void* scales,
                                    const void* zeros, const void* bias,
                                    int m_rows, int n_total, int k_total,
                                    int k_per_split, int nsplits,
                                    int64_t a_stride, int nw, bool combine,
                                    hipStream_t stream) {
  wq_launch_dense(
      out, part, bias, m_rows, n_total, nsplits, nw, combine, stream,
      [&](auto MT, auto NW, dim3 grid, dim3 block) {
        hipLaunchKernelGGL((w4_skinny_gemm_kernel<MT(), NW(), 1>), grid,
                           block, 0, stream, (float*)part, (bf16*)out,
                           (const bf16*)a, (const uint32_t*)qw,
                           (const uint16_t*)scales, (const uint8_t*)zeros,
                           (const bf16*)bias, m_rows, n_total, k_total,
                           k_per_split, nsplits, a_stride);
      });
}

// nw = 64-row N sub-tiles per workgroup (1 or 2); slabs = ceil(max_rows/64).
extern "C" void arks_w4_moe_gemm(void* out, const void* a, const void* qw,
                                 const void* scales, const void* zeros,
                                 const void* counts, const void* pairs,
                                 int n_experts, int t_cols, int n_pairs,
                                 int src_div, int slabs, int n_total,
                                 int k_total, int nw, hipStream_t stream) {
  dim3 grid(n_total / (64 * nw), n_experts, slabs), block(256);
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, block, 0, stream, (bf16*)out,
                       (const bf16*)a, (const uint32_t*)qw,
                       (const uint16_t*)scales, (const uint8_t*)zeros,
                       (const int*)counts, (const int*)pairs, t_cols, n_pairs,
                       src_div, n_total, k_total);
  };
  if (nw == 2)
    launch(w4_moe_gemm_kernel<2, 1>);
  else
    launch(w4_moe_gemm_kernel<1, 1>);
}

extern "C" void arks_w4_dequant(void* out, const void* qw, const void* scales,
                                const void* zeros, int n_total, int k_total,
                                hipStream_t stream) {
  const int64_t words = (int64_t)n_total * (k_total / 8);
  dim3 grid((unsigned)((words + 255) / 256)), block(256);
  hipLaunchKernelGGL(w4_dequant_kernel, grid, block, 0, stream, (bf16*)out,
                     (const uint32_t*)qw, (const uint16_t*)scales,
                     (const uint8_t*)zeros, n_total, k_total);
}
