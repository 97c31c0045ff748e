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
// Not here: the mfma_scale_f32_*_f8f6f4 instructions (they need a quantized
// A operand; decode is bound by the weight bytes and the activations stay
// bf16) and a routed grouped expert GEMM (MX4 routed experts are dequantized
// to bf16 at load).
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

}  // namespace arks

using namespace arks;

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

extern "C" void arks_mx4_dequant(void* out, const void* w, const void* scales,
                                 int n_total, int k_total,
                                 hipStream_t stream) {
  const int64_t blocks = (int64_t)n_total * (k_total / 32);
  dim3 grid((unsigned)((blocks + 255) / 256)), block(256);
  hipLaunchKernelGGL(mx4_dequant_kernel, grid, block, 0, stream, (bf16*)out,
                     (const uint8_t*)w, (const uint8_t*)scales, n_total,
                     k_total);
}
