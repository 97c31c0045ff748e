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
// w8_skinny_gemm_kernel (M <= 64) is w4_skinny_gemm_kernel's design fed by
// bytes (read the notes there and in skinny_gemm.hip first): grid =
// (N/(64*NW), nsplits); swapped operands (A-frag = W rows, B-frag =
// activations), C fragment at [n = 4*la+r, m = lane%16]; A staged through a
// 2-slot LDS ring, batched and branchless, its loads issued BEFORE the W
// prefetch (vmcnt is issue-ordered) and its LDS writes after the chunk's
// MFMAs; W prefetched PF chunks ahead in a register ring with compile-time
// slots, 16 B per lane per load.
//   A lane's W bytes of a chunk are 32 CONSECUTIVE k of its row (two 16 B
//   loads; k = 32*la + 8*s + j for the chunk's four k-steps s), and the
//   activation fragment is read from LDS at the same 32*la + 8*s.
//   KC = 128 = one scale block along K, so a chunk's scale is constant per n
//   row: the chunk accumulates into its own f32 fragment and contributes
//       s[n] * acc_chunk.
//   No zero-point, hence no activation sums (the W4 kernel's asum).
//   Split-K partials use skinny_gemm.hip's [split][16*MT rows][N] f32 layout
//   so splitk_add_rmsnorm / splitk_rope_cache / skinny_combine read them
//   unchanged. N % (64*NW) == 0, K % 128 == 0, k_per_split % 128 == 0.
// The body is a copy of the W4 loop rather than a shared template so that
// the W4 kernel's code generation does not move.
//
// w8_dequant_kernel expands the weight to bf16 [N, K] for the library GEMM
// (M above the slab limit).
#include "common.h"

#include <algorithm>

namespace arks {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;

constexpr int W8_KC = 128;  // K per chunk = scale block
constexpr int W8_AP = 8;    // a_lds row pad (bf16): rows stay 16B-aligned

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

// One chunk of W for a lane: per N sub-tile the 32 bytes of its A-fragment
// row, plus the scales of the four C-fragment rows it accumulates.
template <int NW>
struct W8Chunk {
  u32x4 q[NW][2];
  f32x4 sc[NW];
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
  constexpr int MROWS = 16 * MT;
  constexpr int NT = 64 * NW;
  constexpr int KC = W8_KC;
  const int n0 = blockIdx.x * NT;
  const int kb = blockIdx.y * k_per_split;
  const int ke = min(k_total, kb + k_per_split);  // multiple of 128

  const int tid = threadIdx.x;
  const int wave = tid / WAVE_SIZE;
  const int lane = tid % WAVE_SIZE;
  const int lq = lane % 16;
  const int la = lane / 16;

  __shared__ __attribute__((aligned(16))) union {
    bf16 a_buf[2][64][KC + W8_AP];
    float c_buf[NT][64 + 1];
  } lds;

  f32x4 acc[NW][MT];
#pragma unroll
  for (int j = 0; j < NW; ++j)
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[j][t] = {0.f, 0.f, 0.f, 0.f};

  // A-fragment row of this lane in sub-tile j: n0 + 64*j + 16*wave + lq;
  // its C-fragment rows: n0 + 64*j + 16*wave + 4*la + r.
  const uint8_t* wrow = w8 + (int64_t)(n0 + wave * 16 + lq) * k_total + 32 * la;
  const int nc = n0 + wave * 16 + 4 * la;

  // Staging of one 128-wide chunk: the global loads of chunk c+1 issue at
  // the top of iteration c and their ds_writes come after its MFMAs. No
  // tails (K and the split ranges are multiples of 128), no per-item
  // guards. Rows >= m_rows are clamped duplicates that no reader consumes.
  constexpr int NIT = MROWS * 16 / 256;  // == MT
  auto load_a = [&](int kc, ushort8 (&gv)[NIT]) {
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int i = tid + it * 256;
      const int row = min(i / 16, m_rows - 1);
      gv[it] = *reinterpret_cast<const ushort8*>(
          a + (int64_t)row * a_stride + kc + (i % 16) * 8);
    }
  };
  auto store_a = [&](const ushort8 (&gv)[NIT], int buf) {
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int i = tid + it * 256;
      *reinterpret_cast<ushort8*>(&lds.a_buf[buf][i / 16][(i % 16) * 8]) =
          gv[it];
    }
  };

  // W ring of PF+1 chunks with COMPILE-TIME slots (the loop below is
  // unrolled over them). Branchless: past the end of the split the address
  // clamps to its last chunk (a re-read that nothing consumes); under a
  // branch the compiler cannot count the loads in flight and drains the
  // prefetch in front of the A ds_writes.
  W8Chunk<NW> wreg[PF + 1];
  auto load_w = [&](int kc, W8Chunk<NW>& dst) {
    kc = min(kc, ke - KC);
    const int64_t g = (int64_t)(kc / KC) * n_total;
#pragma unroll
    for (int j = 0; j < NW; ++j) {
      const uint8_t* p = wrow + (int64_t)j * 64 * k_total + kc;
      dst.q[j][0] = *reinterpret_cast<const u32x4*>(p);
      dst.q[j][1] = *reinterpret_cast<const u32x4*>(p + 16);
      dst.sc[j] = *reinterpret_cast<const f32x4*>(scales + g + nc + j * 64);
    }
  };

  // A loads issue BEFORE the W prefetch (issue-ordered vmcnt: the wait in
  // front of the A ds_writes then leaves the younger W loads in flight).
  if (kb >= ke) return;  // uniform; the host never launches an empty split
  {
    ushort8 gv[NIT];
    load_a(kb, gv);
#pragma unroll
    for (int p = 0; p <= PF; ++p) load_w(kb + p * KC, wreg[p]);
    store_a(gv, 0);
  }
  __syncthreads();

  int buf = 0;
  for (int kc0 = kb; kc0 < ke; kc0 += (PF + 1) * KC) {
#pragma unroll
    for (int u = 0; u <= PF; ++u) {
      const int kc = kc0 + u * KC;
      if (kc >= ke) break;  // uniform
      ushort8 gv[NIT];
      load_a(min(kc + KC, ke - KC), gv);  // last chunk: an unused re-read
      const W8Chunk<NW> cur = wreg[u];
      load_w(kc + (PF + 1) * KC, wreg[u]);  // refill the slot just read

      f32x4 cacc[NW][MT];
#pragma unroll
      for (int j = 0; j < NW; ++j)
#pragma unroll
        for (int t = 0; t < MT; ++t) cacc[j][t] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        bf16x8 wf[NW];
#pragma unroll
        for (int j = 0; j < NW; ++j)
          wf[j] = w8_frag(cur.q[j][s / 2][2 * (s % 2)],
                          cur.q[j][s / 2][2 * (s % 2) + 1]);
#pragma unroll
        for (int t = 0; t < MT; ++t) {
          ushort8 af = *reinterpret_cast<const ushort8*>(
              &lds.a_buf[buf][t * 16 + lq][32 * la + 8 * s]);
#pragma unroll
          for (int j = 0; j < NW; ++j)
            cacc[j][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                wf[j], *reinterpret_cast<bf16x8*>(&af), cacc[j][t], 0, 0, 0);
        }
      }
      // acc += s * cacc
#pragma unroll
      for (int j = 0; j < NW; ++j)
#pragma unroll
        for (int t = 0; t < MT; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            acc[j][t][r] =
                __builtin_fmaf(cur.sc[j][r], cacc[j][t][r], acc[j][t][r]);
      store_a(gv, buf ^ 1);
      __syncthreads();  // next chunk's A is staged; this slot may be reused
      buf ^= 1;
    }
  }

  if (nsplits > 1) {
    // [split][m][n] f32 partials, one 16 B store per lane per tile (the
    // layout of skinny_gemm.hip's store_partials). Rows >= m_rows hold
    // garbage and are never read.
    float* p = part + (int64_t)blockIdx.y * MROWS * n_total + nc;
#pragma unroll
    for (int j = 0; j < NW; ++j)
#pragma unroll
      for (int t = 0; t < MT; ++t)
        *reinterpret_cast<f32x4*>(p + (int64_t)(t * 16 + lq) * n_total +
                                  j * 64) = acc[j][t];
    return;
  }

  // Direct epilogue: transpose C^T through LDS, add bias, round to bf16.
  __syncthreads();  // all a_buf reads done before the union flips to c_buf
#pragma unroll
  for (int j = 0; j < NW; ++j)
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        lds.c_buf[j * 64 + wave * 16 + 4 * la + r][t * 16 + lq] = acc[j][t][r];
  __syncthreads();
  for (int i = tid; i < m_rows * NT; i += 256) {
    const int m = i / NT;
    const int n = i % NT;
    float v = lds.c_buf[n][m];
    if (bias != nullptr) v += bf16_bits_to_float(bias[n0 + n]);
    out[(int64_t)m * n_total + n0 + n] = float_to_bf16_bits(v);
  }
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

extern "C" void arks_skinny_combine(void* out, const void* part,
                                    const void* bias, int m_rows, int n_total,
                                    int nsplits, int mrows_pad,
                                    hipStream_t stream);

static int w8_mt(int m_rows) { return std::min((m_rows + 15) / 16, 4); }

// Rows per split slab of the partials that arks_w8_skinny_gemm writes.
extern "C" int arks_w8_slab_rows(int m_rows) { return 16 * w8_mt(m_rows); }

// nw = 64-row N sub-tiles per workgroup (1 or 2). combine = false (nsplits > 1
// only) leaves the f32 partials in `part` for a consumer that reduces them.
extern "C" void arks_w8_skinny_gemm(void* part, void* out, const void* a,
                                    const void* w8, const void* scales,
                                    const void* bias, int m_rows, int n_total,
                                    int k_total, int k_per_split, int nsplits,
                                    int64_t a_stride, int nw, bool combine,
                                    hipStream_t stream) {
  dim3 grid(n_total / (64 * nw), nsplits), block(256);
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, block, 0, stream, (float*)part,
                       (bf16*)out, (const bf16*)a, (const uint8_t*)w8,
                       (const float*)scales, (const bf16*)bias, m_rows,
                       n_total, k_total, k_per_split, nsplits, a_stride);
  };
  constexpr int PF = 1;
  const int mt = w8_mt(m_rows);
  if (nw == 2) {
    switch (mt) {
      case 1: launch(w8_skinny_gemm_kernel<1, 2, PF>); break;
      case 2: launch(w8_skinny_gemm_kernel<2, 2, PF>); break;
      case 3: launch(w8_skinny_gemm_kernel<3, 2, PF>); break;
      default: launch(w8_skinny_gemm_kernel<4, 2, PF>); break;
    }
  } else {
    switch (mt) {
      case 1: launch(w8_skinny_gemm_kernel<1, 1, PF>); break;
      case 2: launch(w8_skinny_gemm_kernel<2, 1, PF>); break;
      case 3: launch(w8_skinny_gemm_kernel<3, 1, PF>); break;
      default: launch(w8_skinny_gemm_kernel<4, 1, PF>); break;
    }
  }
  if (nsplits > 1 && combine)
    arks_skinny_combine(out, part, bias, m_rows, n_total, nsplits,
                        arks_w8_slab_rows(m_rows), stream);
}

extern "C" void arks_w8_dequant(void* out, const void* w8, const void* scales,
                                int n_total, int k_total, hipStream_t stream) {
  const int64_t vecs = (int64_t)n_total * (k_total / 16);
  dim3 grid((unsigned)((vecs + 255) / 256)), block(256);
  hipLaunchKernelGGL(w8_dequant_kernel, grid, block, 0, stream, (bf16*)out,
                     (const uint8_t*)w8, (const float*)scales, n_total,
                     k_total);
}
