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
// w4_skinny_gemm_kernel (M <= 64) is skinny_gemm.hip's design fed by nibbles:
//   grid = (N/(64*NW), nsplits); swapped operands (A-frag = W rows, B-frag =
//   activations), C fragment at [n = 4*la+r, m = lane%16]; A staged through
//   a 2-slot LDS ring, batched and branchless, its loads issued BEFORE the W
//   prefetch (vmcnt is issue-ordered, see skinny_gemm.hip) and its LDS
//   writes after the chunk's MFMAs; W prefetched PF chunks ahead in a
//   register ring with compile-time slots, 16 B per lane.
//   A lane's 16 B are 32 CONSECUTIVE k of its row (k = 32*la + 8*s + j for
//   the chunk's four k-steps s), not the bf16 kernel's 8*la + 32*s: the MFMA
//   sums over all 32 k of a step whatever their order, so it is enough that
//   the activation fragment is read from LDS at the same 32*la + 8*s.
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
//   Split-K partials use skinny_gemm.hip's [split][16*MT rows][N] f32 layout
//   so splitk_add_rmsnorm / splitk_rope_cache / skinny_combine read them
//   unchanged. N % (64*NW) == 0, K % 128 == 0, k_per_split % 128 == 0.
//
// w4_moe_gemm_kernel is the same chunk loop over the stacked experts of an
// MoE block ([E, N, K/8] / [E, K/128, N]), its rows gathered and scattered
// through the routing table that moe_route_kernel (moe.hip) writes; comment
// at the kernel. Its body is a copy of the dense loop rather than a shared
// template so that the dense kernel's code generation does not move.
//
// w4_dequant_kernel expands the packed weight to bf16 [N, K] for the library
// GEMM (M > 64).
#include "common.h"

#include <algorithm>

namespace arks {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;

constexpr int W4_KC = 128;  // K per chunk = quantization group
constexpr int W4_AP = 8;    // a_lds row pad (bf16): rows stay 16B-aligned

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

// Sum over an aligned 16-lane group with DPP adds (xor 1, xor 2 inside the
// quad, then the mirrored quad and the mirrored half): every lane of the
// group ends up with the total. No LDS traffic, unlike a shuffle.
__device__ __forceinline__ float row16_sum(float v) {
  union {
    float f;
    int i;
  } a, b;
#define ARKS_W4_DPP_ADD(ctrl)                                             \
  a.f = v;                                                                \
  b.i = __builtin_amdgcn_update_dpp(0, a.i, ctrl, 0xF, 0xF, true);        \
  v += b.f;
  ARKS_W4_DPP_ADD(0xB1)   // quad_perm [1,0,3,2]
  ARKS_W4_DPP_ADD(0x4E)   // quad_perm [2,3,0,1]
  ARKS_W4_DPP_ADD(0x141)  // row_half_mirror
  ARKS_W4_DPP_ADD(0x140)  // row_mirror
#undef ARKS_W4_DPP_ADD
  return v;
}

// One chunk of W for a lane: per N sub-tile 32 nibbles of its A-fragment row,
// plus scale / zero-point of the four C-fragment rows it accumulates.
template <int NW>
struct W4Chunk {
  u32x4 q[NW];
  ushort4v sc[NW];   // f16 bits
  uint32_t zr[NW];   // four u8
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
  constexpr int MROWS = 16 * MT;
  constexpr int NT = 64 * NW;
  constexpr int KC = W4_KC;
  const int n0 = blockIdx.x * NT;
  const int kb = blockIdx.y * k_per_split;
  const int ke = min(k_total, kb + k_per_split);  // multiple of 128

  const int tid = threadIdx.x;
  const int wave = tid / WAVE_SIZE;
  const int lane = tid % WAVE_SIZE;
  const int lq = lane % 16;
  const int la = lane / 16;

  __shared__ __attribute__((aligned(16))) union {
    struct {
      bf16 a_buf[2][64][KC + W4_AP];
      float asum[2][64];  // sum over the chunk's 128 k of each A row
    } s;
    float c_buf[NT][64 + 1];
  } lds;

  f32x4 acc[NW][MT];
#pragma unroll
  for (int j = 0; j < NW; ++j)
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[j][t] = {0.f, 0.f, 0.f, 0.f};

  const int kwords = k_total / 8;
  // A-fragment row of this lane in sub-tile j: n0 + 64*j + 16*wave + lq;
  // its C-fragment rows: n0 + 64*j + 16*wave + 4*la + r.
  const uint32_t* qrow = qw + (int64_t)(n0 + wave * 16 + lq) * kwords + 4 * la;
  const int nc = n0 + wave * 16 + 4 * la;

  // Staging of one 128-wide chunk in two halves, so that the global loads
  // of chunk c+1 issue at the top of iteration c and their ds_writes come
  // after its MFMAs: the loads have the whole compute phase to land and the
  // wait in front of the writes costs nothing. No tails (K and the split
  // ranges are multiples of 128), no per-item guards. 16 threads = one
  // aligned 16-lane DPP row per A row, so the row sum is four DPP adds;
  // every lane of the row then holds it and all 16 write the same word
  // (no guard: a guard costs a branch and a wait per item). Rows >= m_rows
  // are clamped duplicates that no reader consumes.
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
      const ushort8 v = gv[it];
      *reinterpret_cast<ushort8*>(&lds.s.a_buf[buf][i / 16][(i % 16) * 8]) = v;
      float sum = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) sum += bf16_bits_to_float(v[e]);
      lds.s.asum[buf][i / 16] = row16_sum(sum);
    }
  };

  // W ring of PF+1 chunks with COMPILE-TIME slots (the loop below is
  // unrolled over them): no register shifting, which would read a load's
  // destination and so wait for it one iteration after it was issued.
  W4Chunk<NW> wreg[PF + 1];
  // Branchless: past the end of the split the address clamps to its last
  // chunk (a re-read that nothing consumes). Under a branch the compiler
  // cannot count the loads in flight and falls back to s_waitcnt vmcnt(0)
  // in front of the A ds_writes, draining the prefetch just issued.
  auto load_w = [&](int kc, W4Chunk<NW>& dst) {
    kc = min(kc, ke - KC);
    const int64_t g = (int64_t)(kc / KC) * n_total;
#pragma unroll
    for (int j = 0; j < NW; ++j) {
      dst.q[j] = *reinterpret_cast<const u32x4*>(
          qrow + (int64_t)j * 64 * kwords + kc / 8);
      dst.sc[j] =
          *reinterpret_cast<const ushort4v*>(scales + g + nc + j * 64);
      dst.zr[j] = *reinterpret_cast<const uint32_t*>(zeros + g + nc + j * 64);
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
      const W4Chunk<NW> cur = wreg[u];
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
        for (int j = 0; j < NW; ++j) wf[j] = w4_frag(cur.q[j][s]);
#pragma unroll
        for (int t = 0; t < MT; ++t) {
          ushort8 af = *reinterpret_cast<const ushort8*>(
              &lds.s.a_buf[buf][t * 16 + lq][32 * la + 8 * s]);
#pragma unroll
          for (int j = 0; j < NW; ++j)
            cacc[j][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                wf[j], *reinterpret_cast<bf16x8*>(&af), cacc[j][t], 0, 0, 0);
        }
      }
      // acc += s * (cacc - (128 + z) * asum), contraction written out.
#pragma unroll
      for (int j = 0; j < NW; ++j) {
        float sf[4], zf[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          sf[r] = f16_bits_to_float(cur.sc[j][r]);
          zf[r] = -(128.f + (float)((cur.zr[j] >> (8 * r)) & 0xFFu));
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

// One 64-entry slab of one expert's routing list: the chunk loop of
// w4_skinny_gemm_kernel (same staging, W ring, folded zero-point) with the
// activation rows GATHERED through the list and the result rows SCATTERED to
// out[p]. MT is the slab's live 16-row tiles, so an expert with 4 rows pays
// for one tile, not four. No split-K, no bias.
//   prow[i] (LDS, i < 16*MT): pair index of list entry i, entries past the
//   end clamped to the last valid one (duplicates that are never stored).
template <int MT, int NW, int PF, typename Lds>
__device__ __forceinline__ void w4_moe_slab(
    Lds& lds, const int* prow, bf16* __restrict__ out,
    const bf16* __restrict__ a, const uint32_t* __restrict__ qw,
    const uint16_t* __restrict__ scales, const uint8_t* __restrict__ zeros,
    const int rows, const int src_div, const int n_total, const int k_total) {
  constexpr int NT = 64 * NW;
  constexpr int KC = W4_KC;
  const int n0 = blockIdx.x * NT;
  const int tid = threadIdx.x;
  const int wave = tid / WAVE_SIZE;
  const int lane = tid % WAVE_SIZE;
  const int lq = lane % 16;
  const int la = lane / 16;

  f32x4 acc[NW][MT];
#pragma unroll
  for (int j = 0; j < NW; ++j)
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[j][t] = {0.f, 0.f, 0.f, 0.f};

  const int kwords = k_total / 8;
  const uint32_t* qrow = qw + (int64_t)(n0 + wave * 16 + lq) * kwords + 4 * la;
  const int nc = n0 + wave * 16 + 4 * la;

  // Source rows of this thread's staging items, resolved once: the chunk
  // loop below is then the dense kernel's, branch for branch.
  constexpr int NIT = MT;
  const bf16* arow[NIT];
#pragma unroll
  for (int it = 0; it < NIT; ++it)
    arow[it] = a + (int64_t)(prow[(tid + it * 256) / 16] / src_div) * k_total +
               (tid % 16) * 8;
  auto load_a = [&](int kc, ushort8 (&gv)[NIT]) {
#pragma unroll
    for (int it = 0; it < NIT; ++it)
      gv[it] = *reinterpret_cast<const ushort8*>(arow[it] + kc);
  };
  auto store_a = [&](const ushort8 (&gv)[NIT], int buf) {
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int i = tid + it * 256;
      const ushort8 v = gv[it];
      *reinterpret_cast<ushort8*>(&lds.s.a_buf[buf][i / 16][(i % 16) * 8]) = v;
      float sum = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) sum += bf16_bits_to_float(v[e]);
      lds.s.asum[buf][i / 16] = row16_sum(sum);
    }
  };

  W4Chunk<NW> wreg[PF + 1];
  auto load_w = [&](int kc, W4Chunk<NW>& dst) {
    kc = min(kc, k_total - KC);  // branchless, see w4_skinny_gemm_kernel
    const int64_t g = (int64_t)(kc / KC) * n_total;
#pragma unroll
    for (int j = 0; j < NW; ++j) {
      dst.q[j] = *reinterpret_cast<const u32x4*>(
          qrow + (int64_t)j * 64 * kwords + kc / 8);
      dst.sc[j] =
          *reinterpret_cast<const ushort4v*>(scales + g + nc + j * 64);
      dst.zr[j] = *reinterpret_cast<const uint32_t*>(zeros + g + nc + j * 64);
    }
  };

  {
    ushort8 gv[NIT];
    load_a(0, gv);
#pragma unroll
    for (int p = 0; p <= PF; ++p) load_w(p * KC, wreg[p]);
    store_a(gv, 0);
  }
  __syncthreads();

  int buf = 0;
  for (int kc0 = 0; kc0 < k_total; kc0 += (PF + 1) * KC) {
#pragma unroll
    for (int u = 0; u <= PF; ++u) {
      const int kc = kc0 + u * KC;
      if (kc >= k_total) break;  // uniform
      ushort8 gv[NIT];
      load_a(min(kc + KC, k_total - KC), gv);
      const W4Chunk<NW> cur = wreg[u];
      load_w(kc + (PF + 1) * KC, wreg[u]);

      f32x4 cacc[NW][MT];
#pragma unroll
      for (int j = 0; j < NW; ++j)
#pragma unroll
        for (int t = 0; t < MT; ++t) cacc[j][t] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        bf16x8 wf[NW];
#pragma unroll
        for (int j = 0; j < NW; ++j) wf[j] = w4_frag(cur.q[j][s]);
#pragma unroll
        for (int t = 0; t < MT; ++t) {
          ushort8 af = *reinterpret_cast<const ushort8*>(
              &lds.s.a_buf[buf][t * 16 + lq][32 * la + 8 * s]);
#pragma unroll
          for (int j = 0; j < NW; ++j)
            cacc[j][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                wf[j], *reinterpret_cast<bf16x8*>(&af), cacc[j][t], 0, 0, 0);
        }
      }
#pragma unroll
      for (int j = 0; j < NW; ++j) {
        float sf[4], zf[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          sf[r] = f16_bits_to_float(cur.sc[j][r]);
          zf[r] = -(128.f + (float)((cur.zr[j] >> (8 * r)) & 0xFFu));
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
      store_a(gv, buf ^ 1);
      __syncthreads();
      buf ^= 1;
    }
  }

  // Epilogue: transpose C^T through LDS, round to bf16, scatter row m of the
  // slab to out[prow[m]]; rows >= `rows` are the clamped duplicates.
  __syncthreads();
#pragma unroll
  for (int j = 0; j < NW; ++j)
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        lds.c_buf[j * 64 + wave * 16 + 4 * la + r][t * 16 + lq] = acc[j][t][r];
  __syncthreads();
  for (int i = tid; i < rows * NT; i += 256) {
    const int m = i / NT;
    const int n = i % NT;
    out[(int64_t)prow[m] * n_total + n0 + n] =
        float_to_bf16_bits(lds.c_buf[n][m]);
  }
}

// Routed grouped W4A16 GEMM over the local experts of an MoE block:
//   for e < E_local, i < counts[e], p = pairs[e][i]:
//     out[p, :] = a[p / src_div, :] @ dequant(W[e])^T
// grid = (N/(64*NW), E_local, slabs); a workgroup takes entries
// [64*z, 64*z + 64) of its expert's list and returns before any other load
// when the list is shorter. The grid depends on (N, E_local, max_rows) only,
// never on the routing, so the launch is capturable.
// The live rows of a slab are a run-time number (1..8 per expert at decode
// while max_rows is the batch size), so the body is instantiated for
// MT = 1..4 and picked once at the top by mt = ceil(rows / 16), uniform over
// the workgroup: nothing inside the chunk loop branches (a branch around the
// W loads breaks the vmcnt counting, profiles/w4_gemm.md section 2). The
// register allocation is that of MT = 4 for every mt.
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

  __shared__ __attribute__((aligned(16))) union {
    struct {
      bf16 a_buf[2][64][W4_KC + W4_AP];
      float asum[2][64];
    } s;
    float c_buf[64 * NW][64 + 1];
  } lds;
  __shared__ int prow[64];
  if (threadIdx.x < 64) {
    const int p = pairs[(int64_t)e * t_cols + r0 + min((int)threadIdx.x,
                                                       rows - 1)];
    prow[threadIdx.x] = min(max(p, 0), n_pairs - 1);
  }
  __syncthreads();

  const int64_t wq = (int64_t)e * n_total * (k_total / 8);
  const int64_t wg = (int64_t)e * (k_total / W4_KC) * n_total;
#define ARKS_W4_MOE_SLAB(MT)                                                 \
  w4_moe_slab<MT, NW, PF>(lds, prow, out, a, qw + wq, scales + wg,           \
                          zeros + wg, rows, src_div, n_total, k_total)
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

extern "C" void arks_skinny_combine(void* out, const void* part,
                                    const void* bias, int m_rows, int n_total,
                                    int nsplits, int mrows_pad,
                                    hipStream_t stream);

static int w4_mt(int m_rows) { return std::min((m_rows + 15) / 16, 4); }

// Rows per split slab of the partials that arks_w4_skinny_gemm writes.
extern "C" int arks_w4_slab_rows(int m_rows) { return 16 * w4_mt(m_rows); }

// nw = 64-row N sub-tiles per workgroup (1 or 2). combine = false (nsplits > 1
// only) leaves the f32 partials in `part` for a consumer that reduces them.
extern "C" void arks_w4_skinny_gemm(void* part, void* out, const void* a,
                                    const void* qw, const void* scales,
                                    const void* zeros, const void* bias,
                                    int m_rows, int n_total, int k_total,
                                    int k_per_split, int nsplits,
                                    int64_t a_stride, int nw, bool combine,
                                    hipStream_t stream) {
  dim3 grid(n_total / (64 * nw), nsplits), block(256);
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, block, 0, stream, (float*)part,
                       (bf16*)out, (const bf16*)a, (const uint32_t*)qw,
                       (const uint16_t*)scales, (const uint8_t*)zeros,
                       (const bf16*)bias, m_rows, n_total, k_total,
                       k_per_split, nsplits, a_stride);
  };
  constexpr int PF = 1;
  const int mt = w4_mt(m_rows);
  if (nw == 2) {
    switch (mt) {
      case 1: launch(w4_skinny_gemm_kernel<1, 2, PF>); break;
      case 2: launch(w4_skinny_gemm_kernel<2, 2, PF>); break;
      case 3: launch(w4_skinny_gemm_kernel<3, 2, PF>); break;
      default: launch(w4_skinny_gemm_kernel<4, 2, PF>); break;
    }
  } else {
    switch (mt) {
      case 1: launch(w4_skinny_gemm_kernel<1, 1, PF>); break;
      case 2: launch(w4_skinny_gemm_kernel<2, 1, PF>); break;
      case 3: launch(w4_skinny_gemm_kernel<3, 1, PF>); break;
      default: launch(w4_skinny_gemm_kernel<4, 1, PF>); break;
    }
  }
  if (nsplits > 1 && combine)
    arks_skinny_combine(out, part, bias, m_rows, n_total, nsplits,
                        arks_w4_slab_rows(m_rows), stream);
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
