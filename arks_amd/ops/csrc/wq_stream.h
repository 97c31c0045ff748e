// The streaming chunk loop of the quantized skinny GEMMs (M <= 64 rows per
// launch or per routed slab): C[M,N] = A[M,K] @ dequant(W)[N,K]^T for weights
// quantized in groups of 128 along K. One body, wq_stream, parametrised by
//   a weight format  (w4_gemm.hip W4Weights, w8_gemm.hip W8Weights,
//       mx4_gemm.hip Mx4Weights, whose groups of 32 are one lane's share of
//       a chunk): what a lane's chunk of W is, how it is loaded, how eight
//       weights become a bf16 fragment, and how a chunk's f32 fragment is
//       scaled into the accumulator (with or without the sums of the
//       activations);
//   a row source     (WqDenseRows, WqRoutedRows below): where the A rows come
//       from, which K-range is summed and where the result rows go.
// MT (live 16-row M tiles), NW (64-row N sub-tiles per workgroup, 1 or 2) and
// PF (chunks of W prefetched ahead) are template parameters; everything is
// resolved at compile time, there is no run-time format switch.
//
// The design is skinny_gemm.hip's (read the notes there first):
//   256 threads; swapped operands (A-frag = W rows, B-frag = activations),
//   C fragment at [n = 4*la+r, m = lane%16]. Wave w owns rows 16w..16w+15 of
//   each 64-row sub-tile: a lane's A-fragment row is n0 + 64*j + 16*wave + lq,
//   its C-fragment rows are n0 + 64*j + 16*wave + 4*la + r.
//   A is staged through a 2-slot LDS ring, batched and branchless, its global
//   loads issued BEFORE the W prefetch and its LDS writes after the chunk's
//   MFMAs; W is prefetched PF chunks ahead in a register ring with
//   compile-time slots.
//   A lane's W of a chunk are 32 CONSECUTIVE k of its row (k = 32*la + 8*s + j
//   for the chunk's four k-steps s), not the bf16 kernel's 8*la + 32*s: the
//   MFMA sums over all 32 k of a step whatever their order, so it is enough
//   that the activation fragment is read from LDS at the same 32*la + 8*s.
//   KC = 128 = the quantization group, so a chunk's scale (and zero-point)
//   is constant per n row: each chunk accumulates into its own f32 fragment,
//   which the format then scales into the accumulator.
//   Split-K partials use skinny_gemm.hip's [split][16*MT rows][N] f32 layout
//   so splitk_add_rmsnorm / splitk_rope_cache / skinny_combine read them
//   unchanged. N % (64*NW) == 0, K % 128 == 0, k_per_split % 128 == 0.
#pragma once

#include "common.h"

#include <algorithm>
#include <type_traits>

namespace arks {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;

constexpr int WQ_KC = 128;  // K per chunk = quantization group / scale block
constexpr int WQ_AP = 8;    // a_buf row pad (bf16): rows stay 16B-aligned

// Sum over an aligned 16-lane group with DPP adds (xor 1, xor 2 inside the
// quad, then the mirrored quad and the mirrored half): every lane of the
// group ends up with the total. No LDS traffic, unlike a shuffle.
__device__ __forceinline__ float row16_sum(float v) {
  union {
    float f;
    int i;
  } a, b;
#define ARKS_WQ_DPP_ADD(ctrl)                                             \
  a.f = v;                                                                \
  b.i = __builtin_amdgcn_update_dpp(0, a.i, ctrl, 0xF, 0xF, true);        \
  v += b.f;
  ARKS_WQ_DPP_ADD(0xB1)   // quad_perm [1,0,3,2]
  ARKS_WQ_DPP_ADD(0x4E)   // quad_perm [2,3,0,1]
  ARKS_WQ_DPP_ADD(0x141)  // row_half_mirror
  ARKS_WQ_DPP_ADD(0x140)  // row_mirror
#undef ARKS_WQ_DPP_ADD
  return v;
}

// A thread's place in the workgroup and the workgroup's N tile.
struct WqLane {
  int tid, wave, lq, la;
  int n0;  // first output column of the workgroup
  int nc;  // first of this lane's four C-fragment rows in sub-tile 0
  __device__ __forceinline__ explicit WqLane(const int nt)
      : tid(threadIdx.x),
        wave(tid / WAVE_SIZE),
        lq(tid % WAVE_SIZE % 16),
        la(tid % WAVE_SIZE / 16),
        n0(blockIdx.x * nt),
        nc(n0 + wave * 16 + 4 * la) {}
};

// LDS of a workgroup: the A ring (with, for a format that folds a zero-point,
// the sum over the chunk's 128 k of each A row), reused by the epilogue's
// transpose.
template <bool ASUM>
struct WqStage {
  bf16 a_buf[2][64][WQ_KC + WQ_AP];
};
template <>
struct WqStage<true> {
  bf16 a_buf[2][64][WQ_KC + WQ_AP];
  float asum[2][64];
};
template <int NW, bool ASUM>
union WqLds {
  WqStage<ASUM> s;
  float c_buf[64 * NW][64 + 1];
};

// Transpose C^T through LDS: afterwards c_buf[n][m] is the result at row m,
// column n0 + n.
template <int MT, int NW, typename Lds>
__device__ __forceinline__ void wq_transpose(Lds& lds, const WqLane& ln,
                                             const f32x4 (&acc)[NW][MT]) {
  __syncthreads();  // all a_buf reads done before the union flips to c_buf
#pragma unroll
  for (int j = 0; j < NW; ++j)
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        lds.c_buf[j * 64 + ln.wave * 16 + 4 * ln.la + r][t * 16 + ln.lq] =
            acc[j][t][r];
  __syncthreads();
}

// Dense rows: A [m_rows, K] with row stride a_stride, K-range [kb, ke) of
// split blockIdx.y; f32 partials when K is split, else bias + bf16 rows.
template <int MT>
struct WqDenseRows {
  float* __restrict__ part;       // [nsplits, 16*MT, N] (nsplits > 1)
  bf16* __restrict__ out;         // [M, N] (nsplits == 1)
  const bf16* __restrict__ a;     // [M, K] (row stride a_stride)
  const bf16* __restrict__ bias;  // [N] or null (applied when nsplits == 1)
  int m_rows, nsplits;
  int64_t a_stride;

  // Rows >= m_rows are clamped duplicates that no reader consumes.
  __device__ __forceinline__ void load(const int tid, const int kc,
                                       ushort8 (&gv)[MT]) const {
#pragma unroll
    for (int it = 0; it < MT; ++it) {
      const int i = tid + it * 256;
      const int row = min(i / 16, m_rows - 1);
      gv[it] = *reinterpret_cast<const ushort8*>(
          a + (int64_t)row * a_stride + kc + (i % 16) * 8);
    }
  }

  template <int NW, typename Lds>
  __device__ __forceinline__ void finish(Lds& lds, const WqLane& ln,
                                         const f32x4 (&acc)[NW][MT],
                                         const int n_total) const {
    if (nsplits > 1) {
      // [split][m][n] f32 partials, one 16 B store per lane per tile (the
      // layout of skinny_gemm.hip's store_partials). Rows >= m_rows hold
      // garbage and are never read.
      float* p = part + (int64_t)blockIdx.y * (16 * MT) * n_total + ln.nc;
#pragma unroll
      for (int j = 0; j < NW; ++j)
#pragma unroll
        for (int t = 0; t < MT; ++t)
          *reinterpret_cast<f32x4*>(p + (int64_t)(t * 16 + ln.lq) * n_total +
                                    j * 64) = acc[j][t];
      return;
    }
    // Direct epilogue: transpose, add bias, round to bf16.
    constexpr int NT = 64 * NW;
    wq_transpose<MT, NW>(lds, ln, acc);
    for (int i = ln.tid; i < m_rows * NT; i += 256) {
      const int m = i / NT;
      const int n = i % NT;
      float v = lds.c_buf[n][m];
      if (bias != nullptr) v += bf16_bits_to_float(bias[ln.n0 + n]);
      out[(int64_t)m * n_total + ln.n0 + n] = float_to_bf16_bits(v);
    }
  }
};

// Routed rows: one 64-entry slab of an expert's routing list. Row i of the
// slab is gathered from a[prow[i] / src_div] and scattered to out[prow[i]];
// the whole K, no split, no bias.
//   prow[i] (LDS, i < 16*MT): pair index of list entry i, entries past the
//   end clamped to the last valid one (duplicates that are never stored).
template <int MT>
struct WqRoutedRows {
  bf16* __restrict__ out;
  const int* prow;
  int rows;  // live rows of the slab, <= 16*MT
  // Source rows of this thread's staging items, resolved once, so that the
  // chunk loop gathers without a branch or a table read.
  const bf16* arow[MT];

  __device__ __forceinline__ WqRoutedRows(bf16* out, const bf16* a,
                                          const int* prow, const int rows,
                                          const int src_div, const int k_total)
      : out(out), prow(prow), rows(rows) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int it = 0; it < MT; ++it)
      arow[it] = a +
                 (int64_t)(prow[(tid + it * 256) / 16] / src_div) * k_total +
                 (tid % 16) * 8;
  }

  __device__ __forceinline__ void load(const int, const int kc,
                                       ushort8 (&gv)[MT]) const {
#pragma unroll
    for (int it = 0; it < MT; ++it)
      gv[it] = *reinterpret_cast<const ushort8*>(arow[it] + kc);
  }

  // Rows >= `rows` are the clamped duplicates.
  template <int NW, typename Lds>
  __device__ __forceinline__ void finish(Lds& lds, const WqLane& ln,
                                         const f32x4 (&acc)[NW][MT],
                                         const int n_total) const {
    constexpr int NT = 64 * NW;
    wq_transpose<MT, NW>(lds, ln, acc);
    for (int i = ln.tid; i < rows * NT; i += 256) {
      const int m = i / NT;
      const int n = i % NT;
      out[(int64_t)prow[m] * n_total + ln.n0 + n] =
          float_to_bf16_bits(lds.c_buf[n][m]);
    }
  }
};

// The chunk loop over K-range [kb, ke) (multiples of 128, kb < ke) and the
// row source's epilogue. Weights wq: a format with
//   NW, ASUM        sub-tiles per workgroup; whether staging sums A rows
//   Chunk           a lane's W of one chunk, scales included
//   load(kc, dst)   issue the global loads of chunk kc
//   frag(c, j, s)   the bf16 A-fragment of sub-tile j, k-step s
//   scale<MT>(acc, cacc, c, lds, buf, lq)   acc += scaled chunk fragment
template <int MT, int PF, typename Weights, typename Rows, typename Lds>
__device__ __forceinline__ void wq_stream(Lds& lds, const WqLane& ln,
                                          const Weights& wq, const Rows& rows,
                                          const int kb, const int ke,
                                          const int n_total) {
  constexpr int NW = Weights::NW;
  constexpr int KC = WQ_KC;
  using Chunk = typename Weights::Chunk;
  const int tid = ln.tid;
  const int lq = ln.lq;
  const int la = ln.la;

  f32x4 acc[NW][MT];
#pragma unroll
  for (int j = 0; j < NW; ++j)
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[j][t] = {0.f, 0.f, 0.f, 0.f};

  // Staging of one 128-wide chunk in two halves, so that the global loads
  // of chunk c+1 issue at the top of iteration c and their ds_writes come
  // after its MFMAs: the loads have the whole compute phase to land and the
  // wait in front of the writes costs nothing. No tails (K and the split
  // ranges are multiples of 128), no per-item guards: 256 threads stage 16
  // rows per item, MT items each. With ASUM, 16 threads = one aligned
  // 16-lane DPP row per A row, so the row sum is four DPP adds; every lane
  // of the row then holds it and all 16 write the same word (no guard: a
  // guard costs a branch and a wait per item).
  auto store_a = [&](const ushort8 (&gv)[MT], int buf) {
#pragma unroll
    for (int it = 0; it < MT; ++it) {
      const int i = tid + it * 256;
      const ushort8 v = gv[it];
      *reinterpret_cast<ushort8*>(&lds.s.a_buf[buf][i / 16][(i % 16) * 8]) = v;
      if constexpr (Weights::ASUM) {
        float sum = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) sum += bf16_bits_to_float(v[e]);
        lds.s.asum[buf][i / 16] = row16_sum(sum);
      }
    }
  };

  // W ring of PF+1 chunks with COMPILE-TIME slots (the loop below is
  // unrolled over them): no register shifting, which would read a load's
  // destination and so wait for it one iteration after it was issued.
  Chunk wreg[PF + 1];
  // Branchless: past the end of the range the address clamps to its last
  // chunk (a re-read that nothing consumes). Under a branch the compiler
  // cannot count the loads in flight and falls back to s_waitcnt vmcnt(0)
  // in front of the A ds_writes, draining the prefetch just issued.
  auto load_w = [&](int kc, Chunk& dst) { wq.load(min(kc, ke - KC), dst); };

  // A loads issue BEFORE the W prefetch (issue-ordered vmcnt: the wait in
  // front of the A ds_writes then leaves the younger W loads in flight).
  {
    ushort8 gv[MT];
    rows.load(tid, kb, gv);
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
      ushort8 gv[MT];
      rows.load(tid, min(kc + KC, ke - KC), gv);  // last: an unused re-read
      const Chunk cur = wreg[u];
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
        for (int j = 0; j < NW; ++j) wf[j] = Weights::frag(cur, j, s);
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
      Weights::template scale<MT>(acc, cacc, cur, lds, buf, lq);
      store_a(gv, buf ^ 1);
      __syncthreads();  // next chunk's A is staged; this slot may be reused
      buf ^= 1;
    }
  }
  rows.template finish<NW>(lds, ln, acc, n_total);
}

// Body of a dense kernel: grid = (N/(64*NW), nsplits).
template <int MT, int PF, typename Weights>
__device__ __forceinline__ void wq_dense_gemm(
    const WqLane& ln, const Weights& wq, const WqDenseRows<MT>& rows,
    const int n_total, const int k_total, const int k_per_split) {
  __shared__ __attribute__((aligned(16)))
  WqLds<Weights::NW, Weights::ASUM> lds;
  const int kb = blockIdx.y * k_per_split;
  const int ke = min(k_total, kb + k_per_split);  // multiple of 128
  if (kb >= ke) return;  // uniform; the host never launches an empty split
  wq_stream<MT, PF>(lds, ln, wq, rows, kb, ke, n_total);
}

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------
inline int wq_mt(int m_rows) { return std::min((m_rows + 15) / 16, 4); }

}  // namespace arks

extern "C" void arks_skinny_combine(void* out, const void* part,
                                    const void* bias, int m_rows, int n_total,
                                    int nsplits, int mrows_pad,
                                    hipStream_t stream);
// Rows per split slab of the partials that a dense launch writes
// (w4_gemm.hip).
extern "C" int arks_wq_slab_rows(int m_rows);

namespace arks {

// A dense launch: launch(MT, NW, grid, block), MT and NW passed as
// std::integral_constant, starts the instantiation for m_rows (MT = 1..4) and
// nw (64-row N sub-tiles per workgroup, 1 or 2). combine = false (nsplits > 1
// only) leaves the f32 partials in `part` for a consumer that reduces them.
template <typename F>
void wq_launch_dense(void* out, const void* part, const void* bias,
                     const int m_rows, const int n_total, const int nsplits,
                     const int nw, const bool combine, hipStream_t stream,
                     F&& launch) {
  const dim3 grid(n_total / (64 * nw), nsplits), block(256);
  auto with_nw = [&](auto NW) {
    switch (wq_mt(m_rows)) {
      case 1: launch(std::integral_constant<int, 1>{}, NW, grid, block); break;
      case 2: launch(std::integral_constant<int, 2>{}, NW, grid, block); break;
      case 3: launch(std::integral_constant<int, 3>{}, NW, grid, block); break;
      default: launch(std::integral_constant<int, 4>{}, NW, grid, block);
    }
  };
  if (nw == 2)
    with_nw(std::integral_constant<int, 2>{});
  else
    with_nw(std::integral_constant<int, 1>{});
  if (nsplits > 1 && combine)
    arks_skinny_combine(out, part, bias, m_rows, n_total, nsplits,
                        arks_wq_slab_rows(m_rows), stream);
}

}  // namespace arks
