// Routed grouped bf16 GEMM over the local experts of an MoE block, gfx950:
//   for e < E_local, i < counts[e], p = pairs[e][i]:
//     out[p, :] = a[p / src_div, :] @ W[e]        W bf16 [E, K, N], N contiguous
// W is MoEMLP.w13 / w2 as the model holds them ([E, in, out]); counts / pairs
// are the routing table of moe_route_kernel (moe.hip). Only the experts the
// batch selected are read.
//
// The weight is K-MAJOR: a 16 B global load gives 8 consecutive n at one k,
// while the MFMA fragment wants 8 consecutive k at one n. wq_stream.h feeds
// fragments straight from registers because its weights are [N, K] rows; here
// the transposition goes through LDS, as the attention kernels do for V
// (attn_decode.hip): b128 stores into an image of 4k x 16n blocks, fragments
// read back with ds_read_b64_tr_b16.
//
// Work split: 256 threads, grid = (N/128, E_local, slabs of 64 list rows), a
// function of (N, E_local, max_rows) only. A workgroup owns 128 output
// columns of one expert for one slab and walks the WHOLE K in chunks of 64,
// so the reduction order over K is a function of K alone: chunk after chunk,
// two 32-k MFMA steps per chunk, into one f32 fragment per (n, m) tile. Wave
// w owns columns 32w..32w+31 (two 16-column tiles) and all MT live 16-row M
// tiles. No K split, no atomics, no workspace; one RNE rounding at the store.
// A row's result is therefore bit-identical whatever the batch, the routing,
// the slab it lands in and the MT body that computes it.
//
// Data flow per chunk (KC = 64):
//   global -> registers   W: a wave reads 4 k-rows x 256 B (whole contiguous
//                         row segments of the N tile), 4 x 16 B per thread
//                         per chunk. A: gathered rows through prow[], 16 B
//                         per thread per 32 rows. Both are issued up to
//                         THREE chunks ahead into a register ring with
//                         compile-time slots (the loop is unrolled by two), A
//                         before W as in wq_stream, all addresses clamped
//                         instead of branched so that the waits stay counted.
//   registers -> LDS      after the chunk's MFMAs, into the other half of a
//                         double-buffered image; one barrier per chunk.
//   LDS -> fragments      W by two tr16 reads per (16-column tile, k-step),
//                         A by one b128 read per (M tile, k-step).
//   Swapped operands as in wq_stream (A-frag = W^T rows, B-frag =
//   activations): the C fragment is [n = 4*la + r, m = lane % 16], so a lane
//   stores its four n of row m as one 8 B store straight from registers.
//
// W image: block (kb = k/4, cb = n/16) holds 4 k x 16 n row-major (128 B),
// exactly what one tr16 read of 16 lanes consumes (lane l reads 8 B at
// 8*l and receives k = 0..3 of column l). Blocks of one kb are 80 bf16
// (40 dwords) apart, kb rows 672 bf16 (336 dwords) apart:
//   b128 stores  16 lanes of a pass write one k-row's 8 blocks (2 lanes per
//                block); 40*cb mod 64 = 0,40,16,56,32,8,48,24 plus 8*(k%4):
//                eight disjoint 8-dword bank groups;
//   tr16 reads   32 lanes of a pass read blocks kb and kb + 2 of one cb;
//                2*336 mod 64 = 32: the two 32-dword blocks take the two
//                halves of the 64 banks.
// A image: [64 rows][64 + 8] bf16; the 36-dword row stride puts the sixteen
// rows of a b128 fragment read on sixteen disjoint 4-dword bank groups.
// LDS = 2 * (21504 + 9216) + 256 = 61696 B: two workgroups per CU.
//
// N % 128 == 0, K % 64 == 0 (bindings.cpp checks both).
#include "common.h"

namespace arks {

typedef __attribute__((ext_vector_type(8))) __bf16 mg_bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 mg_bf16x4;
typedef __attribute__((ext_vector_type(4))) float mg_f32x4;

constexpr int MG_NT = 128;    // output columns per workgroup
constexpr int MG_SLAB = 64;   // list rows per workgroup
constexpr int MG_KC = 64;     // k per chunk
constexpr int MG_AP = 8;      // A image row pad (bf16)
constexpr int MG_WB = 80;     // W image: bf16 between blocks of one kb
constexpr int MG_WKB = 672;   // W image: bf16 between kb rows

struct MgLds {
  bf16 w[2][(MG_KC / 4) * MG_WKB];
  bf16 a[2][MG_SLAB][MG_KC + MG_AP];
  int prow[MG_SLAB];
};

// One chunk in flight for a thread: AI = ceil(MT / 2) gathered 16 B pieces of
// A (32 rows per piece over the workgroup) and four 16 B pieces of W.
template <int AI>
struct MgChunk {
  ushort8 a[AI];
  ushort8 w[4];
};

// The chunk loop and the epilogue for MT live 16-row tiles.
template <int MT>
__device__ __forceinline__ void mg_slab(MgLds& lds, bf16* __restrict__ out,
                                        const bf16* __restrict__ a,
                                        const bf16* __restrict__ w,
                                        const int rows, const int src_div,
                                        const int n_total, const int k_total) {
  constexpr int AI = (MT + 1) / 2;
  const int tid = threadIdx.x;
  const int wave = tid / WAVE_SIZE;
  const int lq = tid % WAVE_SIZE % 16;
  const int la = tid % WAVE_SIZE / 16;
  const int n0 = blockIdx.x * MG_NT;

  // Sources of this thread's staging pieces, resolved once. A: piece `it`
  // is row tid/8 + 32*it, k = 8*(tid%8).. of the chunk (rows past the list's
  // end are prow's clamped duplicates, never stored). W: piece q is k-row
  // 16*q + tid/16 of the chunk, columns n0 + 8*(tid%16)..; a wave's 64 lanes
  // cover four whole 256 B row segments = the eight blocks of one kb.
  const bf16* asrc[AI];
#pragma unroll
  for (int it = 0; it < AI; ++it)
    asrc[it] = a + (int64_t)(lds.prow[tid / 8 + 32 * it] / src_div) * k_total +
               (tid % 8) * 8;
  const bf16* wsrc = w + (int64_t)(tid / 16) * n_total + n0 + (tid % 16) * 8;
  // kb = 4*q + wave, block cb = (tid%16)/2, row k%4 = lane/16, half tid%2
  const int wdst = wave * MG_WKB + ((tid % 16) / 2) * MG_WB + la * 16 +
                   (tid % 2) * 8;

  const int kend = k_total - MG_KC;  // first k of the last chunk
  // Branchless: past the end the address clamps to the last chunk (a re-read
  // that nothing consumes), so the compiler can count the loads in flight.
  auto load = [&](int kc, MgChunk<AI>& c) {
    kc = min(kc, kend);
#pragma unroll
    for (int it = 0; it < AI; ++it)
      c.a[it] = *reinterpret_cast<const ushort8*>(asrc[it] + kc);
#pragma unroll
    for (int q = 0; q < 4; ++q)
      c.w[q] = *reinterpret_cast<const ushort8*>(
          wsrc + (int64_t)(kc + 16 * q) * n_total);
  };
  auto stage = [&](const MgChunk<AI>& c, const int buf) {
#pragma unroll
    for (int it = 0; it < AI; ++it)
      *reinterpret_cast<ushort8*>(&lds.a[buf][tid / 8 + 32 * it][(tid % 8) * 8]) =
          c.a[it];
#pragma unroll
    for (int q = 0; q < 4; ++q)
      *reinterpret_cast<ushort8*>(&lds.w[buf][wdst + 4 * q * MG_WKB]) = c.w[q];
  };

  mg_f32x4 acc[2][MT];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[j][t] = {0.f, 0.f, 0.f, 0.f};

  // Ring of two chunks in registers; chunk 0 goes to LDS before the loop.
  MgChunk<AI> ring[2];
  load(0, ring[0]);
  load(MG_KC, ring[1]);
  stage(ring[0], 0);
  load(2 * MG_KC, ring[0]);
  __syncthreads();

  // Iteration kc: LDS half `buf` holds chunk kc, ring[u ^ 1] chunk kc + 64,
  // ring[u] chunk kc + 128 (in flight).
  int buf = 0;
  for (int kc0 = 0; kc0 < k_total; kc0 += 2 * MG_KC) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int kc = kc0 + u * MG_KC;
      if (kc >= k_total) break;  // uniform
      // Take chunk kc + 64 out of its slot and refill the slot with chunk
      // kc + 192 BEFORE the MFMAs: the wait in front of the LDS writes below
      // then leaves two younger chunks in flight.
      const MgChunk<AI> next = ring[u ^ 1];
      load(kc + 3 * MG_KC, ring[u ^ 1]);
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        mg_bf16x8 wf[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          // k = 32s + 8la + 0..3 is block kb = 8s + 2la, + 4..7 the next one
          const bf16* blk = &lds.w[buf][(8 * s + 2 * la) * MG_WKB +
                                        (2 * wave + j) * MG_WB + 4 * lq];
          const mg_bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
              (__attribute__((address_space(3))) mg_bf16x4*)(blk));
          const mg_bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
              (__attribute__((address_space(3))) mg_bf16x4*)(blk + MG_WKB));
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            wf[j][i] = lo[i];
            wf[j][i + 4] = hi[i];
          }
        }
#pragma unroll
        for (int t = 0; t < MT; ++t) {
          ushort8 af = *reinterpret_cast<const ushort8*>(
              &lds.a[buf][t * 16 + lq][32 * s + 8 * la]);
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc[j][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                wf[j], *reinterpret_cast<mg_bf16x8*>(&af), acc[j][t], 0, 0, 0);
        }
      }
      // chunk kc + 64 into the other half: its readers passed the barrier of
      // the previous iteration.
      stage(next, buf ^ 1);
      __syncthreads();
      buf ^= 1;
    }
  }

  // acc[j][t][r] is out row t*16 + lq, column n0 + 32*wave + 16*j + 4*la + r.
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    const int m = t * 16 + lq;
    if (m >= rows) continue;
    bf16* orow = out + (int64_t)lds.prow[m] * n_total + n0 + 32 * wave + 4 * la;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      ushort4v v;
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = float_to_bf16_bits(acc[j][t][r]);
      *reinterpret_cast<ushort4v*>(orow + 16 * j) = v;
    }
  }
}

// Grid = (N/128, E_local, slabs). The same uniform early return, prow table
// and clamps as w4_moe_gemm_kernel (w4_gemm.hip): counts to t_cols, pair
// indices to n_pairs, so no table content can index past what the host
// checked. MT = ceil(rows / 16) is picked once, uniformly.
__global__ __launch_bounds__(256) void moe_bf16_gemm_kernel(
    bf16* __restrict__ out,          // [n_pairs, N]
    const bf16* __restrict__ a,      // [>= ceil(n_pairs / src_div), K]
    const bf16* __restrict__ w,      // [E, K, N]
    const int* __restrict__ counts,  // [E]
    const int* __restrict__ pairs,   // [E, t_cols]
    const int t_cols, const int n_pairs, const int src_div, const int n_total,
    const int k_total) {
  const int e = blockIdx.y;
  const int cnt = min(max(counts[e], 0), t_cols);
  const int r0 = blockIdx.z * MG_SLAB;
  if (r0 >= cnt) return;  // uniform
  const int rows = min(cnt - r0, MG_SLAB);

  __shared__ __attribute__((aligned(16))) MgLds lds;
  if (threadIdx.x < MG_SLAB) {
    const int p = pairs[(int64_t)e * t_cols + r0 +
                        min((int)threadIdx.x, rows - 1)];
    lds.prow[threadIdx.x] = min(max(p, 0), n_pairs - 1);
  }
  __syncthreads();

  const bf16* we = w + (int64_t)e * k_total * n_total;
  switch ((rows + 15) / 16) {
    case 1: mg_slab<1>(lds, out, a, we, rows, src_div, n_total, k_total); break;
    case 2: mg_slab<2>(lds, out, a, we, rows, src_div, n_total, k_total); break;
    case 3: mg_slab<3>(lds, out, a, we, rows, src_div, n_total, k_total); break;
    default: mg_slab<4>(lds, out, a, we, rows, src_div, n_total, k_total);
  }
}

}  // namespace arks

using namespace arks;

// slabs = ceil(max_rows / 64).
extern "C" void arks_moe_bf16_gemm(void* out, const void* a, const void* w,
                                   const void* counts, const void* pairs,
                                   int n_experts, int t_cols, int n_pairs,
                                   int src_div, int slabs, int n_total,
                                   int k_total, hipStream_t stream) {
  dim3 grid(n_total / MG_NT, n_experts, slabs), block(256);
  hipLaunchKernelGGL(moe_bf16_gemm_kernel, grid, block, 0, stream, (bf16*)out,
                     (const bf16*)a, (const bf16*)w, (const int*)counts,
                     (const int*)pairs, t_cols, n_pairs, src_div, n_total,
                     k_total);
}
