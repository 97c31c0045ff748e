// Skinny-M GEMM for the decode hot path (gfx950): C[M,N] = A[M,K] @ W[N,K]^T,
// M <= 64 (one decode token per sequence). At these shapes the GEMM is pure
// weight streaming (arithmetic intensity M/2 flop/byte), but hipBLASLt's
// tuned algos reach only 1.3-2.9 TB/s on the decode shapes
// (profiles/r01_p2, profiles/data/dec_top r2).
//
//   grid = (N/64, nsplits), or (N/128, nsplits) and (N/112, nsplits) for the
//   tall-K configs: a workgroup owns an N-tile of 16 rows per wave and a
//   K-range.
//   W is read exactly once, 16 B/lane (guide G13), into a register ring of
//   SK_D = 4 chunks of 128 k per wave (16 KB of W per wave in flight).
//   A (the activations, tiny, L2-hot) rides in the same ring, one chunk
//   piece per thread issued right ahead of the W loads of its chunk, and
//   reaches the MFMAs through two ping-pong LDS buffers.
//   Two things bound this kernel (profiles/r05_skinny_stream.md):
//   (1) What a CU can fetch. A workgroup stages M x 128 of A per chunk
//   against (16 x waves) x 128 of W, through the same load path, so with
//   four waves at M = 64 half of a CU's fetches are A re-read from L2; a
//   probe build without the A loads ran the down-proj 9 us (23 %) faster.
//   Two answers, by K-range. The tall-K configs run eight waves per
//   workgroup: the same W per CU against half the A (seven where 112-row
//   tiles put a workgroup on every CU and 128-row tiles do not: the 7B
//   down-proj, 32 x 8 = 256 workgroups against 224, 8 % less W through each
//   CU's load path; in the graph 34.8 -> 32.9 us,
//   profiles/r08_all_cus.md). Split-K plans whose
//   K-range is at most 512 (qkv, o_proj) run skinny_resident_kernel
//   (config 3, below): one workgroup per CU fetches its A slice once, keeps
//   it in LDS and streams all of the CU's slabs of W past it, 0.44 bytes of
//   A per byte of W at the qkv shape instead of 1 (cold, per call: qkv
//   14.9 -> 12.5 us, o_proj 11.5 -> 10.2; profiles/r07_resident_a.md).
//   (2) The s_waitcnt pattern of the compiled loop, because vmcnt retires
//   in issue order (ISA audits: profiles/r02_final.md and r05). On its own
//   the pattern below did not move the measured time (the loop was fetch-
//   bound, not latency-bound), and neither did (1) on the old shifted ring
//   (down-proj, cold: 39.7 us; ring alone 39.0; eight waves alone 37.8;
//   both 32.4): with half the A, the loop is latency-bound again unless W
//   stays in flight. The rules the loop follows:
//     - per-item guards in a staging loop compile to load -> vmcnt(0) ->
//       ds_write per item: the staging is batched and branchless;
//     - a ring that is shifted (wreg[p] = wreg[p+1]) copies registers whose
//       loads are still out, which costs a vmcnt(0) per chunk: the ring is
//       indexed statically, the loop body is one whole turn of it;
//     - a branch around a load makes every later count conservative: the
//       steady-state turn has none, K-ranges of at most four chunks (qkv,
//       o_proj) are issued whole in the prologue, and each possible number
//       of trailing chunks has its own straight-line path;
//     - the scheduler moves loads and ds_writes across one another, which
//       changes the counts: sched_barrier fences pin the issue order.
//   In the compiled steady state every wait is a counted vmcnt(N) that
//   leaves three chunks of W outstanding; vmcnt(0) appears only where the
//   last chunk of a K-range is consumed.
//   Swapped operands (A-frag = W rows, B-frag = activations) put the C
//   fragment at [n, m], n = 4*la+r, col = lane%16 (same trick as the
//   attention kernels, guide common-mistake #6).
//   nsplits > 1 (small N) writes f32 partials [split][m][n]: 16*MT rows
//   per split, row stride N, one 16 B store per lane per M tile. That is
//   the orientation of every reader, so the reduction (fixed split order
//   from 0.f, then bias, then bf16 rounding; deterministic, no atomics)
//   is a coalesced row read. On the decode path the consumer does it —
//   splitk_add_rmsnorm_kernel (elementwise.hip) after o_proj/down_proj,
//   splitk_rope_cache_kernel (kvcache.hip) after qkv — through
//   splitk_reduce (common.h); skinny_combine_kernel is the fallback that
//   materialises a bf16 [M, N].
//
// The file builds twelve kernels: skinny_gemm_kernel<MT> for MT 1..4 (launch
// config 0, MT from M, four waves), <4, false, 8> for the tall-K plan of
// the down-proj shape (config 1, eight waves), <4, true, 8> with
// non-temporal W loads (config 2), <4, false, 7> for tall-K plans that fill
// more CUs on 112-row tiles (config 4, seven waves),
// skinny_resident_kernel<MT> for MT 1..4 (config 3: split-K with K-ranges of
// at most 512, A resident in LDS), and skinny_combine_kernel. The
// experiments that lost — global-direct A reads,
// wave-private barrier-free staging, silu_mul fused into the A staging,
// shifted rings of other (KC, PF) — are recorded with their numbers in
// profiles/r02_final.md, eight-wave and two-per-CU decompositions of the
// resident kernel in profiles/r07_resident_a.md, a flat grid with the split
// fastest (split = id % nsplits, so that an XCD's L2 sees one K-slice of A)
// in profiles/r08_all_cus.md: qkv 12.5 -> 12.8 us in the graph, the
// down-proj +0.3 to +1.5 us cold. The MLP runs silu_mul_kernel
// (elementwise.hip) ahead of the down-proj.
//
// N must be a multiple of 64 (of 16 for the tall-K configs, whose last tile
// may hang over N by whole waves) and K of 32 (true for every Qwen/Llama
// shape; the Python wrapper falls back to hipBLASLt otherwise).
#include "common.h"

#include <algorithm>
#include <atomic>
#include <cfloat>
#include <type_traits>

namespace arks {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

__device__ __forceinline__ f32x4 sk_mfma(bf16x8 a, bf16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

constexpr int SK_AP = 8;   // a_lds row pad (bf16): rows stay 16B-aligned

// Split-K epilogue: f32 partials [split][m][n] (row stride n_total, 16*MT
// rows per split). A lane holds four consecutive n for one m per M tile, so
// each tile is one 16 B store; the four la groups of a row write 64 B
// contiguous. Rows >= m_rows hold garbage and are never read.
template <int MT>
__device__ __forceinline__ void store_partials(float* __restrict__ part,
                                               const f32x4 (&acc)[MT],
                                               const int n_total,
                                               const int n, const int lq) {
  float* p = part + (int64_t)blockIdx.y * (16 * MT) * n_total + n;
#pragma unroll
  for (int t = 0; t < MT; ++t)
    *reinterpret_cast<f32x4*>(p + (int64_t)(t * 16 + lq) * n_total) = acc[t];
}

constexpr int SK_KC = 128;  // K elements per chunk (four MFMA k-steps)
constexpr int SK_D = 4;     // chunks a wave keeps in flight (register ring)

// MT = number of 16-row M tiles (M <= 16*MT, MT in 1..4).
// NT: non-temporal W loads (W is streamed exactly once; keeps it out of
// the LLC so KV/activation lines survive across decode steps).
//
// Pipeline (per workgroup, chunk i = K columns [kb + 128 i, +128)):
//   prologue  issue A_0 W_0 A_1 W_1 ... A_{D-1} W_{D-1}, no wait between
//             them; ds_write A_0; barrier
//   step i    MFMAs of chunk i (W from ring slot i % D, A from LDS i & 1)
//             issue A_{i+D}, W_{i+D} into the slot just consumed
//             ds_write A_{i+1} into LDS (i+1) & 1; barrier
// vmcnt retires in issue order, so the order above is what keeps the
// stream up: A_j and W_j sit together in the queue (within a chunk the
// compiler may interleave its A pieces among its W loads), the wait for
// W_i leaves chunks i+1 .. i+D-1 outstanding and the wait for A_{i+1}
// leaves W_{i+1} and everything newer. The ring is indexed statically
// (the loop body is one turn of D steps, no register is copied while its
// load is in flight); the up to 2D-1 chunks after the last full turn take
// one straight-line path per count, so every wait on every path is an
// exact compile-time count. 16 (W) + 1024*MT/threads (A) VGPRs per chunk in
// flight; the launch bound of two waves per SIMD keeps two 4-wave
// workgroups (or one 8-wave workgroup) on a CU.
//
// WAVES = waves per workgroup, 16 rows of W each (N tile = 16*WAVES). The A
// chunk a workgroup stages is as many bytes as the W chunk of four waves,
// and it comes through the same per-CU load path (from L2), so at WAVES = 4
// half of what a CU fetches is A. The tall-K configs run WAVES = 8, one
// 128-row workgroup per CU: the same W per CU against half the A; or
// WAVES = 7 where that occupies more CUs. There the 448 threads stage 28
// rows of A per pass, three passes for 64 rows: 48 + 64 VGPRs of ring
// against 32 + 64, 238 in all, no scratch. A wave's MFMA sequence does not
// depend on WAVES.
template <int MT, bool NT = false, int WAVES = 4>
__global__ __launch_bounds__(64 * WAVES, 2) void skinny_gemm_kernel(
    float* __restrict__ part,   // [nsplits, 16*MT, N] (nsplits > 1)
    bf16* __restrict__ out,     // [M, N] (nsplits == 1)
    const bf16* __restrict__ a, // [M, K] (row stride a_stride)
    const bf16* __restrict__ w, // [N, K] row-major
    const bf16* __restrict__ bias,  // [N] or null (applied when nsplits==1)
    const int m_rows, const int n_total, const int k_total,
    const int k_per_split, const int nsplits, const int64_t a_stride) {
  constexpr int KC = SK_KC;
  constexpr int D = SK_D;
  constexpr int KSTEPS = KC / 32;
  constexpr int CPT = KC / 8;  // 16 B column-groups per A row
  constexpr int THREADS = 64 * WAVES;
  constexpr int NTW = 16 * WAVES;        // N rows per workgroup
  constexpr int RPP = THREADS / CPT;     // A rows staged per pass
  // A loads per thread per chunk. Seven waves stage 28 rows per pass, which
  // does not divide 64: the third pass runs past row 63 (see arow, write_a).
  constexpr int NIT = (16 * MT + RPP - 1) / RPP;
  static_assert(D % 2 == 0, "LDS slot parity follows the ring slot");
  const int n0 = blockIdx.x * NTW;
  const int kb = blockIdx.y * k_per_split;
  const int ke = min(k_total, kb + k_per_split);
  const int klen = max(ke - kb, 0);        // multiple of 32
  const int nch = (klen + KC - 1) / KC;    // chunks, the last may be short

  const int tid = threadIdx.x;
  const int wave = tid / WAVE_SIZE;
  const int lane = tid % WAVE_SIZE;
  const int lq = lane % 16;
  const int la = lane / 16;

  // Ping-pong A buffers; the direct-path C transpose reuses the same LDS
  // after the main loop.
  __shared__ __attribute__((aligned(16))) union {
    bf16 a_buf[2][64][KC + SK_AP];
    float c_buf[NTW][64 + 1];
  } lds;

  f32x4 acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) acc[t] = {0.f, 0.f, 0.f, 0.f};

  // The last workgroup of a WAVES = 7 or 8 launch may hang over N (N is a
  // multiple of 16, not of the tile): its upper waves stream the last row
  // again and store nothing.
  const bool wave_live = n0 + wave * 16 < n_total;
  const bf16* wrow =
      w + (int64_t)min(n0 + wave * 16 + lq, n_total - 1) * k_total + 8 * la;

  // Cooperative A staging: thread -> (row, 16 B column group) by the
  // COMPILE-TIME chunk width (a runtime divisor costs a ~30-op division per
  // index, PMC r2). Branchless: rows past m_rows and columns past k_total
  // are clamped to real in-bounds values that the MFMAs never consume.
  // Where the passes overshoot the 16*MT rows (WAVES = 7), the threads past
  // the last row load it again (m_rows - 1 <= 16*MT - 1 is their clamp too)
  // and write_a puts the same bytes in the same place a second time: no
  // guard around a load or a ds_write, and the counts stay exact.
  const int acol = (tid % CPT) * 8;
  const bf16* arow[NIT];
#pragma unroll
  for (int it = 0; it < NIT; ++it)
    arow[it] = a + (int64_t)min(tid / CPT + it * RPP, m_rows - 1) * a_stride;

  // The register ring: W fragments and the A piece of D chunks.
  ushort8 wreg[D][KSTEPS];
  ushort8 areg[D][NIT];

  // Issue every load of chunk `ch`, A ahead of W, nothing waited for.
  // Addresses past the K-range are clamped into the row (k-steps past ke
  // are never consumed), so nothing reads past the end of A or W.
  // A chunk that does not exist (`live` false; prologue of a K-range shorter
  // than the ring) is still issued, so that the counts stay exact, but
  // every lane reads the first 16 B of the operand: one line, not sixteen.
  auto issue = [&](int ch, ushort8 (&wd)[KSTEPS], ushort8 (&ad)[NIT],
                   bool live) {
    const int kc = kb + ch * KC;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const bf16* src = arow[it] + min(kc + acol, k_total - 8);
      ad[it] = *reinterpret_cast<const ushort8*>(live ? src : a);
    }
#pragma unroll
    for (int s = 0; s < KSTEPS; ++s) {
      const bf16* wsrc = wrow + min(kc + s * 32, k_total - 32);
      const ushort8* src =
          reinterpret_cast<const ushort8*>(live ? wsrc : w);
      if constexpr (NT)
        wd[s] = __builtin_nontemporal_load(src);
      else
        wd[s] = *src;
    }
  };
  auto write_a = [&](const ushort8 (&ad)[NIT], int buf) {
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      int row = tid / CPT + it * RPP;
      if constexpr (NIT * RPP != 16 * MT) row = min(row, 16 * MT - 1);
      *reinterpret_cast<ushort8*>(&lds.a_buf[buf][row][acol]) = ad[it];
    }
  };
  // MFMAs of one chunk, ascending k; kw = valid width (multiple of 32).
  auto mfma_chunk = [&](const ushort8 (&wd)[KSTEPS], int buf, int kw) {
#pragma unroll
    for (int s = 0; s < KSTEPS; ++s) {
      if (s * 32 >= kw) break;
      ushort8 wv = wd[s];
      bf16x8 wfrag = *reinterpret_cast<bf16x8*>(&wv);
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        ushort8 af = *reinterpret_cast<const ushort8*>(
            &lds.a_buf[buf][t * 16 + lq][s * 32 + 8 * la]);
        acc[t] = sk_mfma(wfrag, *reinterpret_cast<bf16x8*>(&af), acc[t]);
      }
    }
  };

#pragma unroll
  for (int p = 0; p < D; ++p) {
    issue(p, wreg[p], areg[p], p < nch);
    __builtin_amdgcn_sched_barrier(0);  // chunks enter the queue in order
  }
  write_a(areg[0], 0);
  __syncthreads();

  int c = 0;  // next chunk to consume; a multiple of D, so it is in slot 0
  // One turn of the ring: D full chunks from slots 0..D-1, the first
  // `nrefill` of them refilled with chunk c + D + s (which must exist; it
  // may be the short tail). Straight-line code, no branch around a load.
  auto ring_turn = [&](auto nrefill) {
    constexpr int R = decltype(nrefill)::value;
#pragma unroll
    for (int s = 0; s < D; ++s) {
      // The fences pin the order the counts above rely on: left alone, the
      // scheduler hoists the ds_writes (and their wait) over the refill.
      mfma_chunk(wreg[s], s & 1, KC);
      __builtin_amdgcn_sched_barrier(0);
      if (s < R) issue(c + D + s, wreg[s], areg[s], true);
      __builtin_amdgcn_sched_barrier(0);
      if (s + 1 < D || R > 0) {
        write_a(areg[(s + 1) % D], (s + 1) & 1);
        __syncthreads();
      }
    }
    c += D;
  };
  // The last `n` chunks (slots 0..n-1), nothing refilled; only the last
  // one may be short.
  auto drain = [&](auto nleft) {
    constexpr int R = decltype(nleft)::value;
#pragma unroll
    for (int s = 0; s < R; ++s) {
      mfma_chunk(wreg[s], s & 1, s + 1 < R ? KC : klen - (c + s) * KC);
      if (s + 1 < R) {
        write_a(areg[s + 1], (s + 1) & 1);
        __syncthreads();
      }
    }
  };
  using std::integral_constant;
  // Steady state: every slot refilled, no branch and no vmcnt(0) inside.
  while (c + 2 * D <= nch) ring_turn(integral_constant<int, D>{});
  // D..2D-1 chunks left: one partly refilled turn, then the rest. Each
  // count has its own straight-line path, so its waits are exact counts.
  switch (nch - c) {
    case 7: ring_turn(integral_constant<int, 3>{});
            drain(integral_constant<int, 3>{}); break;
    case 6: ring_turn(integral_constant<int, 2>{});
            drain(integral_constant<int, 2>{}); break;
    case 5: ring_turn(integral_constant<int, 1>{});
            drain(integral_constant<int, 1>{}); break;
    case 4: drain(integral_constant<int, 4>{}); break;
    case 3: drain(integral_constant<int, 3>{}); break;
    case 2: drain(integral_constant<int, 2>{}); break;
    case 1: drain(integral_constant<int, 1>{}); break;
    default: break;  // empty K-range
  }
  static_assert(D == 4, "the tail switch is written out for D = 4");

  if (nsplits > 1) {
    if (wave_live)
      store_partials<MT>(part, acc, n_total, n0 + wave * 16 + 4 * la, lq);
    return;
  }

  // Direct epilogue: transpose C^T through LDS so the [M, N] store is
  // row-contiguous (128 B per m-row per workgroup).
  __syncthreads();  // all a_buf reads done before the union flips to c_buf
#pragma unroll
  for (int t = 0; t < MT; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      lds.c_buf[wave * 16 + 4 * la + r][t * 16 + lq] = acc[t][r];
    }
  }
  __syncthreads();
  const int nvalid = min(NTW, n_total - n0);
  for (int i = tid; i < m_rows * NTW; i += THREADS) {
    const int m = i / NTW;
    const int n = i % NTW;
    if (n >= nvalid) continue;
    float v = lds.c_buf[n][m];
    if (bias != nullptr) v += bf16_bits_to_float(bias[n0 + n]);
    out[(int64_t)m * n_total + n0 + n] = float_to_bf16_bits(v);
  }
}

// ---------------------------------------------------------------------------
// A-resident kernel for short K-ranges (launch config 3, split-K only).
//
// grid = (groups, nsplits). A workgroup belongs to one split and owns a run
// of 16-row slabs of W (wave v takes every SKR_WAVES-th of them). Its whole
// A slice, 16*MT x K-range, is staged into LDS once (row stride
// k_per_split + SK_AP, dynamic LDS); after that one barrier the waves run
// on their own: no A load, no ds_write and no barrier per chunk.
//
// Per wave:
//   prologue  issue the A piece (one row of the slice per wave per pass, all
//             passes at once), then the W of the first R slabs, whole;
//             wait for A only (a counted vmcnt: the W stays out while A
//             is written to LDS), ds_write it, barrier. A goes first
//             because vmcnt retires in issue order: behind the W loads,
//             the wait for A would be a wait for all of them.
//   slab i    MFMAs over the K-range, ascending k (W from ring slot i % R,
//             A from LDS); store_partials; refill the slot with slab i + R
// The ring is indexed statically and holds whole slabs: R = 2 slabs of 3-4
// chunks or 3 of 1-2 (at most 128 VGPRs of W). The chunk count of the
// K-range (1..4, uniform per workgroup) selects one straight-line
// instantiation of the whole stream, and within it every possible number
// of slabs left after the last full turn has its own path, as in the
// kernel above, so every wait is an exact count (ISA table in
// profiles/r07_resident_a.md; vmcnt(0) only where a wave's last slab is
// consumed). Slots that no slab is left for are still loaded in the
// prologue, one line, as in `issue` of the kernel above.
// Four waves, one workgroup per CU measured fastest (eight waves, or more
// workgroups than CUs, lost 1-4 us per call at the decode shapes).
// An accumulator sees the MFMA sequence of skinny_gemm_kernel<MT> for the
// same split boundaries, so the partials are bit-equal to config 0's.
// ---------------------------------------------------------------------------
constexpr int SKR_WAVES = 4;
constexpr int SKR_KMAX = 512;  // longest K-range (four chunks)

template <int MT>
__global__ __launch_bounds__(64 * SKR_WAVES, 2) void skinny_resident_kernel(
    float* __restrict__ part,   // [nsplits, 16*MT, N]
    const bf16* __restrict__ a, // [M, K] (row stride a_stride)
    const bf16* __restrict__ w, // [N, K] row-major
    const int m_rows, const int n_total, const int k_total,
    const int k_per_split, const int64_t a_stride, const int slabs_per_group) {
  constexpr int KC = SK_KC;
  constexpr int WAVES = SKR_WAVES;
  constexpr int NA = 16 * MT / WAVES;  // A rows (loads) per thread
  static_assert(NA * WAVES == 16 * MT, "A rows must divide over the waves");
  extern __shared__ __attribute__((aligned(16))) bf16 a_lds[];
  const int lstride = k_per_split + SK_AP;  // a_lds row stride (bf16)

  const int kb = blockIdx.y * k_per_split;
  const int ke = min(k_total, kb + k_per_split);
  const int klen = max(ke - kb, 0);        // multiple of 32, <= SKR_KMAX
  const int nch = (klen + KC - 1) / KC;

  const int tid = threadIdx.x;
  const int wave = tid / WAVE_SIZE;
  const int lane = tid % WAVE_SIZE;
  const int lq = lane % 16;
  const int la = lane / 16;

  // This workgroup's slabs [slab0, slab0 + nwg); wave v takes slab0 + v,
  // slab0 + v + WAVES, ...: nsl of them (0 where the groups outnumber N).
  const int slab0 = blockIdx.x * slabs_per_group;
  const int nwg = max(min(slabs_per_group, n_total / 16 - slab0), 0);
  const int nsl = (nwg - wave + WAVES - 1) / WAVES;

  // A piece of this thread: row it * WAVES + wave, 16 B at column lcol of
  // the K-range. Branchless: rows past m_rows are clamped to the last row,
  // and lanes past the K-range to its last vector, which they load and
  // write again (the same bytes to the same place). With a guard around the
  // ds_writes the compiler sinks the loads into it, behind the W loads,
  // and the wait for A becomes a vmcnt(0).
  ushort8 areg[NA];
  const int lcol = max(min(8 * lane, klen - 8), 0);
  const int acol = min(kb + lcol, k_total - 8);
  auto load_a = [&]() {
#pragma unroll
    for (int it = 0; it < NA; ++it)
      areg[it] = *reinterpret_cast<const ushort8*>(
          a + (int64_t)min(it * WAVES + wave, m_rows - 1) * a_stride + acol);
    __builtin_amdgcn_sched_barrier(0);  // A enters the queue ahead of W
  };
  auto stage_a = [&]() {
#pragma unroll
    for (int it = 0; it < NA; ++it)
      *reinterpret_cast<ushort8*>(
          &a_lds[(it * WAVES + wave) * lstride + lcol]) = areg[it];
    __syncthreads();
  };

  const bf16* wlane = w + 8 * la;
  const bf16* afrag = a_lds + lq * lstride + 8 * la;
  using std::integral_constant;

  auto stream = [&](auto nch_c) {
    constexpr int NCH = decltype(nch_c)::value;
    constexpr int KS = NCH * (KC / 32);   // k-steps (loads) per slab
    constexpr int R = NCH >= 3 ? 2 : 3;   // slabs in flight
    ushort8 wreg[R][KS];

    // Issue the W of the wave's slab i, whole; nothing waited for. k-steps
    // past the K-range are clamped into the row and never consumed.
    auto issue = [&](int i, ushort8 (&wd)[KS], bool live) {
      const bf16* wrow =
          wlane +
          (int64_t)((slab0 + wave + i * WAVES) * 16 + lq) * k_total;
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const bf16* src = wrow + min(kb + s * 32, k_total - 32);
        wd[s] = *reinterpret_cast<const ushort8*>(live ? src : w);
      }
    };
    // MFMAs of slab i from its ring slot, ascending k, then its partials.
    auto consume = [&](int i, const ushort8 (&wd)[KS]) {
      f32x4 acc[MT];
#pragma unroll
      for (int t = 0; t < MT; ++t) acc[t] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        // only the last chunk may be short
        if (s >= KS - KC / 32 && s * 32 >= klen) break;
        ushort8 wv = wd[s];
        bf16x8 wfrag = *reinterpret_cast<bf16x8*>(&wv);
#pragma unroll
        for (int t = 0; t < MT; ++t) {
          ushort8 af = *reinterpret_cast<const ushort8*>(
              afrag + t * 16 * lstride + s * 32);
          acc[t] = sk_mfma(wfrag, *reinterpret_cast<bf16x8*>(&af), acc[t]);
        }
      }
      store_partials<MT>(part, acc, n_total,
                         (slab0 + wave + i * WAVES) * 16 + 4 * la, lq);
    };

    // Every load of a path is issued inside it. The marker differs per
    // path, which keeps the compiler from hoisting the common loads above
    // the switch: with loads out across it, the paths after the first
    // opened with a vmcnt(0) ahead of their W loads.
    asm volatile("; resident path, %0 chunks" ::"n"(NCH));
    load_a();
#pragma unroll
    for (int p = 0; p < R; ++p) {
      issue(p, wreg[p], p < nsl);
      __builtin_amdgcn_sched_barrier(0);  // slabs enter the queue in order
    }
    stage_a();
    __builtin_amdgcn_sched_barrier(0);

    int c = 0;  // next slab to consume; a multiple of R, so it is in slot 0
    // One turn of the ring: R slabs from slots 0..R-1, the first `nrefill`
    // slots refilled with slab c + R + s (which must exist).
    auto ring_turn = [&](auto nrefill) {
      constexpr int NR = decltype(nrefill)::value;
#pragma unroll
      for (int s = 0; s < R; ++s) {
        consume(c + s, wreg[s]);
        __builtin_amdgcn_sched_barrier(0);
        if (s < NR) issue(c + R + s, wreg[s], true);
        __builtin_amdgcn_sched_barrier(0);
      }
      c += R;
    };
    auto drain = [&](auto nleft) {
      constexpr int NL = decltype(nleft)::value;
#pragma unroll
      for (int s = 0; s < NL; ++s) consume(c + s, wreg[s]);
    };
    // REM slabs left, 0 < REM < 2R: a partly refilled turn, then the rest.
    auto tail = [&](auto rem) {
      constexpr int REM = decltype(rem)::value;
      if constexpr (REM >= 2 * R) {
        // not reachable for this R
      } else if constexpr (REM >= R) {
        ring_turn(integral_constant<int, REM - R>{});
        drain(integral_constant<int, REM - R>{});
      } else {
        drain(integral_constant<int, REM>{});
      }
    };
    // Steady state: every slot refilled, no branch around a load.
    while (c + 2 * R <= nsl) ring_turn(integral_constant<int, R>{});
    switch (nsl - c) {
      case 5: tail(integral_constant<int, 5>{}); break;
      case 4: tail(integral_constant<int, 4>{}); break;
      case 3: tail(integral_constant<int, 3>{}); break;
      case 2: tail(integral_constant<int, 2>{}); break;
      case 1: tail(integral_constant<int, 1>{}); break;
      default: break;
    }
    static_assert(R <= 3, "the tail switch is written out for R <= 3");
  };

  switch (nch) {
    case 4: stream(integral_constant<int, 4>{}); break;
    case 3: stream(integral_constant<int, 3>{}); break;
    case 2: stream(integral_constant<int, 2>{}); break;
    default: stream(integral_constant<int, 1>{}); break;  // or empty: zeros
  }
}

// Reduce the split partials: out[m][n] = bf16(sum_s part[s][m][n] + bias[n]).
// Partials and output share the [m][n] orientation, so this is elementwise:
// each thread owns four consecutive n of one row (16 B loads per split, all
// issued before the adds; 8 B store). The decode path does not launch this —
// its consumers (rmsnorm / rope) reduce the partials themselves; it remains
// for callers that need a materialised [M, N].
__global__ __launch_bounds__(256) void skinny_combine_kernel(
    bf16* __restrict__ out, const float* __restrict__ part,
    const bf16* __restrict__ bias, const int m_rows, const int n_total,
    const int nsplits, const int64_t split_stride) {
  const int nq = n_total / 4;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= m_rows * nq) return;
  const int m = i / nq;
  const int n = (i % nq) * 4;
  const float* const p[1] = {part + (int64_t)m * n_total + n};
  float4v s[1];
  splitk_reduce<1, 2>(p, split_stride, nsplits, s);
  ushort4v o;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float v = s[0][e];
    if (bias != nullptr) v += bf16_bits_to_float(bias[n + e]);
    o[e] = float_to_bf16_bits(v);
  }
  *reinterpret_cast<ushort4v*>(out + (int64_t)m * n_total + n) = o;
}

}  // namespace arks

using namespace arks;

// Fallback for callers that need a materialised [M, N]: reduce partials
// written by a partials-only GEMM launch (mrows_pad = rows per split slab).
extern "C" void arks_skinny_combine(void* out, const void* part,
                                    const void* bias, int m_rows, int n_total,
                                    int nsplits, int mrows_pad,
                                    hipStream_t stream) {
  dim3 cgrid((m_rows * (n_total / 4) + 255) / 256), cblock(256);
  hipLaunchKernelGGL(skinny_combine_kernel, cgrid, cblock, 0, stream,
                     (bf16*)out, (const float*)part, (const bf16*)bias, m_rows,
                     n_total, nsplits, (int64_t)mrows_pad * n_total);
}

// M tiles of the kernel that `config` launches for m_rows rows: configs 0
// and 3 take MT from M, the tall-K configs (1, 2, 4) always run MT = 4
// (64-row slabs, which the tall-K plan's consumers expect).
static int skinny_mt(int m_rows, int config) {
  return config == 0 || config == 3 ? std::min((m_rows + 15) / 16, 4) : 4;
}

// Rows per split slab of the partials that arks_skinny_gemm writes.
extern "C" int arks_skinny_slab_rows(int m_rows, int config) {
  return 16 * skinny_mt(m_rows, config);
}

// Longest k_per_split config 3 takes (its A slice must fit in LDS).
extern "C" int arks_skinny_resident_kmax() { return SKR_KMAX; }

// Compute units of the current device, queried once per device.
static int device_cu_count() {
  constexpr int MAX_DEV = 64;
  static std::atomic<int> cus[MAX_DEV];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_DEV) dev = 0;
  int n = cus[dev].load(std::memory_order_relaxed);
  if (n == 0) {
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount,
                              dev) != hipSuccess || n <= 0)
      n = 1;
    cus[dev].store(n, std::memory_order_relaxed);
  }
  return n;
}

// Config 3. groups = workgroups per split; 0 = one workgroup per compute
// unit over all splits, so that every A slice is fetched once per CU and
// the (slab, split) units come out even (qkv at 7B: 32 x 8 workgroups of 9
// slabs on 256 CUs).
template <int MT>
static void launch_resident(float* part, const bf16* a, const bf16* w,
                            int m_rows, int n_total, int k_total,
                            int k_per_split, int nsplits, int64_t a_stride,
                            int groups, hipStream_t stream) {
  const int slabs = n_total / 16;
  // An explicit count is taken as given: groups past the last slab exit
  // after the barrier.
  if (groups <= 0)
    groups = std::min(std::max(device_cu_count() / nsplits, 1), slabs);
  const int per_group = (slabs + groups - 1) / groups;
  const size_t lds = (size_t)16 * MT * (k_per_split + SK_AP) * sizeof(bf16);
  // Above 64 KB (K-range 512 at MT = 4) the size has to be opted into.
  if (lds > 64 * 1024)
    (void)hipFuncSetAttribute(
        reinterpret_cast<const void*>(&skinny_resident_kernel<MT>),
        hipFuncAttributeMaxDynamicSharedMemorySize,
        16 * MT * (SKR_KMAX + SK_AP) * (int)sizeof(bf16));
  hipLaunchKernelGGL(skinny_resident_kernel<MT>, dim3(groups, nsplits),
                     dim3(64 * SKR_WAVES), lds, stream, part, a, w, m_rows,
                     n_total, k_total, k_per_split, a_stride, per_group);
}

// config 0: MT from M, four waves; 1: tall-K plan (MT=4, eight waves);
// 2: tall-K with non-temporal W loads; 3: A-resident, split-K only
// (nsplits > 1, k_per_split <= SKR_KMAX), `groups` workgroups per split
// (0 = auto; the other configs ignore it); 4: tall-K on seven waves
// (112-row tiles: 3584 / 112 x 8 splits is one workgroup on each of 256
// CUs, where 128-row tiles leave 32 idle; N a multiple of 16).
// combine = false (nsplits > 1 only) stops after the GEMM: the f32 partials
// stay in `part` for a consumer kernel that reduces them itself.
extern "C" void arks_skinny_gemm(void* part, void* out, const void* a,
                                 const void* w, const void* bias, int m_rows,
                                 int n_total, int k_total, int k_per_split,
                                 int nsplits, int64_t a_stride, int config,
                                 bool combine, hipStream_t stream,
                                 int groups = 0) {
  if (config == 3) {
    auto launch = [&](auto mt) {
      launch_resident<decltype(mt)::value>(
          (float*)part, (const bf16*)a, (const bf16*)w, m_rows, n_total,
          k_total, k_per_split, nsplits, a_stride, groups, stream);
    };
    switch (skinny_mt(m_rows, config)) {
      case 1: launch(std::integral_constant<int, 1>{}); break;
      case 2: launch(std::integral_constant<int, 2>{}); break;
      case 3: launch(std::integral_constant<int, 3>{}); break;
      default: launch(std::integral_constant<int, 4>{}); break;
    }
    if (combine)
      arks_skinny_combine(out, part, bias, m_rows, n_total, nsplits,
                          arks_skinny_slab_rows(m_rows, config), stream);
    return;
  }
  // The tall-K configs run 8 or 7 waves (128 or 112 rows of W) per
  // workgroup.
  const int waves = config == 0 ? 4 : config == 4 ? 7 : 8;
  dim3 grid((n_total + 16 * waves - 1) / (16 * waves), nsplits);
  dim3 block(64 * waves);
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, block, 0, stream, (float*)part,
                       (bf16*)out, (const bf16*)a, (const bf16*)w,
                       (const bf16*)bias, m_rows, n_total, k_total,
                       k_per_split, nsplits, a_stride);
  };
  if (config == 4) {
    launch(skinny_gemm_kernel<4, false, 7>);
  } else if (config == 2) {
    launch(skinny_gemm_kernel<4, true, 8>);
  } else if (config == 1) {
    launch(skinny_gemm_kernel<4, false, 8>);
  } else {
    switch (skinny_mt(m_rows, config)) {
      case 1: launch(skinny_gemm_kernel<1>); break;
      case 2: launch(skinny_gemm_kernel<2>); break;
      case 3: launch(skinny_gemm_kernel<3>); break;
      default: launch(skinny_gemm_kernel<4>); break;
    }
  }
  if (nsplits > 1 && combine)
    arks_skinny_combine(out, part, bias, m_rows, n_total, nsplits,
                        arks_skinny_slab_rows(m_rows, config), stream);
}
