// Skinny-M GEMM for the decode hot path (gfx950): C[M,N] = A[M,K] @ W[N,K]^T,
// M <= 64 (one decode token per sequence). At these shapes the GEMM is pure
// weight streaming (arithmetic intensity M/2 flop/byte), but hipBLASLt's
// tuned algos reach only 1.3-2.9 TB/s on the decode shapes
// (profiles/r01_p2, profiles/data/dec_top r2). This kernel streams W at
// near-HBM rate:
//
//   grid = (N/64, nsplits): a workgroup owns a 64-row N-tile and a K-range.
//   W is read exactly once, 16 B/lane (guide G13), staged PF chunks ahead
//   in registers; A (the activations, tiny, L2/LLC-hot) is staged through
//   a ring of AB LDS buffers. What actually governs throughput here (r2
//   ISA audit, profiles/r02_final.md): the staging loops must be BATCHED
//   and BRANCHLESS — with per-item guards the compiler emits
//   global_load -> s_waitcnt vmcnt(0) -> ds_write per item, and because
//   vmcnt is an issue-ordered counter each of those waits also drains
//   every in-flight W prefetch, pinning the stream at ~3 TB/s no matter
//   how deep PF is. With batched staging, PF=1/AB=3 reaches ~3.9 TB/s on
//   the down-proj shape (hipBLASLt in-graph: 2.9).
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
// The file builds seven kernels: skinny_gemm_kernel<MT, 128, 1> for MT 1..4
// (AB=2 ring; launch config 0, MT from M), the tall-K kernel
// <4, 128, 2, AB=3> for the down-proj shape (config 1), the same with
// non-temporal W loads (config 2), and skinny_combine_kernel. The
// experiments that lost to these — global-direct A reads, wave-private
// barrier-free staging, silu_mul fused into the A staging, other (KC, PF)
// pairs — are recorded with their numbers in profiles/r02_final.md; the MLP
// runs silu_mul_kernel (elementwise.hip) ahead of the down-proj.
//
// N must be a multiple of 64 and K of 32 (true for every Qwen/Llama shape;
// the Python wrapper falls back to hipBLASLt otherwise).
#include "common.h"

#include <algorithm>
#include <cfloat>

namespace arks {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

__device__ __forceinline__ f32x4 sk_mfma(bf16x8 a, bf16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

constexpr int SK_NT = 64;  // N rows per workgroup (16 per wave)
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

// MT = number of 16-row M tiles (M <= 16*MT, MT in 1..4).
// KC = K elements per staged chunk (ping-pong pair in LDS).
// PF = W register-prefetch distance in chunks (in-flight W = PF*KC*2 B/row).
// AB = depth of the A ring in LDS (chunks staged AB-1 ahead).
// NT: non-temporal W loads (W is streamed exactly once; keeps it out of
// the LLC so KV/activation lines survive across decode steps).
template <int MT, int KC, int PF, int AB = 2, bool NT = false>
__global__ __launch_bounds__(256) void skinny_gemm_kernel(
    float* __restrict__ part,   // [nsplits, 16*MT, N] (nsplits > 1)
    bf16* __restrict__ out,     // [M, N] (nsplits == 1)
    const bf16* __restrict__ a, // [M, K] (row stride a_stride)
    const bf16* __restrict__ w, // [N, K] row-major
    const bf16* __restrict__ bias,  // [N] or null (applied when nsplits==1)
    const int m_rows, const int n_total, const int k_total,
    const int k_per_split, const int nsplits, const int64_t a_stride) {
  constexpr int MROWS = 16 * MT;
  constexpr int KSTEPS = KC / 32;
  const int n0 = blockIdx.x * SK_NT;
  const int kb = blockIdx.y * k_per_split;
  const int ke = min(k_total, kb + k_per_split);

  const int tid = threadIdx.x;
  const int wave = tid / WAVE_SIZE;
  const int lane = tid % WAVE_SIZE;
  const int lq = lane % 16;
  const int la = lane / 16;

  // Ping-pong A buffers; the direct-path C transpose reuses the same LDS
  // after the main loop.
  __shared__ __attribute__((aligned(16))) union {
    bf16 a_buf[AB][64][KC + SK_AP];
    float c_buf[SK_NT][64 + 1];
  } lds;

  f32x4 acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) acc[t] = {0.f, 0.f, 0.f, 0.f};

  const bf16* wrow = w + (int64_t)(n0 + wave * 16 + lq) * k_total;

  // Cooperative A staging of one chunk into buffer `buf` (no barrier here).
  // The thread->(row, col) map divides by the COMPILE-TIME chunk width, not
  // the runtime tail width: a runtime divisor compiles to a ~30-op integer
  // division sequence per index — PMC r2 (profiles/data/pmc_skinny_r2)
  // measured 2,200 VALU insts/wave (15x the MFMA count) from exactly this,
  // serializing the inter-barrier path. Tail chunks just predicate columns.
  // BRANCHLESS batched staging: all loads issue back-to-back into
  // registers, then all ds_writes. With per-item guards (`continue` /
  // row<m_rows branches) the compiler emitted load -> s_waitcnt vmcnt(0) ->
  // ds_write per item — four FULL vmem drains per chunk that serialized the
  // whole W stream (ISA audit r2, profiles/data/pmc_skinny_r2). Guards are
  // replaced by address clamps: duplicated rows / tail columns load real
  // in-bounds values that the MFMA loop never consumes.
  auto stage_a = [&](int kc, int buf) {
    constexpr int CPT = KC / 8;  // 16 B column-groups per row
    constexpr int NIT = MROWS * CPT / 256;
    ushort8 gv[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int i = tid + it * 256;
      const int row = min(i / CPT, m_rows - 1);
      const int kcol = min(kc + (i % CPT) * 8, k_total - 8);
      const bf16* base = a + (int64_t)row * a_stride + kcol;
      gv[it] = *reinterpret_cast<const ushort8*>(base);
    }
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int i = tid + it * 256;
      const int row = i / CPT;
      const int col8 = (i % CPT) * 8;
      ushort8 v = gv[it];
      *reinterpret_cast<ushort8*>(&lds.a_buf[buf][row][col8]) = v;
    }
  };

  // W fragments, register-staged PF chunks ahead (ring of PF+1 buffers,
  // shifted each chunk — the shifts are v_movs that dual-issue with MFMA).
  ushort8 wreg[PF + 1][KSTEPS];
  auto load_w = [&](int kc, ushort8 (&dst)[KSTEPS]) {
    if (kc >= ke) {
#pragma unroll
      for (int s = 0; s < KSTEPS; ++s) dst[s] = ushort8{};
      return;
    }
    const int kw = min(KC, ke - kc);
#pragma unroll
    for (int s = 0; s < KSTEPS; ++s) {
      const ushort8* src =
          reinterpret_cast<const ushort8*>(wrow + kc + s * 32 + 8 * la);
      if (s * 32 >= kw)
        dst[s] = ushort8{};
      else if constexpr (NT)
        dst[s] = __builtin_nontemporal_load(src);
      else
        dst[s] = *src;
    }
  };

  // A staging issues BEFORE the W prefetch: vmcnt is an ISSUE-ORDERED
  // counter, so a ds_write waiting on a later-issued A load would otherwise
  // drain every in-flight W prefetch each chunk — serializing the W stream
  // (measured: ~2x loss; the reordered kernel overlaps W with compute).
#pragma unroll
  for (int p = 0; p < AB - 1; ++p)
    if (kb + p * KC < ke) stage_a(kb + p * KC, p);
#pragma unroll
  for (int p = 0; p <= PF; ++p) load_w(kb + p * KC, wreg[p]);
  __syncthreads();

  int buf = 0;  // LDS slot holding the current chunk (ring of AB slots)
  for (int kc = kb; kc < ke; kc += KC) {
    const int kw = min(KC, ke - kc);  // multiple of 32
    if (kc + (AB - 1) * KC < ke) {
      int tgt = buf + (AB - 1);
      if (tgt >= AB) tgt -= AB;
      stage_a(kc + (AB - 1) * KC, tgt);  // A loads + ds_writes first (see
                                         // vmcnt note above)
    }
    ushort8 wnext[KSTEPS];
    load_w(kc + (PF + 1) * KC, wnext);  // issues during this chunk's MFMAs

#pragma unroll
    for (int s = 0; s < KSTEPS; ++s) {
      if (s * 32 >= kw) break;
      bf16x8 wfrag = *reinterpret_cast<bf16x8*>(&wreg[0][s]);
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        ushort8 af = *reinterpret_cast<const ushort8*>(
            &lds.a_buf[buf][t * 16 + lq][s * 32 + 8 * la]);
        acc[t] = sk_mfma(wfrag, *reinterpret_cast<bf16x8*>(&af), acc[t]);
      }
    }
#pragma unroll
    for (int p = 0; p < PF; ++p)
#pragma unroll
      for (int s = 0; s < KSTEPS; ++s) wreg[p][s] = wreg[p + 1][s];
#pragma unroll
    for (int s = 0; s < KSTEPS; ++s) wreg[PF][s] = wnext[s];
    __syncthreads();  // staged writes have had >= one full compute phase to
                      // land; also fences slot reuse
    buf = (buf + 1 == AB) ? 0 : buf + 1;
  }

  if (nsplits > 1) {
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
  for (int i = tid; i < m_rows * SK_NT; i += 256) {
    const int m = i / SK_NT;
    const int n = i % SK_NT;
    float v = lds.c_buf[n][m];
    if (bias != nullptr) v += bf16_bits_to_float(bias[n0 + n]);
    out[(int64_t)m * n_total + n0 + n] = float_to_bf16_bits(v);
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

// M tiles of the kernel that `config` launches for m_rows rows: the default
// ring (config 0) takes MT from M, the tall-K kernels (1, 2) are built for
// MT = 4 only.
static int skinny_mt(int m_rows, int config) {
  return config == 0 ? std::min((m_rows + 15) / 16, 4) : 4;
}

// Rows per split slab of the partials that arks_skinny_gemm writes.
extern "C" int arks_skinny_slab_rows(int m_rows, int config) {
  return 16 * skinny_mt(m_rows, config);
}

// config 0: default AB=2 ring, MT from M; 1: tall-K (PF=2, AB=3, MT=4);
// 2: tall-K with non-temporal W loads.
// combine = false (nsplits > 1 only) stops after the GEMM: the f32 partials
// stay in `part` for a consumer kernel that reduces them itself.
extern "C" void arks_skinny_gemm(void* part, void* out, const void* a,
                                 const void* w, const void* bias, int m_rows,
                                 int n_total, int k_total, int k_per_split,
                                 int nsplits, int64_t a_stride, int config,
                                 bool combine, hipStream_t stream) {
  dim3 grid(n_total / SK_NT, nsplits), block(256);
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, block, 0, stream, (float*)part,
                       (bf16*)out, (const bf16*)a, (const bf16*)w,
                       (const bf16*)bias, m_rows, n_total, k_total,
                       k_per_split, nsplits, a_stride);
  };
  if (config == 2) {
    launch(skinny_gemm_kernel<4, 128, 2, 3, true>);
  } else if (config == 1) {
    launch(skinny_gemm_kernel<4, 128, 2, 3>);
  } else {
    switch (skinny_mt(m_rows, config)) {
      case 1: launch(skinny_gemm_kernel<1, 128, 1>); break;
      case 2: launch(skinny_gemm_kernel<2, 128, 1>); break;
      case 3: launch(skinny_gemm_kernel<3, 128, 1>); break;
      default: launch(skinny_gemm_kernel<4, 128, 1>); break;
    }
  }
  if (nsplits > 1 && combine)
    arks_skinny_combine(out, part, bias, m_rows, n_total, nsplits,
                        arks_skinny_slab_rows(m_rows, config), stream);
}
