// Sort-free top-k / top-p / min-p filter for the samplers.
//
// The kept set of a row is a prefix of the strict order (value descending,
// index ascending, NaN never) that sample_take already defines, so one pair
// (cut_val, cut_idx) describes it: token i is kept iff
//   v_i > cut_val || (v_i == cut_val && i <= cut_idx).
// sample_cutoff_kernel computes that pair for every row in one launch, and
// the Gumbel sampler (sampling.hip) skips what lies past it. Definition:
// ref.sample_cutoff.
//
// A bf16 logit has 65,536 possible values, so no sort is needed: a two-level
// 256-bin radix select over an order-preserving 16-bit key finds the cutoff
// value. Level 1 (the key's high byte) carries a count and a probability mass
// per bin; level 2 (the low byte, within the bin level 1 picked) carries
// counts only, since each of its bins is one exact value whose mass is
// count * mass(value). Masses are 2^40 fixed point: integer LDS atomics
// commute, so the histograms, and with them the cutoff, are bit-identical
// from run to run however the hardware orders the adds.
//
// One 1024-thread workgroup per row; the row (304 KB at a 152k vocabulary)
// is read three times, a fourth only when ties of the cutoff value have to
// be split by index, and stays in L2 after the first.
#include "common.h"

#include <cfloat>

namespace arks {

constexpr int CUT_BLOCK = 1024;
constexpr int CUT_WAVES = CUT_BLOCK / WAVE_SIZE;
constexpr int CUT_BINS = 256;
// Private histogram copies, picked by lane % copies and laid out
// [bin][copy]: the lanes of one wave that hit the same bin (logits crowd
// into a handful of level-1 bins, which are two octaves wide) spread over
// that many addresses in different banks instead of serialising on one.
constexpr int CUT_COPIES1 = 16;
constexpr int CUT_COPIES2 = 8;  // x 2 histograms (top-k bin, top-p bin)
constexpr int CUT_SLOTS = CUT_BINS * CUT_COPIES1;
static_assert(CUT_SLOTS == 2 * CUT_BINS * CUT_COPIES2, "one LDS array, two uses");
constexpr int CUT_ALL = 0x7fffffff;  // every tie kept; also the keep-all index
constexpr int CUT_UNROLL = 4;        // 16-byte loads in flight per thread
constexpr float CUT_ONE = 1099511627776.f;  // 2^40

__device__ __forceinline__ bool cut_is_nan(uint32_t bits) {
  return (bits & 0x7fffu) > 0x7f80u;
}

// Order-preserving key of a non-NaN bf16: unsigned key order = float order.
// -0 takes the key of +0, so that one key is one float value.
__device__ __forceinline__ uint32_t cut_key(uint32_t bits) {
  bits = bits == 0x8000u ? 0u : bits;
  return bits ^ ((bits & 0x8000u) ? 0xffffu : 0x8000u);
}

__device__ __forceinline__ float cut_key_value(uint32_t key) {
  return bf16_bits_to_float(
      (uint16_t)(key ^ ((key & 0x8000u) ? 0x8000u : 0xffffu)));
}

// exp((v - max) / T) in 2^40 fixed point, scale = log2(e) / T. A token equal
// to the maximum weighs exactly 1, also where the maximum is +-inf and
// v - max would be NaN. The difference may overflow to -inf (weight 0) but
// never to NaN; weights under 2^-40 truncate to 0, so the raw v_exp_f32,
// which flushes results under 2^-126, loses nothing. Levels 1 and 2 both
// come through here, so a level-2 bin's mass is its share of level 1's.
__device__ __forceinline__ uint64_t cut_mass(float v, float mx, float scale) {
  if (v == mx) return 1ull << 40;
  const float d = v - mx;
  return (uint64_t)(__builtin_amdgcn_exp2f(d * scale) * CUT_ONE);
}

// f(bits, index) for every token of the row, spread over the workgroup in no
// particular order. Whole 16-byte vectors are loaded CUT_UNROLL at a time,
// all issued before the first is used; the up to 7 tokens before the first
// aligned address (a row stride that is no multiple of 8 shifts later rows)
// and the up to 7 after the last whole vector are handled scalar.
template <typename F>
__device__ __forceinline__ void cut_for_each(const bf16* __restrict__ lrow,
                                             const int vocab, F&& f) {
  const int skew = (int)((reinterpret_cast<uintptr_t>(lrow) & 15) >> 1);
  const int head = min(vocab, (8 - skew) & 7);
  const int nvec = (vocab - head) / 8;
  const ushort8* body = reinterpret_cast<const ushort8*>(lrow + head);
  for (int i0 = threadIdx.x; i0 < nvec; i0 += CUT_UNROLL * CUT_BLOCK) {
    ushort8 x[CUT_UNROLL];
#pragma unroll
    for (int u = 0; u < CUT_UNROLL; ++u) {
      const int i = i0 + u * CUT_BLOCK;
      if (i < nvec) x[u] = body[i];
    }
#pragma unroll
    for (int u = 0; u < CUT_UNROLL; ++u) {
      const int i = i0 + u * CUT_BLOCK;
      if (i < nvec) {
#pragma unroll
        for (int j = 0; j < 8; ++j) f((uint32_t)x[u][j], head + i * 8 + j);
      }
    }
  }
  const int tail = head + nvec * 8;
  if ((int)threadIdx.x < head) f((uint32_t)lrow[threadIdx.x], (int)threadIdx.x);
  if (tail + (int)threadIdx.x < vocab)
    f((uint32_t)lrow[tail + threadIdx.x], tail + (int)threadIdx.x);
}

// Wave 0 scans 256 bins in descending key order, four per lane: lane l holds
// bins 255 - 4l - j (j = 0..3) with counts c[j] and masses m[j]. Returns the
// count and mass of all bins above the lane's first one, and the totals.
__device__ __forceinline__ void cut_wave_scan(const uint32_t (&c)[4],
                                              const uint64_t (&m)[4],
                                              uint32_t& c_above,
                                              uint64_t& m_above,
                                              uint32_t& c_total,
                                              uint64_t& m_total) {
  const int lane = threadIdx.x % WAVE_SIZE;
  uint32_t ci = c[0] + c[1] + c[2] + c[3];
  uint64_t mi = m[0] + m[1] + m[2] + m[3];
  const uint32_t c_own = ci;
  const uint64_t m_own = mi;
#pragma unroll
  for (int off = 1; off < WAVE_SIZE; off <<= 1) {
    const uint32_t oc = __shfl_up(ci, off, WAVE_SIZE);
    const unsigned long long om =
        __shfl_up((unsigned long long)mi, off, WAVE_SIZE);
    if (lane >= off) {
      ci += oc;
      mi += om;
    }
  }
  c_total = __shfl(ci, WAVE_SIZE - 1, WAVE_SIZE);
  m_total = __shfl((unsigned long long)mi, WAVE_SIZE - 1, WAVE_SIZE);
  c_above = ci - c_own;
  m_above = mi - m_own;
}

// What the scans hand on through LDS. A candidate is (value, ties): the kept
// set is everything above the value plus the first `ties` tokens of that
// value in index order (CUT_ALL = all of them).
struct CutState {
  float mx;
  int kbin, pbin;        // level-1 bins of the top-k / top-p crossing, -1 = off
  uint32_t k_above;      // tokens in bins above kbin
  uint64_t p_above;      // mass in bins above pbin
  uint64_t p_target;     // floor(top_p * Z), at least 1
  uint32_t total;        // non-NaN tokens
  float val;             // the winning candidate
  int ties;
  float wave_max[CUT_WAVES];
  uint32_t wave_cnt[CUT_WAVES];
};

// The tighter of two candidates: the higher value; at equal values the one
// that keeps fewer ties. NaN never tightens.
__device__ __forceinline__ void cut_tighten(float val, int ties, float& best,
                                            int& best_ties) {
  if (val > best || (val == best && ties < best_ties)) {
    best = val;
    best_ties = ties;
  }
}

__global__ __launch_bounds__(CUT_BLOCK) void sample_cutoff_kernel(
    float* __restrict__ cut_val,             // [rows]
    int* __restrict__ cut_idx,               // [rows]
    const bf16* __restrict__ logits,         // [rows, vocab]
    const float* __restrict__ temperatures,  // [rows]
    const int* __restrict__ top_k,           // [rows], <= 0 or >= vocab: off
    const float* __restrict__ top_p,         // [rows], >= 1: off
    const float* __restrict__ min_p,         // [rows], <= 0: off
    const int vocab) {
  const int row = blockIdx.x;
  const float t = temperatures[row];
  const int k_arg = top_k[row];
  const uint32_t k = (k_arg > 0 && k_arg < vocab) ? (uint32_t)k_arg : 0u;
  const float tp = top_p[row];
  const float mp = min_p[row];
  const bool p_on = tp < 1.f;
  const bool m_on = mp > 0.f;
  if (!(t > 0.f) || (k == 0u && !p_on && !m_on)) {
    if (threadIdx.x == 0) {
      cut_val[row] = -INFINITY;
      cut_idx[row] = CUT_ALL;
    }
    return;
  }
  const bf16* lrow = logits + (int64_t)row * vocab;
  const int lane = threadIdx.x % WAVE_SIZE;
  const int wave = threadIdx.x / WAVE_SIZE;

  __shared__ uint32_t h_cnt[CUT_SLOTS];
  __shared__ uint64_t h_mass[CUT_SLOTS];
  __shared__ uint32_t f_cnt[2][CUT_BINS];  // folded copies
  __shared__ uint64_t f_mass[CUT_BINS];
  __shared__ CutState st;

  for (int i = threadIdx.x; i < CUT_SLOTS; i += CUT_BLOCK) {
    h_cnt[i] = 0u;
    h_mass[i] = 0ull;
  }

  // ---- pass A: the maximum over non-NaN tokens (fmaxf drops NaN) --------
  float mx = -INFINITY;
  cut_for_each(lrow, vocab, [&](uint32_t bits, int) {
    mx = fmaxf(mx, bf16_bits_to_float((uint16_t)bits));
  });
  mx = wave_reduce_max(mx);
  if (lane == 0) st.wave_max[wave] = mx;
  __syncthreads();
  mx = st.wave_max[0];
#pragma unroll
  for (int w = 1; w < CUT_WAVES; ++w) mx = fmaxf(mx, st.wave_max[w]);
  const float scale = 1.4426950408889634f / t;

  // ---- pass B: level-1 histogram, count and mass per high byte ----------
  {
    const int copy = lane % CUT_COPIES1;
    cut_for_each(lrow, vocab, [&](uint32_t bits, int) {
      if (cut_is_nan(bits)) return;
      const int slot = (int)(cut_key(bits) >> 8) * CUT_COPIES1 + copy;
      atomicAdd(&h_cnt[slot], 1u);
      atomicAdd(reinterpret_cast<unsigned long long*>(&h_mass[slot]),
                (unsigned long long)cut_mass(
                    bf16_bits_to_float((uint16_t)bits), mx, scale));
    });
  }
  __syncthreads();
  if (threadIdx.x < CUT_BINS) {
    uint32_t c = 0u;
    uint64_t m = 0ull;
#pragma unroll
    for (int j = 0; j < CUT_COPIES1; ++j) {
      c += h_cnt[threadIdx.x * CUT_COPIES1 + j];
      m += h_mass[threadIdx.x * CUT_COPIES1 + j];
    }
    f_cnt[0][threadIdx.x] = c;
    f_mass[threadIdx.x] = m;
  }
  if (threadIdx.x == 0) {
    st.kbin = -1;
    st.pbin = -1;
    st.val = -INFINITY;
    st.ties = CUT_ALL;
  }
  __syncthreads();
  if (wave == 0) {
    uint32_t c[4];
    uint64_t m[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      c[j] = f_cnt[0][255 - 4 * lane - j];
      m[j] = f_mass[255 - 4 * lane - j];
    }
    uint32_t ca, ct;
    uint64_t ma, z;
    cut_wave_scan(c, m, ca, ma, ct, z);
    // the nucleus ends where the exclusive cumulative mass reaches
    // top_p * Z; at least 1, so that the top token (mass 2^40) is inside
    uint64_t target = 0ull;
    if (p_on) {
      target = (uint64_t)((double)fmaxf(tp, 0.f) * (double)z);
      target = target < 1ull ? 1ull : target;
    }
    if (lane == 0) {
      st.total = ct;
      st.p_target = target;
    }
    // exactly one bin holds each crossing (none for top-k when fewer than
    // k tokens are not NaN)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (k != 0u && c[j] != 0u && ca < k && k <= ca + c[j]) {
        st.kbin = 255 - 4 * lane - j;
        st.k_above = ca;
      }
      if (p_on && m[j] != 0ull && ma < target && target <= ma + m[j]) {
        st.pbin = 255 - 4 * lane - j;
        st.p_above = ma;
      }
      ca += c[j];
      ma += m[j];
    }
  }
  __syncthreads();
  if (st.total == 0u) {  // nothing but NaN: nothing to keep, nothing to cut
    if (threadIdx.x == 0) {
      cut_val[row] = -INFINITY;
      cut_idx[row] = CUT_ALL;
    }
    return;
  }

  // ---- pass C: level-2 counts over the low byte, both bins at once ------
  const int kbin = st.kbin;
  const int pbin = st.pbin;
  const int pset = pbin == kbin ? 0 : 1;
  if (kbin >= 0 || pbin >= 0) {
    for (int i = threadIdx.x; i < CUT_SLOTS; i += CUT_BLOCK) h_cnt[i] = 0u;
    __syncthreads();
    const int copy = lane % CUT_COPIES2;
    cut_for_each(lrow, vocab, [&](uint32_t bits, int) {
      if (cut_is_nan(bits)) return;
      const uint32_t key = cut_key(bits);
      const int hi = (int)(key >> 8);
      const int slot = (int)(key & 0xffu) * CUT_COPIES2 + copy;
      if (hi == kbin) atomicAdd(&h_cnt[slot], 1u);
      if (hi == pbin && pset == 1)
        atomicAdd(&h_cnt[CUT_BINS * CUT_COPIES2 + slot], 1u);
    });
    __syncthreads();
    if (threadIdx.x < 2 * CUT_BINS) {
      uint32_t c = 0u;
#pragma unroll
      for (int j = 0; j < CUT_COPIES2; ++j)
        c += h_cnt[threadIdx.x * CUT_COPIES2 + j];
      f_cnt[threadIdx.x / CUT_BINS][threadIdx.x % CUT_BINS] = c;
    }
    __syncthreads();
    if (wave == 0) {
      // each bin is one value: its mass is count * mass(value)
      uint32_t ck[4], cp[4];
      uint64_t q[4], m[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int b = 255 - 4 * lane - j;
        ck[j] = kbin >= 0 ? f_cnt[0][b] : 0u;
        cp[j] = pbin >= 0 ? f_cnt[pset][b] : 0u;
        q[j] = cp[j] != 0u
                   ? cut_mass(cut_key_value((uint32_t)(pbin << 8 | b)), mx,
                              scale)
                   : 0ull;
        m[j] = q[j] * cp[j];
      }
      uint32_t ca, ct;
      uint64_t ma, mt;
      cut_wave_scan(ck, m, ca, ma, ct, mt);
      ca += st.k_above;
      ma += st.p_above;
      const uint64_t target = st.p_target;
      float val = -INFINITY;
      int ties = CUT_ALL;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int b = 255 - 4 * lane - j;
        if (ck[j] != 0u && ca < k && k <= ca + ck[j]) {
          // the k-th token has this value; k - above of its ties still fit
          const uint32_t fit = k - ca;
          cut_tighten(cut_key_value((uint32_t)(kbin << 8 | b)),
                      fit == ck[j] ? CUT_ALL : (int)fit, val, ties);
        }
        if (m[j] != 0ull && ma < target && target <= ma + m[j]) {
          // tie number i (from 0) is kept while above + i * q < target
          const uint64_t fit = (target - ma + q[j] - 1ull) / q[j];
          cut_tighten(cut_key_value((uint32_t)(pbin << 8 | b)),
                      fit >= cp[j] ? CUT_ALL : (int)fit, val, ties);
        }
        ca += ck[j];
        ma += m[j];
      }
      // at most two lanes hold a candidate: fold them with the same rule
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(val, off, WAVE_SIZE);
        const int ot = __shfl_xor(ties, off, WAVE_SIZE);
        cut_tighten(ov, ot, val, ties);
      }
      if (lane == 0) {
        st.val = val;
        st.ties = ties;
      }
    }
    __syncthreads();
  }

  // min-p needs no histogram: p >= min_p * p_max  <=>  v >= max + T ln(min_p),
  // every tie kept; never above the maximum, so the top token survives
  float val = st.val;
  int ties = st.ties;
  if (m_on) cut_tighten(fminf(mx + t * logf(mp), mx), CUT_ALL, val, ties);

  if (ties == CUT_ALL) {
    if (threadIdx.x == 0) {
      cut_val[row] = val;
      cut_idx[row] = CUT_ALL;
    }
    return;
  }

  // ---- pass D: the index of the ties-th token equal to val ---------------
  // Each thread owns a contiguous run of vectors (thread 0 also the scalar
  // head, the last thread the tail), so thread order is index order.
  const int skew = (int)((reinterpret_cast<uintptr_t>(lrow) & 15) >> 1);
  const int head = min(vocab, (8 - skew) & 7);
  const int nvec = (vocab - head) / 8;
  const int tail = head + nvec * 8;
  const int per = (nvec + CUT_BLOCK - 1) / CUT_BLOCK;
  const int v0 = min((int)threadIdx.x * per, nvec);
  const int v1 = min(v0 + per, nvec);
  const ushort8* body = reinterpret_cast<const ushort8*>(lrow + head);
  // f(index) for the thread's tokens equal to val, ascending
  auto for_equal = [&](auto&& f) {
    if (threadIdx.x == 0)
      for (int i = 0; i < head; ++i)
        if (bf16_bits_to_float(lrow[i]) == val) f(i);
    for (int i = v0; i < v1; ++i) {
      const ushort8 x = body[i];
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (bf16_bits_to_float(x[j]) == val) f(head + i * 8 + j);
    }
    if (threadIdx.x == CUT_BLOCK - 1)
      for (int i = tail; i < vocab; ++i)
        if (bf16_bits_to_float(lrow[i]) == val) f(i);
  };
  uint32_t mine = 0u;
  for_equal([&](int) { ++mine; });
  uint32_t incl = mine;
#pragma unroll
  for (int off = 1; off < WAVE_SIZE; off <<= 1) {
    const uint32_t o = __shfl_up(incl, off, WAVE_SIZE);
    if (lane >= off) incl += o;
  }
  if (lane == WAVE_SIZE - 1) st.wave_cnt[wave] = incl;
  __syncthreads();
  uint32_t before = incl - mine;
  for (int w = 0; w < wave; ++w) before += st.wave_cnt[w];
  // the one thread whose run holds occurrence number `ties` (from 1)
  if (before < (uint32_t)ties && (uint32_t)ties <= before + mine) {
    uint32_t left = (uint32_t)ties - before;
    int found = CUT_ALL;
    for_equal([&](int idx) {
      if (--left == 0u) found = idx;
    });
    cut_val[row] = val;
    cut_idx[row] = found;
  }
}

// In place: -inf past the row's cutoff (NaN included: it is never kept).
// grid = (rows, ceil(vocab / 2048)), a thread owns 8 consecutive tokens.
// Keep-all rows are not touched at all.
__global__ void apply_sample_cutoff_kernel(bf16* __restrict__ logits,
                                           const float* __restrict__ cut_val,
                                           const int* __restrict__ cut_idx,
                                           const int vocab) {
  const int row = blockIdx.x;
  const float cv = cut_val[row];
  const int ci = cut_idx[row];
  if (cv == -INFINITY && ci == CUT_ALL) return;
  const int idx0 = (blockIdx.y * 256 + threadIdx.x) * 8;
  if (idx0 >= vocab) return;
  bf16* lrow = logits + (int64_t)row * vocab;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int idx = idx0 + j;
    if (idx >= vocab) break;
    const float v = bf16_bits_to_float(lrow[idx]);
    if (!(v > cv || (v == cv && idx <= ci))) lrow[idx] = 0xff80;  // bf16 -inf
  }
}

}  // namespace arks

using namespace arks;

extern "C" {

void arks_sample_cutoff(void* cut_val, void* cut_idx, const void* logits,
                        const void* temperatures, const void* top_k,
                        const void* top_p, const void* min_p, int rows,
                        int vocab, hipStream_t stream) {
  hipLaunchKernelGGL(sample_cutoff_kernel, dim3(rows), dim3(CUT_BLOCK), 0,
                     stream, (float*)cut_val, (int*)cut_idx,
                     (const bf16*)logits, (const float*)temperatures,
                     (const int*)top_k, (const float*)top_p,
                     (const float*)min_p, vocab);
}

void arks_apply_sample_cutoff(void* logits, const void* cut_val,
                              const void* cut_idx, int rows, int vocab,
                              hipStream_t stream) {
  hipLaunchKernelGGL(apply_sample_cutoff_kernel,
                     dim3(rows, (vocab + 2047) / 2048), dim3(256), 0, stream,
                     (bf16*)logits, (const float*)cut_val,
                     (const int*)cut_idx, vocab);
}

}  // extern "C"
