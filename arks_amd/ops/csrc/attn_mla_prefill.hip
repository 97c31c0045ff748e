// Non-absorbed MLA prefill attention for gfx950: causal varlen flash
// attention over CONTIGUOUS up-projected keys and values, QK width 192
// (128 "nope" columns per head + 64 rope columns shared by every head) and V
// width 128, plus the gather that copies a sequence's latent rows out of the
// paged cache for the up-projection GEMMs.
//
// attn_mla.hip attends in the 576-wide latent space: 1088 MACs per (query,
// key, head) pair, one workgroup per query token and head tile. That suits
// decode. A prefill chunk re-reads its whole prefix once per query token
// there; here a workgroup carries a tile of 128 or 256 query rows of one
// head over the keys (320 MACs per pair), so a staged 64-key tile is used by
// every row of the tile.
//
// The structure is the 32x32 ladder of attn_extend2.hip: each wave owns 32 q
// rows, QK^T is v_mfma_f32_32x32x16_bf16 with swapped operands (A = keys,
// B = Q) so a lane's C fragment holds the scores of ONE q row, the online
// softmax stays in registers with the defer-max rescale, P is packed into the
// PV A-fragment with v_cvt_pk_bf16_f32 + permlane32_swap, 64-key tiles are
// double-buffered in LDS with register staging and one barrier per tile.
// What differs:
//   - a K row in LDS is 384 B assembled from two global sources (the head's
//     256 B of k_nope and the shared 128 B of k_pe), XOR-swizzled in 16 B
//     chunks inside each 128 B group for ds_read_b128; QK runs 12 contraction
//     steps against 12 Q fragments (48 VGPRs);
//   - k_nope and v take a token stride and a head stride each, so the
//     head-major result of a batched matmul is read in place;
//   - the keys are contiguous per sequence (cu_seqlens_kv): no block table;
//   - a wave skips the tiles none of its 32 rows can see: in a 256-row tile
//     of a fresh prefill wave 0 sees one of the four diagonal key tiles;
//   - no KV split: heads x q tiles give the parallelism;
//   - the tile height is a template parameter (4 or 8 waves), chosen by the
//     caller's tile table; what was measured for it is in profiles/mla.md.
#include "common.h"

#include <cfloat>

namespace arks {

typedef __attribute__((ext_vector_type(8))) __bf16 mp_bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 mp_bf16x4;
typedef __attribute__((ext_vector_type(16))) float mp_f32x16;

__device__ __forceinline__ mp_f32x16 mp_mfma32(mp_bf16x8 a, mp_bf16x8 b,
                                               mp_f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

// v_cvt_pk_bf16_f32: pack two f32 into one dword of two bf16 (RNE).
__device__ __forceinline__ uint32_t mp_cvt_pk_bf16(float lo, float hi) {
  uint32_t r;
  asm volatile("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
  return r;
}

constexpr int MP_NOPE = 128;             // per-head key columns
constexpr int MP_ROPE = 64;              // shared rope key columns
constexpr int MP_QK = MP_NOPE + MP_ROPE; // 192: QK^T contraction width
constexpr int MP_V = 128;                // value / output width
constexpr int MP_KVBLK = 64;             // keys per LDS tile
constexpr int MP_STEPS = MP_QK / 16;     // 12 QK^T contraction steps
constexpr int MP_DTILES = MP_V / 32;     // 4 output tiles of 32 columns
constexpr int MP_CB = MP_V / 16;         // 16-column blocks per V row
// V image: 4-key x 16-column blocks padded to 80 elements (160 B), the
// geometry of attn_extend2.hip (conflict-free b128 staging writes, tr16
// reads).
constexpr int MP_VBLK = 80;
constexpr int MP_KBUF = MP_KVBLK * MP_QK;     // bf16 per K buffer (24 KB)
constexpr int MP_VBUF = 16 * MP_CB * MP_VBLK; // bf16 per V buffer (20 KB)
constexpr int MP_LDS_BYTES = 2 * (MP_KBUF + MP_VBUF) * 2;  // 88 KB
constexpr float MP_LOG2E = 1.44269504088896340736f;
constexpr float MP_RESCALE_THR = 8.f;  // defer-max threshold (exp2 domain)

template <int NWAVES>
__global__ __launch_bounds__(NWAVES * 64) void attn_mla_prefill_kernel(
    bf16* __restrict__ out,           // [T, H, 128]
    const bf16* __restrict__ q,       // [T, H, 192], row stride q_ts
    const bf16* __restrict__ k_nope,  // [Tkv, H, 128] by (kn_ts, kn_hs)
    const bf16* __restrict__ k_pe,    // [Tkv, 64]
    const bf16* __restrict__ v,       // [Tkv, H, 128] by (v_ts, v_hs)
    const int* __restrict__ cu_seqlens_q,   // [S + 1]
    const int* __restrict__ cu_seqlens_kv,  // [S + 1]
    const int* __restrict__ tile_info,      // [ntiles, 2] = (seq_idx, q0)
    const float scale, const int num_heads, const int total_q,
    const int total_kv, const int64_t q_ts, const int64_t kn_ts,
    const int64_t kn_hs, const int64_t v_ts, const int64_t v_hs) {
  constexpr int NT = NWAVES * 64;
  constexpr int QTILE = NWAVES * 32;
  constexpr int KCH = MP_QK / 8;                 // 24 16-byte chunks per K row
  constexpr int KVPT = MP_KVBLK * KCH / NT;      // K chunks per thread
  constexpr int VVPT = MP_KVBLK * MP_V / 8 / NT; // V chunks per thread

  const int h = blockIdx.x;
  const int seq_idx = tile_info[blockIdx.y * 2];
  const int q0 = tile_info[blockIdx.y * 2 + 1];
  const int q_start = cu_seqlens_q[seq_idx];
  const int q_len = cu_seqlens_q[seq_idx + 1] - q_start;
  const int kv_start = cu_seqlens_kv[seq_idx];
  const int kv_len = cu_seqlens_kv[seq_idx + 1] - kv_start;
  const int kv_off = kv_len - q_len;  // prefix length
  // A table row that does not describe rows of q and keys of k/v (the op
  // layer never builds one) is skipped whole: nothing is read or written.
  if (q0 < 0 || q0 >= q_len || kv_off < 0 || q_start < 0 || kv_start < 0 ||
      q_start + q_len > total_q || kv_start + kv_len > total_kv)
    return;

  const int tid = threadIdx.x;
  const int wave = tid / WAVE_SIZE;
  const int lane = tid % WAVE_SIZE;
  const int col = lane & 31;   // q row within the wave (QK^T) / column (PV)
  const int half = lane >> 5;

  extern __shared__ __attribute__((aligned(16))) char mp_lds[];
  bf16* k_lds = reinterpret_cast<bf16*>(mp_lds);  // [2][64][192], swizzled
  bf16* v_img = k_lds + 2 * MP_KBUF;              // [2][16][8][80]

  // Q fragments, loaded once: the lane's q row is q0 + 32 wave + col and
  // fragment s holds columns 16 s + 8 half .. + 7 (nope, then rope).
  const int wrow0 = q0 + wave * 32;  // this wave's first q row
  const int my_qrow = wrow0 + col;
  const bool qrow_valid = my_qrow < q_len;
  const int my_pos = kv_off + my_qrow;  // last key this q row sees
  mp_bf16x8 qfrag[MP_STEPS];
  {
    const bf16* qp = q + (int64_t)(q_start + (qrow_valid ? my_qrow : 0)) * q_ts +
                     (int64_t)h * MP_QK + 8 * half;
#pragma unroll
    for (int s = 0; s < MP_STEPS; ++s) {
      ushort8 u = *reinterpret_cast<const ushort8*>(qp + s * 16);
      qfrag[s] = *reinterpret_cast<mp_bf16x8*>(&u);
    }
  }

  // Online softmax state of q row `my_qrow` (replicated in both lane
  // halves). The running max is in raw score units, the scale is folded
  // into the exp2 argument; a masked score is a sentinel far enough below
  // any real score that its exp2 underflows to exactly 0.
  constexpr float MASKED = -3e38f;
  float m_run = -1e30f;
  float l_run = 0.f;
  mp_f32x16 oacc[MP_DTILES];
#pragma unroll
  for (int n = 0; n < MP_DTILES; ++n) oacc[n] = {};

  // Causal tile skip: the loop ends at the last key the tile's last row sees.
  const int kmax = min(kv_len, kv_off + q0 + QTILE);
  const int ntiles = (kmax + MP_KVBLK - 1) / MP_KVBLK;
  // ... and this wave's part of it at the last key ITS last row sees.
  // (none where the wave's rows lie past the sequence's end)
  const int wave_kmax = wrow0 < q_len ? min(kmax, kv_off + wrow0 + 32) : 0;
  const float scale2 = scale * MP_LOG2E;

  const bf16* kn_base = k_nope + (int64_t)kv_start * kn_ts + (int64_t)h * kn_hs;
  const bf16* kp_base = k_pe + (int64_t)kv_start * MP_ROPE;
  const bf16* v_base = v + (int64_t)kv_start * v_ts + (int64_t)h * v_hs;

  // Staging. K chunk e of a tile: key e / 24, 16-byte chunk c = e % 24 of
  // its 384 B row, chunks 0..15 from k_nope and 16..23 from k_pe. Keys past
  // kmax (the last tile only) are clamped to the last live key, so every load
  // stays inside the sequence and carries no per-element branch; their
  // scores are masked and their P is 0, so what they hold is never used
  // (finite x 0: the clamped rows are real data, never NaN padding).
  auto load_tile = [&](int j, ushort8* kr, ushort8* vr) {
    const int key_base = j * MP_KVBLK;
#pragma unroll
    for (int vv = 0; vv < KVPT; ++vv) {
      const int e = tid + NT * vv;
      const int key = e / KCH;
      const int c = e % KCH;
      const int kg = min(key_base + key, kmax - 1);
      const bf16* src = c < MP_NOPE / 8
                            ? kn_base + (int64_t)kg * kn_ts + c * 8
                            : kp_base + (int64_t)kg * MP_ROPE + (c * 8 - MP_NOPE);
      kr[vv] = *reinterpret_cast<const ushort8*>(src);
    }
#pragma unroll
    for (int vv = 0; vv < VVPT; ++vv) {
      const int e = tid + NT * vv;
      const int key = e / (MP_V / 8);
      const int col8 = (e % (MP_V / 8)) * 8;
      const int kg = min(key_base + key, kmax - 1);
      vr[vv] = *reinterpret_cast<const ushort8*>(v_base + (int64_t)kg * v_ts +
                                                 col8);
    }
  };

  auto store_tile = [&](int buf, const ushort8* kr, const ushort8* vr) {
#pragma unroll
    for (int vv = 0; vv < KVPT; ++vv) {
      const int e = tid + NT * vv;
      const int key = e / KCH;
      const int c = e % KCH;
      // XOR of bits 4..6 stays inside the chunk's 128 B group of the row
      const int swz = (c * 16) ^ ((key & 7) << 4);
      *reinterpret_cast<ushort8*>(
          reinterpret_cast<char*>(k_lds + buf * MP_KBUF + key * MP_QK) + swz) =
          kr[vv];
    }
#pragma unroll
    for (int vv = 0; vv < VVPT; ++vv) {
      const int e = tid + NT * vv;
      const int key = e / (MP_V / 8);
      const int col8 = (e % (MP_V / 8)) * 8;
      // V image: block (key / 4, col8 / 16), row key % 4, column col8 % 16
      bf16* blk = v_img + buf * MP_VBUF +
                  ((key >> 2) * MP_CB + (col8 >> 4)) * MP_VBLK;
      *reinterpret_cast<ushort8*>(blk + (key & 3) * 16 + (col8 & 15)) = vr[vv];
    }
  };

  {
    ushort8 kr0[KVPT], vr0[VVPT];
    load_tile(0, kr0, vr0);
    store_tile(0, kr0, vr0);
  }
  __syncthreads();

  int buf = 0;
  for (int j = 0; j < ntiles; ++j, buf ^= 1) {
    const int key_base = j * MP_KVBLK;
    // prefetch tile j + 1 into registers; the loads fly during the MFMAs
    ushort8 krn[KVPT], vrn[VVPT];
    if (j + 1 < ntiles) load_tile(j + 1, krn, vrn);

    // Wave-uniform: tiles past this wave's last visible key are staged for
    // the waves below it in the tile, not computed here.
    if (key_base < wave_kmax) {
      // ---- QK^T (swapped): A = 32 keys, B = Q; C[key][q row = col]. Two
      // 32-key subtiles interleave on independent accumulators.
      mp_f32x16 sc[2];
      sc[0] = {};
      sc[1] = {};
      const char* krow0 = reinterpret_cast<const char*>(
          k_lds + buf * MP_KBUF + col * MP_QK);
      const char* krow1 = krow0 + 32 * MP_QK * 2;
      const int swz_mask = (col & 7) << 4;
#pragma unroll
      for (int s = 0; s < MP_STEPS; ++s) {
        const int off = ((s * 16 + 8 * half) * 2) ^ swz_mask;
        ushort8 u0 = *reinterpret_cast<const ushort8*>(krow0 + off);
        ushort8 u1 = *reinterpret_cast<const ushort8*>(krow1 + off);
        sc[0] = mp_mfma32(*reinterpret_cast<mp_bf16x8*>(&u0), qfrag[s], sc[0]);
        sc[1] = mp_mfma32(*reinterpret_cast<mp_bf16x8*>(&u1), qfrag[s], sc[1]);
      }

      // ---- masked softmax in registers (exp2 domain). C register 4g + r of
      // subtile `sub` is key key_base + 32 sub + 8g + 4 half + r. Only
      // diagonal and ragged tiles pay the per-key compares.
      float p[32];
      const bool full_vis = (wrow0 + 31 < q_len) &&
                            (key_base + MP_KVBLK - 1 <= kv_off + wrow0) &&
                            (key_base + MP_KVBLK <= kmax);
      if (full_vis) {
#pragma unroll
        for (int sub = 0; sub < 2; ++sub)
#pragma unroll
          for (int r16 = 0; r16 < 16; ++r16) p[sub * 16 + r16] = sc[sub][r16];
      } else {
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
          const int kb_s = key_base + 32 * sub + 4 * half;
#pragma unroll
          for (int r16 = 0; r16 < 16; ++r16) {
            const int kg = kb_s + 8 * (r16 >> 2) + (r16 & 3);
            const bool ok = qrow_valid && kg <= my_pos && kg < kmax;
            p[sub * 16 + r16] = ok ? sc[sub][r16] : MASKED;
          }
        }
      }
      float mt[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) mt[i] = fmaxf(p[i], p[i + 16]);
#pragma unroll
      for (int w = 8; w > 0; w >>= 1)
#pragma unroll
        for (int i = 0; i < w; ++i) mt[i] = fmaxf(mt[i], mt[i + w]);
      const float tmax = fmaxf(mt[0], __shfl_xor(mt[0], 32, WAVE_SIZE));

      // defer-max: rescale O only when some row's tile max exceeds its
      // running max by more than the threshold (exp2(8) = 256 stays finite)
      const float thr_raw = MP_RESCALE_THR / scale2;
      if (!__all(tmax - m_run <= thr_raw)) {
        const float m_new = fmaxf(m_run, tmax);
        const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * scale2);
        l_run *= alpha;
        m_run = m_new;
        // O rows live across registers (C layout): fetch each row's alpha
        // from the lane that owns that q row
#pragma unroll
        for (int r16 = 0; r16 < 16; ++r16) {
          const int row = 8 * (r16 >> 2) + 4 * half + (r16 & 3);
          const float a_r = __shfl(alpha, 32 * half + row, WAVE_SIZE);
#pragma unroll
          for (int n = 0; n < MP_DTILES; ++n) oacc[n][r16] *= a_r;
        }
      }

      const float nms = -m_run * scale2;
#pragma unroll
      for (int i = 0; i < 32; ++i)
        p[i] = __builtin_amdgcn_exp2f(__builtin_fmaf(p[i], scale2, nms));
      float st[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) st[i] = p[i] + p[i + 16];
#pragma unroll
      for (int w = 8; w > 0; w >>= 1)
#pragma unroll
        for (int i = 0; i < w; ++i) st[i] += st[i + w];
      l_run += st[0] + __shfl_xor(st[0], 32, WAVE_SIZE);

      // ---- P -> bf16 PV A-fragments: 8 cvt_pk words per subtile; the
      // permlane32_swap pairs give each lane half its step-t fragment from
      // both halves' key sets.
      uint32_t afrag[4][4];  // [k-step t][4 dwords = 8 bf16]
#pragma unroll
      for (int sub = 0; sub < 2; ++sub) {
        uint32_t w0[4], w1[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int b = sub * 16 + 4 * g;
          w0[g] = mp_cvt_pk_bf16(p[b + 0], p[b + 1]);
          w1[g] = mp_cvt_pk_bf16(p[b + 2], p[b + 3]);
        }
#pragma unroll
        for (int tau = 0; tau < 2; ++tau) {
          auto r0 = __builtin_amdgcn_permlane32_swap(
              w0[2 * tau], w0[2 * tau + 1], false, false);
          auto r1 = __builtin_amdgcn_permlane32_swap(
              w1[2 * tau], w1[2 * tau + 1], false, false);
          const int t = sub * 2 + tau;
          afrag[t][0] = r0[0];
          afrag[t][1] = r1[0];
          afrag[t][2] = r0[1];
          afrag[t][3] = r1[1];
        }
      }

      // ---- PV: O[q row][col] += P[q row][key] V[key][col]; B fragments are
      // tr16 reads of the V image (step t: keys 16t + 8 half .. + 7).
      const int g4 = lane >> 4;
      bf16* vbase = v_img + buf * MP_VBUF;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int kb = 4 * t + 2 * (g4 >> 1);
#pragma unroll
        for (int n = 0; n < MP_DTILES; ++n) {
          const int cb = 2 * n + (g4 & 1);
          mp_bf16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
              (__attribute__((address_space(3))) mp_bf16x4*)(
                  reinterpret_cast<char*>(vbase + (kb * MP_CB + cb) * MP_VBLK) +
                  (lane & 15) * 8));
          mp_bf16x4 v2 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
              (__attribute__((address_space(3))) mp_bf16x4*)(
                  reinterpret_cast<char*>(vbase +
                                          ((kb + 1) * MP_CB + cb) * MP_VBLK) +
                  (lane & 15) * 8));
          mp_bf16x8 vb;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            vb[e] = v1[e];
            vb[e + 4] = v2[e];
          }
          oacc[n] = mp_mfma32(*reinterpret_cast<mp_bf16x8*>(&afrag[t][0]), vb,
                              oacc[n]);
        }
      }
    }

    // write-late: scatter the prefetched tile into the idle buffer
    if (j + 1 < ntiles) store_tile(buf ^ 1, krn, vrn);
    __syncthreads();
  }

  // ---- Epilogue. O register 4g + r of output tile n is q row 8g + 4 half +
  // r, column 32n + col; l_run of row `row` lives in lane `row`.
#pragma unroll
  for (int r16 = 0; r16 < 16; ++r16) {
    const int row = 8 * (r16 >> 2) + 4 * half + (r16 & 3);
    const int qrow = wrow0 + row;
    const float lr = __shfl(l_run, 32 * half + row, WAVE_SIZE);
    if (qrow >= q_len) continue;
    const float inv = lr > 0.f ? 1.f / lr : 0.f;
    const int64_t obase =
        ((int64_t)(q_start + qrow) * num_heads + h) * MP_V + col;
#pragma unroll
    for (int n = 0; n < MP_DTILES; ++n)
      out[obase + 32 * n] = float_to_bf16_bits(oacc[n][r16] * inv);
  }
}

// Copy the live latent rows of the selected sequences out of the paged
// cache into c_kv [Tkv, 512] and k_pe [Tkv, 64]: one 16-byte chunk per
// thread, 72 chunks per 576-wide row. Row r belongs to the sequence whose
// [cu_seqlens_kv[s], cu_seqlens_kv[s + 1]) holds it (unselected sequences
// have an empty range); position r - cu_seqlens_kv[s] of it is read through
// the block table.
constexpr int MP_PAGE = 16;
constexpr int MP_LAT = 512;
constexpr int MP_ROWCH = (MP_LAT + MP_ROPE) / 8;  // 72

__global__ __launch_bounds__(256) void mla_gather_rows_kernel(
    bf16* __restrict__ c_kv, bf16* __restrict__ k_pe,
    const bf16* __restrict__ cache,         // [num_blocks, 16, 576]
    const int* __restrict__ block_tables,   // [S, max_blocks]
    const int* __restrict__ cu_seqlens_kv,  // [S + 1]
    const int total_rows, const int num_seqs, const int max_blocks,
    const int num_blocks) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int row = (int)(g / MP_ROWCH);
  const int c = (int)(g % MP_ROWCH);
  if (row >= total_rows) return;
  // last s with cu_seqlens_kv[s] <= row
  int lo = 0, hi = num_seqs - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (cu_seqlens_kv[mid] <= row) lo = mid; else hi = mid - 1;
  }
  const int pos = row - cu_seqlens_kv[lo];
  const int page = min(pos / MP_PAGE, max_blocks - 1);
  int id = block_tables[(int64_t)lo * max_blocks + page];
  id = min(max(id, 0), num_blocks - 1);
  const ushort8 val = *reinterpret_cast<const ushort8*>(
      cache + ((int64_t)id * MP_PAGE + pos % MP_PAGE) * (MP_LAT + MP_ROPE) +
      c * 8);
  bf16* dst = c < MP_LAT / 8 ? c_kv + (int64_t)row * MP_LAT + c * 8
                             : k_pe + (int64_t)row * MP_ROPE + (c * 8 - MP_LAT);
  *reinterpret_cast<ushort8*>(dst) = val;
}

}  // namespace arks

using namespace arks;

extern "C" void arks_attn_mla_prefill(
    void* out, const void* q, const void* k_nope, const void* k_pe,
    const void* v, const void* cu_seqlens_q, const void* cu_seqlens_kv,
    const void* tile_info, int ntiles, int qtile, float scale, int num_heads,
    int total_q, int total_kv, int64_t q_ts, int64_t kn_ts, int64_t kn_hs, int64_t v_ts, int64_t v_hs,
    hipStream_t stream) {
  dim3 grid(num_heads, ntiles);
  static bool attr_set[2] = {false, false};
  auto launch = [&](auto kern, int nthreads, int idx) {
    if (!attr_set[idx]) {
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                hipFuncAttributeMaxDynamicSharedMemorySize,
                                MP_LDS_BYTES);
      attr_set[idx] = true;
    }
    hipLaunchKernelGGL(kern, grid, dim3(nthreads), MP_LDS_BYTES, stream,
                       (bf16*)out, (const bf16*)q, (const bf16*)k_nope,
                       (const bf16*)k_pe, (const bf16*)v,
                       (const int*)cu_seqlens_q, (const int*)cu_seqlens_kv,
                       (const int*)tile_info, scale, num_heads, total_q,
                       total_kv, q_ts, kn_ts, kn_hs, v_ts, v_hs);
  };
  if (qtile == 256) {
    launch(attn_mla_prefill_kernel<8>, 512, 0);
  } else {
    launch(attn_mla_prefill_kernel<4>, 256, 1);
  }
}

extern "C" void arks_mla_gather_rows(void* c_kv, void* k_pe, const void* cache,
                                     const void* block_tables,
                                     const void* cu_seqlens_kv, int total_rows,
                                     int num_seqs, int max_blocks,
                                     int num_blocks, hipStream_t stream) {
  const int64_t chunks = (int64_t)total_rows * MP_ROWCH;
  dim3 grid((unsigned)((chunks + 255) / 256));
  hipLaunchKernelGGL(mla_gather_rows_kernel, grid, dim3(256), 0, stream,
                     (bf16*)c_kv, (bf16*)k_pe, (const bf16*)cache,
                     (const int*)block_tables, (const int*)cu_seqlens_kv,
                     total_rows, num_seqs, max_blocks, num_blocks);
}
