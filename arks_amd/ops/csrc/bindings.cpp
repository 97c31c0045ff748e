// Python bindings for the arks_amd gfx950 kernels (torch extension).
// Host-side validation lives here; kernels are in the *.hip files.
#include <torch/extension.h>

#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

namespace py = pybind11;

// --- kernel launchers (see the .hip files) ---
extern "C" {
void arks_rmsnorm(void* out, const void* input, const void* weight, float eps,
                  int rows, int hidden, hipStream_t stream);
void arks_fused_add_rmsnorm(void* out, const void* input, void* residual,
                            const void* weight, float eps, int rows, int hidden,
                            hipStream_t stream);
void arks_silu_mul(void* out, const void* gate_up, int64_t rows, int d,
                   hipStream_t stream);
int arks_pool_max_hidden();
void arks_pool_embed(void* out, void* carry, void* part, const void* x,
                     const void* residual, const void* weight,
                     const void* segs, const void* slabs, int nsegs,
                     int nslabs, float eps, int hidden, int dims,
                     int normalize, hipStream_t stream);
void arks_rope_inplace(const void* positions, void* q, void* k,
                       const void* cos_sin, int num_tokens, int head_dim,
                       int num_q_heads, int num_kv_heads, int64_t q_stride,
                       int64_t k_stride, hipStream_t stream);
void arks_reshape_and_cache(const void* k, const void* v, void* k_cache,
                            void* v_cache, const void* slot_mapping,
                            int num_tokens, int num_kv_heads, int head_dim,
                            int block_size, int64_t kv_stride, int kv_fp8,
                            hipStream_t stream);
void arks_rope_and_cache(const void* positions, void* q, void* k,
                         const void* v, void* k_cache, void* v_cache,
                         const void* slot_mapping, const void* cos_sin,
                         int num_tokens, int head_dim, int num_q_heads,
                         int num_kv_heads, int block_size, int64_t q_stride,
                         int64_t k_stride, int kv_fp8, hipStream_t stream);
void arks_attn_decode_paged(void* out, void* part_out, const void* q,
                            const void* k_cache, const void* v_cache,
                            const void* block_tables, const void* seq_lens,
                            float scale, int num_seqs, int num_q_heads,
                            int num_kv_heads, int head_dim, int max_blocks,
                            int nparts, int64_t q_stride, int kv_fp8,
                            int window, hipStream_t stream);
void arks_attn_prefill_varlen(void* out, const void* q, const void* k,
                              const void* v, const void* cu_seqlens,
                              const void* tile_info, int ntiles, float scale,
                              int num_q_heads, int num_kv_heads, int head_dim,
                              int64_t q_stride, int64_t kv_stride, int window,
                              hipStream_t stream);
void arks_attn_extend_paged(void* out, const void* q, const void* k_cache,
                            const void* v_cache, const void* block_tables,
                            const void* kv_lens, const void* cu_seqlens_q,
                            const void* tile_info, int ntiles, float scale,
                            int num_q_heads, int num_kv_heads, int head_dim,
                            int max_blocks, int64_t q_stride, int kv_fp8,
                            int window, hipStream_t stream);
void arks_attn_extend_paged2(void* out, const void* q, const void* k_cache,
                             const void* v_cache, const void* block_tables,
                             const void* kv_lens, const void* cu_seqlens_q,
                             const void* tile_info, void* part_ws, int ntiles,
                             float scale, int num_q_heads, int num_kv_heads,
                             int head_dim, int max_blocks, int64_t q_stride,
                             int window, hipStream_t stream);
void arks_attn_extend2_combine(void* out, const void* part_ws,
                               const void* combine_table,
                               const void* cu_seqlens_q, int n_split,
                               float scale, int num_q_heads, int head_dim,
                               hipStream_t stream);
void arks_quant_fp8_rows(void* out, void* inv_scale, const void* x, int rows,
                         int cols, hipStream_t stream);
void arks_rmsnorm_fp8(void* out, void* inv_scale, const void* input,
                      void* residual, const void* weight, float eps, int rows,
                      int hidden, int fused_add, hipStream_t stream);
void arks_silu_mul_fp8(void* out, void* inv_scale, const void* gate_up,
                       int rows, int d, hipStream_t stream);
void arks_skinny_gemm(void* part, void* out, const void* a, const void* w,
                      const void* bias, int m_rows, int n_total, int k_total,
                      int k_per_split, int nsplits, int64_t a_stride,
                      int config, bool combine, hipStream_t stream,
                      int groups);
int arks_skinny_slab_rows(int m_rows, int config);
int arks_skinny_resident_kmax();
void arks_skinny_combine(void* out, const void* part, const void* bias,
                         int m_rows, int n_total, int nsplits, int mrows_pad,
                         hipStream_t stream);
void arks_splitk_add_rmsnorm(void* out, const void* part, const void* bias,
                             void* residual, const void* weight, float eps,
                             int rows, int hidden, int nsplits, int mrows_pad,
                             hipStream_t stream);
void arks_splitk_rope_and_cache(const void* positions, const void* part,
                                const void* bias, void* q_out, void* k_cache,
                                void* v_cache, const void* slot_mapping,
                                const void* cos_sin, int num_tokens,
                                int head_dim, int num_q_heads,
                                int num_kv_heads, int block_size, int nsplits,
                                int mrows_pad, int kv_fp8, int groups,
                                hipStream_t stream);
void arks_greedy_sample(void* out, void* pairs, const void* logits, int rows,
                        int vocab, int chunks, hipStream_t stream);
void arks_gumbel_sample(void* out, void* pairs, const void* logits,
                        const void* temperatures, const void* uniform,
                        int rows, int vocab, int chunks, hipStream_t stream);
void arks_greedy_sample_masked(void* out, const void* logits,
                               const void* masks, const void* mask_row,
                               int rows, int vocab, int slots,
                               hipStream_t stream);
void arks_gumbel_sample_masked(void* out, const void* logits,
                               const void* temperatures, const void* uniform,
                               const void* masks, const void* mask_row,
                               int rows, int vocab, int slots,
                               hipStream_t stream);
void arks_apply_token_bitmask(void* logits, int is_fp32, const void* masks,
                              const void* mask_row, int rows, int vocab,
                              int slots, hipStream_t stream);
void arks_ar_seq_inc(void* seq, hipStream_t stream);
void arks_one_shot_allreduce(void* out, const void* src, void* mail_ptrs[8],
                             void* flag_ptrs[8], void* seq, int rank,
                             int world, int64_t n, hipStream_t stream);
void arks_moe_topk(void* weights, void* ids, const void* logits, int T,
                   int E, int k, int renorm, hipStream_t stream);
void arks_moe_mix(void* out, const void* y, const void* weights,
                  const void* ids, int T, int H, int k, int expert_base,
                  int n_local, hipStream_t stream);
void arks_moe_mix_rows(void* out, const void* y, const void* weights,
                       const void* rows, int T, int H, int k,
                       hipStream_t stream);
void arks_lora_shrink(void* h, const void* x, const void* a, const void* tiles,
                      int ntiles, int T, int K, int SR, int max_loras,
                      hipStream_t stream);
void arks_lora_expand(void* y, const void* h, const void* b, const void* tiles,
                      int ntiles, int T, int N, int R, int S, int off1,
                      int off2, int max_loras, hipStream_t stream);
void arks_w4_skinny_gemm(void* part, void* out, const void* a, const void* qw,
                         const void* scales, const void* zeros,
                         const void* bias, int m_rows, int n_total,
                         int k_total, int k_per_split, int nsplits,
                         int64_t a_stride, int nw, bool combine,
                         hipStream_t stream);
int arks_wq_slab_rows(int m_rows);
void arks_w4_dequant(void* out, const void* qw, const void* scales,
                     const void* zeros, int n_total, int k_total,
                     hipStream_t stream);
void arks_w4_moe_gemm(void* out, const void* a, const void* qw,
                      const void* scales, const void* zeros,
                      const void* counts, const void* pairs, int n_experts,
                      int t_cols, int n_pairs, int src_div, int slabs,
                      int n_total, int k_total, int nw, hipStream_t stream);
void arks_w8_skinny_gemm(void* part, void* out, const void* a, const void* w8,
                         const void* scales, const void* bias, int m_rows,
                         int n_total, int k_total, int k_per_split,
                         int nsplits, int64_t a_stride, int nw, bool combine,
                         hipStream_t stream);
void arks_w8_dequant(void* out, const void* w8, const void* scales,
                     int n_total, int k_total, hipStream_t stream);
void arks_w8_moe_gemm(void* out, const void* a, const void* w8,
                      const void* scales, const void* counts,
                      const void* pairs, int n_experts, int t_cols,
                      int n_pairs, int src_div, int slabs, int n_total,
                      int k_total, int nw, hipStream_t stream);
void arks_mx4_skinny_gemm(void* part, void* out, const void* a, const void* w,
                          const void* scales, const void* bias, int m_rows,
                          int n_total, int k_total, int k_per_split,
                          int nsplits, int64_t a_stride, int nw, bool combine,
                          hipStream_t stream);
void arks_mx4_dequant(void* out, const void* w, const void* scales,
                      int n_total, int k_total, hipStream_t stream);
void arks_moe_route(void* counts, void* pairs, const void* ids, int n_pairs,
                    int T, int expert_base, int n_local, hipStream_t stream);
void arks_mfma_probe(void* d, const void* a, const void* b, hipStream_t stream);
void arks_mfma_probe32(void* d, const void* a, const void* b, hipStream_t stream);
void arks_tr16_probe(void* out, int stride_bytes, hipStream_t stream);
}

namespace {

hipStream_t current_stream() {
  return c10::hip::getCurrentHIPStream().stream();
}

// KV caches may be bf16 or fp8 e4m3 (kv_cache_dtype="fp8"); returns fp8?
bool check_kv_cache(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  if (t.scalar_type() == torch::kFloat8_e4m3fn) return true;
  TORCH_CHECK(t.scalar_type() == torch::kBFloat16, name, " must be bf16/fp8");
  return false;
}

void check_bf16_contig(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
  TORCH_CHECK(t.scalar_type() == torch::kBFloat16, name, " must be bf16");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

// bf16 tensor whose trailing dims are contiguous; dim-0 rows may be strided
// (a view into the fused QKV buffer).
void check_bf16_rowstrided(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
  TORCH_CHECK(t.scalar_type() == torch::kBFloat16, name, " must be bf16");
  TORCH_CHECK(t.stride(-1) == 1, name, " last dim must be contiguous");
  if (t.dim() == 3) {
    TORCH_CHECK(t.stride(1) == t.size(2), name, " inner dims must be dense");
  }
}

void rmsnorm(torch::Tensor out, torch::Tensor input, torch::Tensor weight,
             double eps) {
  check_bf16_contig(out, "out");
  check_bf16_contig(input, "input");
  check_bf16_contig(weight, "weight");
  const int hidden = input.size(-1);
  TORCH_CHECK(hidden % 8 == 0, "hidden must be a multiple of 8");
  const int rows = input.numel() / hidden;
  arks_rmsnorm(out.data_ptr(), input.data_ptr(), weight.data_ptr(), (float)eps,
               rows, hidden, current_stream());
}

void fused_add_rmsnorm(torch::Tensor out, torch::Tensor input,
                       torch::Tensor residual, torch::Tensor weight,
                       double eps) {
  check_bf16_contig(out, "out");
  check_bf16_contig(input, "input");
  check_bf16_contig(residual, "residual");
  const int hidden = input.size(-1);
  TORCH_CHECK(hidden % 8 == 0, "hidden must be a multiple of 8");
  const int rows = input.numel() / hidden;
  arks_fused_add_rmsnorm(out.data_ptr(), input.data_ptr(), residual.data_ptr(),
                         weight.data_ptr(), (float)eps, rows, hidden,
                         current_stream());
}

void silu_mul(torch::Tensor out, torch::Tensor gate_up) {
  check_bf16_contig(out, "out");
  check_bf16_contig(gate_up, "gate_up");
  const int d = out.size(-1);
  TORCH_CHECK(gate_up.size(-1) == 2 * d, "gate_up last dim must be 2*d");
  TORCH_CHECK(d % 8 == 0, "d must be a multiple of 8");
  const int64_t rows = out.numel() / d;
  arks_silu_mul(out.data_ptr(), gate_up.data_ptr(), rows, d, current_stream());
}

void rope_inplace(torch::Tensor positions, torch::Tensor q, torch::Tensor k,
                  torch::Tensor cos_sin, int64_t head_dim) {
  check_bf16_rowstrided(q, "q");
  check_bf16_rowstrided(k, "k");
  TORCH_CHECK(q.dim() == 2 && k.dim() == 2, "q/k must be 2-D [T, H*D]");
  TORCH_CHECK(positions.scalar_type() == torch::kInt64, "positions must be i64");
  TORCH_CHECK(cos_sin.scalar_type() == torch::kFloat32, "cos_sin must be f32");
  TORCH_CHECK(head_dim % 4 == 0, "head_dim must be a multiple of 4");
  const int num_tokens = q.size(0);
  const int num_q_heads = q.size(-1) / head_dim;
  const int num_kv_heads = k.size(-1) / head_dim;
  arks_rope_inplace(positions.data_ptr(), q.data_ptr(), k.data_ptr(),
                    cos_sin.data_ptr(), num_tokens, (int)head_dim, num_q_heads,
                    num_kv_heads, q.stride(0), k.stride(0), current_stream());
}

void reshape_and_cache(torch::Tensor k, torch::Tensor v, torch::Tensor k_cache,
                       torch::Tensor v_cache, torch::Tensor slot_mapping) {
  check_bf16_rowstrided(k, "k");
  check_bf16_rowstrided(v, "v");
  const bool kv_fp8 = check_kv_cache(k_cache, "k_cache");
  check_kv_cache(v_cache, "v_cache");
  TORCH_CHECK(slot_mapping.scalar_type() == torch::kInt64);
  TORCH_CHECK(k.stride(0) == v.stride(0), "k/v must share row stride");
  const int num_tokens = k.size(0);
  const int num_kv_heads = k_cache.size(1);
  const int block_size = k_cache.size(2);
  const int head_dim = k_cache.size(3);
  TORCH_CHECK(head_dim % 8 == 0);
  arks_reshape_and_cache(k.data_ptr(), v.data_ptr(), k_cache.data_ptr(),
                         v_cache.data_ptr(), slot_mapping.data_ptr(),
                         num_tokens, num_kv_heads, head_dim, block_size,
                         k.stride(0), kv_fp8 ? 1 : 0, current_stream());
}

void rope_and_cache(torch::Tensor positions, torch::Tensor q,
                    torch::Tensor k, torch::Tensor v, torch::Tensor k_cache,
                    torch::Tensor v_cache, torch::Tensor slot_mapping,
                    torch::Tensor cos_sin, int64_t head_dim) {
  TORCH_CHECK(positions.scalar_type() == torch::kInt64);
  TORCH_CHECK(slot_mapping.scalar_type() == torch::kInt64);
  TORCH_CHECK(cos_sin.scalar_type() == torch::kFloat32 &&
              cos_sin.is_contiguous());
  check_bf16_rowstrided(q, "q");
  check_bf16_rowstrided(k, "k");
  check_bf16_rowstrided(v, "v");
  const bool kv_fp8 = check_kv_cache(k_cache, "k_cache");
  check_kv_cache(v_cache, "v_cache");
  TORCH_CHECK(k.stride(0) == v.stride(0), "k/v must share row stride");
  const int T = q.size(0);
  const int nq = (int)(q.numel() / std::max<int64_t>(T, 1) / head_dim);
  const int nkv = (int)(k.numel() / std::max<int64_t>(T, 1) / head_dim);
  const int block_size = k_cache.size(2);
  arks_rope_and_cache(positions.data_ptr(), q.data_ptr(), k.data_ptr(),
                      v.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(),
                      slot_mapping.data_ptr(), cos_sin.data_ptr(), T,
                      (int)head_dim, nq, nkv, block_size, q.stride(0),
                      k.stride(0), kv_fp8 ? 1 : 0, current_stream());
}

void attention_decode_paged(torch::Tensor out, torch::Tensor q,
                            torch::Tensor k_cache, torch::Tensor v_cache,
                            torch::Tensor block_tables, torch::Tensor seq_lens,
                            double scale, torch::Tensor part_out,
                            int64_t nparts, int64_t window) {
  check_bf16_contig(out, "out");
  check_bf16_rowstrided(q, "q");
  const bool kv_fp8 = check_kv_cache(k_cache, "k_cache");
  check_kv_cache(v_cache, "v_cache");
  TORCH_CHECK(block_tables.scalar_type() == torch::kInt32);
  TORCH_CHECK(seq_lens.scalar_type() == torch::kInt32);
  const int num_seqs = q.size(0);
  const int num_q_heads = q.size(1);
  const int head_dim = q.size(2);
  const int num_kv_heads = k_cache.size(1);
  TORCH_CHECK(k_cache.size(2) == 16, "KV block size must be 16");
  TORCH_CHECK(head_dim == 64 || head_dim == 128, "head_dim must be 64 or 128");
  const int gq = num_q_heads / num_kv_heads;
  TORCH_CHECK(gq >= 1 && gq <= 8 && gq * num_kv_heads == num_q_heads,
              "q/kv head ratio must be integral and <= 8");
  const int max_blocks = block_tables.size(1);
  if (nparts > 1) {
    TORCH_CHECK(part_out.scalar_type() == torch::kFloat32 &&
                part_out.numel() >=
                    (int64_t)num_seqs * num_kv_heads * nparts * gq *
                        (head_dim + 2),
                "part_out workspace too small");
  }
  arks_attn_decode_paged(out.data_ptr(),
                         nparts > 1 ? part_out.data_ptr() : nullptr,
                         q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(),
                         block_tables.data_ptr(), seq_lens.data_ptr(),
                         (float)scale, num_seqs, num_q_heads, num_kv_heads,
                         head_dim, max_blocks, (int)nparts, q.stride(0),
                         kv_fp8 ? 1 : 0, (int)window, current_stream());
}

void attention_prefill_varlen(torch::Tensor out, torch::Tensor q,
                              torch::Tensor k, torch::Tensor v,
                              torch::Tensor cu_seqlens, torch::Tensor tile_info,
                              double scale, int64_t window) {
  check_bf16_contig(out, "out");
  check_bf16_rowstrided(q, "q");
  check_bf16_rowstrided(k, "k");
  check_bf16_rowstrided(v, "v");
  TORCH_CHECK(k.stride(0) == v.stride(0), "k/v must share row stride");
  TORCH_CHECK(cu_seqlens.scalar_type() == torch::kInt32);
  TORCH_CHECK(tile_info.scalar_type() == torch::kInt32);
  TORCH_CHECK(tile_info.dim() == 2 && tile_info.size(1) == 2);
  const int num_q_heads = q.size(1);
  const int head_dim = q.size(2);
  const int num_kv_heads = k.size(1);
  TORCH_CHECK(head_dim == 64 || head_dim == 128, "head_dim must be 64 or 128");
  const int ntiles = tile_info.size(0);
  arks_attn_prefill_varlen(out.data_ptr(), q.data_ptr(), k.data_ptr(),
                           v.data_ptr(), cu_seqlens.data_ptr(),
                           tile_info.data_ptr(), ntiles, (float)scale,
                           num_q_heads, num_kv_heads, head_dim, q.stride(0),
                           k.stride(0), (int)window, current_stream());
}

void attention_extend_paged(torch::Tensor out, torch::Tensor q,
                            torch::Tensor k_cache, torch::Tensor v_cache,
                            torch::Tensor block_tables, torch::Tensor kv_lens,
                            torch::Tensor cu_seqlens_q, torch::Tensor tile_info,
                            double scale, int64_t window) {
  check_bf16_contig(out, "out");
  check_bf16_rowstrided(q, "q");
  const bool kv_fp8 = check_kv_cache(k_cache, "k_cache");
  check_kv_cache(v_cache, "v_cache");
  TORCH_CHECK(block_tables.scalar_type() == torch::kInt32);
  TORCH_CHECK(kv_lens.scalar_type() == torch::kInt32);
  TORCH_CHECK(cu_seqlens_q.scalar_type() == torch::kInt32);
  TORCH_CHECK(tile_info.scalar_type() == torch::kInt32);
  TORCH_CHECK(tile_info.dim() == 2 && tile_info.size(1) == 2);
  const int num_q_heads = q.size(1);
  const int head_dim = q.size(2);
  const int num_kv_heads = k_cache.size(1);
  TORCH_CHECK(k_cache.size(2) == 16, "KV block size must be 16");
  TORCH_CHECK(head_dim == 64 || head_dim == 128, "head_dim must be 64 or 128");
  const int ntiles = tile_info.size(0);
  const int max_blocks = block_tables.size(1);
  arks_attn_extend_paged(out.data_ptr(), q.data_ptr(), k_cache.data_ptr(),
                         v_cache.data_ptr(), block_tables.data_ptr(),
                         kv_lens.data_ptr(), cu_seqlens_q.data_ptr(),
                         tile_info.data_ptr(), ntiles, (float)scale,
                         num_q_heads, num_kv_heads, head_dim, max_blocks,
                         q.stride(0), kv_fp8 ? 1 : 0, (int)window,
                         current_stream());
}

// 8-wave 32x32-MFMA ladder (attn_extend2.hip): 256-row q tiles, bf16 KV.
void attention_extend_paged2(torch::Tensor out, torch::Tensor q,
                             torch::Tensor k_cache, torch::Tensor v_cache,
                             torch::Tensor block_tables, torch::Tensor kv_lens,
                             torch::Tensor cu_seqlens_q,
                             torch::Tensor tile_info, torch::Tensor part_ws,
                             double scale, int64_t window) {
  check_bf16_contig(out, "out");
  check_bf16_rowstrided(q, "q");
  check_bf16_contig(k_cache, "k_cache");
  check_bf16_contig(v_cache, "v_cache");
  TORCH_CHECK(block_tables.scalar_type() == torch::kInt32);
  TORCH_CHECK(kv_lens.scalar_type() == torch::kInt32);
  TORCH_CHECK(cu_seqlens_q.scalar_type() == torch::kInt32);
  TORCH_CHECK(tile_info.scalar_type() == torch::kInt32);
  TORCH_CHECK(tile_info.dim() == 2 && tile_info.size(1) == 4,
              "tile_info rows are (seq, q0, part, nparts)");
  const int num_q_heads = q.size(1);
  const int head_dim = q.size(2);
  const int num_kv_heads = k_cache.size(1);
  TORCH_CHECK(k_cache.size(2) == 16, "KV block size must be 16");
  TORCH_CHECK(head_dim == 64 || head_dim == 128, "head_dim must be 64 or 128");
  const int ntiles = tile_info.size(0);
  const int max_blocks = block_tables.size(1);
  void* ws = nullptr;
  if (part_ws.numel() > 0) {
    // sized by the host: split rows sort first, so only their slabs exist
    TORCH_CHECK(part_ws.scalar_type() == torch::kFloat32);
    ws = part_ws.data_ptr();
  }
  arks_attn_extend_paged2(out.data_ptr(), q.data_ptr(), k_cache.data_ptr(),
                          v_cache.data_ptr(), block_tables.data_ptr(),
                          kv_lens.data_ptr(), cu_seqlens_q.data_ptr(),
                          tile_info.data_ptr(), ws, ntiles, (float)scale,
                          num_q_heads, num_kv_heads, head_dim, max_blocks,
                          q.stride(0), (int)window, current_stream());
}

void attention_extend2_combine(torch::Tensor out, torch::Tensor part_ws,
                               torch::Tensor combine_table,
                               torch::Tensor cu_seqlens_q, double scale) {
  check_bf16_rowstrided(out, "out");
  TORCH_CHECK(part_ws.scalar_type() == torch::kFloat32);
  TORCH_CHECK(combine_table.scalar_type() == torch::kInt32 &&
              combine_table.dim() == 2 && combine_table.size(1) == 4);
  const int num_q_heads = out.size(1);
  const int head_dim = out.size(2);
  arks_attn_extend2_combine(out.data_ptr(), part_ws.data_ptr(),
                            combine_table.data_ptr(), cu_seqlens_q.data_ptr(),
                            combine_table.size(0), (float)scale, num_q_heads,
                            head_dim, current_stream());
}

// Shared argument checks of the skinny GEMM entries; returns the bias
// pointer (or null). out is ignored for a partials-only launch.
const void* check_skinny_args(const torch::Tensor& out,
                              const torch::Tensor& part,
                              const torch::Tensor& a, const torch::Tensor& w,
                              const c10::optional<torch::Tensor>& bias,
                              int64_t k, int64_t nsplits, int64_t mrows,
                              int64_t n_mult, bool partials_only,
                              const char* what) {
  check_bf16_rowstrided(a, "a");
  check_bf16_contig(w, "w");
  const int64_t m = a.size(0), n = w.size(0);
  TORCH_CHECK(m >= 1 && m <= 64, what, " needs 1 <= M <= 64");
  TORCH_CHECK(n % n_mult == 0 && k % 32 == 0, "N%", n_mult,
              "==0 and K%32==0 required");
  if (partials_only) {
    TORCH_CHECK(nsplits > 1, what, ": partials-only needs nsplits > 1");
  } else {
    check_bf16_contig(out, "out");
    TORCH_CHECK(out.size(0) == m && out.size(1) == n);
  }
  const void* bias_ptr = nullptr;
  if (bias.has_value()) {
    check_bf16_contig(*bias, "bias");
    TORCH_CHECK(bias->numel() == n);
    bias_ptr = bias->data_ptr();
  }
  if (nsplits > 1) {
    TORCH_CHECK(part.is_cuda() && part.scalar_type() == torch::kFloat32 &&
                part.is_contiguous() &&
                part.numel() >= (int64_t)nsplits * n * mrows,
                what, " workspace too small");
  }
  return bias_ptr;
}

// config selects the kernel (skinny_gemm.hip): 0 = default ring with MT from
// M, 1 = tall-K, 2 = tall-K with non-temporal W loads, 3 = A-resident (split-K
// with a K-range that fits in LDS; groups = workgroups per split, 0 = auto),
// 4 = tall-K on 112-row tiles. The tall-K configs (1, 2, 4) take any N that
// is a multiple of 16 (a tile may hang over N by whole waves); 0 and 3 need
// a multiple of 64.
void skinny_gemm_impl(torch::Tensor out, torch::Tensor part, torch::Tensor a,
                      torch::Tensor w, c10::optional<torch::Tensor> bias,
                      int64_t k_per_split, int64_t nsplits, int64_t config,
                      int64_t groups, bool combine) {
  const int m = a.size(0), k = a.size(1), n = w.size(0);
  TORCH_CHECK(w.size(1) == k);
  TORCH_CHECK(0 <= config && config <= 4, "config in 0..4");
  TORCH_CHECK(k_per_split >= 32 && k_per_split % 32 == 0 &&
              nsplits * k_per_split >= k, "splits must cover K");
  TORCH_CHECK(config != 3 ||
                  (nsplits > 1 && k_per_split <= arks_skinny_resident_kmax()),
              "config 3 needs nsplits > 1 and k_per_split <= ",
              arks_skinny_resident_kmax());
  TORCH_CHECK(0 <= groups && groups <= 65535, "groups in 0..65535");
  TORCH_CHECK(nsplits <= 65535, "too many splits");
  const int mrows = arks_skinny_slab_rows(m, (int)config);
  const void* bias_ptr =
      check_skinny_args(out, part, a, w, bias, k, nsplits, mrows,
                        config == 0 || config == 3 ? 64 : 16, !combine,
                        "skinny_gemm");
  arks_skinny_gemm(nsplits > 1 ? part.data_ptr() : nullptr,
                   combine ? out.data_ptr() : nullptr, a.data_ptr(),
                   w.data_ptr(), bias_ptr, m, n, k, (int)k_per_split,
                   (int)nsplits, a.stride(0), (int)config, combine,
                   current_stream(), (int)groups);
}

void skinny_gemm(torch::Tensor out, torch::Tensor part, torch::Tensor a,
                 torch::Tensor w, c10::optional<torch::Tensor> bias,
                 int64_t k_per_split, int64_t nsplits, int64_t config,
                 int64_t groups) {
  skinny_gemm_impl(out, part, a, w, bias, k_per_split, nsplits, config, groups,
                   true);
}

// Partials-only launch (nsplits > 1): leaves the f32 split-K partials
// [nsplits, slab rows, N] in `part` (slab rows = 16 * MT of the kernel that
// config launches) for a consumer that reduces them (splitk_add_rmsnorm /
// splitk_rope_and_cache / skinny_combine). The bias is applied by that
// consumer, not here.
void skinny_gemm_partials(torch::Tensor part, torch::Tensor a, torch::Tensor w,
                          int64_t k_per_split, int64_t nsplits,
                          int64_t config, int64_t groups) {
  skinny_gemm_impl(torch::Tensor(), part, a, w, c10::nullopt, k_per_split,
                   nsplits, config, groups, false);
}

// Packed W4 weight (w4_gemm.hip): qweight i32 [N, K/8], scales f16 [K/128, N],
// zeros u8 [K/128, N]. Returns (n, k).
std::pair<int64_t, int64_t> check_w4_packed(const torch::Tensor& qw,
                                            const torch::Tensor& scales,
                                            const torch::Tensor& zeros) {
  TORCH_CHECK(qw.is_cuda() && qw.scalar_type() == torch::kInt32 &&
              qw.dim() == 2 && qw.is_contiguous(),
              "qweight must be contiguous int32 [N, K/8] on GPU");
  const int64_t n = qw.size(0), k = qw.size(1) * 8;
  TORCH_CHECK(k >= 128 && k % 128 == 0, "W4 needs K % 128 == 0, got K=", k);
  TORCH_CHECK(n % 64 == 0, "W4 needs N % 64 == 0, got N=", n);
  TORCH_CHECK(scales.is_cuda() && scales.scalar_type() == torch::kFloat16 &&
              scales.is_contiguous() && scales.dim() == 2 &&
              scales.size(0) == k / 128 && scales.size(1) == n,
              "scales must be contiguous f16 [K/128, N] on GPU");
  TORCH_CHECK(zeros.is_cuda() && zeros.scalar_type() == torch::kUInt8 &&
              zeros.is_contiguous() && zeros.dim() == 2 &&
              zeros.size(0) == k / 128 && zeros.size(1) == n,
              "zeros must be contiguous uint8 [K/128, N] on GPU");
  TORCH_CHECK(scales.device() == qw.device() && zeros.device() == qw.device());
  return {n, k};
}

// Everything a dense quantized skinny GEMM (w4_/w8_skinny_gemm[_partials])
// checks that does not depend on the weight format, for a weight [n, k] on
// `dev`. nw = 64-row N sub-tiles per workgroup (1 or 2); combine = false
// leaves the split-K partials in `part` (bias is then applied by the
// consumer). Returns the pointers the launch takes: part, out and bias, each
// null where the kernel must not touch it.
struct WqSkinnyArgs {
  void* part;
  void* out;
  const void* bias;
};
WqSkinnyArgs check_wq_skinny(const torch::Tensor& out,
                             const torch::Tensor& part,
                             const torch::Tensor& a,
                             const c10::optional<torch::Tensor>& bias,
                             int64_t n, int64_t k, c10::Device dev,
                             int64_t k_per_split, int64_t nsplits, int64_t nw,
                             bool combine) {
  check_bf16_rowstrided(a, "a");
  TORCH_CHECK(a.dim() == 2 && a.size(1) == k, "a must be [M, K]");
  TORCH_CHECK(a.device() == dev);
  const int64_t m = a.size(0);
  TORCH_CHECK(m >= 1 && m <= 64, "wq_skinny_gemm needs 1 <= M <= 64");
  TORCH_CHECK(a.stride(0) % 8 == 0 &&
              reinterpret_cast<uintptr_t>(a.data_ptr()) % 16 == 0,
              "a rows must be 16-byte aligned");
  TORCH_CHECK((nw == 1 || nw == 2) && n % (64 * nw) == 0,
              "nw in {1, 2} with N % (64 * nw) == 0");
  TORCH_CHECK(nsplits >= 1 && k_per_split >= 128 && k_per_split % 128 == 0 &&
              nsplits * k_per_split >= k && (nsplits - 1) * k_per_split < k,
              "splits of a multiple of 128 must cover K exactly");
  WqSkinnyArgs r{nullptr, nullptr, nullptr};
  if (combine) {
    check_bf16_contig(out, "out");
    TORCH_CHECK(out.dim() == 2 && out.size(0) == m && out.size(1) == n);
    r.out = out.data_ptr();
    if (bias.has_value()) {
      check_bf16_contig(*bias, "bias");
      TORCH_CHECK(bias->numel() == n);
      r.bias = bias->data_ptr();
    }
  } else {
    TORCH_CHECK(nsplits > 1, "partials-only needs nsplits > 1");
  }
  if (nsplits > 1) {
    TORCH_CHECK(part.is_cuda() && part.scalar_type() == torch::kFloat32 &&
                part.is_contiguous() &&
                part.numel() >= nsplits * n * arks_wq_slab_rows((int)m) &&
                reinterpret_cast<uintptr_t>(part.data_ptr()) % 16 == 0,
                "wq_skinny_gemm workspace too small");
    r.part = part.data_ptr();
  }
  return r;
}

void w4_skinny_gemm_impl(torch::Tensor out, torch::Tensor part,
                         torch::Tensor a, torch::Tensor qw,
                         torch::Tensor scales, torch::Tensor zeros,
                         c10::optional<torch::Tensor> bias,
                         int64_t k_per_split, int64_t nsplits, int64_t nw,
                         bool combine) {
  const auto [n, k] = check_w4_packed(qw, scales, zeros);
  const auto p = check_wq_skinny(out, part, a, bias, n, k, qw.device(),
                                 k_per_split, nsplits, nw, combine);
  arks_w4_skinny_gemm(p.part, p.out, a.data_ptr(), qw.data_ptr(),
                      scales.data_ptr(), zeros.data_ptr(), p.bias,
                      (int)a.size(0), (int)n, (int)k, (int)k_per_split,
                      (int)nsplits, a.stride(0), (int)nw, combine,
                      current_stream());
}

void w4_skinny_gemm(torch::Tensor out, torch::Tensor part, torch::Tensor a,
                    torch::Tensor qw, torch::Tensor scales,
                    torch::Tensor zeros, c10::optional<torch::Tensor> bias,
                    int64_t k_per_split, int64_t nsplits, int64_t nw) {
  w4_skinny_gemm_impl(out, part, a, qw, scales, zeros, bias, k_per_split,
                      nsplits, nw, true);
}

void w4_skinny_gemm_partials(torch::Tensor part, torch::Tensor a,
                             torch::Tensor qw, torch::Tensor scales,
                             torch::Tensor zeros, int64_t k_per_split,
                             int64_t nsplits, int64_t nw) {
  w4_skinny_gemm_impl(torch::Tensor(), part, a, qw, scales, zeros,
                      c10::nullopt, k_per_split, nsplits, nw, false);
}

// out bf16 [>= N*K elements] receives the dequantized [N, K] weight.
void w4_dequant(torch::Tensor out, torch::Tensor qw, torch::Tensor scales,
                torch::Tensor zeros) {
  const auto [n, k] = check_w4_packed(qw, scales, zeros);
  check_bf16_contig(out, "out");
  TORCH_CHECK(out.numel() >= n * k && out.device() == qw.device() &&
              reinterpret_cast<uintptr_t>(out.data_ptr()) % 16 == 0,
              "w4_dequant output too small");
  TORCH_CHECK(n * (k / 8) < (int64_t)1 << 39);
  arks_w4_dequant(out.data_ptr(), qw.data_ptr(), scales.data_ptr(),
                  zeros.data_ptr(), (int)n, (int)k, current_stream());
}

// W8 weight (w8_gemm.hip): e4m3fn [N, K] as in the checkpoint, scales f32
// [K/128, N] (block scales expanded per output row). Returns (n, k).
std::pair<int64_t, int64_t> check_w8_weight(const torch::Tensor& w8,
                                            const torch::Tensor& scales) {
  TORCH_CHECK(w8.is_cuda() && w8.scalar_type() == at::kFloat8_e4m3fn &&
              w8.dim() == 2 && w8.is_contiguous() &&
              reinterpret_cast<uintptr_t>(w8.data_ptr()) % 16 == 0,
              "w8 weight must be contiguous float8_e4m3fn [N, K] on GPU");
  const int64_t n = w8.size(0), k = w8.size(1);
  TORCH_CHECK(k >= 128 && k % 128 == 0, "W8 needs K % 128 == 0, got K=", k);
  TORCH_CHECK(n % 64 == 0, "W8 needs N % 64 == 0, got N=", n);
  TORCH_CHECK(scales.is_cuda() && scales.scalar_type() == torch::kFloat32 &&
              scales.is_contiguous() && scales.dim() == 2 &&
              scales.size(0) == k / 128 && scales.size(1) == n &&
              reinterpret_cast<uintptr_t>(scales.data_ptr()) % 16 == 0,
              "scales must be contiguous f32 [K/128, N] on GPU");
  TORCH_CHECK(scales.device() == w8.device());
  return {n, k};
}

void w8_skinny_gemm_impl(torch::Tensor out, torch::Tensor part,
                         torch::Tensor a, torch::Tensor w8,
                         torch::Tensor scales,
                         c10::optional<torch::Tensor> bias,
                         int64_t k_per_split, int64_t nsplits, int64_t nw,
                         bool combine) {
  const auto [n, k] = check_w8_weight(w8, scales);
  const auto p = check_wq_skinny(out, part, a, bias, n, k, w8.device(),
                                 k_per_split, nsplits, nw, combine);
  arks_w8_skinny_gemm(p.part, p.out, a.data_ptr(), w8.data_ptr(),
                      scales.data_ptr(), p.bias, (int)a.size(0), (int)n,
                      (int)k, (int)k_per_split, (int)nsplits, a.stride(0),
                      (int)nw, combine, current_stream());
}

void w8_skinny_gemm(torch::Tensor out, torch::Tensor part, torch::Tensor a,
                    torch::Tensor w8, torch::Tensor scales,
                    c10::optional<torch::Tensor> bias, int64_t k_per_split,
                    int64_t nsplits, int64_t nw) {
  w8_skinny_gemm_impl(out, part, a, w8, scales, bias, k_per_split, nsplits,
                      nw, true);
}

void w8_skinny_gemm_partials(torch::Tensor part, torch::Tensor a,
                             torch::Tensor w8, torch::Tensor scales,
                             int64_t k_per_split, int64_t nsplits,
                             int64_t nw) {
  w8_skinny_gemm_impl(torch::Tensor(), part, a, w8, scales, c10::nullopt,
                      k_per_split, nsplits, nw, false);
}

// out bf16 [>= N*K elements] receives the dequantized [N, K] weight.
void w8_dequant(torch::Tensor out, torch::Tensor w8, torch::Tensor scales) {
  const auto [n, k] = check_w8_weight(w8, scales);
  check_bf16_contig(out, "out");
  TORCH_CHECK(out.numel() >= n * k && out.device() == w8.device() &&
              reinterpret_cast<uintptr_t>(out.data_ptr()) % 16 == 0,
              "w8_dequant output too small");
  TORCH_CHECK(n * (k / 16) < (int64_t)1 << 39);
  arks_w8_dequant(out.data_ptr(), w8.data_ptr(), scales.data_ptr(), (int)n,
                  (int)k, current_stream());
}

// MX4 weight (mx4_gemm.hip): the checkpoint's tensors, u8 [N, K/2] with two
// e2m1 nibbles per byte and u8 [N, K/32] e8m0 scales. Returns (n, k).
std::pair<int64_t, int64_t> check_mx4_weight(const torch::Tensor& w,
                                             const torch::Tensor& scales) {
  TORCH_CHECK(w.is_cuda() && w.scalar_type() == torch::kUInt8 &&
              w.dim() == 2 && w.is_contiguous() &&
              reinterpret_cast<uintptr_t>(w.data_ptr()) % 16 == 0,
              "mx4 weight must be contiguous uint8 [N, K/2] on GPU");
  const int64_t n = w.size(0), k = w.size(1) * 2;
  TORCH_CHECK(k >= 128 && k % 128 == 0, "MX4 needs K % 128 == 0, got K=", k);
  TORCH_CHECK(n % 64 == 0, "MX4 needs N % 64 == 0, got N=", n);
  TORCH_CHECK(scales.is_cuda() && scales.scalar_type() == torch::kUInt8 &&
              scales.is_contiguous() && scales.dim() == 2 &&
              scales.size(0) == n && scales.size(1) == k / 32 &&
              reinterpret_cast<uintptr_t>(scales.data_ptr()) % 4 == 0,
              "scales must be contiguous uint8 [N, K/32] on GPU");
  TORCH_CHECK(scales.device() == w.device());
  return {n, k};
}

void mx4_skinny_gemm_impl(torch::Tensor out, torch::Tensor part,
                          torch::Tensor a, torch::Tensor w,
                          torch::Tensor scales,
                          c10::optional<torch::Tensor> bias,
                          int64_t k_per_split, int64_t nsplits, int64_t nw,
                          bool combine) {
  const auto [n, k] = check_mx4_weight(w, scales);
  const auto p = check_wq_skinny(out, part, a, bias, n, k, w.device(),
                                 k_per_split, nsplits, nw, combine);
  arks_mx4_skinny_gemm(p.part, p.out, a.data_ptr(), w.data_ptr(),
                       scales.data_ptr(), p.bias, (int)a.size(0), (int)n,
                       (int)k, (int)k_per_split, (int)nsplits, a.stride(0),
                       (int)nw, combine, current_stream());
}

void mx4_skinny_gemm(torch::Tensor out, torch::Tensor part, torch::Tensor a,
                     torch::Tensor w, torch::Tensor scales,
                     c10::optional<torch::Tensor> bias, int64_t k_per_split,
                     int64_t nsplits, int64_t nw) {
  mx4_skinny_gemm_impl(out, part, a, w, scales, bias, k_per_split, nsplits,
                       nw, true);
}

void mx4_skinny_gemm_partials(torch::Tensor part, torch::Tensor a,
                              torch::Tensor w, torch::Tensor scales,
                              int64_t k_per_split, int64_t nsplits,
                              int64_t nw) {
  mx4_skinny_gemm_impl(torch::Tensor(), part, a, w, scales, c10::nullopt,
                       k_per_split, nsplits, nw, false);
}

// out bf16 [>= N*K elements] receives the dequantized [N, K] weight.
void mx4_dequant(torch::Tensor out, torch::Tensor w, torch::Tensor scales) {
  const auto [n, k] = check_mx4_weight(w, scales);
  check_bf16_contig(out, "out");
  TORCH_CHECK(out.numel() >= n * k && out.device() == w.device() &&
              reinterpret_cast<uintptr_t>(out.data_ptr()) % 16 == 0,
              "mx4_dequant output too small");
  TORCH_CHECK(n * (k / 32) < (int64_t)1 << 39);
  arks_mx4_dequant(out.data_ptr(), w.data_ptr(), scales.data_ptr(), (int)n,
                   (int)k, current_stream());
}

// Routed grouped GEMM over stacked experts (w4_moe_gemm_kernel):
//   out[p] = a[p / src_div] @ dequant(W[e])^T for p in pairs[e][:counts[e]].
// qweight i32 [E, N, K/8], scales f16 [E, K/128, N], zeros u8 [E, K/128, N],
// counts i32 [E], pairs i32 [E, T], out bf16 [n_pairs, N]. Everything the
// kernel indexes by is checked here; the table's contents are clamped to
// these extents in the kernel.
void w4_moe_gemm(torch::Tensor out, torch::Tensor a, torch::Tensor qw,
                 torch::Tensor scales, torch::Tensor zeros,
                 torch::Tensor counts, torch::Tensor pairs, int64_t top_k,
                 int64_t src_div, int64_t max_rows) {
  TORCH_CHECK(qw.is_cuda() && qw.scalar_type() == torch::kInt32 &&
              qw.dim() == 3 && qw.is_contiguous(),
              "qweight must be contiguous int32 [E, N, K/8] on GPU");
  const int64_t ne = qw.size(0), n = qw.size(1), k = qw.size(2) * 8;
  TORCH_CHECK(ne >= 1 && ne <= 65535, "need 1 <= E_local <= 65535");
  TORCH_CHECK(k >= 128 && k % 128 == 0, "W4 needs K % 128 == 0, got K=", k);
  TORCH_CHECK(n >= 64 && n % 64 == 0, "W4 needs N % 64 == 0, got N=", n);
  TORCH_CHECK(n * (k / 8) < ((int64_t)1 << 31), "expert weight too large");
  TORCH_CHECK(scales.is_cuda() && scales.scalar_type() == torch::kFloat16 &&
              scales.is_contiguous() && scales.dim() == 3 &&
              scales.size(0) == ne && scales.size(1) == k / 128 &&
              scales.size(2) == n,
              "scales must be contiguous f16 [E, K/128, N] on GPU");
  TORCH_CHECK(zeros.is_cuda() && zeros.scalar_type() == torch::kUInt8 &&
              zeros.is_contiguous() && zeros.dim() == 3 &&
              zeros.size(0) == ne && zeros.size(1) == k / 128 &&
              zeros.size(2) == n,
              "zeros must be contiguous uint8 [E, K/128, N] on GPU");
  check_bf16_contig(a, "a");
  check_bf16_contig(out, "out");
  TORCH_CHECK(a.dim() == 2 && a.size(1) == k, "a must be [rows, K]");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(a.data_ptr()) % 16 == 0,
              "a rows must be 16-byte aligned");
  TORCH_CHECK(counts.is_cuda() && counts.scalar_type() == torch::kInt32 &&
              counts.is_contiguous() && counts.dim() == 1 &&
              counts.size(0) == ne, "counts must be int32 [E_local] on GPU");
  TORCH_CHECK(pairs.is_cuda() && pairs.scalar_type() == torch::kInt32 &&
              pairs.is_contiguous() && pairs.dim() == 2 &&
              pairs.size(0) == ne && pairs.size(1) >= 1,
              "pairs must be int32 [E_local, T] on GPU, got ", pairs.sizes());
  const int64_t t_cols = pairs.size(1);
  TORCH_CHECK(top_k >= 1, "top_k must be >= 1");
  const int64_t n_pairs = t_cols * top_k;
  TORCH_CHECK(out.dim() == 2 && out.size(1) == n && out.size(0) == n_pairs,
              "out must be [T*k, N] = [", n_pairs, ", ", n, "], got ",
              out.sizes());
  TORCH_CHECK(n_pairs < ((int64_t)1 << 31) / 2);
  TORCH_CHECK(src_div >= 1 && a.size(0) * src_div >= n_pairs,
              "a has ", a.size(0), " rows, too few for ", n_pairs,
              " pairs at src_div=", src_div);
  TORCH_CHECK(max_rows >= 1 && max_rows <= t_cols,
              "need 1 <= max_rows <= T, got ", max_rows);
  const auto dev = qw.device();
  TORCH_CHECK(scales.device() == dev && zeros.device() == dev &&
              a.device() == dev && out.device() == dev &&
              counts.device() == dev && pairs.device() == dev);
  const int64_t slabs = (max_rows + 63) / 64;
  TORCH_CHECK(slabs <= 65535, "max_rows too large");
  // NW = 2 halves the activation re-read per tile and pays above 32 rows
  // (ops._wq_plan); a slab of an expert's list rarely holds that many
  // unless the batch does.
  const int nw = (max_rows > 32 && n % 128 == 0) ? 2 : 1;
  arks_w4_moe_gemm(out.data_ptr(), a.data_ptr(), qw.data_ptr(),
                   scales.data_ptr(), zeros.data_ptr(), counts.data_ptr(),
                   pairs.data_ptr(), (int)ne, (int)t_cols, (int)n_pairs,
                   (int)src_div, (int)slabs, (int)n, (int)k, nw,
                   current_stream());
}

// The same over stacked W8 experts (w8_moe_gemm_kernel): w8 e4m3fn [E, N, K]
// (the checkpoint's bytes), scales f32 [E, K/128, N].
void w8_moe_gemm(torch::Tensor out, torch::Tensor a, torch::Tensor w8,
                 torch::Tensor scales, torch::Tensor counts,
                 torch::Tensor pairs, int64_t top_k, int64_t src_div,
                 int64_t max_rows) {
  TORCH_CHECK(w8.is_cuda() && w8.scalar_type() == at::kFloat8_e4m3fn &&
              w8.dim() == 3 && w8.is_contiguous() &&
              reinterpret_cast<uintptr_t>(w8.data_ptr()) % 16 == 0,
              "w8 weight must be contiguous float8_e4m3fn [E, N, K] on GPU");
  const int64_t ne = w8.size(0), n = w8.size(1), k = w8.size(2);
  TORCH_CHECK(ne >= 1 && ne <= 65535, "need 1 <= E_local <= 65535");
  TORCH_CHECK(k >= 128 && k % 128 == 0, "W8 needs K % 128 == 0, got K=", k);
  TORCH_CHECK(n >= 64 && n % 64 == 0, "W8 needs N % 64 == 0, got N=", n);
  TORCH_CHECK(n * k < ((int64_t)1 << 31), "expert weight too large");
  TORCH_CHECK(scales.is_cuda() && scales.scalar_type() == torch::kFloat32 &&
              scales.is_contiguous() && scales.dim() == 3 &&
              scales.size(0) == ne && scales.size(1) == k / 128 &&
              scales.size(2) == n &&
              reinterpret_cast<uintptr_t>(scales.data_ptr()) % 16 == 0,
              "scales must be contiguous f32 [E, K/128, N] on GPU");
  check_bf16_contig(a, "a");
  check_bf16_contig(out, "out");
  TORCH_CHECK(a.dim() == 2 && a.size(1) == k, "a must be [rows, K]");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(a.data_ptr()) % 16 == 0,
              "a rows must be 16-byte aligned");
  TORCH_CHECK(counts.is_cuda() && counts.scalar_type() == torch::kInt32 &&
              counts.is_contiguous() && counts.dim() == 1 &&
              counts.size(0) == ne, "counts must be int32 [E_local] on GPU");
  TORCH_CHECK(pairs.is_cuda() && pairs.scalar_type() == torch::kInt32 &&
              pairs.is_contiguous() && pairs.dim() == 2 &&
              pairs.size(0) == ne && pairs.size(1) >= 1,
              "pairs must be int32 [E_local, T] on GPU, got ", pairs.sizes());
  const int64_t t_cols = pairs.size(1);
  TORCH_CHECK(top_k >= 1, "top_k must be >= 1");
  const int64_t n_pairs = t_cols * top_k;
  TORCH_CHECK(out.dim() == 2 && out.size(1) == n && out.size(0) == n_pairs,
              "out must be [T*k, N] = [", n_pairs, ", ", n, "], got ",
              out.sizes());
  TORCH_CHECK(n_pairs < ((int64_t)1 << 31) / 2);
  TORCH_CHECK(src_div >= 1 && a.size(0) * src_div >= n_pairs,
              "a has ", a.size(0), " rows, too few for ", n_pairs,
              " pairs at src_div=", src_div);
  TORCH_CHECK(max_rows >= 1 && max_rows <= t_cols,
              "need 1 <= max_rows <= T, got ", max_rows);
  const auto dev = w8.device();
  TORCH_CHECK(scales.device() == dev && a.device() == dev &&
              out.device() == dev && counts.device() == dev &&
              pairs.device() == dev);
  const int64_t slabs = (max_rows + 63) / 64;
  TORCH_CHECK(slabs <= 65535, "max_rows too large");
  const int nw = (max_rows > 32 && n % 128 == 0) ? 2 : 1;  // as w4_moe_gemm
  arks_w8_moe_gemm(out.data_ptr(), a.data_ptr(), w8.data_ptr(),
                   scales.data_ptr(), counts.data_ptr(), pairs.data_ptr(),
                   (int)ne, (int)t_cols, (int)n_pairs, (int)src_div,
                   (int)slabs, (int)n, (int)k, nw, current_stream());
}

// Checks shared by the consumers of split-K partials [nsplits, mrows, n].
const void* check_partials(const torch::Tensor& part,
                           const c10::optional<torch::Tensor>& bias,
                           int64_t nsplits, int64_t mrows, int64_t rows,
                           int64_t n) {
  TORCH_CHECK(part.is_cuda() && part.scalar_type() == torch::kFloat32 &&
              part.is_contiguous(), "part must be contiguous f32 on GPU");
  TORCH_CHECK(nsplits >= 1 && mrows >= rows && rows >= 0 && n % 8 == 0);
  TORCH_CHECK(part.numel() >= nsplits * mrows * n, "partials too small");
  if (!bias.has_value()) return nullptr;
  check_bf16_contig(*bias, "bias");
  TORCH_CHECK(bias->numel() == n);
  return bias->data_ptr();
}

void skinny_combine(torch::Tensor out, torch::Tensor part,
                    c10::optional<torch::Tensor> bias, int64_t nsplits,
                    int64_t mrows) {
  check_bf16_contig(out, "out");
  TORCH_CHECK(out.dim() == 2);
  const int m = out.size(0), n = out.size(1);
  const void* bias_ptr = check_partials(part, bias, nsplits, mrows, m, n);
  if (m == 0) return;
  arks_skinny_combine(out.data_ptr(), part.data_ptr(), bias_ptr, m, n,
                      (int)nsplits, (int)mrows, current_stream());
}

// fused_add_rmsnorm whose input is the split-K partials of the producing
// skinny GEMM instead of its combined bf16 output.
void splitk_add_rmsnorm(torch::Tensor out, torch::Tensor part,
                        c10::optional<torch::Tensor> bias,
                        torch::Tensor residual, torch::Tensor weight,
                        double eps, int64_t nsplits, int64_t mrows) {
  check_bf16_contig(out, "out");
  check_bf16_contig(residual, "residual");
  check_bf16_contig(weight, "weight");
  TORCH_CHECK(out.dim() == 2 && residual.dim() == 2);
  const int rows = out.size(0), hidden = out.size(1);
  TORCH_CHECK(residual.size(0) == rows && residual.size(1) == hidden &&
              weight.numel() == hidden);
  const void* bias_ptr = check_partials(part, bias, nsplits, mrows, rows,
                                        hidden);
  if (rows == 0) return;
  arks_splitk_add_rmsnorm(out.data_ptr(), part.data_ptr(), bias_ptr,
                          residual.data_ptr(), weight.data_ptr(), (float)eps,
                          rows, hidden, (int)nsplits, (int)mrows,
                          current_stream());
}

// rope_and_cache whose q/k/v input is the split-K partials of the fused qkv
// skinny GEMM. Writes rotated q to q_out [T, Hq*D]; k/v only to the cache.
// groups = workgroups per token (1 = the whole token in one workgroup).
void splitk_rope_and_cache(torch::Tensor positions, torch::Tensor part,
                           c10::optional<torch::Tensor> bias,
                           torch::Tensor q_out, torch::Tensor k_cache,
                           torch::Tensor v_cache, torch::Tensor slot_mapping,
                           torch::Tensor cos_sin, int64_t head_dim,
                           int64_t nsplits, int64_t mrows, int64_t groups) {
  TORCH_CHECK(1 <= groups && groups <= 65535, "groups in 1..65535");
  TORCH_CHECK(positions.scalar_type() == torch::kInt64 &&
              positions.is_contiguous());
  TORCH_CHECK(slot_mapping.scalar_type() == torch::kInt64 &&
              slot_mapping.is_contiguous());
  TORCH_CHECK(cos_sin.scalar_type() == torch::kFloat32 &&
              cos_sin.is_contiguous() && cos_sin.size(-1) == head_dim);
  check_bf16_contig(q_out, "q_out");
  const bool kv_fp8 = check_kv_cache(k_cache, "k_cache");
  TORCH_CHECK(check_kv_cache(v_cache, "v_cache") == kv_fp8);
  TORCH_CHECK(q_out.dim() == 2 && head_dim % 8 == 0);
  const int T = q_out.size(0);
  const int nq = (int)(q_out.size(1) / head_dim);
  const int nkv = k_cache.size(1);
  const int block_size = k_cache.size(2);
  TORCH_CHECK(nq * head_dim == q_out.size(1) && k_cache.size(3) == head_dim &&
              v_cache.sizes() == k_cache.sizes());
  TORCH_CHECK(positions.numel() == T && slot_mapping.numel() == T);
  const void* bias_ptr = check_partials(part, bias, nsplits, mrows, T,
                                        (int64_t)(nq + 2 * nkv) * head_dim);
  arks_splitk_rope_and_cache(positions.data_ptr(), part.data_ptr(), bias_ptr,
                             q_out.data_ptr(), k_cache.data_ptr(),
                             v_cache.data_ptr(), slot_mapping.data_ptr(),
                             cos_sin.data_ptr(), T, (int)head_dim, nq, nkv,
                             block_size, (int)nsplits, (int)mrows,
                             kv_fp8 ? 1 : 0, (int)groups, current_stream());
}

void rmsnorm_fp8(torch::Tensor out, torch::Tensor inv_scale,
                 torch::Tensor input, c10::optional<torch::Tensor> residual,
                 torch::Tensor weight, double eps) {
  check_bf16_contig(input, "input");
  check_bf16_contig(weight, "weight");
  TORCH_CHECK(out.scalar_type() == torch::kFloat8_e4m3fn && out.is_contiguous());
  TORCH_CHECK(inv_scale.scalar_type() == torch::kFloat32);
  const int hidden = input.size(-1);
  TORCH_CHECK(hidden % 8 == 0 && hidden <= 8192,
              "rmsnorm_fp8 requires hidden % 8 == 0 and hidden <= 8192");
  const int rows = input.numel() / hidden;
  void* res_ptr = nullptr;
  if (residual.has_value()) {
    check_bf16_contig(*residual, "residual");
    res_ptr = residual->data_ptr();
  }
  arks_rmsnorm_fp8(out.data_ptr(), inv_scale.data_ptr(), input.data_ptr(),
                   res_ptr, weight.data_ptr(), (float)eps, rows, hidden,
                   residual.has_value() ? 1 : 0, current_stream());
}

void silu_mul_fp8(torch::Tensor out, torch::Tensor inv_scale,
                  torch::Tensor gate_up) {
  check_bf16_contig(gate_up, "gate_up");
  TORCH_CHECK(out.scalar_type() == torch::kFloat8_e4m3fn && out.is_contiguous());
  TORCH_CHECK(inv_scale.scalar_type() == torch::kFloat32);
  const int d = out.size(-1);
  TORCH_CHECK(gate_up.size(-1) == 2 * d && d % 8 == 0);
  TORCH_CHECK((int64_t)d * 2 <= 160 * 1024, "row too large for LDS staging");
  const int rows = out.numel() / d;
  arks_silu_mul_fp8(out.data_ptr(), inv_scale.data_ptr(), gate_up.data_ptr(),
                    rows, d, current_stream());
}

void quant_fp8_rows(torch::Tensor out, torch::Tensor inv_scale,
                    torch::Tensor x) {
  check_bf16_contig(x, "x");
  TORCH_CHECK(out.scalar_type() == torch::kFloat8_e4m3fn && out.is_contiguous());
  TORCH_CHECK(inv_scale.scalar_type() == torch::kFloat32);
  TORCH_CHECK(x.size(1) % 8 == 0, "cols must be a multiple of 8");
  arks_quant_fp8_rows(out.data_ptr(), inv_scale.data_ptr(), x.data_ptr(),
                      x.size(0), x.size(1), current_stream());
}

// chunks = workgroups per row. Above 1, `pairs` is the workspace the chunk
// winners go through: int32 [rows, chunks, 2] (value bits, index).
static void* check_sample_pairs(const torch::Tensor& out,
                                const torch::Tensor& logits,
                                const c10::optional<torch::Tensor>& pairs,
                                int64_t chunks) {
  check_bf16_contig(logits, "logits");
  TORCH_CHECK(logits.dim() == 2);
  TORCH_CHECK(out.scalar_type() == torch::kInt64 && out.is_contiguous() &&
              out.numel() >= logits.size(0));
  TORCH_CHECK(1 <= chunks && chunks <= 65535, "chunks in 1..65535");
  if (chunks == 1) return nullptr;
  TORCH_CHECK(pairs.has_value() && pairs->is_cuda() &&
                  pairs->scalar_type() == torch::kInt32 &&
                  pairs->is_contiguous() &&
                  pairs->numel() >= logits.size(0) * chunks * 2,
              "chunks > 1 needs an int32 workspace of rows * chunks * 2");
  return pairs->data_ptr();
}

void greedy_sample(torch::Tensor out, torch::Tensor logits,
                   c10::optional<torch::Tensor> pairs, int64_t chunks) {
  void* ws = check_sample_pairs(out, logits, pairs, chunks);
  arks_greedy_sample(out.data_ptr(), ws, logits.data_ptr(), logits.size(0),
                     logits.size(1), (int)chunks, current_stream());
}

void gumbel_sample(torch::Tensor out, torch::Tensor logits,
                   torch::Tensor temperatures, torch::Tensor uniform,
                   c10::optional<torch::Tensor> pairs, int64_t chunks) {
  void* ws = check_sample_pairs(out, logits, pairs, chunks);
  TORCH_CHECK(temperatures.scalar_type() == torch::kFloat32);
  TORCH_CHECK(uniform.scalar_type() == torch::kFloat32);
  arks_gumbel_sample(out.data_ptr(), ws, logits.data_ptr(),
                     temperatures.data_ptr(), uniform.data_ptr(),
                     logits.size(0), logits.size(1), (int)chunks,
                     current_stream());
}

// masks [slots, ceil(vocab/32)] int32, mask_row [rows] int32 (-1 = none)
static void check_bitmask(const torch::Tensor& logits,
                          const torch::Tensor& masks,
                          const torch::Tensor& mask_row) {
  TORCH_CHECK(logits.dim() == 2 && masks.dim() == 2 && mask_row.dim() == 1);
  TORCH_CHECK(masks.is_cuda() && mask_row.is_cuda());
  TORCH_CHECK(masks.scalar_type() == torch::kInt32 && masks.is_contiguous());
  TORCH_CHECK(mask_row.scalar_type() == torch::kInt32 &&
              mask_row.is_contiguous());
  TORCH_CHECK(masks.size(1) == (logits.size(1) + 31) / 32,
              "masks must have ceil(vocab/32) words per row");
  TORCH_CHECK(mask_row.size(0) == logits.size(0), "one mask_row per row");
}

void greedy_sample_masked(torch::Tensor out, torch::Tensor logits,
                          torch::Tensor masks, torch::Tensor mask_row) {
  check_bf16_contig(logits, "logits");
  check_bitmask(logits, masks, mask_row);
  TORCH_CHECK(out.scalar_type() == torch::kInt64 &&
              out.numel() == logits.size(0));
  arks_greedy_sample_masked(out.data_ptr(), logits.data_ptr(),
                            masks.data_ptr(), mask_row.data_ptr(),
                            logits.size(0), logits.size(1), masks.size(0),
                            current_stream());
}

void gumbel_sample_masked(torch::Tensor out, torch::Tensor logits,
                          torch::Tensor temperatures, torch::Tensor uniform,
                          torch::Tensor masks, torch::Tensor mask_row) {
  check_bf16_contig(logits, "logits");
  check_bitmask(logits, masks, mask_row);
  TORCH_CHECK(out.scalar_type() == torch::kInt64 &&
              out.numel() == logits.size(0));
  TORCH_CHECK(temperatures.scalar_type() == torch::kFloat32 &&
              temperatures.numel() == logits.size(0));
  TORCH_CHECK(uniform.scalar_type() == torch::kFloat32 &&
              uniform.is_contiguous() && uniform.numel() == logits.numel());
  arks_gumbel_sample_masked(out.data_ptr(), logits.data_ptr(),
                            temperatures.data_ptr(), uniform.data_ptr(),
                            masks.data_ptr(), mask_row.data_ptr(),
                            logits.size(0), logits.size(1), masks.size(0),
                            current_stream());
}

void apply_token_bitmask(torch::Tensor logits, torch::Tensor masks,
                         torch::Tensor mask_row) {
  TORCH_CHECK(logits.is_cuda() && logits.is_contiguous());
  const bool f32 = logits.scalar_type() == torch::kFloat32;
  TORCH_CHECK(f32 || logits.scalar_type() == torch::kBFloat16,
              "logits must be bf16 or fp32");
  check_bitmask(logits, masks, mask_row);
  arks_apply_token_bitmask(logits.data_ptr(), f32 ? 1 : 0, masks.data_ptr(),
                           mask_row.data_ptr(), logits.size(0), logits.size(1),
                           masks.size(0), current_stream());
}

// D[16,16] = A[16,32] @ B[32,16], all bf16 in / f32 out. Verifies the MFMA
// fragment layout assumption on hardware.
void tr16_probe(torch::Tensor out, int64_t stride_bytes) {
  TORCH_CHECK(out.scalar_type() == torch::kInt16 && out.numel() >= 256);
  arks_tr16_probe(out.data_ptr(), (int)stride_bytes, current_stream());
}

void mfma_probe32(torch::Tensor d, torch::Tensor a, torch::Tensor b) {
  check_bf16_contig(a, "a");
  check_bf16_contig(b, "b");
  TORCH_CHECK(d.scalar_type() == torch::kFloat32 && d.is_contiguous());
  TORCH_CHECK(a.size(0) == 32 && a.size(1) == 16);
  TORCH_CHECK(b.size(0) == 16 && b.size(1) == 32);
  arks_mfma_probe32(d.data_ptr(), a.data_ptr(), b.data_ptr(), current_stream());
}

// --- p2p one-shot all-reduce plumbing (allreduce.hip) ---
// IPC-shared buffers are raw hipMalloc allocations: a handle for a torch
// caching-allocator tensor maps the UNDERLYING block, so the opened peer
// pointer would miss the tensor's offset inside it.
py::tuple ipc_alloc(int64_t nbytes) {
  void* ptr = nullptr;
  auto err = hipMalloc(&ptr, (size_t)nbytes);
  TORCH_CHECK(err == hipSuccess, "hipMalloc: ", hipGetErrorString(err));
  (void)hipMemset(ptr, 0, (size_t)nbytes);
  hipIpcMemHandle_t h;
  err = hipIpcGetMemHandle(&h, ptr);
  TORCH_CHECK(err == hipSuccess, "hipIpcGetMemHandle: ",
              hipGetErrorString(err));
  return py::make_tuple(
      reinterpret_cast<int64_t>(ptr),
      py::bytes(reinterpret_cast<const char*>(&h), sizeof(h)));
}

void ipc_alloc_free(int64_t ptr) {
  (void)hipFree(reinterpret_cast<void*>(ptr));
}

// test hook: arm a raw flag buffer with huge values (0x7f per byte) so the
// single-GPU sequential harness never spins
void arm_flags(int64_t ptr, int64_t n) {
  (void)hipMemset(reinterpret_cast<void*>(ptr), 0x7f, (size_t)n * 8);
}

py::bytes ipc_handle(torch::Tensor t) {
  TORCH_CHECK(t.is_cuda(), "ipc_handle wants a CUDA tensor");
  hipIpcMemHandle_t h;
  auto err = hipIpcGetMemHandle(&h, t.data_ptr());
  TORCH_CHECK(err == hipSuccess, "hipIpcGetMemHandle: ",
              hipGetErrorString(err));
  return py::bytes(reinterpret_cast<const char*>(&h), sizeof(h));
}

int64_t ipc_open(py::bytes handle) {
  std::string s = handle;
  TORCH_CHECK(s.size() == sizeof(hipIpcMemHandle_t), "bad handle size");
  hipIpcMemHandle_t h;
  memcpy(&h, s.data(), sizeof(h));
  void* ptr = nullptr;
  auto err = hipIpcOpenMemHandle(&ptr, h, hipIpcMemLazyEnablePeerAccess);
  TORCH_CHECK(err == hipSuccess, "hipIpcOpenMemHandle: ",
              hipGetErrorString(err));
  return reinterpret_cast<int64_t>(ptr);
}

void ipc_close(int64_t ptr) {
  (void)hipIpcCloseMemHandle(reinterpret_cast<void*>(ptr));
}

void one_shot_allreduce(torch::Tensor out, torch::Tensor src,
                        std::vector<int64_t> mail,
                        std::vector<int64_t> flags, torch::Tensor seq,
                        int64_t rank) {  // mail/flags: ipc_alloc'd raw ptrs
  check_bf16_contig(out, "out");
  check_bf16_contig(src, "src");
  TORCH_CHECK(seq.is_cuda() && seq.scalar_type() == torch::kInt64);
  const int world = (int)mail.size();
  TORCH_CHECK(world == (int)flags.size());
  TORCH_CHECK(world == 1 || world == 2 || world == 4 || world == 8,
              "world must be 1/2/4/8");
  const int64_t n = src.numel();
  TORCH_CHECK(n % 8 == 0, "numel must be a multiple of 8");
  TORCH_CHECK(out.numel() == n);
  void* mp[8] = {};
  void* fp[8] = {};
  for (int p = 0; p < world; ++p) {
    mp[p] = reinterpret_cast<void*>(mail[p]);
    fp[p] = reinterpret_cast<void*>(flags[p]);
  }
  auto stream = current_stream();
  arks_ar_seq_inc(seq.data_ptr(), stream);
  arks_one_shot_allreduce(out.data_ptr(), src.data_ptr(), mp, fp,
                          seq.data_ptr(), (int)rank, world, n, stream);
}

void moe_topk(torch::Tensor weights, torch::Tensor ids,
              torch::Tensor logits, int64_t k, int64_t renorm) {
  TORCH_CHECK(logits.is_cuda() && logits.is_contiguous() &&
              logits.scalar_type() == torch::kFloat32, "logits f32 contig");
  TORCH_CHECK(weights.scalar_type() == torch::kFloat32 &&
              ids.scalar_type() == torch::kInt32);
  const int T = logits.size(0), E = logits.size(1);
  TORCH_CHECK(k >= 1 && k <= 16 && E <= 1024 && k <= E,
              "need 1 <= k <= min(16, E), E <= 1024");
  arks_moe_topk(weights.data_ptr(), ids.data_ptr(), logits.data_ptr(), T, E,
                (int)k, (int)renorm, current_stream());
}

// counts i32 [n_local], pairs i32 [n_local, T] from ids i32 [T, k].
void moe_route(torch::Tensor counts, torch::Tensor pairs, torch::Tensor ids,
               int64_t expert_base) {
  TORCH_CHECK(ids.is_cuda() && ids.scalar_type() == torch::kInt32 &&
              ids.is_contiguous() && ids.dim() == 2 && ids.size(0) >= 1 &&
              ids.size(1) >= 1, "ids must be contiguous int32 [T, k] on GPU");
  const int64_t T = ids.size(0), n_pairs = ids.numel();
  TORCH_CHECK(n_pairs < ((int64_t)1 << 30));
  TORCH_CHECK(counts.is_cuda() && counts.scalar_type() == torch::kInt32 &&
              counts.is_contiguous() && counts.dim() == 1 &&
              counts.size(0) >= 1 && counts.size(0) <= 65535,
              "counts must be int32 [E_local] on GPU");
  TORCH_CHECK(pairs.is_cuda() && pairs.scalar_type() == torch::kInt32 &&
              pairs.is_contiguous() && pairs.dim() == 2 &&
              pairs.size(0) == counts.size(0) && pairs.size(1) == T,
              "pairs must be int32 [E_local, T] on GPU");
  TORCH_CHECK(counts.device() == ids.device() &&
              pairs.device() == ids.device());
  arks_moe_route(counts.data_ptr(), pairs.data_ptr(), ids.data_ptr(),
                 (int)n_pairs, (int)T, (int)expert_base, (int)counts.size(0),
                 current_stream());
}

void moe_mix(torch::Tensor out, torch::Tensor y, torch::Tensor weights,
             torch::Tensor ids, int64_t expert_base, int64_t n_local) {
  check_bf16_contig(out, "out");
  check_bf16_contig(y, "y");
  TORCH_CHECK(weights.scalar_type() == torch::kFloat32 &&
              ids.scalar_type() == torch::kInt32);
  const int T = out.size(0), H = out.size(1);
  const int k = weights.size(1);
  TORCH_CHECK(k <= 16 && H % 2 == 0);
  TORCH_CHECK(y.size(1) == T && y.size(2) == H && y.size(0) == n_local);
  arks_moe_mix(out.data_ptr(), y.data_ptr(), weights.data_ptr(),
               ids.data_ptr(), T, H, k, (int)expert_base, (int)n_local,
               current_stream());
}

void moe_mix_rows(torch::Tensor out, torch::Tensor y,
                  torch::Tensor weights, torch::Tensor rows) {
  check_bf16_contig(out, "out");
  check_bf16_contig(y, "y");
  TORCH_CHECK(weights.scalar_type() == torch::kFloat32 &&
              rows.scalar_type() == torch::kInt32);
  const int T = out.size(0), H = out.size(1);
  const int k = weights.size(1);
  TORCH_CHECK(k <= 16 && H % 2 == 0);
  TORCH_CHECK(rows.size(0) == T && rows.size(1) == k);
  arks_moe_mix_rows(out.data_ptr(), y.data_ptr(), weights.data_ptr(),
                    rows.data_ptr(), T, H, k, current_stream());
}

// --- multi-LoRA (lora.hip) ---
void check_lora_tiles(const torch::Tensor& tiles) {
  TORCH_CHECK(tiles.is_cuda() && tiles.scalar_type() == torch::kInt32 &&
                  tiles.is_contiguous() && tiles.dim() == 2 &&
                  tiles.size(1) == 3,
              "tiles must be a contiguous int32 [ntiles, 3] GPU tensor");
}

void check_align16(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, name,
              " must be 16-byte aligned");
}

// h[row, :] = x[row, :] . A[slot]^T for the rows the tile table covers.
void lora_shrink(torch::Tensor h, torch::Tensor x, torch::Tensor a,
                 torch::Tensor tiles) {
  check_bf16_contig(x, "x");
  check_bf16_contig(a, "A");
  check_lora_tiles(tiles);
  TORCH_CHECK(x.dim() == 2 && a.dim() == 3, "x is [T, K], A is [L, S*R, K]");
  const int64_t T = x.size(0), K = x.size(1), SR = a.size(1);
  TORCH_CHECK(a.size(2) == K, "A depth ", a.size(2), " != x width ", K);
  TORCH_CHECK(K % 32 == 0, "lora_shrink requires K % 32 == 0, got ", K);
  TORCH_CHECK(SR % 16 == 0 && SR >= 16, "S*R must be a multiple of 16");
  TORCH_CHECK(h.is_cuda() && h.scalar_type() == torch::kFloat32 &&
                  h.is_contiguous() && h.dim() == 2 && h.size(1) == SR &&
                  h.size(0) >= T,
              "h must be a contiguous f32 [>=T, S*R] workspace");
  check_align16(x, "x");
  check_align16(a, "A");
  arks_lora_shrink(h.data_ptr(), x.data_ptr(), a.data_ptr(), tiles.data_ptr(),
                   (int)tiles.size(0), (int)T, (int)K, (int)SR,
                   (int)a.size(0), current_stream());
}

// y[row, n] += sum_j h[row, s(n) R + j] B[slot][n, j], in place.
void lora_expand(torch::Tensor y, torch::Tensor h, torch::Tensor b,
                 torch::Tensor tiles, std::vector<int64_t> slice_offsets) {
  check_bf16_contig(y, "y");
  check_bf16_contig(b, "B");
  check_lora_tiles(tiles);
  TORCH_CHECK(y.dim() == 2 && b.dim() == 3, "y is [T, N], B is [L, N, R]");
  const int64_t T = y.size(0), N = y.size(1), R = b.size(2);
  TORCH_CHECK(b.size(1) == N, "B rows ", b.size(1), " != y width ", N);
  TORCH_CHECK(N % 16 == 0, "lora_expand requires N % 16 == 0, got ", N);
  TORCH_CHECK(R == 16 || R == 32 || R == 64, "rank must be 16, 32 or 64");
  const int64_t S = (int64_t)slice_offsets.size() - 1;
  TORCH_CHECK(S >= 1 && S <= 3, "1 to 3 slices");
  TORCH_CHECK(slice_offsets[0] == 0 && slice_offsets[S] == N,
              "slice_offsets must run from 0 to N");
  for (int64_t s = 0; s < S; ++s) {
    TORCH_CHECK(slice_offsets[s] < slice_offsets[s + 1] &&
                    slice_offsets[s + 1] % 16 == 0,
                "slice offsets must increase in multiples of 16");
  }
  TORCH_CHECK(h.is_cuda() && h.scalar_type() == torch::kFloat32 &&
                  h.is_contiguous() && h.dim() == 2 && h.size(1) == S * R &&
                  h.size(0) >= T,
              "h must be a contiguous f32 [>=T, S*R] workspace");
  check_align16(y, "y");
  check_align16(h, "h");
  check_align16(b, "B");
  arks_lora_expand(y.data_ptr(), h.data_ptr(), b.data_ptr(), tiles.data_ptr(),
                   (int)tiles.size(0), (int)T, (int)N, (int)R, (int)S,
                   S > 1 ? (int)slice_offsets[1] : (int)N,
                   S > 2 ? (int)slice_offsets[2] : (int)N, (int)b.size(0),
                   current_stream());
}

// Embedding pooling (pooling.hip): one f32 vector per row of the segment
// table. The table's contents are validated where it is built
// (ops.build_pool_table); here the buffers are checked against its shape.
void pool_embed(torch::Tensor out, torch::Tensor carry, torch::Tensor part,
                torch::Tensor x, torch::Tensor residual, torch::Tensor weight,
                torch::Tensor segs, torch::Tensor slabs, double eps,
                int64_t dims, bool normalize) {
  check_bf16_contig(x, "x");
  check_bf16_contig(residual, "residual");
  check_bf16_contig(weight, "weight");
  TORCH_CHECK(x.dim() == 2 && x.sizes() == residual.sizes(),
              "x and residual are [T, H]");
  const int64_t H = x.size(1);
  TORCH_CHECK(H % 8 == 0, "pool_embed requires H % 8 == 0, got ", H);
  TORCH_CHECK(H <= arks_pool_max_hidden(), "pool_embed supports H <= ",
              arks_pool_max_hidden(), ", got ", H);
  TORCH_CHECK(weight.numel() == H, "weight must be [H]");
  TORCH_CHECK(dims >= 1 && dims <= H, "dims must be in [1, ", H, "], got ",
              dims);
  auto i32 = [](const torch::Tensor& t, int64_t cols, const char* name) {
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kInt32 &&
                    t.is_contiguous() && t.dim() == 2 && t.size(1) == cols,
                name, " must be a contiguous int32 [n, ", cols, "] GPU tensor");
  };
  i32(segs, 8, "segs");
  i32(slabs, 4, "slabs");
  auto f32 = [](const torch::Tensor& t, const char* name) {
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kFloat32 &&
                    t.is_contiguous(),
                name, " must be a contiguous f32 GPU tensor");
  };
  f32(out, "out");
  f32(carry, "carry");
  f32(part, "part");
  const int64_t S = segs.size(0), NS = slabs.size(0);
  TORCH_CHECK(S >= 1, "empty segment table");
  TORCH_CHECK(out.dim() == 2 && out.size(0) == S && out.size(1) == dims,
              "out must be [num_segments, dims]");
  TORCH_CHECK(carry.dim() == 2 && carry.size(1) == H, "carry must be [slots, H]");
  TORCH_CHECK(part.numel() >= NS * H, "partial workspace too small");
  check_align16(x, "x");
  check_align16(residual, "residual");
  check_align16(weight, "weight");
  if (NS > 0) check_align16(part, "part");
  if (carry.numel() > 0) check_align16(carry, "carry");
  arks_pool_embed(out.data_ptr(), carry.data_ptr(), part.data_ptr(),
                  x.data_ptr(), residual.data_ptr(), weight.data_ptr(),
                  segs.data_ptr(), slabs.data_ptr(), (int)S, (int)NS,
                  (float)eps, (int)H, (int)dims, normalize ? 1 : 0,
                  current_stream());
}

void mfma_probe(torch::Tensor d, torch::Tensor a, torch::Tensor b) {
  check_bf16_contig(a, "a");
  check_bf16_contig(b, "b");
  TORCH_CHECK(d.scalar_type() == torch::kFloat32 && d.is_contiguous());
  TORCH_CHECK(a.size(0) == 16 && a.size(1) == 32);
  TORCH_CHECK(b.size(0) == 32 && b.size(1) == 16);
  arks_mfma_probe(d.data_ptr(), a.data_ptr(), b.data_ptr(), current_stream());
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("rmsnorm", &rmsnorm);
  m.def("fused_add_rmsnorm", &fused_add_rmsnorm);
  m.def("silu_mul", &silu_mul);
  m.def("rope_inplace", &rope_inplace);
  m.def("reshape_and_cache", &reshape_and_cache);
  m.def("rope_and_cache", &rope_and_cache);
  m.def("attention_decode_paged", &attention_decode_paged);
  m.def("attention_prefill_varlen", &attention_prefill_varlen);
  m.def("attention_extend_paged", &attention_extend_paged);
  m.def("attention_extend_paged2", &attention_extend_paged2);
  m.def("attention_extend2_combine", &attention_extend2_combine);
  m.def("quant_fp8_rows", &quant_fp8_rows);
  m.def("rmsnorm_fp8", &rmsnorm_fp8);
  m.def("silu_mul_fp8", &silu_mul_fp8);
  m.def("skinny_gemm", &skinny_gemm, py::arg("out"), py::arg("part"),
        py::arg("a"), py::arg("w"), py::arg("bias"), py::arg("k_per_split"),
        py::arg("nsplits"), py::arg("config") = 0, py::arg("groups") = 0);
  m.def("skinny_gemm_partials", &skinny_gemm_partials, py::arg("part"),
        py::arg("a"), py::arg("w"), py::arg("k_per_split"),
        py::arg("nsplits"), py::arg("config") = 0, py::arg("groups") = 0);
  m.def("skinny_combine", &skinny_combine);
  m.def("w4_skinny_gemm", &w4_skinny_gemm);
  m.def("w4_skinny_gemm_partials", &w4_skinny_gemm_partials);
  m.def("w4_dequant", &w4_dequant);
  m.def("w4_moe_gemm", &w4_moe_gemm);
  m.def("w8_skinny_gemm", &w8_skinny_gemm);
  m.def("w8_skinny_gemm_partials", &w8_skinny_gemm_partials);
  m.def("w8_dequant", &w8_dequant);
  m.def("w8_moe_gemm", &w8_moe_gemm);
  m.def("mx4_skinny_gemm", &mx4_skinny_gemm);
  m.def("mx4_skinny_gemm_partials", &mx4_skinny_gemm_partials);
  m.def("mx4_dequant", &mx4_dequant);
  m.def("splitk_add_rmsnorm", &splitk_add_rmsnorm);
  m.def("splitk_rope_and_cache", &splitk_rope_and_cache, py::arg("positions"),
        py::arg("part"), py::arg("bias"), py::arg("q_out"), py::arg("k_cache"),
        py::arg("v_cache"), py::arg("slot_mapping"), py::arg("cos_sin"),
        py::arg("head_dim"), py::arg("nsplits"), py::arg("mrows"),
        py::arg("groups") = 1);
  m.def("greedy_sample", &greedy_sample, py::arg("out"), py::arg("logits"),
        py::arg("pairs") = py::none(), py::arg("chunks") = 1);
  m.def("gumbel_sample", &gumbel_sample, py::arg("out"), py::arg("logits"),
        py::arg("temperatures"), py::arg("uniform"),
        py::arg("pairs") = py::none(), py::arg("chunks") = 1);
  m.def("greedy_sample_masked", &greedy_sample_masked);
  m.def("gumbel_sample_masked", &gumbel_sample_masked);
  m.def("apply_token_bitmask", &apply_token_bitmask);
  m.def("ipc_alloc", &ipc_alloc);
  m.def("arm_flags", &arm_flags);
  m.def("ipc_alloc_free", &ipc_alloc_free);
  m.def("ipc_handle", &ipc_handle);
  m.def("ipc_open", &ipc_open);
  m.def("ipc_close", &ipc_close);
  m.def("one_shot_allreduce", &one_shot_allreduce);
  m.def("moe_topk", &moe_topk);
  m.def("moe_route", &moe_route);
  m.def("moe_mix", &moe_mix);
  m.def("moe_mix_rows", &moe_mix_rows);
  m.def("lora_shrink", &lora_shrink);
  m.def("lora_expand", &lora_expand);
  m.def("pool_embed", &pool_embed);
  m.def("mfma_probe", &mfma_probe);
  m.def("mfma_probe32", &mfma_probe32);
  m.def("tr16_probe", &tr16_probe);
}
