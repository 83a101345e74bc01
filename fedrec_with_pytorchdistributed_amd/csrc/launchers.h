// The launcher ABI: one declaration of every plain-C launcher (fr_*) the kernel files export.
//
// Torch-free.  Every *.hip file includes it, so each definition is checked against its
// declaration where it is written; the binding sources (bind_*.cpp) include it to call them.
// extern "C" symbols carry no types at link time: a launcher declared anywhere else could
// drift from its definition and still link.  A launcher returns non-zero for a shape it was
// not written for (the two-pass ones return the scratch floats they need, negative = rejected).
#pragma once
#include <hip/hip_runtime_api.h>

extern "C" {

// ---- gemm_bf16.hip ---------------------------------------------------------------------------
int fr_num_cus();  // the current device's CU count, queried once (256 if the query fails); every file's grid sizing
void fr_gemm_set_variant(int v);
int fr_gemm_nt_bf16(const void* A, const void* W, const float* bias, const void* R, void* C, int M, int N, int K, int act,
                    int c_rows, hipStream_t s);
int fr_gemm_nt_bf16_split(const void* A, const void* W, const float* bias, void* C, int M, int N, int K, int c_rows,
                          const int* full_rows, int n_partial, hipStream_t s);
int fr_gemm_gelu_bwd_colpart(const void* A, const void* W, const void* Z, void* C, float* colpart, int M, int N, int K,
                             int c_rows, hipStream_t s);
int fr_gemm_nt_bf16_dual(const void* A, const void* W, const float* bias, void* C, void* Z, int M, int N, int K,
                         int c_rows, hipStream_t s);

// ---- gemm_wgrad.hip --------------------------------------------------------------------------
long fr_wgrad_bf16(const void* dY, const void* X, float* C, float* scratch, int M, int N, int K, int accumulate,
                   hipStream_t s);

// ---- layernorm.hip ---------------------------------------------------------------------------
void fr_ln_set_wide(int v);
int fr_layer_norm_bf16(const void* x, const float* w, const float* b, void* y, int rows, int D, float eps,
                       const void* res, hipStream_t s);
int fr_layer_norm_scatter_bf16(const void* x, const float* w, const float* b, void* y, int rows, int D, float eps,
                               const void* res, const int* dst, hipStream_t s);
int fr_layer_norm_bwd_bf16(const void* x, const float* w, const void* dy, void* dx, float* dw, float* db, int rows, int D,
                           float eps, hipStream_t s, float* dxs, void* dxz, float pdrop, unsigned long long seed,
                           unsigned long long offset);
int fr_gelu_bf16(const void* z, const void* dh, void* out, long n, int bwd, hipStream_t s);
int fr_embed_ln_bf16(const int* tokens, const void* word, const void* pos, const float* w, const float* b, void* y,
                     int rows, int D, int T, float eps, hipStream_t s);
int fr_embed_ln_rows_bf16(const int* tokens, const int* src, const void* word, const void* pos, const float* w,
                          const float* b, void* y, int rows, int D, int T, float eps, hipStream_t s);

// ---- dropout.hip -----------------------------------------------------------------------------
int fr_dropout_add_bf16(const void* h, const void* res, void* out, long n, float p, unsigned long long seed,
                        unsigned long long offset, hipStream_t s);

// ---- title_attn.hip (T <= 64; longer titles go on to title_attn_long.hip) --------------------
void fr_title_attn_set_waves(int w);
int fr_title_attention_bf16(const void* qkv, const int* mask, void* out, int n_titles, int T, int H, int D,
                            hipStream_t s);
int fr_title_attention_drop_bf16(const void* qkv, const int* mask, void* out, int n_titles, int T, int H, int D,
                                 float pdrop, unsigned long long seed, unsigned long long offset, hipStream_t s);
int fr_title_plan(const int* mask, int n, int T, int* rowmap, int* src, int* kv_start, int* kv_len, int* qstart,
                  int* n_kv, hipStream_t s);
int fr_title_attention_packed_bf16(const void* qkv, const int* rowmap, const int* kv_start, const int* kv_len,
                                   const int* qstart, void* out, int n_titles, int T, int H, int D, hipStream_t s);

// ---- title_attn_bwd.hip ----------------------------------------------------------------------
void fr_title_attn_bwd_set_variant(int v);
int fr_title_attention_bwd_bf16(const void* qkv, const void* dout, const int* mask, void* dqkv, int n_titles, int T, int H,
                                int D, hipStream_t s);
int fr_title_attention_bwd_drop_bf16(const void* qkv, const void* dout, const int* mask, void* dqkv, int n_titles,
                                     int T, int H, int D, float pdrop, unsigned long long seed,
                                     unsigned long long offset, hipStream_t s);

// ---- title_attn_long.hip (64 < T <= 512; called by the two files above) ----------------------
int fr_title_attention_long_bf16(const void* qkv, const int* mask, void* out, int n_titles, int T, int H, int D,
                                 hipStream_t s);
int fr_title_attention_bwd_long_bf16(const void* qkv, const void* dout, const int* mask, void* dqkv, int n_titles,
                                     int T, int H, int D, hipStream_t s);

// ---- train_grad.hip --------------------------------------------------------------------------
int fr_colsum_chunks();
int fr_colsum_bf16(const void* x, int M, int N, float* partial, float* out, hipStream_t s, int ld);
int fr_gelu_bwd_colsum_bf16(const void* df, const void* z, void* dz, int M, int N, float* partial, float* out,
                            hipStream_t s);
int fr_embed_grad_bf16(const void* dx, const int* sorted, const int* perm, int R, int D, float* dword, int* scratch,
                       hipStream_t s);

// ---- text_head.hip ---------------------------------------------------------------------------
void fr_head_score_set_rows(int r);
void fr_head_score_set_ilv(int v);
int fr_head_supported(int D, int Q, int T);
int fr_head_g_supported(int D, int Q, int T);
int fr_head_score(const void* table, const int* ids, int U, int T, int D, int Q, const void* W1, const float* b1,
                  const float* w2, const float* b2, void* e_out, float* a_out, const int* nreal, hipStream_t s);
int fr_head_pool(const void* table, const int* ids, const float* a, const int* tokens, int U, int T, int D, float* pooled,
                 float* alpha, const int* nreal, hipStream_t s, void* pooled_b);
int fr_head_pool_bwd(const void* table, const int* ids, const float* alpha, const float* g, int U, int T, int D,
                     float* da, float* db2p, const int* nreal, hipStream_t s);
long fr_head_wgrad(const void* e, const void* table, const int* ids, const float* da, const float* db2p,
                   const float* w2, int U, int T, int D, int Q, float* dW1, float* db1, float* dw2, float* db2,
                   float* scratch, const int* nreal, hipStream_t s);
int fr_head_pool_bwd_g(const void* table, const int* ids, const float* alpha, const float* g, int U, int T, int D,
                       int Q, float* da, float* db2p, void* e, float* cs, const int* nreal, hipStream_t s);
long fr_head_wgrad_g(const void* G, const void* table, const int* ids, const float* cs, const float* db2p,
                     const float* w2, int U, int T, int D, int Q, float* dW1, float* db1, float* dw2, float* db2,
                     float* scratch, const int* nreal, hipStream_t s, const void* pend, int pend_cblocks,
                     int pend_total);

// ---- additive_pool.hip -----------------------------------------------------------------------
int fr_additive_pool_fwd(const void* x, const void* e, const float* w2, const float* b2, float* out, float* alpha,
                         int n, int T, int D, int Q, int is_bf16, const int* keep, hipStream_t s);
int fr_additive_pool_rows(int T, int D, int Q, int is_bf16);
int fr_additive_pool_bwd(const void* x, const void* e, const float* alpha, const float* w2, const float* g, float* dx,
                         void* dpre, float* dw2, float* db2, float* dsum, int n, int T, int D, int Q, int R,
                         int is_bf16, hipStream_t s);
int fr_upool_bwd_da(const float* x, const float* e, const float* alpha, const float* w2, const float* g, float* dx,
                    float* dpre, float* da8, int n, int T, int D, int Q, hipStream_t s, void* dpre_b);

// ---- user_attn.hip ---------------------------------------------------------------------------
int fr_user_attn_fwd(const float* qkv, float* ctx, float* stats, int B, int H, int NH, int dk, const int* keep,
                     hipStream_t s, void* ctx_b);
int fr_user_qkv_attn_fwd(const void* xd, const void* W, const float* bias, int Din, float* qkv, float* ctx,
                         float* stats, int B, int H, int NH, int dk, const int* keep, hipStream_t s, void* ctx_b);
int fr_user_attn_bwd_dctx(const float* qkv, const float* stats, const float* dctx, void* dqkv, const void* dpre,
                          const void* w1t, int Qd, int B, int H, int NH, int dk, const int* keep, hipStream_t s);
int fr_user_attn_bwd(const float* qkv, const float* stats, const float* dctx, void* dqkv, int B, int H, int NH,
                     int dk, const int* keep, hipStream_t s, int out_bf16);

// ---- score_ce.hip ----------------------------------------------------------------------------
void fr_score_set_variant(int v);
int fr_score_ce(const float* cand, const float* user, float* loss, float* scores, float* dcand, float* duser, int B,
                int C, int D, int sigm, const int* ci, float* loss_total, hipStream_t s);
int fr_user_pool_score(const float* x, const float* e, const float* w2, const float* b2, const int* keep,
                       const float* cand, const int* ci, int B, int T, int D, int Q, int C, int sigm, float* lossb,
                       float* scores, float* dcand, float* loss_total, float* dctx, float* dpre, void* dpre_b,
                       float* da8, hipStream_t s);

// ---- news_grad.hip ---------------------------------------------------------------------------
void fr_segsum_set_variant(int v);
void fr_segsum_set_ldp_block(int v);
int fr_segsum_chunks(int R);
int fr_segment_sum_rows(const float* rows, const int* perm, const int* seg_ptr, const int* inv, float* out, int U, int D,
                        int R, float* scratch, hipStream_t s, int zero_empty);
int fr_segment_sum_rows_ldp(const float* rows, const int* perm, const int* seg_ptr, const int* inv, float* out, int U,
                            int D, int R, float* scratch, float clip, float noise_std, unsigned long long seed,
                            unsigned long long offset, const unsigned long long* dev_off, hipStream_t s);
int fr_ldp_rows(const float* rows, float* out, int R, int D, float clip, float noise_std, unsigned long long seed,
                unsigned long long offset, hipStream_t s, const unsigned long long* dev_off);

// ---- small_gemm.hip --------------------------------------------------------------------------
void fr_small_gemm_set_rd(int v);
void fr_small_gemm_set_defer(int on);
long fr_small_gemm(const void* const* ptrs, const int* ints, const float* floats, const unsigned long long* seeds,
                   const unsigned long long* dev_off, int n, float* scratch, int tile, hipStream_t s);
int fr_small_gemm_has_pending();
int fr_small_gemm_batch_bytes();  // also text_head.hip: the pending batch that rides in fr_head_wgrad_g
int fr_small_gemm_take_pending(void* dst, int dst_bytes, int* c_blocks, int* total);
int fr_small_gemm_flush_pending(hipStream_t s);
long fr_colsum_f32(const float* const* xs, float* const* outs, const int* ints, int n, float* part, hipStream_t s);
int fr_gather_dropout(const float* v, const int* idx, void* out, int out_bf16, int M, int K, float p,
                      unsigned long long seed, unsigned long long offset, const unsigned long long* dev_off,
                      hipStream_t s);

// ---- adam.hip --------------------------------------------------------------------------------
int fr_adam_flat(float* p, const float* g, float* m, float* v, void* plow, long n, float lr, float b1, float b2,
                 float omb1, float omb2, float eps, float bc1, float bc2, float grad_scale, hipStream_t s);
int fr_adam_dev(float* p, float* g, float* m, float* v, void* plow, long n, float lr, double b1, double b2, float omb1,
                float omb2, float eps, float grad_scale, const long long* step, const float* loss, float* ring,
                int ring_n, hipStream_t s, int nseg, const float* const* gsrc, const long* goff, const long* gn,
                const int* skip);
int fr_multi_cast(const float* const* src, void* const* dst, const long* n, const int* to_bf16, int nseg,
                  long long* bump, hipStream_t s, long long* bump2, const long* nsrc, const int* fill, int ntseg,
                  const float* const* tsrc, void* const* tdst, const int* tR, const int* tC, const int* tld);
int fr_multi_cast_t(const float* const* src, void* const* dst, const int* R, const int* C, const int* ld, int nseg,
                    hipStream_t s);

// ---- batch.hip -------------------------------------------------------------------------------
int fr_sample_batch(const int* rows, const int* pos, const long long* neg_ptr, const int* negs, const long long* his_ptr,
                    const int* his, int* cand, int* hout, int B, int npr, int H, int truncate, unsigned long long seed,
                    unsigned long long offset, int valid, hipStream_t s);
int fr_dedup(const int* ids, int R, int num_news, int* uniq, int* inv, int* perm, int* seg_ptr, int* u_count,
             hipStream_t s);
int fr_multi_copy(const int* const* src, int* const* dst, const long* nsrc, const long* ndst, const int* fill, int n,
                  hipStream_t s);

// ---- topk_scores.hip -------------------------------------------------------------------------
void fr_topk_set_splits(int s);
int fr_topk_splits(long B, long N);
int fr_topk_scores(const float* user, const float* table, const int* exclude, void* ws, float* scores, int* ids, long B,
                   long N, int D, long E, int k, int min_id, hipStream_t s);

// ---- rank_impressions.hip --------------------------------------------------------------------
long fr_rank_impressions_ws(long M);
int fr_rank_impressions(const float* user, const float* table, const int* pos, const long long* neg_ptr,
                        const int* negs, void* ws, int* counts, long B, long N, int D, long I, long M, long row0,
                        hipStream_t s);

// ---- mmr_rerank.hip --------------------------------------------------------------------------
int fr_mmr_rerank(const float* table, const int* ids, const float* rel, int* ids_out, float* rel_out, float* ild,
                  long B, long N, int P, int D, int k, float lam, hipStream_t s);

// ---- robust_agg.hip --------------------------------------------------------------------------
int fr_trimmed_mean(const float* stack, float* out, long long* dropped, int W, long n, int trim, hipStream_t s);

// ---- sparse_delta.hip ------------------------------------------------------------------------
long fr_topk_delta_ws(long n);  // workspace of fr_topk_delta in 32-bit words
int fr_topk_delta(const float* local, const float* global, float* residual, int* idx, float* val, unsigned* ws, long n,
                  long k, hipStream_t s);
int fr_sparse_combine(const float* base, const int* idx, const float* val, const float* weights, float* out, int W,
                      long k, long n, hipStream_t s);

// ---- quant_delta.hip -------------------------------------------------------------------------
int fr_quantize_delta(const float* local, const float* global, float* residual, unsigned char* codes, float* scales,
                      long n, int bits, unsigned long long seed, unsigned long long offset, hipStream_t s);
int fr_dequant_combine(const float* base, const unsigned char* codes, const float* scales, const float* weights,
                       float* out, int W, long n, int bits, hipStream_t s);

// ---- secagg.hip ------------------------------------------------------------------------------
int fr_secagg_mask(const float* x, int* out, long n, float scale, float clipv, const unsigned long long* seeds,
                   const int* signs, int npeers, unsigned long long round, hipStream_t s);
int fr_secagg_unmask(const int* x, float* out, long n, float inv_scale, hipStream_t s);
int fr_secagg_hist(const float* x, long n, unsigned* scratch, int* out, const unsigned long long* seeds,
                   const int* signs, int npeers, unsigned long long round, hipStream_t s);
int fr_secagg_mask_exact(const float* x, int* out, long n, const int* H, int W, const unsigned long long* seeds,
                         const int* signs, int npeers, unsigned long long round, hipStream_t s);
int fr_secagg_unmask_exact(const int* x, float* out, long n, const int* H, int W, hipStream_t s);

// ---- ipc_allreduce.hip -----------------------------------------------------------------------
int fr_ipc_create(long cap, void* handle_out);
int fr_ipc_open(int id, const void* handles, int me, int W, const long long* local_ptrs);
long long fr_ipc_region(int id);
int* fr_ipc_status(int id);
int fr_ipc_allreduce(int id, void* x, long n, int is_int, long long epoch, int mode, int blocks, double timeout_s,
                     hipStream_t s);
int fr_ipc_allreduce_local(const int* ids, void* const* xs, int W, long n, int is_int, long long epoch, int mode,
                           int blocks, double timeout_s, hipStream_t s);
int fr_ipc_destroy(int id);
}
