// fedrec ops of the user-side training step: user attention (user_attn.hip), candidate scoring +
// cross-entropy (score_ce.hip), the news-gradient segment sums (news_grad.hip) and the batched
// small GEMMs with their column sums and gathers (small_gemm.hip).
#include "binding_util.h"

at::Tensor fedrec::g_sg_pending_scratch;

namespace {

// ctx_b (optional, bf16 [B, H, heads * head_dim], written): ctx rounded to bf16 as well
Tensor2 user_attention_fwd(const at::Tensor& qkv, int64_t heads, int64_t head_dim, const OptTensor& keep,
                           const OptTensor& ctx_b) {
  check_dev(qkv, "qkv");
  TORCH_CHECK(qkv.scalar_type() == at::kFloat && qkv.dim() == 3, "fedrec::user_attention_fwd: fp32 [B,H,3D]");
  const c10::DeviceGuard g(qkv.device());
  const int64_t B = qkv.size(0), H = qkv.size(1);
  TORCH_CHECK(qkv.size(2) == 3 * heads * head_dim, "fedrec::user_attention_fwd: width");
  auto ctx = at::empty({B, H, heads * head_dim}, qkv.options());
  auto stats = at::empty({B, heads, H, 2}, qkv.options());
  void* cb = nullptr;
  if (ctx_b.has_value()) {
    check_dev(*ctx_b, "ctx_b");
    TORCH_CHECK(ctx_b->scalar_type() == at::kBFloat16 && ctx_b->numel() == ctx.numel(),
                "fedrec::user_attention_fwd: ctx_b bf16 like ctx");
    cb = H <= 64 ? ctx_b->data_ptr() : nullptr;  // long histories: converted below
  }
  check_rc(fr_user_attn_fwd(qkv.data_ptr<float>(), ctx.data_ptr<float>(), stats.data_ptr<float>(), (int)B, (int)H,
                            (int)heads, (int)head_dim, key_mask_ptr(keep, B, H, "user_attention_fwd"), cur_stream(), cb),
           "user_attention_fwd");
  if (ctx_b.has_value() && cb == nullptr) ctx_b->copy_(ctx.view_as(*ctx_b));
  return {ctx, stats};
}

// The Q|K|V projection fused into the attention forward (user_attn.hip user_qkv_attn_fwd_kernel):
// xd bf16 [B*H, Din] (the gathered, dropped-out history rows), W bf16 [3*heads*head_dim, Din],
// bias fp32 [3*heads*head_dim] -> (ctx [B, H, D], stats, qkv [B, H, 3D] fp32 -- the backward's
// input).  H <= 64; ctx_b (optional): ctx rounded to bf16 as well.
Tensor3 user_qkv_attention_fwd(const at::Tensor& xd, const at::Tensor& W, const at::Tensor& bias, int64_t B, int64_t heads,
                               int64_t head_dim, const OptTensor& keep, const OptTensor& ctx_b) {
  check_dev(xd, "xd");
  check_dev(W, "W");
  check_dev(bias, "bias");
  const c10::DeviceGuard g(xd.device());
  TORCH_CHECK(xd.scalar_type() == at::kBFloat16 && W.scalar_type() == at::kBFloat16 && bias.scalar_type() == at::kFloat &&
                  xd.dim() == 2 && W.dim() == 2 && xd.is_contiguous() && W.is_contiguous() && bias.is_contiguous(),
              "fedrec::user_qkv_attention_fwd: contiguous bf16 xd [B*H, Din], bf16 W [3D, Din], fp32 bias [3D]");
  const int64_t D = heads * head_dim, Din = xd.size(1);
  TORCH_CHECK(B > 0 && xd.size(0) % B == 0, "fedrec::user_qkv_attention_fwd: xd rows = B*H");
  const int64_t H = xd.size(0) / B;
  TORCH_CHECK(W.size(0) == 3 * D && W.size(1) == Din && bias.numel() == 3 * D && H >= 1 && H <= 64,
              "fedrec::user_qkv_attention_fwd: W [3D, Din], bias [3D], H <= 64");
  auto opt = xd.options().dtype(at::kFloat);
  auto qkv = at::empty({B, H, 3 * D}, opt);
  auto ctx = at::empty({B, H, D}, opt);
  auto stats = at::empty({B, heads, H, 2}, opt);
  void* cb = nullptr;
  if (ctx_b.has_value()) {
    check_dev(*ctx_b, "ctx_b");
    TORCH_CHECK(ctx_b->scalar_type() == at::kBFloat16 && ctx_b->numel() == ctx.numel() && ctx_b->is_contiguous(),
                "fedrec::user_qkv_attention_fwd: ctx_b bf16 like ctx");
    cb = ctx_b->data_ptr();
  }
  check_rc(fr_user_qkv_attn_fwd(xd.data_ptr(), W.data_ptr(), bias.data_ptr<float>(), (int)Din, qkv.data_ptr<float>(),
                                ctx.data_ptr<float>(), stats.data_ptr<float>(), (int)B, (int)H, (int)heads,
                                (int)head_dim, key_mask_ptr(keep, B, H, "user_qkv_attention_fwd"), cur_stream(), cb),
           "user_qkv_attention_fwd");
  return {ctx, stats, qkv};
}

// The attention backward with the additive pool's input-gradient GEMM fused in (user_attn.hip,
// FD form): dctx = dctx_direct (read, not written) + dpre W1 per head slice; dpre bf16 [B*H, Qd],
// w1t bf16 [D, Qd] (W1^T, the step's cast).  -> dqkv bf16 [B, H, 3D].  H <= 64.
at::Tensor user_attention_bwd_dctx(const at::Tensor& qkv, const at::Tensor& stats, const at::Tensor& dctx,
                                   const at::Tensor& dpre, const at::Tensor& w1t, int64_t heads, int64_t head_dim,
                                   const OptTensor& keep) {
  check_dev(qkv, "qkv");
  check_dev(stats, "stats");
  check_dev(dctx, "dctx");
  check_dev(dpre, "dpre");
  check_dev(w1t, "w1t");
  const c10::DeviceGuard g(qkv.device());
  TORCH_CHECK(qkv.scalar_type() == at::kFloat && qkv.dim() == 3 && qkv.is_contiguous(),
              "fedrec::user_attention_bwd_dctx: fp32 contiguous qkv [B,H,3D]");
  const int64_t B = qkv.size(0), H = qkv.size(1), D = heads * head_dim;
  TORCH_CHECK(qkv.size(2) == 3 * D && H <= 64, "fedrec::user_attention_bwd_dctx: qkv width 3D, H <= 64");
  TORCH_CHECK(stats.scalar_type() == at::kFloat && stats.is_contiguous() && stats.numel() == B * heads * H * 2,
              "fedrec::user_attention_bwd_dctx: stats");
  TORCH_CHECK(dctx.scalar_type() == at::kFloat && dctx.is_contiguous() && dctx.numel() == B * H * D,
              "fedrec::user_attention_bwd_dctx: fp32 contiguous dctx [B,H,D]");
  TORCH_CHECK(dpre.scalar_type() == at::kBFloat16 && w1t.scalar_type() == at::kBFloat16 && dpre.is_contiguous() &&
                  w1t.is_contiguous() && dpre.dim() == 2 && w1t.dim() == 2 && dpre.size(0) == B * H &&
                  w1t.size(0) == D && w1t.size(1) == dpre.size(1),
              "fedrec::user_attention_bwd_dctx: bf16 dpre [B*H, Qd], bf16 w1t [D, Qd]");
  auto out = at::empty({B, H, 3 * D}, qkv.options().dtype(at::kBFloat16));
  check_rc(fr_user_attn_bwd_dctx(qkv.data_ptr<float>(), stats.data_ptr<float>(), dctx.data_ptr<float>(), out.data_ptr(),
                                 dpre.data_ptr(), w1t.data_ptr(), (int)dpre.size(1), (int)B, (int)H, (int)heads,
                                 (int)head_dim, key_mask_ptr(keep, B, H, "user_attention_bwd_dctx"), cur_stream()),
           "user_attention_bwd_dctx");
  return out;
}

// bf16_out: dqkv in bf16 (the input / weight gradient GEMMs' operand)
at::Tensor user_attention_bwd(const at::Tensor& qkv, const at::Tensor& stats, const at::Tensor& dctx, int64_t heads,
                              int64_t head_dim, const OptTensor& keep, bool bf16_out) {
  check_dev(qkv, "qkv");
  check_dev(stats, "stats");
  check_dev(dctx, "dctx");
  const c10::DeviceGuard g(qkv.device());
  const int64_t B = qkv.size(0), H = qkv.size(1);
  auto d = as_f32(dctx);
  const bool bf = bf16_out && H <= 64;  // long histories: converted below
  auto dqkv = at::empty_like(qkv, bf ? qkv.options().dtype(at::kBFloat16) : qkv.options());
  check_rc(fr_user_attn_bwd(qkv.data_ptr<float>(), stats.data_ptr<float>(), d.data_ptr<float>(), dqkv.data_ptr(),
                            (int)B, (int)H, (int)heads, (int)head_dim, key_mask_ptr(keep, B, H, "user_attention_bwd"),
                            cur_stream(), bf ? 1 : 0),
           "user_attention_bwd");
  return bf16_out && !bf ? dqkv.to(at::kBFloat16) : dqkv;
}

// The user side's tail in one launch (csrc/score_ce.hip user_pool_score_kernel): the additive
// pool of ctx [B, T, D] with scores from e [B, T, Q], the candidate scores + CE against rows
// ci of the table, their gradients into dcand_out [B C, D], and (want_bwd) the pool's backward
// for du.  -> (loss, scores, dctx, dpre, dpre_b, da8); an empty loss when the shape is outside
// the kernel's domain (the caller takes the separate kernels).
Tensor6 user_pool_score(const at::Tensor& x, const at::Tensor& e, const at::Tensor& w2, const at::Tensor& b2,
                        const OptTensor& keep, const at::Tensor& table, const at::Tensor& ci, int64_t act,
                        at::Tensor dcand_out, bool want_bwd) {
  for (const at::Tensor* t : {&x, &e, &w2, &b2, &table, &ci}) check_dev(*t, "user_pool_score input");
  check_dev(dcand_out, "dcand_out");
  TORCH_CHECK(x.scalar_type() == at::kFloat && e.scalar_type() == at::kFloat && w2.scalar_type() == at::kFloat &&
                  b2.scalar_type() == at::kFloat && table.scalar_type() == at::kFloat &&
                  ci.scalar_type() == at::kInt && dcand_out.scalar_type() == at::kFloat && x.dim() == 3 &&
                  e.dim() == 3 && table.dim() == 2,
              "fedrec::user_pool_score: fp32 x [B,T,D], e [B,T,Q], table [U,D]; int32 ci");
  const c10::DeviceGuard g(x.device());
  const int64_t B = x.size(0), T = x.size(1), D = x.size(2), Q = e.size(2);
  TORCH_CHECK(e.size(0) == B && e.size(1) == T && w2.numel() == Q && table.size(1) == D && B > 0 &&
                  ci.numel() % B == 0 && dcand_out.numel() == ci.numel() * D,
              "fedrec::user_pool_score: shapes");
  const int64_t C = ci.numel() / B;
  auto fo = x.options();
  auto lossb = at::empty({B + 1}, fo);
  auto loss = lossb.narrow(0, B, 1).squeeze(0);
  auto scores = at::empty({B, C}, fo);
  const int64_t nb = want_bwd ? B : 0;
  auto dctx = at::empty({nb, T, D}, fo);
  auto dpre = at::empty({nb, T, Q}, fo);
  auto dpre_b = at::empty({nb, T, Q}, fo.dtype(at::kBFloat16));
  auto da8 = at::empty({nb * T, 8}, fo);
  const int* kp = nullptr;
  at::Tensor k32;
  if (defined(keep)) {
    k32 = as_i32(*keep);
    TORCH_CHECK(k32.numel() == B * T, "fedrec::user_pool_score: keep [B, T]");
    kp = k32.data_ptr<int>();
  }
  const int rc = fr_user_pool_score(x.contiguous().data_ptr<float>(), e.contiguous().data_ptr<float>(),
                                    w2.contiguous().data_ptr<float>(), b2.data_ptr<float>(), kp, table.data_ptr<float>(),
                                    ci.data_ptr<int>(), (int)B, (int)T, (int)D, (int)Q, (int)C, (int)act,
                                    lossb.data_ptr<float>(), scores.data_ptr<float>(), dcand_out.data_ptr<float>(),
                                    loss.data_ptr<float>(), want_bwd ? dctx.data_ptr<float>() : nullptr,
                                    want_bwd ? dpre.data_ptr<float>() : nullptr,
                                    want_bwd ? dpre_b.data_ptr() : nullptr, want_bwd ? da8.data_ptr<float>() : nullptr,
                                    cur_stream());
  if (rc != 0) return {at::empty({0}, fo), scores, dctx, dpre, dpre_b, da8};
  return {loss, scores, dctx, dpre, dpre_b, da8};
}

// ci (optional): candidates as rows of a table -- cand is then [U, D], candidate (b, c) its row
// ci[b C + c]; dcand_out (optional): a [B C, D] fp32 buffer the candidate gradient is written to
Tensor4 score_ce(const at::Tensor& cand, const at::Tensor& user, int64_t act, const OptTensor& ci,
                 const OptTensor& dcand_out) {
  check_dev(cand, "cand");
  check_dev(user, "user");
  TORCH_CHECK(cand.scalar_type() == at::kFloat && user.scalar_type() == at::kFloat && cand.is_contiguous() &&
                  user.is_contiguous(),
              "fedrec::score_ce: contiguous fp32");
  const c10::DeviceGuard g(cand.device());
  const bool gathered = defined(ci);
  const int64_t B = user.size(0), D = user.size(1);
  int64_t C;
  if (gathered) {
    check_dev(*ci, "ci");
    TORCH_CHECK(cand.dim() == 2 && cand.size(1) == D && ci->scalar_type() == at::kInt && ci->is_contiguous() &&
                    B > 0 && ci->numel() % B == 0,
                "fedrec::score_ce: table [U, D] + int32 ci [B C]");
    C = ci->numel() / B;  // ci values index the table: produced by dedup (in range by construction)
  } else {
    TORCH_CHECK(cand.dim() == 3 && cand.size(0) == B && cand.size(2) == D, "fedrec::score_ce: cand [B, C, D]");
    C = cand.size(1);
  }
  // per-impression losses, then the deterministic colsum (no float atomics: bit-reproducible loss)
  auto lossb = at::empty({std::max<int64_t>(B, 1) + 1}, cand.options());
  auto loss = lossb.narrow(0, B > 0 ? B : 0, 1).squeeze(0);  // 0-d view (view({}) would pick view(ScalarType))
  auto scores = at::empty({B, C}, cand.options());
  at::Tensor dcand;
  if (defined(dcand_out)) {
    check_dev(*dcand_out, "dcand_out");
    TORCH_CHECK(dcand_out->scalar_type() == at::kFloat && dcand_out->is_contiguous() && dcand_out->numel() == B * C * D,
                "fedrec::score_ce: dcand_out fp32 [B C, D]");
    dcand = *dcand_out;
  } else {
    dcand = at::empty({B, C, D}, cand.options());
  }
  auto duser = at::empty_like(user);
  // the batch loss is summed inside the launch by its last block (impression order); the
  // wave-per-impression form leaves it to a deterministic colsum
  auto run = [&](float* loss_total) {
    return fr_score_ce(cand.data_ptr<float>(), user.data_ptr<float>(), lossb.data_ptr<float>(), scores.data_ptr<float>(),
                       dcand.data_ptr<float>(), duser.data_ptr<float>(), (int)B, (int)C, (int)D, (int)act,
                       gathered ? ci->data_ptr<int>() : nullptr, loss_total, cur_stream());
  };
  const int rc = run(loss.data_ptr<float>());
  if (rc == 2) {
    check_rc(run(nullptr), "score_ce");
    const float* xs[1] = {lossb.data_ptr<float>()};
    float* os[1] = {loss.data_ptr<float>()};
    const int ints[4] = {(int)B, 1, 1, 0};
    const long need = fr_colsum_f32(xs, os, ints, 1, nullptr, cur_stream());
    auto part = at::empty({std::max<long>(need, 1)}, cand.options());
    TORCH_CHECK(need >= 0 && fr_colsum_f32(xs, os, ints, 1, part.data_ptr<float>(), cur_stream()) == 0,
                "fedrec::score_ce: loss sum");
  } else {
    check_rc(rc, "score_ce");
  }
  // with dcand_out the gradient lives in the caller's buffer (no output aliasing an input)
  if (defined(dcand_out)) return {loss, scores, at::empty({0}, cand.options()), duser};
  return {loss, scores, dcand, duser};
}

at::Tensor segment_sum_rows(const at::Tensor& rows, const at::Tensor& perm, const at::Tensor& seg_ptr, int64_t num_out,
                            double clip, double noise_std, int64_t seed, int64_t offset, const OptTensor& inv,
                            bool zero_empty, const OptTensor& dev_off) {
  check_dev(rows, "rows");
  check_dev(perm, "perm");
  check_dev(seg_ptr, "seg_ptr");
  TORCH_CHECK(rows.scalar_type() == at::kFloat && perm.scalar_type() == at::kInt && seg_ptr.scalar_type() == at::kInt,
              "fedrec::segment_sum_rows: dtypes");
  TORCH_CHECK(seg_ptr.numel() == num_out + 1, "fedrec::segment_sum_rows: seg_ptr size");
  const c10::DeviceGuard g(rows.device());
  const int64_t D = rows.size(-1);
  // empty segments (padded unique lists of the step graphs) come out as zero rows: the chunked
  // kernel writes them itself (no separate fill launch), the block-per-row form clears first
  auto out = at::empty({num_out, D}, rows.options());
  at::Tensor src = rows;
  const int64_t R = perm.numel();
  auto scratch = at::empty({(int64_t)fr_segsum_chunks((int)R) * 2 * D}, rows.options());
  const int* invp = nullptr;
  if (defined(inv)) {
    check_dev(*inv, "inv");
    TORCH_CHECK(inv->scalar_type() == at::kInt && inv->numel() == R, "fedrec::segment_sum_rows: inv int32[R]");
    invp = inv->data_ptr<int>();
  }
  if (clip > 0.0 || noise_std > 0.0) {  // LDP: clip + noise every occurrence
    const unsigned long long* dop = nullptr;
    if (defined(dev_off)) {  // device step counter (graph replays: fresh noise)
      check_dev(*dev_off, "dev_off");
      TORCH_CHECK(dev_off->scalar_type() == at::kLong && dev_off->numel() == 1, "fedrec::segment_sum_rows: dev_off int64[1]");
      dop = (const unsigned long long*)dev_off->data_ptr();
    }
    TORCH_CHECK(rows.numel() / D == R, "fedrec::segment_sum_rows: rows / perm sizes");
    // fused into the chunk pass when the layout allows (K16 + K17 in one launch)
    if (fr_segment_sum_rows_ldp(rows.data_ptr<float>(), perm.data_ptr<int>(), seg_ptr.data_ptr<int>(), invp,
                                out.data_ptr<float>(), (int)num_out, (int)D, (int)R, scratch.data_ptr<float>(),
                                (float)clip, (float)noise_std, (unsigned long long)seed, (unsigned long long)offset, dop,
                                cur_stream()) == 0)
      return out;
    src = at::empty_like(rows);  // the parallel clip + noise pass first, then the plain sum
    check_rc(fr_ldp_rows(rows.data_ptr<float>(), src.data_ptr<float>(), (int)(rows.numel() / D), (int)D, (float)clip,
                         (float)noise_std, (unsigned long long)seed, (unsigned long long)offset, cur_stream(), dop),
             "ldp_rows");
  }
  check_rc(fr_segment_sum_rows(src.data_ptr<float>(), perm.data_ptr<int>(), seg_ptr.data_ptr<int>(), invp,
                               out.data_ptr<float>(), (int)num_out, (int)D, (int)R, scratch.data_ptr<float>(),
                               cur_stream(), zero_empty ? 1 : 0),
           "segment_sum_rows");
  return out;
}

// ---- small GEMMs on MFMA (small_gemm.hip): up to 6 independent GEMMs per launch ------------
// ints: 14 per GEMM (M, N, K, lda, ldb, ldc, a_mode, b_mode, act, accumulate, drop_ld, drop_on, gather_on, kseg);
// A / B fp32 or bf16 (the kernel takes the dtype flags from the tensors), C fp32;
// tile: 0 = the launcher's choice, 1..4 = 64x64 / 128x64 / 64x128 / 128x128 (benchmarks);
// Bseg: per GEMM 0 or 2 extra [kseg, N] row blocks of a K-segmented B (kseg > 0)
// floats: (alpha, pdrop) per GEMM; seeds: (seed, offset) per GEMM.  C tensors are written.
// elements addressable from t.data_ptr() to the end of its storage (strided operand views)
int64_t avail(const at::Tensor& t) {
  return (int64_t)(t.storage().nbytes() / t.element_size()) - t.storage_offset();
}

void small_gemm(const std::vector<at::Tensor>& A, const c10::List<OptTensor>& gidx, const std::vector<at::Tensor>& B,
                const c10::List<OptTensor>& bias, const std::vector<at::Tensor>& C, at::IntArrayRef ints,
                at::ArrayRef<double> floats, at::IntArrayRef seeds, const OptTensor& dev_off,
                const std::vector<at::Tensor>& Bseg, int64_t tile, const c10::List<OptTensor>& asum) {
  const size_t n = A.size();
  TORCH_CHECK(n >= 1 && n <= 6 && B.size() == n && C.size() == n && gidx.size() == n && bias.size() == n &&
                  asum.size() == n &&
                  ints.size() == 14 * n && floats.size() == 2 * n && seeds.size() == 2 * n,
              "fedrec::small_gemm: descriptor sizes");
  const c10::DeviceGuard g(A[0].device());
  std::vector<const void*> ptrs(8 * n);
  std::vector<int> iv(16 * n);
  size_t seg_used = 0;
  std::vector<float> fv(2 * n);
  std::vector<unsigned long long> sv(2 * n);
  for (size_t i = 0; i < n; ++i) {
    const int64_t* q = ints.data() + 14 * i;
    const int64_t M = q[0], N = q[1], K = q[2], lda = q[3], ldb = q[4], ldc = q[5], am = q[6], bm = q[7];
    for (const at::Tensor* t : {&A[i], &B[i], &C[i]}) {  // row-major views with any leading dimension
      TORCH_CHECK(t->is_cuda() && (t->scalar_type() == at::kFloat || (t != &C[i] && t->scalar_type() == at::kBFloat16)) &&
                      (t->dim() == 0 || t->stride(-1) == 1),
                  "fedrec::small_gemm: fp32 / bf16 device operands (fp32 C) with unit inner stride");
    }
    // bounds of the strided accesses the kernel makes (a kernel never sees a shape it was not written for)
    const auto gv = gidx.get(i);
    const bool gathered = defined(gv);
    const int64_t gather_on = q[12];
    // a gathered operand's rows are gidx values (checked in range by the producer: dedup)
    if (!(gathered && gather_on == 1))
      TORCH_CHECK(avail(A[i]) >= (am == 0 ? (M - 1) * lda + K : (K - 1) * lda + M) || M == 0 || K == 0,
                  "fedrec::small_gemm: A too small");
    const int64_t kseg = q[13];
    const int64_t b_rows = kseg > 0 ? std::min<int64_t>(K, kseg) : K;
    if (!(gathered && gather_on == 2))
      TORCH_CHECK(avail(B[i]) >= (bm == 0 ? (N - 1) * ldb + K : (b_rows - 1) * ldb + N) || N == 0 || K == 0,
                  "fedrec::small_gemm: B too small");
    TORCH_CHECK(gathered == (gather_on != 0), "fedrec::small_gemm: gidx given iff gather_on");
    TORCH_CHECK(avail(C[i]) >= (M - 1) * ldc + N || M == 0 || N == 0, "fedrec::small_gemm: C too small");
    ptrs[8 * i + 0] = A[i].data_ptr();
    ptrs[8 * i + 1] = nullptr;
    ptrs[8 * i + 5] = ptrs[8 * i + 6] = nullptr;
    if (kseg > 0) {  // the extra row blocks of a K-segmented B come from Bseg in order
      TORCH_CHECK(bm == 1 && seg_used + 2 <= Bseg.size(), "fedrec::small_gemm: K-segmented B needs b_mode 1 + 2 Bseg");
      for (int j = 0; j < 2; ++j) {
        const at::Tensor& t = Bseg[seg_used + j];
        TORCH_CHECK(t.is_cuda() && t.scalar_type() == B[i].scalar_type() && t.stride(-1) == 1 &&
                        avail(t) >= (kseg - 1) * ldb + N,
                    "fedrec::small_gemm: Bseg block");
        ptrs[8 * i + 5 + j] = t.data_ptr();
      }
      seg_used += 2;
    }
    if (gathered) {
      TORCH_CHECK(gv->is_cuda() && gv->scalar_type() == at::kInt && gv->numel() >= (gather_on == 1 ? M : K),
                  "fedrec::small_gemm: gidx int32[M] (A rows) or int32[K] (B rows)");
      ptrs[8 * i + 1] = gv->data_ptr();
    }
    ptrs[8 * i + 2] = B[i].data_ptr();
    const auto bv = bias.get(i);
    ptrs[8 * i + 3] = nullptr;
    if (defined(bv)) {
      TORCH_CHECK(bv->is_cuda() && bv->scalar_type() == at::kFloat && bv->numel() >= N, "fedrec::small_gemm: bias");
      ptrs[8 * i + 3] = bv->data_ptr();
    }
    ptrs[8 * i + 4] = C[i].data_ptr();
    ptrs[8 * i + 7] = nullptr;
    const auto av = asum.get(i);
    if (defined(av)) {  // column sums of A (a_mode 1): fp32 [M], contiguous
      TORCH_CHECK(av->is_cuda() && av->scalar_type() == at::kFloat && av->is_contiguous() && av->numel() >= M &&
                      am == 1,
                  "fedrec::small_gemm: asum fp32 [M] (a_mode 1)");
      ptrs[8 * i + 7] = av->data_ptr();
    }
    for (int j = 0; j < 14; ++j) iv[16 * i + j] = (int)q[j];
    iv[16 * i + 14] = A[i].scalar_type() == at::kBFloat16;
    iv[16 * i + 15] = B[i].scalar_type() == at::kBFloat16;
    fv[2 * i] = (float)floats[2 * i];
    fv[2 * i + 1] = (float)floats[2 * i + 1];
    sv[2 * i] = (unsigned long long)seeds[2 * i];
    sv[2 * i + 1] = (unsigned long long)seeds[2 * i + 1];
  }
  const unsigned long long* dop = nullptr;
  if (defined(dev_off)) {  // int64 device counter added to every dropout offset
    TORCH_CHECK(dev_off->is_cuda() && dev_off->scalar_type() == at::kLong && dev_off->numel() >= 1,
                "fedrec::small_gemm: dev_off int64[1]");
    dop = (const unsigned long long*)dev_off->data_ptr<int64_t>();
  }
  // first call: validate + ask for split-K partial space; second call: launch
  auto run = [&](float* scratch) {
    return fr_small_gemm(ptrs.data(), iv.data(), fv.data(), sv.data(), dop, (int)n, scratch, (int)tile, cur_stream());
  };
  const long need = run(nullptr);
  TORCH_CHECK(need >= 0, "fedrec::small_gemm: descriptor rejected (code ", need, ")");
  if (need > 0) {
    auto scratch = at::empty({need}, A[0].options().dtype(at::kFloat));
    const long rc = run(scratch.data_ptr<float>());
    TORCH_CHECK(rc == 0, "fedrec::small_gemm: launch failed (code ", rc, ")");
    if (fr_small_gemm_has_pending() && !fedrec::g_sg_pending_scratch.defined()) fedrec::g_sg_pending_scratch = scratch;
  }
}

// deferred split-K reductions (ops.functional.deferred_reduces): the next small-GEMM launch whose
// split descs are all weight gradients leaves its reduction to the text head's reduce launch
bool small_gemm_flush_pending() {
  const bool had = fr_small_gemm_flush_pending(cur_stream()) != 0;
  fedrec::g_sg_pending_scratch = at::Tensor();
  return had;
}

// column sums of fp32 matrices [M, N] (row stride ld) into out[N] (accumulate: out += sums)
void colsum_f32(const std::vector<at::Tensor>& X, const std::vector<at::Tensor>& out, at::IntArrayRef ints) {
  const size_t n = X.size();
  TORCH_CHECK(n >= 1 && n <= 6 && out.size() == n && ints.size() == 4 * n, "fedrec::colsum_f32: sizes");
  const c10::DeviceGuard g(X[0].device());
  std::vector<const float*> xs(n);
  std::vector<float*> os(n);
  std::vector<int> iv(4 * n);
  for (size_t i = 0; i < n; ++i) {
    TORCH_CHECK(X[i].is_cuda() && X[i].scalar_type() == at::kFloat && out[i].is_cuda() &&
                    out[i].scalar_type() == at::kFloat && (X[i].dim() == 0 || X[i].stride(-1) == 1) &&
                    (out[i].dim() == 0 || out[i].stride(-1) == 1),
                "fedrec::colsum_f32: fp32 device");
    const int64_t M = ints[4 * i], N = ints[4 * i + 1], ld = ints[4 * i + 2];
    TORCH_CHECK(avail(out[i]) >= N && (M == 0 || avail(X[i]) >= (M - 1) * ld + N), "fedrec::colsum_f32: shapes");
    xs[i] = X[i].data_ptr<float>();
    os[i] = out[i].data_ptr<float>();
    for (int j = 0; j < 4; ++j) iv[4 * i + j] = (int)ints[4 * i + j];
  }
  const long need = fr_colsum_f32(xs.data(), os.data(), iv.data(), (int)n, nullptr, cur_stream());
  TORCH_CHECK(need >= 0, "fedrec::colsum_f32: descriptor rejected");
  auto part = at::empty({std::max<long>(need, 1)}, X[0].options());
  TORCH_CHECK(fr_colsum_f32(xs.data(), os.data(), iv.data(), (int)n, part.data_ptr<float>(), cur_stream()) == 0,
              "fedrec::colsum_f32: launch failed");
}

// out[m] = v[idx[m]] * Philox dropout mask (small_gemm.hip), fp32 or bf16 (bf16_out)
at::Tensor gather_dropout(const at::Tensor& v, const at::Tensor& idx, double p, int64_t seed, int64_t offset,
                          const OptTensor& dev_off, bool bf16_out) {
  check_dev(v, "v");
  check_dev(idx, "idx");
  TORCH_CHECK(v.scalar_type() == at::kFloat && v.dim() == 2 && idx.scalar_type() == at::kInt && idx.dim() == 1,
              "fedrec::gather_dropout: fp32 v [U, K], int32 idx [M]");
  TORCH_CHECK(v.size(1) % 4 == 0, "fedrec::gather_dropout: K % 4");
  const c10::DeviceGuard g(v.device());
  const unsigned long long* dp = nullptr;
  if (defined(dev_off)) {
    check_dev(*dev_off, "dev_off");
    TORCH_CHECK(dev_off->scalar_type() == at::kLong && dev_off->numel() >= 1, "fedrec::gather_dropout: dev_off");
    dp = (const unsigned long long*)dev_off->data_ptr<int64_t>();
  }
  auto out = at::empty({idx.size(0), v.size(1)}, v.options().dtype(bf16_out ? at::kBFloat16 : at::kFloat));
  check_rc(fr_gather_dropout(v.data_ptr<float>(), idx.data_ptr<int>(), out.data_ptr(), bf16_out ? 1 : 0,
                             (int)idx.size(0), (int)v.size(1), (float)p, (unsigned long long)seed,
                             (unsigned long long)offset, dp, cur_stream()),
           "gather_dropout");
  return out;
}

}  // namespace

TORCH_LIBRARY_FRAGMENT(fedrec, m) {
  m.def("score_set_variant(int v) -> ()", [](int64_t v) { fr_score_set_variant((int)v); });
  m.def("segsum_set_variant(int v) -> ()", [](int64_t v) { fr_segsum_set_variant((int)v); });
  m.def("segsum_set_ldp_block(int v) -> ()", [](int64_t v) { fr_segsum_set_ldp_block((int)v); });
  m.def("small_gemm_set_rd(int v) -> ()", [](int64_t v) { fr_small_gemm_set_rd((int)v); });
  m.def("small_gemm_set_defer(bool on) -> ()", [](bool on) { fr_small_gemm_set_defer(on ? 1 : 0); });
  m.def("small_gemm_flush_pending() -> bool", &small_gemm_flush_pending);
  m.def("user_attention_fwd(Tensor qkv, int heads, int head_dim, Tensor? keep=None, Tensor(a!)? ctx_b=None) -> (Tensor, Tensor)", on_gpu(&user_attention_fwd));
  m.def("user_qkv_attention_fwd(Tensor xd, Tensor W, Tensor bias, int B, int heads, int head_dim, Tensor? keep=None, "
        "Tensor(a!)? ctx_b=None) -> (Tensor, Tensor, Tensor)", on_gpu(&user_qkv_attention_fwd));
  m.def("user_attention_bwd_dctx(Tensor qkv, Tensor stats, Tensor dctx, Tensor dpre, Tensor w1t, int heads, "
        "int head_dim, Tensor? keep=None) -> Tensor", on_gpu(&user_attention_bwd_dctx));
  m.def("user_attention_bwd(Tensor qkv, Tensor stats, Tensor dctx, int heads, int head_dim, Tensor? keep=None, bool bf16_out=False) -> Tensor", on_gpu(&user_attention_bwd));
  m.def("user_pool_score(Tensor x, Tensor e, Tensor w2, Tensor b2, Tensor? keep, Tensor table, Tensor ci, int act, Tensor(a!) dcand_out, bool want_bwd) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)", on_gpu(&user_pool_score));
  m.def("score_ce(Tensor cand, Tensor user, int act, Tensor? ci=None, Tensor(a!)? dcand_out=None) -> (Tensor, Tensor, Tensor, Tensor)", on_gpu(&score_ce));
  m.def("segment_sum_rows(Tensor rows, Tensor perm, Tensor seg_ptr, int num_out, float clip, float noise_std, int seed, int offset, Tensor? inv=None, bool zero_empty=False, Tensor? dev_off=None) -> Tensor", on_gpu(&segment_sum_rows));
  m.def("small_gemm(Tensor[] A, Tensor?[] gidx, Tensor[] B, Tensor?[] bias, Tensor(a!)[] C, int[] ints, float[] floats, int[] seeds, Tensor? dev_off, Tensor[] Bseg, int tile, Tensor?[] asum) -> ()", on_gpu(&small_gemm));
  m.def("colsum_f32(Tensor[] X, Tensor(a!)[] out, int[] ints) -> ()", on_gpu(&colsum_f32));
  m.def("gather_dropout(Tensor v, Tensor idx, float p, int seed, int offset, Tensor? dev_off, bool bf16_out=False) -> Tensor", on_gpu(&gather_dropout));
}
