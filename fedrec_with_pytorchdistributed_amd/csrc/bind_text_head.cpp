// fedrec ops of the fused text head over gathered hidden states (text_head.hip) and of the
// additive-attention pooling (additive_pool.hip).
#include "binding_util.h"

namespace {

// table [rows, D] bf16 (the HBM hidden-state cache viewed as rows, or a batch's hidden states);
// ids [U] int32 title indices (None: titles 0..U-1 of the table); T tokens per title.
int64_t head_titles(const at::Tensor& table, const OptTensor& ids, int64_t T) {
  check_dev(table, "table");
  TORCH_CHECK(table.dim() == 2 && table.is_contiguous() && table.scalar_type() == at::kBFloat16,
              "fedrec::head: table [rows, D] contiguous bf16");
  TORCH_CHECK(T >= 1 && table.size(0) % T == 0, "fedrec::head: table rows not a multiple of T");
  if (ids.has_value()) {
    check_dev(*ids, "ids");
    TORCH_CHECK(ids->dim() == 1 && ids->is_contiguous() && ids->scalar_type() == at::kInt, "fedrec::head: ids int32 [U]");
    return ids->size(0);
  }
  return table.size(0) / T;
}

Tensor2 head_score(const at::Tensor& table, const OptTensor& ids, int64_t T, const at::Tensor& w1, const at::Tensor& b1,
                   const at::Tensor& w2, const at::Tensor& b2, bool store_e, const OptTensor& nreal) {
  const int64_t U = head_titles(table, ids, T), D = table.size(1), Q = w1.size(0);
  check_dev(w1, "w1");
  TORCH_CHECK(w1.scalar_type() == at::kBFloat16 && w1.is_contiguous() && w1.size(1) == D, "fedrec::head_score: w1 bf16 [Q, D]");
  TORCH_CHECK(b1.scalar_type() == at::kFloat && w2.scalar_type() == at::kFloat && b2.scalar_type() == at::kFloat &&
                  b1.numel() == Q && w2.numel() == Q && b2.numel() == 1 && b1.is_contiguous() && w2.is_contiguous() &&
                  b1.is_cuda() && w2.is_cuda() && b2.is_cuda(),
              "fedrec::head_score: b1 / w2 [Q], b2 [1] fp32 device");
  TORCH_CHECK(fr_head_supported((int)D, (int)Q, (int)T), "fedrec::head_score: unsupported shape D=", D, " Q=", Q, " T=", T);
  // (ids are not range-checked here: that needs a device->host read every step; the engine's
  // ids come from the dedup over [0, N) by construction)
  const c10::DeviceGuard g(table.device());
  auto e = store_e ? at::empty({U * T, Q}, table.options()) : at::empty({0}, table.options());
  auto a = at::empty({U * T}, table.options().dtype(at::kFloat));
  check_rc(fr_head_score(table.data_ptr(), opt_int_ptr(ids), (int)U, (int)T, (int)D, (int)Q, w1.data_ptr(),
                         b1.data_ptr<float>(), w2.data_ptr<float>(), b2.data_ptr<float>(),
                         store_e ? e.data_ptr() : nullptr, a.data_ptr<float>(), opt_nreal(nreal, table), cur_stream()),
           "head_score");
  return {e, a};
}

// want_bf16: also the pooled rows rounded to bf16 (the fc GEMM's operand; empty otherwise)
Tensor3 head_pool(const at::Tensor& table, const OptTensor& ids, int64_t T, const at::Tensor& a, const OptTensor& tokens,
                  const OptTensor& nreal, bool want_bf16) {
  const int64_t U = head_titles(table, ids, T), D = table.size(1);
  check_dev(a, "a");
  TORCH_CHECK(a.scalar_type() == at::kFloat && a.numel() == U * T && a.is_contiguous(), "fedrec::head_pool: a [U*T] fp32");
  if (tokens.has_value()) {
    check_dev(*tokens, "tokens");
    TORCH_CHECK(tokens->scalar_type() == at::kInt && tokens->dim() == 3 && tokens->size(1) == 2 &&
                    tokens->size(2) == T && tokens->is_contiguous() && tokens->size(0) * T >= table.size(0),
                "fedrec::head_pool: tokens int32 [N, 2, T] covering the table");
  }
  const c10::DeviceGuard g(table.device());
  auto pooled = at::empty({U, D}, a.options());
  auto alpha = at::empty({U, T}, a.options());
  auto pooled_b = at::empty({want_bf16 ? U : 0, D}, a.options().dtype(at::kBFloat16));
  check_rc(fr_head_pool(table.data_ptr(), opt_int_ptr(ids), a.data_ptr<float>(), opt_int_ptr(tokens), (int)U, (int)T,
                        (int)D, pooled.data_ptr<float>(), alpha.data_ptr<float>(), opt_nreal(nreal, table), cur_stream(),
                        want_bf16 ? pooled_b.data_ptr() : nullptr),
           "head_pool");
  return {pooled, alpha, pooled_b};
}

Tensor2 head_pool_bwd(const at::Tensor& table, const OptTensor& ids, int64_t T, const at::Tensor& alpha,
                      const at::Tensor& g, const OptTensor& nreal) {
  const int64_t U = head_titles(table, ids, T), D = table.size(1);
  check_dev(alpha, "alpha");
  check_dev(g, "g");
  TORCH_CHECK(alpha.scalar_type() == at::kFloat && alpha.numel() == U * T && alpha.is_contiguous() &&
                  g.scalar_type() == at::kFloat && g.numel() == U * D && g.is_contiguous(),
              "fedrec::head_pool_bwd: alpha [U, T], g [U, D] fp32");
  const c10::DeviceGuard dg(table.device());
  auto da = at::empty({U * T}, alpha.options());
  auto db2p = at::empty({std::max<int64_t>(U, 1)}, alpha.options());
  check_rc(fr_head_pool_bwd(table.data_ptr(), opt_int_ptr(ids), alpha.data_ptr<float>(), g.data_ptr<float>(), (int)U,
                            (int)T, (int)D, da.data_ptr<float>(), db2p.data_ptr<float>(), opt_nreal(nreal, table),
                            cur_stream()),
           "head_pool_bwd");
  return {da, db2p};
}

Tensor4 head_wgrad(const at::Tensor& table, const OptTensor& ids, int64_t T, const at::Tensor& e, const at::Tensor& da,
                   const at::Tensor& w2, const at::Tensor& db2p, const OptTensor& nreal) {
  const int64_t U = head_titles(table, ids, T), D = table.size(1), Q = w2.numel();
  check_dev(e, "e");
  check_dev(da, "da");
  check_dev(w2, "w2");
  check_dev(db2p, "db2p");
  TORCH_CHECK(e.scalar_type() == at::kBFloat16 && e.is_contiguous() && e.numel() == U * T * Q,
              "fedrec::head_wgrad: e bf16 [U*T, Q]");
  TORCH_CHECK(da.scalar_type() == at::kFloat && da.numel() == U * T && w2.scalar_type() == at::kFloat &&
                  w2.is_contiguous() && db2p.scalar_type() == at::kFloat && db2p.numel() >= U,
              "fedrec::head_wgrad: da / w2 / db2p");
  TORCH_CHECK(fr_head_supported((int)D, (int)Q, (int)T), "fedrec::head_wgrad: unsupported shape");
  const c10::DeviceGuard g(table.device());
  auto fopt = da.options();
  auto dW1 = at::empty({Q, D}, fopt);
  auto small = at::empty({2 * Q + 1}, fopt);
  float* db1 = small.data_ptr<float>();
  float* dw2 = db1 + Q;
  float* db2 = dw2 + Q;
  auto run = [&](float* scratch, const int* nr) {  // scratch null: the query pass (floats of scratch needed)
    return fr_head_wgrad(e.data_ptr(), table.data_ptr(), opt_int_ptr(ids), da.data_ptr<float>(), db2p.data_ptr<float>(),
                         w2.data_ptr<float>(), (int)U, (int)T, (int)D, (int)Q, dW1.data_ptr<float>(), db1, dw2, db2,
                         scratch, nr, cur_stream());
  };
  const long need = run(nullptr, nullptr);
  TORCH_CHECK(need > 0, "fedrec::head_wgrad: unsupported shape");
  auto scratch = at::empty({need}, fopt);
  check_rc((int)run(scratch.data_ptr<float>(), opt_nreal(nreal, table)), "head_wgrad");
  return {dW1, small.narrow(0, 0, Q), small.narrow(0, Q, Q), small.narrow(0, 2 * Q, 1)};
}

// the G path: the pool backward also rewrites e (bf16 [U*T, Q], in place) into g = da (1 - e^2)
// and writes the per-title column partials cs [2, U, Q]; the weight gradient is then a plain
// TN GEMM over g (head_wgrad_g).  Q = 384 only (head_g_supported).
Tensor3 head_pool_bwd_g(const at::Tensor& table, const OptTensor& ids, int64_t T, const at::Tensor& alpha,
                        const at::Tensor& g, at::Tensor e, const OptTensor& nreal) {
  const int64_t U = head_titles(table, ids, T), D = table.size(1);
  check_dev(alpha, "alpha");
  check_dev(g, "g");
  check_dev(e, "e");
  TORCH_CHECK(alpha.scalar_type() == at::kFloat && alpha.numel() == U * T && alpha.is_contiguous() &&
                  g.scalar_type() == at::kFloat && g.numel() == U * D && g.is_contiguous(),
              "fedrec::head_pool_bwd_g: alpha [U, T], g [U, D] fp32");
  TORCH_CHECK(e.scalar_type() == at::kBFloat16 && e.is_contiguous() && U > 0 && e.numel() % (U * T) == 0,
              "fedrec::head_pool_bwd_g: e bf16 [U*T, Q]");
  const int64_t Q = U > 0 ? e.numel() / (U * T) : 0;
  TORCH_CHECK(fr_head_g_supported((int)D, (int)Q, (int)T), "fedrec::head_pool_bwd_g: unsupported shape");
  const c10::DeviceGuard dg(table.device());
  auto da = at::empty({U * T}, alpha.options());
  auto db2p = at::empty({std::max<int64_t>(U, 1)}, alpha.options());
  auto cs = at::empty({2, U, Q}, alpha.options());
  check_rc(fr_head_pool_bwd_g(table.data_ptr(), opt_int_ptr(ids), alpha.data_ptr<float>(), g.data_ptr<float>(),
                              (int)U, (int)T, (int)D, (int)Q, da.data_ptr<float>(), db2p.data_ptr<float>(),
                              e.data_ptr(), cs.data_ptr<float>(), opt_nreal(nreal, table), cur_stream()),
           "head_pool_bwd_g");
  return {da, db2p, cs};
}

Tensor4 head_wgrad_g(const at::Tensor& table, const OptTensor& ids, int64_t T, const at::Tensor& G, const at::Tensor& cs,
                     const at::Tensor& w2, const at::Tensor& db2p, const OptTensor& nreal,
                     const c10::optional<std::vector<at::Tensor>>& out) {
  const int64_t U = head_titles(table, ids, T), D = table.size(1), Q = w2.numel();
  check_dev(G, "G");
  check_dev(cs, "cs");
  check_dev(w2, "w2");
  check_dev(db2p, "db2p");
  TORCH_CHECK(G.scalar_type() == at::kBFloat16 && G.is_contiguous() && G.numel() == U * T * Q,
              "fedrec::head_wgrad_g: G bf16 [U*T, Q]");
  TORCH_CHECK(cs.scalar_type() == at::kFloat && cs.is_contiguous() && cs.numel() == 2 * U * Q &&
                  w2.scalar_type() == at::kFloat && w2.is_contiguous() && db2p.scalar_type() == at::kFloat &&
                  db2p.numel() >= U,
              "fedrec::head_wgrad_g: cs [2, U, Q] / w2 / db2p");
  TORCH_CHECK(fr_head_g_supported((int)D, (int)Q, (int)T), "fedrec::head_wgrad_g: unsupported shape");
  const c10::DeviceGuard g(table.device());
  auto fopt = cs.options();
  at::Tensor dW1, small, o_db1, o_dw2, o_db2;
  float *db1, *dw2, *db2;
  if (out.has_value()) {  // the destinations given (the flat gradient buffer's slots): dW1, db1, dw2, db2
    TORCH_CHECK(out->size() == 4, "fedrec::head_wgrad_g: out = [dW1, db1, dw2, db2]");
    const int64_t sizes[4] = {Q * D, Q, Q, 1};
    for (int i = 0; i < 4; ++i) {
      const auto& t = (*out)[i];
      check_dev(t, "head_wgrad_g out");
      TORCH_CHECK(t.scalar_type() == at::kFloat && t.is_contiguous() && t.numel() == sizes[i] &&
                      t.device() == table.device() && (i > 0 || ((uintptr_t)t.data_ptr() & 15) == 0),
                  "fedrec::head_wgrad_g: out tensors fp32 contiguous [Q, D] / [Q] / [Q] / [1]");
    }
    dW1 = (*out)[0];
    o_db1 = (*out)[1];
    o_dw2 = (*out)[2];
    o_db2 = (*out)[3];
    db1 = o_db1.data_ptr<float>();
    dw2 = o_dw2.data_ptr<float>();
    db2 = o_db2.data_ptr<float>();
  } else {
    dW1 = at::empty({Q, D}, fopt);
    small = at::empty({2 * Q + 1}, fopt);
    db1 = small.data_ptr<float>();
    dw2 = db1 + Q;
    db2 = dw2 + Q;
    o_db1 = small.narrow(0, 0, Q);
    o_dw2 = small.narrow(0, Q, Q);
    o_db2 = small.narrow(0, 2 * Q, 1);
  }
  auto run = [&](float* scratch, const int* nr, const void* pend, int pc, int pt) {  // scratch null: the query pass
    return fr_head_wgrad_g(G.data_ptr(), table.data_ptr(), opt_int_ptr(ids), cs.data_ptr<float>(), db2p.data_ptr<float>(),
                           w2.data_ptr<float>(), (int)U, (int)T, (int)D, (int)Q, dW1.data_ptr<float>(), db1, dw2, db2,
                           scratch, nr, cur_stream(), pend, pc, pt);
  };
  const long need = run(nullptr, nullptr, nullptr, 0, 0);
  TORCH_CHECK(need > 0, "fedrec::head_wgrad_g: unsupported shape");
  auto scratch = at::empty({need}, fopt);
  // a deferred small-GEMM split-K reduction (the text FC backward's weight gradients) rides in
  // the reduce launch; its partials stay alive until that launch is enqueued
  std::vector<unsigned char> pend((size_t)fr_small_gemm_batch_bytes());
  int pc = 0, pt = 0;
  const bool has_pend = fr_small_gemm_take_pending(pend.data(), (int)pend.size(), &pc, &pt) != 0;
  check_rc((int)run(scratch.data_ptr<float>(), opt_nreal(nreal, table), has_pend ? pend.data() : nullptr, pc, pt),
           "head_wgrad_g");
  if (has_pend) fedrec::g_sg_pending_scratch = at::Tensor();
  return {dW1, o_db1, o_dw2, o_db2};
}

// ---- additive-attention pooling (additive_pool.hip) --------------------------------------------
// x [n, T, D], e [n, T, Q] of one dtype (bf16 or fp32), w2 [Q] fp32: the kernels index all three by
// x's n, T and e's Q, so a mismatch reads out of bounds.  One message per rule; the device checks
// come after every shape check (they do not depend on the shapes)
void pool_args(const char* op, const at::Tensor& x, const at::Tensor& e, const at::Tensor& w2) {
  TORCH_CHECK(x.dim() == 3 && e.dim() == 3 && x.scalar_type() == e.scalar_type() &&
                  (x.scalar_type() == at::kBFloat16 || x.scalar_type() == at::kFloat),
              op, ": x [n, T, D] and e [n, T, Q] of one dtype, bf16 or fp32");
  TORCH_CHECK(e.size(0) == x.size(0) && e.size(1) == x.size(1), op, ": e must share x's [n, T] (got e [", e.size(0),
              ", ", e.size(1), "], x [", x.size(0), ", ", x.size(1), "])");
  TORCH_CHECK(w2.scalar_type() == at::kFloat && w2.is_contiguous() && w2.numel() == e.size(2), op,
              ": w2 must be contiguous fp32 of Q = ", e.size(2), " elements (got ", w2.numel(), ")");
  TORCH_CHECK(x.is_contiguous() && e.is_contiguous(), op, ": x and e must be contiguous");
}

Tensor2 additive_pool_fwd(const at::Tensor& x, const at::Tensor& e, const at::Tensor& w2, const at::Tensor& b2,
                          const OptTensor& keep) {
  const char* op = "fedrec::additive_pool_fwd";
  pool_args(op, x, e, w2);
  TORCH_CHECK(b2.scalar_type() == at::kFloat && b2.numel() == 1, op, ": b2 must be fp32 of one element");
  TORCH_CHECK(x.is_cuda() && e.is_cuda() && w2.is_cuda() && b2.is_cuda(), op, ": x, e, w2 and b2 must be device tensors");
  const c10::DeviceGuard g(x.device());
  const int64_t n = x.size(0), T = x.size(1), D = x.size(2), Q = e.size(2);
  const bool bf = x.scalar_type() == at::kBFloat16;
  auto out = at::empty({n, D}, x.options().dtype(at::kFloat));
  auto alpha = at::empty({n, T}, x.options().dtype(at::kFloat));
  check_rc(fr_additive_pool_fwd(x.data_ptr(), e.data_ptr(), w2.data_ptr<float>(), b2.data_ptr<float>(),
                                out.data_ptr<float>(), alpha.data_ptr<float>(), (int)n, (int)T, (int)D, (int)Q, bf,
                                key_mask_ptr(keep, n, T, "additive_pool_fwd"), cur_stream()),
           "additive_pool_fwd");
  return {out, alpha};
}

Tensor5 additive_pool_bwd(const at::Tensor& x, const at::Tensor& e, const at::Tensor& alpha, const at::Tensor& w2,
                          const at::Tensor& g, bool want_dx) {
  const char* op = "fedrec::additive_pool_bwd";
  pool_args(op, x, e, w2);
  const int64_t n = x.size(0), T = x.size(1), D = x.size(2), Q = e.size(2);
  TORCH_CHECK(alpha.scalar_type() == at::kFloat && alpha.dim() == 2 && alpha.size(0) == n && alpha.size(1) == T &&
                  alpha.is_contiguous(),
              op, ": alpha must be contiguous fp32 [n, T] = [", n, ", ", T, "]");
  TORCH_CHECK(g.scalar_type() == at::kFloat && g.dim() == 2 && g.size(0) == n && g.size(1) == D && g.is_contiguous(), op,
              ": g must be contiguous fp32 [n, D] = [", n, ", ", D, "]");
  TORCH_CHECK(x.is_cuda() && e.is_cuda() && alpha.is_cuda() && w2.is_cuda() && g.is_cuda(), op,
              ": x, e, alpha, w2 and g must be device tensors");
  const c10::DeviceGuard dg(x.device());
  const bool bf = x.scalar_type() == at::kBFloat16;
  auto fopt = x.options().dtype(at::kFloat);
  at::Tensor dx = want_dx ? at::empty({n, T, D}, fopt) : at::empty({0}, fopt);
  auto dpre = at::empty({n, T, Q}, e.options());
  // partial rows, one per block (no float atomics)
  const int64_t R = std::max<int64_t>(1, n * fr_additive_pool_rows((int)T, (int)D, (int)Q, bf ? 1 : 0));
  auto red = at::empty({2 * R * Q + R}, fopt);  // [dw2 rows | dpre col-sum rows | db2 rows]
  float* dw2p = red.data_ptr<float>();
  float* dsump = dw2p + R * Q;
  float* db2p = dsump + R * Q;
  const int rc = fr_additive_pool_bwd(x.data_ptr(), e.data_ptr(), alpha.data_ptr<float>(), w2.data_ptr<float>(),
                                      g.data_ptr<float>(), want_dx ? dx.data_ptr<float>() : nullptr, dpre.data_ptr(),
                                      dw2p, db2p, dsump, (int)n, (int)T, (int)D, (int)Q, (int)R, bf, cur_stream());
  TORCH_CHECK(rc <= 0, "fedrec::additive_pool_bwd: kernel launch rejected the arguments (code ", rc, ")");
  if (n == 0) {  // nothing was launched, the partial row is unwritten: the sums are zero, no dsum
    auto zeros = at::zeros({Q + 1}, fopt);
    return {dx, dpre, zeros.narrow(0, 0, Q), zeros.narrow(0, Q, 1), at::empty({0}, fopt)};
  }
  // the partial rows -> sums, one deterministic colsum launch (dw2, db2 and, from the text
  // kernel, the dpre column sums)
  auto sums = at::empty({2 * Q + 1}, fopt);
  const float* xs[3] = {dw2p, db2p, dsump};
  float* os[3] = {sums.data_ptr<float>(), sums.data_ptr<float>() + Q, sums.data_ptr<float>() + Q + 1};
  const int ints[12] = {(int)R, (int)Q, (int)Q, 0, (int)R, 1, 1, 0, (int)R, (int)Q, (int)Q, 0};
  const int ncs = rc == 0 ? 3 : 2;
  const long need = fr_colsum_f32(xs, os, ints, ncs, nullptr, cur_stream());
  auto part = at::empty({std::max<long>(need, 1)}, fopt);
  TORCH_CHECK(need >= 0 && fr_colsum_f32(xs, os, ints, ncs, part.data_ptr<float>(), cur_stream()) == 0,
              "fedrec::additive_pool_bwd: colsum failed");
  auto dw2 = sums.narrow(0, 0, Q);
  auto db2 = sums.narrow(0, Q, 1);
  auto dsum = rc == 0 ? sums.narrow(0, Q + 1, Q) : at::empty({0}, fopt);
  return {dx, dpre, dw2, db2, dsum};
}

// user pool backward with da out (column 0 of [n T, 8]) instead of dw2 / db2 (fr_upool_bwd_da)
// bf16_out: dpre rounded to bf16 as a fourth output (the bf16 dctx GEMM's operand); otherwise
// the fourth output is empty
Tensor4 upool_bwd_da(const at::Tensor& x, const at::Tensor& e, const at::Tensor& alpha, const at::Tensor& w2,
                     const at::Tensor& g, bool bf16_out) {
  for (auto* t : {&x, &e, &alpha, &w2, &g}) {
    check_dev(*t, "upool_bwd_da input");
    TORCH_CHECK(t->scalar_type() == at::kFloat && t->is_contiguous(), "fedrec::upool_bwd_da: contiguous fp32");
  }
  const c10::DeviceGuard dg(x.device());
  const int64_t n = x.size(0), T = x.size(1), D = x.size(2), Q = e.size(2);
  TORCH_CHECK(e.size(0) == n && e.size(1) == T && alpha.numel() == n * T && w2.numel() == Q && g.numel() == n * D,
              "fedrec::upool_bwd_da: shapes");
  auto dx = at::empty({n, T, D}, x.options());
  auto dpre = at::empty({n, T, Q}, x.options());
  auto da8 = at::empty({n * T, 8}, x.options());
  auto dpre_b = at::empty({bf16_out ? n : 0, T, Q}, x.options().dtype(at::kBFloat16));
  check_rc(fr_upool_bwd_da(x.data_ptr<float>(), e.data_ptr<float>(), alpha.data_ptr<float>(), w2.data_ptr<float>(),
                           g.data_ptr<float>(), dx.data_ptr<float>(), dpre.data_ptr<float>(), da8.data_ptr<float>(),
                           (int)n, (int)T, (int)D, (int)Q, cur_stream(), bf16_out ? dpre_b.data_ptr() : nullptr),
           "upool_bwd_da");
  return {dx, dpre, da8, dpre_b};
}

}  // namespace

TORCH_LIBRARY_FRAGMENT(fedrec, m) {
  m.def("head_score_set_rows(int r) -> ()", [](int64_t r) { fr_head_score_set_rows((int)r); });
  m.def("head_score_set_ilv(int v) -> ()", [](int64_t v) { fr_head_score_set_ilv((int)v); });
  m.def("head_supported(int D, int Q, int T) -> bool",
        [](int64_t D, int64_t Q, int64_t T) { return fr_head_supported((int)D, (int)Q, (int)T) != 0; });
  m.def("head_g_supported(int D, int Q, int T) -> bool",
        [](int64_t D, int64_t Q, int64_t T) { return fr_head_g_supported((int)D, (int)Q, (int)T) != 0; });
  m.def("head_score(Tensor table, Tensor? ids, int T, Tensor w1, Tensor b1, Tensor w2, Tensor b2, bool store_e, Tensor? nreal=None) -> (Tensor, Tensor)", on_gpu(&head_score));
  m.def("head_pool(Tensor table, Tensor? ids, int T, Tensor a, Tensor? tokens, Tensor? nreal=None, bool want_bf16=False) -> (Tensor, Tensor, Tensor)", on_gpu(&head_pool));
  m.def("head_pool_bwd(Tensor table, Tensor? ids, int T, Tensor alpha, Tensor g, Tensor? nreal=None) -> (Tensor, Tensor)", on_gpu(&head_pool_bwd));
  m.def("head_wgrad(Tensor table, Tensor? ids, int T, Tensor e, Tensor da, Tensor w2, Tensor db2p, Tensor? nreal=None) -> (Tensor, Tensor, Tensor, Tensor)", on_gpu(&head_wgrad));
  m.def("head_pool_bwd_g(Tensor table, Tensor? ids, int T, Tensor alpha, Tensor g, Tensor(a!) e, Tensor? nreal=None) -> (Tensor, Tensor, Tensor)", on_gpu(&head_pool_bwd_g));
  m.def("head_wgrad_g(Tensor table, Tensor? ids, int T, Tensor G, Tensor cs, Tensor w2, Tensor db2p, Tensor? nreal=None, Tensor(a!)[]? out=None) -> (Tensor, Tensor, Tensor, Tensor)", on_gpu(&head_wgrad_g));
  m.def("additive_pool_fwd(Tensor x, Tensor e, Tensor w2, Tensor b2, Tensor? keep=None) -> (Tensor, Tensor)", on_gpu(&additive_pool_fwd));
  m.def("additive_pool_bwd(Tensor x, Tensor e, Tensor alpha, Tensor w2, Tensor g, bool want_dx) -> (Tensor, Tensor, Tensor, Tensor, Tensor)", on_gpu(&additive_pool_bwd));
  m.def("upool_bwd_da(Tensor x, Tensor e, Tensor alpha, Tensor w2, Tensor g, bool bf16_out=False) -> (Tensor, Tensor, Tensor, Tensor)", on_gpu(&upool_bwd_da));
}

// the pool ops take host tensors too: they reach the argument checks and fail the device check last
// (there is no host kernel; ops.additive_pool_* sends host tensors to the torch oracle before it gets here)
TORCH_LIBRARY_IMPL(fedrec, CPU, m) {
  m.impl("additive_pool_fwd", &additive_pool_fwd);
  m.impl("additive_pool_bwd", &additive_pool_bwd);
}
