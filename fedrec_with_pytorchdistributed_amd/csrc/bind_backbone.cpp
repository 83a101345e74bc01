// fedrec ops of the text backbone: GEMMs (gemm_bf16.hip, gemm_wgrad.hip), LayerNorm / GELU /
// embedding (layernorm.hip), dropout (dropout.hip), title attention (title_attn*.hip) and the
// training-path reductions (train_grad.hip).
#include "binding_util.h"

namespace {

at::Tensor linear(const at::Tensor& x, const at::Tensor& w, const OptTensor& b, int64_t act, const OptTensor& residual) {
  check_dev(x, "x");
  check_dev(w, "w");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 && w.scalar_type() == at::kBFloat16, "fedrec::linear: bf16 x/w");
  const c10::DeviceGuard g(x.device());
  const int64_t K = x.size(-1), N = w.size(0);
  TORCH_CHECK(w.size(1) == K, "fedrec::linear: K mismatch");
  const int64_t M = x.numel() / K;
  auto out_shape = x.sizes().vec();
  out_shape.back() = N;
  auto out = gemm_out(x, M, N).view(out_shape);
  at::Tensor bf;
  const float* bp = bias_ptr(b, N, "linear", bf);
  const void* rp = opt_bf16_ptr(residual, M * N, "residual", "linear", "residual");
  if (M == 0) return out;
  check_rc(fr_gemm_nt_bf16(x.data_ptr(), w.data_ptr(), bp, rp, out.data_ptr(), (int)M, (int)N, (int)K, (int)act,
                           (int)gemm_rows(M), cur_stream()),
           "linear");
  return out;
}

at::Tensor linear_split(const at::Tensor& x, const at::Tensor& w, const OptTensor& b, const at::Tensor& full_rows,
                        int64_t n_partial) {
  check_dev(x, "x");
  check_dev(w, "w");
  check_dev(full_rows, "full_rows");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 && w.scalar_type() == at::kBFloat16, "fedrec::linear_split: bf16 x/w");
  TORCH_CHECK(full_rows.scalar_type() == at::kInt && full_rows.numel() == 1, "fedrec::linear_split: full_rows int32[1]");
  const c10::DeviceGuard g(x.device());
  const int64_t K = x.size(-1), N = w.size(0);
  TORCH_CHECK(w.size(1) == K && n_partial > 0 && n_partial <= N, "fedrec::linear_split: shapes");
  const int64_t M = x.numel() / K;
  auto out = gemm_out(x, M, N).view({M, N});
  at::Tensor bf;
  const float* bp = bias_ptr(b, N, "linear_split", bf);
  if (M == 0) return out;
  check_rc(fr_gemm_nt_bf16_split(x.data_ptr(), w.data_ptr(), bp, out.data_ptr(), (int)M, (int)N, (int)K,
                                 (int)gemm_rows(M), full_rows.data_ptr<int>(), (int)n_partial, cur_stream()),
           "linear_split");
  return out;
}

// ---- training FFN1: h = GELU(z), z = x w^T + b from one GEMM pass ------------------------------
Tensor2 linear_gelu_dual(const at::Tensor& x, const at::Tensor& w, const at::Tensor& b) {
  check_dev(x, "x");
  check_dev(w, "w");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 && w.scalar_type() == at::kBFloat16, "fedrec::linear_gelu_dual: bf16");
  const c10::DeviceGuard g(x.device());
  const int64_t K = x.size(-1), N = w.size(0);
  TORCH_CHECK(w.size(1) == K, "fedrec::linear_gelu_dual: K mismatch");
  const int64_t M = x.numel() / K, c_rows = gemm_rows(M);
  auto h = gemm_out(x, M, N).view({M, N});
  auto z = gemm_out(x, M, N).view({M, N});
  at::Tensor bf;
  const float* bp = bias_ptr(b, N, "linear_gelu_dual", bf);
  if (M == 0) return {h, z};
  const int rc = fr_gemm_nt_bf16_dual(x.data_ptr(), w.data_ptr(), bp, h.data_ptr(), z.data_ptr(), (int)M, (int)N, (int)K,
                                      (int)c_rows, cur_stream());
  if (rc == 3) {  // outside the fused kernel's domain: GEMM, then the GELU pass
    check_rc(fr_gemm_nt_bf16(x.data_ptr(), w.data_ptr(), bp, nullptr, z.data_ptr(), (int)M, (int)N, (int)K, 0,
                             (int)c_rows, cur_stream()),
             "linear_gelu_dual");
    check_rc(fr_gelu_bf16(z.data_ptr(), nullptr, h.data_ptr(), (long)(M * N), 0, cur_stream()), "linear_gelu_dual");
  } else {
    check_rc(rc, "linear_gelu_dual");
  }
  return {h, z};
}

// dz = (dh W^T) * GELU'(z) and its column sums (FFN1 bias gradient) from one GEMM pass;
// returns (dz, colsum) -- colsum is undefined when the shape is outside the fused kernel's
// domain (the caller then sums dz itself)
Tensor2 linear_gelu_bwd(const at::Tensor& x, const at::Tensor& w, const at::Tensor& z) {
  check_dev(x, "x");
  check_dev(w, "w");
  check_dev(z, "z");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 && w.scalar_type() == at::kBFloat16 && z.scalar_type() == at::kBFloat16,
              "fedrec::linear_gelu_bwd: bf16");
  const c10::DeviceGuard g(x.device());
  const int64_t K = x.size(-1), N = w.size(0), M = x.numel() / K;
  TORCH_CHECK(w.size(1) == K && z.numel() == M * N, "fedrec::linear_gelu_bwd: shapes");
  const int64_t c_rows = gemm_rows(M);
  auto out = gemm_out(x, M, N).view({M, N});
  auto part = at::empty({c_rows / 256 * 2, N}, x.options().dtype(at::kFloat));
  const int rc = fr_gemm_gelu_bwd_colpart(x.data_ptr(), w.data_ptr(), z.data_ptr(), out.data_ptr(),
                                          part.data_ptr<float>(), (int)M, (int)N, (int)K, (int)c_rows, cur_stream());
  if (rc == 0) return {out, part.sum(0)};
  check_rc(fr_gemm_nt_bf16(x.data_ptr(), w.data_ptr(), nullptr, z.data_ptr(), out.data_ptr(), (int)M, (int)N, (int)K, 3,
                           (int)c_rows, cur_stream()),
           "linear_gelu_bwd");
  return {out, at::Tensor()};
}

// dW[N, K] = dy[M, N]^T x[M, K] in fp32 (gemm_wgrad.hip)
at::Tensor wgrad(const at::Tensor& dy, const at::Tensor& x) {
  check_dev(dy, "dy");
  check_dev(x, "x");
  TORCH_CHECK(dy.scalar_type() == at::kBFloat16 && x.scalar_type() == at::kBFloat16, "fedrec::wgrad: bf16 dy/x");
  const c10::DeviceGuard g(dy.device());
  const int64_t N = dy.size(-1), K = x.size(-1), M = dy.numel() / std::max<int64_t>(N, 1);
  TORCH_CHECK(x.numel() == M * K, "fedrec::wgrad: row count mismatch");
  TORCH_CHECK(N % 8 == 0 && K % 8 == 0, "fedrec::wgrad: N, K must be multiples of 8");
  TORCH_CHECK(M < (1ll << 31), "fedrec::wgrad: too many rows");
  auto C = at::empty({N, K}, dy.options().dtype(at::kFloat));
  if (M == 0) return C.zero_();
  const long need = fr_wgrad_bf16(dy.data_ptr(), x.data_ptr(), C.data_ptr<float>(), nullptr, (int)M, (int)N, (int)K, 0,
                                  cur_stream());
  TORCH_CHECK(need >= 0, "fedrec::wgrad: unsupported shape");
  if (need > 0) {
    auto scratch = at::empty({need}, C.options());
    TORCH_CHECK(fr_wgrad_bf16(dy.data_ptr(), x.data_ptr(), C.data_ptr<float>(), scratch.data_ptr<float>(), (int)M,
                              (int)N, (int)K, 0, cur_stream()) == 0,
                "fedrec::wgrad: launch");
  }
  return C;
}

// ---- LayerNorm, GELU, embedding (layernorm.hip) ------------------------------------------------
at::Tensor layer_norm(const at::Tensor& x, const at::Tensor& w, const at::Tensor& b, double eps,
                      const OptTensor& residual) {
  check_dev(x, "x");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16, "fedrec::layer_norm: bf16");
  const c10::DeviceGuard g(x.device());
  const int64_t D = x.size(-1);
  auto wf = as_f32(w), bf = as_f32(b);
  const void* rp = opt_bf16_ptr(residual, x.numel(), "residual", "layer_norm", "residual must match x (bf16)");
  auto y = at::empty_like(x);
  check_rc(fr_layer_norm_bf16(x.data_ptr(), wf.data_ptr<float>(), bf.data_ptr<float>(), y.data_ptr(),
                              (int)(x.numel() / D), (int)D, (float)eps, rp, cur_stream()),
           "layer_norm");
  return y;
}

at::Tensor layer_norm_scatter(const at::Tensor& x, const at::Tensor& w, const at::Tensor& b, double eps,
                              const OptTensor& residual, const at::Tensor& dst, const OptTensor& out) {
  check_dev(x, "x");
  check_dev(dst, "dst");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16, "fedrec::layer_norm_scatter: bf16");
  const c10::DeviceGuard g(x.device());
  const int64_t D = x.size(-1), rows = x.numel() / D;
  TORCH_CHECK(dst.scalar_type() == at::kInt && dst.numel() == rows && D % 256 == 0,
              "fedrec::layer_norm_scatter: dst int32[rows], D % 256 == 0");
  auto wf = as_f32(w), bf = as_f32(b);
  const void* rp = opt_bf16_ptr(residual, x.numel(), "residual", "layer_norm_scatter", "residual must match x (bf16)");
  // out (optional): the destination rows in place (the hidden-state cache's chunk) -- no copy
  at::Tensor y;
  if (defined(out)) {
    check_dev(*out, "out");
    TORCH_CHECK(out->scalar_type() == at::kBFloat16 && out->is_contiguous() && out->numel() == x.numel(),
                "fedrec::layer_norm_scatter: out bf16 contiguous, x's size");
    y = *out;
  } else {
    y = at::empty_like(x);
  }
  check_rc(fr_layer_norm_scatter_bf16(x.data_ptr(), wf.data_ptr<float>(), bf.data_ptr<float>(), y.data_ptr(), (int)rows,
                                      (int)D, (float)eps, rp, dst.data_ptr<int>(), cur_stream()),
           "layer_norm_scatter");
  return y;
}

Tensor4 layer_norm_bwd_impl(const at::Tensor& x, const at::Tensor& w, const at::Tensor& dy, double eps, bool want_dxsum) {
  check_dev(x, "x");
  check_dev(dy, "dy");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 && dy.scalar_type() == at::kBFloat16, "fedrec::layer_norm_bwd: bf16");
  const c10::DeviceGuard g(x.device());
  const int64_t D = x.size(-1);
  auto wf = as_f32(w);
  auto dx = at::empty_like(x);
  // the kernel accumulates dw / db (/ dx column sums) across row blocks: one zeroed buffer,
  // one fill launch (three at::zeros were 75 fill launches per config-5 step)
  auto acc = at::zeros({want_dxsum ? 3 : 2, D}, x.options().dtype(at::kFloat));
  auto dw = acc[0];
  auto db = acc[1];
  at::Tensor dxs = want_dxsum ? acc[2] : at::Tensor();
  check_rc(fr_layer_norm_bwd_bf16(x.data_ptr(), wf.data_ptr<float>(), dy.data_ptr(), dx.data_ptr(), dw.data_ptr<float>(),
                                  db.data_ptr<float>(), (int)(x.numel() / D), (int)D, (float)eps, cur_stream(),
                                  want_dxsum ? dxs.data_ptr<float>() : nullptr, nullptr, 0.f, 0ull, 0ull),
           "layer_norm_bwd");
  return {dx, dw, db, dxs};
}

Tensor3 layer_norm_bwd(const at::Tensor& x, const at::Tensor& w, const at::Tensor& dy, double eps) {
  auto r = layer_norm_bwd_impl(x, w, dy, eps, false);
  return {std::get<0>(r), std::get<1>(r), std::get<2>(r)};
}

// + the column sums of dx (bias gradient of the layer feeding the LayerNorm)
Tensor4 layer_norm_bwd_colsum(const at::Tensor& x, const at::Tensor& w, const at::Tensor& dy, double eps) {
  return layer_norm_bwd_impl(x, w, dy, eps, true);
}

// + the dropout backward of the layer feeding the LayerNorm: (dx, dx o Z, dw, db, colsum(dx o Z))
Tensor5 layer_norm_bwd_drop(const at::Tensor& x, const at::Tensor& w, const at::Tensor& dy, double eps, double p,
                            int64_t seed, int64_t offset) {
  check_dev(x, "x");
  check_dev(dy, "dy");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 && dy.scalar_type() == at::kBFloat16, "fedrec::layer_norm_bwd_drop: bf16");
  TORCH_CHECK(x.is_contiguous() && dy.is_contiguous() && dy.numel() == x.numel(), "fedrec::layer_norm_bwd_drop: shapes");
  const c10::DeviceGuard g(x.device());
  const int64_t D = x.size(-1);
  auto wf = as_f32(w);
  auto dx = at::empty_like(x);
  auto dxz = at::empty_like(x);
  auto acc = at::zeros({3, D}, x.options().dtype(at::kFloat));
  check_rc(fr_layer_norm_bwd_bf16(x.data_ptr(), wf.data_ptr<float>(), dy.data_ptr(), dx.data_ptr(),
                                  acc[0].data_ptr<float>(), acc[1].data_ptr<float>(), (int)(x.numel() / D), (int)D,
                                  (float)eps, cur_stream(), acc[2].data_ptr<float>(), dxz.data_ptr(), (float)p,
                                  (unsigned long long)seed, (unsigned long long)offset),
           "layer_norm_bwd_drop");
  return {dx, dxz, acc[0], acc[1], acc[2]};
}

at::Tensor gelu(const at::Tensor& z, const OptTensor& dh) {
  check_dev(z, "z");
  TORCH_CHECK(z.scalar_type() == at::kBFloat16, "fedrec::gelu: bf16");
  const c10::DeviceGuard g(z.device());
  auto out = at::empty_like(z);
  const void* dp = opt_bf16_ptr(dh, z.numel(), "dh", "gelu", "dh");
  check_rc(fr_gelu_bf16(z.data_ptr(), dp, out.data_ptr(), (long)z.numel(), dp ? 1 : 0, cur_stream()), "gelu");
  return out;
}

at::Tensor embed_ln(const at::Tensor& tokens, const at::Tensor& word, const at::Tensor& pos, const at::Tensor& w,
                    const at::Tensor& b, double eps) {
  check_dev(word, "word");
  check_dev(pos, "pos");
  TORCH_CHECK(word.scalar_type() == at::kBFloat16 && pos.scalar_type() == at::kBFloat16, "fedrec::embed_ln: bf16");
  const c10::DeviceGuard g(word.device());
  auto tok = as_i32(tokens);
  TORCH_CHECK(tok.dim() == 2, "fedrec::embed_ln: tokens [n, T]");
  const int64_t n = tok.size(0), T = tok.size(1), D = word.size(1);
  TORCH_CHECK(T <= pos.size(0), "fedrec::embed_ln: T > max positions");
  auto wf = as_f32(w), bf = as_f32(b);
  auto y = at::empty({n * T, D}, word.options());
  check_rc(fr_embed_ln_bf16(tok.data_ptr<int>(), word.data_ptr(), pos.data_ptr(), wf.data_ptr<float>(),
                            bf.data_ptr<float>(), y.data_ptr(), (int)(n * T), (int)D, (int)T, (float)eps, cur_stream()),
           "embed_ln");
  return y;
}

at::Tensor embed_ln_rows(const at::Tensor& tokens, const at::Tensor& src, const at::Tensor& word, const at::Tensor& pos,
                         const at::Tensor& w, const at::Tensor& b, double eps) {
  check_dev(word, "word");
  check_dev(pos, "pos");
  check_dev(src, "src");
  TORCH_CHECK(word.scalar_type() == at::kBFloat16 && pos.scalar_type() == at::kBFloat16, "fedrec::embed_ln_rows: bf16");
  const c10::DeviceGuard g(word.device());
  auto tok = as_i32(tokens);
  TORCH_CHECK(tok.dim() == 2 && src.scalar_type() == at::kInt && src.numel() == tok.numel(),
              "fedrec::embed_ln_rows: tokens [n, T], src [n*T] int32");
  const int64_t n = tok.size(0), T = tok.size(1), D = word.size(1);
  TORCH_CHECK(T <= pos.size(0) && D % 256 == 0, "fedrec::embed_ln_rows: T <= max positions, D % 256 == 0");
  auto wf = as_f32(w), bf = as_f32(b);
  auto y = at::empty({n * T, D}, word.options());
  check_rc(fr_embed_ln_rows_bf16(tok.data_ptr<int>(), src.data_ptr<int>(), word.data_ptr(), pos.data_ptr(),
                                 wf.data_ptr<float>(), bf.data_ptr<float>(), y.data_ptr(), (int)(n * T), (int)D, (int)T,
                                 (float)eps, cur_stream()),
           "embed_ln_rows");
  return y;
}

// ---- dropout (backbone train mode; dropout.hip) ------------------------------------------------
at::Tensor dropout_add(const at::Tensor& h, const OptTensor& res, double p, int64_t seed, int64_t offset) {
  check_dev(h, "h");
  TORCH_CHECK(h.scalar_type() == at::kBFloat16, "fedrec::dropout_add: bf16");
  const c10::DeviceGuard g(h.device());
  const void* rp = opt_bf16_ptr(res, h.numel(), "res", "dropout_add", "res");
  auto out = at::empty_like(h);
  check_rc(fr_dropout_add_bf16(h.data_ptr(), rp, out.data_ptr(), (long)h.numel(), (float)p, (unsigned long long)seed,
                               (unsigned long long)offset, cur_stream()),
           "dropout_add");
  return out;
}

// ---- title attention (title_attn.hip, title_attn_bwd.hip; T > 64: title_attn_long.hip) --------
at::Tensor title_attention(const at::Tensor& qkv, const at::Tensor& mask, int64_t n_heads) {
  check_dev(qkv, "qkv");
  TORCH_CHECK(qkv.scalar_type() == at::kBFloat16, "fedrec::title_attention: bf16");
  const c10::DeviceGuard g(qkv.device());
  auto mk = as_i32(mask);
  const int64_t n = mk.size(0), T = mk.size(1), D = qkv.size(-1) / 3;
  TORCH_CHECK(qkv.numel() == n * T * 3 * D, "fedrec::title_attention: qkv shape");
  auto out = at::empty({n * T, D}, qkv.options());
  check_rc(fr_title_attention_bf16(qkv.data_ptr(), mk.data_ptr<int>(), out.data_ptr(), (int)n, (int)T, (int)n_heads,
                                   (int)D, cur_stream()),
           "title_attention");
  return out;
}

at::Tensor title_attention_drop(const at::Tensor& qkv, const at::Tensor& mask, int64_t n_heads, double p, int64_t seed,
                                int64_t offset) {
  check_dev(qkv, "qkv");
  TORCH_CHECK(qkv.scalar_type() == at::kBFloat16, "fedrec::title_attention_drop: bf16");
  const c10::DeviceGuard g(qkv.device());
  auto mk = as_i32(mask);
  const int64_t n = mk.size(0), T = mk.size(1), D = qkv.size(-1) / 3;
  TORCH_CHECK(qkv.numel() == n * T * 3 * D, "fedrec::title_attention_drop: qkv shape");
  auto out = at::empty({n * T, D}, qkv.options());
  check_rc(fr_title_attention_drop_bf16(qkv.data_ptr(), mk.data_ptr<int>(), out.data_ptr(), (int)n, (int)T,
                                        (int)n_heads, (int)D, (float)p, (unsigned long long)seed,
                                        (unsigned long long)offset, cur_stream()),
           "title_attention_drop");
  return out;
}

at::Tensor title_attention_bwd(const at::Tensor& qkv, const at::Tensor& dout, const at::Tensor& mask, int64_t n_heads) {
  check_dev(qkv, "qkv");
  check_dev(dout, "dout");
  TORCH_CHECK(qkv.scalar_type() == at::kBFloat16 && dout.scalar_type() == at::kBFloat16, "fedrec::title_attention_bwd");
  const c10::DeviceGuard g(qkv.device());
  auto mk = as_i32(mask);
  const int64_t n = mk.size(0), T = mk.size(1), D = qkv.size(-1) / 3;
  auto dqkv = at::empty_like(qkv);
  check_rc(fr_title_attention_bwd_bf16(qkv.data_ptr(), dout.data_ptr(), mk.data_ptr<int>(), dqkv.data_ptr(), (int)n,
                                       (int)T, (int)n_heads, (int)D, cur_stream()),
           "title_attention_bwd");
  return dqkv;
}

at::Tensor title_attention_bwd_drop(const at::Tensor& qkv, const at::Tensor& dout, const at::Tensor& mask,
                                    int64_t n_heads, double p, int64_t seed, int64_t offset) {
  check_dev(qkv, "qkv");
  check_dev(dout, "dout");
  TORCH_CHECK(qkv.scalar_type() == at::kBFloat16 && dout.scalar_type() == at::kBFloat16,
              "fedrec::title_attention_bwd_drop");
  const c10::DeviceGuard g(qkv.device());
  auto mk = as_i32(mask);
  const int64_t n = mk.size(0), T = mk.size(1), D = qkv.size(-1) / 3;
  TORCH_CHECK(qkv.numel() == n * T * 3 * D && dout.numel() == n * T * D, "fedrec::title_attention_bwd_drop: shapes");
  auto dqkv = at::empty_like(qkv);
  check_rc(fr_title_attention_bwd_drop_bf16(qkv.data_ptr(), dout.data_ptr(), mk.data_ptr<int>(), dqkv.data_ptr(),
                                            (int)n, (int)T, (int)n_heads, (int)D, (float)p, (unsigned long long)seed,
                                            (unsigned long long)offset, cur_stream()),
           "title_attention_bwd_drop");
  return dqkv;
}

// ---- packed title rows (frozen backbone forward; title_attn.hip) ----------------------------
Tensor6 title_plan(const at::Tensor& mask) {
  check_dev(mask, "mask");
  const c10::DeviceGuard g(mask.device());
  auto mk = as_i32(mask);
  TORCH_CHECK(mk.dim() == 2, "fedrec::title_plan: mask [n, T]");
  const int64_t n = mk.size(0), T = mk.size(1);
  TORCH_CHECK(T >= 1 && T <= 64, "fedrec::title_plan: T in [1, 64]");
  auto io = mk.options();
  auto rowmap = at::empty({n, T}, io), src = at::empty({n * T}, io);
  auto kv_start = at::empty({n}, io), kv_len = at::empty({n}, io), qstart = at::empty({n}, io);
  auto n_kv = at::zeros({1}, io);
  check_rc(fr_title_plan(mk.data_ptr<int>(), (int)n, (int)T, rowmap.data_ptr<int>(), src.data_ptr<int>(),
                         kv_start.data_ptr<int>(), kv_len.data_ptr<int>(), qstart.data_ptr<int>(), n_kv.data_ptr<int>(),
                         cur_stream()),
           "title_plan");
  return {rowmap, src, kv_start, kv_len, qstart, n_kv};
}

at::Tensor title_attention_packed(const at::Tensor& qkv, const at::Tensor& rowmap, const at::Tensor& kv_start,
                                  const at::Tensor& kv_len, const at::Tensor& qstart, int64_t n_heads) {
  check_dev(qkv, "qkv");
  check_dev(rowmap, "rowmap");
  check_dev(kv_start, "kv_start");
  check_dev(kv_len, "kv_len");
  TORCH_CHECK(qkv.scalar_type() == at::kBFloat16, "fedrec::title_attention_packed: bf16");
  TORCH_CHECK(rowmap.dim() == 2 && rowmap.scalar_type() == at::kInt, "fedrec::title_attention_packed: rowmap [n, T]");
  const c10::DeviceGuard g(qkv.device());
  const int64_t n = rowmap.size(0), T = rowmap.size(1), D = qkv.size(-1) / 3;
  check_dev(qstart, "qstart");
  TORCH_CHECK(qkv.numel() == n * T * 3 * D && kv_start.numel() == n && kv_len.numel() == n && qstart.numel() == n,
              "fedrec::title_attention_packed: shapes");
  auto out = at::empty({n * T, D}, qkv.options());
  check_rc(fr_title_attention_packed_bf16(qkv.data_ptr(), rowmap.data_ptr<int>(), kv_start.data_ptr<int>(),
                                          kv_len.data_ptr<int>(), qstart.data_ptr<int>(), out.data_ptr(), (int)n, (int)T,
                                          (int)n_heads, (int)D, cur_stream()),
           "title_attention_packed");
  return out;
}

// ---- training-path reductions (train_grad.hip) ----------------------------------------------
// streaming GELU backward + its column sums: (dz, colsum)
Tensor2 gelu_bwd_colsum(const at::Tensor& df, const at::Tensor& z) {
  check_dev(df, "df");
  check_dev(z, "z");
  TORCH_CHECK(df.scalar_type() == at::kBFloat16 && z.scalar_type() == at::kBFloat16 && df.numel() == z.numel(),
              "fedrec::gelu_bwd_colsum: bf16, same shape");
  const c10::DeviceGuard g(df.device());
  const int64_t N = df.size(-1), M = df.numel() / N;
  auto dz = at::empty_like(df);
  auto out = at::zeros({N}, df.options().dtype(at::kFloat));
  if (M == 0) return {dz, out};
  auto partial = at::empty({(int64_t)fr_colsum_chunks() * N}, df.options().dtype(at::kFloat));
  check_rc(fr_gelu_bwd_colsum_bf16(df.data_ptr(), z.data_ptr(), dz.data_ptr(), (int)M, (int)N,
                                   partial.data_ptr<float>(), out.data_ptr<float>(), cur_stream()),
           "gelu_bwd_colsum");
  return {dz, out};
}

at::Tensor colsum(const at::Tensor& x) {
  TORCH_CHECK(x.is_cuda(), "fedrec::colsum: x must be a device tensor");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16, "fedrec::colsum: bf16");
  const c10::DeviceGuard g(x.device());
  // contiguous [.., N], or a 2-D column slice with unit column stride (row stride = ld)
  const bool strided = x.dim() == 2 && x.stride(1) == 1 && x.stride(0) != x.size(1);
  TORCH_CHECK(strided || x.is_contiguous(), "fedrec::colsum: contiguous rows or a 2-D column slice");
  const int64_t N = x.size(-1), M = x.numel() / N;
  const int64_t ld = strided ? x.stride(0) : N;
  TORCH_CHECK(((uintptr_t)x.data_ptr()) % 16 == 0, "fedrec::colsum: 16-byte aligned rows");
  auto out = at::empty({N}, x.options().dtype(at::kFloat));
  if (M == 0) return out.zero_();
  auto partial = at::empty({(int64_t)fr_colsum_chunks() * N}, x.options().dtype(at::kFloat));
  check_rc(fr_colsum_bf16(x.data_ptr(), (int)M, (int)N, partial.data_ptr<float>(), out.data_ptr<float>(), cur_stream(),
                          (int)ld),
           "colsum");
  return out;
}

at::Tensor embed_grad(const at::Tensor& dx, const at::Tensor& sorted, const at::Tensor& perm, int64_t num_rows) {
  check_dev(dx, "dx");
  check_dev(sorted, "sorted");
  check_dev(perm, "perm");
  TORCH_CHECK(dx.scalar_type() == at::kBFloat16 && dx.dim() == 2, "fedrec::embed_grad: dx bf16 [R, D]");
  TORCH_CHECK(sorted.scalar_type() == at::kInt && perm.scalar_type() == at::kInt && sorted.numel() == dx.size(0) &&
                  perm.numel() == dx.size(0),
              "fedrec::embed_grad: sorted/perm int32 [R]");
  const c10::DeviceGuard g(dx.device());
  auto dword = at::zeros({num_rows, dx.size(1)}, dx.options().dtype(at::kFloat));
  auto scratch = at::zeros({dx.size(0) + 1}, sorted.options());
  check_rc(fr_embed_grad_bf16(dx.data_ptr(), sorted.data_ptr<int>(), perm.data_ptr<int>(), (int)dx.size(0),
                              (int)dx.size(1), dword.data_ptr<float>(), scratch.data_ptr<int>(), cur_stream()),
           "embed_grad");
  return dword;
}

}  // namespace

TORCH_LIBRARY_FRAGMENT(fedrec, m) {
  m.def("gemm_set_variant(int v) -> ()", [](int64_t v) { fr_gemm_set_variant((int)v); });
  m.def("ln_set_wide(int v) -> ()", [](int64_t v) { fr_ln_set_wide((int)v); });
  m.def("title_attn_set_waves(int w) -> ()", [](int64_t w) { fr_title_attn_set_waves((int)w); });
  m.def("title_attn_bwd_set_variant(int v) -> ()", [](int64_t v) { fr_title_attn_bwd_set_variant((int)v); });
  m.def("linear(Tensor x, Tensor w, Tensor? b, int act, Tensor? residual) -> Tensor", on_gpu(&linear));
  m.def("linear_split(Tensor x, Tensor w, Tensor? b, Tensor full_rows, int n_partial) -> Tensor", on_gpu(&linear_split));
  m.def("linear_gelu_dual(Tensor x, Tensor w, Tensor b) -> (Tensor, Tensor)", on_gpu(&linear_gelu_dual));
  m.def("linear_gelu_bwd(Tensor x, Tensor w, Tensor z) -> (Tensor, Tensor)", on_gpu(&linear_gelu_bwd));
  m.def("wgrad(Tensor dy, Tensor x) -> Tensor", on_gpu(&wgrad));
  m.def("layer_norm(Tensor x, Tensor w, Tensor b, float eps, Tensor? residual=None) -> Tensor", on_gpu(&layer_norm));
  m.def("layer_norm_scatter(Tensor x, Tensor w, Tensor b, float eps, Tensor? residual, Tensor dst, Tensor(a!)? out=None) -> Tensor", on_gpu(&layer_norm_scatter));
  m.def("layer_norm_bwd(Tensor x, Tensor w, Tensor dy, float eps) -> (Tensor, Tensor, Tensor)", on_gpu(&layer_norm_bwd));
  m.def("layer_norm_bwd_colsum(Tensor x, Tensor w, Tensor dy, float eps) -> (Tensor, Tensor, Tensor, Tensor)", on_gpu(&layer_norm_bwd_colsum));
  m.def("layer_norm_bwd_drop(Tensor x, Tensor w, Tensor dy, float eps, float p, int seed, int offset) -> "
        "(Tensor, Tensor, Tensor, Tensor, Tensor)", on_gpu(&layer_norm_bwd_drop));
  m.def("gelu(Tensor z, Tensor? dh) -> Tensor", on_gpu(&gelu));
  m.def("embed_ln(Tensor tokens, Tensor word, Tensor pos, Tensor w, Tensor b, float eps) -> Tensor", on_gpu(&embed_ln));
  m.def("embed_ln_rows(Tensor tokens, Tensor src, Tensor word, Tensor pos, Tensor w, Tensor b, float eps) -> Tensor", on_gpu(&embed_ln_rows));
  m.def("dropout_add(Tensor h, Tensor? res, float p, int seed, int offset) -> Tensor", on_gpu(&dropout_add));
  m.def("title_attention(Tensor qkv, Tensor mask, int n_heads) -> Tensor", on_gpu(&title_attention));
  m.def("title_attention_drop(Tensor qkv, Tensor mask, int n_heads, float p, int seed, int offset) -> Tensor", on_gpu(&title_attention_drop));
  m.def("title_attention_bwd(Tensor qkv, Tensor dout, Tensor mask, int n_heads) -> Tensor", on_gpu(&title_attention_bwd));
  m.def("title_attention_bwd_drop(Tensor qkv, Tensor dout, Tensor mask, int n_heads, float p, int seed, int offset) -> Tensor", on_gpu(&title_attention_bwd_drop));
  m.def("title_plan(Tensor mask) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)", on_gpu(&title_plan));
  m.def("title_attention_packed(Tensor qkv, Tensor rowmap, Tensor kv_start, Tensor kv_len, Tensor qstart, int n_heads) -> Tensor", on_gpu(&title_attention_packed));
  m.def("gelu_bwd_colsum(Tensor df, Tensor z) -> (Tensor, Tensor)", on_gpu(&gelu_bwd_colsum));
  m.def("colsum(Tensor x) -> Tensor", on_gpu(&colsum));
  m.def("embed_grad(Tensor dx, Tensor sorted, Tensor perm, int num_rows) -> Tensor", on_gpu(&embed_grad));
}
