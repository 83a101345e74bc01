// fedrec_sparse ops: top-k sparsified uploads with error feedback (sparse_delta.hip).  A namespace of
// its own: the fedrec::, fedrec_eval::, fedrec_rerank:: and fedrec_agg:: op sets are pinned as they
// stand (tests/golden/op_schemas*.txt).
#include "binding_util.h"

namespace {

// the byte ranges [p, p + 4 n) of two tensors meet
bool overlaps(const at::Tensor& a, const at::Tensor& b) {
  const char* pa = static_cast<const char*>(a.data_ptr());
  const char* pb = static_cast<const char*>(b.data_ptr());
  return pa < pb + b.numel() * b.element_size() && pb < pa + a.numel() * a.element_size();
}

void check_vec(const at::Tensor& t, const char* op, const char* name) {
  TORCH_CHECK(t.scalar_type() == at::kFloat, op, ": ", name, " must be fp32");
  TORCH_CHECK(t.dim() == 1, op, ": ", name, " [n] (got ", t.dim(), " dims)");
  TORCH_CHECK(t.is_contiguous(), op, ": ", name, " must be contiguous");
}

// ---- exact magnitude top-k of (local - global) + residual (sparse_delta.hip): -> (idx [k] int32
// ascending, val [k] fp32); residual keeps what was not sent.  Dtype, shape, contiguity, bounds and
// aliasing are checked first (they do not depend on where the tensors live), then the device
Tensor2 topk_delta(const at::Tensor& local, const at::Tensor& global_, at::Tensor& residual, int64_t k) {
  const char* op = "fedrec_sparse::topk_delta";
  check_vec(local, op, "local");
  check_vec(global_, op, "global");
  check_vec(residual, op, "residual");
  const int64_t n = local.numel();
  TORCH_CHECK(global_.numel() == n && residual.numel() == n, op, ": local, global and residual must have one length (got ",
              n, ", ", global_.numel(), ", ", residual.numel(), ")");
  TORCH_CHECK(n >= 1 && n < (int64_t(1) << 31), op, ": 1 <= n < 2^31 (got n ", n, ")");
  TORCH_CHECK(k >= 1 && k <= n, op, ": 1 <= k <= n (got k ", k, ", n ", n, ")");
  TORCH_CHECK(local.device() == residual.device() && global_.device() == residual.device(), op,
              ": local, global and residual must be on one device");
  TORCH_CHECK(!overlaps(residual, local) && !overlaps(residual, global_), op,
              ": residual must not overlap local or global");
  TORCH_CHECK(residual.is_cuda(), op, ": local, global and residual must be device tensors");
  const c10::DeviceGuard g(residual.device());
  auto idx = at::empty({k}, residual.options().dtype(at::kInt));
  auto val = at::empty({k}, residual.options());
  auto ws = at::empty({fr_topk_delta_ws((long)n)}, residual.options().dtype(at::kInt));
  const int rc = fr_topk_delta(local.data_ptr<float>(), global_.data_ptr<float>(), residual.data_ptr<float>(),
                               idx.data_ptr<int>(), val.data_ptr<float>(), (unsigned*)ws.data_ptr<int>(), (long)n, (long)k,
                               cur_stream());
  TORCH_CHECK(rc == 0, op, ": unsupported shape (code ", rc, ")");
  return {idx, val};
}

// ---- base + (sum over clients of weights[c] * scatter(idx[c], val[c])) / sum(weights)
// (sparse_delta.hip): each row of idx strictly ascending in [0, n) is the CALLER's check
// (ops.reference.sparse_upload_check); the kernel stays in bounds for any content
at::Tensor combine(const at::Tensor& base, const at::Tensor& idx, const at::Tensor& val, const at::Tensor& weights) {
  const char* op = "fedrec_sparse::combine";
  check_vec(base, op, "base");
  TORCH_CHECK(idx.scalar_type() == at::kInt, op, ": idx must be int32");
  TORCH_CHECK(val.scalar_type() == at::kFloat, op, ": val must be fp32");
  TORCH_CHECK(idx.dim() == 2 && val.dim() == 2 && idx.sizes() == val.sizes(), op, ": idx and val [W, k] of one shape");
  TORCH_CHECK(idx.is_contiguous() && val.is_contiguous(), op, ": idx and val must be contiguous");
  check_vec(weights, op, "weights");
  const int64_t n = base.numel(), W = idx.size(0), k = idx.size(1);
  TORCH_CHECK(n >= 1 && n < (int64_t(1) << 31), op, ": 1 <= n < 2^31 (got n ", n, ")");
  TORCH_CHECK(W >= 1 && W <= 65536 && weights.numel() == W, op, ": 1 <= W <= 65536 and weights [W] (got W ", W,
              ", weights ", weights.numel(), ")");
  TORCH_CHECK(k >= 1 && k <= n, op, ": 1 <= k <= n (got k ", k, ", n ", n, ")");
  TORCH_CHECK(idx.device() == base.device() && val.device() == base.device() && weights.device() == base.device(), op,
              ": base, idx, val and weights must be on one device");
  TORCH_CHECK(base.is_cuda(), op, ": base, idx, val and weights must be device tensors");
  const c10::DeviceGuard g(base.device());
  auto out = at::empty_like(base);
  const int rc = fr_sparse_combine(base.data_ptr<float>(), idx.data_ptr<int>(), val.data_ptr<float>(),
                                   weights.data_ptr<float>(), out.data_ptr<float>(), (int)W, (long)k, (long)n, cur_stream());
  TORCH_CHECK(rc == 0, op, ": unsupported shape (code ", rc, ")");
  return out;
}

}  // namespace

// registered for every backend, as fedrec_agg is: a host tensor reaches the checks above and fails the
// device check last (ops.topk_delta / ops.sparse_combine send host tensors to the torch oracles)
TORCH_LIBRARY_FRAGMENT(fedrec_sparse, m) {
  m.def("topk_delta(Tensor local, Tensor global_, Tensor(a!) residual, int k) -> (Tensor, Tensor)", &topk_delta);
  m.def("combine(Tensor base, Tensor idx, Tensor val, Tensor weights) -> Tensor", &combine);
}
