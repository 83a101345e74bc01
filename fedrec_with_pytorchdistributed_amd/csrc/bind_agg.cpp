// fedrec_agg ops: Byzantine-robust aggregation (robust_agg.hip).  A namespace of its own: the
// fedrec::, fedrec_eval:: and fedrec_rerank:: op sets are pinned as they stand
// (tests/golden/op_schemas*.txt).
#include "binding_util.h"

namespace {

// ---- coordinate-wise trimmed mean / median (robust_agg.hip): stack [W, n] fp32 -> (out [n] fp32,
// dropped [W] int64).  Dtype, shape, contiguity and bounds are checked first (they do not depend on
// where the tensor lives), then the device
Tensor2 trimmed_mean(const at::Tensor& stack, int64_t trim) {
  TORCH_CHECK(stack.scalar_type() == at::kFloat, "fedrec_agg::trimmed_mean: stack must be fp32");
  TORCH_CHECK(stack.dim() == 2, "fedrec_agg::trimmed_mean: stack [W, n] (got ", stack.dim(), " dims)");
  TORCH_CHECK(stack.is_contiguous(), "fedrec_agg::trimmed_mean: stack must be contiguous");
  const int64_t W = stack.size(0), n = stack.size(1);
  TORCH_CHECK(W >= 1 && W <= 32 && n >= 1, "fedrec_agg::trimmed_mean: 1 <= W <= 32, n >= 1 (got W ", W, ", n ", n, ")");
  TORCH_CHECK(trim >= 0 && 2 * trim < W, "fedrec_agg::trimmed_mean: 0 <= 2 * trim < W (got trim ", trim, ", W ", W,
              ")");
  TORCH_CHECK(stack.is_cuda(), "fedrec_agg::trimmed_mean: stack must be a device tensor");
  const c10::DeviceGuard g(stack.device());
  auto out = at::empty({n}, stack.options());
  auto dropped = at::empty({W}, stack.options().dtype(at::kLong));
  const int rc = fr_trimmed_mean(stack.data_ptr<float>(), out.data_ptr<float>(),
                                 (long long*)dropped.data_ptr<int64_t>(), (int)W, (long)n, (int)trim, cur_stream());
  TORCH_CHECK(rc == 0, "fedrec_agg::trimmed_mean: unsupported shape (code ", rc, ")");
  return {out, dropped};
}

}  // namespace

// registered for every backend, as fedrec_rerank is: a host tensor reaches the checks above and fails
// the device check last (ops.trimmed_mean sends host tensors to the torch oracle before it gets here)
TORCH_LIBRARY_FRAGMENT(fedrec_agg, m) {
  m.def("trimmed_mean(Tensor stack, int trim) -> (Tensor, Tensor)", &trimmed_mean);
}
