// fedrec_geomed ops: geometric-median aggregation on the Gram matrix (geomed.hip).  A namespace of its
// own: the fedrec::, fedrec_eval::, fedrec_rerank::, fedrec_agg::, fedrec_krum::, fedrec_sparse:: and
// fedrec_quant:: op sets are pinned as they stand (tests/golden/op_schemas*.txt).
#include "binding_util.h"

namespace {

// dtype, shape, contiguity and bounds first (they do not depend on where the tensor lives); the
// messages are those of ops/reference.py geomed_*_check

// ---- Weiszfeld weights and distances from the centred Gram matrix, 32 rounds in one wave (geomed.hip)
Tensor2 geomed_weights(const at::Tensor& G) {
  const char* op = "fedrec_geomed::weights";
  TORCH_CHECK(G.scalar_type() == at::kDouble, op, ": G must be fp64");
  TORCH_CHECK(G.dim() == 2 && G.size(0) == G.size(1), op, ": G [W, W]");
  TORCH_CHECK(G.is_contiguous(), op, ": G must be contiguous");
  const int64_t W = G.size(0);
  TORCH_CHECK(W >= 1 && W <= 32, op, ": 1 <= W <= 32 (got W ", W, ")");
  TORCH_CHECK(G.is_cuda(), op, ": G must be a device tensor");
  const c10::DeviceGuard g(G.device());
  auto a = at::empty({W}, G.options());
  auto dist = at::empty({W}, G.options().dtype(at::kFloat));
  const int rc = fr_geomed_weights(G.data_ptr<double>(), a.data_ptr<double>(), dist.data_ptr<float>(), (int)W, cur_stream());
  TORCH_CHECK(rc == 0, op, ": unsupported shape (code ", rc, ")");
  return {a, dist};
}

// ---- sum_c fp32(a_c) x_c over the rows of non-zero weight (geomed.hip); a stays on the device
at::Tensor geomed_combine(const at::Tensor& stack, const at::Tensor& a) {
  const char* op = "fedrec_geomed::combine";
  TORCH_CHECK(stack.scalar_type() == at::kFloat, op, ": stack must be fp32");
  TORCH_CHECK(stack.dim() == 2, op, ": stack [W, n] (got ", stack.dim(), " dims)");
  TORCH_CHECK(stack.is_contiguous(), op, ": stack must be contiguous");
  const int64_t W = stack.size(0), n = stack.size(1);
  TORCH_CHECK(W >= 1 && W <= 32 && n >= 1, op, ": 1 <= W <= 32, n >= 1 (got W ", W, ", n ", n, ")");
  TORCH_CHECK(a.scalar_type() == at::kDouble, op, ": a must be fp64");
  TORCH_CHECK(a.dim() == 1 && a.numel() == W, op, ": a [W] (got ", a.numel(), " elements, W ", W, ")");
  TORCH_CHECK(a.is_contiguous(), op, ": a must be contiguous");
  TORCH_CHECK(stack.device() == a.device(), op, ": stack and a must be on one device");
  TORCH_CHECK(stack.is_cuda(), op, ": stack and a must be device tensors");
  const c10::DeviceGuard g(stack.device());
  auto out = at::empty({n}, stack.options());
  const int rc = fr_geomed_combine(stack.data_ptr<float>(), a.data_ptr<double>(), out.data_ptr<float>(), (int)W, (long)n,
                                   cur_stream());
  TORCH_CHECK(rc == 0, op, ": unsupported shape (code ", rc, ")");
  return out;
}

}  // namespace

// registered for every backend, as fedrec_krum is: a host tensor reaches the checks above and fails the
// device check last (ops.geomed_* send host tensors to the torch oracles before they get here)
TORCH_LIBRARY_FRAGMENT(fedrec_geomed, m) {
  m.def("weights(Tensor G) -> (Tensor, Tensor)", &geomed_weights);
  m.def("combine(Tensor stack, Tensor a) -> Tensor", &geomed_combine);
}
