// fedrec_krum ops: multi-Krum aggregation (krum.hip).  A namespace of its own: the fedrec::,
// fedrec_eval::, fedrec_rerank::, fedrec_agg::, fedrec_sparse:: and fedrec_quant:: op sets are pinned as
// they stand (tests/golden/op_schemas*.txt).
#include "binding_util.h"

namespace {

// dtype, shape, contiguity and bounds first (they do not depend on where the tensor lives); the
// messages are those of ops/reference.py krum_*_check
void check_stack(const at::Tensor& stack, const char* op) {
  TORCH_CHECK(stack.scalar_type() == at::kFloat, op, ": stack must be fp32");
  TORCH_CHECK(stack.dim() == 2, op, ": stack [W, n] (got ", stack.dim(), " dims)");
  TORCH_CHECK(stack.is_contiguous(), op, ": stack must be contiguous");
  const int64_t W = stack.size(0), n = stack.size(1);
  TORCH_CHECK(W >= 1 && W <= 32 && n >= 1, op, ": 1 <= W <= 32, n >= 1 (got W ", W, ", n ", n, ")");
}

// ---- G = Y Y^T of the centred rows y_c = stack[c] - center, fp64 [W, W] (krum.hip)
at::Tensor centered_gram(const at::Tensor& stack, const at::Tensor& center, int64_t max_blocks) {
  const char* op = "fedrec_krum::centered_gram";
  check_stack(stack, op);
  const int64_t W = stack.size(0), n = stack.size(1);
  TORCH_CHECK(center.scalar_type() == at::kFloat, op, ": center must be fp32");
  TORCH_CHECK(center.dim() == 1 && center.numel() == n, op, ": center [n] (got ", center.numel(), " elements, n ", n, ")");
  TORCH_CHECK(center.is_contiguous(), op, ": center must be contiguous");
  TORCH_CHECK(max_blocks >= 0 && max_blocks < (int64_t(1) << 31), op, ": max_blocks >= 0 (got ", max_blocks, ")");
  TORCH_CHECK(stack.device() == center.device(), op, ": stack and center must be on one device");
  TORCH_CHECK(stack.is_cuda(), op, ": stack and center must be device tensors");
  const c10::DeviceGuard g(stack.device());
  auto part = at::empty({(int64_t)fr_krum_gram_ws((int)W, (long)n)}, stack.options());
  auto G = at::empty({W, W}, stack.options().dtype(at::kDouble));
  const int rc = fr_krum_gram(stack.data_ptr<float>(), center.data_ptr<float>(), part.data_ptr<float>(),
                              G.data_ptr<double>(), (int)W, (long)n, (int)max_blocks, cur_stream());
  TORCH_CHECK(rc == 0, op, ": unsupported shape (code ", rc, ")");
  return G;
}

// ---- Krum scores and the m best clients from the Gram matrix (krum.hip)
Tensor2 krum_select(const at::Tensor& G, int64_t f, int64_t m) {
  const char* op = "fedrec_krum::select";
  TORCH_CHECK(G.scalar_type() == at::kDouble, op, ": G must be fp64");
  TORCH_CHECK(G.dim() == 2 && G.size(0) == G.size(1), op, ": G [W, W]");
  TORCH_CHECK(G.is_contiguous(), op, ": G must be contiguous");
  const int64_t W = G.size(0);
  TORCH_CHECK(W >= 1 && W <= 32, op, ": 1 <= W <= 32 (got W ", W, ")");
  TORCH_CHECK(f >= 0 && W >= 2 * f + 3, op, ": f >= 0 and W >= 2 f + 3 (got f ", f, ", W ", W, ")");
  TORCH_CHECK(m >= 1 && m <= W - f, op, ": 1 <= m <= W - f (got m ", m, ", W ", W, ", f ", f, ")");
  TORCH_CHECK(G.is_cuda(), op, ": G must be a device tensor");
  const c10::DeviceGuard g(G.device());
  auto selected = at::empty({W}, G.options().dtype(at::kInt));
  auto scores = at::empty({W}, G.options().dtype(at::kFloat));
  const int rc = fr_krum_select(G.data_ptr<double>(), selected.data_ptr<int>(), scores.data_ptr<float>(), (int)W, (int)f,
                                (int)m, cur_stream());
  TORCH_CHECK(rc == 0, op, ": unsupported shape (code ", rc, ")");
  return {selected, scores};
}

// ---- the client-order mean of the selected rows (krum.hip); selected stays on the device
at::Tensor selected_mean(const at::Tensor& stack, const at::Tensor& selected) {
  const char* op = "fedrec_krum::selected_mean";
  check_stack(stack, op);
  const int64_t W = stack.size(0), n = stack.size(1);
  TORCH_CHECK(selected.scalar_type() == at::kInt, op, ": selected must be int32");
  TORCH_CHECK(selected.dim() == 1 && selected.numel() == W, op, ": selected [W] (got ", selected.numel(), " elements, W ", W,
              ")");
  TORCH_CHECK(selected.is_contiguous(), op, ": selected must be contiguous");
  TORCH_CHECK(stack.device() == selected.device(), op, ": stack and selected must be on one device");
  TORCH_CHECK(stack.is_cuda(), op, ": stack and selected must be device tensors");
  const c10::DeviceGuard g(stack.device());
  auto out = at::empty({n}, stack.options());
  const int rc = fr_krum_selected_mean(stack.data_ptr<float>(), selected.data_ptr<int>(), out.data_ptr<float>(), (int)W,
                                       (long)n, cur_stream());
  TORCH_CHECK(rc == 0, op, ": unsupported shape (code ", rc, ")");
  return out;
}

}  // namespace

// registered for every backend, as fedrec_agg is: a host tensor reaches the checks above and fails the
// device check last (ops.krum_* send host tensors to the torch oracles before they get here)
TORCH_LIBRARY_FRAGMENT(fedrec_krum, m) {
  m.def("centered_gram(Tensor stack, Tensor center, int max_blocks=0) -> Tensor", &centered_gram);
  m.def("select(Tensor G, int f, int m) -> (Tensor, Tensor)", &krum_select);
  m.def("selected_mean(Tensor stack, Tensor selected) -> Tensor", &selected_mean);
}
