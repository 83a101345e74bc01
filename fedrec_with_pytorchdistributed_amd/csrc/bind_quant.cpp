// fedrec_quant ops: block-quantized uploads with error feedback (quant_delta.hip).  A namespace of its
// own: the fedrec::, fedrec_eval::, fedrec_rerank::, fedrec_agg:: and fedrec_sparse:: op sets are pinned
// as they stand (tests/golden/op_schemas*.txt).
#include "binding_util.h"

namespace {

// the byte ranges of two tensors meet
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

// ---- stochastic int8 / int4 codes of (local - global) + residual with one scale per 256 coordinates
// (quant_delta.hip): -> (codes uint8 [ceil(n bits / 8)], scales fp32 [ceil(n / 256)]); residual keeps the
// quantisation error.  Dtype, shape, contiguity, bounds and aliasing are checked first (they do not
// depend on where the tensors live), then the device
Tensor2 quantize_delta(const at::Tensor& local, const at::Tensor& global_, at::Tensor& residual, int64_t bits,
                       int64_t seed, int64_t offset) {
  const char* op = "fedrec_quant::quantize_delta";
  check_vec(local, op, "local");
  check_vec(global_, op, "global");
  check_vec(residual, op, "residual");
  const int64_t n = local.numel();
  TORCH_CHECK(global_.numel() == n && residual.numel() == n, op, ": local, global and residual must have one length (got ",
              n, ", ", global_.numel(), ", ", residual.numel(), ")");
  TORCH_CHECK(n >= 1 && n < (int64_t(1) << 31), op, ": 1 <= n < 2^31 (got n ", n, ")");
  TORCH_CHECK(bits == 8 || bits == 4, op, ": bits must be 8 or 4 (got ", bits, ")");
  TORCH_CHECK(local.device() == residual.device() && global_.device() == residual.device(), op,
              ": local, global and residual must be on one device");
  TORCH_CHECK(!overlaps(residual, local) && !overlaps(residual, global_), op,
              ": residual must not overlap local or global");
  TORCH_CHECK(residual.is_cuda(), op, ": local, global and residual must be device tensors");
  const c10::DeviceGuard g(residual.device());
  auto codes = at::empty({(n * bits + 7) / 8}, residual.options().dtype(at::kByte));
  auto scales = at::empty({(n + 255) / 256}, residual.options());
  const int rc = fr_quantize_delta(local.data_ptr<float>(), global_.data_ptr<float>(), residual.data_ptr<float>(),
                                   codes.data_ptr<uint8_t>(), scales.data_ptr<float>(), (long)n, (int)bits,
                                   (unsigned long long)seed, (unsigned long long)offset, cur_stream());
  TORCH_CHECK(rc == 0, op, ": unsupported shape (code ", rc, ")");
  return {codes, scales};
}

// ---- base + (sum over clients of weights[c] * (q[c] * scale[c])) / sum(weights) (quant_delta.hip):
// finite scales are the CALLER's check (ops.reference.quant_upload_check); the kernel stays in bounds
// for any content
at::Tensor dequant_combine(const at::Tensor& base, const at::Tensor& codes, const at::Tensor& scales,
                           const at::Tensor& weights, int64_t bits) {
  const char* op = "fedrec_quant::dequant_combine";
  check_vec(base, op, "base");
  TORCH_CHECK(codes.scalar_type() == at::kByte, op, ": codes must be uint8");
  TORCH_CHECK(scales.scalar_type() == at::kFloat, op, ": scales must be fp32");
  TORCH_CHECK(codes.dim() == 2 && scales.dim() == 2, op, ": codes [W, nbytes] and scales [W, nb]");
  TORCH_CHECK(codes.is_contiguous() && scales.is_contiguous(), op, ": codes and scales must be contiguous");
  check_vec(weights, op, "weights");
  const int64_t n = base.numel(), W = codes.size(0);
  TORCH_CHECK(n >= 1 && n < (int64_t(1) << 31), op, ": 1 <= n < 2^31 (got n ", n, ")");
  TORCH_CHECK(bits == 8 || bits == 4, op, ": bits must be 8 or 4 (got ", bits, ")");
  TORCH_CHECK(W >= 1 && W <= 65536 && weights.numel() == W && scales.size(0) == W, op,
              ": 1 <= W <= 65536, scales [W, nb] and weights [W] (got W ", W, ", scales ", scales.size(0), ", weights ",
              weights.numel(), ")");
  const int64_t nbytes = (n * bits + 7) / 8, nb = (n + 255) / 256;
  TORCH_CHECK(codes.size(1) == nbytes && scales.size(1) == nb, op, ": n ", n, " at ", bits, " bits takes codes [W, ", nbytes,
              "] and scales [W, ", nb, "] (got ", codes.size(1), ", ", scales.size(1), ")");
  TORCH_CHECK(codes.device() == base.device() && scales.device() == base.device() && weights.device() == base.device(), op,
              ": base, codes, scales and weights must be on one device");
  TORCH_CHECK(base.is_cuda(), op, ": base, codes, scales and weights must be device tensors");
  const c10::DeviceGuard g(base.device());
  auto out = at::empty_like(base);
  const int rc = fr_dequant_combine(base.data_ptr<float>(), codes.data_ptr<uint8_t>(), scales.data_ptr<float>(),
                                    weights.data_ptr<float>(), out.data_ptr<float>(), (int)W, (long)n, (int)bits, cur_stream());
  TORCH_CHECK(rc == 0, op, ": unsupported shape (code ", rc, ")");
  return out;
}

}  // namespace

// registered for every backend, as fedrec_sparse is: a host tensor reaches the checks above and fails the
// device check last (ops.quantize_delta / ops.dequant_combine send host tensors to the torch oracles)
TORCH_LIBRARY_FRAGMENT(fedrec_quant, m) {
  m.def("quantize_delta(Tensor local, Tensor global_, Tensor(a!) residual, int bits, int seed, int offset) -> (Tensor, Tensor)",
        &quantize_delta);
  m.def("dequant_combine(Tensor base, Tensor codes, Tensor scales, Tensor weights, int bits) -> Tensor", &dequant_combine);
}
