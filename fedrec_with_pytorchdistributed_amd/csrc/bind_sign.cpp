// fedrec_sign ops: 1-bit scaled-sign uploads with error feedback (sign_delta.hip) and their rotated forms (the
// rotate_sign_* kernels of rotate_delta.hip).  A namespace of its own, as fedrec_quant and fedrec_rotate are.
// n_pad = 4096 ceil(n / 4096).
#include "binding_util.h"

namespace {

constexpr int64_t CHUNK = 4096;

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

// the coordinates the codes run over: n itself (1 <= n < 2^31), or rotated n_pad (1 <= n <= 2^31 - 4096)
int64_t coded(int64_t n, bool rotated, const char* op) {
  if (!rotated) {
    TORCH_CHECK(n >= 1 && n < (int64_t(1) << 31), op, ": 1 <= n < 2^31 (got n ", n, ")");
    return n;
  }
  TORCH_CHECK(n >= 1 && n <= (int64_t(1) << 31) - CHUNK, op, ": 1 <= n <= 2^31 - 4096 (got n ", n, ")");
  return (n + CHUNK - 1) / CHUNK * CHUNK;
}

// what quantize and rotate_quantize check alike, device last -> the coordinates coded
int64_t check_quantize(const at::Tensor& local, const at::Tensor& global_, const at::Tensor& residual, bool rotated,
                       const char* op) {
  const char* rname = rotated ? "residual_rot" : "residual";
  check_vec(local, op, "local");
  check_vec(global_, op, "global");
  check_vec(residual, op, rname);
  const int64_t n = local.numel();
  TORCH_CHECK(global_.numel() == n, op, ": local and global must have one length (got ", n, ", ", global_.numel(), ")");
  const int64_t m = coded(n, rotated, op);
  TORCH_CHECK(residual.numel() == m, op, ": ", rname, " must have ", m, " coordinates for n ", n, " (got ", residual.numel(), ")");
  TORCH_CHECK(local.device() == residual.device() && global_.device() == residual.device(), op, ": local, global and ",
              rname, " must be on one device");
  TORCH_CHECK(!overlaps(residual, local) && !overlaps(residual, global_), op, ": ", rname, " must not overlap local or global");
  TORCH_CHECK(residual.is_cuda(), op, ": local, global and ", rname, " must be device tensors");
  return m;
}

// what combine and rotate_combine check alike, device last
void check_combine(const at::Tensor& base, const at::Tensor& codes, const at::Tensor& scales, const at::Tensor& weights,
                   bool rotated, const char* op) {
  check_vec(base, op, "base");
  TORCH_CHECK(codes.scalar_type() == at::kByte, op, ": codes must be uint8");
  TORCH_CHECK(scales.scalar_type() == at::kFloat, op, ": scales must be fp32");
  TORCH_CHECK(codes.dim() == 2 && scales.dim() == 2, op, ": codes [W, nbytes] and scales [W, nb]");
  TORCH_CHECK(codes.is_contiguous() && scales.is_contiguous(), op, ": codes and scales must be contiguous");
  check_vec(weights, op, "weights");
  const int64_t n = base.numel(), W = codes.size(0);
  const int64_t m = coded(n, rotated, op);
  TORCH_CHECK(W >= 1 && W <= 65536 && weights.numel() == W && scales.size(0) == W, op,
              ": 1 <= W <= 65536, scales [W, nb] and weights [W] (got W ", W, ", scales ", scales.size(0), ", weights ",
              weights.numel(), ")");
  const int64_t nbytes = (m + 7) / 8, nb = (m + 255) / 256;
  TORCH_CHECK(codes.size(1) == nbytes && scales.size(1) == nb, op, ": n ", n, " takes codes [W, ", nbytes,
              "] and scales [W, ", nb, "] (got ", codes.size(1), ", ", scales.size(1), ")");
  TORCH_CHECK(codes.device() == base.device() && scales.device() == base.device() && weights.device() == base.device(), op,
              ": base, codes, scales and weights must be on one device");
  TORCH_CHECK(base.is_cuda(), op, ": base, codes, scales and weights must be device tensors");
}

// ---- the sign bits of a = (local - global) + residual and one mean magnitude per 256 coordinates (sign_delta.hip):
// -> (codes uint8 [ceil(n / 8)], scales fp32 [ceil(n / 256)]); residual keeps a - copysign(scale, a)
Tensor2 quantize(const at::Tensor& local, const at::Tensor& global_, at::Tensor& residual) {
  const char* op = "fedrec_sign::quantize";
  const int64_t n = check_quantize(local, global_, residual, false, op);
  const c10::DeviceGuard g(residual.device());
  auto codes = at::empty({(n + 7) / 8}, residual.options().dtype(at::kByte));
  auto scales = at::empty({(n + 255) / 256}, residual.options());
  const int rc = fr_sign_quantize(local.data_ptr<float>(), global_.data_ptr<float>(), residual.data_ptr<float>(),
                                  codes.data_ptr<uint8_t>(), scales.data_ptr<float>(), (long)n, cur_stream());
  TORCH_CHECK(rc == 0, op, ": unsupported shape (code ", rc, ")");
  return {codes, scales};
}

// ---- base + (sum over clients of +-(weights[c] * scale[c])) / sum(weights) (sign_delta.hip): finite scales are the
// CALLER's check (ops.reference.quant_upload_check); the kernel stays in bounds for any content
at::Tensor combine(const at::Tensor& base, const at::Tensor& codes, const at::Tensor& scales, const at::Tensor& weights) {
  const char* op = "fedrec_sign::combine";
  check_combine(base, codes, scales, weights, false, op);
  const c10::DeviceGuard g(base.device());
  auto out = at::empty_like(base);
  const int rc = fr_sign_combine(base.data_ptr<float>(), codes.data_ptr<uint8_t>(), scales.data_ptr<float>(),
                                 weights.data_ptr<float>(), out.data_ptr<float>(), (int)codes.size(0), (long)base.numel(),
                                 cur_stream());
  TORCH_CHECK(rc == 0, op, ": unsupported shape (code ", rc, ")");
  return out;
}

// ---- quantize of rotate(local - global) + residual_rot over n_pad coordinates in one launch (rotate_delta.hip):
// -> (codes uint8 [n_pad / 8], scales fp32 [n_pad / 256]); residual_rot [n_pad] stays in the rotated domain
Tensor2 rotate_quantize(const at::Tensor& local, const at::Tensor& global_, at::Tensor& residual, int64_t seed) {
  const char* op = "fedrec_sign::rotate_quantize";
  const int64_t n_pad = check_quantize(local, global_, residual, true, op);
  const c10::DeviceGuard g(residual.device());
  auto codes = at::empty({n_pad / 8}, residual.options().dtype(at::kByte));
  auto scales = at::empty({n_pad / 256}, residual.options());
  const int rc = fr_rotate_sign_quantize(local.data_ptr<float>(), global_.data_ptr<float>(), residual.data_ptr<float>(),
                                         codes.data_ptr<uint8_t>(), scales.data_ptr<float>(), (long)local.numel(),
                                         (unsigned long long)seed, cur_stream());
  TORCH_CHECK(rc == 0, op, ": unsupported shape (code ", rc, ")");
  return {codes, scales};
}

// ---- base + the inverse rotation of combine's mean over n_pad rotated coordinates (rotate_delta.hip)
at::Tensor rotate_combine(const at::Tensor& base, const at::Tensor& codes, const at::Tensor& scales,
                          const at::Tensor& weights, int64_t seed) {
  const char* op = "fedrec_sign::rotate_combine";
  check_combine(base, codes, scales, weights, true, op);
  const c10::DeviceGuard g(base.device());
  auto out = at::empty_like(base);
  const int rc = fr_rotate_sign_combine(base.data_ptr<float>(), codes.data_ptr<uint8_t>(), scales.data_ptr<float>(),
                                        weights.data_ptr<float>(), out.data_ptr<float>(), (int)codes.size(0),
                                        (long)base.numel(), (unsigned long long)seed, cur_stream());
  TORCH_CHECK(rc == 0, op, ": unsupported shape (code ", rc, ")");
  return out;
}

}  // namespace

// registered for every backend, as fedrec_quant is: a host tensor reaches the checks above and fails the device check
// last (ops.sign_* send host tensors to the torch oracles)
TORCH_LIBRARY_FRAGMENT(fedrec_sign, m) {
  m.def("quantize(Tensor local, Tensor global_, Tensor(a!) residual) -> (Tensor, Tensor)", &quantize);
  m.def("combine(Tensor base, Tensor codes, Tensor scales, Tensor weights) -> Tensor", &combine);
  m.def("rotate_quantize(Tensor local, Tensor global_, Tensor(a!) residual_rot, int seed) -> (Tensor, Tensor)", &rotate_quantize);
  m.def("rotate_combine(Tensor base, Tensor codes, Tensor scales, Tensor weights, int seed) -> Tensor", &rotate_combine);
}
