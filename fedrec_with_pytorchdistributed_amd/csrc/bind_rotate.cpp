// fedrec_rotate ops: randomized-Hadamard rotation in front of the block quantiser (rotate_delta.hip).  A namespace of
// its own, as fedrec_quant, fedrec_sparse, fedrec_lowrank and fedrec_sketch are.  n_pad = 4096 ceil(n / 4096).
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

// 1 <= n with n_pad < 2^31 -> n_pad
int64_t pad_of(int64_t n, const char* op) {
  TORCH_CHECK(n >= 1 && n <= (int64_t(1) << 31) - CHUNK, op, ": 1 <= n <= 2^31 - 4096 (got n ", n, ")");
  return (n + CHUNK - 1) / CHUNK * CHUNK;
}

void check_bits(int64_t bits, const char* op) {
  TORCH_CHECK(bits == 8 || bits == 4, op, ": bits must be 8 or 4 (got ", bits, ")");
}

// ---- forward: x [n] -> [n_pad]; inverse: x [n_pad] -> [n] (n: the length to take, 0 = all of it)
at::Tensor rotate(const at::Tensor& x, int64_t seed, bool inverse, int64_t n) {
  const char* op = "fedrec_rotate::rotate";
  check_vec(x, op, "x");
  int64_t n_out;
  if (inverse) {
    TORCH_CHECK(x.numel() >= CHUNK && x.numel() % CHUNK == 0, op, ": the inverse takes whole chunks of 4096 (got ", x.numel(), ")");
    n = n ? n : x.numel();
    TORCH_CHECK(pad_of(n, op) == x.numel(), op, ": n ", n, " does not pad to x's ", x.numel(), " coordinates");
    n_out = n;
  } else {
    TORCH_CHECK(n == 0 || n == x.numel(), op, ": n is the inverse's (got ", n, " for x of ", x.numel(), ")");
    n = x.numel();
    n_out = pad_of(n, op);
  }
  TORCH_CHECK(x.is_cuda(), op, ": x must be a device tensor");
  const c10::DeviceGuard g(x.device());
  auto out = at::empty({n_out}, x.options());
  const int rc = fr_rotate(x.data_ptr<float>(), out.data_ptr<float>(), (long)n, inverse ? 1 : 0, (unsigned long long)seed, cur_stream());
  TORCH_CHECK(rc == 0, op, ": unsupported shape (code ", rc, ")");
  return out;
}

// ---- the block quantiser's codes of rotate(local - global) + residual_rot: -> (codes uint8 [n_pad bits / 8], scales
// fp32 [n_pad / 256]); residual_rot [n_pad] keeps the quantisation error, in the rotated domain
Tensor2 quantize(const at::Tensor& local, const at::Tensor& global_, at::Tensor& residual, int64_t bits, int64_t seed,
                 int64_t offset) {
  const char* op = "fedrec_rotate::quantize";
  check_vec(local, op, "local");
  check_vec(global_, op, "global");
  check_vec(residual, op, "residual_rot");
  const int64_t n = local.numel();
  TORCH_CHECK(global_.numel() == n, op, ": local and global must have one length (got ", n, ", ", global_.numel(), ")");
  const int64_t n_pad = pad_of(n, op);
  TORCH_CHECK(residual.numel() == n_pad, op, ": residual_rot must have the ", n_pad, " coordinates n ", n, " pads to (got ",
              residual.numel(), ")");
  check_bits(bits, op);
  TORCH_CHECK(local.device() == residual.device() && global_.device() == residual.device(), op,
              ": local, global and residual_rot must be on one device");
  TORCH_CHECK(!overlaps(residual, local) && !overlaps(residual, global_), op, ": residual_rot must not overlap local or global");
  TORCH_CHECK(residual.is_cuda(), op, ": local, global and residual_rot must be device tensors");
  const c10::DeviceGuard g(residual.device());
  auto codes = at::empty({n_pad * bits / 8}, residual.options().dtype(at::kByte));
  auto scales = at::empty({n_pad / 256}, residual.options());
  const int rc = fr_rotate_quantize(local.data_ptr<float>(), global_.data_ptr<float>(), residual.data_ptr<float>(),
                                    codes.data_ptr<uint8_t>(), scales.data_ptr<float>(), (long)n, (int)bits,
                                    (unsigned long long)seed, (unsigned long long)offset, cur_stream());
  TORCH_CHECK(rc == 0, op, ": unsupported shape (code ", rc, ")");
  return {codes, scales};
}

// ---- base + the inverse rotation of (sum over clients of weights[c] * (q[c] * scale[c])) / sum(weights): finite
// scales are the CALLER's check (ops.reference.quant_upload_check); the kernel stays in bounds for any content
at::Tensor combine(const at::Tensor& base, const at::Tensor& codes, const at::Tensor& scales, const at::Tensor& weights,
                   int64_t bits, int64_t seed) {
  const char* op = "fedrec_rotate::combine";
  check_vec(base, op, "base");
  TORCH_CHECK(codes.scalar_type() == at::kByte, op, ": codes must be uint8");
  TORCH_CHECK(scales.scalar_type() == at::kFloat, op, ": scales must be fp32");
  TORCH_CHECK(codes.dim() == 2 && scales.dim() == 2, op, ": codes [W, nbytes] and scales [W, nb]");
  TORCH_CHECK(codes.is_contiguous() && scales.is_contiguous(), op, ": codes and scales must be contiguous");
  check_vec(weights, op, "weights");
  const int64_t n = base.numel(), W = codes.size(0);
  const int64_t n_pad = pad_of(n, op);
  check_bits(bits, op);
  TORCH_CHECK(W >= 1 && W <= 65536 && weights.numel() == W && scales.size(0) == W, op,
              ": 1 <= W <= 65536, scales [W, nb] and weights [W] (got W ", W, ", scales ", scales.size(0), ", weights ",
              weights.numel(), ")");
  const int64_t nbytes = n_pad * bits / 8, nb = n_pad / 256;
  TORCH_CHECK(codes.size(1) == nbytes && scales.size(1) == nb, op, ": n ", n, " at ", bits, " bits takes codes [W, ", nbytes,
              "] and scales [W, ", nb, "] (got ", codes.size(1), ", ", scales.size(1), ")");
  TORCH_CHECK(codes.device() == base.device() && scales.device() == base.device() && weights.device() == base.device(), op,
              ": base, codes, scales and weights must be on one device");
  TORCH_CHECK(base.is_cuda(), op, ": base, codes, scales and weights must be device tensors");
  const c10::DeviceGuard g(base.device());
  auto out = at::empty_like(base);
  const int rc = fr_rotate_combine(base.data_ptr<float>(), codes.data_ptr<uint8_t>(), scales.data_ptr<float>(),
                                   weights.data_ptr<float>(), out.data_ptr<float>(), (int)W, (long)n, (int)bits,
                                   (unsigned long long)seed, cur_stream());
  TORCH_CHECK(rc == 0, op, ": unsupported shape (code ", rc, ")");
  return out;
}

}  // namespace

// registered for every backend, as fedrec_quant is: a host tensor reaches the checks above and fails the device check
// last (ops.rotate* send host tensors to the torch oracles)
TORCH_LIBRARY_FRAGMENT(fedrec_rotate, m) {
  m.def("rotate(Tensor x, int seed, bool inverse, int n) -> Tensor", &rotate);
  m.def("quantize(Tensor local, Tensor global_, Tensor(a!) residual_rot, int bits, int seed, int offset) -> (Tensor, Tensor)",
        &quantize);
  m.def("combine(Tensor base, Tensor codes, Tensor scales, Tensor weights, int bits, int seed) -> Tensor", &combine);
}
