// fedrec_dp ops: client-level DP on a round delta, clip + noise (dp_clip.hip).  A namespace of its own: the
// fedrec::, fedrec_eval::, fedrec_rerank::, fedrec_agg::, fedrec_krum::, fedrec_geomed::, fedrec_sparse:: and
// fedrec_quant:: op sets are pinned as they stand (tests/golden/op_schemas*.txt).
#include "binding_util.h"

namespace {

// dtype, shape, contiguity and bounds first (they do not depend on where the tensors live); the messages
// are those of ops/reference.py dp_*_check
int64_t check_pair(const at::Tensor& local, const at::Tensor& base, const char* op) {
  TORCH_CHECK(local.scalar_type() == at::kFloat && base.scalar_type() == at::kFloat, op, ": local and base must be fp32");
  TORCH_CHECK(local.dim() == 1 && base.dim() == 1, op, ": local [n] and base [n] (got ", local.dim(), " and ", base.dim(),
              " dims)");
  TORCH_CHECK(local.is_contiguous() && base.is_contiguous(), op, ": local and base must be contiguous");
  const int64_t n = local.numel();
  TORCH_CHECK(base.numel() == n, op, ": local and base must have one length (got ", n, ", ", base.numel(), ")");
  TORCH_CHECK(n >= 1, op, ": n >= 1 (got n ", n, ")");
  TORCH_CHECK(local.device() == base.device(), op, ": local and base must be on one device");
  return n;
}

// ---- || local - base ||^2 in fp64, in a fixed order, into a 16-byte device state (dp_clip.hip): int32 [4]
// holding sq (fp64), the clip scale s (fp32) and clipped (int32); the last two are clip_noise's to fill in
at::Tensor delta_sqnorm(const at::Tensor& local, const at::Tensor& base, int64_t max_blocks) {
  const char* op = "fedrec_dp::delta_sqnorm";
  const int64_t n = check_pair(local, base, op);
  TORCH_CHECK(max_blocks >= 0 && max_blocks < (int64_t(1) << 31), op, ": max_blocks >= 0 (got ", max_blocks, ")");
  TORCH_CHECK(local.is_cuda(), op, ": local and base must be device tensors");
  const c10::DeviceGuard g(local.device());
  auto part = at::empty({(int64_t)fr_dp_sqnorm_ws((long)n)}, local.options().dtype(at::kDouble));
  auto state = at::empty({4}, local.options().dtype(at::kInt));
  const int rc = fr_dp_delta_sqnorm(local.data_ptr<float>(), base.data_ptr<float>(), part.data_ptr<double>(),
                                    state.data_ptr(), (long)n, (int)max_blocks, cur_stream());
  TORCH_CHECK(rc == 0, op, ": unsupported shape (code ", rc, ")");
  return state;
}

// ---- base + s (local - base) + std z with s from the state's sq (dp_clip.hip); s and clipped go into state
at::Tensor clip_noise(const at::Tensor& local, const at::Tensor& base, at::Tensor& state, double clip, double std_,
                      int64_t seed, int64_t offset) {
  const char* op = "fedrec_dp::clip_noise";
  const int64_t n = check_pair(local, base, op);
  TORCH_CHECK(state.scalar_type() == at::kInt && state.dim() == 1 && state.numel() == 4 && state.is_contiguous(), op,
              ": state must be the int32 [4] of delta_sqnorm");
  TORCH_CHECK(clip > 0.0, op, ": clip > 0 (got ", clip, ")");
  TORCH_CHECK(std_ >= 0.0 && (double)(float)std_ < (double)INFINITY, op, ": 0 <= std < inf (got ", std_, ")");
  TORCH_CHECK(local.device() == state.device(), op, ": local, base and state must be on one device");
  TORCH_CHECK(local.is_cuda(), op, ": local, base and state must be device tensors");
  const c10::DeviceGuard g(local.device());
  auto out = at::empty({n}, local.options());
  const int rc = fr_dp_clip_noise(local.data_ptr<float>(), base.data_ptr<float>(), out.data_ptr<float>(), state.data_ptr(),
                                  (long)n, clip, (float)std_, (unsigned long long)seed, (unsigned long long)offset,
                                  cur_stream());
  TORCH_CHECK(rc == 0, op, ": unsupported argument (code ", rc, ")");
  return out;
}

}  // namespace

// registered for every backend, as fedrec_krum is: a host tensor reaches the checks above and fails the
// device check last (ops.dp_* send host tensors to the torch oracles before they get here)
TORCH_LIBRARY_FRAGMENT(fedrec_dp, m) {
  m.def("delta_sqnorm(Tensor local, Tensor base, int max_blocks=0) -> Tensor", &delta_sqnorm);
  m.def("clip_noise(Tensor local, Tensor base, Tensor(a!) state, float clip, float std, int seed, int offset) -> Tensor",
        &clip_noise);
}
