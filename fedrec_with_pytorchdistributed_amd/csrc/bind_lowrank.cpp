// fedrec_lowrank ops: low-rank (PowerSGD) uploads with error feedback (lowrank_delta.hip).  A namespace of its
// own, as fedrec_quant and fedrec_sparse are.  The plan's tables (ops/reference.py LowRankPlan) come as int32
// device tensors; the kernels check every table row against the tensors' lengths before they touch memory.
#include "binding_util.h"

namespace {

void check_vec(const at::Tensor& t, const char* op, const char* name, const at::Tensor& like) {
  TORCH_CHECK(t.scalar_type() == at::kFloat, op, ": ", name, " must be fp32");
  TORCH_CHECK(t.dim() == 1, op, ": ", name, " must be 1-D (got ", t.dim(), " dims)");
  TORCH_CHECK(t.is_contiguous(), op, ": ", name, " must be contiguous");
  TORCH_CHECK(t.device() == like.device(), op, ": ", name, " must be on the device of the other tensors");
}

// an int32 [rows, width] table with at least min_rows rows
int check_table(const at::Tensor& t, int64_t width, int64_t min_rows, const char* op, const char* name,
                const at::Tensor& like) {
  TORCH_CHECK(t.scalar_type() == at::kInt && t.dim() == 2 && t.size(1) == width && t.is_contiguous(), op, ": ", name,
              " must be a contiguous int32 [*, ", width, "] table");
  TORCH_CHECK(t.size(0) >= min_rows && t.size(0) < (int64_t(1) << 31), op, ": ", name, " needs at least ", min_rows,
              " rows (got ", t.size(0), ")");
  TORCH_CHECK(t.device() == like.device(), op, ": ", name, " must be on the device of the other tensors");
  return (int)t.size(0);
}

void check_rank(int64_t R, const char* op) {
  TORCH_CHECK(R == 1 || R == 2 || R == 4 || R == 8, op, ": rank must be 1, 2, 4 or 8 (got ", R, ")");
}

// local, global, residual [n] and the payload [L >= F]
int64_t check_round(const at::Tensor& local, const at::Tensor& global_, const at::Tensor& residual,
                    const at::Tensor& payload, int64_t F, const char* op) {
  check_vec(local, op, "local", residual);
  check_vec(global_, op, "global", residual);
  check_vec(residual, op, "residual", residual);
  check_vec(payload, op, "payload", residual);
  const int64_t n = residual.numel();
  TORCH_CHECK(local.numel() == n && global_.numel() == n, op, ": local, global and residual must have one length (got ",
              local.numel(), ", ", global_.numel(), ", ", n, ")");
  TORCH_CHECK(n >= 1 && n < (int64_t(1) << 31), op, ": 1 <= n < 2^31 (got n ", n, ")");
  TORCH_CHECK(F >= 1 && payload.numel() >= F && payload.numel() < (int64_t(1) << 31), op, ": 1 <= factors <= payload length < 2^31 (got ",
              F, ", ", payload.numel(), ")");
  TORCH_CHECK(residual.is_cuda(), op, ": the tensors must be device tensors");
  return n;
}

void project(const at::Tensor& local, const at::Tensor& global_, const at::Tensor& residual, const at::Tensor& basis,
             at::Tensor& payload, const at::Tensor& mats, const at::Tensor& tiles, int64_t R, int64_t max_blocks) {
  const char* op = "fedrec_lowrank::project";
  check_rank(R, op);
  check_vec(basis, op, "basis", residual);
  const int64_t F = basis.numel(), n = check_round(local, global_, residual, payload, F, op);
  const int M = check_table(mats, 4, 1, op, "mats", residual), nt = check_table(tiles, 2, 1, op, "tiles", residual);
  const c10::DeviceGuard g(residual.device());
  const int rc = fr_lowrank_project(local.data_ptr<float>(), global_.data_ptr<float>(), residual.data_ptr<float>(),
                                    basis.data_ptr<float>(), payload.data_ptr<float>(), mats.data_ptr<int>(),
                                    tiles.data_ptr<int>(), nt, M, (int)R, (long)n, (long)F, (int)max_blocks, cur_stream());
  TORCH_CHECK(rc == 0, op, ": unsupported shape (code ", rc, ")");
}

void orth(at::Tensor& payload, const at::Tensor& mats, int64_t R, int64_t F) {
  const char* op = "fedrec_lowrank::orth";
  check_rank(R, op);
  check_vec(payload, op, "payload", payload);
  TORCH_CHECK(F >= 1 && payload.numel() >= F && payload.numel() < (int64_t(1) << 31), op,
              ": 1 <= factors <= payload length < 2^31 (got ", F, ", ", payload.numel(), ")");
  const int M = check_table(mats, 4, 1, op, "mats", payload);
  TORCH_CHECK(payload.is_cuda(), op, ": the tensors must be device tensors");
  const c10::DeviceGuard g(payload.device());
  const int rc = fr_lowrank_orth(payload.data_ptr<float>(), mats.data_ptr<int>(), M, (int)R, (long)F, cur_stream());
  TORCH_CHECK(rc == 0, op, ": unsupported shape (code ", rc, ")");
}

void backproject(const at::Tensor& local, const at::Tensor& global_, const at::Tensor& residual, at::Tensor& payload,
                 const at::Tensor& mats, const at::Tensor& tiles, const at::Tensor& ftiles, int64_t R, int64_t F,
                 int64_t max_blocks) {
  const char* op = "fedrec_lowrank::backproject";
  check_rank(R, op);
  const int64_t n = check_round(local, global_, residual, payload, F, op);
  const int M = check_table(mats, 4, 1, op, "mats", residual), nt = check_table(tiles, 3, 1, op, "tiles", residual),
            nf = check_table(ftiles, 4, 1, op, "ftiles", residual);
  const c10::DeviceGuard g(residual.device());
  auto part = at::empty({(int64_t)nt * 64 * R}, residual.options());
  const int rc = fr_lowrank_backproject(local.data_ptr<float>(), global_.data_ptr<float>(), residual.data_ptr<float>(),
                                        payload.data_ptr<float>(), part.data_ptr<float>(), mats.data_ptr<int>(),
                                        tiles.data_ptr<int>(), nt, ftiles.data_ptr<int>(), nf, M, (int)R, (long)n, (long)F,
                                        (int)max_blocks, cur_stream());
  TORCH_CHECK(rc == 0, op, ": unsupported shape (code ", rc, ")");
}

void residual_(const at::Tensor& local, const at::Tensor& global_, at::Tensor& residual, at::Tensor& payload,
               const at::Tensor& mats, const at::Tensor& rest, const at::Tensor& tiles, int64_t R, int64_t F,
               int64_t max_blocks) {
  const char* op = "fedrec_lowrank::residual";
  check_rank(R, op);
  const int64_t n = check_round(local, global_, residual, payload, F, op);
  const int M = check_table(mats, 4, 1, op, "mats", residual), S = check_table(rest, 3, 0, op, "rest", residual),
            nt = check_table(tiles, 3, 1, op, "tiles", residual);
  const c10::DeviceGuard g(residual.device());
  const int rc = fr_lowrank_residual(local.data_ptr<float>(), global_.data_ptr<float>(), residual.data_ptr<float>(),
                                     payload.data_ptr<float>(), mats.data_ptr<int>(), rest.data_ptr<int>(),
                                     tiles.data_ptr<int>(), nt, M, S, (int)R, (long)n, (long)F, (long)payload.numel(),
                                     (int)max_blocks, cur_stream());
  TORCH_CHECK(rc == 0, op, ": unsupported shape (code ", rc, ")");
}

at::Tensor combine(const at::Tensor& base, const at::Tensor& stack, const at::Tensor& weights, const at::Tensor& mats,
                   const at::Tensor& rest, const at::Tensor& tiles, int64_t R, int64_t F, int64_t max_blocks) {
  const char* op = "fedrec_lowrank::combine";
  check_rank(R, op);
  check_vec(base, op, "base", base);
  check_vec(weights, op, "weights", base);
  TORCH_CHECK(stack.scalar_type() == at::kFloat && stack.dim() == 2 && stack.is_contiguous() &&
                  stack.device() == base.device(),
              op, ": stack must be a contiguous fp32 [W, L] tensor on base's device");
  const int64_t n = base.numel(), W = stack.size(0), L = stack.size(1);
  TORCH_CHECK(n >= 1 && n < (int64_t(1) << 31), op, ": 1 <= n < 2^31 (got n ", n, ")");
  TORCH_CHECK(W >= 1 && W <= 65536 && weights.numel() == W, op, ": 1 <= W <= 65536 and weights [W] (got W ", W,
              ", weights ", weights.numel(), ")");
  TORCH_CHECK(F >= 1 && L >= F && L < (int64_t(1) << 31), op, ": 1 <= factors <= payload length < 2^31 (got ", F, ", ", L,
              ")");
  const int M = check_table(mats, 4, 1, op, "mats", base), S = check_table(rest, 3, 0, op, "rest", base),
            nt = check_table(tiles, 3, 1, op, "tiles", base);
  TORCH_CHECK(base.is_cuda(), op, ": the tensors must be device tensors");
  const c10::DeviceGuard g(base.device());
  auto out = base.clone();  // (a coordinate no tile covers keeps base)
  const int rc = fr_lowrank_combine(base.data_ptr<float>(), stack.data_ptr<float>(), weights.data_ptr<float>(),
                                    out.data_ptr<float>(), mats.data_ptr<int>(), rest.data_ptr<int>(), tiles.data_ptr<int>(),
                                    nt, M, S, (int)R, (int)W, (long)n, (long)F, (long)L, (int)max_blocks, cur_stream());
  TORCH_CHECK(rc == 0, op, ": unsupported shape (code ", rc, ")");
  return out;
}

}  // namespace

// registered for every backend, as fedrec_quant is: a host tensor reaches the checks above and fails the device
// check last (the ops.lowrank_* dispatchers send host tensors to the torch oracles)
TORCH_LIBRARY_FRAGMENT(fedrec_lowrank, m) {
  m.def("project(Tensor local, Tensor global_, Tensor residual, Tensor basis, Tensor(a!) payload, Tensor mats, "
        "Tensor tiles, int rank, int max_blocks=0) -> ()", &project);
  m.def("orth(Tensor(a!) payload, Tensor mats, int rank, int factors) -> ()", &orth);
  m.def("backproject(Tensor local, Tensor global_, Tensor residual, Tensor(a!) payload, Tensor mats, Tensor tiles, "
        "Tensor ftiles, int rank, int factors, int max_blocks=0) -> ()", &backproject);
  m.def("residual(Tensor local, Tensor global_, Tensor(a!) residual, Tensor(b!) payload, Tensor mats, Tensor rest, "
        "Tensor tiles, int rank, int factors, int max_blocks=0) -> ()", &residual_);
  m.def("combine(Tensor base, Tensor stack, Tensor weights, Tensor mats, Tensor rest, Tensor tiles, int rank, "
        "int factors, int max_blocks=0) -> Tensor", &combine);
}
