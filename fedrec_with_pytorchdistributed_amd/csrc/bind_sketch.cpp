// fedrec_sketch ops: count-sketch (FetchSGD) uploads (sketch_delta.hip).  A namespace of its own, as fedrec_quant,
// fedrec_sparse and fedrec_lowrank are.  The hash comes as its words, the int32 [nb, 8, 4] plan of ops/reference.py
// sketch_plan; the kernels mask every index they derive from it, so any content is memory-safe.
#include "binding_util.h"

namespace {

constexpr int64_t TILE = 1024;

void check_vec(const at::Tensor& t, const char* op, const char* name) {
  TORCH_CHECK(t.scalar_type() == at::kFloat, op, ": ", name, " must be fp32");
  TORCH_CHECK(t.dim() == 1, op, ": ", name, " [n] (got ", t.dim(), " dims)");
  TORCH_CHECK(t.is_contiguous(), op, ": ", name, " must be contiguous");
}

void check_shape(int64_t R, int64_t C, const char* op) {
  TORCH_CHECK(R == 1 || R == 3 || R == 5, op, ": rows must be 1, 3 or 5 (got ", R, ")");
  TORCH_CHECK(C >= TILE && C <= (int64_t(1) << 30) && (C & (C - 1)) == 0, op, ": cols must be a power of two in [", TILE,
              ", 2^30] (got ", C, ")");
}

// the plan of nb blocks on like's device -> nb
int check_plan(const at::Tensor& plan, int64_t nb, const char* op, const at::Tensor& like) {
  TORCH_CHECK(plan.scalar_type() == at::kInt && plan.dim() == 3 && plan.size(0) == nb && plan.size(1) == 8 &&
                  plan.size(2) == 4 && plan.is_contiguous(),
              op, ": plan must be a contiguous int32 [", nb, ", 8, 4] tensor");
  TORCH_CHECK(plan.device() == like.device(), op, ": plan must be on the device of the other tensors");
  return (int)nb;
}

void check_table(const at::Tensor& t, const char* op) {
  TORCH_CHECK(t.scalar_type() == at::kFloat && t.dim() == 2 && t.is_contiguous(), op,
              ": table must be a contiguous fp32 [rows, cols] tensor");
  check_shape(t.size(0), t.size(1), op);
}

at::Tensor delta(const at::Tensor& local, const at::Tensor& global_, const at::Tensor& plan, int64_t R, int64_t C) {
  const char* op = "fedrec_sketch::delta";
  check_vec(local, op, "local");
  check_vec(global_, op, "global");
  const int64_t n = local.numel();
  TORCH_CHECK(global_.numel() == n, op, ": local and global must have one length (got ", n, ", ", global_.numel(), ")");
  TORCH_CHECK(n >= 1 && n < (int64_t(1) << 31), op, ": 1 <= n < 2^31 (got n ", n, ")");
  check_shape(R, C, op);
  TORCH_CHECK(global_.device() == local.device(), op, ": local and global must be on one device");
  const int nb = check_plan(plan, (n + C - 1) / C, op, local);
  TORCH_CHECK(local.is_cuda(), op, ": the tensors must be device tensors");
  const c10::DeviceGuard g(local.device());
  auto S = at::empty({R, C}, local.options());
  const int rc = fr_sketch_delta(local.data_ptr<float>(), global_.data_ptr<float>(), plan.data_ptr<int>(),
                                 S.data_ptr<float>(), (long)n, nb, (int)R, (long)C, cur_stream());
  TORCH_CHECK(rc == 0, op, ": unsupported shape (code ", rc, ")");
  return S;
}

at::Tensor estimate(const at::Tensor& table, const at::Tensor& plan, int64_t n) {
  const char* op = "fedrec_sketch::estimate";
  check_table(table, op);
  const int64_t R = table.size(0), C = table.size(1);
  TORCH_CHECK(n >= 1 && n < (int64_t(1) << 31), op, ": 1 <= n < 2^31 (got n ", n, ")");
  const int nb = check_plan(plan, (n + C - 1) / C, op, table);
  TORCH_CHECK(table.is_cuda(), op, ": the tensors must be device tensors");
  const c10::DeviceGuard g(table.device());
  auto est = at::empty({n}, table.options());
  const int rc = fr_sketch_estimate(table.data_ptr<float>(), plan.data_ptr<int>(), est.data_ptr<float>(), (long)n, nb,
                                    (int)R, (long)C, cur_stream());
  TORCH_CHECK(rc == 0, op, ": unsupported shape (code ", rc, ")");
  return est;
}

void accumulate_(at::Tensor& table, const at::Tensor& stack, const at::Tensor& weights) {
  const char* op = "fedrec_sketch::accumulate_";
  TORCH_CHECK(table.scalar_type() == at::kFloat && table.is_contiguous(), op, ": table must be contiguous fp32");
  const int64_t L = table.numel();
  TORCH_CHECK(stack.scalar_type() == at::kFloat && stack.dim() == 2 && stack.is_contiguous() && stack.size(1) == L, op,
              ": stack must be a contiguous fp32 [W, ", L, "] tensor");
  check_vec(weights, op, "weights");
  const int64_t W = stack.size(0);
  TORCH_CHECK(W >= 1 && W <= 32 && weights.numel() == W, op, ": 1 <= W <= 32 and weights [W] (got W ", W, ", weights ",
              weights.numel(), ")");
  TORCH_CHECK(L >= 4 && L % 4 == 0 && L < (int64_t(1) << 31), op, ": the table's length must be a multiple of 4 below 2^31 (got ",
              L, ")");
  TORCH_CHECK(stack.device() == table.device() && weights.device() == table.device(), op,
              ": table, stack and weights must be on one device");
  TORCH_CHECK(table.is_cuda(), op, ": the tensors must be device tensors");
  const c10::DeviceGuard g(table.device());
  const int rc = fr_sketch_accumulate(table.data_ptr<float>(), stack.data_ptr<float>(), weights.data_ptr<float>(), (int)W,
                                      (long)L, cur_stream());
  TORCH_CHECK(rc == 0, op, ": unsupported shape (code ", rc, ")");
}

void clear_(at::Tensor& table, const at::Tensor& idx, const at::Tensor& plan) {
  const char* op = "fedrec_sketch::clear_";
  check_table(table, op);
  TORCH_CHECK(idx.scalar_type() == at::kInt && idx.dim() == 1 && idx.is_contiguous(), op, ": idx must be a contiguous int32 [k] tensor");
  TORCH_CHECK(plan.dim() == 3 && plan.size(0) >= 1 && plan.size(0) * table.size(1) <= (int64_t(1) << 31), op,
              ": the plan's blocks must cover at most 2^31 coordinates");
  const int nb = check_plan(plan, plan.size(0), op, table);
  TORCH_CHECK(idx.device() == table.device(), op, ": idx must be on the device of the other tensors");
  TORCH_CHECK(table.is_cuda(), op, ": the tensors must be device tensors");
  const c10::DeviceGuard g(table.device());
  const int rc = fr_sketch_clear(table.data_ptr<float>(), idx.data_ptr<int>(), plan.data_ptr<int>(), (long)idx.numel(), nb,
                                 (int)table.size(0), (long)table.size(1), cur_stream());
  TORCH_CHECK(rc == 0, op, ": unsupported shape (code ", rc, ")");
}

}  // namespace

// registered for every backend, as fedrec_quant is: a host tensor reaches the checks above and fails the device
// check last (the ops.sketch_* dispatchers send host tensors to the torch oracles)
TORCH_LIBRARY_FRAGMENT(fedrec_sketch, m) {
  m.def("delta(Tensor local, Tensor global_, Tensor plan, int rows, int cols) -> Tensor", &delta);
  m.def("estimate(Tensor table, Tensor plan, int n) -> Tensor", &estimate);
  m.def("accumulate_(Tensor(a!) table, Tensor stack, Tensor weights) -> ()", &accumulate_);
  m.def("clear_(Tensor(a!) table, Tensor idx, Tensor plan) -> ()", &clear_);
}
