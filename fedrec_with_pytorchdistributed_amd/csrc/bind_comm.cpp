// fedrec ops of the communication path: the peer-to-peer all-reduce over IPC-mapped buffers
// (ipc_allreduce.hip) and the secure-aggregation masks (secagg.hip).
#include "binding_util.h"

namespace {

std::tuple<int64_t, at::Tensor> ipc_create(int64_t cap) {
  auto h = at::empty({64}, at::TensorOptions().dtype(at::kByte));
  const int id = fr_ipc_create((long)cap, h.data_ptr());
  TORCH_CHECK(id >= 0, "fedrec::ipc_create failed (code ", id, ")");
  return {id, h};
}

void ipc_open(int64_t id, const at::Tensor& handles, int64_t me, int64_t W, const OptTensor& local) {
  TORCH_CHECK(!handles.is_cuda() && handles.scalar_type() == at::kByte && handles.numel() == 64 * W &&
                  handles.is_contiguous(),
              "fedrec::ipc_open: handles uint8 [W*64] on the host");
  const long long* lp = nullptr;
  at::Tensor lc;
  if (local.has_value()) {
    lc = local->to(at::kLong).contiguous();
    TORCH_CHECK(!lc.is_cuda() && lc.numel() == W, "fedrec::ipc_open: local_ptrs int64 [W] on the host");
    lp = (const long long*)lc.data_ptr<int64_t>();
  }
  const int rc = fr_ipc_open((int)id, handles.data_ptr(), (int)me, (int)W, lp);
  TORCH_CHECK(rc == 0, "fedrec::ipc_open failed (code ", rc, ")");
}

// the context's status word as a device tensor view (no ownership; valid until ipc_destroy):
// the in-graph Adam reads it to skip the update of a step whose all-reduce timed out
at::Tensor ipc_status_word(int64_t id) {
  int* st = fr_ipc_status((int)id);
  TORCH_CHECK(st != nullptr, "fedrec::ipc_status_word: bad id");
  int dev = 0;
  TORCH_CHECK(hipPointerGetAttribute(&dev, HIP_POINTER_ATTRIBUTE_DEVICE_ORDINAL, (hipDeviceptr_t)st) == hipSuccess,
              "fedrec::ipc_status_word: pointer attribute");
  return at::from_blob(st, {1}, at::TensorOptions().dtype(at::kInt).device(at::Device(at::kCUDA, dev)));
}

int64_t ipc_status(int64_t id) {  // device -> host read (tests / diagnostics only)
  int* st = fr_ipc_status((int)id);
  TORCH_CHECK(st != nullptr, "fedrec::ipc_status: bad id");
  int v = 0;
  TORCH_CHECK(hipMemcpy(&v, st, sizeof(int), hipMemcpyDeviceToHost) == hipSuccess, "fedrec::ipc_status: copy");
  return v;
}

void ipc_allreduce_(int64_t id, at::Tensor x, int64_t epoch, int64_t mode, int64_t blocks, double timeout_s) {
  check_dev(x, "x");
  TORCH_CHECK(x.is_contiguous() && (x.scalar_type() == at::kFloat || x.scalar_type() == at::kInt) && x.numel() % 4 == 0,
              "fedrec::ipc_allreduce_: contiguous fp32 / int32, numel % 4 == 0");
  const c10::DeviceGuard g(x.device());
  check_rc(fr_ipc_allreduce((int)id, x.data_ptr(), (long)x.numel(), x.scalar_type() == at::kInt ? 1 : 0,
                            (long long)epoch, (int)mode, (int)blocks, timeout_s, cur_stream()),
           "ipc_allreduce_");
}

// single-process rehearsal: every rank's context + tensor, one launch playing all ranks
void ipc_allreduce_local_(at::IntArrayRef ids, at::TensorList xs, int64_t epoch, int64_t mode, int64_t blocks,
                          double timeout_s) {
  TORCH_CHECK(ids.size() == xs.size() && !xs.empty() && xs.size() <= 16, "fedrec::ipc_allreduce_local_: W tensors");
  std::vector<int> iv(ids.begin(), ids.end());
  std::vector<void*> pv;
  for (const auto& x : xs) {
    check_dev(x, "x");
    TORCH_CHECK(x.is_contiguous() && x.scalar_type() == xs[0].scalar_type() && x.numel() == xs[0].numel() &&
                    (x.scalar_type() == at::kFloat || x.scalar_type() == at::kInt) && x.numel() % 4 == 0,
                "fedrec::ipc_allreduce_local_: contiguous fp32 / int32 tensors of one size, numel % 4 == 0");
    pv.push_back(x.data_ptr());
  }
  const c10::DeviceGuard g(xs[0].device());
  check_rc(fr_ipc_allreduce_local(iv.data(), pv.data(), (int)xs.size(), (long)xs[0].numel(),
                                  xs[0].scalar_type() == at::kInt ? 1 : 0, (long long)epoch, (int)mode, (int)blocks,
                                  timeout_s, cur_stream()),
           "ipc_allreduce_local_");
}

// ---- secure aggregation (secagg.hip) -----------------------------------------------------------
std::tuple<at::Tensor> secagg_mask(const at::Tensor& x, const at::Tensor& seeds, const at::Tensor& signs, double scale,
                                   double clipv, int64_t round) {
  check_dev(x, "x");
  TORCH_CHECK(x.scalar_type() == at::kFloat, "fedrec::secagg_mask: fp32");
  const c10::DeviceGuard g(x.device());
  auto sd = seeds.to(x.device(), at::kLong).contiguous();
  auto sg = signs.to(x.device(), at::kInt).contiguous();
  auto out = at::empty(x.sizes(), x.options().dtype(at::kInt));
  check_rc(fr_secagg_mask(x.data_ptr<float>(), out.data_ptr<int>(), (long)x.numel(), (float)scale, (float)clipv,
                          (const unsigned long long*)sd.data_ptr<int64_t>(), sg.data_ptr<int>(), (int)sd.numel(),
                          (unsigned long long)round, cur_stream()),
           "secagg_mask");
  return {out};
}

at::Tensor secagg_unmask(const at::Tensor& x, double inv_scale) {
  check_dev(x, "x");
  TORCH_CHECK(x.scalar_type() == at::kInt, "fedrec::secagg_unmask: int32");
  const c10::DeviceGuard g(x.device());
  auto out = at::empty(x.sizes(), x.options().dtype(at::kFloat));
  check_rc(fr_secagg_unmask(x.data_ptr<int>(), out.data_ptr<float>(), (long)x.numel(), (float)inv_scale, cur_stream()),
           "secagg_unmask");
  return out;
}

// exact secure aggregation (parallel/secagg.py ExactMasker): a masked exponent histogram agrees on
// the fixed-point bound (one tiny all-reduce), then the masked payload -- no host read, no sync
at::Tensor secagg_hist(const at::Tensor& x, const at::Tensor& seeds, const at::Tensor& signs, int64_t round) {
  check_dev(x, "x");
  check_dev(seeds, "seeds");
  check_dev(signs, "signs");
  TORCH_CHECK(x.scalar_type() == at::kFloat && x.is_contiguous() && seeds.scalar_type() == at::kLong &&
                  signs.scalar_type() == at::kInt && seeds.numel() == signs.numel(),
              "fedrec::secagg_hist: dtypes");
  const c10::DeviceGuard g(x.device());
  auto scratch = at::zeros({2}, x.options().dtype(at::kInt));
  auto out = at::empty({256}, x.options().dtype(at::kInt));
  check_rc(fr_secagg_hist(x.data_ptr<float>(), (long)x.numel(), (unsigned*)scratch.data_ptr<int>(), out.data_ptr<int>(),
                          (const unsigned long long*)seeds.data_ptr<int64_t>(), signs.data_ptr<int>(),
                          (int)seeds.numel(), (unsigned long long)round, cur_stream()),
           "secagg_hist");
  return out;
}

at::Tensor secagg_mask_exact(const at::Tensor& x, const at::Tensor& seeds, const at::Tensor& signs,
                             const at::Tensor& hist, int64_t W, int64_t round) {
  check_dev(x, "x");
  check_dev(seeds, "seeds");
  check_dev(signs, "signs");
  check_dev(hist, "hist");
  TORCH_CHECK(x.scalar_type() == at::kFloat && x.is_contiguous() && hist.scalar_type() == at::kInt &&
                  hist.numel() == 256 && seeds.scalar_type() == at::kLong && signs.scalar_type() == at::kInt &&
                  seeds.numel() == signs.numel(),
              "fedrec::secagg_mask_exact: dtypes");
  const c10::DeviceGuard g(x.device());
  auto out = at::empty(x.sizes(), x.options().dtype(at::kInt));
  check_rc(fr_secagg_mask_exact(x.data_ptr<float>(), out.data_ptr<int>(), (long)x.numel(), hist.data_ptr<int>(),
                                (int)W, (const unsigned long long*)seeds.data_ptr<int64_t>(), signs.data_ptr<int>(),
                                (int)seeds.numel(), (unsigned long long)round, cur_stream()),
           "secagg_mask_exact");
  return out;
}

void secagg_unmask_exact_(const at::Tensor& q, const at::Tensor& hist, int64_t W, at::Tensor out) {
  check_dev(q, "q");
  check_dev(hist, "hist");
  check_dev(out, "out");
  TORCH_CHECK(q.scalar_type() == at::kInt && out.scalar_type() == at::kFloat && q.numel() == out.numel() &&
                  hist.scalar_type() == at::kInt && hist.numel() == 256 && out.is_contiguous(),
              "fedrec::secagg_unmask_exact_");
  const c10::DeviceGuard g(q.device());
  check_rc(fr_secagg_unmask_exact(q.data_ptr<int>(), out.data_ptr<float>(), (long)q.numel(), hist.data_ptr<int>(),
                                  (int)W, cur_stream()),
           "secagg_unmask_exact_");
}

}  // namespace

TORCH_LIBRARY_FRAGMENT(fedrec, m) {
  m.def("ipc_create(int cap) -> (int, Tensor)", &ipc_create);
  m.def("ipc_open(int id, Tensor handles, int me, int W, Tensor? local_ptrs) -> ()", &ipc_open);
  m.def("ipc_region(int id) -> int", [](int64_t id) { return (int64_t)fr_ipc_region((int)id); });
  m.def("ipc_status(int id) -> int", &ipc_status);
  m.def("ipc_status_word(int id) -> Tensor", &ipc_status_word);
  m.def("ipc_destroy(int id) -> ()", [](int64_t id) { (void)fr_ipc_destroy((int)id); });
  m.def("ipc_allreduce_(int id, Tensor(a!) x, int epoch, int mode, int blocks, float timeout_s=60.) -> ()", on_gpu(&ipc_allreduce_));
  m.def("ipc_allreduce_local_(int[] ids, Tensor(a!)[] xs, int epoch, int mode, int blocks, float timeout_s=60.) -> ()", on_gpu(&ipc_allreduce_local_));
  m.def("secagg_mask(Tensor x, Tensor seeds, Tensor signs, float scale, float clipv, int round) -> (Tensor)", on_gpu(&secagg_mask));
  m.def("secagg_unmask(Tensor x, float inv_scale) -> Tensor", on_gpu(&secagg_unmask));
  m.def("secagg_hist(Tensor x, Tensor seeds, Tensor signs, int round) -> Tensor", on_gpu(&secagg_hist));
  m.def("secagg_mask_exact(Tensor x, Tensor seeds, Tensor signs, Tensor hist, int W, int round) -> Tensor", on_gpu(&secagg_mask_exact));
  m.def("secagg_unmask_exact_(Tensor q, Tensor hist, int W, Tensor(a!) out) -> ()", on_gpu(&secagg_unmask_exact_));
}
