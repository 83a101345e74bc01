// fedrec ops of the optimizer step (adam.hip): Adam over the flat buffers, the weight casts and
// the small batched copies (batch.hip fr_multi_copy) that share their launches.
#include "binding_util.h"

namespace {

// Adam with the step count (and the per-step loss ring) on the device: capturable in a graph.
// step: int64 [1], already advanced for this step (the step's cast launch, multi_cast bump2)
// gsrc / goff (optional): the step's per-parameter gradient tensors and their flat offsets --
// Adam gathers the gradient from them and writes it into g (no separate copy launch)
void adam_dev(at::Tensor p, at::Tensor g, at::Tensor m, at::Tensor v, const at::Tensor& step,
              const at::Tensor& loss, at::Tensor ring, double lr, double b1, double b2, double eps, double grad_scale,
              const c10::optional<std::vector<OptTensor>>& gsrc, const c10::optional<std::vector<int64_t>>& goff,
              const OptTensor& skip) {
  for (auto* t : {&p, &m, &v}) check_dev(*t, "adam_dev buffer");
  const int* skp = nullptr;
  if (defined(skip)) {  // the gradient all-reduce's status word (int32 [1])
    check_dev(*skip, "skip");
    TORCH_CHECK(skip->scalar_type() == at::kInt && skip->numel() == 1 && skip->device() == p.device(),
                "fedrec::adam_dev: skip int32 [1] on p's device");
    skp = skip->data_ptr<int>();
  }
  check_dev(g, "g");
  check_dev(step, "step");
  TORCH_CHECK(p.scalar_type() == at::kFloat && g.scalar_type() == at::kFloat && m.scalar_type() == at::kFloat &&
                  v.scalar_type() == at::kFloat && p.numel() == g.numel() && p.numel() == m.numel() &&
                  p.numel() == v.numel() && p.is_contiguous() && g.is_contiguous() && m.is_contiguous() &&
                  v.is_contiguous(),
              "fedrec::adam_dev: fp32 flat buffers of one size");
  TORCH_CHECK(step.scalar_type() == at::kLong && step.numel() == 1, "fedrec::adam_dev: int64 step [1]");
  const bool has_ring = ring.numel() > 0;
  if (has_ring) {
    check_dev(loss, "loss");
    check_dev(ring, "ring");
    TORCH_CHECK(loss.scalar_type() == at::kFloat && loss.numel() == 1 && ring.scalar_type() == at::kFloat &&
                    ring.is_contiguous(),
                "fedrec::adam_dev: fp32 loss [1] and ring");
  }
  const c10::DeviceGuard dg(p.device());
  std::vector<const float*> sp;
  std::vector<long> so, sn;
  if (gsrc.has_value()) {
    TORCH_CHECK(goff.has_value() && goff->size() == gsrc->size(), "fedrec::adam_dev: gsrc / goff sizes");
    for (size_t j = 0; j < gsrc->size(); ++j) {
      const auto& t = (*gsrc)[j];
      if (t.has_value()) {
        check_dev(*t, "adam_dev gradient segment");
        TORCH_CHECK(t->scalar_type() == at::kFloat && t->is_contiguous(), "fedrec::adam_dev: fp32 contiguous grads");
      }
      sp.push_back(t.has_value() ? t->data_ptr<float>() : nullptr);
      so.push_back((long)(*goff)[j]);
      sn.push_back(t.has_value() ? (long)t->numel() : 0L);
    }
  }
  check_rc(fr_adam_dev(p.data_ptr<float>(), g.data_ptr<float>(), m.data_ptr<float>(), v.data_ptr<float>(), nullptr,
                       (long)p.numel(), (float)lr, b1, b2, (float)(1.0 - b1), (float)(1.0 - b2), (float)eps,
                       (float)grad_scale, (const long long*)step.data_ptr<int64_t>(),
                       has_ring ? loss.data_ptr<float>() : nullptr, has_ring ? ring.data_ptr<float>() : nullptr,
                       (int)ring.numel(), cur_stream(), (int)sp.size(), sp.data(), so.data(), sn.data(), skp),
           "adam_dev");
}

void adam_flat(at::Tensor p, const at::Tensor& g, at::Tensor m, at::Tensor v, const OptTensor& plow, double lr,
               double b1, double b2, double eps, double bc1, double bc2, double grad_scale) {
  check_dev(p, "p");
  check_dev(g, "g");
  check_dev(m, "m");
  check_dev(v, "v");
  TORCH_CHECK(p.scalar_type() == at::kFloat && p.numel() == g.numel() && p.numel() == m.numel() && p.numel() == v.numel(),
              "fedrec::adam_flat: fp32 flat buffers of one size");
  void* lp = nullptr;
  if (defined(plow)) {
    check_dev(*plow, "p_lowp");
    TORCH_CHECK(plow->scalar_type() == at::kBFloat16 && plow->numel() == p.numel(), "fedrec::adam_flat: p_lowp");
    lp = plow->data_ptr();
  }
  const c10::DeviceGuard dg(p.device());
  check_rc(fr_adam_flat(p.data_ptr<float>(), g.data_ptr<float>(), m.data_ptr<float>(), v.data_ptr<float>(), lp,
                        (long)p.numel(), (float)lr, (float)b1, (float)b2, (float)(1.0 - b1), (float)(1.0 - b2),
                        (float)eps, (float)bc1, (float)bc2, (float)grad_scale, cur_stream()),
           "adam_flat");
}

// A cast destination given as a transposed view of a bf16 matrix (dst = T[:, a:b].t(): sizes
// [R, C], strides (1, ld >= R)) of a contiguous fp32 [R, C] source: the cast writes the
// transposed copy (multi_cast's T segments; the register-direct GEMMs' k-contiguous weights)
struct TSegs {
  std::vector<const float*> src;
  std::vector<void*> dst;
  std::vector<int> R, C, ld;
};
bool is_tdst(const at::Tensor& src, const at::Tensor& dst) {
  return dst.dim() == 2 && src.dim() == 2 && dst.scalar_type() == at::kBFloat16 && src.scalar_type() == at::kFloat &&
         src.is_contiguous() && src.sizes() == dst.sizes() && dst.stride(0) == 1 && dst.size(0) > 1 &&
         dst.stride(1) >= dst.size(0) && src.is_cuda() && dst.is_cuda();
}
void add_tseg(TSegs& t, const at::Tensor& src, const at::Tensor& dst) {
  TORCH_CHECK(t.src.size() < 8, "fedrec: at most 8 transposed cast segments per launch");
  t.src.push_back(src.data_ptr<float>());
  t.dst.push_back(dst.data_ptr());
  t.R.push_back((int)src.size(0));
  t.C.push_back((int)src.size(1));
  t.ld.push_back((int)dst.stride(1));
}

// fp32 tensors -> bf16 / fp32 destinations (contiguous slices allowed) in one launch per 96
// (adam.hip), any size / alignment; false = not launched (an empty segment).  bump (optional
// int64 [1] on the same device): advanced by one by the first launch
bool multi_cast(const std::vector<at::Tensor>& src, const std::vector<at::Tensor>& dst, const OptTensor& bump,
                const OptTensor& bump2) {
  const size_t n = src.size();
  TORCH_CHECK(n >= 1 && dst.size() == n, "fedrec::multi_cast: sizes");
  const c10::DeviceGuard g(dst[0].device());
  auto bptr = [&](const OptTensor& b, const char* name) -> long long* {
    if (!defined(b)) return nullptr;
    TORCH_CHECK(b->device() == dst[0].device() && b->scalar_type() == at::kLong && b->numel() == 1 && b->is_contiguous(),
                "fedrec::multi_cast: ", name, " must be an int64 [1] tensor on the destinations' device");
    return (long long*)b->data_ptr<int64_t>();
  };
  long long* bp = bptr(bump, "bump");
  long long* bp2 = bptr(bump2, "bump2");
  std::vector<const float*> sp;
  std::vector<void*> dp;
  std::vector<long> ne;
  std::vector<int> bf;
  TSegs ts;
  for (size_t i = 0; i < n; ++i) {
    if (is_tdst(src[i], dst[i])) {
      add_tseg(ts, src[i], dst[i]);
      continue;
    }
    TORCH_CHECK(src[i].is_cuda() && dst[i].is_cuda() && src[i].is_contiguous() && dst[i].is_contiguous() &&
                    src[i].scalar_type() == at::kFloat &&
                    (dst[i].scalar_type() == at::kBFloat16 || dst[i].scalar_type() == at::kFloat) &&
                    src[i].numel() == dst[i].numel(),
                "fedrec::multi_cast: contiguous fp32 sources, bf16/fp32 destinations of the same size "
                "(or transposed bf16 views)");
    sp.push_back(src[i].data_ptr<float>());
    dp.push_back(dst[i].data_ptr());
    ne.push_back((long)src[i].numel());
    bf.push_back(dst[i].scalar_type() == at::kBFloat16 ? 1 : 0);
  }
  const size_t nn = sp.size();
  for (size_t i = 0; i < nn; ++i)
    if (ne[i] <= 0) return false;
  TORCH_CHECK(nn >= 1, "fedrec::multi_cast: at least one plain segment");
  for (size_t i0 = 0; i0 < nn; i0 += 96) {  // 96 segments per launch (kernel-argument size)
    const int k = (int)std::min<size_t>(96, nn - i0);
    const bool first = i0 == 0;
    TORCH_CHECK(fr_multi_cast(sp.data() + i0, dp.data() + i0, ne.data() + i0, bf.data() + i0, k, first ? bp : nullptr,
                              cur_stream(), first ? bp2 : nullptr, nullptr, nullptr, first ? (int)ts.src.size() : 0,
                              ts.src.data(), ts.dst.data(), ts.R.data(), ts.C.data(), ts.ld.data()) == 0,
                "fedrec::multi_cast: launch rejected");
  }
  return true;
}

// A step graph's per-replay launch: the batch into the graph's static inputs (copies of 4-byte
// words; a destination longer than its source gets the fill word past it) and the step's weight
// casts + counter bumps (multi_cast), ONE launch instead of a copy launch and an in-graph cast
// launch.  false = nothing launched (an empty cast segment).
bool copy_cast(const std::vector<at::Tensor>& csrc, const std::vector<at::Tensor>& cdst, at::IntArrayRef fill,
               const std::vector<at::Tensor>& src, const std::vector<at::Tensor>& dst, const OptTensor& bump,
               const OptTensor& bump2) {
  const size_t nc = csrc.size(), n = src.size();
  TORCH_CHECK(cdst.size() == nc && fill.size() == nc && dst.size() == n && nc + n >= 1 && nc + n <= 96,
              "fedrec::copy_cast: sizes");
  const at::Tensor& ref = nc ? cdst[0] : dst[0];
  const c10::DeviceGuard g(ref.device());
  auto bptr = [&](const OptTensor& b) -> long long* {
    if (!defined(b)) return nullptr;
    TORCH_CHECK(b->device() == ref.device() && b->scalar_type() == at::kLong && b->numel() == 1 && b->is_contiguous(),
                "fedrec::copy_cast: bumps must be int64 [1] tensors on the destinations' device");
    return (long long*)b->data_ptr<int64_t>();
  };
  long long* bp = bptr(bump);
  long long* bp2 = bptr(bump2);
  std::vector<const float*> sp;
  std::vector<void*> dp;
  std::vector<long> ne, ns;
  std::vector<int> bf, fv;
  for (size_t i = 0; i < nc; ++i) {
    TORCH_CHECK(csrc[i].is_cuda() && cdst[i].is_cuda() && csrc[i].is_contiguous() && cdst[i].is_contiguous() &&
                    csrc[i].element_size() == 4 && cdst[i].scalar_type() == csrc[i].scalar_type() &&
                    csrc[i].numel() <= cdst[i].numel(),
                "fedrec::copy_cast: copies are contiguous device tensors of one 4-byte dtype, source <= destination");
    if (cdst[i].numel() == 0) continue;
    sp.push_back((const float*)csrc[i].data_ptr());
    dp.push_back(cdst[i].data_ptr());
    ne.push_back((long)cdst[i].numel());
    ns.push_back((long)csrc[i].numel());
    bf.push_back(0);
    fv.push_back((int)fill[i]);
  }
  TSegs ts;
  for (size_t i = 0; i < n; ++i) {
    if (is_tdst(src[i], dst[i])) {
      add_tseg(ts, src[i], dst[i]);
      continue;
    }
    TORCH_CHECK(src[i].is_cuda() && dst[i].is_cuda() && src[i].is_contiguous() && dst[i].is_contiguous() &&
                    src[i].scalar_type() == at::kFloat &&
                    (dst[i].scalar_type() == at::kBFloat16 || dst[i].scalar_type() == at::kFloat) &&
                    src[i].numel() == dst[i].numel(),
                "fedrec::copy_cast: contiguous fp32 cast sources, bf16/fp32 destinations of the same size "
                "(or transposed bf16 views)");
    if (src[i].numel() == 0) return false;
    sp.push_back(src[i].data_ptr<float>());
    dp.push_back(dst[i].data_ptr());
    ne.push_back((long)src[i].numel());
    ns.push_back((long)src[i].numel());
    bf.push_back(dst[i].scalar_type() == at::kBFloat16 ? 1 : 0);
    fv.push_back(0);
  }
  if (sp.empty()) return false;
  TORCH_CHECK(fr_multi_cast(sp.data(), dp.data(), ne.data(), bf.data(), (int)sp.size(), bp, cur_stream(), bp2,
                            ns.data(), fv.data(), (int)ts.src.size(), ts.src.data(), ts.dst.data(), ts.R.data(),
                            ts.C.data(), ts.ld.data()) == 0,
              "fedrec::copy_cast: launch rejected (more than 8 padded copies?)");
  return true;
}

// fp32 [R, C] masters -> transposed bf16 copies (dst: [C, ld] views, ld = row stride >= R) in one
// launch per 96 (adam.hip); false = not launched (shape / alignment), the caller transposes itself
bool multi_cast_t(const std::vector<at::Tensor>& src, const std::vector<at::Tensor>& dst) {
  const size_t n = src.size();
  TORCH_CHECK(n >= 1 && dst.size() == n, "fedrec::multi_cast_t: sizes");
  const c10::DeviceGuard g(dst[0].device());
  std::vector<const float*> sp(n);
  std::vector<void*> dp(n);
  std::vector<int> R(n), C(n), ld(n);
  for (size_t i = 0; i < n; ++i) {
    TORCH_CHECK(src[i].is_cuda() && dst[i].is_cuda() && src[i].is_contiguous() && src[i].dim() == 2 &&
                    dst[i].dim() == 2 && src[i].scalar_type() == at::kFloat && dst[i].scalar_type() == at::kBFloat16 &&
                    dst[i].size(0) == src[i].size(1) && dst[i].size(1) == src[i].size(0) && dst[i].stride(1) == 1,
                "fedrec::multi_cast_t: fp32 [R, C] sources, bf16 [C, R] row-major destinations");
    sp[i] = src[i].data_ptr<float>();
    dp[i] = dst[i].data_ptr();
    R[i] = (int)src[i].size(0);
    C[i] = (int)src[i].size(1);
    ld[i] = (int)dst[i].stride(0);
    if (R[i] % 64 || C[i] % 64 || ld[i] % 8 || ((uintptr_t)sp[i] & 15) || ((uintptr_t)dp[i] & 15)) return false;
  }
  for (size_t i0 = 0; i0 < n; i0 += 96) {
    const int k = (int)std::min<size_t>(96, n - i0);
    TORCH_CHECK(fr_multi_cast_t(sp.data() + i0, dp.data() + i0, R.data() + i0, C.data() + i0, ld.data() + i0, k,
                                cur_stream()) == 0,
                "fedrec::multi_cast_t: launch rejected");
  }
  return true;
}

// several small copies (+ fills of the tails) in one launch, in 4-byte words
void multi_copy(const std::vector<at::Tensor>& src, const std::vector<at::Tensor>& dst, at::IntArrayRef fill) {
  const size_t n = src.size();
  TORCH_CHECK(n >= 1 && n <= 8 && dst.size() == n && fill.size() == n, "fedrec::multi_copy: sizes");
  const c10::DeviceGuard g(dst[0].device());
  std::vector<const int*> sp(n);
  std::vector<int*> dp(n);
  std::vector<long> ns(n), nd(n);
  std::vector<int> fv(n);
  for (size_t i = 0; i < n; ++i) {
    TORCH_CHECK(src[i].is_cuda() && dst[i].is_cuda() && src[i].is_contiguous() && dst[i].is_contiguous() &&
                    src[i].element_size() % 4 == 0 && dst[i].element_size() == src[i].element_size(),
                "fedrec::multi_copy: contiguous device tensors of one 4/8-byte dtype");
    sp[i] = (const int*)src[i].data_ptr();
    dp[i] = (int*)dst[i].data_ptr();
    ns[i] = (long)(src[i].numel() * src[i].element_size() / 4);
    nd[i] = (long)(dst[i].numel() * dst[i].element_size() / 4);
    TORCH_CHECK(ns[i] <= nd[i], "fedrec::multi_copy: source larger than destination");
    fv[i] = (int)fill[i];
  }
  check_rc(fr_multi_copy(sp.data(), dp.data(), ns.data(), nd.data(), fv.data(), (int)n, cur_stream()), "multi_copy");
}

}  // namespace

TORCH_LIBRARY_FRAGMENT(fedrec, m) {
  m.def("adam_dev(Tensor(a!) p, Tensor(d!) g, Tensor(b!) m, Tensor(c!) v, Tensor step, Tensor loss, Tensor(f!) ring, float lr, float b1, float b2, float eps, float grad_scale, Tensor?[]? gsrc=None, int[]? goff=None, Tensor? skip=None) -> ()", on_gpu(&adam_dev));
  m.def("adam_flat(Tensor(a!) p, Tensor g, Tensor(b!) m, Tensor(c!) v, Tensor(d!)? p_lowp, float lr, float b1, float b2, float eps, float bc1, float bc2, float grad_scale) -> ()", on_gpu(&adam_flat));
  m.def("multi_cast(Tensor[] src, Tensor(a!)[] dst, Tensor(b!)? bump=None, Tensor(c!)? bump2=None) -> bool", on_gpu(&multi_cast));
  m.def("multi_cast_t(Tensor[] src, Tensor(a!)[] dst) -> bool", on_gpu(&multi_cast_t));
  m.def("copy_cast(Tensor[] csrc, Tensor(a!)[] cdst, int[] fill, Tensor[] src, Tensor(b!)[] dst, Tensor(c!)? bump=None, "
        "Tensor(d!)? bump2=None) -> bool", on_gpu(&copy_cast));
  m.def("multi_copy(Tensor[] src, Tensor(a!)[] dst, int[] fill) -> ()", on_gpu(&multi_copy));
}
