// Shared by the binding sources (bind_*.cpp): the torch.ops.fedrec.* registrations for the
// gfx950 kernels (TORCH_LIBRARY_FRAGMENT per kernel family; no pybind).
//
// Each op validates shapes/dtypes on the host (a kernel never sees a shape it was not
// written for), allocates outputs with the caching allocator, and launches on the current
// HIP stream.  The kernels live in *.hip files compiled without torch headers; they export
// plain C launchers (fr_*, declared once in launchers.h) that return a non-zero code for an
// unsupported shape.  An op's wrapper sits in one file with its registration: one m.def with the
// schema and, through on_gpu(), the kernel for the CUDA dispatch key (m.def + m.impl in one
// statement).  The helpers here have internal linkage, as the wrappers do.
#pragma once
#include <ATen/ATen.h>
#include <c10/core/DeviceGuard.h>
#include <c10/hip/HIPStream.h>
#include <torch/library.h>

#include <algorithm>
#include <tuple>
#include <vector>

#include "launchers.h"

namespace fedrec {
// the partials of a deferred small-GEMM split-K reduction, held until the launch that reduces
// them: set by small_gemm, released by head_wgrad_g / small_gemm_flush_pending (bind_user.cpp)
extern at::Tensor g_sg_pending_scratch;
}  // namespace fedrec

namespace {

using OptTensor = c10::optional<at::Tensor>;
using Tensor2 = std::tuple<at::Tensor, at::Tensor>;
using Tensor3 = std::tuple<at::Tensor, at::Tensor, at::Tensor>;
using Tensor4 = std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor>;
using Tensor5 = std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor>;
using Tensor6 = std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor>;

inline hipStream_t cur_stream() { return c10::hip::getCurrentHIPStream().stream(); }

inline void check_dev(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), "fedrec: ", name, " must be a device tensor");
  TORCH_CHECK(t.is_contiguous(), "fedrec: ", name, " must be contiguous");
}

inline void check_rc(int rc, const char* op) {
  TORCH_CHECK(rc == 0, "fedrec::", op, ": unsupported shape (code ", rc, ")");
}

template <class F>
torch::CppFunction on_gpu(F* f) { return torch::dispatch(c10::kCUDA, f); }

inline bool defined(const OptTensor& t) { return t.has_value() && t->defined(); }

inline at::Tensor as_i32(const at::Tensor& t) { return t.to(at::kInt).contiguous(); }  // masks, tokens
inline at::Tensor as_f32(const at::Tensor& t) { return t.to(at::kFloat).contiguous(); }  // LayerNorm w / b, biases

// GEMM outputs: rows padded to the 256-row tile, so the epilogue stores without a row predicate;
// the flat [M * N] head of a [gemm_rows(M) * N] allocation
inline int64_t gemm_rows(int64_t M) { return (M + 255) / 256 * 256; }
inline at::Tensor gemm_out(const at::Tensor& x, int64_t M, int64_t N) {
  return at::empty({gemm_rows(M) * N}, x.options()).narrow(0, 0, M * N);
}

// optional bias as contiguous fp32 of N elements (hold keeps the converted copy alive)
inline const float* bias_ptr(const OptTensor& b, int64_t N, const char* op, at::Tensor& hold) {
  if (!defined(b)) return nullptr;
  hold = as_f32(*b);
  TORCH_CHECK(hold.numel() == N, "fedrec::", op, ": bias size");
  return hold.data_ptr<float>();
}

// optional bf16 device tensor of numel elements (a residual, a gradient to fuse in)
inline const void* opt_bf16_ptr(const OptTensor& t, int64_t numel, const char* name, const char* op, const char* what) {
  if (!defined(t)) return nullptr;
  check_dev(*t, name);
  TORCH_CHECK(t->scalar_type() == at::kBFloat16 && t->numel() == numel, "fedrec::", op, ": ", what);
  return t->data_ptr();
}

// keep: optional [B, H] int32 mask (nonzero = attend / pool), the mask_padding option
inline const int* key_mask_ptr(const OptTensor& keep, int64_t B, int64_t H, const char* what) {
  if (!defined(keep)) return nullptr;
  check_dev(*keep, "keep");
  TORCH_CHECK(keep->scalar_type() == at::kInt && keep->is_contiguous() && keep->numel() == B * H, "fedrec::", what,
              ": keep int32 [B, H]");
  return keep->data_ptr<int>();
}

inline const int* opt_int_ptr(const OptTensor& t) { return t.has_value() ? t->data_ptr<int>() : nullptr; }

// the text-head ops' optional device count of REAL titles (a padded step graph: titles past it
// are skipped, their outputs zero): int32 [1] on the table's device
inline const int* opt_nreal(const OptTensor& t, const at::Tensor& table) {
  if (!t.has_value()) return nullptr;
  TORCH_CHECK(t->scalar_type() == at::kInt && t->numel() == 1 && t->device() == table.device(),
              "fedrec::head_*: nreal int32 [1] on the table's device");
  return t->data_ptr<int>();
}

}  // namespace
