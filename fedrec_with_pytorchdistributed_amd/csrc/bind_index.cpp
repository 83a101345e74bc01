// fedrec_index ops: Elias-Fano coding of a top-k upload's index list (index_code.hip).  A namespace of its own, as
// fedrec_sparse and fedrec_sign are: the older op sets are pinned as they stand (tests/golden/op_schemas*.txt).
#include "binding_util.h"

namespace {

struct EfPlan {
  int b;
  long low_words, high_bits, high_words;
};

EfPlan plan(int64_t n, int64_t k, const char* op) {
  TORCH_CHECK(n >= 1 && n < (int64_t(1) << 31), op, ": 1 <= n < 2^31 (got n ", n, ")");
  TORCH_CHECK(k >= 1 && k <= n, op, ": 1 <= k <= n (got k ", k, ", n ", n, ")");
  EfPlan p;
  TORCH_CHECK(fr_ef_plan((long)n, (long)k, &p.b, &p.low_words, &p.high_bits, &p.high_words) == 0, op, ": no plan");
  return p;
}

// ---- idx int32 [k], strictly ascending in [0, n) (topk_delta's; the CALLER's contract: any content stays in bounds
// and gives some words) -> words int32 [low_words + high_words]
at::Tensor encode(const at::Tensor& idx, int64_t n) {
  const char* op = "fedrec_index::encode";
  TORCH_CHECK(idx.scalar_type() == at::kInt, op, ": idx must be int32");
  TORCH_CHECK(idx.dim() == 1, op, ": idx [k] (got ", idx.dim(), " dims)");
  TORCH_CHECK(idx.is_contiguous(), op, ": idx must be contiguous");
  const EfPlan p = plan(n, idx.numel(), op);
  TORCH_CHECK(idx.is_cuda(), op, ": idx must be a device tensor");
  const c10::DeviceGuard g(idx.device());
  auto words = at::empty({p.low_words + p.high_words}, idx.options());
  const int rc = fr_ef_encode(idx.data_ptr<int>(), words.data_ptr<int>(), (long)n, (long)idx.numel(), cur_stream());
  TORCH_CHECK(rc == 0, op, ": unsupported shape (code ", rc, ")");
  return words;
}

// ---- words int32 [W, low_words + high_words] -> (idx int32 [W, k], count int64 [W]): count[c] is row c's set high
// bits, idx[c, i] the value at rank i or -1 where there is none in [0, n).  Whether a row IS a code is the CALLER's
// check (ops.reference.ef_decoded_check); the kernels stay in bounds for any content
Tensor2 decode(const at::Tensor& words, int64_t n, int64_t k) {
  const char* op = "fedrec_index::decode";
  TORCH_CHECK(words.scalar_type() == at::kInt, op, ": words must be int32");
  TORCH_CHECK(words.dim() == 2, op, ": words [W, low_words + high_words] (got ", words.dim(), " dims)");
  TORCH_CHECK(words.is_contiguous(), op, ": words must be contiguous");
  const EfPlan p = plan(n, k, op);
  const int64_t W = words.size(0);
  TORCH_CHECK(W >= 1 && W <= 65535, op, ": 1 <= W <= 65535 (got W ", W, ")");
  TORCH_CHECK(words.size(1) == p.low_words + p.high_words, op, ": n ", n, ", k ", k, " take words [W, ",
              p.low_words + p.high_words, "] (got ", words.size(1), ")");
  TORCH_CHECK(words.is_cuda(), op, ": words must be a device tensor");
  const c10::DeviceGuard g(words.device());
  auto idx = at::empty({W, k}, words.options());
  auto count = at::empty({W}, words.options().dtype(at::kLong));
  auto ws = at::empty({fr_ef_decode_ws((long)n, (long)k, (int)W)}, words.options());
  const int rc = fr_ef_decode(words.data_ptr<int>(), idx.data_ptr<int>(), (long*)count.data_ptr<int64_t>(),
                              (unsigned*)ws.data_ptr<int>(), (int)W, (long)n, (long)k, cur_stream());
  TORCH_CHECK(rc == 0, op, ": unsupported shape (code ", rc, ")");
  return {idx, count};
}

}  // namespace

// registered for every backend, as fedrec_sparse is: a host tensor reaches the checks above and fails the device check
// last (ops.ef_encode / ops.ef_decode send host tensors to the torch oracles)
TORCH_LIBRARY_FRAGMENT(fedrec_index, m) {
  m.def("encode(Tensor idx, int n) -> Tensor", &encode);
  m.def("decode(Tensor words, int n, int k) -> (Tensor, Tensor)", &decode);
}
