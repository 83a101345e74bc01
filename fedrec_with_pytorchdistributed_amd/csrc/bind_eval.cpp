// fedrec_eval ops: full-impression ranking (rank_impressions.hip).  A namespace of its own: the
// fedrec:: op set is pinned as it stands (tests/golden/op_schemas.txt).
#include "binding_util.h"

namespace {

// ---- full-impression ranking (rank_impressions.hip): user b is impression row0 + b of the corpus
// CSR (pos [I], neg_ptr [I + 1], negs [M], passed whole) -> counts [B, 4] int32 (n_gt, n_eq, n_neg,
// n_nan): the negatives scoring above / equal to the positive, the list length, the NaN candidates
at::Tensor rank_impressions(const at::Tensor& user, const at::Tensor& table, const at::Tensor& pos,
                            const at::Tensor& neg_ptr, const at::Tensor& negs, int64_t row0) {
  check_dev(user, "user");
  check_dev(table, "table");
  check_dev(pos, "pos");
  check_dev(neg_ptr, "neg_ptr");
  check_dev(negs, "negs");
  TORCH_CHECK(user.scalar_type() == at::kFloat && table.scalar_type() == at::kFloat,
              "fedrec_eval::rank_impressions: user / table must be fp32 (got ", user.scalar_type(), " / ",
              table.scalar_type(), ")");
  TORCH_CHECK(user.dim() == 2 && table.dim() == 2 && user.size(1) == table.size(1),
              "fedrec_eval::rank_impressions: user [B, D], table [N, D]");
  TORCH_CHECK(pos.scalar_type() == at::kInt && negs.scalar_type() == at::kInt && pos.dim() == 1 && negs.dim() == 1,
              "fedrec_eval::rank_impressions: pos [I], negs [M] int32");
  TORCH_CHECK(neg_ptr.scalar_type() == at::kLong && neg_ptr.dim() == 1,
              "fedrec_eval::rank_impressions: neg_ptr [I + 1] int64");
  TORCH_CHECK(neg_ptr.numel() == pos.numel() + 1, "fedrec_eval::rank_impressions: neg_ptr.numel() == pos.numel() + 1");
  for (auto* t : {&table, &pos, &neg_ptr, &negs})
    TORCH_CHECK(t->device() == user.device(), "fedrec_eval::rank_impressions: every tensor on the user's device");
  const int64_t B = user.size(0), N = table.size(0), D = user.size(1), I = pos.numel(), M = negs.numel();
  TORCH_CHECK(D % 4 == 0 && D >= 4 && D <= 512, "fedrec_eval::rank_impressions: D % 4 == 0, 4 <= D <= 512 (got ", D,
              ")");
  TORCH_CHECK(B >= 1 && N >= 1 && N < 2147483648LL && M < 2147483648LL,
              "fedrec_eval::rank_impressions: B >= 1, 1 <= N < 2^31, M < 2^31");
  TORCH_CHECK(row0 >= 0 && row0 + B <= I, "fedrec_eval::rank_impressions: 0 <= row0, row0 + B <= I (got row0 ", row0,
              ", B ", B, ", I ", I, ")");
  const c10::DeviceGuard g(user.device());
  auto iopt = user.options().dtype(at::kInt);
  auto counts = at::empty({B, 4}, iopt);
  auto ws = at::empty({(int64_t)fr_rank_impressions_ws((long)M)}, iopt);
  const int rc = fr_rank_impressions(user.data_ptr<float>(), table.data_ptr<float>(), pos.data_ptr<int>(),
                                     (const long long*)neg_ptr.data_ptr<int64_t>(), negs.data_ptr<int>(), ws.data_ptr(),
                                     counts.data_ptr<int>(), (long)B, (long)N, (int)D, (long)I, (long)M, (long)row0,
                                     cur_stream());
  TORCH_CHECK(rc != 2, "fedrec_eval::rank_impressions: user / table must be 16-byte aligned");
  check_rc(rc, "rank_impressions");
  return counts;
}

}  // namespace

TORCH_LIBRARY_FRAGMENT(fedrec_eval, m) {
  m.def("rank_impressions(Tensor user, Tensor table, Tensor pos, Tensor neg_ptr, Tensor negs, int row0=0) -> Tensor", on_gpu(&rank_impressions));
}
