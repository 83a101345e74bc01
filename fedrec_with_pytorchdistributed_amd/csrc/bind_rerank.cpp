// fedrec_rerank ops: diversity re-rank of a candidate pool (mmr_rerank.hip).  A namespace of its
// own: the fedrec:: and fedrec_eval:: op sets are pinned as they stand (tests/golden/op_schemas*.txt).
#include "binding_util.h"

namespace {

// ---- Maximal Marginal Relevance (mmr_rerank.hip): table [N, D] fp32, pool ids [B, P] int32 (< 0 =
// empty slot), rel [B, P] fp32 -> (ids_out [B, k] int32, rel_out [B, k] fp32, ild [B] fp32).  Shapes,
// dtypes and bounds are checked first (they do not depend on where the tensors live), then devices
// and alignment; the contents of ids are trusted
Tensor3 mmr_rerank(const at::Tensor& table, const at::Tensor& ids, const at::Tensor& rel, int64_t k, double lam) {
  TORCH_CHECK(table.scalar_type() == at::kFloat && rel.scalar_type() == at::kFloat,
              "fedrec_rerank::mmr_rerank: table / rel must be fp32 (got ", table.scalar_type(), " / ",
              rel.scalar_type(), ")");
  TORCH_CHECK(ids.scalar_type() == at::kInt, "fedrec_rerank::mmr_rerank: ids must be int32 (got ", ids.scalar_type(),
              ")");
  TORCH_CHECK(table.dim() == 2 && ids.dim() == 2 && rel.dim() == 2 && rel.size(0) == ids.size(0) &&
                  rel.size(1) == ids.size(1),
              "fedrec_rerank::mmr_rerank: table [N, D], ids [B, P], rel [B, P]");
  const int64_t N = table.size(0), D = table.size(1), B = ids.size(0), P = ids.size(1);
  TORCH_CHECK(D % 4 == 0 && D >= 4 && D <= 512, "fedrec_rerank::mmr_rerank: D % 4 == 0, 4 <= D <= 512 (got ", D, ")");
  TORCH_CHECK(P >= 1 && P <= 128, "fedrec_rerank::mmr_rerank: 1 <= P <= 128 (got ", P, ")");
  TORCH_CHECK(k >= 1 && k <= P, "fedrec_rerank::mmr_rerank: 1 <= k <= P (got k ", k, ", P ", P, ")");
  TORCH_CHECK(lam >= 0.0 && lam <= 1.0, "fedrec_rerank::mmr_rerank: 0 <= lam <= 1 (got ", lam, ")");
  TORCH_CHECK(B >= 1 && B < 2147483648LL && N >= 1 && N < 2147483648LL,
              "fedrec_rerank::mmr_rerank: 1 <= B < 2^31, 1 <= N < 2^31");
  check_dev(table, "table");
  check_dev(ids, "ids");
  check_dev(rel, "rel");
  TORCH_CHECK(ids.device() == table.device() && rel.device() == table.device(),
              "fedrec_rerank::mmr_rerank: every tensor on the table's device");
  const c10::DeviceGuard g(table.device());
  auto ids_out = at::empty({B, k}, ids.options());
  auto rel_out = at::empty({B, k}, rel.options());
  auto ild = at::empty({B}, rel.options());
  const int rc = fr_mmr_rerank(table.data_ptr<float>(), ids.data_ptr<int>(), rel.data_ptr<float>(),
                               ids_out.data_ptr<int>(), rel_out.data_ptr<float>(), ild.data_ptr<float>(), (long)B,
                               (long)N, (int)P, (int)D, (int)k, (float)lam, cur_stream());
  TORCH_CHECK(rc != 2, "fedrec_rerank::mmr_rerank: table must be 16-byte aligned");
  TORCH_CHECK(rc == 0, "fedrec_rerank::mmr_rerank: unsupported shape (code ", rc, ")");
  return {ids_out, rel_out, ild};
}

}  // namespace

// registered for every backend: a host tensor reaches the checks above and fails the device check
// (ops.mmr_rerank sends host tensors to the torch oracle before it gets here)
TORCH_LIBRARY_FRAGMENT(fedrec_rerank, m) {
  m.def("mmr_rerank(Tensor table, Tensor ids, Tensor rel, int k, float lam) -> (Tensor, Tensor, Tensor)", &mmr_rerank);
}
