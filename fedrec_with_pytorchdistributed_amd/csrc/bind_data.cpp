// fedrec ops of the data path and of ranking: batch sampling and id dedup (batch.hip), the
// catalog top-k (topk_scores.hip).
#include "binding_util.h"

namespace {

// the dedup's one-kernel-chain path covers up to this many ids; past it the sort path queues
// work after its unique-count read (the engine then waits on an event: dedup_sync_max())
constexpr int64_t kDedupKernelMax = 8192;

Tensor4 dedup(const at::Tensor& ids, int64_t num_news) {
  check_dev(ids, "ids");
  TORCH_CHECK(ids.scalar_type() == at::kInt && ids.dim() == 1, "fedrec::dedup: int32 [R]");
  const c10::DeviceGuard g(ids.device());
  const int64_t R = ids.numel();
  auto opt = ids.options();
  if (R == 0 || R > kDedupKernelMax) {  // large batches: sort-based path (still on the device)
    auto sorted = at::sort(ids.to(at::kLong), /*stable=*/true, 0, false);
    auto sid = std::get<0>(sorted);
    auto perm = std::get<1>(sorted).to(at::kInt);
    auto uq = std::get<0>(at::_unique2(sid, true, true, true));
    (void)num_news;
    auto flags = at::ones({R}, opt);
    if (R > 1) flags.slice(0, 1).copy_(sid.slice(0, 1).ne(sid.slice(0, 0, R - 1)).to(at::kInt));
    auto rank = at::cumsum(flags, 0).to(at::kInt) - 1;
    auto inv = at::empty({R}, opt);
    inv.index_put_({perm.to(at::kLong)}, rank);
    const int64_t U = uq.numel();
    auto counts = at::bincount(rank.to(at::kLong), {}, U);
    auto seg = at::zeros({U + 1}, opt);
    seg.slice(0, 1).copy_(at::cumsum(counts, 0).to(at::kInt));
    return {uq.to(at::kInt), inv, perm, seg};
  }
  auto uniq = at::empty({R}, opt);
  auto inv = at::empty({R}, opt);
  auto perm = at::empty({R}, opt);
  auto seg = at::empty({R + 1}, opt);
  auto ucount = at::empty({1}, opt);
  // num_news bounds the ids (the engine passes its table size): <= 2^19 selects 32-bit sort keys
  check_rc(fr_dedup(ids.data_ptr<int>(), (int)R, (int)std::min<int64_t>(num_news, 1 << 30), uniq.data_ptr<int>(),
                    inv.data_ptr<int>(), perm.data_ptr<int>(), seg.data_ptr<int>(), ucount.data_ptr<int>(),
                    cur_stream()),
           "dedup");
  const int64_t U = ucount.item<int>();  // the backbone grid depends on U: one small D2H per step
  return {uniq.slice(0, 0, U), inv, perm, seg.slice(0, 0, U + 1)};
}

Tensor2 sample_batch(const at::Tensor& rows, const at::Tensor& pos, const at::Tensor& neg_ptr, const at::Tensor& negs,
                     const at::Tensor& his_ptr, const at::Tensor& his, int64_t npratio, int64_t H, bool truncate,
                     int64_t seed, int64_t offset, bool valid) {
  for (auto* t : {&rows, &pos, &negs, &his}) {
    check_dev(*t, "sample_batch input");
    TORCH_CHECK(t->scalar_type() == at::kInt, "fedrec::sample_batch: int32 ids");
  }
  check_dev(neg_ptr, "neg_ptr");
  check_dev(his_ptr, "his_ptr");
  TORCH_CHECK(neg_ptr.scalar_type() == at::kLong && his_ptr.scalar_type() == at::kLong, "fedrec::sample_batch: int64 ptr");
  TORCH_CHECK(neg_ptr.numel() == pos.numel() + 1 && his_ptr.numel() == pos.numel() + 1, "fedrec::sample_batch: CSR");
  const c10::DeviceGuard g(rows.device());
  const int64_t B = rows.numel();
  // cand and his side by side in one buffer: the dedup reads [cand | his] as one id list without
  // a concatenating copy (LocalEngine.prepare)
  auto both = at::empty({B * (npratio + 1) + B * H}, rows.options());
  auto cand = both.narrow(0, 0, B * (npratio + 1)).view({B, npratio + 1});
  auto hout = both.narrow(0, B * (npratio + 1), B * H).view({B, H});
  check_rc(fr_sample_batch(rows.data_ptr<int>(), pos.data_ptr<int>(), (const long long*)neg_ptr.data_ptr<int64_t>(),
                           negs.data_ptr<int>(), (const long long*)his_ptr.data_ptr<int64_t>(), his.data_ptr<int>(),
                           cand.data_ptr<int>(), hout.data_ptr<int>(), (int)B, (int)npratio, (int)H, truncate ? 1 : 0,
                           (unsigned long long)seed, (unsigned long long)offset, valid ? 1 : 0, cur_stream()),
           "sample_batch");
  return {cand, hout};
}

// ---- catalog top-k (topk_scores.hip): scores = user table^T fused with an ordered top-k select ----
// -> (scores [B, k] fp32, ids [B, k] int32): the k best rows n >= min_id, n not in exclude[b, :],
// score not NaN, by (score descending, id ascending); short lists end in (-inf, -1)
Tensor2 topk_scores(const at::Tensor& user, const at::Tensor& table, int64_t k, const OptTensor& exclude,
                    int64_t min_id) {
  check_dev(user, "user");
  check_dev(table, "table");
  TORCH_CHECK(user.scalar_type() == at::kFloat && table.scalar_type() == at::kFloat,
              "fedrec::topk_scores: user / table must be fp32 (got ", user.scalar_type(), " / ", table.scalar_type(), ")");
  TORCH_CHECK(user.dim() == 2 && table.dim() == 2 && user.size(1) == table.size(1),
              "fedrec::topk_scores: user [B, D], table [N, D]");
  TORCH_CHECK(user.device() == table.device(), "fedrec::topk_scores: user and table on one device");
  const int64_t B = user.size(0), N = table.size(0), D = user.size(1);
  TORCH_CHECK(k >= 1 && k <= 128, "fedrec::topk_scores: 1 <= k <= 128 (got ", k, ")");
  TORCH_CHECK(D % 4 == 0 && D >= 4 && D <= 512, "fedrec::topk_scores: D % 4 == 0, 4 <= D <= 512 (got ", D, ")");
  TORCH_CHECK(B >= 1 && N >= 1 && N < 2147483648LL, "fedrec::topk_scores: B >= 1, 1 <= N < 2^31");
  int64_t E = 0;
  const int* ep = nullptr;
  if (defined(exclude)) {
    check_dev(*exclude, "exclude");
    TORCH_CHECK(exclude->scalar_type() == at::kInt && exclude->dim() == 2 && exclude->size(0) == B &&
                    exclude->device() == user.device(),
                "fedrec::topk_scores: exclude int32 [B, E] on the user's device");
    E = exclude->size(1);
    if (E > 0) ep = exclude->data_ptr<int>();
  }
  const int mid = (int)std::min<int64_t>(std::max<int64_t>(min_id, 0), 2147483647LL);
  const c10::DeviceGuard g(user.device());
  auto scores = at::empty({B, k}, user.options());
  auto ids = at::empty({B, k}, user.options().dtype(at::kInt));
  auto ws = at::empty({B, (int64_t)fr_topk_splits((long)B, (long)N), k}, user.options().dtype(at::kLong));
  const int rc = fr_topk_scores(user.data_ptr<float>(), table.data_ptr<float>(), ep, ws.data_ptr(),
                                scores.data_ptr<float>(), ids.data_ptr<int>(), (long)B, (long)N, (int)D, (long)E, (int)k,
                                mid, cur_stream());
  TORCH_CHECK(rc != 2, "fedrec::topk_scores: user / table must be 16-byte aligned");
  check_rc(rc, "topk_scores");
  return {scores, ids};
}

}  // namespace

TORCH_LIBRARY_FRAGMENT(fedrec, m) {
  m.def("topk_set_splits(int s) -> ()", [](int64_t s) { fr_topk_set_splits((int)s); });
  m.def("dedup_sync_max() -> int", []() -> int64_t { return kDedupKernelMax; });
  m.def("dedup(Tensor ids, int num_news) -> (Tensor, Tensor, Tensor, Tensor)", on_gpu(&dedup));
  m.def("sample_batch(Tensor rows, Tensor pos, Tensor neg_ptr, Tensor negs, Tensor his_ptr, Tensor his, int npratio, int H, bool truncate, int seed, int offset, bool valid=False) -> (Tensor, Tensor)", on_gpu(&sample_batch));
  m.def("topk_scores(Tensor user, Tensor table, int k, Tensor? exclude=None, int min_id=0) -> (Tensor, Tensor)", on_gpu(&topk_scores));
}
