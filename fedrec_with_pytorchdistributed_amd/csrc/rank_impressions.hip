// Full-impression ranking: every negative an impression showed is scored against the user and
// compared with the positive's score -- only four integers per impression are written, no score
// and no gathered row.
//
//   s(b, n) = sum_d user[b, d] * table[n, d]      fp32 operands, fp32 accumulate (ranking is the
//                                                 output, so no bf16 rounding: as topk_scores.hip)
//   user b is impression i = row0 + b of the corpus CSR (pos [I], neg_ptr [I + 1], negs [M])
//   counts[b] = (n_gt, n_eq, n_neg, n_nan): the negatives whose score is greater than / equal to
//   s(b, pos[i]), the length of the list, and the candidates (positive included) whose score is
//   NaN (NaN compares false: such a candidate is in neither n_gt nor n_eq)
//
// One reduction order.  16 lanes share a row: lane l of the group owns columns 64 t + 4 l + (0..3),
// t ascending, each product added by one explicit fmaf (x, y, z, w in turn) -- no contraction left
// to the compiler -- and the 16 partial sums meet in an xor butterfly (8, 4, 2, 1; a + b = b + a
// bitwise, so every lane of the group ends with the same value).  ri_dot is the only place a score
// is formed: the positive and every negative go through it, whichever wave or lane group holds
// them, so a negative with the positive's id ties bitwise and counts[b] does not depend on B, row0,
// the grid or the split of a long list.
//
// Shape.  A wave owns one work item: a chunk of up to RI_CH consecutive negatives of one
// impression.  It holds u in registers (NT float4 per lane), reads the chunk's ids with two
// coalesced loads, and gathers rows straight into registers, 4 rows per wave-instruction (one per
// 16-lane group: 256-B contiguous segments) and two such quads in flight.  The positive's score is
// recomputed by every wave that needs it (one more row) rather than passed between waves.
//
// Ragged lists.  Chunk 0 of impression b is wave b of rank_first_kernel.  Chunks 1.. of a list
// longer than RI_CH are separate work items, so that a 5,000-negative list costs 40 waves a chunk
// each and not one wave 5,000 rows (the ragged-list split rule: lists longer than a quarter of a
// wave's share of the rows).  Their slots need no queue and no atomics: with o(b) the offset of
// impression b's list inside the batch's span of negs, impression b owns slots
// [o(b) / RI_CH, o(b + 1) / RI_CH) -- disjoint by construction and never fewer than its extra
// chunks (floor(o / C) + ceil(len / C) - 1 <= floor((o + len) / C)).  rank_first_kernel writes
// b + 1 into the slots it uses and 0 into the rest of its range; rank_extra_kernel gives every
// slot a wave, which stores its integer partial at the slot; rank_fold_kernel adds impression b's
// partials to counts[b] in slot order, in registers.  Integer adds only: nothing depends on
// arrival order.
//
// Ids are trusted to lie in [0, N) (the engine checks its arrays once); they are clamped all the
// same, so a bad id reads a wrong row and no foreign memory.  A neg_ptr that is not monotone within
// [0, M] gives its impression an empty list.
#include "common.h"
#include "launchers.h"

namespace {

constexpr int RI_CH = 128;  // negatives per work item: 2 ids per lane, 32 quads of 4 rows

struct RiCounts {
  int gt, eq, nan;
};

// lane l16 of a 16-lane group: its NT float4 of one row (columns past D: zero).  No branch around
// a load -- a column past D re-reads the row's last float4 and is zeroed by a select -- so all NT
// loads of a row, and those of the next row, are in flight together
template <int NT>
__device__ __forceinline__ void ri_load(float4 (&v)[NT], const float* __restrict__ row, int D, int l16) {
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int c = 64 * t + 4 * l16;
    const float4 x = *(const float4*)(row + min(c, D - 4));
    const bool z = c >= D;
    v[t] = make_float4(z ? 0.f : x.x, z ? 0.f : x.y, z ? 0.f : x.z, z ? 0.f : x.w);
  }
}

// THE score: u . v of one row, the same value in all 16 lanes of the group
template <int NT>
__device__ __forceinline__ float ri_dot(const float4 (&u)[NT], const float4 (&v)[NT]) {
  float acc = 0.f;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    acc = __builtin_fmaf(u[t].x, v[t].x, acc);
    acc = __builtin_fmaf(u[t].y, v[t].y, acc);
    acc = __builtin_fmaf(u[t].z, v[t].z, acc);
    acc = __builtin_fmaf(u[t].w, v[t].w, acc);
  }
  acc += __shfl_xor(acc, 8, 64);
  acc += __shfl_xor(acc, 4, 64);
  acc += __shfl_xor(acc, 2, 64);
  acc += __shfl_xor(acc, 1, 64);
  return acc;
}

__device__ __forceinline__ int ri_group4_sum(int v) {
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}

// impression i's list [s, e) inside negs [0, M) and its offset o in the batch's span (P0 =
// neg_ptr[row0]); a pointer pair that is not monotone within [0, M] -> the empty list at o = 0
__device__ __forceinline__ void ri_span(const long long* __restrict__ neg_ptr, long i, long long P0, long M,
                                        long long& s, long long& e, long long& o) {
  s = neg_ptr[i];
  e = neg_ptr[i + 1];
  const bool ok = P0 >= 0 && P0 <= s && s <= e && e <= (long long)M;
  o = ok ? s - P0 : 0;
  s = ok ? s : 0;
  e = ok ? e : 0;
}

// one wave: u of user b and the positive's score
template <int NT>
__device__ __forceinline__ float ri_user_pos(float4 (&u)[NT], const float* __restrict__ user,
                                             const float* __restrict__ table, const int* __restrict__ pos, long b,
                                             long i, int N, int D, int l16) {
  ri_load<NT>(u, user + (size_t)b * D, D, l16);
  const int p = min(max(pos[i], 0), N - 1);
  float4 v[NT];
  ri_load<NT>(v, table + (size_t)p * D, D, l16);
  return ri_dot<NT>(u, v);
}

// one wave: negatives negs[j0 .. j0 + n), n <= RI_CH, against sp -> the wave's counts (every lane)
template <int NT>
__device__ __forceinline__ RiCounts ri_chunk(const float4 (&u)[NT], float sp, const float* __restrict__ table,
                                             const int* __restrict__ negs, long long j0, int n, int N, int D,
                                             int lane) {
  const int g = lane >> 4, l16 = lane & 15;
  const int ids0 = lane < n ? negs[j0 + lane] : 0;
  const int ids1 = lane + 64 < n ? negs[j0 + 64 + lane] : 0;
  int gt = 0, eq = 0, nan = 0;
  const int nq = (n + 3) >> 2;
  for (int q = 0; q < nq; q += 2) {  // wave-uniform
    const int r0 = 4 * q + g, r1 = r0 + 4;
    // (a quad's four rows lie in one half of the chunk: which id register holds them is wave-uniform)
    const int id0 = __shfl(q < 16 ? ids0 : ids1, r0 & 63, 64);
    const int id1 = __shfl(q + 1 < 16 ? ids0 : ids1, r1 & 63, 64);
    const bool on0 = r0 < n, on1 = r1 < n;
    float4 v0[NT], v1[NT];
    // (a group past the end of the list reads row 0 and its score is not counted)
    ri_load<NT>(v0, table + (size_t)min(max(id0, 0), N - 1) * D, D, l16);
    ri_load<NT>(v1, table + (size_t)min(max(id1, 0), N - 1) * D, D, l16);
    const float s0 = ri_dot<NT>(u, v0);
    const float s1 = ri_dot<NT>(u, v1);
    gt += (on0 && s0 > sp) + (on1 && s1 > sp);
    eq += (on0 && s0 == sp) + (on1 && s1 == sp);
    nan += (on0 && s0 != s0) + (on1 && s1 != s1);
  }
  RiCounts c;
  c.gt = ri_group4_sum(gt);
  c.eq = ri_group4_sum(eq);
  c.nan = ri_group4_sum(nan);
  return c;
}

// wave b: chunk 0 of impression row0 + b -> counts[b]; the slots of its further chunks -> item
template <int NT>
__global__ __launch_bounds__(256) void rank_first_kernel(const float* __restrict__ user,
                                                         const float* __restrict__ table,
                                                         const int* __restrict__ pos,
                                                         const long long* __restrict__ neg_ptr,
                                                         const int* __restrict__ negs, int4* __restrict__ counts,
                                                         int* __restrict__ item, long B, int N, int D, long M,
                                                         long row0, long Q) {
  const int lane = threadIdx.x & 63;
  const long b = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;  // wave-uniform; the kernel has no barrier
  const long i = row0 + b;
  long long s, e, o;
  ri_span(neg_ptr, i, neg_ptr[row0], M, s, e, o);
  const long long len = e - s;
  float4 u[NT];
  const float sp = ri_user_pos<NT>(u, user, table, pos, b, i, N, D, lane & 15);
  const RiCounts c = ri_chunk<NT>(u, sp, table, negs, s, (int)min(len, (long long)RI_CH), N, D, lane);
  if (lane == 0) counts[b] = make_int4(c.gt, c.eq, (int)len, c.nan + (sp != sp ? 1 : 0));
  // slots [o / CH, (o + len) / CH): the first `extra` of them are chunks 1.. of this impression
  const long long w0 = o / RI_CH, w1 = (o + len) / RI_CH, extra = (len + RI_CH - 1) / RI_CH - 1;
  for (long long w = w0 + lane; w < w1 && w < Q; w += 64) item[w] = w - w0 < extra ? (int)(b + 1) : 0;
}

// wave w: slot w of the batch, if an impression uses it -> part[w]
template <int NT>
__global__ __launch_bounds__(256) void rank_extra_kernel(const float* __restrict__ user,
                                                         const float* __restrict__ table,
                                                         const int* __restrict__ pos,
                                                         const long long* __restrict__ neg_ptr,
                                                         const int* __restrict__ negs, const int* __restrict__ item,
                                                         int4* __restrict__ part, long B, int N, int D, long M,
                                                         long row0, long Q) {
  const int lane = threadIdx.x & 63;
  const long long P0 = neg_ptr[row0], P1 = neg_ptr[row0 + B];
  long long W = P0 >= 0 && P0 <= P1 && P1 <= (long long)M ? (P1 - P0) / RI_CH : 0;  // slots in use: [0, W)
  W = min(W, (long long)Q);
  for (long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); w < W; w += (long long)gridDim.x * 4) {
    const int it = __builtin_amdgcn_readfirstlane(item[w]);
    if (it <= 0 || it > B) continue;  // wave-uniform
    const long b = it - 1, i = row0 + b;
    long long s, e, o;
    ri_span(neg_ptr, i, P0, M, s, e, o);
    const long long ch = w - o / RI_CH + 1;  // this slot's chunk of the list
    const long long j0 = s + ch * RI_CH;
    if (ch < 1 || j0 >= e) continue;
    float4 u[NT];
    const float sp = ri_user_pos<NT>(u, user, table, pos, b, i, N, D, lane & 15);
    const RiCounts c = ri_chunk<NT>(u, sp, table, negs, j0, (int)min(e - j0, (long long)RI_CH), N, D, lane);
    if (lane == 0) part[w] = make_int4(c.gt, c.eq, 0, c.nan);
  }
}

// thread b: counts[b] += the partials of impression b's further chunks, in slot order
__global__ __launch_bounds__(256) void rank_fold_kernel(const long long* __restrict__ neg_ptr,
                                                        const int4* __restrict__ part, int4* __restrict__ counts,
                                                        long B, long M, long row0, long Q) {
  const long b = (long)blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  long long s, e, o;
  ri_span(neg_ptr, row0 + b, neg_ptr[row0], M, s, e, o);
  const long long len = e - s, w0 = o / RI_CH, extra = (len + RI_CH - 1) / RI_CH - 1;
  if (extra <= 0) return;
  int4 c = counts[b];
  for (long long w = w0; w < w0 + extra && w < Q; ++w) {
    const int4 p = part[w];
    c.x += p.x;
    c.y += p.y;
    c.w += p.w;
  }
  counts[b] = c;
}

template <int NT>
void ri_launch(const float* user, const float* table, const int* pos, const long long* neg_ptr, const int* negs,
               int4* counts, int* item, int4* part, long B, int N, int D, long M, long row0, long Q, hipStream_t s) {
  hipLaunchKernelGGL(rank_first_kernel<NT>, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, s, user, table, pos, neg_ptr,
                     negs, counts, item, B, N, D, M, row0, Q);
  // a wave per slot; past 16,384 workgroups (4 resident rounds of the chip) the waves stride
  const long gx = min((Q + 3) / 4, 16384L);
  hipLaunchKernelGGL(rank_extra_kernel<NT>, dim3((unsigned)gx), dim3(256), 0, s, user, table, pos, neg_ptr, negs,
                     (const int*)item, part, B, N, D, M, row0, Q);
  hipLaunchKernelGGL(rank_fold_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, neg_ptr,
                     (const int4*)part, counts, B, M, row0, Q);
}

}  // namespace

// int32 words of workspace a launch over a corpus of M negatives needs: per slot one item word and
// one int4 partial (the partials first: 16-byte aligned)
extern "C" long fr_rank_impressions_ws(long M) { return (M / RI_CH + 1) * 5; }

// 0 ok; 1 unsupported shape; 2 misaligned pointer.  ws: int32 [fr_rank_impressions_ws(M)], 16-byte aligned
extern "C" int fr_rank_impressions(const float* user, const float* table, const int* pos, const long long* neg_ptr,
                                   const int* negs, void* ws, int* counts, long B, long N, int D, long I, long M,
                                   long row0, hipStream_t s) {
  if (B < 1 || N < 1 || N >= 2147483648L || I < 1 || M < 0 || M >= 2147483648L || row0 < 0 || row0 + B > I ||
      (B + 3) / 4 > 2147483647L || D < 4 || D > 512 || D % 4 != 0)
    return 1;
  if ((((uintptr_t)user) & 15) || (((uintptr_t)table) & 15) || (((uintptr_t)ws) & 15) || (((uintptr_t)counts) & 15))
    return 2;
  const long Q = M / RI_CH + 1;
  int4* part = (int4*)ws;
  int* item = (int*)ws + 4 * Q;
  const int NT = (D + 63) / 64;
#define RI_CASE(n)                                                                                             \
  case n:                                                                                                      \
    ri_launch<n>(user, table, pos, neg_ptr, negs, (int4*)counts, item, part, B, (int)N, D, M, row0, Q, s);     \
    break;
  switch (NT) {
    RI_CASE(1) RI_CASE(2) RI_CASE(3) RI_CASE(4) RI_CASE(5) RI_CASE(6) RI_CASE(7) RI_CASE(8)
    default:
      return 1;
  }
#undef RI_CASE
  return 0;
}
