// Catalog top-k: scores = U V^T over the whole news table fused with an ordered per-user top-k
// select -- the [B, N] score matrix is never written.
//
//   s[b, n] = sum_d user[b, d] * table[n, d]     fp32 operands, fp32 accumulate
//             (v_mfma_f32_16x16x4_f32, as user_attn.hip: ranking is the output, so no bf16 rounding)
//   row n is eligible for user b iff n >= min_id, n not in exclude[b, :], s[b, n] is not NaN
//   output: the k best eligible rows by (score descending, id ascending); short lists end in
//           (id -1, score -inf)
//
// Ordering key.  (score, id) packs into one u64: the score's bits mapped monotonically to an
// unsigned (-0 first folded into +0, so the two zeros tie and the id decides) in the high word,
// ~id in the low word.  "better" is then one unsigned compare, every key of a user is distinct,
// and 0 is below every real key (~id >= 0x80000000): 0 is the empty slot.  A total order over
// distinct keys makes the selected list independent of the order candidates arrive in, so the
// result is bitwise independent of the grid, the split count and the LDS insertion order (integer
// LDS atomics hand out buffer slots; no float atomics anywhere).  A score is the MFMA's k-ordered
// sum of one (user, row) pair and does not depend on which tile or split the row falls in.
//
// topk_partial_kernel: grid (ceil(B / 64), S splits of the table's 16-row tiles), 256 threads.
//   * wave w holds the A fragments of users [16 w, 16 w + 16) in registers for the whole launch
//     (4 floats per 16 columns of D: 100 VGPRs at D = 400);
//   * the block streams its split's 16-row table tiles through a two-stage LDS ring (global loads
//     of tile t + 1 in flight while tile t is multiplied; one barrier per tile).  A lane reads its
//     table row's 4 consecutive k as one ds_read_b128, so MFMA step t of a 16-column group takes
//     k = 16 g + 4 (lane >> 4) + t from both operands -- a fixed permutation of the k order;
//   * the 16 x 16 accumulator tile (lane: table row lane & 15, users 4 (lane >> 4) + r) is compared
//     in place against each user's threshold key; survivors are appended
//     to the user's LDS candidate buffer (capacity KP + 32, KP = k rounded up to 16/32/64/128);
//   * a buffer that could overflow on the next tile (> KP + 16 entries) is pruned by its wave: a
//     the user's excluded ids are dropped from the buffer (the exclusion test runs here, on
//     survivors only, every candidate of the buffer against one excluded id at a time), then a
//     register bitonic sort of the padded buffer, the best k written back, the threshold raised to
//     the k-th key.  Worst case (a user's scores rising with the row index): every tile survives
//     and the user is pruned every second tile -- the wave sorts instead of multiplying, the
//     result is unchanged;
//   * at the end every user's buffer is sorted and its best k keys go to ws[b][split][k].
// topk_merge_kernel: one wave per user folds the S partial lists through the same sort (KP kept +
//   a chunk of new keys per round) and decodes keys into (score, id).
#include "common.h"
#include "launchers.h"

namespace {

typedef unsigned long long u64;

constexpr int TK_UB = 64;    // users per block: 4 waves x one 16-row A tile
constexpr int TK_ROWS = 16;  // table rows per LDS stage (one MFMA N tile)

__device__ __forceinline__ u64 tk_key(float s, int id) {
  uint32_t u = __float_as_uint(s);
  u = u == 0x80000000u ? 0u : u;                            // -0 ranks as +0
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);           // monotone: larger score, larger u
  return ((u64)u << 32) | (uint32_t)(~(uint32_t)id);        // smaller id, larger key
}

__device__ __forceinline__ void tk_decode(u64 key, float& s, int& id) {
  if (key == 0) {
    s = -INFINITY;
    id = -1;
    return;
  }
  uint32_t u = (uint32_t)(key >> 32);
  u = (u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u;
  s = __uint_as_float(u);
  id = (int)(~(uint32_t)key);
}

__device__ __forceinline__ u64 tk_shfl_idx(u64 v, int src) {
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src, 64);
  const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src, 64);
  return ((u64)hi << 32) | lo;
}

__device__ __forceinline__ u64 tk_shfl_xor(u64 v, int j) {
  const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, j, 64);
  const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), j, 64);
  return ((u64)hi << 32) | lo;
}

// Bitonic sort, descending, of the NPL * 64 keys element e = r * 64 + lane <- v[r] of one wave.
// Partner distances >= 64 are register pairs of a lane, smaller ones a lane exchange.  Every
// register index is a compile-time constant (no private memory).
// K0 = NPL * 64 runs the last phase only: the merge of a bitonic sequence (descending, then ascending).
template <int NPL, int K0 = 2>
__device__ __forceinline__ void tk_sort_desc(u64 (&v)[NPL], int lane) {
#pragma unroll
  for (int k = K0; k <= NPL * 64; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
      if (j >= 64) {
        const int jr = j >> 6;
#pragma unroll
        for (int r = 0; r < NPL; ++r) {
          if (r & jr) continue;
          const bool desc = ((r * 64) & k) == 0;  // k >= 128: the bit lies in r
          const u64 a = v[r], b = v[r | jr];
          const bool sw = desc ? a < b : a > b;
          v[r] = sw ? b : a;
          v[r | jr] = sw ? a : b;
        }
      } else {
#pragma unroll
        for (int r = 0; r < NPL; ++r) {
          const int e = r * 64 + lane;
          const u64 o = tk_shfl_xor(v[r], j);
          const bool take_max = ((lane & j) == 0) == ((e & k) == 0);
          const u64 hi = v[r] > o ? v[r] : o, lo = v[r] > o ? o : v[r];
          v[r] = take_max ? hi : lo;
        }
      }
    }
  }
}

// LDS traffic between the lanes of ONE wave (candidate buffers are wave-private): the hardware
// runs a wave's LDS operations in order; this keeps the compiler from moving them
__device__ __forceinline__ void tk_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int NK16, int KP>
struct TkCfg {
  static constexpr int DP = NK16 * 16;                 // D padded to whole 16-column groups
  static constexpr int LD = DP + 4;                    // LDS row stride: b128 row reads hit distinct banks
  static constexpr int CAP = KP + 32;                  // candidate slots per user
  static constexpr int TRIG = CAP - TK_ROWS;           // prune when a tile's 16 survivors might not fit
  static constexpr int NPL = KP <= 32 ? 1 : KP / 32;   // sorted keys per lane (NPL * 64 >= CAP)
  static constexpr int C4 = DP / 4;                    // float4 chunks per staged row
  static constexpr int NIT = (TK_ROWS * C4 + 255) / 256;
};

// the global loads of table tile t (rows clamped to N - 1, columns >= D zero): all issued
// before anything waits on them
template <typename C>
__device__ __forceinline__ void tk_tile_load(float4 (&st)[C::NIT], const float* __restrict__ table, int t, int N, int D,
                                             int tid) {
#pragma unroll
  for (int it = 0; it < C::NIT; ++it) {
    const int i = tid + 256 * it;
    const int row = min(i / C::C4, TK_ROWS - 1), c = (i % C::C4) * 4;
    const int n = min(t * TK_ROWS + row, N - 1);
    const float4 v = *(const float4*)(table + (size_t)n * D + min(c, D - 4));
    const bool z = c >= D;
    st[it] = make_float4(z ? 0.f : v.x, z ? 0.f : v.y, z ? 0.f : v.z, z ? 0.f : v.w);
  }
}

template <typename C>
__device__ __forceinline__ void tk_tile_store(const float4 (&st)[C::NIT], float* __restrict__ tile, int tid) {
#pragma unroll
  for (int it = 0; it < C::NIT; ++it) {
    const int i = tid + 256 * it;
    const int row = i / C::C4, c = (i - row * C::C4) * 4;
    if (i < TK_ROWS * C::C4) *(float4*)(tile + row * C::LD + c) = st[it];
  }
}

// the user's candidate buffer -> v (element e = r * 64 + lane; empty slots 0), the user's excluded
// ids ex[0..E) dropped (one wave-uniform load per entry, compared against every candidate at
// once: the exclusion test costs E loads per prune, not per survivor), sorted descending
template <typename C>
__device__ __forceinline__ int tk_load_sorted(u64 (&v)[C::NPL], const u64* __restrict__ ubuf, const int* ucnt,
                                              const int* __restrict__ ex, int E, int lane) {
  const int c = __builtin_amdgcn_readfirstlane(*ucnt);
#pragma unroll
  for (int r = 0; r < C::NPL; ++r) {
    const int e = r * 64 + lane;
    const u64 x = ubuf[min(e, C::CAP - 1)];
    v[r] = e < c ? x : 0ull;
  }
  if (ex != nullptr) {
    for (int e = 0; e < E; ++e) {
      const uint32_t x = ~(uint32_t)ex[e];  // the key's low word of id ex[e] (an empty slot's is ~(-1))
#pragma unroll
      for (int r = 0; r < C::NPL; ++r) v[r] = (uint32_t)v[r] == x ? 0ull : v[r];
    }
  }
  tk_sort_desc<C::NPL>(v, lane);
  return c;
}

template <int NK16, int KP>
__global__ __launch_bounds__(256) void topk_partial_kernel(const float* __restrict__ user,
                                                           const float* __restrict__ table,
                                                           const int* __restrict__ exclude, u64* __restrict__ ws, int B,
                                                           int N, int D, int E, int k, int min_id, int tiles_per_split,
                                                           int S) {
  typedef TkCfg<NK16, KP> C;
  __shared__ __attribute__((aligned(16))) float tile[2][TK_ROWS * C::LD];
  __shared__ u64 buf[TK_UB][C::CAP];
  __shared__ u64 thr[TK_UB];
  __shared__ int cnt[TK_UB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fq = lane >> 4;
  const int b0 = blockIdx.x * TK_UB, split = blockIdx.y;
  const int T = (N + TK_ROWS - 1) / TK_ROWS;
  const int t0 = split * tiles_per_split, t1 = min(T, t0 + tiles_per_split);
  if (tid < TK_UB) {
    thr[tid] = 0ull;
    cnt[tid] = 0;
  }
  // A fragments: user row 16 wave + fr, columns 16 g + 4 fq + (0..3)
  float a[NK16][4];
  {
    const int ub = b0 + wave * 16 + fr;
    const float* up = user + (size_t)min(ub, B - 1) * D;
#pragma unroll
    for (int g = 0; g < NK16; ++g) {
      const int c = 16 * g + 4 * fq;
      const float4 v = *(const float4*)(up + min(c, D - 4));
      const bool z = c >= D || ub >= B;
      a[g][0] = z ? 0.f : v.x;
      a[g][1] = z ? 0.f : v.y;
      a[g][2] = z ? 0.f : v.z;
      a[g][3] = z ? 0.f : v.w;
    }
  }
  float4 st[C::NIT];
  if (t0 < t1) {
    tk_tile_load<C>(st, table, t0, N, D, tid);
    tk_tile_store<C>(st, tile[0], tid);
  }
  __syncthreads();
  for (int t = t0; t < t1; ++t) {
    const int cur = (t - t0) & 1;
    const bool more = t + 1 < t1;
    if (more) tk_tile_load<C>(st, table, t + 1, N, D, tid);
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    {
      const float* tp = tile[cur] + fr * C::LD + 4 * fq;
#pragma unroll
      for (int g = 0; g < NK16; ++g) {
        const float4 bv = *(const float4*)(tp + 16 * g);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[g][0], bv.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[g][1], bv.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[g][2], bv.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[g][3], bv.w, acc, 0, 0, 0);
      }
    }
    // select: lane = table row n, users 4 fq + r of this wave
    const int n = t * TK_ROWS + fr;
    const bool nok = n < N && n >= min_id;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int ul = wave * 16 + 4 * fq + r;
      const float s = acc[r];
      const u64 key = tk_key(s, n);
      const bool ok = nok && b0 + ul < B && s == s && key > thr[ul];
      if (ok) {  // (excluded rows too: they are dropped when the buffer is pruned)
        const int pos = atomicAdd(&cnt[ul], 1);  // <= TRIG before the tile, <= 16 per tile: pos < CAP
        if (pos < C::CAP) buf[ul][pos] = key;
      }
    }
    tk_wave_sync();
    {
      const int c = lane < 16 ? cnt[wave * 16 + lane] : 0;
      u64 m = __ballot(c > C::TRIG);
      while (m != 0) {
        const int ul = __builtin_amdgcn_readfirstlane(wave * 16 + (__ffsll((long long)m) - 1));
        m &= m - 1;
        u64 v[C::NPL];
        const int c0 = tk_load_sorted<C>(v, buf[ul], &cnt[ul],
                                         exclude != nullptr ? exclude + (size_t)(b0 + ul) * E : nullptr, E, lane);
        tk_wave_sync();
#pragma unroll
        for (int r = 0; r < C::NPL; ++r) {
          const int e = r * 64 + lane;
          if (e < k) buf[ul][e] = v[r];
          if (e == k - 1) thr[ul] = v[r];
        }
        if (lane == 0) cnt[ul] = min(c0, k);
        tk_wave_sync();
      }
    }
    if (more) tk_tile_store<C>(st, tile[cur ^ 1], tid);
    __syncthreads();
  }
  // every user's best k of this split, sorted
  for (int uu = 0; uu < 16; ++uu) {
    const int ul = wave * 16 + uu, gb = b0 + ul;
    if (gb >= B) break;  // wave-uniform
    u64 v[C::NPL];
    (void)tk_load_sorted<C>(v, buf[ul], &cnt[ul], exclude != nullptr ? exclude + (size_t)gb * E : nullptr, E, lane);
    u64* dst = ws + ((size_t)gb * S + split) * k;
#pragma unroll
    for (int r = 0; r < C::NPL; ++r) {
      const int e = r * 64 + lane;
      if (e < k) dst[e] = v[r];
    }
  }
}

// one wave per user: the S sorted partial lists -> the best k, decoded.  The running best (sorted,
// elements [0, k)) and one more list laid out ascending at the top end form a bitonic sequence:
// each list costs the sort's last phase only; a list whose head is below the k-th best is skipped
template <int KP>
__global__ __launch_bounds__(64) void topk_merge_kernel(const u64* __restrict__ ws, float* __restrict__ scores,
                                                        int* __restrict__ ids, int S, int k) {
  constexpr int NPL = KP <= 32 ? 1 : KP / 32;
  constexpr int M = NPL * 64;
  const int lane = threadIdx.x;
  const u64* list = ws + (size_t)blockIdx.x * S * k;
  u64 v[NPL];
#pragma unroll
  for (int r = 0; r < NPL; ++r) v[r] = 0ull;
  u64 kth = 0ull;  // the current k-th best (0: fewer than k so far)
  for (int sp = 0; sp < S; ++sp, list += k) {
    if (list[0] <= kth) continue;  // wave-uniform (a list is sorted: nothing in it can enter)
#pragma unroll
    for (int r = 0; r < NPL; ++r) {
      const int i = M - 1 - (r * 64 + lane);  // element M - 1 - i <- list[i]
      const u64 x = list[min(i, k - 1)];
      if (r * 64 + lane >= M - KP) v[r] = i < k ? x : 0ull;
    }
    tk_sort_desc<NPL, M>(v, lane);
#pragma unroll
    for (int r = 0; r < NPL; ++r) {
      const int e = r * 64 + lane;
      v[r] = e < k ? v[r] : 0ull;
      const u64 q = tk_shfl_idx(v[r], (k - 1) & 63);
      if (((k - 1) >> 6) == r) kth = q;
    }
  }
#pragma unroll
  for (int r = 0; r < NPL; ++r) {
    const int e = r * 64 + lane;
    if (e < k) {
      float s;
      int id;
      tk_decode(v[r], s, id);
      scores[(size_t)blockIdx.x * k + e] = s;
      ids[(size_t)blockIdx.x * k + e] = id;
    }
  }
}

int g_topk_splits = 0;  // 0 = the launcher's choice (tests force 1, 2, 7)

template <int NK16, int KP>
void tk_launch(const float* user, const float* table, const int* exclude, u64* ws, int B, int N, int D, int E, int k,
               int min_id, int tps, int S, hipStream_t s) {
  hipLaunchKernelGGL((topk_partial_kernel<NK16, KP>), dim3((B + TK_UB - 1) / TK_UB, S), dim3(256), 0, s, user, table,
                     exclude, ws, B, N, D, E, k, min_id, tps, S);
}

template <int NK16>
void tk_launch_k(int KP, const float* user, const float* table, const int* exclude, u64* ws, int B, int N, int D,
                 int E, int k, int min_id, int tps, int S, hipStream_t s) {
  if (KP == 16)
    tk_launch<NK16, 16>(user, table, exclude, ws, B, N, D, E, k, min_id, tps, S, s);
  else if (KP == 32)
    tk_launch<NK16, 32>(user, table, exclude, ws, B, N, D, E, k, min_id, tps, S, s);
  else if (KP == 64)
    tk_launch<NK16, 64>(user, table, exclude, ws, B, N, D, E, k, min_id, tps, S, s);
  else
    tk_launch<NK16, 128>(user, table, exclude, ws, B, N, D, E, k, min_id, tps, S, s);
}

bool tk_shape_ok(long B, long N, int D, long E, int k) {
  return B >= 1 && N >= 1 && N < 2147483648L && B < 2147483648L && E >= 0 && E < 2147483648L && k >= 1 && k <= 128 &&
         D >= 4 && D <= 512 && D % 4 == 0;
}

}  // namespace

extern "C" void fr_topk_set_splits(int s) { g_topk_splits = s < 0 ? 0 : s; }

// the number of table splits a launch of this shape uses (the workspace is [B, S, k] u64)
extern "C" int fr_topk_splits(long B, long N) {
  const long T = (N + TK_ROWS - 1) / TK_ROWS;
  long S = g_topk_splits;
  if (S <= 0) {
    // ~2 resident blocks on each of the 256 CUs, at least 8 table tiles per split
    const long rt = (B + TK_UB - 1) / TK_UB;
    S = (512 + rt - 1) / rt;
    if (S > T / 8) S = T / 8;
    if (S > 64) S = 64;
  }
  if (S > T) S = T;
  if (S < 1) S = 1;
  const long tps = (T + S - 1) / S;
  return (int)((T + tps - 1) / tps);  // no empty split
}

// 0 ok; 1 unsupported shape; 2 misaligned pointer.  ws: u64 [B, fr_topk_splits(B, N), k]
extern "C" int fr_topk_scores(const float* user, const float* table, const int* exclude, void* ws, float* scores,
                              int* ids, long B, long N, int D, long E, int k, int min_id, hipStream_t s) {
  if (!tk_shape_ok(B, N, D, E, k)) return 1;
  if ((((uintptr_t)user) & 15) || (((uintptr_t)table) & 15) || (((uintptr_t)ws) & 7)) return 2;
  const int S = fr_topk_splits(B, N);
  const long T = (N + TK_ROWS - 1) / TK_ROWS;
  const int tps = (int)((T + S - 1) / S);
  if ((B + TK_UB - 1) / TK_UB > 2147483647L || S > 65535) return 1;
  const int KP = k <= 16 ? 16 : (k <= 32 ? 32 : (k <= 64 ? 64 : 128));
  const int* ex = E > 0 ? exclude : nullptr;
  u64* w = (u64*)ws;
  if (D <= 128)
    tk_launch_k<8>(KP, user, table, ex, w, (int)B, (int)N, D, (int)E, k, min_id, tps, S, s);
  else if (D <= 400)
    tk_launch_k<25>(KP, user, table, ex, w, (int)B, (int)N, D, (int)E, k, min_id, tps, S, s);
  else
    tk_launch_k<32>(KP, user, table, ex, w, (int)B, (int)N, D, (int)E, k, min_id, tps, S, s);
  if (KP == 16)
    hipLaunchKernelGGL(topk_merge_kernel<16>, dim3((unsigned)B), dim3(64), 0, s, w, scores, ids, S, k);
  else if (KP == 32)
    hipLaunchKernelGGL(topk_merge_kernel<32>, dim3((unsigned)B), dim3(64), 0, s, w, scores, ids, S, k);
  else if (KP == 64)
    hipLaunchKernelGGL(topk_merge_kernel<64>, dim3((unsigned)B), dim3(64), 0, s, w, scores, ids, S, k);
  else
    hipLaunchKernelGGL(topk_merge_kernel<128>, dim3((unsigned)B), dim3(64), 0, s, w, scores, ids, S, k);
  return 0;
}
