// Count-sketch uploads (FetchSGD: Rothchild et al. 2020): the sketch of a round delta, its median-of-rows estimate,
// the weighted sum of W sketches onto an error table, and the clearing of the buckets of recovered coordinates.
//
// The hash (ops/reference.py sketch_plan is the same contract in torch) is a block permutation, so that a bucket can
// GATHER its inputs in a fixed order and no float atomic is needed.  T = 1024 is the tile, C (a power of two >= T) the
// buckets of a row, G = C / T, R in {1, 3, 5} the rows, nb = ceil(n / C) the blocks.  Coordinate i is (q, p_hi, p_lo)
// = (i / C, (i % C) / T, i % T); row r sends it to bucket j_hi T + j_lo with
//   j_hi = (p_hi + rot_q) & (G - 1)                one tile rotation per block, shared by the rows
//   j_lo = (p_lo m + o) & (T - 1)                  m odd, so p_lo = ((j_lo - o) minv) & (T - 1), m minv = 1 mod 2^32
//   sign = -1 iff bit 31 of fmix32(uint32(i) ^ sx) the murmur3 finaliser
// plan int32 [nb, 8, 4]: slot r < 5 of block q holds (m, o, sx, minv) of row r, slot 7 holds rot_q.  Inside a block
// every row is a bijection: bucket (r, j) takes exactly one coordinate of every block.  Every index below is masked
// with T - 1 or G - 1 before it is used, so the kernels stay in bounds whatever the plan holds.
//
// sketch_delta: local, global [n] fp32 -> S [R, C].  a_i = local_i - global_i (one fp32 subtraction); every bucket
// starts at +0.0 and adds +a_i or -a_i of its coordinate of block q for q = 0, 1, .. in that order (one fp32 addition
// per block; a coordinate i >= n adds a zero, which changes no bit: the sum is never -0.0).  The result depends on (n,
// R, C, seed) and the inputs only -- there is no grid to show.  One workgroup of 256 threads owns output tile j_hi of
// all R rows with R x 4 accumulators per thread in registers.  Per block q the tile's sources are ONE contiguous run
// of T coordinates, q C + p_hi T with p_hi = (j_hi - rot_q) & (G - 1): each thread loads 16 bytes of local and of
// global (a ragged last run, or pointers that are not 16-byte aligned such as a view x[1:], element by element),
// subtracts and puts a into one half of an 8 KB LDS ring; the loads of block q + 1 are issued before block q is
// gathered.  Thread t owns buckets j_lo = t + 256 e: a wave's 64 inverse positions ((j_lo - o) minv) step by the odd
// minv, so they spread evenly over the LDS banks.  Global traffic: 8 n bytes read once, 4 R C written; no atomics, no
// second pass.
//
// sketch_estimate: S [R, C] -> est [n]: est_i = the median over r of sign_r(i) S[r][h_r(i)] under the monotone uint32
// key of robust_agg.hip (NaN -> 0xFFFFFFFF; sign bit set -> ~bits; else bits | 0x80000000: -0.0 < +0.0), turned back
// into its float (the NaN key comes back as 0x7FFFFFFF).  One workgroup per source tile (q, p_hi): the R table tiles
// it hashes into (20 KB at R = 5) are loaded with 16-byte loads into LDS, thread t takes coordinates p_lo = t + 256 e
// (the forward positions p_lo m + o step by the odd m: spread over the banks again), the median is a compile-time
// min / max network on the keys, and the stores of a wave are 256 contiguous bytes.
//
// sketch_accumulate: E [L] += (sum over c < W in order of w_c S_c[.]) / (w_0 + .. + w_{W-1}), every product, sum,
// the division and the final addition rounded on its own (the convention of dequant_combine); register-direct 16-byte
// loads with client c + 1 in flight during the adds of client c; W <= 32, L a multiple of 4, 16-byte aligned rows.
//
// sketch_clear: E[r][h_r(i)] = +0.0 for every i of idx [k] and every row; an index outside [0, nb C) is skipped.
// Zeroing is idempotent, so two members that share a bucket need no order.
#include "common.h"
#include "launchers.h"

// every sum, product and difference below is rounded on its own, whatever flags build this file
#pragma clang fp contract(off)

namespace {

constexpr int BLOCK = 256;
constexpr uint32_t T = 1024;  // the tile
constexpr int PER = T / BLOCK;  // buckets (or coordinates) of a tile per thread

__device__ __forceinline__ uint32_t fmix32(uint32_t h) {
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  return h ^ (h >> 16);
}

// x with its sign bit flipped iff bit 31 of h is set
__device__ __forceinline__ float signed_by(float x, uint32_t h) {
  return __uint_as_float(__float_as_uint(x) ^ (h & 0x80000000u));
}

__device__ __forceinline__ uint32_t key_of(float x) {
  const uint32_t b = __float_as_uint(x);
  const uint32_t k = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  return (b & 0x7FFFFFFFu) > 0x7F800000u ? 0xFFFFFFFFu : k;
}
__device__ __forceinline__ float value_of(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

__device__ __forceinline__ uint32_t umin(uint32_t a, uint32_t b) { return a < b ? a : b; }
__device__ __forceinline__ uint32_t umax(uint32_t a, uint32_t b) { return a > b ? a : b; }
__device__ __forceinline__ uint32_t med3(uint32_t a, uint32_t b, uint32_t c) {
  return umax(umin(a, b), umin(umax(a, b), c));
}
template <int R>
__device__ __forceinline__ uint32_t median(const uint32_t (&k)[R]) {
  if constexpr (R == 1) return k[0];
  if constexpr (R == 3) return med3(k[0], k[1], k[2]);
  if constexpr (R == 5) {
    // the lowest and the highest of four cannot be the median of five
    const uint32_t f = umax(umin(k[0], k[1]), umin(k[2], k[3])), g = umin(umax(k[0], k[1]), umax(k[2], k[3]));
    return med3(k[4], f, g);
  }
}

// a[4 t .. 4 t + 3] of the run that starts at coordinate i0: local - global, +0.0 past n
__device__ __forceinline__ void load_run(const float* __restrict__ local, const float* __restrict__ global, uint32_t i0,
                                         uint32_t n, int vec, f32x4& l, f32x4& g) {
  const uint32_t i = i0 + 4u * threadIdx.x;
  if (vec && i0 + T <= n) {
    l = *reinterpret_cast<const f32x4*>(local + i);
    g = *reinterpret_cast<const f32x4*>(global + i);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool in = i + e < n;
      l[e] = in ? local[i + e] : 0.f;
      g[e] = in ? global[i + e] : 0.f;
    }
  }
}

template <int R>
__global__ __launch_bounds__(BLOCK) void sketch_delta_kernel(const float* __restrict__ local,
                                                            const float* __restrict__ global,
                                                            const uint32_t* __restrict__ plan, float* __restrict__ S,
                                                            uint32_t n, uint32_t nb, uint32_t C, int vec) {
  __shared__ __attribute__((aligned(16))) float ring[2][T];
  const uint32_t G = C / T, j_hi = blockIdx.x, t = threadIdx.x;
  float acc[R][PER];
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int e = 0; e < PER; ++e) acc[r][e] = 0.f;
  f32x4 l, g;
  uint32_t i0 = ((j_hi - plan[28]) & (G - 1)) * T;  // block 0's run
  load_run(local, global, i0, n, vec, l, g);
  for (uint32_t q = 0; q < nb; ++q) {
    const uint32_t* __restrict__ pq = plan + 32u * q;
    float* buf = ring[q & 1];
    *reinterpret_cast<f32x4*>(buf + 4 * t) = f32x4{l[0] - g[0], l[1] - g[1], l[2] - g[2], l[3] - g[3]};
    const uint32_t cur = i0;
    if (q + 1 < nb) {  // in flight across this block's gather
      i0 = (q + 1) * C + ((j_hi - pq[32 + 28]) & (G - 1)) * T;
      load_run(local, global, i0, n, vec, l, g);
    }
    // one barrier per block: the half written here was last read two blocks ago, before the barrier of the block between
    __syncthreads();
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const uint32_t o = pq[4 * r + 1], sx = pq[4 * r + 2], minv = pq[4 * r + 3];
#pragma unroll
      for (int e = 0; e < PER; ++e) {
        const uint32_t p_lo = ((t + BLOCK * e - o) * minv) & (T - 1);
        acc[r][e] = acc[r][e] + signed_by(buf[p_lo], fmix32((cur + p_lo) ^ sx));
      }
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int e = 0; e < PER; ++e) S[(size_t)r * C + j_hi * T + t + BLOCK * e] = acc[r][e];
}

template <int R>
__global__ __launch_bounds__(BLOCK) void sketch_estimate_kernel(const float* __restrict__ S,
                                                               const uint32_t* __restrict__ plan,
                                                               float* __restrict__ est, uint32_t n, uint32_t C) {
  __shared__ __attribute__((aligned(16))) float tile[R][T];
  const uint32_t G = C / T, q = blockIdx.x / G, p_hi = blockIdx.x % G, t = threadIdx.x;
  const uint32_t* __restrict__ pq = plan + 32u * q;
  const uint32_t j_hi = (p_hi + pq[28]) & (G - 1), i0 = q * C + p_hi * T;
  if (i0 >= n) return;  // (workgroup-uniform: before the barrier)
#pragma unroll
  for (int r = 0; r < R; ++r)
    *reinterpret_cast<f32x4*>(&tile[r][4 * t]) = *reinterpret_cast<const f32x4*>(S + (size_t)r * C + j_hi * T + 4 * t);
  __syncthreads();
  uint32_t key[PER][R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const uint32_t m = pq[4 * r], o = pq[4 * r + 1], sx = pq[4 * r + 2];
#pragma unroll
    for (int e = 0; e < PER; ++e) {
      const uint32_t p_lo = t + BLOCK * e;
      key[e][r] = key_of(signed_by(tile[r][(p_lo * m + o) & (T - 1)], fmix32((i0 + p_lo) ^ sx)));
    }
  }
#pragma unroll
  for (int e = 0; e < PER; ++e) {
    const uint32_t i = i0 + t + BLOCK * e;
    if (i < n) est[i] = value_of(median<R>(key[e]));
  }
}

__global__ __launch_bounds__(BLOCK) void sketch_accumulate_kernel(float* __restrict__ E, const float* __restrict__ stack,
                                                                 const float* __restrict__ wts, int W, uint32_t L) {
  const uint32_t i = 4u * (blockIdx.x * BLOCK + threadIdx.x);
  if (i >= L) return;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  float ws = 0.f;
  f32x4 cur = *reinterpret_cast<const f32x4*>(stack + i);
  for (int c = 0; c < W; ++c) {
    f32x4 nxt = cur;
    if (c + 1 < W) nxt = *reinterpret_cast<const f32x4*>(stack + (size_t)(c + 1) * L + i);  // before this client's adds
    const float w = wts[c];
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] = acc[e] + w * cur[e];
    ws = ws + w;
    cur = nxt;
  }
  f32x4 x = *reinterpret_cast<const f32x4*>(E + i);
#pragma unroll
  for (int e = 0; e < 4; ++e) x[e] = x[e] + acc[e] / ws;
  *reinterpret_cast<f32x4*>(E + i) = x;
}

template <int R>
__global__ __launch_bounds__(BLOCK) void sketch_clear_kernel(float* __restrict__ E, const int* __restrict__ idx,
                                                            const uint32_t* __restrict__ plan, uint32_t k, uint32_t nb,
                                                            uint32_t C) {
  const uint32_t s = blockIdx.x * BLOCK + threadIdx.x;
  if (s >= k) return;
  const uint32_t i = (uint32_t)idx[s], q = i / C;
  if (q >= nb) return;  // (a negative index too: it is >= 2^31 here)
  const uint32_t* pq = plan + 32u * q;
  const uint32_t j_hi = (((i % C) / T) + pq[28]) & (C / T - 1), p_lo = i % T;
#pragma unroll
  for (int r = 0; r < R; ++r) E[(size_t)r * C + j_hi * T + ((p_lo * pq[4 * r] + pq[4 * r + 1]) & (T - 1))] = 0.f;
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// rows in {1, 3, 5}, cols a power of two in [T, 2^30], 1 <= n < 2^31 and nb blocks that cover n
inline bool shape_ok(int R, long C, long n, long nb) {
  return (R == 1 || R == 3 || R == 5) && C >= (long)T && C <= (1L << 30) && (C & (C - 1)) == 0 && n >= 1 &&
         n < (1L << 31) && nb == (n + C - 1) / C;
}

}  // namespace

// 1: a shape outside shape_ok; 2: a pointer that is not 4-byte aligned (S: 16-byte); 3: a runtime error
extern "C" int fr_sketch_delta(const float* local, const float* global, const int* plan, float* S, long n, int nb,
                               int R, long C, hipStream_t s) {
  if (!shape_ok(R, C, n, nb)) return 1;
  if ((((uintptr_t)local | (uintptr_t)global | (uintptr_t)plan) & 3u) || !aligned16(S)) return 2;
  const int vec = aligned16(local) && aligned16(global);
  const dim3 grid((unsigned)(C / T)), blk(BLOCK);
  const uint32_t* p = reinterpret_cast<const uint32_t*>(plan);
#define FR_SKETCH_DELTA(RR) \
  hipLaunchKernelGGL(sketch_delta_kernel<RR>, grid, blk, 0, s, local, global, p, S, (uint32_t)n, (uint32_t)nb, (uint32_t)C, vec)
  if (R == 1) FR_SKETCH_DELTA(1);
  else if (R == 3) FR_SKETCH_DELTA(3);
  else FR_SKETCH_DELTA(5);
#undef FR_SKETCH_DELTA
  return hipGetLastError() == hipSuccess ? 0 : 3;
}

extern "C" int fr_sketch_estimate(const float* S, const int* plan, float* est, long n, int nb, int R, long C,
                                  hipStream_t s) {
  if (!shape_ok(R, C, n, nb)) return 1;
  if ((((uintptr_t)est | (uintptr_t)plan) & 3u) || !aligned16(S)) return 2;
  const dim3 grid((unsigned)(nb * (C / T))), blk(BLOCK);
  const uint32_t* p = reinterpret_cast<const uint32_t*>(plan);
  if (R == 1) hipLaunchKernelGGL(sketch_estimate_kernel<1>, grid, blk, 0, s, S, p, est, (uint32_t)n, (uint32_t)C);
  else if (R == 3) hipLaunchKernelGGL(sketch_estimate_kernel<3>, grid, blk, 0, s, S, p, est, (uint32_t)n, (uint32_t)C);
  else hipLaunchKernelGGL(sketch_estimate_kernel<5>, grid, blk, 0, s, S, p, est, (uint32_t)n, (uint32_t)C);
  return hipGetLastError() == hipSuccess ? 0 : 3;
}

// E [L] and stack [W, L].  1: a shape outside 1 <= W <= 32, 4 <= L < 2^31, L % 4 == 0; 2: E or stack not 16-byte
// aligned, weights not 4-byte aligned; 3: a runtime error
extern "C" int fr_sketch_accumulate(float* E, const float* stack, const float* weights, int W, long L, hipStream_t s) {
  if (W < 1 || W > 32 || L < 4 || L >= (1L << 31) || (L & 3)) return 1;
  if (!aligned16(E) || !aligned16(stack) || ((uintptr_t)weights & 3u)) return 2;
  const dim3 grid((unsigned)((L / 4 + BLOCK - 1) / BLOCK)), blk(BLOCK);
  hipLaunchKernelGGL(sketch_accumulate_kernel, grid, blk, 0, s, E, stack, weights, W, (uint32_t)L);
  return hipGetLastError() == hipSuccess ? 0 : 3;
}

// E [R, C], idx [k], plan of nb blocks.  1: a shape outside shape_ok (n = nb C) or k outside [0, 2^31); 2: a pointer
// that is not 4-byte aligned; 3: a runtime error
extern "C" int fr_sketch_clear(float* E, const int* idx, const int* plan, long k, int nb, int R, long C, hipStream_t s) {
  if (nb < 1 || (long)nb * C > (1L << 31) || !shape_ok(R, C, 1, 1) || k < 0 || k >= (1L << 31)) return 1;
  if (((uintptr_t)E | (uintptr_t)idx | (uintptr_t)plan) & 3u) return 2;
  if (k == 0) return 0;
  const dim3 grid((unsigned)((k + BLOCK - 1) / BLOCK)), blk(BLOCK);
  const uint32_t* p = reinterpret_cast<const uint32_t*>(plan);
  if (R == 1) hipLaunchKernelGGL(sketch_clear_kernel<1>, grid, blk, 0, s, E, idx, p, (uint32_t)k, (uint32_t)nb, (uint32_t)C);
  else if (R == 3) hipLaunchKernelGGL(sketch_clear_kernel<3>, grid, blk, 0, s, E, idx, p, (uint32_t)k, (uint32_t)nb, (uint32_t)C);
  else hipLaunchKernelGGL(sketch_clear_kernel<5>, grid, blk, 0, s, E, idx, p, (uint32_t)k, (uint32_t)nb, (uint32_t)C);
  return hipGetLastError() == hipSuccess ? 0 : 3;
}
