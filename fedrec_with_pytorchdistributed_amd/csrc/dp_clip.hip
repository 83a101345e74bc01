// Client-level differential privacy on a star client's round update (DP-FedAvg: McMahan, Ramage, Talwar,
// Zhang 2018): the delta local - base is clipped to an L2 norm and the client's share of the Gaussian noise
// goes on top, before anything leaves the client.  Two ops, three launches, nothing returns to the host
// between them: delta_sqnorm (chunk partials + finish) leaves the squared norm in a 16-byte state on the
// device, clip_noise reads it there.
//
// The contract (ops/reference.py dp_delta_sqnorm / dp_clip_noise are the same forms in torch):
//   * delta_sqnorm: d_k = local_k - base_k, one fp32 subtraction; sq = sum_k double(d_k)^2 (the square of an
//     fp32 value is exact in fp64, so the fma below and a separate product + sum hold the same bits).  The
//     order depends on n alone: chunk p covers [1024 p, 1024 (p + 1)); lane l of the wave that owns it takes
//     the coordinate quads l, l + 64, l + 128, l + 192 of the chunk and adds its 16 squares in ascending
//     coordinate order from +0.0; the 64 lane sums meet in an xor butterfly 32, 16, 8, 4, 2, 1; lane 0 writes
//     part[p].  The finish adds the partials as krum_finish_kernel does: slot t of 64 adds p = t, t + 64, ...
//     ascending from +0.0, then the slots in order.  Coordinates at and past n are zeros.  No float atomics:
//     sq is bitwise independent of the grid.
//   * clip_noise: s = fp32(min(1, clip / sqrt(sq))) with the root and the division in IEEE fp64, s = 1 where
//     sq is 0 or not finite (a non-finite model goes out as it is; the coordinator rejects it).  p_k = local_k
//     where s == 1 (bit for bit), else base_k + s * d_k, no FMA.  out_k = p_k when std == 0, else
//     p_k + std * z_k, no FMA, with z_k the box_muller normal of Philox(seed, offset) at counter k >> 2,
//     component k & 3 (words (x, y) make components 0 and 1, (z, w) 2 and 3).  clipped = (s < 1).
//
// dp_sqnorm_kernel<VEC> -- register-direct, no LDS.  One load instruction of a wave covers 64 lanes x 16 B = 1
// KB contiguous, eight whole 128-byte lines; the four local and four base loads of a chunk are issued back
// to back, and the NEXT chunk's eight loads are issued before the current chunk's squares and butterfly
// (two register sets of 32 VGPRs; 84 VGPRs and 5 waves per SIMD as compiled): 8 KB per wave are in flight
// across the sum, and the other waves of the SIMD cover the drain before the next issue.  VEC =
// false (n % 4 != 0, or a row that is not 16-byte aligned): the same coordinates by 4-byte loads, the same
// bits.  Traffic: 8 n bytes read, 8 bytes per 8 KB written.
// dp_finish_kernel -- one block of 1024: all threads stage 4096 partials at a time into LDS (four 8-byte
// loads in flight per thread, one latency per tile instead of one per dependent add), wave 0 adds its 64
// slots from LDS, thread 0 the slots.  P = 65,946 (67.5 M coordinates) is 17 tiles.
// dp_clip_noise_kernel<NOISE, VEC> -- a lane owns DP_Q = 4 coordinate quads per pass, 256 quads apart, so
// each of its loads and stores is again 1 KB contiguous per wave.  All 16-byte loads of a pass are issued
// first, then the DP_Q Philox calls (ten rounds of integer multiplies each: the integer pipe works under the
// memory latency), then the Box-Muller pairs, the clip and the stores.  Every thread derives s from sq by
// the same fp64 operations (a broadcast 8-byte load, one sqrt, one division: no launch of its own for
// it); thread 0 records s and clipped.  s == 1 never reads base; NOISE = false carries no RNG, and with s == 1
// it is a plain copy.  Traffic: 12 n bytes clipped, 8 n unclipped.
#include "common.h"
#include "launchers.h"

// s * d and the add that follows, std * z and its add are each rounded on their own whatever flags build
// this file: plain operators under this pragma (see sparse_delta.hip).  __fmul_rn / __fadd_rn do NOT say so:
// the HIP header defines them as x * y and x + y under its own contraction mode, and once inlined the
// backend fused them into v_fmac_f32 (the bitwise test at n = 1023 found it)
#pragma clang fp contract(off)

namespace {

constexpr int DP_L = 1024;     // coordinates per chunk
constexpr int DP_SLOTS = 64;   // partial sums in the finish
constexpr int DP_TILE = 4096;  // partials staged in LDS at a time (a multiple of DP_SLOTS)
constexpr int DP_Q = 4;        // coordinate quads per lane and pass in clip_noise

// the device state of one privatisation: 16 bytes
struct DpState {
  double sq;    // || local - base ||^2
  float s;      // the clip scale
  int clipped;  // s < 1
};

// four consecutive floats from p[k ..], zeros at and past n (VEC: k % 4 == 0 and n % 4 == 0).  No branch: a
// coordinate past n reads element 0 instead and is replaced by a select, so the loads of a chunk are
// issued back to back and counted, not fenced, by the wait that precedes their first use
template <bool VEC>
__device__ __forceinline__ f32x4 dp_load(const float* __restrict__ p, long k, long n) {
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  if constexpr (VEC) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(p + (k < n ? k : 0));
    return k < n ? v : zero;
  } else {
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float x = p[k + e < n ? k + e : 0];
      v[e] = k + e < n ? x : 0.f;
    }
    return v;
  }
}

template <bool VEC>
__device__ __forceinline__ void dp_store(float* __restrict__ p, long k, long n, const f32x4& v) {
  if constexpr (VEC) {
    if (k < n) *reinterpret_cast<f32x4*>(p + k) = v;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (k + e < n) p[k + e] = v[e];
  }
}

// chunk p's eight loads: quads lane, lane + 64, lane + 128, lane + 192 of local and of base
template <bool VEC>
__device__ __forceinline__ void dp_load_chunk(const float* __restrict__ local, const float* __restrict__ base, long p,
                                              int lane, long n, f32x4 (&a)[4], f32x4 (&b)[4]) {
  const long k0 = p * DP_L + 4 * lane;
#pragma unroll
  for (int j = 0; j < 4; ++j) a[j] = dp_load<VEC>(local, k0 + 256 * j, n);
#pragma unroll
  for (int j = 0; j < 4; ++j) b[j] = dp_load<VEC>(base, k0 + 256 * j, n);
}

// the chunk held in (a, b): 16 squares per lane in ascending coordinate order, the butterfly, part[p]
__device__ __forceinline__ void dp_chunk_sum(const f32x4 (&a)[4], const f32x4 (&b)[4], double* __restrict__ part, long p,
                                             int lane) {
  double acc = 0.0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const double d = (double)(a[j][e] - b[j][e]);
      acc = fma(d, d, acc);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc = acc + __shfl_xor(acc, o, 64);
  if (lane == 0) part[p] = acc;
}

template <bool VEC>
__global__ __launch_bounds__(256) void dp_sqnorm_kernel(const float* __restrict__ local, const float* __restrict__ base,
                                                        double* __restrict__ part, long n, long P) {
  const int lane = threadIdx.x & 63;
  const long nwaves = (long)gridDim.x * 4;
  long p = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (p >= P) return;
  f32x4 a[4], b[4];
  dp_load_chunk<VEC>(local, base, p, lane, n, a, b);
  while (p + nwaves < P) {  // wave-uniform; the next chunk's loads stay in flight across this chunk's sum
    f32x4 na[4], nb[4];
    dp_load_chunk<VEC>(local, base, p + nwaves, lane, n, na, nb);
    dp_chunk_sum(a, b, part, p, lane);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      a[j] = na[j];
      b[j] = nb[j];
    }
    p += nwaves;
  }
  dp_chunk_sum(a, b, part, p, lane);
}

__global__ __launch_bounds__(1024) void dp_finish_kernel(const double* __restrict__ part, DpState* __restrict__ st,
                                                         long P) {
  __shared__ double tile[DP_TILE];
  __shared__ double red[DP_SLOTS];
  const int t = threadIdx.x;
  double s = 0.0;
  for (long p0 = 0; p0 < P; p0 += DP_TILE) {
    const int cnt = P - p0 < DP_TILE ? (int)(P - p0) : DP_TILE;
    double v[DP_TILE / 1024];
#pragma unroll
    for (int u = 0; u < DP_TILE / 1024; ++u) v[u] = t + 1024 * u < cnt ? part[p0 + t + 1024 * u] : 0.0;
#pragma unroll
    for (int u = 0; u < DP_TILE / 1024; ++u) tile[t + 1024 * u] = v[u];
    __syncthreads();
    if (t < DP_SLOTS)  // p0 is a multiple of DP_SLOTS: tile[i] is partial p0 + i of slot i % DP_SLOTS
      for (int i = t; i < cnt; i += DP_SLOTS) s = s + tile[i];
    __syncthreads();
  }
  if (t < DP_SLOTS) red[t] = s;
  __syncthreads();
  if (t == 0) {
    double tot = red[0];
    for (int k = 1; k < DP_SLOTS; ++k) tot = tot + red[k];
    st->sq = tot;
    st->s = 0.f;  // clip_noise fills these two in
    st->clipped = 0;
  }
}

// fp32(min(1, clip / sqrt(sq))); 1 for sq == 0 and for a sq that is not finite (NaN compares false)
__device__ __forceinline__ float dp_scale(double sq, double clip) {
  if (!(sq > 0.0) || !(sq < (double)INFINITY)) return 1.f;
  const double r = clip / sqrt(sq);
  return r < 1.0 ? (float)r : 1.f;
}

// one pass of a lane: DP_Q quads, 256 quads apart.  FULL: every coordinate of the pass lies below n, so
// nothing is guarded and the pass is straight-line code: the loads go out first, the Philox rounds follow
// while they fly, and only then is the first loaded register touched (the fence keeps that order)
template <bool NOISE, bool VEC, bool CLIP, bool FULL>
__device__ __forceinline__ void dp_pass(const float* __restrict__ local, const float* __restrict__ base,
                                        float* __restrict__ out, long q0, long n, float s, float std,
                                        unsigned long long seed, unsigned long long offset) {
  const long lim = FULL ? 0x7fffffffffffffffL : n;  // a constant bound folds the selects and guards away
  f32x4 a[DP_Q], b[DP_Q];
#pragma unroll
  for (int u = 0; u < DP_Q; ++u) a[u] = dp_load<VEC>(local, 4 * (q0 + 256 * u), lim);
  if constexpr (CLIP) {  // an unclipped model never reads base
#pragma unroll
    for (int u = 0; u < DP_Q; ++u) b[u] = dp_load<VEC>(base, 4 * (q0 + 256 * u), lim);
  }
  uint4 w[DP_Q];
  if constexpr (NOISE) {
#pragma unroll
    for (int u = 0; u < DP_Q; ++u) w[u] = Philox::gen(seed, offset, (uint64_t)(q0 + 256 * u));
    __builtin_amdgcn_sched_barrier(0);
  }
#pragma unroll
  for (int u = 0; u < DP_Q; ++u) {
    f32x4 p = a[u];
    if constexpr (CLIP) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float sd = s * (a[u][e] - b[u][e]);
        p[e] = b[u][e] + sd;
      }
    }
    if constexpr (NOISE) {
      const float2 z01 = box_muller(w[u].x, w[u].y), z23 = box_muller(w[u].z, w[u].w);
      const float sz[4] = {std * z01.x, std * z01.y, std * z23.x, std * z23.y};
#pragma unroll
      for (int e = 0; e < 4; ++e) p[e] = p[e] + sz[e];
    }
    dp_store<VEC>(out, 4 * (q0 + 256 * u), lim, p);
  }
}

template <bool NOISE, bool VEC, bool CLIP>
__device__ __forceinline__ void dp_passes(const float* __restrict__ local, const float* __restrict__ base,
                                          float* __restrict__ out, long n, float s, float std, unsigned long long seed,
                                          unsigned long long offset) {
  const long nq = (n + 3) / 4, pass = (long)gridDim.x * (256 * DP_Q);
  for (long q0 = (long)blockIdx.x * (256 * DP_Q) + threadIdx.x; q0 < nq; q0 += pass) {
    if (4 * (q0 + 256 * (DP_Q - 1)) + 3 < n)  // the lane's last coordinate: true for whole waves but the tail's
      dp_pass<NOISE, VEC, CLIP, true>(local, base, out, q0, n, s, std, seed, offset);
    else
      dp_pass<NOISE, VEC, CLIP, false>(local, base, out, q0, n, s, std, seed, offset);
  }
}

template <bool NOISE, bool VEC>
__global__ __launch_bounds__(256) void dp_clip_noise_kernel(const float* __restrict__ local,
                                                            const float* __restrict__ base, float* __restrict__ out,
                                                            DpState* __restrict__ st, long n, double clip, float std,
                                                            unsigned long long seed, unsigned long long offset) {
  const float s = dp_scale(st->sq, clip);  // the same bits in every thread
  const bool clipped = s < 1.f;            // uniform over the grid
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    st->s = s;
    st->clipped = clipped ? 1 : 0;
  }
  if (clipped) dp_passes<NOISE, VEC, true>(local, base, out, n, s, std, seed, offset);
  else dp_passes<NOISE, VEC, false>(local, base, out, n, s, std, seed, offset);
}

bool dp_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

// doubles of scratch fr_dp_delta_sqnorm needs for n coordinates: one partial per chunk
extern "C" long fr_dp_sqnorm_ws(long n) { return n < 1 ? -1 : (n + DP_L - 1) / DP_L; }

// local, base [n] fp32 -> state (16 bytes: sq fp64, s fp32 = 0, clipped int32 = 0).  max_blocks > 0 caps the
// grid (sq does not depend on it).  1: n < 1
extern "C" int fr_dp_delta_sqnorm(const float* local, const float* base, double* part, void* state, long n,
                                  int max_blocks, hipStream_t s) {
  if (n < 1) return 1;
  const long P = (n + DP_L - 1) / DP_L;
  long grid = (P + 3) / 4;
  const long cap = max_blocks > 0 ? max_blocks : (long)fr_num_cus() * 8;
  grid = grid < cap ? grid : cap;
  const bool vec = n % 4 == 0 && dp_aligned(local) && dp_aligned(base);
  const dim3 g((unsigned)grid), b(256);
  if (vec) hipLaunchKernelGGL((dp_sqnorm_kernel<true>), g, b, 0, s, local, base, part, n, P);
  else hipLaunchKernelGGL((dp_sqnorm_kernel<false>), g, b, 0, s, local, base, part, n, P);
  hipLaunchKernelGGL(dp_finish_kernel, dim3(1), dim3(1024), 0, s, part, static_cast<DpState*>(state), P);
  return 0;
}

// out [n] = the delta clipped to L2 norm `clip` on top of base, plus std x the normals of Philox(seed, offset);
// state as fr_dp_delta_sqnorm left it for the same local and base, s and clipped are filled in.  out must
// not overlap local or base.  1: n < 1, 2: clip is not positive, 3: std is negative or not finite
extern "C" int fr_dp_clip_noise(const float* local, const float* base, float* out, void* state, long n, double clip,
                                float std, unsigned long long seed, unsigned long long offset, hipStream_t s) {
  if (n < 1) return 1;
  if (!(clip > 0.0)) return 2;
  if (!(std >= 0.f) || !(std < INFINITY)) return 3;
  const bool vec = n % 4 == 0 && dp_aligned(local) && dp_aligned(base) && dp_aligned(out);
  const long nq = (n + 3) / 4, need = (nq + 256 * DP_Q - 1) / (256 * DP_Q), cap = (long)fr_num_cus() * 8;
  const dim3 g((unsigned)(need < cap ? need : cap)), b(256);
  DpState* st = static_cast<DpState*>(state);
#define DP_LAUNCH(NOISE, VEC) \
  hipLaunchKernelGGL((dp_clip_noise_kernel<NOISE, VEC>), g, b, 0, s, local, base, out, st, n, clip, std, seed, offset)
  if (std > 0.f) {
    if (vec) DP_LAUNCH(true, true);
    else DP_LAUNCH(true, false);
  } else {
    if (vec) DP_LAUNCH(false, true);
    else DP_LAUNCH(false, false);
  }
#undef DP_LAUNCH
  return 0;
}
