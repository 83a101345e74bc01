// Geometric-median aggregation (RFA: Pillutla, Kakade, Harchaoui 2022) of W <= 32 client vectors by
// Weiszfeld's iteration run on the Gram matrix instead of on the stack.  Every iterate lies in the
// affine span of the rows, z = center + sum_c a_c y_c (y_c = x_c - center, sum a = 1), so
//   ||x_i - z||^2 = G_ii - 2 (G a)_i + a^T G a
// with G = Y Y^T from krum.hip's centered_gram: the iteration needs W numbers per client, not n.
// Two launches behind the Gram, no host synchronisation between them.
//
// The contract (ops/reference.py geomed_weights / geomed_combine are the same forms in torch):
//   * weights: client c is valid iff G_cc is finite; nu2 = 1e-12 m + 1e-300 with m the lower median of
//     the valid G_cc; a = 1 / nv on the nv valid clients, 0 elsewhere; then exactly GM_ITERS = 32
//     rounds, all fp64, every product and sum rounded on its own (no FMA):
//       g_c = sum_j Gm_cj a_j, j ascending from +0.0 (Gm: G with the columns of invalid clients zeroed),
//       q = sum_c p_c, p_c = a_c g_c on valid c and 0 elsewhere, c ascending from +0.0,
//       d2_c = max((G_cc - 2 g_c) + q, 0), w_c = 1 / sqrt(d2_c + nu2) on valid c and 0 elsewhere,
//       a_c = w_c / s, s = sum_c w_c, c ascending from +0.0.
//     dist_c = fp32(sqrt(d2_c)) of the last round, +inf for an invalid client; no valid client: a = NaN.
//   * combine: a32 = fp32(a); out = a32_{c0} x_{c0}, then + a32_c x_c over the clients with a32_c != 0 in
//     client order, product and sum rounded separately in fp32.  Rows of weight zero are never read.
//
// geomed_weights_kernel -- one wave, lane c = client c.  The lane loads row c of G once into 32 fp64
// registers (columns of invalid clients and columns >= W become zeros there) and never touches memory
// again until it writes a_c and dist_c.  a_j reaches the other lanes by v_readlane_b32 with a
// compile-time j (two per double, into an SGPR pair that feeds v_mul_f64 directly): no LDS, no
// ds_bpermute in the loop.  q and s are taken the same way, lane 0 .. W - 1 in ascending order, so
// every lane holds the same bits and they are the oracle's.  Validity is data (a zeroed column, a
// v_cndmask): the only branches are on j < W, uniform over the wave.  fp64 division and sqrt are the
// compiler's IEEE expansions (no -ffast-math, no rcp / rsq shortcuts).
//   budget: 87 VGPRs as compiled (64 of row + state), one wave on one SIMD; per round 3 W readlane
//     pairs and 3 W dependent fp64 adds, one division and one sqrt + division.  Measured as one
//     event-timed launch (launch included): 41 us at W = 4, 47 at W = 8, 75 at W = 32
//     (docs/PERFORMANCE.md 0a-8); the kernel alone was not traced.
//
// geomed_combine_kernel<V> -- thread 0 of a block compacts the (row, a32) pairs with a32 != 0 into
// LDS once; a lane owns V consecutive coordinates (V = 4: 16-byte loads and stores, taken when n % 4
// == 0 and stack and out are 16-byte aligned; V = 1 otherwise, the same bits); eight row loads are
// issued before the first multiply-add of the group and the adds then run strictly in client order;
// the first contributing row initialises the accumulator (no 0 + x, which would turn -0.0 to +0.0).
// Grid-stride, at most 8 blocks per CU.
//   budget per wave (V = 4): 8 rows x 64 lanes x 16 B = 8 KB of loads in flight, x 8 waves per SIMD
//     x 4 SIMDs = 256 KB per CU at most; VGPRs: 86 as compiled (32 row data + 4 accumulator + eight
//     64-bit addresses + the grid-stride state), 5 waves per SIMD -> 160 KB per CU in flight.
//     Traffic: m n 4 B read (m rows of non-zero weight) + n 4 B written.  Times: docs/PERFORMANCE.md.
#include "common.h"
#include "launchers.h"

// a_c * x and the add that follows, G_cj * a_j and its add, are each rounded on their own whatever
// flags build this file (plain operators under this pragma; see sparse_delta.hip)
#pragma clang fp contract(off)

namespace {

constexpr int GM_MAXW = 32;
constexpr int GM_ITERS = 32;

// lane j's value of v in every lane; j is uniform (a constant where the loop is unrolled)
__device__ __forceinline__ double gm_readlane(double v, int j) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), j);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), j);
  return __hiloint2double(hi, lo);
}

// sum over lanes 0 .. W - 1 of v in ascending order from +0.0: the same bits in every lane
__device__ __forceinline__ double gm_sum(double v, int W) {
  double s = 0.0;
#pragma unroll
  for (int j = 0; j < GM_MAXW; ++j)
    if (j < W) s = s + gm_readlane(v, j);
  return s;
}

__global__ __launch_bounds__(64) void geomed_weights_kernel(const double* __restrict__ G, double* __restrict__ a_out,
                                                            float* __restrict__ dist, int W) {
  const int c = threadIdx.x;
  const bool in = c < W;
  const double qnan = __longlong_as_double(0x7ff8000000000000LL);
  const double gcc = in ? G[c * W + c] : qnan;
  const bool valid = fabs(gcc) < (double)INFINITY;  // NaN compares false
  const unsigned long long vmask = __ballot(valid);
  const int nv = __popcll(vmask);
  double row[GM_MAXW];
#pragma unroll
  for (int j = 0; j < GM_MAXW; ++j) row[j] = (in && j < W && ((vmask >> j) & 1ull)) ? G[c * W + j] : 0.0;

  // the lower median of the valid diagonal: the valid lane whose (value, index) rank is (nv - 1) / 2
  int rank = 0;
#pragma unroll
  for (int j = 0; j < GM_MAXW; ++j) {
    if (j < W) {
      const double gj = gm_readlane(gcc, j);
      rank += (((vmask >> j) & 1ull) && (gj < gcc || (gj == gcc && j < c))) ? 1 : 0;
    }
  }
  const unsigned long long hit = __ballot(valid && rank == (nv - 1) / 2);
  const double med = gm_readlane(gcc, hit ? __ffsll((long long)hit) - 1 : 0);
  const double nu2 = 1e-12 * med + 1e-300;

  double a = valid ? 1.0 / (double)nv : 0.0, d2 = 0.0;
#pragma unroll 1
  for (int it = 0; it < GM_ITERS; ++it) {
    double g = 0.0;
#pragma unroll
    for (int j = 0; j < GM_MAXW; ++j)
      if (j < W) g = g + row[j] * gm_readlane(a, j);
    const double q = gm_sum(valid ? a * g : 0.0, W);
    const double t = (gcc - 2.0 * g) + q;
    d2 = t < 0.0 ? 0.0 : t;  // a NaN stays one, as torch's clamp_min keeps it
    const double w = valid ? 1.0 / sqrt(d2 + nu2) : 0.0;
    a = w / gm_sum(w, W);
  }
  if (in) {
    a_out[c] = nv ? a : qnan;
    dist[c] = valid ? (float)sqrt(d2) : INFINITY;
  }
}

template <int V>
struct GmVec;
template <>
struct GmVec<1> {
  typedef float T;
};
template <>
struct GmVec<4> {
  typedef f32x4 T;
};

// n % V == 0 and 16-byte aligned rows and out when V == 4 (the launcher's choice)
template <int V>
__global__ __launch_bounds__(256) void geomed_combine_kernel(const float* __restrict__ stack,
                                                             const double* __restrict__ a, float* __restrict__ out,
                                                             int W, long n) {
  typedef typename GmVec<V>::T VT;
  __shared__ int idx[GM_MAXW];
  __shared__ float wt[GM_MAXW];
  __shared__ int s_m;
  if (threadIdx.x == 0) {
    int cnt = 0;
    for (int c = 0; c < W; ++c) {
      const float a32 = (float)a[c];
      if (a32 != 0.f) {  // true for a NaN weight: its row is read and out is NaN everywhere
        idx[cnt] = c;
        wt[cnt++] = a32;
      }
    }
    s_m = cnt;
  }
  __syncthreads();
  const int m = s_m;
  const long nv = n / V;
  for (long g = blockIdx.x * (long)blockDim.x + threadIdx.x; g < nv; g += (long)gridDim.x * blockDim.x) {
    VT acc = VT(0.f);  // what an all-zero weight vector leaves
    for (int j0 = 0; j0 < m; j0 += 8) {  // m is block-uniform: eight row loads issued, then added in order
      VT v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        v[u] = VT(0.f);
        if (j0 + u < m) v[u] = *reinterpret_cast<const VT*>(stack + (size_t)idx[j0 + u] * (size_t)n + (size_t)g * V);
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        if (j0 + u < m) {
          const VT p = v[u] * wt[j0 + u];
          acc = (j0 + u == 0) ? p : acc + p;
        }
      }
    }
    *reinterpret_cast<VT*>(out + (size_t)g * V) = acc;
  }
}

bool gm_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

// G [W, W] fp64 -> a [W] fp64 (the Weiszfeld weights, summing to 1), dist [W] fp32 (each client's
// distance to the aggregate).  1: outside 1 <= W <= 32
extern "C" int fr_geomed_weights(const double* G, double* a, float* dist, int W, hipStream_t s) {
  if (W < 1 || W > GM_MAXW) return 1;
  hipLaunchKernelGGL(geomed_weights_kernel, dim3(1), dim3(64), 0, s, G, a, dist, W);
  return 0;
}

// stack [W, n] fp32 contiguous, a [W] fp64 on the device -> out [n] = sum_c fp32(a_c) x_c over the rows
// of non-zero weight in client order
extern "C" int fr_geomed_combine(const float* stack, const double* a, float* out, int W, long n, hipStream_t s) {
  if (W < 1 || W > GM_MAXW || n < 1) return 1;
  const bool vec = n % 4 == 0 && gm_aligned(stack) && gm_aligned(out);
  const long nv = vec ? n / 4 : n, need = (nv + 255) / 256, cap = (long)fr_num_cus() * 8;
  const dim3 g((unsigned)(need < cap ? need : cap)), b(256);
  if (vec) hipLaunchKernelGGL((geomed_combine_kernel<4>), g, b, 0, s, stack, a, out, W, n);
  else hipLaunchKernelGGL((geomed_combine_kernel<1>), g, b, 0, s, stack, a, out, W, n);
  return 0;
}
