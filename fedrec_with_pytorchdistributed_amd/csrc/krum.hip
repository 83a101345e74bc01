// Multi-Krum aggregation (Blanchard et al. 2017) of W <= 32 client vectors: the pairwise squared
// distances come from the Gram matrix of the CENTRED rows, G = Y Y^T with y_c = x_c - center, taken in
// one streaming pass on the fp32 matrix cores; a one-wave select scores and picks the clients; a
// third kernel averages the picked rows.  Three launches, no host synchronisation between them.
//
// The contract (ops/reference.py krum_gram / krum_select / krum_mean are the same forms in torch):
//   * centered_gram: y_ck = x_ck - center_k, one fp32 subtraction in registers (no centred copy of
//     the stack exists); G_ij = sum_k y_ik y_jk, fp32 products and sums inside a chunk of KR_L = 1024
//     coordinates, fp64 across the chunks.  G is symmetric bit for bit.
//   * select: d_cj = max((G_cc + G_jj) - 2 G_cj, 0) in fp64, rounded to fp32, +inf where the fp64
//     value is not finite; score_c = the W - f - 2 smallest d_cj (j != c) added in ascending order in
//     fp32; the m clients with the lowest (score, client index) get selected = 1.
//   * selected_mean: out = (x[s_0] + x[s_1] + ...) / float(m), s the selected clients in CLIENT order,
//     fp32 adds left to right from the first selected row, one IEEE division.
//
// krum_gram_kernel<T, VEC> -- register-direct, no LDS.  v_mfma_f32_16x16x4_f32 takes A[i][k] from lane
// (i = lane % 16, k = lane / 16) and B[k][j] from lane (j = lane % 16, k = lane / 16): for a Gram both
// are the SAME register.  Lane (r, q) loads 16 contiguous bytes of its own row r at coordinates
// k0 + 4 q .. + 3 and again at k0 + 16 + 4 q .. + 3, and issues one MFMA per loaded element; which four
// coordinates meet in one MFMA does not matter to a Gram sum as long as both operands agree, and
// they are one register.  17 <= W <= 32 (T = 3): a second register holds rows 16 .. 31 at the same
// coordinates; tiles (0,0), (0,1), (1,1) are accumulated (12 VGPRs), the lower-left tile follows by
// symmetry.  Rows >= W are zeros, never loads; coordinates >= n are zeros for x and center alike.
//   line use: one load instruction covers, per row, 4 lanes x 16 B = 64 contiguous bytes; the two
//     loads of a step cover the row's whole 128-byte line [k0, k0 + 32) and are issued back to back,
//     so a line leaves HBM once and every byte of it is used (rows are 128-byte aligned in steps
//     when the row start is; otherwise a step straddles two lines that the neighbouring steps of the
//     same wave finish).  VEC = false (row starts not 16-byte aligned, or n % 4 != 0): the same
//     coordinates by 4-byte loads, bitwise the same G.
//   center: 16 lanes share an address (one broadcast request); read once per chunk, by the one
//     wave that owns the chunk, and it serves both row registers.
//   order: chunk p covers [p L, (p + 1) L) whatever the grid; its wave walks steps s = 0 .. L / 32 - 1,
//     per step the low 16 coordinates' four elements, then the high 16's: L / 4 = 256 MFMAs chained
//     on each accumulator.  The chunk's accumulators go to part[p] as they lie in the registers
//     (16-byte stores, lanes without a valid element store nothing).  krum_finish_kernel then adds a
//     G element's P partials in fp64 in one fixed order that depends on P alone: slot t of 64 adds
//     p = t, t + 64, ... ascending, the 64 slots are added in slot order (64 slots x 16 elements per
//     block: with 16 slots the chain of dependent loads took 1 ms at P = 65,946); only i <= j is summed and
//     mirrored.  G is bitwise independent of grid and block count.  No float atomics.
//   containment: element (i, j) of an MFMA takes products of rows i and j only, so a NaN or inf in
//     row c reaches G[c][*] and G[*][c] alone.
//   budget per chunk at W = 32 (VEC): 32 rows x 4 KB + 4 KB center read, 3 KB partial written (2.3 %
//     of the read; again read by the finish: 4.7 % extra traffic in all); 8 KB of row loads in flight
//     per wave (two steps), x 7 waves per SIMD = 224 KB per CU; VGPRs: 72 = 12
//     accumulators + 2 x (16 row + 8 center) in flight + addresses; MFMA: 24 per step x 32 cycles = 768 cycles per 4 KB per SIMD, 16 KB
//     per 768 cycles per CU -> 13 TB/s at 256 CUs and 2.4 GHz, above what HBM delivers: the kernel is
//     bound by its loads, the MFMA pipe is 40-60 % busy.  W <= 16: 8 MFMAs per step whatever W, so
//     W = 4 (512 B per step) has a matrix-pipe ceiling of 4.9 TB/s, about HBM's.
//
// krum_select_kernel: one wave, lane c owns client c; distances through LDS; the W - f - 2 smallest are
// taken by repeated (value, index) minimum -- ascending order without a sort network; ranks by a loop.
// krum_mean_kernel<V>: the selected rows' indices compacted into LDS, one lane owns V consecutive
// coordinates (V = 4 with 16-byte loads where rows are 16-byte aligned), eight row loads in flight.
#include "common.h"
#include "launchers.h"

namespace {

constexpr int KR_MAXW = 32;
constexpr int KR_L = 1024;   // coordinates per chunk
constexpr int KR_STEP = 32;  // coordinates per step: one 128-byte line of every row
constexpr int KR_SLOTS = 64; // partial sums per G element in the finish

// four consecutive floats from p[k ..], zeros at and past n (VEC: k % 4 == 0 and n % 4 == 0)
template <bool VEC>
__device__ __forceinline__ f32x4 kr_load(const float* __restrict__ p, long k, long n) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if constexpr (VEC) {
    if (k < n) v = *reinterpret_cast<const f32x4*>(p + k);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (k + e < n) v[e] = p[k + e];
  }
  return v;
}

template <int T, bool VEC>
__global__ __launch_bounds__(256) void krum_gram_kernel(const float* __restrict__ stack,
                                                        const float* __restrict__ center,
                                                        float* __restrict__ part, int W, long n, long P) {
  const int lane = threadIdx.x & 63, fr = lane & 15, fq = lane >> 4;
  const long wave = (long)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (long)gridDim.x * 4;
  const bool ok0 = fr < W, ok1 = T == 3 && 16 + fr < W;
  const float* __restrict__ r0 = stack + (size_t)(ok0 ? fr : 0) * (size_t)n;
  const float* __restrict__ r1 = stack + (size_t)(ok1 ? 16 + fr : 0) * (size_t)n;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  for (long p = wave; p < P; p += nwaves) {
    f32x4 a00 = zero, a01 = zero, a11 = zero;
    const long c0 = p * KR_L, left = n - c0;
    const int steps = left >= KR_L ? KR_L / KR_STEP : (int)((left + KR_STEP - 1) / KR_STEP);
    // UN steps' loads issued before the first MFMA (UN divides L / 32: a step at or past `steps` lies
    // inside the chunk and past n, all zeros; four steps at W <= 16 measured no faster)
    constexpr int UN = 2;
    for (int s = 0; s < steps; s += UN) {
      f32x4 y0l[UN], y0h[UN], y1l[UN], y1h[UN];
#pragma unroll
      for (int u = 0; u < UN; ++u) {
        const long k = c0 + (long)(s + u) * KR_STEP + 4 * fq;
        const f32x4 cl = kr_load<VEC>(center, k, n), ch = kr_load<VEC>(center, k + 16, n);
        y0l[u] = y0h[u] = y1l[u] = y1h[u] = zero;
        if (ok0) {
          y0l[u] = kr_load<VEC>(r0, k, n) - cl;
          y0h[u] = kr_load<VEC>(r0, k + 16, n) - ch;
        }
        if constexpr (T == 3) {
          if (ok1) {
            y1l[u] = kr_load<VEC>(r1, k, n) - cl;
            y1h[u] = kr_load<VEC>(r1, k + 16, n) - ch;
          }
        }
      }
#pragma unroll
      for (int u = 0; u < UN; ++u) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          a00 = __builtin_amdgcn_mfma_f32_16x16x4f32(y0l[u][e], y0l[u][e], a00, 0, 0, 0);
          if constexpr (T == 3) {
            a01 = __builtin_amdgcn_mfma_f32_16x16x4f32(y0l[u][e], y1l[u][e], a01, 0, 0, 0);
            a11 = __builtin_amdgcn_mfma_f32_16x16x4f32(y1l[u][e], y1l[u][e], a11, 0, 0, 0);
          }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          a00 = __builtin_amdgcn_mfma_f32_16x16x4f32(y0h[u][e], y0h[u][e], a00, 0, 0, 0);
          if constexpr (T == 3) {
            a01 = __builtin_amdgcn_mfma_f32_16x16x4f32(y0h[u][e], y1h[u][e], a01, 0, 0, 0);
            a11 = __builtin_amdgcn_mfma_f32_16x16x4f32(y1h[u][e], y1h[u][e], a11, 0, 0, 0);
          }
        }
      }
    }
    // accumulator element r of a tile is (row 4 fq + r, column fr) of it
    float* dst = part + ((size_t)p * T) * 256 + lane * 4;
    if (ok0 && 4 * fq < W) *reinterpret_cast<f32x4*>(dst) = a00;
    if constexpr (T == 3) {
      if (ok1) *reinterpret_cast<f32x4*>(dst + 256) = a01;
      if (ok1 && 16 + 4 * fq < W) *reinterpret_cast<f32x4*>(dst + 512) = a11;
    }
  }
}

// block b: the 16 consecutive register-image elements [16 b, 16 b + 16) of the T tiles x 64 slots
__global__ __launch_bounds__(1024) void krum_finish_kernel(const float* __restrict__ part, double* __restrict__ G,
                                                          int W, long P, int T) {
  __shared__ double red[KR_SLOTS][17];
  const int e16 = threadIdx.x & 15, slot = threadIdx.x >> 4;
  const int raw = blockIdx.x * 16 + e16, t = raw >> 8, ln = (raw & 255) >> 2, r = raw & 3;
  const int gi = (t == 2 ? 16 : 0) + 4 * (ln >> 4) + r, gj = (t >= 1 ? 16 : 0) + (ln & 15);
  const bool valid = gi < W && gj < W && gi <= gj;
  double s = 0.0;
  if (valid) {
    const size_t stride = (size_t)T * 256;
#pragma unroll 8
    for (long p = slot; p < P; p += KR_SLOTS) s += (double)part[(size_t)p * stride + raw];
  }
  red[slot][e16] = s;
  __syncthreads();
  if (slot == 0 && valid) {
    double tot = red[0][e16];
    for (int k = 1; k < KR_SLOTS; ++k) tot += red[k][e16];
    G[gi * W + gj] = tot;
    G[gj * W + gi] = tot;
  }
}

__global__ __launch_bounds__(64) void krum_select_kernel(const double* __restrict__ G, int* __restrict__ selected,
                                                         float* __restrict__ scores, int W, int f, int m) {
  __shared__ float d[KR_MAXW][KR_MAXW + 1];
  __shared__ float sc[KR_MAXW];
  const int c = threadIdx.x;
  float score = 0.f;
  if (c < W) {
    const double gcc = G[c * W + c];
    for (int j = 0; j < W; ++j) {
      const double t = (gcc + G[j * W + j]) - 2.0 * G[c * W + j];
      d[c][j] = fabs(t) < (double)INFINITY ? (float)fmax(t, 0.0) : INFINITY;  // NaN compares false
    }
    unsigned taken = 1u << c;
    for (int it = 0; it < W - f - 2; ++it) {  // ascending: the (value, index) minimum of what is left
      float best = 0.f;
      int bj = -1;
      for (int j = 0; j < W; ++j) {
        const float v = d[c][j];
        if (!((taken >> j) & 1u) && (bj < 0 || v < best)) {
          best = v;
          bj = j;
        }
      }
      taken |= 1u << bj;
      score += best;
    }
    sc[c] = score;
    scores[c] = score;
  }
  __syncthreads();
  if (c < W) {
    int rank = 0;
    for (int j = 0; j < W; ++j) {
      const float sj = sc[j];
      rank += (sj < score || (sj == score && j < c)) ? 1 : 0;
    }
    selected[c] = rank < m ? 1 : 0;
  }
}

template <int V>
struct KrVec;
template <>
struct KrVec<1> {
  typedef float T;
};
template <>
struct KrVec<4> {
  typedef f32x4 T;
};

// n % V == 0 and 16-byte aligned rows and out when V == 4 (the launcher's choice)
template <int V>
__global__ __launch_bounds__(256) void krum_mean_kernel(const float* __restrict__ stack,
                                                        const int* __restrict__ selected, float* __restrict__ out,
                                                        int W, long n) {
  typedef typename KrVec<V>::T VT;
  __shared__ int idx[KR_MAXW];
  __shared__ int s_m;
  if (threadIdx.x == 0) {
    int cnt = 0;
    for (int c = 0; c < W; ++c)
      if (selected[c] != 0) idx[cnt++] = c;
    s_m = cnt;
  }
  __syncthreads();
  const int m = s_m;
  const float denom = (float)m;
  const long nv = n / V;
  for (long g = blockIdx.x * (long)blockDim.x + threadIdx.x; g < nv; g += (long)gridDim.x * blockDim.x) {
    VT acc = VT(0.f);
    for (int j0 = 0; j0 < m; j0 += 8) {  // m is block-uniform: eight row loads issued, then added in order
      VT v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        v[u] = VT(0.f);
        if (j0 + u < m) v[u] = *reinterpret_cast<const VT*>(stack + (size_t)idx[j0 + u] * (size_t)n + (size_t)g * V);
      }
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (j0 + u < m) acc = (j0 + u == 0) ? v[u] : acc + v[u];
    }
    *reinterpret_cast<VT*>(out + (size_t)g * V) = acc / denom;
  }
}

bool kr_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

// floats of scratch fr_krum_gram needs for [W, n]: one register image of the tiles per chunk
extern "C" long fr_krum_gram_ws(int W, long n) {
  if (W < 1 || W > KR_MAXW || n < 1) return -1;
  return ((n + KR_L - 1) / KR_L) * (W <= 16 ? 1 : 3) * 256;
}

// stack [W, n] fp32 contiguous, center [n] -> G [W, W] fp64 (every element written).  max_blocks > 0
// caps the grid (G does not depend on it).  1: a shape outside 1 <= W <= 32, n >= 1
extern "C" int fr_krum_gram(const float* stack, const float* center, float* part, double* G, int W, long n,
                            int max_blocks, hipStream_t s) {
  if (W < 1 || W > KR_MAXW || n < 1) return 1;
  const long P = (n + KR_L - 1) / KR_L;
  long grid = (P + 3) / 4;
  const long cap = max_blocks > 0 ? max_blocks : (long)fr_num_cus() * 8;
  grid = grid < cap ? grid : cap;
  const bool vec = n % 4 == 0 && kr_aligned(stack) && kr_aligned(center);
  const int T = W <= 16 ? 1 : 3;
  const dim3 g((unsigned)grid), b(256);
  if (T == 1 && vec) hipLaunchKernelGGL((krum_gram_kernel<1, true>), g, b, 0, s, stack, center, part, W, n, P);
  else if (T == 1) hipLaunchKernelGGL((krum_gram_kernel<1, false>), g, b, 0, s, stack, center, part, W, n, P);
  else if (vec) hipLaunchKernelGGL((krum_gram_kernel<3, true>), g, b, 0, s, stack, center, part, W, n, P);
  else hipLaunchKernelGGL((krum_gram_kernel<3, false>), g, b, 0, s, stack, center, part, W, n, P);
  hipLaunchKernelGGL(krum_finish_kernel, dim3(16 * T), dim3(16 * KR_SLOTS), 0, s, part, G, W, P, T);
  return 0;
}

// G [W, W] fp64 -> selected [W] int32 (0 / 1), scores [W] fp32.  1: outside 1 <= W <= 32, f >= 0,
// W >= 2 f + 3, 1 <= m <= W - f
extern "C" int fr_krum_select(const double* G, int* selected, float* scores, int W, int f, int m, hipStream_t s) {
  if (W < 1 || W > KR_MAXW || f < 0 || W < 2 * f + 3 || m < 1 || m > W - f) return 1;
  hipLaunchKernelGGL(krum_select_kernel, dim3(1), dim3(64), 0, s, G, selected, scores, W, f, m);
  return 0;
}

// stack [W, n] fp32 contiguous, selected [W] int32 on the device -> out [n]: the client-order mean of
// the rows with selected != 0 (NaN when there is none)
extern "C" int fr_krum_selected_mean(const float* stack, const int* selected, float* out, int W, long n,
                                     hipStream_t s) {
  if (W < 1 || W > KR_MAXW || n < 1) return 1;
  const bool vec = n % 4 == 0 && kr_aligned(stack) && kr_aligned(out);
  const long nv = vec ? n / 4 : n, need = (nv + 255) / 256, cap = (long)fr_num_cus() * 8;
  const dim3 g((unsigned)(need < cap ? need : cap)), b(256);
  if (vec) hipLaunchKernelGGL((krum_mean_kernel<4>), g, b, 0, s, stack, selected, out, W, n);
  else hipLaunchKernelGGL((krum_mean_kernel<1>), g, b, 0, s, stack, selected, out, W, n);
  return 0;
}
