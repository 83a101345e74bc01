// Low-rank (PowerSGD: Vogels, Karimireddy, Jaggi 2019) uploads with error feedback: every matrix of the flat
// buffer sends a rank-R factorisation P^ Q'^T of its round delta (R in {1, 2, 4, 8}), every other coordinate
// ("rest": biases, vectors, alignment padding) travels dense; what was not sent stays in the residual.
//
// The plan (ops/reference.py LowRankPlan, a pure function of the layout and R) is a set of int32 tables:
//   mats  [M, 4]  flat offset, rows, cols, offset `fac` of the matrix' factors in the payload: P^ [rows, R] at
//                 fac, Q' [cols, R] at fac + rows R (both row-major); the factors fill [0, F) of the payload
//   rest  [S, 3]  flat start, length, payload offset (>= F) of a dense segment
//   and one tile table per kernel, so that ONE launch covers every matrix (no per-matrix launch loop).
// The basis (the Q of this round) has the payload's factor layout: last round's payload[:F] is the next basis.
//
// One round on a client, a = (local - theta_g) + residual (one fp32 subtraction, one fp32 addition, formed in
// registers by every kernel that needs it, never written):
//   project      P = a Q        fp32 MFMA 16x16x4, tolerance contract (summation order below)
//   orth         P^ = orth(P)   modified Gram-Schmidt, each column projected twice, fp64 dots and norms
//   backproject  Q' = a^T P^    fp32 MFMA 16x16x4, tolerance contract
//   residual     d_ij = sum over t < R ascending of P^_it Q'_jt, every product and sum rounded on its own;
//                residual = a - d; rest: payload = a, residual = +0.0        bitwise contract
//   combine      out = base + (sum over c in client order of w_c d_c) / sum(w)  bitwise contract, rounded as
//                dequant_combine rounds (acc from +0.0, three roundings per client, one division)
// Every result is bitwise independent of the grid: a tile's arithmetic is a function of the matrix shape alone.
//
// lr_project_kernel -- a block (4 waves) owns 16 rows of one matrix.  v_mfma_f32_16x16x4_f32 takes A[i][k] from
//   lane (i = lane % 16, k = lane / 16) and B[k][j] from lane (j = lane % 16, k = lane / 16).  Lane (i, g) loads 16
//   bytes of row i of local, theta_g and residual at columns k .. k + 3, k = k0 + 64 wave + 16 u + 4 g, forms a in
//   registers and feeds four MFMAs, element e of the load as the k-index g of MFMA e; the B side takes
//   Q[k + e][j] under the same permutation from LDS (lanes j >= R supply zeros: the kernel is bound by its
//   loads, the idle MFMA columns cost nothing).  K walks in slabs of 256 columns: Q's slab (256 x R floats, at
//   most 8 KB) is staged in LDS, wave w owns columns [64 w, 64 w + 64) of it, four 16-k groups (12 loads of 16
//   bytes) in flight per lane.  The four waves' accumulators are added through LDS in wave order.  Rows >= rows
//   and columns >= cols are zeros, never loads; cols % 4 != 0 loads element by element, bitwise the same.
// lr_backproject_kernel -- the A operand is a^T: lane (i, g) supplies a[row g][column i], so the 16 lanes of a
//   group read 16 consecutive floats of a row; a wave owns four column tiles (64 columns: a quarter-wave reads
//   256 contiguous bytes of a row).  A block owns 64 columns and a chunk of 256 rows (a function of the shape
//   alone): slabs of 64 rows, P^'s slab staged in LDS for the B operand, wave w owns rows [16 w, 16 w + 16) of
//   the slab, 16 x 3 loads in flight per lane.  The waves are added through LDS in wave order, the chunk's
//   partial goes to a workspace and lr_backproject_finish_kernel adds a column group's chunks in ascending order.
// lr_orth_kernel -- one workgroup of 1024 per matrix, P in global memory (rows reaches 30,522: no LDS residency);
//   thread t owns rows t, t + 1024, ...: no other thread touches them, so no fence is needed between the steps.
//   Block sums are fp64: a thread's rows in ascending order, a xor tree over the wave, the 16 waves in order.
//   A column whose squared norm after projection is 0 or <= 2^-40 times the one before becomes zeros.
// lr_residual_kernel / lr_combine_kernel<R> -- tiles of 32 rows x 256 columns (a thread: 8 rows x 4 consecutive
//   columns, 16-byte loads and stores), the tile's P^ rows and Q' rows staged in LDS (per client in turn in the
//   combine); rest tiles are 1024 elements of a segment.
// Every tile checks its table rows against n, F and L before it touches memory: a table that does not fit the
// tensors makes a tile do nothing, whatever the payload holds.
#include "common.h"
#include "launchers.h"

// every product, sum and difference below is rounded on its own, whatever flags build this file (plain
// operators under this pragma: the __f*_rn helpers were fused after inlining)
#pragma clang fp contract(off)

namespace {

constexpr int LR_MAXR = 8;
constexpr int LR_BLOCK = 256;
constexpr int LR_PK = 256;     // project: columns per K slab, 64 per wave
constexpr int LR_BCOLS = 64;   // backproject: columns per block
constexpr int LR_BCHUNK = 256; // backproject: rows per block (one partial)
constexpr int LR_BSLAB = 64;   // backproject: rows per LDS slab, 16 per wave
constexpr int LR_TR = 32;      // elementwise tile: rows
constexpr int LR_TC = 256;     // elementwise tile: columns
constexpr int LR_REST = 1024;  // elementwise tile: elements of a rest segment
constexpr int LR_ORTH = 1024;  // threads of the orth workgroup

struct LrMat {
  int off, rows, cols, fac;
  bool ok;
};

// row m of mats, checked against the flat length n and the factor length F
__device__ __forceinline__ LrMat lr_mat(const int* __restrict__ mats, int m, int M, int R, long n, long F) {
  LrMat t = {0, 0, 0, 0, false};
  if (m < 0 || m >= M) return t;
  t.off = mats[4 * m], t.rows = mats[4 * m + 1], t.cols = mats[4 * m + 2], t.fac = mats[4 * m + 3];
  t.ok = t.off >= 0 && t.rows >= 1 && t.cols >= 1 && t.fac >= 0 && (long)t.off + (long)t.rows * t.cols <= n &&
         (long)t.fac + ((long)t.rows + t.cols) * R <= F;
  return t;
}

// a at four consecutive coordinates from p = row start + column k; zeros at and past `cols` and where !ok
// (VEC: p % 4 == 0, k % 4 == 0 and cols % 4 == 0 on 16-byte aligned tensors)
template <bool VEC>
__device__ __forceinline__ f32x4 lr_a4(const float* __restrict__ l, const float* __restrict__ g,
                                       const float* __restrict__ r, long p, int k, int cols, bool ok) {
  f32x4 a = {0.f, 0.f, 0.f, 0.f};
  if (!ok) return a;
  if constexpr (VEC) {
    if (k < cols) {
      const f32x4 lv = *reinterpret_cast<const f32x4*>(l + p), gv = *reinterpret_cast<const f32x4*>(g + p),
                  rv = *reinterpret_cast<const f32x4*>(r + p);
      a = (lv - gv) + rv;
    }
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (k + e < cols) a[e] = (l[p + e] - g[p + e]) + r[p + e];
  }
  return a;
}

template <bool VEC>
__device__ __forceinline__ void lr_put4(float* __restrict__ o, long p, int k, int cols, const f32x4& v) {
  if constexpr (VEC) {
    if (k < cols) *reinterpret_cast<f32x4*>(o + p) = v;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (k + e < cols) o[p + e] = v[e];
  }
}

// ---- project ---------------------------------------------------------------------------------
template <bool VEC>
__device__ __forceinline__ void lr_project_tile(const float* __restrict__ l, const float* __restrict__ g,
                                                const float* __restrict__ r, const float* __restrict__ Q,
                                                float* __restrict__ P, const LrMat& t, int row0, int R, float* qs,
                                                f32x4* red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, fr = lane & 15, fq = lane >> 4;
  const int i = row0 + fr;
  const bool ok = i < t.rows;
  const long rb = (long)t.off + (long)(ok ? i : 0) * t.cols;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < t.cols; k0 += LR_PK) {
    __syncthreads();  // the slab before this one has been read
    const int left = t.cols - k0, valid = (left < LR_PK ? left : LR_PK) * R;
    for (int x = threadIdx.x; x < LR_PK * R; x += LR_BLOCK) qs[x] = x < valid ? Q[(long)k0 * R + x] : 0.f;
    f32x4 a[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int k = k0 + 64 * wave + 16 * u + 4 * fq;
      a[u] = lr_a4<VEC>(l, g, r, rb + k, k, t.cols, ok);
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 4; ++u) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int kk = 64 * wave + 16 * u + 4 * fq + e;
        const float b = fr < R ? qs[kk * R + fr] : 0.f;
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][e], b, acc, 0, 0, 0);
      }
    }
  }
  red[wave * 64 + lane] = acc;
  __syncthreads();
  if (wave == 0) {  // accumulator element e of lane (fr, fq): row 4 fq + e, column fr
    f32x4 s = red[lane];
    s = s + red[64 + lane];
    s = s + red[128 + lane];
    s = s + red[192 + lane];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int row = row0 + 4 * fq + e;
      if (row < t.rows && fr < R) P[(long)row * R + fr] = s[e];
    }
  }
}

// tiles [ntiles, 2]: matrix, first row
__global__ __launch_bounds__(LR_BLOCK) void lr_project_kernel(const float* __restrict__ l, const float* __restrict__ g,
                                                              const float* __restrict__ r,
                                                              const float* __restrict__ basis,
                                                              float* __restrict__ payload, const int* __restrict__ mats,
                                                              const int* __restrict__ tiles, int ntiles, int M, int R,
                                                              long n, long F, int vec) {
  __shared__ float qs[LR_PK * LR_MAXR];
  __shared__ f32x4 red[LR_BLOCK];
  for (int ti = blockIdx.x; ti < ntiles; ti += gridDim.x) {  // (block-uniform: the barriers inside meet)
    const LrMat t = lr_mat(mats, tiles[2 * ti], M, R, n, F);
    const int row0 = tiles[2 * ti + 1];
    if (!t.ok || row0 < 0 || row0 >= t.rows) continue;
    const float* Q = basis + t.fac + (long)t.rows * R;
    float* P = payload + t.fac;
    if (vec && (t.cols & 3) == 0 && (t.off & 3) == 0) lr_project_tile<true>(l, g, r, Q, P, t, row0, R, qs, red);
    else lr_project_tile<false>(l, g, r, Q, P, t, row0, R, qs, red);
  }
}

// ---- orth ------------------------------------------------------------------------------------
// the block's sum of v, the same bits in every thread: xor tree in the wave, the 16 waves in order
__device__ __forceinline__ double lr_block_sum(double v, double* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();  // the sum before this one has been read
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  double tot = sh[0];
  for (int w = 1; w < LR_ORTH / 64; ++w) tot += sh[w];
  return tot;
}

__global__ __launch_bounds__(LR_ORTH) void lr_orth_kernel(float* __restrict__ payload, const int* __restrict__ mats,
                                                          int M, int R, long F) {
  __shared__ double sh[LR_ORTH / 64];
  const LrMat t = lr_mat(mats, blockIdx.x, M, R, (long)1 << 62, F);
  if (!t.ok) return;
  float* P = payload + t.fac;
  const int rows = t.rows, tid = threadIdx.x;
  for (int c = 0; c < R; ++c) {
    double s = 0.0;
    for (int i = tid; i < rows; i += LR_ORTH) {
      const double v = (double)P[(long)i * R + c];
      s += v * v;
    }
    const double n0 = lr_block_sum(s, sh);
    for (int pass = 0; pass < 2; ++pass) {
      for (int b = 0; b < c; ++b) {
        double d = 0.0;
        for (int i = tid; i < rows; i += LR_ORTH) d += (double)P[(long)i * R + b] * (double)P[(long)i * R + c];
        d = lr_block_sum(d, sh);
        for (int i = tid; i < rows; i += LR_ORTH)
          P[(long)i * R + c] = (float)((double)P[(long)i * R + c] - d * (double)P[(long)i * R + b]);
      }
    }
    s = 0.0;
    for (int i = tid; i < rows; i += LR_ORTH) {
      const double v = (double)P[(long)i * R + c];
      s += v * v;
    }
    const double n1 = lr_block_sum(s, sh);
    const bool zero = n1 == 0.0 || n1 <= 0x1p-40 * n0;  // (a NaN compares false: it stays in the column)
    const double nrm = sqrt(n1);
    for (int i = tid; i < rows; i += LR_ORTH)
      P[(long)i * R + c] = zero ? 0.f : (float)((double)P[(long)i * R + c] / nrm);
  }
}

// ---- backproject -----------------------------------------------------------------------------
// tiles [ntiles, 3]: matrix, first column (a multiple of 64), row chunk; part [ntiles, 64, R]
__global__ __launch_bounds__(LR_BLOCK) void lr_backproject_kernel(const float* __restrict__ l,
                                                                  const float* __restrict__ g,
                                                                  const float* __restrict__ r,
                                                                  const float* __restrict__ payload,
                                                                  float* __restrict__ part,
                                                                  const int* __restrict__ mats,
                                                                  const int* __restrict__ tiles, int ntiles, int M,
                                                                  int R, long n, long F) {
  __shared__ float ps[LR_BSLAB * LR_MAXR];
  __shared__ f32x4 red[4 * LR_BLOCK];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, fr = lane & 15, fq = lane >> 4;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  for (int ti = blockIdx.x; ti < ntiles; ti += gridDim.x) {
    const LrMat t = lr_mat(mats, tiles[3 * ti], M, R, n, F);
    const int col0 = tiles[3 * ti + 1], chunk = tiles[3 * ti + 2];
    if (!t.ok || col0 < 0 || col0 >= t.cols || chunk < 0 || (long)chunk * LR_BCHUNK >= t.rows) continue;
    const float* Ph = payload + t.fac;
    const int rbeg = chunk * LR_BCHUNK, rend = t.rows - rbeg < LR_BCHUNK ? t.rows : rbeg + LR_BCHUNK;
    f32x4 acc[4] = {zero, zero, zero, zero};
    for (int s0 = rbeg; s0 < rend; s0 += LR_BSLAB) {
      __syncthreads();
      const int left = rend - s0, valid = (left < LR_BSLAB ? left : LR_BSLAB) * R;
      for (int x = threadIdx.x; x < LR_BSLAB * R; x += LR_BLOCK) ps[x] = x < valid ? Ph[(long)s0 * R + x] : 0.f;
      float a[4][4];
#pragma unroll
      for (int st = 0; st < 4; ++st) {
        const int row = s0 + 16 * wave + 4 * st + fq;
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
          const int col = col0 + 16 * ct + fr;
          const long p = (long)t.off + (long)row * t.cols + col;
          a[st][ct] = row < rend && col < t.cols ? (l[p] - g[p]) + r[p] : 0.f;
        }
      }
      __syncthreads();
#pragma unroll
      for (int st = 0; st < 4; ++st) {
        const float b = fr < R ? ps[(16 * wave + 4 * st + fq) * R + fr] : 0.f;
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[st][ct], b, acc[ct], 0, 0, 0);
      }
    }
    __syncthreads();  // (red of the tile before this one has been read)
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) red[(wave * 4 + ct) * 64 + lane] = acc[ct];
    __syncthreads();
    if (wave == 0) {  // element e of lane (fr, fq) of tile ct: column col0 + 16 ct + 4 fq + e of a, factor fr
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        f32x4 s = red[ct * 64 + lane];
        s = s + red[(4 + ct) * 64 + lane];
        s = s + red[(8 + ct) * 64 + lane];
        s = s + red[(12 + ct) * 64 + lane];
        if (fr < R) {
#pragma unroll
          for (int e = 0; e < 4; ++e) part[((long)ti * LR_BCOLS + 16 * ct + 4 * fq + e) * R + fr] = s[e];
        }
      }
    }
  }
}

// tiles [ntiles, 4]: matrix, first column, the column group's first backproject tile, its chunks
__global__ __launch_bounds__(LR_BLOCK) void lr_backproject_finish_kernel(const float* __restrict__ part,
                                                                         float* __restrict__ payload,
                                                                         const int* __restrict__ mats,
                                                                         const int* __restrict__ tiles, int ntiles,
                                                                         int nparts, int M, int R, long F) {
  for (int ti = blockIdx.x; ti < ntiles; ti += gridDim.x) {
    const LrMat t = lr_mat(mats, tiles[4 * ti], M, R, (long)1 << 62, F);
    const int col0 = tiles[4 * ti + 1], first = tiles[4 * ti + 2], nch = tiles[4 * ti + 3];
    if (!t.ok || col0 < 0 || col0 >= t.cols || first < 0 || nch < 1 || (long)first + nch > nparts) continue;
    float* Qn = payload + t.fac + (long)t.rows * R;
    for (int x = threadIdx.x; x < LR_BCOLS * R; x += LR_BLOCK) {
      const int col = col0 + x / R;
      if (col >= t.cols) continue;
      float s = part[(long)first * LR_BCOLS * R + x];
      for (int c = 1; c < nch; ++c) s = s + part[((long)first + c) * LR_BCOLS * R + x];
      Qn[(long)col * R + x % R] = s;
    }
  }
}

// ---- residual and combine --------------------------------------------------------------------
// d of one coordinate: p_0 q_0, then + p_t q_t for t = 1 .. R - 1, every operation rounded
template <int R>
__device__ __forceinline__ float lr_decode(const float (&p)[R], const float (&q)[R]) {
  float d = p[0] * q[0];
#pragma unroll
  for (int t = 1; t < R; ++t) d = d + p[t] * q[t];
  return d;
}

struct LrRest {
  int start, len, pay;
  bool ok;
};

__device__ __forceinline__ LrRest lr_rest(const int* __restrict__ rest, int s, int S, int e0, long n, long F, long L) {
  LrRest t = {0, 0, 0, false};
  if (s < 0 || s >= S) return t;
  t.start = rest[3 * s], t.len = rest[3 * s + 1], t.pay = rest[3 * s + 2];
  t.ok = t.start >= 0 && t.len >= 1 && (long)t.start + t.len <= n && (long)t.pay >= F && (long)t.pay + t.len <= L &&
         e0 >= 0 && e0 < t.len;
  return t;
}

// the tile's P^ rows and Q' rows of the payload at `pay` -> LDS
template <int R>
__device__ __forceinline__ void lr_stage(const float* __restrict__ pay, const LrMat& t, int r0, int c0, float* ps,
                                         float* qs) {
  const int nr = (t.rows - r0 < LR_TR ? t.rows - r0 : LR_TR) * R, nc = (t.cols - c0 < LR_TC ? t.cols - c0 : LR_TC) * R;
  const float* P = pay + t.fac + (long)r0 * R;
  const float* Q = pay + t.fac + ((long)t.rows + c0) * R;
  for (int x = threadIdx.x; x < LR_TR * R; x += LR_BLOCK) ps[x] = x < nr ? P[x] : 0.f;
  for (int x = threadIdx.x; x < LR_TC * R; x += LR_BLOCK) qs[x] = x < nc ? Q[x] : 0.f;
}

template <int R, bool VEC>
__device__ __forceinline__ void lr_residual_tile(const float* __restrict__ l, const float* __restrict__ g,
                                                 float* __restrict__ res, const LrMat& t, int r0, int c0,
                                                 const float* ps, const float* qs) {
  const int cg = threadIdx.x & 63, rg = threadIdx.x >> 6, c = c0 + 4 * cg;
  if (c >= t.cols) return;
  float q[4][R];
#pragma unroll
  for (int e = 0; e < 4; ++e)
#pragma unroll
    for (int k = 0; k < R; ++k) q[e][k] = qs[(4 * cg + e) * R + k];
#pragma unroll
  for (int rr = 0; rr < LR_TR / 4; ++rr) {
    const int i = r0 + rg * (LR_TR / 4) + rr;
    if (i >= t.rows) break;
    const long p0 = (long)t.off + (long)i * t.cols + c;
    const f32x4 a = lr_a4<VEC>(l, g, res, p0, c, t.cols, true);
    float p[R];
#pragma unroll
    for (int k = 0; k < R; ++k) p[k] = ps[(rg * (LR_TR / 4) + rr) * R + k];
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = a[e] - lr_decode<R>(p, q[e]);
    lr_put4<VEC>(res, p0, c, t.cols, o);
  }
}

// tiles [ntiles, 3]: (matrix m >= 0, first row, first column) or (-1 - segment, first element, 0)
template <int R>
__global__ __launch_bounds__(LR_BLOCK) void lr_residual_kernel(const float* __restrict__ l, const float* __restrict__ g,
                                                               float* __restrict__ res, float* __restrict__ payload,
                                                               const int* __restrict__ mats,
                                                               const int* __restrict__ rest,
                                                               const int* __restrict__ tiles, int ntiles, int M, int S,
                                                               long n, long F, long L, int vec) {
  __shared__ float ps[LR_TR * R];
  __shared__ float qs[LR_TC * R];
  for (int ti = blockIdx.x; ti < ntiles; ti += gridDim.x) {
    const int id = tiles[3 * ti], r0 = tiles[3 * ti + 1], c0 = tiles[3 * ti + 2];
    if (id >= 0) {
      const LrMat t = lr_mat(mats, id, M, R, n, F);
      if (!t.ok || r0 < 0 || r0 >= t.rows || c0 < 0 || c0 >= t.cols) continue;
      __syncthreads();
      lr_stage<R>(payload, t, r0, c0, ps, qs);
      __syncthreads();
      if (vec && (t.cols & 3) == 0 && (t.off & 3) == 0) lr_residual_tile<R, true>(l, g, res, t, r0, c0, ps, qs);
      else lr_residual_tile<R, false>(l, g, res, t, r0, c0, ps, qs);
    } else {
      const LrRest t = lr_rest(rest, -1 - id, S, r0, n, F, L);
      if (!t.ok) continue;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int j = r0 + e * LR_BLOCK + (int)threadIdx.x;
        if (j < t.len) {
          const long p = (long)t.start + j;
          payload[(long)t.pay + j] = (l[p] - g[p]) + res[p];
          res[p] = 0.f;
        }
      }
    }
  }
}

template <int R, bool VEC>
__device__ __forceinline__ void lr_combine_tile(const float* __restrict__ base, const float* __restrict__ stack,
                                                const float* __restrict__ wts, float* __restrict__ out, int W, long L,
                                                const LrMat& t, int r0, int c0, float* ps, float* qs) {
  const int cg = threadIdx.x & 63, rg = threadIdx.x >> 6, c = c0 + 4 * cg;
  const bool live = c < t.cols;
  float acc[LR_TR / 4][4];
#pragma unroll
  for (int rr = 0; rr < LR_TR / 4; ++rr)
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[rr][e] = 0.f;
  float ws = 0.f;
  for (int cl = 0; cl < W; ++cl) {
    __syncthreads();
    lr_stage<R>(stack + (long)cl * L, t, r0, c0, ps, qs);
    __syncthreads();
    const float w = wts[cl];
    ws = ws + w;
    if (!live) continue;
    float q[4][R];
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int k = 0; k < R; ++k) q[e][k] = qs[(4 * cg + e) * R + k];
#pragma unroll
    for (int rr = 0; rr < LR_TR / 4; ++rr) {
      float p[R];
#pragma unroll
      for (int k = 0; k < R; ++k) p[k] = ps[(rg * (LR_TR / 4) + rr) * R + k];
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[rr][e] = acc[rr][e] + w * lr_decode<R>(p, q[e]);
    }
  }
  if (!live) return;
#pragma unroll
  for (int rr = 0; rr < LR_TR / 4; ++rr) {
    const int i = r0 + rg * (LR_TR / 4) + rr;
    if (i < t.rows) {
      const long p0 = (long)t.off + (long)i * t.cols + c;
      f32x4 o = {0.f, 0.f, 0.f, 0.f};
      if constexpr (VEC) {
        o = *reinterpret_cast<const f32x4*>(base + p0);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (c + e < t.cols) o[e] = base[p0 + e];
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = o[e] + acc[rr][e] / ws;
      lr_put4<VEC>(out, p0, c, t.cols, o);
    }
  }
}

// stack [W, L]: the clients' payloads
template <int R>
__global__ __launch_bounds__(LR_BLOCK) void lr_combine_kernel(const float* __restrict__ base,
                                                              const float* __restrict__ stack,
                                                              const float* __restrict__ wts, float* __restrict__ out,
                                                              const int* __restrict__ mats,
                                                              const int* __restrict__ rest,
                                                              const int* __restrict__ tiles, int ntiles, int M, int S,
                                                              int W, long n, long F, long L, int vec) {
  __shared__ float ps[LR_TR * R];
  __shared__ float qs[LR_TC * R];
  for (int ti = blockIdx.x; ti < ntiles; ti += gridDim.x) {
    const int id = tiles[3 * ti], r0 = tiles[3 * ti + 1], c0 = tiles[3 * ti + 2];
    if (id >= 0) {
      const LrMat t = lr_mat(mats, id, M, R, n, F);
      if (!t.ok || r0 < 0 || r0 >= t.rows || c0 < 0 || c0 >= t.cols) continue;
      if (vec && (t.cols & 3) == 0 && (t.off & 3) == 0)
        lr_combine_tile<R, true>(base, stack, wts, out, W, L, t, r0, c0, ps, qs);
      else lr_combine_tile<R, false>(base, stack, wts, out, W, L, t, r0, c0, ps, qs);
    } else {
      const LrRest t = lr_rest(rest, -1 - id, S, r0, n, F, L);
      if (!t.ok) continue;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int j = r0 + e * LR_BLOCK + (int)threadIdx.x;
        if (j < t.len) {
          float acc = 0.f, ws = 0.f;
          for (int cl = 0; cl < W; ++cl) {
            const float w = wts[cl];
            acc = acc + w * stack[(long)cl * L + t.pay + j];
            ws = ws + w;
          }
          out[(long)t.start + j] = base[(long)t.start + j] + acc / ws;
        }
      }
    }
  }
}

inline bool lr_al16(const void* p) { return ((uintptr_t)p & 15u) == 0; }
inline bool lr_rank(int R) { return R == 1 || R == 2 || R == 4 || R == 8; }

inline unsigned lr_grid(long tiles, int max_blocks) {
  const long cap = max_blocks > 0 ? max_blocks : (long)fr_num_cus() * 8;
  return (unsigned)(tiles < cap ? tiles : cap);
}

}  // namespace

// Every launcher: 1 a shape outside 1 <= n < 2^31, F <= L < 2^31, R in {1, 2, 4, 8}, M >= 1, a table without
// rows; 3 a runtime error.  max_blocks > 0 caps the grid (no result depends on it).

// payload[fac ..] = P = a Q of every matrix; basis [F] holds Q at the place of Q'; tiles [ntiles, 2]
extern "C" int fr_lowrank_project(const float* local, const float* global, const float* residual, const float* basis,
                                  float* payload, const int* mats, const int* tiles, int ntiles, int M, int R, long n,
                                  long F, int max_blocks, hipStream_t s) {
  if (n < 1 || n >= (1L << 31) || F < 1 || F >= (1L << 31) || !lr_rank(R) || M < 1 || ntiles < 1) return 1;
  const int vec = lr_al16(local) && lr_al16(global) && lr_al16(residual);
  hipLaunchKernelGGL(lr_project_kernel, dim3(lr_grid(ntiles, max_blocks)), dim3(LR_BLOCK), 0, s, local, global,
                     residual, basis, payload, mats, tiles, ntiles, M, R, n, F, vec);
  return hipGetLastError() == hipSuccess ? 0 : 3;
}

// P -> P^ in place, one workgroup per matrix
extern "C" int fr_lowrank_orth(float* payload, const int* mats, int M, int R, long F, hipStream_t s) {
  if (F < 1 || F >= (1L << 31) || !lr_rank(R) || M < 1 || M > 65535) return 1;
  hipLaunchKernelGGL(lr_orth_kernel, dim3(M), dim3(LR_ORTH), 0, s, payload, mats, M, R, F);
  return hipGetLastError() == hipSuccess ? 0 : 3;
}

// payload[fac + rows R ..] = Q' = a^T P^; part: ntiles * 64 * R floats; tiles [ntiles, 3], ftiles [nf, 4]
extern "C" int fr_lowrank_backproject(const float* local, const float* global, const float* residual, float* payload,
                                      float* part, const int* mats, const int* tiles, int ntiles, const int* ftiles,
                                      int nf, int M, int R, long n, long F, int max_blocks, hipStream_t s) {
  if (n < 1 || n >= (1L << 31) || F < 1 || F >= (1L << 31) || !lr_rank(R) || M < 1 || ntiles < 1 || nf < 1) return 1;
  hipLaunchKernelGGL(lr_backproject_kernel, dim3(lr_grid(ntiles, max_blocks)), dim3(LR_BLOCK), 0, s, local, global,
                     residual, payload, part, mats, tiles, ntiles, M, R, n, F);
  hipLaunchKernelGGL(lr_backproject_finish_kernel, dim3(lr_grid(nf, max_blocks)), dim3(LR_BLOCK), 0, s, part, payload,
                     mats, ftiles, nf, ntiles, M, R, F);
  return hipGetLastError() == hipSuccess ? 0 : 3;
}

#define LR_BY_RANK(KERNEL, ...)                                                                     \
  switch (R) {                                                                                       \
    case 1: hipLaunchKernelGGL(KERNEL<1>, grid, dim3(LR_BLOCK), 0, s, __VA_ARGS__); break;          \
    case 2: hipLaunchKernelGGL(KERNEL<2>, grid, dim3(LR_BLOCK), 0, s, __VA_ARGS__); break;          \
    case 4: hipLaunchKernelGGL(KERNEL<4>, grid, dim3(LR_BLOCK), 0, s, __VA_ARGS__); break;          \
    default: hipLaunchKernelGGL(KERNEL<8>, grid, dim3(LR_BLOCK), 0, s, __VA_ARGS__); break;         \
  }

// residual = a - decode(payload) on the matrices; payload = a and residual = +0.0 on the rest; tiles [ntiles, 3]
extern "C" int fr_lowrank_residual(const float* local, const float* global, float* residual, float* payload,
                                   const int* mats, const int* rest, const int* tiles, int ntiles, int M, int S, int R,
                                   long n, long F, long L, int max_blocks, hipStream_t s) {
  if (n < 1 || n >= (1L << 31) || F < 1 || L < F || L >= (1L << 31) || !lr_rank(R) || M < 1 || S < 0 || ntiles < 1)
    return 1;
  const int vec = lr_al16(local) && lr_al16(global) && lr_al16(residual);
  const dim3 grid(lr_grid(ntiles, max_blocks));
  LR_BY_RANK(lr_residual_kernel, local, global, residual, payload, mats, rest, tiles, ntiles, M, S, n, F, L, vec)
  return hipGetLastError() == hipSuccess ? 0 : 3;
}

// out = base + (sum over the W rows of stack [W, L] of weights[c] * decode(row c)) / sum(weights)
extern "C" int fr_lowrank_combine(const float* base, const float* stack, const float* weights, float* out,
                                  const int* mats, const int* rest, const int* tiles, int ntiles, int M, int S, int R,
                                  int W, long n, long F, long L, int max_blocks, hipStream_t s) {
  if (n < 1 || n >= (1L << 31) || F < 1 || L < F || L >= (1L << 31) || !lr_rank(R) || M < 1 || S < 0 || ntiles < 1 ||
      W < 1 || W > 65536 || (long)W * L >= (1L << 40))
    return 1;
  const int vec = lr_al16(base) && lr_al16(out);
  const dim3 grid(lr_grid(ntiles, max_blocks));
  LR_BY_RANK(lr_combine_kernel, base, stack, weights, out, mats, rest, tiles, ntiles, M, S, W, n, F, L, vec)
  return hipGetLastError() == hipSuccess ? 0 : 3;
}
