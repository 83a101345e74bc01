// Top-k sparsified uploads with error feedback (Stich et al. 2018; Lin et al. 2018): the exact
// magnitude top-k of one very long row, and the owner-computes scatter of W sparse lists.
//
// topk_delta: local, global, residual [n] fp32, 1 <= k <= n < 2^31 -> idx [k] int32, val [k] fp32,
// residual updated in place.  The contract (ops/reference.py topk_delta is the same form in torch):
//   a[i]   = (local[i] - global[i]) + residual[i]     one fp32 subtraction, one fp32 addition
//   key[i] = bits(a[i]) & 0x7fffffff as uint32        magnitude order: +-0 lowest, inf above every
//                                                     finite value, every NaN above inf
//   the selected set is the first k entries of a stable descending sort of key (ties: lower index);
//   idx is that set ascending, val[j] = a[idx[j]] (its bits), and afterwards residual[i] = +0.0 at
//   the selected coordinates and a[i] elsewhere.
// Every output bit is a function of the inputs alone: integer counts decide everything, so grid,
// block size and launch order cannot show.
//
// A radix select on the key, 11 + 11 + 10 bits, with no host synchronisation -- the launch sequence
// depends on (n, k) and the pointers' alignment only; threshold, remaining count and block offsets
// stay in the workspace:
//   hist<21, first>   a -> residual, histogram of key >> 21            reads 12 n, writes 4 n bytes
//   select            the digit that holds the k-th largest key; k -= count above it
//   hist<10>, select  the same among the keys that share the digits found so far      4 n each
//   hist<0>, select   -> T, the k-th largest key, and krem = k - count(key > T)
//   count             per block of SPAN coordinates: count(key > T), count(key == T)  4 n
//   scan              exclusive scan of the block counts (one block)
//   write             i is selected iff key > T, or key == T and fewer than krem equal keys precede
//                     it; its slot is the number of selected coordinates before it, so idx comes
//                     out ascending with no sort                          4 n + what is selected
// Histograms live in LDS per block and reach the global bins with integer atomics (integer sums
// commute).  Real deltas sit in a handful of exponents, so before a wave touches a bin it takes
// the first active lane's digit, counts the lanes that share it with a ballot and adds that count
// once; only the lanes with another digit add on their own (Guideline 12: aggregate in the wave
// before the shared bin).  No float atomics anywhere.
//
// Addressing: coordinates are shifted by off = (residual's address / 4) & 3, so that a group of
// four shifted coordinates is one 16-byte line of residual; groups wholly inside [off, off + n) use
// 16-byte loads and stores, the ragged first and last group go element by element (a view such as
// x[1:] is a legal input).  local and global take the 16-byte path when they are misaligned like
// residual, else scalar loads.
//
// combine: base [n], idx [W, k] int32 (each row strictly ascending in [0, n): the caller's check),
// val [W, k], weights [W] -> out [n]:  acc = +0.0; for c = 0 .. W-1 in order acc[idx[c, j]] +=
// weights[c] * val[c, j] (product and sum rounded separately); out = base + acc / wsum, wsum the
// sequential fp32 sum of the weights from +0.0.  A block owns TILE coordinates whose accumulators
// live in LDS; per client it finds the tile's lower bound in that client's list by binary search
// (64 clients' searches run side by side), walks the entries below the upper bound and adds them,
// then waits at a barrier: indices are unique within a client, so no races and no atomics.  The
// kernel is memory-safe for ANY idx content: it writes tile[idx - lo] only after lo <= idx < hi.
#include "common.h"
#include "launchers.h"

// weights[c] * val and the add that follows are rounded separately, whatever flags build this file.
// The arithmetic below is written with plain operators under this pragma: __fmul_rn / __fadd_rn are
// inline functions of a header compiled with contraction allowed, and were fused after inlining
#pragma clang fp contract(off)

namespace {

typedef unsigned long long u64;

constexpr int BLOCK = 256;
constexpr int SPAN = 4096;             // shifted coordinates per block in count / write
constexpr int WAVE_SPAN = SPAN / 4;    // one wave's contiguous run: 4 iterations of 64 lanes x 4
constexpr int ITERS = WAVE_SPAN / 256;
constexpr int NBINS = 2048;
constexpr int WS_HIST = 3 * NBINS;     // three histograms, then state[4] = {T, krem, -, -}
constexpr int WS_HEAD = WS_HIST + 4;   // then 2 words per block: count(key > T), count(key == T)
constexpr int TILE = 4096;             // combine: coordinates per block

__device__ __forceinline__ uint32_t key_of(float a) { return __float_as_uint(a) & 0x7FFFFFFFu; }

// four shifted coordinates v0 .. v0 + 3 of p (p[v - off]); valid: bit e set iff off <= v0 + e < hi
__device__ __forceinline__ f32x4 load_grp(const float* __restrict__ p, uint32_t v0, uint32_t off, uint32_t hi,
                                          bool vec, unsigned& valid) {
  f32x4 x = {0.f, 0.f, 0.f, 0.f};
  if (v0 >= off && v0 + 4u <= hi) {
    valid = 0xFu;
    if (vec) {
      x = *reinterpret_cast<const f32x4*>(p + (v0 - off));
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) x[e] = p[v0 + e - off];
    }
  } else {
    valid = 0u;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint32_t v = v0 + e;
      if (v >= off && v < hi) {
        x[e] = p[v - off];
        valid |= 1u << e;
      }
    }
  }
  return x;
}

// every lane of the wave calls it: one add for the lanes that share the first active lane's bin
__device__ __forceinline__ void hist_add(unsigned* h, unsigned d, bool act) {
  const u64 m = __ballot(act);
  if (m == 0) return;
  const int leader = __ffsll(m) - 1;
  const unsigned d0 = __shfl(d, leader, 64);
  const u64 same = __ballot(act && d == d0);
  if (lane_id() == leader) atomicAdd(&h[d0], (unsigned)__popcll(same));
  else if (act && d != d0) atomicAdd(&h[d], 1u);
}

// FIRST: a = (local - global) + residual -> residual.  Histogram of digit (key >> SHIFT) & (2^BITS - 1)
// over the keys whose bits above the digit equal those of state[0]
template <int SHIFT, int BITS, bool FIRST>
__global__ __launch_bounds__(BLOCK) void hist_kernel(const float* __restrict__ local, const float* __restrict__ global,
                                                    float* __restrict__ residual, uint32_t off, uint32_t hi, int vec_lg,
                                                    const unsigned* __restrict__ state, unsigned* __restrict__ hist) {
  __shared__ unsigned h[NBINS];
  for (int b = threadIdx.x; b < NBINS; b += BLOCK) h[b] = 0;
  __syncthreads();
  const uint32_t prefix = FIRST ? 0u : state[0];
  const uint32_t ngroups = (hi + 3u) >> 2;
  for (uint32_t g0 = blockIdx.x * (uint32_t)BLOCK; g0 < ngroups; g0 += gridDim.x * (uint32_t)BLOCK) {
    const uint32_t g = g0 + threadIdx.x;
    const uint32_t v0 = g << 2;
    unsigned valid = 0;
    f32x4 a = {0.f, 0.f, 0.f, 0.f};
    if (g < ngroups) {
      a = load_grp(residual, v0, off, hi, true, valid);
      if (FIRST) {
        unsigned vl;
        const f32x4 l = load_grp(local, v0, off, hi, vec_lg != 0, vl);
        const f32x4 gl = load_grp(global, v0, off, hi, vec_lg != 0, vl);
#pragma unroll
        for (int e = 0; e < 4; ++e) a[e] = (l[e] - gl[e]) + a[e];
        if (valid == 0xFu) {
          *reinterpret_cast<f32x4*>(residual + (v0 - off)) = a;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if ((valid >> e) & 1u) residual[v0 + e - off] = a[e];
        }
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint32_t key = key_of(a[e]);
      bool act = ((valid >> e) & 1u) != 0;
      if (!FIRST) act = act && (key >> (SHIFT + BITS)) == (prefix >> (SHIFT + BITS));
      hist_add(h, (key >> SHIFT) & ((1u << BITS) - 1u), act);
    }
  }
  __syncthreads();
  for (int b = threadIdx.x; b < NBINS; b += BLOCK)
    if (h[b]) atomicAdd(&hist[b], h[b]);
}

// one block: the digit d with count(digit > d) < krem <= count(digit >= d) among the histogrammed
// keys; state[0] |= d << shift, state[1] = krem - count(digit > d)
__global__ __launch_bounds__(BLOCK) void select_kernel(const unsigned* __restrict__ hist, int shift, unsigned k_first,
                                                      int first, unsigned* __restrict__ state) {
  constexpr int PER = NBINS / BLOCK;
  __shared__ unsigned s[BLOCK];
  const int t = threadIdx.x;
  const unsigned prefix = first ? 0u : state[0];
  const unsigned krem = first ? k_first : state[1];
  unsigned c[PER], sum = 0;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    c[j] = hist[t * PER + j];
    sum += c[j];
  }
  s[t] = sum;
  __syncthreads();
  for (int o = 1; o < BLOCK; o <<= 1) {  // inclusive suffix sums
    const unsigned v = t + o < BLOCK ? s[t + o] : 0u;
    __syncthreads();
    s[t] += v;
    __syncthreads();
  }
  unsigned above = s[t] - sum;  // keys in the bins of the threads above this one
#pragma unroll
  for (int j = PER - 1; j >= 0; --j) {
    if (above < krem && krem <= above + c[j]) {
      state[0] = prefix | ((unsigned)(t * PER + j) << shift);
      state[1] = krem - above;
    }
    above += c[j];
  }
}

__global__ __launch_bounds__(BLOCK) void count_kernel(const float* __restrict__ residual, uint32_t off, uint32_t hi,
                                                     const unsigned* __restrict__ state, unsigned* __restrict__ cnt) {
  __shared__ unsigned tot[2];
  if (threadIdx.x < 2) tot[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t T = state[0];
  const uint32_t base = blockIdx.x * (uint32_t)SPAN + (threadIdx.x >> 6) * (uint32_t)WAVE_SPAN + lane_id() * 4u;
  unsigned ngt = 0, neq = 0;
#pragma unroll
  for (int it = 0; it < ITERS; ++it) {
    unsigned valid;
    const f32x4 x = load_grp(residual, base + it * 256u, off, hi, true, valid);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint32_t key = key_of(x[e]);
      const bool ok = ((valid >> e) & 1u) != 0;
      ngt += (ok && key > T) ? 1u : 0u;
      neq += (ok && key == T) ? 1u : 0u;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    ngt += __shfl_xor(ngt, o, 64);
    neq += __shfl_xor(neq, o, 64);
  }
  if (lane_id() == 0) {
    atomicAdd(&tot[0], ngt);
    atomicAdd(&tot[1], neq);
  }
  __syncthreads();
  if (threadIdx.x < 2) cnt[2 * (size_t)blockIdx.x + threadIdx.x] = tot[threadIdx.x];
}

// one block: cnt[2 b], cnt[2 b + 1] -> their exclusive prefix sums over b, in place
__global__ __launch_bounds__(BLOCK) void scan_kernel(unsigned* __restrict__ cnt, uint32_t nb) {
  __shared__ unsigned s[2][BLOCK];
  const int t = threadIdx.x;
  const uint32_t chunk = (nb + BLOCK - 1) / BLOCK;
  const uint32_t b0 = t * chunk < nb ? t * chunk : nb, b1 = b0 + chunk < nb ? b0 + chunk : nb;
  unsigned g = 0, q = 0;
  for (uint32_t b = b0; b < b1; ++b) {
    g += cnt[2 * (size_t)b];
    q += cnt[2 * (size_t)b + 1];
  }
  s[0][t] = g;
  s[1][t] = q;
  __syncthreads();
  for (int o = 1; o < BLOCK; o <<= 1) {  // inclusive prefix sums
    const unsigned vg = t >= o ? s[0][t - o] : 0u, vq = t >= o ? s[1][t - o] : 0u;
    __syncthreads();
    s[0][t] += vg;
    s[1][t] += vq;
    __syncthreads();
  }
  unsigned rg = s[0][t] - g, rq = s[1][t] - q;
  for (uint32_t b = b0; b < b1; ++b) {
    const unsigned cg = cnt[2 * (size_t)b], cq = cnt[2 * (size_t)b + 1];
    cnt[2 * (size_t)b] = rg;
    cnt[2 * (size_t)b + 1] = rq;
    rg += cg;
    rq += cq;
  }
}

__global__ __launch_bounds__(BLOCK) void write_kernel(float* __restrict__ residual, uint32_t off, uint32_t hi,
                                                     const unsigned* __restrict__ state,
                                                     const unsigned* __restrict__ offs, int* __restrict__ idx,
                                                     float* __restrict__ val, uint32_t k) {
  __shared__ unsigned wtot[4][2];
  const uint32_t T = state[0], krem = state[1];
  const int w = threadIdx.x >> 6, lane = lane_id();
  const uint32_t base = blockIdx.x * (uint32_t)SPAN + w * (uint32_t)WAVE_SPAN + lane * 4u;
  f32x4 x[ITERS];
  unsigned valid[ITERS];
  unsigned ngt = 0, neq = 0;
#pragma unroll
  for (int it = 0; it < ITERS; ++it) {
    x[it] = load_grp(residual, base + it * 256u, off, hi, true, valid[it]);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint32_t key = key_of(x[it][e]);
      const bool ok = ((valid[it] >> e) & 1u) != 0;
      ngt += (unsigned)__popcll(__ballot(ok && key > T));
      neq += (unsigned)__popcll(__ballot(ok && key == T));
    }
  }
  if (lane == 0) {
    wtot[w][0] = ngt;
    wtot[w][1] = neq;
  }
  __syncthreads();
  unsigned G = offs[2 * (size_t)blockIdx.x], E = offs[2 * (size_t)blockIdx.x + 1];
#pragma unroll
  for (int p = 0; p < 3; ++p)
    if (p < w) {
      G += wtot[p][0];
      E += wtot[p][1];
    }
  unsigned slot_base = G + (E < krem ? E : krem);  // selected before this wave's run
  unsigned erun = E;                               // equal keys before this iteration
  const u64 lt = (1ull << lane) - 1ull;
#pragma unroll
  for (int it = 0; it < ITERS; ++it) {
    const uint32_t v0 = base + it * 256u;
    bool iseq[4], isgt[4];
    unsigned ebefore = erun;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint32_t key = key_of(x[it][e]);
      const bool ok = ((valid[it] >> e) & 1u) != 0;
      iseq[e] = ok && key == T;
      isgt[e] = ok && key > T;
      const u64 m = __ballot(iseq[e]);
      ebefore += (unsigned)__popcll(m & lt);
      erun += (unsigned)__popcll(m);
    }
    bool sel[4];
    unsigned sbefore = slot_base;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      sel[e] = isgt[e] || (iseq[e] && ebefore < krem);
      ebefore += iseq[e] ? 1u : 0u;
      const u64 m = __ballot(sel[e]);
      sbefore += (unsigned)__popcll(m & lt);
      slot_base += (unsigned)__popcll(m);
    }
    bool any = false;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (sel[e]) {
        if (sbefore < k) {  // (always: the counts add up to k; the guard keeps a store in bounds regardless)
          idx[sbefore] = (int)(v0 + e - off);
          val[sbefore] = x[it][e];
        }
        ++sbefore;
        x[it][e] = 0.f;
        any = true;
      }
    }
    if (any) {
      if (valid[it] == 0xFu) {
        *reinterpret_cast<f32x4*>(residual + (v0 - off)) = x[it];
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (sel[e]) residual[v0 + e - off] = 0.f;
      }
    }
  }
}

// ---- combine -----------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void combine_kernel(const float* __restrict__ base, const int* __restrict__ idx,
                                                       const float* __restrict__ val, const float* __restrict__ wts,
                                                       float* __restrict__ out, int W, long k, long n, int vec) {
  __shared__ float tile[TILE];
  __shared__ long lbs[64];
  const int t = threadIdx.x;
  const long lo = (long)blockIdx.x * TILE, hi = lo + TILE < n ? lo + TILE : n;
  for (int i = t; i < TILE; i += BLOCK) tile[i] = 0.f;
  for (int c0 = 0; c0 < W; c0 += 64) {
    __syncthreads();  // the tile is zeroed / the previous chunk's bounds are no longer read
    if (t < 64 && c0 + t < W) {  // the first j with idx[c, j] >= lo
      const int* row = idx + (size_t)(c0 + t) * (size_t)k;
      long a = 0, b = k;
      while (a < b) {
        const long m = (a + b) >> 1;
        if ((long)row[m] < lo) a = m + 1;
        else b = m;
      }
      lbs[t] = a;
    }
    __syncthreads();
    const int cn = W - c0 < 64 ? W - c0 : 64;
    for (int c = 0; c < cn; ++c) {
      const int* row = idx + (size_t)(c0 + c) * (size_t)k;
      const float* vrow = val + (size_t)(c0 + c) * (size_t)k;
      const float wc = wts[c0 + c];
      for (long j = lbs[c] + t; j < k; j += BLOCK) {
        const long ix = row[j];
        if (ix >= hi) break;
        if (ix >= lo) tile[ix - lo] = tile[ix - lo] + wc * vrow[j];  // not fused: contraction is off
      }
      __syncthreads();
    }
  }
  __syncthreads();
  float ws = 0.f;
  for (int c = 0; c < W; ++c) ws = ws + wts[c];
  if (vec && hi - lo == TILE) {
#pragma unroll
    for (int i = t * 4; i < TILE; i += BLOCK * 4) {
      const f32x4 b = *reinterpret_cast<const f32x4*>(base + lo + i);
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = b[e] + tile[i + e] / ws;
      *reinterpret_cast<f32x4*>(out + lo + i) = o;
    }
  } else {
    for (long i = lo + t; i < hi; i += BLOCK) out[i] = base[i] + tile[i - lo] / ws;
  }
}

inline uint32_t misalign(const void* p) { return (uint32_t)(((uintptr_t)p >> 2) & 3u); }

}  // namespace

// the workspace of fr_topk_delta in 32-bit words
extern "C" long fr_topk_delta_ws(long n) {
  const long nb = (n + 3 + SPAN - 1) / SPAN + 1;
  return WS_HEAD + 2 * nb;
}

// 1: a shape outside 1 <= k <= n < 2^31; 2: a pointer that is not 4-byte aligned; 3: a runtime error
extern "C" int fr_topk_delta(const float* local, const float* global, float* residual, int* idx, float* val,
                             unsigned* ws, long n, long k, hipStream_t s) {
  if (n < 1 || n >= (1L << 31) || k < 1 || k > n) return 1;
  if (((uintptr_t)local | (uintptr_t)global | (uintptr_t)residual) & 3u) return 2;
  const uint32_t off = misalign(residual), hi = off + (uint32_t)n;
  const int vec_lg = misalign(local) == off && misalign(global) == off;
  const uint32_t ngroups = (hi + 3u) >> 2;
  const uint32_t nb = (hi + SPAN - 1) / SPAN;
  if (hipMemsetAsync(ws, 0, sizeof(unsigned) * WS_HEAD, s) != hipSuccess) return 3;
  unsigned *h0 = ws, *h1 = ws + NBINS, *h2 = ws + 2 * NBINS, *state = ws + WS_HIST, *cnt = ws + WS_HEAD;
  const uint32_t need = (ngroups + BLOCK - 1) / BLOCK, cap = (uint32_t)fr_num_cus() * 8u;
  const dim3 hg(need < cap ? need : cap), blk(BLOCK);
  hipLaunchKernelGGL((hist_kernel<21, 11, true>), hg, blk, 0, s, local, global, residual, off, hi, vec_lg, state, h0);
  hipLaunchKernelGGL(select_kernel, dim3(1), blk, 0, s, h0, 21, (unsigned)k, 1, state);
  hipLaunchKernelGGL((hist_kernel<10, 11, false>), hg, blk, 0, s, local, global, residual, off, hi, vec_lg, state, h1);
  hipLaunchKernelGGL(select_kernel, dim3(1), blk, 0, s, h1, 10, (unsigned)k, 0, state);
  hipLaunchKernelGGL((hist_kernel<0, 10, false>), hg, blk, 0, s, local, global, residual, off, hi, vec_lg, state, h2);
  hipLaunchKernelGGL(select_kernel, dim3(1), blk, 0, s, h2, 0, (unsigned)k, 0, state);
  hipLaunchKernelGGL(count_kernel, dim3(nb), blk, 0, s, residual, off, hi, state, cnt);
  hipLaunchKernelGGL(scan_kernel, dim3(1), blk, 0, s, cnt, nb);
  hipLaunchKernelGGL(write_kernel, dim3(nb), blk, 0, s, residual, off, hi, state, cnt, idx, val, (uint32_t)k);
  return hipGetLastError() == hipSuccess ? 0 : 3;
}

// 1: a shape outside W >= 1, 1 <= k <= n < 2^31
extern "C" int fr_sparse_combine(const float* base, const int* idx, const float* val, const float* weights, float* out,
                                 int W, long k, long n, hipStream_t s) {
  if (W < 1 || n < 1 || n >= (1L << 31) || k < 1 || k > n) return 1;
  const int vec = (((uintptr_t)base | (uintptr_t)out) & 15u) == 0;
  const long nb = (n + TILE - 1) / TILE;
  hipLaunchKernelGGL(combine_kernel, dim3((unsigned)nb), dim3(BLOCK), 0, s, base, idx, val, weights, out, W, k, n, vec);
  return hipGetLastError() == hipSuccess ? 0 : 3;
}
