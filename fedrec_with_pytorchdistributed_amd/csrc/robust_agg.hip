// Byzantine-robust aggregation: coordinate-wise trimmed mean / median of W <= 32 client vectors
// (Yin et al. 2018), fused.  stack [W, n] fp32 -> out [n] fp32, dropped [W] int64.
//
// The contract (ops/reference.py trimmed_mean is the same form in torch):
//   * key(x): NaN -> 0xFFFFFFFF; sign bit set -> ~bits; else bits | 0x80000000.  A monotone uint32
//     image of the float: -inf < ... < -0.0 < +0.0 < ... < +inf < NaN.  A coordinate's W values are
//     ranked by (key, client index), a total order.
//   * trim > 0: out = (v[trim] + v[trim + 1] + ... + v[W - trim - 1]) / float(W - 2 trim), v the
//     values in rank order, fp32 adds left to right from the first kept value, one IEEE division.
//     dropped[c] counts the coordinates where client c ranked among the trim lowest or trim highest.
//   * trim = 0: nothing is ranked; out = (x[0] + x[1] + ... + x[W - 1]) / float(W) in CLIENT order
//     (the plain mean, bit for bit), dropped = 0.
//
// One lane owns V consecutive coordinates (V = 4 with 16-byte loads where every row start is
// 16-byte aligned and W <= 16; else V = 1) and walks a grid-stride loop over them (a contiguous run
// per block measured 4-8 % slower at n = 67.5 M); all W row loads are issued before the first
// compare.  Only the KEYS are sorted (a Batcher odd-even merge network
// generated at compile time for the exact W: v_min_u32 / v_max_u32 per compare-exchange); the kept
// values are recovered from the sorted keys (key -> float is exact but for a NaN's payload), so no
// value travels through the network.  The dropped bits follow from the two threshold keys
// s[trim - 1] and s[W - trim] in client-order passes that hand the tied clients out by index.
// Every array index is a compile-time constant (no private memory); a coordinate's result depends
// on its own column alone, so out is bitwise independent of grid, block, path and call split.
// dropped: per-lane integer counters -> wave shuffle -> LDS -> one 64-bit integer atomic per client
// per block (integer adds commute: deterministic).  No float atomics.
#include <utility>

#include "common.h"
#include "launchers.h"

namespace {

constexpr int MAXW = 32;
constexpr int MAXCMP = 192;  // Batcher's network at 32 inputs has 191 comparators

struct Net {
  int n;
  unsigned char lo[MAXCMP], hi[MAXCMP];
};

// Batcher's odd-even merge sort for any W: the network of the next power of two with every
// comparator that touches an index >= W left out (those inputs would hold +infinity and never move)
template <int W>
constexpr Net make_net() {
  Net t{};
  for (int p = 1; p < W; p <<= 1)
    for (int k = p; k >= 1; k >>= 1)
      for (int j = k % p; j + k < W; j += 2 * k)
        for (int i = 0; i < k && i + j + k < W; ++i)
          if ((i + j) / (2 * p) == (i + j + k) / (2 * p)) {
            t.lo[t.n] = (unsigned char)(i + j);
            t.hi[t.n] = (unsigned char)(i + j + k);
            ++t.n;
          }
  return t;
}

template <int W>
struct NetOf {
  static constexpr Net net = make_net<W>();
};

__device__ __forceinline__ void cswap(uint32_t& a, uint32_t& b) {
  const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
  a = lo;
  b = hi;
}

template <int W, size_t I>
__device__ __forceinline__ void cswap_at(uint32_t (&a)[W]) {
  constexpr int L = NetOf<W>::net.lo[I], H = NetOf<W>::net.hi[I];
  cswap(a[L], a[H]);
}

template <int W, size_t... Is>
__device__ __forceinline__ void sort_keys(uint32_t (&a)[W], std::index_sequence<Is...>) {
  (cswap_at<W, Is>(a), ...);
}

__device__ __forceinline__ uint32_t key_of(float x) {
  const uint32_t b = __float_as_uint(x);
  const uint32_t k = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  return (b & 0x7FFFFFFFu) > 0x7F800000u ? 0xFFFFFFFFu : k;
}

// the inverse; 0xFFFFFFFF (NaN) comes back as 0x7FFFFFFF, a NaN
__device__ __forceinline__ float value_of(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

// one coordinate: keys in client order -> the trimmed mean; cnt[c] += client c dropped here
template <int W>
__device__ __forceinline__ float one_coord(const uint32_t (&key)[W], int trim, float denom, uint32_t (&cnt)[W]) {
  uint32_t s[W];
#pragma unroll
  for (int c = 0; c < W; ++c) s[c] = key[c];
  sort_keys<W>(s, std::make_index_sequence<NetOf<W>::net.n>{});
  // the thresholds and the kept sum: compile-time indices, the (wave-uniform) trim selects
  uint32_t lo = 0, hi = 0;
  float acc = 0.f;
#pragma unroll
  for (int r = 0; r < W; ++r) {
    if (r == trim - 1) lo = s[r];
    if (r == W - trim) hi = s[r];
    const float v = value_of(s[r]);
    if (r == trim) acc = v;
    else if (r > trim && r < W - trim) acc += v;
  }
  // ties at a threshold: the low side takes the lowest client indices, the high side the highest
  int rem_lo = trim, rem_hi = trim;
#pragma unroll
  for (int c = 0; c < W; ++c) {
    rem_lo -= key[c] < lo ? 1 : 0;
    rem_hi -= key[c] > hi ? 1 : 0;
  }
#pragma unroll
  for (int c = 0; c < W; ++c) {
    const bool t = key[c] == lo && rem_lo > 0;
    rem_lo -= t ? 1 : 0;
    cnt[c] += (key[c] < lo || t) ? 1u : 0u;
  }
#pragma unroll
  for (int c = W - 1; c >= 0; --c) {
    const bool t = key[c] == hi && rem_hi > 0;
    rem_hi -= t ? 1 : 0;
    cnt[c] += (key[c] > hi || t) ? 1u : 0u;
  }
  return acc / denom;
}

template <int V>
struct Vec;
template <>
struct Vec<1> {
  typedef float T;
};
template <>
struct Vec<4> {
  typedef f32x4 T;
};

template <int V>
__device__ __forceinline__ float comp(const typename Vec<V>::T& v, int j) {
  if constexpr (V == 1) return v;
  else return v[j];
}

// n % V == 0 and 16-byte aligned rows when V == 4 (the launcher's choice)
// W <= 8 on the 16-byte path: at least 6 waves per SIMD (<= 80 VGPRs) -- the kernel is bound by the
// bytes it has in flight, and left alone the compiler spends 111 VGPRs at W = 8 (4 waves)
template <int W, int V>
constexpr int min_waves() {
  return V == 4 && W <= 8 ? 6 : 1;
}

template <int W, int V>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(min_waves<W, V>()))) void trimmed_mean_kernel(const float* __restrict__ stack, float* __restrict__ out,
                                                           unsigned long long* __restrict__ dropped, long n,
                                                           int trim) {
  typedef typename Vec<V>::T VT;
  __shared__ uint32_t blk[MAXW];
  if (threadIdx.x < MAXW) blk[threadIdx.x] = 0;
  __syncthreads();
  uint32_t cnt[W];
#pragma unroll
  for (int c = 0; c < W; ++c) cnt[c] = 0;
  const float denom = (float)(W - 2 * trim);
  const long nv = n / V;
  for (long g = blockIdx.x * (long)blockDim.x + threadIdx.x; g < nv; g += (long)gridDim.x * blockDim.x) {
    VT x[W];
#pragma unroll
    for (int c = 0; c < W; ++c) x[c] = *reinterpret_cast<const VT*>(stack + (size_t)c * (size_t)n + (size_t)g * V);
    VT o;
    if (trim == 0) {  // the mean in client order
      o = x[0];
#pragma unroll
      for (int c = 1; c < W; ++c) o += x[c];
      o = o / denom;
    } else {
#pragma unroll
      for (int j = 0; j < V; ++j) {
        uint32_t key[W];
#pragma unroll
        for (int c = 0; c < W; ++c) key[c] = key_of(comp<V>(x[c], j));
        const float r = one_coord<W>(key, trim, denom, cnt);
        if constexpr (V == 1) o = r;
        else o[j] = r;
      }
    }
    *reinterpret_cast<VT*>(out + (size_t)g * V) = o;
  }
  if (trim == 0) return;  // uniform: dropped stays 0
#pragma unroll
  for (int c = 0; c < W; ++c) {
    uint32_t v = cnt[c];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane_id() == 0 && v) atomicAdd(&blk[c], v);
  }
  __syncthreads();
  if (threadIdx.x < W && blk[threadIdx.x]) atomicAdd(&dropped[threadIdx.x], (unsigned long long)blk[threadIdx.x]);
}

template <int W, int V>
void launch(const float* stack, float* out, unsigned long long* dropped, long n, int trim, hipStream_t s) {
  if constexpr (V == 4 && W > 16) {
    (void)stack, (void)out, (void)dropped, (void)n, (void)trim, (void)s;
  } else {
    // (a block's uint32 counters hold its share of n: no overflow below 2^32 coordinates per block)
    const long nv = n / V, need = (nv + 255) / 256, cap = (long)fr_num_cus() * 8;
    const long grid = need < cap ? need : cap;
    hipLaunchKernelGGL((trimmed_mean_kernel<W, V>), dim3((unsigned)grid), dim3(256), 0, s, stack, out, dropped, n, trim);
  }
}

template <int V, size_t... Is>
void dispatch(int W, const float* stack, float* out, unsigned long long* dropped, long n, int trim, hipStream_t s,
              std::index_sequence<Is...>) {
  ((W == (int)Is + 1 ? launch<(int)Is + 1, V>(stack, out, dropped, n, trim, s) : (void)0), ...);
}

}  // namespace

// stack [W, n] fp32 contiguous -> out [n] fp32, dropped [W] int64 (zeroed here).  1: a shape outside
// 1 <= W <= 32, n >= 1, 0 <= 2 trim < W
extern "C" int fr_trimmed_mean(const float* stack, float* out, long long* dropped, int W, long n, int trim,
                               hipStream_t s) {
  if (W < 1 || W > MAXW || n < 1 || trim < 0 || 2 * trim >= W) return 1;
  if (hipMemsetAsync(dropped, 0, sizeof(long long) * (size_t)W, s) != hipSuccess) return 3;
  auto* d = reinterpret_cast<unsigned long long*>(dropped);
  const bool vec = W <= 16 && n % 4 == 0 && ((uintptr_t)stack & 15) == 0 && ((uintptr_t)out & 15) == 0;
  if (vec) dispatch<4>(W, stack, out, d, n, trim, s, std::make_index_sequence<MAXW>{});
  else dispatch<1>(W, stack, out, d, n, trim, s, std::make_index_sequence<MAXW>{});
  return 0;
}
