// Elias-Fano coding of a top-k upload's index list (lossless): k strictly ascending int32 positions in [0, n) become
// b + 1 + n / (k 2^b) bits each instead of 32, and the size depends on (n, k) alone.
//
// The format (ops/reference.py ef_plan / ef_encode / ef_decode are the same definition in integer torch), for
// 1 <= k <= n < 2^31:
//   b           the largest integer with (k << b) <= n (0 when k > n / 2)
//   low         k fields of b bits, idx_i & (2^b - 1); field i at bit i b, LSB first in little-endian uint32 words;
//               low_words = ceil(k b / 32)
//   high        a bit vector of high_bits = k + ((n - 1) >> b) + 1 bits, bit (idx_i >> b) + i set for every i;
//               high_words = ceil(high_bits / 32)
//   blob        the low words, then the high words; every padding bit zero
// Every bit's place is known from (i, idx_i) alone: no prefix sum over code lengths as in Golomb / Rice.
//
// encode, one launch, every output word written exactly once, no atomics on memory, no memset:
//   low blocks   a wave owns 64 consecutive fields = 2 b whole words: the lanes stage their masked low parts in LDS,
//                lane j < 2 b gathers the fields that meet word j through a 64-bit shift and stores it; the wave's
//                stores are 8 b contiguous bytes
//   high blocks  a block owns a tile of TILE blob words, cut on the blob's 16-byte grid.  h_i = (idx_i >> b) + i is
//                strictly increasing, so two binary searches over i (two lanes, side by side) give the run of elements
//                whose bit falls in the tile; the lanes OR their bits into the tile in LDS (an integer OR is order-free)
//                and the tile leaves in 16-byte stores, zeros where no element fell
//
// decode, batched over W blobs, three launches on one stream, no host synchronisation, no spinning:
//   count        popcount of every tile of TILE high words -> part[c, T]
//   scan         one block per blob: the exclusive prefix sums of its tiles in ascending order, count[c] = the total,
//                idx[c, i] = -1 for the ranks i in [count, k) that no set bit will fill
//   decode       a lane takes one high word: popcount, an exclusive scan over the wave (four DPP row shifts, then the
//                row totals by readlane), over the block's waves through LDS, plus the tile's prefix = the rank i of
//                its first set bit.  It walks its set bits (ctz, clear lowest): bit p of word j with rank i is
//                high = 32 j + p - i, the low field is the 64-bit window at bit i b of the low section,
//                idx_i = (high << b) | low.
// The decoder is memory-safe for ANY blob: it writes idx[c, i] only for i < k, reads low word q only for q <
// low_words, and writes -1 where the value is not in [0, n).  A malformed blob yields a wrong idx and a wrong count,
// which the caller rejects (ops.reference.ef_decoded_check, then sparse_upload_check).
#include "common.h"
#include "launchers.h"

namespace {

typedef unsigned long long u64;
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int BLOCK = 256;
constexpr int WAVES = BLOCK / 64;
constexpr int TILE = 256;      // high words per block: one per lane in decode, 64 16-byte stores in encode
constexpr int LOW_ITERS = 4;   // groups of BLOCK fields a low block packs
constexpr unsigned SAT = 0x80000000u;  // a rank at or above every k: prefix sums saturate here instead of wrapping

struct Plan {
  int b;
  long low_words, high_bits, high_words;
};

inline Plan plan_of(long n, long k) {
  Plan p;
  p.b = 0;
  while ((k << (p.b + 1)) <= n) ++p.b;
  p.low_words = (k * p.b + 31) / 32;
  p.high_bits = k + ((n - 1) >> p.b) + 1;
  p.high_words = (p.high_bits + 31) / 32;
  return p;
}

// (idx_i >> b) + i; unsigned, so that ANY int32 gives a position below 2^33
__device__ __forceinline__ long high_pos(const int* __restrict__ idx, long i, int b) {
  return (long)((unsigned)idx[i] >> b) + i;
}

// the first i in [0, k] with high_pos(i) >= target
__device__ __forceinline__ long lower_bound(const int* __restrict__ idx, long k, int b, long target) {
  long lo = 0, hi = k;
  while (lo < hi) {
    const long m = (lo + hi) >> 1;
    if (high_pos(idx, m, b) < target) lo = m + 1;
    else hi = m;
  }
  return lo;
}

// blocks [0, nlow): the low section; blocks [nlow, nlow + ntiles): tiles of the high section.  base4 = low_words & ~3:
// tile T covers the blob words [base4 + TILE T, + TILE), of which those in [low_words, total) are high words
__global__ __launch_bounds__(BLOCK) void ef_encode_kernel(const int* __restrict__ idx, unsigned* __restrict__ words,
                                                         long k, int b, long low_words, long total, int nlow) {
  __shared__ unsigned lds[BLOCK];  // low: a group's fields; high: the tile (TILE == BLOCK)
  const int t = threadIdx.x, lane = lane_id(), w = t >> 6;
  if ((int)blockIdx.x < nlow) {
    const unsigned mask = (1u << b) - 1u;  // (b >= 1 here, and b <= 30)
#pragma unroll 1
    for (int it = 0; it < LOW_ITERS; ++it) {
      const long f0 = ((long)blockIdx.x * LOW_ITERS + it) * BLOCK;  // the block's first field of this group
      if (f0 >= k) break;                                           // (uniform over the block)
      __syncthreads();                                              // the previous group's fields are no longer read
      lds[t] = f0 + t < k ? (unsigned)idx[f0 + t] & mask : 0u;
      __syncthreads();
      const long word = (f0 + 64 * w) / 32 * b + lane;  // 64 fields are 2 b whole words: the wave's start at 2 b g
      if (lane < 2 * b && word < low_words) {
        const int bit0 = 32 * lane;  // the word's first bit in the wave's stream of 64 b bits
        u64 acc = 0;
        for (int f = bit0 / b; f * b < bit0 + 32; ++f)  // (f < 64: bit0 + 32 <= 64 b)
          acc |= (u64)lds[64 * w + f] << (f * b - bit0 + 32);  // the shift is in [33 - b, 63]
        words[word] = (unsigned)(acc >> 32);
      }
    }
    return;
  }
  const long a0 = (low_words & ~3L) + (long)((int)blockIdx.x - nlow) * TILE;  // the tile's first blob word
  const long p0 = (a0 - low_words) * 32, p1 = p0 + 32L * TILE;                // its bits of the high vector
  __shared__ long run[2];
  lds[t] = 0u;
  if (t < 2) run[t] = lower_bound(idx, k, b, t == 0 ? p0 : p1);
  __syncthreads();
  for (long i = run[0] + t; i < run[1]; i += BLOCK) {
    const long h = high_pos(idx, i, b);
    if (h >= p0 && h < p1) atomicOr(&lds[(h - p0) >> 5], 1u << (h & 31));  // (always, for an ascending idx)
  }
  __syncthreads();
  if (t < TILE / 4) {
    const long a = a0 + 4 * t;
    if (a >= low_words && a + 4 <= total) {
      *reinterpret_cast<u32x4*>(words + a) = u32x4{lds[4 * t], lds[4 * t + 1], lds[4 * t + 2], lds[4 * t + 3]};
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (a + e >= low_words && a + e < total) words[a + e] = lds[4 * t + e];
    }
  }
}

// grid (ntiles, W): part[c, T] = the set bits of the high words [TILE T, TILE T + TILE) of blob c
__global__ __launch_bounds__(BLOCK) void ef_count_kernel(const unsigned* __restrict__ words, unsigned* __restrict__ part,
                                                        long low_words, long high_words, long stride, int ntiles) {
  __shared__ unsigned ws[WAVES];
  const unsigned* high = words + (size_t)blockIdx.y * stride + low_words;
  const long j = (long)blockIdx.x * TILE + threadIdx.x;
  unsigned pc = j < high_words ? __popc(high[j]) : 0u;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) pc += __shfl_xor(pc, o, 64);
  if (lane_id() == 0) ws[threadIdx.x >> 6] = pc;
  __syncthreads();
  if (threadIdx.x == 0) part[(size_t)blockIdx.y * ntiles + blockIdx.x] = ws[0] + ws[1] + ws[2] + ws[3];
}

// one block per blob: part[c, :] -> its exclusive prefix sums (saturating at SAT), count[c], and -1 at the ranks
// [count, k) of idx[c]
__global__ __launch_bounds__(BLOCK) void ef_scan_kernel(unsigned* __restrict__ part, long* __restrict__ count,
                                                       int* __restrict__ idx, long k, int ntiles) {
  __shared__ u64 s[BLOCK];
  const int t = threadIdx.x;
  unsigned* row = part + (size_t)blockIdx.x * ntiles;
  const int chunk = (ntiles + BLOCK - 1) / BLOCK;
  const int t0 = t * chunk < ntiles ? t * chunk : ntiles, t1 = t0 + chunk < ntiles ? t0 + chunk : ntiles;
  u64 sum = 0;
  for (int i = t0; i < t1; ++i) sum += row[i];
  s[t] = sum;
  __syncthreads();
  for (int o = 1; o < BLOCK; o <<= 1) {  // inclusive prefix sums
    const u64 v = t >= o ? s[t - o] : 0ull;
    __syncthreads();
    s[t] += v;
    __syncthreads();
  }
  u64 run = s[t] - sum;
  for (int i = t0; i < t1; ++i) {
    const unsigned c = row[i];
    row[i] = run < SAT ? (unsigned)run : SAT;
    run += c;
  }
  const u64 total = s[BLOCK - 1];
  if (t == 0) count[blockIdx.x] = (long)total;
  for (long i = (long)total + t; i < k; i += BLOCK) idx[(size_t)blockIdx.x * k + i] = -1;
}

template <int CTRL>
__device__ __forceinline__ unsigned dpp0(unsigned v) {  // lanes without a source read 0
  return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, true);
}

// the sum of v over the lower lanes of the wave; total: over all 64
__device__ __forceinline__ unsigned wave_exclusive(unsigned v, unsigned& total) {
  unsigned x = v;
  x += dpp0<0x111>(x);  // row_shr:1
  x += dpp0<0x112>(x);  // row_shr:2
  x += dpp0<0x114>(x);  // row_shr:4
  x += dpp0<0x118>(x);  // row_shr:8 -> inclusive within the row of 16
  const unsigned r0 = __builtin_amdgcn_readlane(x, 15), r1 = __builtin_amdgcn_readlane(x, 31),
                 r2 = __builtin_amdgcn_readlane(x, 47), r3 = __builtin_amdgcn_readlane(x, 63);
  const int row = lane_id() >> 4;
  total = r0 + r1 + r2 + r3;
  return x - v + (row > 0 ? r0 : 0u) + (row > 1 ? r1 : 0u) + (row > 2 ? r2 : 0u);
}

// grid (ntiles, W); offs: ef_scan_kernel's prefix sums
__global__ __launch_bounds__(BLOCK) void ef_decode_kernel(const unsigned* __restrict__ words,
                                                         const unsigned* __restrict__ offs, int* __restrict__ idx,
                                                         long n, long k, int b, long low_words, long high_words,
                                                         long stride, int ntiles) {
  __shared__ unsigned ws[WAVES];
  const unsigned* low = words + (size_t)blockIdx.y * stride;
  const unsigned* high = low + low_words;
  int* out = idx + (size_t)blockIdx.y * k;
  const int w = threadIdx.x >> 6;
  const long j = (long)blockIdx.x * TILE + threadIdx.x;
  unsigned bits = j < high_words ? high[j] : 0u;
  unsigned total;
  const unsigned ex = wave_exclusive(__popc(bits), total);
  if (lane_id() == 0) ws[w] = total;
  __syncthreads();
  // below SAT + 32 TILE: no wrap
  unsigned i = offs[(size_t)blockIdx.y * ntiles + blockIdx.x] + ex + (w > 0 ? ws[0] : 0u) + (w > 1 ? ws[1] : 0u) +
               (w > 2 ? ws[2] : 0u);
  const unsigned mask = (1u << b) - 1u;
  while (bits != 0u && (long)i < k) {
    const int p = __builtin_ctz(bits);
    bits &= bits - 1u;
    const long hi = 32 * j + p - (long)i;
    unsigned lo = 0u;
    if (b > 0) {
      const u64 at = (u64)i * (u64)b;  // (< k b <= 32 low_words)
      const long q = (long)(at >> 5);
      const u64 win = (u64)low[q] | (q + 1 < low_words ? (u64)low[q + 1] << 32 : 0ull);
      lo = (unsigned)(win >> (at & 31u)) & mask;
    }
    const long v = hi >= 0 && hi <= (n >> b) ? (hi << b) | (long)lo : -1L;  // (hi << b <= n: no overflow)
    out[i] = v < n ? (int)v : -1;
    ++i;
  }
}

}  // namespace

extern "C" int fr_ef_plan(long n, long k, int* b, long* low_words, long* high_bits, long* high_words) {
  if (n < 1 || n >= (1L << 31) || k < 1 || k > n) return 1;
  const Plan p = plan_of(n, k);
  *b = p.b;
  *low_words = p.low_words;
  *high_bits = p.high_bits;
  *high_words = p.high_words;
  return 0;
}

// 1: a shape outside 1 <= k <= n < 2^31; 2: words off the 16-byte grid; 3: a runtime error
extern "C" int fr_ef_encode(const int* idx, int* words, long n, long k, hipStream_t s) {
  if (n < 1 || n >= (1L << 31) || k < 1 || k > n) return 1;
  if ((uintptr_t)words & 15u) return 2;
  const Plan p = plan_of(n, k);
  const long total = p.low_words + p.high_words;
  const int nlow = p.b ? (int)((k + (long)BLOCK * LOW_ITERS - 1) / ((long)BLOCK * LOW_ITERS)) : 0;
  const int ntiles = (int)((total - (p.low_words & ~3L) + TILE - 1) / TILE);
  hipLaunchKernelGGL(ef_encode_kernel, dim3((unsigned)(nlow + ntiles)), dim3(BLOCK), 0, s, idx, (unsigned*)words, k, p.b,
                     p.low_words, total, nlow);
  return hipGetLastError() == hipSuccess ? 0 : 3;
}

// the workspace of fr_ef_decode in 32-bit words; -1: a shape outside 1 <= k <= n < 2^31, 1 <= W <= 65535
extern "C" long fr_ef_decode_ws(long n, long k, int W) {
  if (n < 1 || n >= (1L << 31) || k < 1 || k > n || W < 1 || W > 65535) return -1;
  return (long)W * ((plan_of(n, k).high_words + TILE - 1) / TILE);
}

// words [W, low_words + high_words] -> idx [W, k], count [W]
extern "C" int fr_ef_decode(const int* words, int* idx, long* count, unsigned* ws, int W, long n, long k, hipStream_t s) {
  if (fr_ef_decode_ws(n, k, W) < 0) return 1;
  const Plan p = plan_of(n, k);
  const long stride = p.low_words + p.high_words;
  const int ntiles = (int)((p.high_words + TILE - 1) / TILE);
  const dim3 grid((unsigned)ntiles, (unsigned)W), blk(BLOCK);
  hipLaunchKernelGGL(ef_count_kernel, grid, blk, 0, s, (const unsigned*)words, ws, p.low_words, p.high_words, stride, ntiles);
  hipLaunchKernelGGL(ef_scan_kernel, dim3((unsigned)W), blk, 0, s, ws, count, idx, k, ntiles);
  hipLaunchKernelGGL(ef_decode_kernel, grid, blk, 0, s, (const unsigned*)words, (const unsigned*)ws, idx, n, k, p.b,
                     p.low_words, p.high_words, stride, ntiles);
  return hipGetLastError() == hipSuccess ? 0 : 3;
}
