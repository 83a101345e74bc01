// Block-quantized uploads with error feedback (QSGD, Alistarh et al. 2017; error feedback as in
// Stich et al. 2018, Karimireddy et al. 2019): stochastic int8 / int4 codes with one fp32 scale per
// 256 coordinates, and the dequantising combine of W clients' uploads.
//
// quantize_delta: local, global, residual [n] fp32, 1 <= n < 2^31, bits in {8, 4}, Q = 2^(bits-1) - 1
// -> codes uint8 [ceil(n bits / 8)], scales fp32 [ceil(n / 256)], residual updated in place.  The
// contract (ops/reference.py quantize_delta is the same form in torch):
//   a[i]     = (local[i] - global[i]) + residual[i]          one fp32 subtraction, one fp32 addition
//   amax_key = max over the block [256 b, min(n, 256 b + 256)) of bits(a[i]) & 0x7fffffff (an integer
//              maximum: order cannot show); amax is the float with those bits
//   amax_key >= 0x7f800000 (an inf or a NaN in the block): scale = the canonical NaN 0x7fc00000, codes
//              0, residual +0.0 over the block -- nothing of it comes back next round
//   s = amax / Q (one IEEE division); s < 2^-126 (an all-zero block, or a quotient that is no normal
//              number): scale = +0.0, codes 0, residual[i] = a[i]
//   else     x = a[i] / s; f = floor(x); p = x - f (exact); word = component i & 3 of
//              philox4x32(seed, offset, i >> 2); up = float(word >> 8) < p * 2^24 (both sides exact);
//              q = clamp(f + up, -Q, Q); residual[i] = a[i] - float(q) * s (product and difference
//              rounded separately)
//   The clamp is part of the contract: fl(amax / fl(amax / Q)) exceeds Q for about one mantissa in
//   eight (up to 127.0000076 / 7.0000005), and the block maximum's own code would then reach Q + 1
//   with probability 2^-17 and wrap in its byte or nibble.
//   8 bits: byte i is q as int8.  4 bits: byte j holds coordinate 2 j in its low nibble and 2 j + 1 in
//   its high nibble, 4-bit two's complement, the padding nibble of an odd n zero.
// Every output bit is a function of the block's own inputs, seed and offset: grid and launch order
// cannot show.
//
// Layout: a lane owns 16 consecutive coordinates (four 16-byte loads from each input), 16 lanes one
// scale block, a wave 1024 coordinates per iteration.  The block maximum is an integer max over the
// lane's 16 keys and four cross-lane steps inside the 16-lane group; no LDS, no atomics.  The lane
// quantises in registers (four Philox calls) and stores 16 bytes of codes (8 at 4 bits), four 16-byte
// lines of residual, and lane 0 of the group the scale: each input is read once (12 n bytes), 4 n +
// n bits / 8 + n / 64 bytes are written.  Scale block b starts at coordinate 256 b of the tensor
// whatever its address; a ragged last block, and every block when a pointer is not 16-byte aligned (a
// view such as x[1:]), loads and stores element by element with the same arithmetic in between.
//
// dequant_combine: base [n], codes [W, nbytes], scales [W, nb], weights [W] -> out [n]:  acc = +0.0;
// for c = 0 .. W-1 in order acc[i] += weights[c] * (float(q[c, i]) * scales[c, i / 256]) (three
// roundings); out = base + acc / wsum, wsum the sequential fp32 sum of the weights from +0.0.  The same
// lane layout; per client a lane loads its 16 bytes of codes (8 at 4 bits) and the block's scale, and
// the loads of client c + 1 are issued before the adds of client c.  Codes are taken as they decode
// (-128 and -8 included) and the kernel reads only inside [0, nbytes) and [0, nb) of each row, so any
// content is memory-safe.  It reads W (n bits / 8 + n / 64) + 4 n bytes and writes 4 n.
#include "common.h"
#include "launchers.h"

// every product, sum and difference below is rounded on its own, whatever flags build this file (plain
// operators under this pragma, as in sparse_delta.hip: the __f*_rn helpers were fused after inlining)
#pragma clang fp contract(off)

namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

constexpr int BLOCK = 256;
constexpr uint32_t LANE_SPAN = 16;    // coordinates per lane
constexpr uint32_t GROUP = 256;       // coordinates per scale block: 16 lanes
constexpr uint32_t WAVE_SPAN = 1024;  // coordinates per wave and iteration: 4 scale blocks

// 16 consecutive floats of p from coordinate i0: 16-byte loads when fast, else guarded by i < n (0.0 past n)
__device__ __forceinline__ void load16(const float* __restrict__ p, uint32_t i0, uint32_t n, bool fast, float (&x)[16]) {
  if (fast) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(p + i0 + 4 * j);
#pragma unroll
      for (int e = 0; e < 4; ++e) x[4 * j + e] = v[e];
    }
  } else {
#pragma unroll
    for (int e = 0; e < 16; ++e) x[e] = i0 + e < n ? p[i0 + e] : 0.f;
  }
}

__device__ __forceinline__ void store16(float* __restrict__ p, uint32_t i0, uint32_t n, bool fast, const float (&x)[16]) {
  if (fast) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      *reinterpret_cast<f32x4*>(p + i0 + 4 * j) = f32x4{x[4 * j], x[4 * j + 1], x[4 * j + 2], x[4 * j + 3]};
  } else {
#pragma unroll
    for (int e = 0; e < 16; ++e)
      if (i0 + e < n) p[i0 + e] = x[e];
  }
}

template <int BITS>
__global__ __launch_bounds__(BLOCK) void quantize_kernel(const float* __restrict__ local, const float* __restrict__ global,
                                                        float* __restrict__ residual, uint8_t* __restrict__ codes,
                                                        float* __restrict__ scales, uint32_t n, uint64_t seed,
                                                        uint64_t offset, int vec) {
  constexpr float Q = (float)((1 << (BITS - 1)) - 1);
  const uint32_t ntiles = (n + WAVE_SPAN - 1) / WAVE_SPAN;
  const uint32_t wave = blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6), nwaves = gridDim.x * (BLOCK / 64);
  const int lane = lane_id();
  for (uint32_t tile = wave; tile < ntiles; tile += nwaves) {  // (wave-uniform trip count: every lane shuffles)
    const uint32_t b0 = tile * WAVE_SPAN + (uint32_t)(lane >> 4) * GROUP;  // the scale block's first coordinate
    const uint32_t i0 = b0 + (uint32_t)(lane & 15) * LANE_SPAN;
    const bool fast = vec && b0 + GROUP <= n;
    float a[16];
    {
      float l[16], g[16], r[16];
      load16(local, i0, n, fast, l);
      load16(global, i0, n, fast, g);
      load16(residual, i0, n, fast, r);
#pragma unroll
      for (int e = 0; e < 16; ++e) a[e] = (l[e] - g[e]) + r[e];
    }
    uint32_t key = 0;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const uint32_t k = __float_as_uint(a[e]) & 0x7FFFFFFFu;
      key = k > key ? k : key;
    }
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {
      const uint32_t k = (uint32_t)__shfl_xor((int)key, o, 64);
      key = k > key ? k : key;
    }
    const bool nonfinite = key >= 0x7F800000u;
    const float s = __uint_as_float(key) / Q;
    const bool live = !nonfinite && s >= 0x1p-126f;
    const float sd = live ? s : 1.f;
    int q[16];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint4 w4 = Philox::gen(seed, offset, (uint64_t)((i0 >> 2) + j));
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float ae = a[4 * j + e];
        const float x = ae / sd;
        const float f = floorf(x);
        const float p = x - f;
        const bool up = (float)(u4_get(w4, e) >> 8) < p * 16777216.0f;
        float qf = f + (up ? 1.f : 0.f);
        qf = fminf(fmaxf(qf, -Q), Q);
        const float d = qf * s;
        const float r = ae - d;
        q[4 * j + e] = live ? (int)qf : 0;
        a[4 * j + e] = live ? r : (nonfinite ? 0.f : ae);
      }
    }
    store16(residual, i0, n, fast, a);
    if ((lane & 15) == 0 && b0 < n) scales[b0 / GROUP] = nonfinite ? __uint_as_float(0x7FC00000u) : (live ? s : 0.f);
    if (BITS == 8) {
      if (fast) {
        u32x4 w;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          w[j] = (uint32_t)(q[4 * j] & 0xFF) | (uint32_t)(q[4 * j + 1] & 0xFF) << 8 | (uint32_t)(q[4 * j + 2] & 0xFF) << 16 |
                 (uint32_t)(q[4 * j + 3] & 0xFF) << 24;
        *reinterpret_cast<u32x4*>(codes + i0) = w;
      } else {
#pragma unroll
        for (int e = 0; e < 16; ++e)
          if (i0 + e < n) codes[i0 + e] = (uint8_t)(q[e] & 0xFF);
      }
    } else {
      // (a coordinate past n has a = 0 in a block that is live or zero: its nibble is 0)
      if (fast) {
        u32x2 w = {0u, 0u};
#pragma unroll
        for (int e = 0; e < 16; ++e) w[e >> 3] |= (uint32_t)(q[e] & 0xF) << (4 * (e & 7));
        *reinterpret_cast<u32x2*>(codes + (i0 >> 1)) = w;
      } else {
#pragma unroll
        for (int e = 0; e < 16; e += 2)
          if (i0 + e < n) codes[(i0 + e) >> 1] = (uint8_t)((q[e] & 0xF) | (i0 + e + 1 < n ? (q[e + 1] & 0xF) << 4 : 0));
      }
    }
  }
}

// one client's codes of a lane's 16 coordinates: 16 bytes at 8 bits, 8 at 4
template <int BITS>
struct Codes {
  uint32_t w[BITS == 8 ? 4 : 2];
};

// row: one client's code bytes; reads [i0 bits / 8, +16 bits / 8) when fast (any alignment), else the
// bytes of the coordinates below n
template <int BITS>
__device__ __forceinline__ Codes<BITS> load_codes(const uint8_t* __restrict__ row, uint32_t i0, uint32_t n, bool fast) {
  Codes<BITS> c;
  constexpr int NBYTES = BITS == 8 ? 16 : 8;
  const uint32_t j0 = BITS == 8 ? i0 : i0 >> 1;
  if (fast) {
    __builtin_memcpy(c.w, row + j0, NBYTES);
  } else {
    const uint32_t nbytes = BITS == 8 ? n : (n + 1) >> 1;
#pragma unroll
    for (int k = 0; k < NBYTES / 4; ++k) c.w[k] = 0u;
#pragma unroll
    for (int k = 0; k < NBYTES; ++k)
      if (j0 + k < nbytes) c.w[k >> 2] |= (uint32_t)row[j0 + k] << (8 * (k & 3));
  }
  return c;
}

template <int BITS>
__device__ __forceinline__ float code_at(const Codes<BITS>& c, int e) {
  if (BITS == 8) return (float)((int)(c.w[e >> 2] << (24 - 8 * (e & 3))) >> 24);
  return (float)((int)(c.w[e >> 3] << (28 - 4 * (e & 7))) >> 28);
}

template <int BITS>
__global__ __launch_bounds__(BLOCK) void dequant_combine_kernel(const float* __restrict__ base,
                                                               const uint8_t* __restrict__ codes,
                                                               const float* __restrict__ scales,
                                                               const float* __restrict__ wts, float* __restrict__ out,
                                                               int W, uint32_t n, int vec) {
  const uint32_t ntiles = (n + WAVE_SPAN - 1) / WAVE_SPAN;
  const uint32_t wave = blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6), nwaves = gridDim.x * (BLOCK / 64);
  const int lane = lane_id();
  const size_t nbytes = BITS == 8 ? (size_t)n : ((size_t)n + 1) >> 1;
  const size_t nb = ((size_t)n + GROUP - 1) / GROUP;
  for (uint32_t tile = wave; tile < ntiles; tile += nwaves) {
    const uint32_t b0 = tile * WAVE_SPAN + (uint32_t)(lane >> 4) * GROUP;
    const uint32_t i0 = b0 + (uint32_t)(lane & 15) * LANE_SPAN;
    if (i0 >= n) continue;  // (no cross-lane step in this kernel)
    const bool fast = b0 + GROUP <= n;
    const uint32_t blk = b0 / GROUP;
    float acc[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    float ws = 0.f;
    Codes<BITS> cur = load_codes<BITS>(codes, i0, n, fast);
    float sc = scales[blk];
    for (int c = 0; c < W; ++c) {
      Codes<BITS> nxt = cur;
      float sn = sc;
      if (c + 1 < W) {  // issued before this client's adds
        nxt = load_codes<BITS>(codes + (size_t)(c + 1) * nbytes, i0, n, fast);
        sn = scales[(size_t)(c + 1) * nb + blk];
      }
      const float w = wts[c];
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[e] = acc[e] + w * (code_at<BITS>(cur, e) * sc);
      ws = ws + w;
      cur = nxt;
      sc = sn;
    }
    float o[16];
    load16(base, i0, n, fast && vec, o);
#pragma unroll
    for (int e = 0; e < 16; ++e) o[e] = o[e] + acc[e] / ws;
    store16(out, i0, n, fast && vec, o);
  }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

inline unsigned grid_for(long n) {
  const long tiles = (n + WAVE_SPAN - 1) / WAVE_SPAN, need = (tiles + BLOCK / 64 - 1) / (BLOCK / 64);
  const long cap = (long)fr_num_cus() * 8;
  return (unsigned)(need < cap ? need : cap);
}

}  // namespace

// 1: a shape outside 1 <= n < 2^31 or bits outside {8, 4}; 2: a float pointer that is not 4-byte aligned;
// 3: a runtime error
extern "C" int fr_quantize_delta(const float* local, const float* global, float* residual, unsigned char* codes,
                                 float* scales, long n, int bits, unsigned long long seed, unsigned long long offset,
                                 hipStream_t s) {
  if (n < 1 || n >= (1L << 31) || (bits != 8 && bits != 4)) return 1;
  if (((uintptr_t)local | (uintptr_t)global | (uintptr_t)residual | (uintptr_t)scales) & 3u) return 2;
  const int vec = aligned16(local) && aligned16(global) && aligned16(residual) && aligned16(codes);
  const dim3 grid(grid_for(n)), blk(BLOCK);
  if (bits == 8)
    hipLaunchKernelGGL(quantize_kernel<8>, grid, blk, 0, s, local, global, residual, codes, scales, (uint32_t)n,
                       (uint64_t)seed, (uint64_t)offset, vec);
  else
    hipLaunchKernelGGL(quantize_kernel<4>, grid, blk, 0, s, local, global, residual, codes, scales, (uint32_t)n,
                       (uint64_t)seed, (uint64_t)offset, vec);
  return hipGetLastError() == hipSuccess ? 0 : 3;
}

// codes [W, ceil(n bits / 8)], scales [W, ceil(n / 256)].  1: a shape outside 1 <= W <= 65536, 1 <= n < 2^31 or
// bits outside {8, 4}; 2: a float pointer that is not 4-byte aligned; 3: a runtime error
extern "C" int fr_dequant_combine(const float* base, const unsigned char* codes, const float* scales,
                                  const float* weights, float* out, int W, long n, int bits, hipStream_t s) {
  if (W < 1 || W > 65536 || n < 1 || n >= (1L << 31) || (bits != 8 && bits != 4)) return 1;
  if (((uintptr_t)base | (uintptr_t)scales | (uintptr_t)weights | (uintptr_t)out) & 3u) return 2;
  const int vec = aligned16(base) && aligned16(out);
  const dim3 grid(grid_for(n)), blk(BLOCK);
  if (bits == 8)
    hipLaunchKernelGGL(dequant_combine_kernel<8>, grid, blk, 0, s, base, codes, scales, weights, out, W, (uint32_t)n, vec);
  else
    hipLaunchKernelGGL(dequant_combine_kernel<4>, grid, blk, 0, s, base, codes, scales, weights, out, W, (uint32_t)n, vec);
  return hipGetLastError() == hipSuccess ? 0 : 3;
}
