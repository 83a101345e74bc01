// 1-bit scaled-sign uploads with error feedback (signSGD, Bernstein et al. 2018; EF-signSGD, Karimireddy et al. 2019;
// composed with top-k it is STC, Sattler et al. 2019, behind the rotation of rotate_delta.hip DRIVE, Vargaftik et al.
// 2021): one sign bit per coordinate and one fp32 magnitude per 256, n / 8 + n / 64 bytes instead of 4 n.  The sign
// with the block's mean magnitude is the L2-optimal 1-bit code of the block; it is deterministic (no Philox).
//
// sign_quantize: local, global, residual [n] fp32, 1 <= n < 2^31 -> codes uint8 [ceil(n / 8)], scales fp32 [ceil(n /
// 256)], residual updated in place.  The contract (ops/reference.py sign_quantize is the same form in torch):
//   a[i] = (local[i] - global[i]) + residual[i]             one fp32 subtraction, one fp32 addition
//   p    = the sum of |a| over the block [256 b, 256 b + 256), +0.0 past n, in this order: the block is 16 runs of 16
//          consecutive coordinates; each run is summed from +0.0 in ascending order; then four butterfly steps over
//          the 16 run sums, p_j = p_j + p_(j ^ o) for o = 1, 2, 4, 8 (additions commute: all 16 hold the same bits)
//   s    = p / float(min(256, n - 256 b))                    one IEEE division: the block's mean magnitude
//   bits(p) & 0x7fffffff >= 0x7f800000 (an inf or a NaN in the block, or a sum that overflows): scale = the
//          canonical NaN 0x7fc00000, codes 0, residual +0.0 over the block -- nothing of it comes back next round
//   s < 2^-126 (an all-zero block, or a mean that is no normal number): scale = +0.0, codes 0, residual[i] = a[i]
//   else bit i & 7 of byte i >> 3 is the sign bit of a[i] (-0.0 codes 1), residual[i] = a[i] - copysign(s, a[i])
//   The padding bits of the last byte are zero.
//
// Layout: quant_delta.hip's.  A lane owns 16 consecutive coordinates -- one run -- (four 16-byte loads from each
// input), 16 lanes one scale block, a wave 1024 coordinates per iteration.  The run sum is in the lane, the four
// butterfly steps are DPP moves inside the 16-lane row (lane_xor of quant_block.h); no LDS, no atomics.  The lane
// gathers its 16 sign bits into a half-word, lane pairs merge theirs with one more DPP move and the even lane stores
// a dword: a wave writes 128 contiguous bytes of codes, four 16-byte lines of residual per lane, and the first lane of
// each group the scale.  12 n bytes are read, 4 n + n / 8 + n / 64 written.  A ragged last block, and every block
// when a pointer is not 16-byte aligned (a view such as x[1:]), loads and stores element by element and byte by byte
// with the same arithmetic in between.
//
// sign_combine: base [n], codes [W, ceil(n / 8)], scales [W, ceil(n / 256)], weights [W] -> out [n]: acc = +0.0; for
// c = 0 .. W-1 in order t = weights[c] * scales[c, i / 256] (one rounding) and acc[i] += bit ? -t : t; out = base +
// acc / wsum, wsum the sequential fp32 sum of the weights from +0.0.  The same lane layout; per client a lane loads
// its half-word of codes (a row starts at c ceil(n / 8) bytes: any alignment) and the block's scale, forms t once and
// adds it 16 times with the sign bit xor-ed in; the loads of client c + 1 are issued before the adds of client c.  At
// W = 8 the codes are n bytes against 8 n for base and out: a wider code load would buy nothing.  The kernel reads only
// inside [0, nbytes) and [0, nb) of each row, so any content is memory-safe.
#include "launchers.h"
#include "sign_block.h"  // the coder on a lane's registers, shared with rotate_delta.hip; fp contract(off) from here on

namespace {

constexpr int BLOCK = 256;
constexpr uint32_t LANE_SPAN = 16;    // coordinates per lane
constexpr uint32_t GROUP = QB_GROUP;  // coordinates per scale block: 16 lanes
constexpr uint32_t WAVE_SPAN = 1024;  // coordinates per wave and iteration: 4 scale blocks

__global__ __launch_bounds__(BLOCK) void sign_quantize_kernel(const float* __restrict__ local,
                                                             const float* __restrict__ global,
                                                             float* __restrict__ residual, uint8_t* __restrict__ codes,
                                                             float* __restrict__ scales, uint32_t n, int vec) {
  const uint32_t ntiles = (n + WAVE_SPAN - 1) / WAVE_SPAN;
  const uint32_t wave = blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6), nwaves = gridDim.x * (BLOCK / 64);
  const int lane = lane_id();
  for (uint32_t tile = wave; tile < ntiles; tile += nwaves) {  // (wave-uniform trip count: every lane takes the DPP steps)
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
    sign_store16(a, i0, b0, n, fast, lane, residual, codes, scales);
  }
}

__global__ __launch_bounds__(BLOCK) void sign_combine_kernel(const float* __restrict__ base,
                                                            const uint8_t* __restrict__ codes,
                                                            const float* __restrict__ scales,
                                                            const float* __restrict__ wts, float* __restrict__ out, int W,
                                                            uint32_t n, int vec) {
  const uint32_t ntiles = (n + WAVE_SPAN - 1) / WAVE_SPAN;
  const uint32_t wave = blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6), nwaves = gridDim.x * (BLOCK / 64);
  const int lane = lane_id();
  const size_t nbytes = ((size_t)n + 7) >> 3;
  const size_t nb = ((size_t)n + GROUP - 1) / GROUP;
  for (uint32_t tile = wave; tile < ntiles; tile += nwaves) {
    const uint32_t b0 = tile * WAVE_SPAN + (uint32_t)(lane >> 4) * GROUP;
    const uint32_t i0 = b0 + (uint32_t)(lane & 15) * LANE_SPAN;
    if (i0 >= n) continue;  // (no cross-lane step in this kernel)
    const bool fast = b0 + GROUP <= n;
    float acc[16], ws;
    sign_decode_sum16(codes, scales, wts, W, nbytes, nb, i0, b0 / GROUP, n, fast, acc, ws);
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

// local, global, residual [n]; codes [ceil(n / 8)], scales [ceil(n / 256)].  1: a shape outside 1 <= n < 2^31; 2: a
// float pointer that is not 4-byte aligned; 3: a runtime error
extern "C" int fr_sign_quantize(const float* local, const float* global, float* residual, unsigned char* codes,
                                float* scales, long n, hipStream_t s) {
  if (n < 1 || n >= (1L << 31)) return 1;
  if (((uintptr_t)local | (uintptr_t)global | (uintptr_t)residual | (uintptr_t)scales) & 3u) return 2;
  const int vec = aligned16(local) && aligned16(global) && aligned16(residual) && aligned16(codes);
  hipLaunchKernelGGL(sign_quantize_kernel, dim3(grid_for(n)), dim3(BLOCK), 0, s, local, global, residual, codes, scales,
                     (uint32_t)n, vec);
  return hipGetLastError() == hipSuccess ? 0 : 3;
}

// base, out [n]; codes [W, ceil(n / 8)], scales [W, ceil(n / 256)].  1: a shape outside 1 <= W <= 65536, 1 <= n <
// 2^31; 2: a float pointer that is not 4-byte aligned; 3: a runtime error
extern "C" int fr_sign_combine(const float* base, const unsigned char* codes, const float* scales, const float* weights,
                               float* out, int W, long n, hipStream_t s) {
  if (W < 1 || W > 65536 || n < 1 || n >= (1L << 31)) return 1;
  if (((uintptr_t)base | (uintptr_t)scales | (uintptr_t)weights | (uintptr_t)out) & 3u) return 2;
  const int vec = aligned16(base) && aligned16(out);
  hipLaunchKernelGGL(sign_combine_kernel, dim3(grid_for(n)), dim3(BLOCK), 0, s, base, codes, scales, weights, out, W,
                     (uint32_t)n, vec);
  return hipGetLastError() == hipSuccess ? 0 : 3;
}
