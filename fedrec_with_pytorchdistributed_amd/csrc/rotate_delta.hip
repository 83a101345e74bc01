// Randomized-Hadamard rotation in front of the block quantiser (Konecny et al. 2016; Suresh, Yu, Kumar, McMahan 2017;
// DRIVE / EDEN, Vargaftik et al. 2021/22): R = 2^-6 H D over chunks of L = 4096 = 2^12 consecutive coordinates, H the
// Sylvester Hadamard matrix, D random signs.  R is orthonormal, so the quantiser's step follows a chunk's norm and
// not its maximum, and a combine may average rotated uploads and rotate back once.
//
// The contract (ops/reference.py rotate / rotate_quantize / rotate_combine are the same forms in torch), n_pad =
// 4096 ceil(n / 4096), the last chunk padded with +0.0:
//   d[i]   = bit 31 of component i & 3 of philox4x32(seed, 2^62, i >> 2): the sign of coordinate i (set: flip), the
//            same on every client and in every round; 2^62 is no (client << 32) | round of the quantiser's stream
//   rotate forward: t = d (.) x (a flip of the sign bit), then stages s = 0 .. 11 in that order: for every pair
//            (p, p | 2^s) with bit s of p clear (u, v) -> (u + v, u - v), one fp32 rounding each, no FMA, no
//            reassociation; then one multiplication by 2^-6.  Inverse: the same stages and scale, then the flip
//            (H is symmetric, H H = L I).  NaN payloads are outside the contract
//   quantize: z = rotate(local - global) (one fp32 subtraction) over n_pad coordinates, then quant_delta.hip's
//            contract on a = z + residual_rot: codes [n_pad bits / 8], scales [n_pad / 256], residual_rot [n_pad]
//            updated in place.  An inf or a NaN anywhere in a chunk reaches all 4096 rotated coordinates, so all 16
//            scale blocks of that chunk are declared non-finite (NaN scale, zero codes, +0.0 residual); the other
//            chunks are untouched
//   combine: per rotated coordinate acc = +0.0; acc += w_c * (float(q_c) * s_c) for c = 0 .. W-1 in order; m = acc /
//            wsum (dequant_combine's three roundings per client); out[i] = base[i] + rotate(m, inverse)[i], i < n
//
// Layout: one 256-thread workgroup owns one chunk, thread t the 16 consecutive coordinates 16 t .. 16 t + 15 (four
// 16-byte loads per input) -- quant_delta.hip's lane layout, so 16 lanes are one scale block and the quantiser of
// quant_block.h runs on the registers as the transform leaves them: z never reaches memory.  Coordinate bits:
//   0-3   four butterfly stages inside the lane's 16 registers
//   4-7   lane bits 0-3, one DPP move per register and stage: quad_perm for xor 1 and 2, row_ror:8 for xor 8, and for
//         xor 4 quad_perm [3,2,1,0] then row_half_mirror (xor 3 then xor 7: two moves, no LDS pipe, no wait count;
//         ds_swizzle_b32 and ds_bpermute_b32 would each be one lgkm round trip).  The lane whose bit is clear keeps
//         own + partner, the other partner - own: one xor of the sign bit under the lane's mask and one addition
//   8-9   lane bits 4-5 with v_permlane16_swap_b32 / v_permlane32_swap_b32 on register pairs: the swap of (a, b)
//         puts a's two halves side by side in one register and b's in the other, a plain add and subtract are the
//         butterflies of both, and a second swap puts them back -- one swap and one VALU op per register and stage
//   10-11 the wave index: each wave writes its 1024 values to LDS (16 KB), one barrier, each thread reads its three
//         partners' and forms stage 10 (xor-wave 1) of itself and of its xor-wave-2 partner, then stage 11.  Slot
//         (j, t) of 16 bytes sits at 16 (256 j + t): consecutive lanes, consecutive 16-byte slots, no bank conflict
// No atomics, no scratch, no inline asm.  The grid is one workgroup per chunk (n_pad < 2^31: fewer than 2^19).  A ragged
// tail chunk, and every chunk when a pointer is not 16-byte aligned (a view such as x[1:]), loads and stores element
// by element with the same arithmetic in between.  quantize reads 8 n + 4 n_pad bytes and writes 4 n_pad + n_pad
// bits / 8 + n_pad / 64; combine reads W (n_pad bits / 8 + n_pad / 64) + 4 n and writes 4 n.
//
// rotate_sign_quantize / rotate_sign_combine are the same two fused kernels with the scaled-sign coder of sign_delta.hip
// (sign_block.h) in place of the quantiser, one bit per rotated coordinate: DRIVE.  The rotation is what makes one bit
// work on a heavy-tailed delta, where the mean magnitude of a block is far below its rms.
#include "launchers.h"
#include "quant_block.h"  // load16 / store16 / lane_xor / quantize_store16 / decode_sum16; fp contract(off) from here on
#include "sign_block.h"   // sign_store16 / sign_decode_sum16: the 1-bit coder of sign_delta.hip on the same registers

namespace {

constexpr int BLOCK = 256;
constexpr uint32_t CHUNK = 4096;
constexpr uint64_t SIGN_STREAM = 1ull << 62;

// one stage across lane bit M: own + partner where the bit is clear, partner - own (= partner + (-own), exact) where set
template <int M>
__device__ __forceinline__ void stage_dpp(float (&x)[16], int lane) {
  const uint32_t neg = (lane & M) ? 0x80000000u : 0u;
#pragma unroll
  for (int e = 0; e < 16; ++e) x[e] = lane_xor<M>(x[e]) + __uint_as_float(__float_as_uint(x[e]) ^ neg);
}

// one stage across lane bit 4 (ROW16) or 5.  swap(a, b) exchanges the upper half of a with the lower half of b: a' =
// (a lo, b lo), b' = (a hi, b hi).  a' + b' holds a's sum in the lower lanes and b's in the upper, a' - b' the
// differences alike, and the same swap of (sum, difference) returns (new a, new b)
template <bool ROW16>
__device__ __forceinline__ void stage_swap(float (&x)[16]) {
#pragma unroll
  for (int e = 0; e < 16; e += 2) {
    auto r = ROW16 ? __builtin_amdgcn_permlane16_swap(__float_as_uint(x[e]), __float_as_uint(x[e + 1]), false, false)
                   : __builtin_amdgcn_permlane32_swap(__float_as_uint(x[e]), __float_as_uint(x[e + 1]), false, false);
    const float a = __uint_as_float(r[0]), b = __uint_as_float(r[1]);
    const float sum = a + b, dif = a - b;
    r = ROW16 ? __builtin_amdgcn_permlane16_swap(__float_as_uint(sum), __float_as_uint(dif), false, false)
              : __builtin_amdgcn_permlane32_swap(__float_as_uint(sum), __float_as_uint(dif), false, false);
    x[e] = __uint_as_float(r[0]);
    x[e + 1] = __uint_as_float(r[1]);
  }
}

// the twelve stages and the scale over the workgroup's chunk; x: the thread's 16 coordinates; xch: 4096 floats of LDS.
// Every thread of the workgroup calls it (one barrier in front of the writes -- a caller may run it again -- and one behind)
__device__ __forceinline__ void fwht_chunk(float (&x)[16], float* __restrict__ xch) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
#pragma unroll
  for (int s = 0; s < 4; ++s)
#pragma unroll
    for (int e = 0; e < 16; ++e)
      if (!(e & (1 << s))) {
        const float u = x[e], v = x[e | (1 << s)];
        x[e] = u + v;
        x[e | (1 << s)] = u - v;
      }
  stage_dpp<1>(x, lane);
  stage_dpp<2>(x, lane);
  stage_dpp<4>(x, lane);
  stage_dpp<8>(x, lane);
  stage_swap<true>(x);
  stage_swap<false>(x);
  f32x4* slots = reinterpret_cast<f32x4*>(xch);
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 4; ++j) slots[256 * j + t] = f32x4{x[4 * j], x[4 * j + 1], x[4 * j + 2], x[4 * j + 3]};
  __syncthreads();
  const bool hi10 = wave & 1, hi11 = wave & 2;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const f32x4 p1 = slots[256 * j + (t ^ 64)], p2 = slots[256 * j + (t ^ 128)], p3 = slots[256 * j + (t ^ 192)];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float own = x[4 * j + e];
      const float y = hi10 ? p1[e] - own : own + p1[e];       // stage 10 of this wave
      const float yp = hi10 ? p3[e] - p2[e] : p2[e] + p3[e];  // stage 10 of the xor-wave-2 partner
      const float z = hi11 ? yp - y : y + yp;                 // stage 11
      x[4 * j + e] = z * 0x1p-6f;
    }
  }
}

// d (.) x over the thread's 16 coordinates from i0 (a multiple of 16)
__device__ __forceinline__ void flip_signs(float (&x)[16], uint32_t i0, uint64_t seed) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint4 w4 = Philox::gen(seed, SIGN_STREAM, (uint64_t)((i0 >> 2) + j));
#pragma unroll
    for (int e = 0; e < 4; ++e)
      x[4 * j + e] = __uint_as_float(__float_as_uint(x[4 * j + e]) ^ (u4_get(w4, e) & 0x80000000u));
  }
}

// x [n_in] (0.0 past it) -> out [n_out]; forward: n_in = n, n_out = n_pad; inverse: n_in = n_pad, n_out = n
template <bool INVERSE>
__global__ __launch_bounds__(BLOCK) void rotate_kernel(const float* __restrict__ x, float* __restrict__ out, uint32_t n_in,
                                                      uint32_t n_out, uint64_t seed, int vec) {
  __shared__ __attribute__((aligned(16))) float xch[CHUNK];
  const uint32_t i0 = blockIdx.x * CHUNK + threadIdx.x * 16u;
  float a[16];
  load16(x, i0, n_in, vec && i0 + 16 <= n_in, a);
  if (!INVERSE) flip_signs(a, i0, seed);
  fwht_chunk(a, xch);
  if (INVERSE) flip_signs(a, i0, seed);
  store16(out, i0, n_out, vec && i0 + 16 <= n_out, a);
}

// residual, codes, scales over n_pad (whole chunks); vec_in: local and global 16-byte aligned; vec_out: residual and codes
template <int BITS>
__global__ __launch_bounds__(BLOCK) void rotate_quantize_kernel(const float* __restrict__ local,
                                                               const float* __restrict__ global,
                                                               float* __restrict__ residual, uint8_t* __restrict__ codes,
                                                               float* __restrict__ scales, uint32_t n, uint32_t n_pad,
                                                               uint64_t seed, uint64_t offset, int vec_in, int vec_out) {
  __shared__ __attribute__((aligned(16))) float xch[CHUNK];
  const int lane = lane_id();
  const uint32_t i0 = blockIdx.x * CHUNK + threadIdx.x * 16u;
  const uint32_t b0 = i0 & ~(QB_GROUP - 1);  // the scale block's first coordinate
  float a[16];
  {
    float l[16], g[16];
    const bool fast = vec_in && i0 + 16 <= n;
    load16(local, i0, n, fast, l);
    load16(global, i0, n, fast, g);
#pragma unroll
    for (int e = 0; e < 16; ++e) a[e] = l[e] - g[e];
  }
  flip_signs(a, i0, seed);
  fwht_chunk(a, xch);
  {
    float r[16];
    load16(residual, i0, n_pad, vec_out, r);
#pragma unroll
    for (int e = 0; e < 16; ++e) a[e] = a[e] + r[e];
  }
  quantize_store16<BITS>(a, i0, b0, n_pad, vec_out, lane, seed, offset, residual, codes, scales);
}

// codes [W, n_pad bits / 8], scales [W, n_pad / 256]; vec: base and out 16-byte aligned
template <int BITS>
__global__ __launch_bounds__(BLOCK) void rotate_combine_kernel(const float* __restrict__ base,
                                                              const uint8_t* __restrict__ codes,
                                                              const float* __restrict__ scales,
                                                              const float* __restrict__ wts, float* __restrict__ out, int W,
                                                              uint32_t n, uint32_t n_pad, uint64_t seed, int vec) {
  __shared__ __attribute__((aligned(16))) float xch[CHUNK];
  const uint32_t i0 = blockIdx.x * CHUNK + threadIdx.x * 16u;
  const size_t nbytes = BITS == 8 ? (size_t)n_pad : (size_t)n_pad >> 1;
  float m[16], ws;
  decode_sum16<BITS>(codes, scales, wts, W, nbytes, n_pad / QB_GROUP, i0, i0 / QB_GROUP, n_pad, true, m, ws);
#pragma unroll
  for (int e = 0; e < 16; ++e) m[e] = m[e] / ws;
  fwht_chunk(m, xch);
  flip_signs(m, i0, seed);
  if (i0 >= n) return;  // (behind the last barrier)
  const bool fast = vec && i0 + 16 <= n;
  float o[16];
  load16(base, i0, n, fast, o);
#pragma unroll
  for (int e = 0; e < 16; ++e) o[e] = o[e] + m[e];
  store16(out, i0, n, fast, o);
}

// rotate_quantize_kernel with the scaled-sign coder of sign_block.h behind the transform (DRIVE): sign_delta.hip's
// contract on a = z + residual over n_pad coordinates, every block full
__global__ __launch_bounds__(BLOCK) void rotate_sign_quantize_kernel(const float* __restrict__ local,
                                                                    const float* __restrict__ global,
                                                                    float* __restrict__ residual,
                                                                    uint8_t* __restrict__ codes, float* __restrict__ scales,
                                                                    uint32_t n, uint32_t n_pad, uint64_t seed, int vec_in,
                                                                    int vec_out) {
  __shared__ __attribute__((aligned(16))) float xch[CHUNK];
  const int lane = lane_id();
  const uint32_t i0 = blockIdx.x * CHUNK + threadIdx.x * 16u;
  const uint32_t b0 = i0 & ~(QB_GROUP - 1);
  float a[16];
  {
    float l[16], g[16];
    const bool fast = vec_in && i0 + 16 <= n;
    load16(local, i0, n, fast, l);
    load16(global, i0, n, fast, g);
#pragma unroll
    for (int e = 0; e < 16; ++e) a[e] = l[e] - g[e];
  }
  flip_signs(a, i0, seed);
  fwht_chunk(a, xch);
  {
    float r[16];
    load16(residual, i0, n_pad, vec_out, r);
#pragma unroll
    for (int e = 0; e < 16; ++e) a[e] = a[e] + r[e];
  }
  sign_store16(a, i0, b0, n_pad, vec_out, lane, residual, codes, scales);
}

// rotate_combine_kernel over sign codes: codes [W, n_pad / 8], scales [W, n_pad / 256]; vec: base and out 16-byte aligned
__global__ __launch_bounds__(BLOCK) void rotate_sign_combine_kernel(const float* __restrict__ base,
                                                                   const uint8_t* __restrict__ codes,
                                                                   const float* __restrict__ scales,
                                                                   const float* __restrict__ wts, float* __restrict__ out,
                                                                   int W, uint32_t n, uint32_t n_pad, uint64_t seed,
                                                                   int vec) {
  __shared__ __attribute__((aligned(16))) float xch[CHUNK];
  const uint32_t i0 = blockIdx.x * CHUNK + threadIdx.x * 16u;
  float m[16], ws;
  sign_decode_sum16(codes, scales, wts, W, (size_t)n_pad >> 3, n_pad / QB_GROUP, i0, i0 / QB_GROUP, n_pad, true, m, ws);
#pragma unroll
  for (int e = 0; e < 16; ++e) m[e] = m[e] / ws;
  fwht_chunk(m, xch);
  flip_signs(m, i0, seed);
  if (i0 >= n) return;  // (behind the last barrier)
  const bool fast = vec && i0 + 16 <= n;
  float o[16];
  load16(base, i0, n, fast, o);
#pragma unroll
  for (int e = 0; e < 16; ++e) o[e] = o[e] + m[e];
  store16(out, i0, n, fast, o);
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }
inline long pad_of(long n) { return (n + CHUNK - 1) / CHUNK * CHUNK; }
inline bool bad_n(long n) { return n < 1 || n > (1L << 31) - CHUNK; }  // n_pad < 2^31

}  // namespace

// forward: x [n] -> out [n_pad]; inverse: x [n_pad] -> out [n].  1: a shape outside 1 <= n <= 2^31 - 4096 (n_pad < 2^31); 2: a pointer that is
// not 4-byte aligned; 3: a runtime error
extern "C" int fr_rotate(const float* x, float* out, long n, int inverse, unsigned long long seed, hipStream_t s) {
  if (bad_n(n)) return 1;
  if (((uintptr_t)x | (uintptr_t)out) & 3u) return 2;
  const long n_pad = pad_of(n);
  const int vec = aligned16(x) && aligned16(out);
  const dim3 grid((unsigned)(n_pad / CHUNK)), blk(BLOCK);
  if (inverse)
    hipLaunchKernelGGL(rotate_kernel<true>, grid, blk, 0, s, x, out, (uint32_t)n_pad, (uint32_t)n, (uint64_t)seed, vec);
  else
    hipLaunchKernelGGL(rotate_kernel<false>, grid, blk, 0, s, x, out, (uint32_t)n, (uint32_t)n_pad, (uint64_t)seed, vec);
  return hipGetLastError() == hipSuccess ? 0 : 3;
}

// local, global [n]; residual [n_pad], codes [n_pad bits / 8], scales [n_pad / 256].  1: a shape outside 1 <= n <= 2^31 -
// 4096 or bits outside {8, 4}; 2: a float pointer that is not 4-byte aligned; 3: a runtime error
extern "C" int fr_rotate_quantize(const float* local, const float* global, float* residual, unsigned char* codes,
                                  float* scales, long n, int bits, unsigned long long seed, unsigned long long offset,
                                  hipStream_t s) {
  if (bad_n(n) || (bits != 8 && bits != 4)) return 1;
  if (((uintptr_t)local | (uintptr_t)global | (uintptr_t)residual | (uintptr_t)scales) & 3u) return 2;
  const long n_pad = pad_of(n);
  const int vec_in = aligned16(local) && aligned16(global), vec_out = aligned16(residual) && aligned16(codes);
  const dim3 grid((unsigned)(n_pad / CHUNK)), blk(BLOCK);
  if (bits == 8)
    hipLaunchKernelGGL(rotate_quantize_kernel<8>, grid, blk, 0, s, local, global, residual, codes, scales, (uint32_t)n,
                       (uint32_t)n_pad, (uint64_t)seed, (uint64_t)offset, vec_in, vec_out);
  else
    hipLaunchKernelGGL(rotate_quantize_kernel<4>, grid, blk, 0, s, local, global, residual, codes, scales, (uint32_t)n,
                       (uint32_t)n_pad, (uint64_t)seed, (uint64_t)offset, vec_in, vec_out);
  return hipGetLastError() == hipSuccess ? 0 : 3;
}

// base, out [n]; codes [W, n_pad bits / 8], scales [W, n_pad / 256].  1: a shape outside 1 <= W <= 65536, 1 <= n <= 2^31 -
// 4096 or bits outside {8, 4}; 2: a float pointer that is not 4-byte aligned; 3: a runtime error
extern "C" int fr_rotate_combine(const float* base, const unsigned char* codes, const float* scales, const float* weights,
                                 float* out, int W, long n, int bits, unsigned long long seed, hipStream_t s) {
  if (W < 1 || W > 65536 || bad_n(n) || (bits != 8 && bits != 4)) return 1;
  if (((uintptr_t)base | (uintptr_t)scales | (uintptr_t)weights | (uintptr_t)out) & 3u) return 2;
  const long n_pad = pad_of(n);
  const int vec = aligned16(base) && aligned16(out);
  const dim3 grid((unsigned)(n_pad / CHUNK)), blk(BLOCK);
  if (bits == 8)
    hipLaunchKernelGGL(rotate_combine_kernel<8>, grid, blk, 0, s, base, codes, scales, weights, out, W, (uint32_t)n,
                       (uint32_t)n_pad, (uint64_t)seed, vec);
  else
    hipLaunchKernelGGL(rotate_combine_kernel<4>, grid, blk, 0, s, base, codes, scales, weights, out, W, (uint32_t)n,
                       (uint32_t)n_pad, (uint64_t)seed, vec);
  return hipGetLastError() == hipSuccess ? 0 : 3;
}

// fr_rotate_quantize with the scaled-sign coder: codes [n_pad / 8].  1: a shape outside 1 <= n <= 2^31 - 4096; 2: a
// float pointer that is not 4-byte aligned; 3: a runtime error
extern "C" int fr_rotate_sign_quantize(const float* local, const float* global, float* residual, unsigned char* codes,
                                       float* scales, long n, unsigned long long seed, hipStream_t s) {
  if (bad_n(n)) return 1;
  if (((uintptr_t)local | (uintptr_t)global | (uintptr_t)residual | (uintptr_t)scales) & 3u) return 2;
  const long n_pad = pad_of(n);
  const int vec_in = aligned16(local) && aligned16(global), vec_out = aligned16(residual) && aligned16(codes);
  hipLaunchKernelGGL(rotate_sign_quantize_kernel, dim3((unsigned)(n_pad / CHUNK)), dim3(BLOCK), 0, s, local, global,
                     residual, codes, scales, (uint32_t)n, (uint32_t)n_pad, (uint64_t)seed, vec_in, vec_out);
  return hipGetLastError() == hipSuccess ? 0 : 3;
}

// fr_rotate_combine over sign codes: codes [W, n_pad / 8].  1: a shape outside 1 <= W <= 65536, 1 <= n <= 2^31 - 4096;
// 2: a float pointer that is not 4-byte aligned; 3: a runtime error
extern "C" int fr_rotate_sign_combine(const float* base, const unsigned char* codes, const float* scales,
                                      const float* weights, float* out, int W, long n, unsigned long long seed,
                                      hipStream_t s) {
  if (W < 1 || W > 65536 || bad_n(n)) return 1;
  if (((uintptr_t)base | (uintptr_t)scales | (uintptr_t)weights | (uintptr_t)out) & 3u) return 2;
  const long n_pad = pad_of(n);
  const int vec = aligned16(base) && aligned16(out);
  hipLaunchKernelGGL(rotate_sign_combine_kernel, dim3((unsigned)(n_pad / CHUNK)), dim3(BLOCK), 0, s, base, codes, scales,
                     weights, out, W, (uint32_t)n, (uint32_t)n_pad, (uint64_t)seed, vec);
  return hipGetLastError() == hipSuccess ? 0 : 3;
}
