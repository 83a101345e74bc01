// The block quantiser on a lane's registers, shared by quant_delta.hip and rotate_delta.hip: a lane owns 16
// consecutive coordinates, 16 lanes one scale block of 256.  The contract is the header of quant_delta.hip.  The lane
// moves (load16 / store16 / lane_xor) also serve the scaled-sign coder of sign_block.h.
#pragma once
#include "common.h"

// every product, sum and difference below, and in the file that includes this one, is rounded on its own, whatever
// flags build it (plain operators under this pragma, as in sparse_delta.hip: the __f*_rn helpers were fused after inlining)
#pragma clang fp contract(off)

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

constexpr uint32_t QB_GROUP = 256;  // coordinates per scale block: 16 lanes

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

// DPP controls (quad_perm [a,b,c,d] = a | b << 2 | c << 4 | d << 6)
constexpr int DPP_XOR1 = 0xB1;         // quad_perm [1,0,3,2]
constexpr int DPP_XOR2 = 0x4E;         // quad_perm [2,3,0,1]
constexpr int DPP_XOR3 = 0x1B;         // quad_perm [3,2,1,0]
constexpr int DPP_HALF_MIRROR = 0x141; // row_half_mirror: lane ^ 7 within 8
constexpr int DPP_ROR8 = 0x128;        // row_ror:8: lane ^ 8 within 16

template <int CTRL>
__device__ __forceinline__ float dpp(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}

// the value of lane ^ M, M in {1, 2, 4, 8}
template <int M>
__device__ __forceinline__ float lane_xor(float v) {
  if (M == 1) return dpp<DPP_XOR1>(v);
  if (M == 2) return dpp<DPP_XOR2>(v);
  if (M == 4) return dpp<DPP_HALF_MIRROR>(dpp<DPP_XOR3>(v));
  return dpp<DPP_ROR8>(v);
}

// a[16]: the lane's values at coordinates i0 .. i0 + 15 of the scale block that starts at b0 (0.0 past n).  The block
// maximum (an integer max over the 16-lane group: every lane of the wave calls this), the scale, the codes and the
// residual of quant_delta.hip's contract; stores them (fast: 16-byte lines, else guarded by i < n)
template <int BITS>
__device__ __forceinline__ void quantize_store16(float (&a)[16], uint32_t i0, uint32_t b0, uint32_t n, bool fast, int lane,
                                                 uint64_t seed, uint64_t offset, float* __restrict__ residual,
                                                 uint8_t* __restrict__ codes, float* __restrict__ scales) {
  constexpr float Q = (float)((1 << (BITS - 1)) - 1);
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
  if ((lane & 15) == 0 && b0 < n) scales[b0 / QB_GROUP] = nonfinite ? __uint_as_float(0x7FC00000u) : (live ? s : 0.f);
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

// acc[16] = the sequential sum over W clients of weights[c] * (float(q[c]) * scale[c]) from +0.0 (three roundings per
// client), ws the weights' sum: dequant_combine's arithmetic on the lane's 16 coordinates.  The loads of client c + 1
// are issued before the adds of client c.  nbytes, nb: the row strides of codes and scales
template <int BITS>
__device__ __forceinline__ void decode_sum16(const uint8_t* __restrict__ codes, const float* __restrict__ scales,
                                             const float* __restrict__ wts, int W, size_t nbytes, size_t nb, uint32_t i0,
                                             uint32_t blk, uint32_t n, bool fast, float (&acc)[16], float& ws) {
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
  ws = 0.f;
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
}
