// The scaled-sign coder on a lane's registers, shared by sign_delta.hip and rotate_delta.hip: quant_block.h's lane
// layout (a lane owns 16 consecutive coordinates, 16 lanes one scale block of 256), so it runs on fwht_chunk's
// registers as they are.  The contract is the header of sign_delta.hip.
#pragma once
#include "quant_block.h"  // load16 / store16 / lane_xor; fp contract(off) from here on

// the value of lane ^ 1 of an integer: the half-word of the lane's pair
__device__ __forceinline__ uint32_t pair_of(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, DPP_XOR1, 0xF, 0xF, false);
}

// a[16]: the lane's values at coordinates i0 .. i0 + 15 of the scale block that starts at b0 (+0.0 past n).  The
// block's magnitude (every lane of the wave calls this: four DPP steps inside the 16-lane group), its state, the
// lane's 16 sign bits and the residual; stores them.  fast: the whole block lies below n and residual and codes are
// 16-byte aligned -- four 16-byte lines of residual, and each lane pair one dword of codes (a wave: 128 contiguous
// bytes); else element by element and byte by byte, guarded by n
__device__ __forceinline__ void sign_store16(float (&a)[16], uint32_t i0, uint32_t b0, uint32_t n, bool fast, int lane,
                                             float* __restrict__ residual, uint8_t* __restrict__ codes,
                                             float* __restrict__ scales) {
  float p = 0.f;
#pragma unroll
  for (int e = 0; e < 16; ++e) p = p + __uint_as_float(__float_as_uint(a[e]) & 0x7FFFFFFFu);
  p = p + lane_xor<1>(p);
  p = p + lane_xor<2>(p);
  p = p + lane_xor<4>(p);
  p = p + lane_xor<8>(p);
  const uint32_t left = n - b0;  // (a block past n stores nothing: any divisor will do)
  const float s = p / (float)(left < QB_GROUP ? left : QB_GROUP);
  const bool nonfinite = (__float_as_uint(p) & 0x7FFFFFFFu) >= 0x7F800000u;
  const bool live = !nonfinite && s >= 0x1p-126f;
  const uint32_t sbits = __float_as_uint(s);
  uint32_t h = 0;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const uint32_t ab = __float_as_uint(a[e]);
    h |= (ab >> 31) << e;
    const float r = a[e] - __uint_as_float(sbits | (ab & 0x80000000u));  // a - copysign(s, a)
    a[e] = live ? r : (nonfinite ? 0.f : a[e]);
  }
  h = live ? h : 0u;
  const uint32_t hi = pair_of(h);  // (every lane: in front of the branches)
  store16(residual, i0, n, fast, a);
  if ((lane & 15) == 0 && b0 < n) scales[b0 / QB_GROUP] = nonfinite ? __uint_as_float(0x7FC00000u) : (live ? s : 0.f);
  if (fast) {
    if (!(lane & 1)) *reinterpret_cast<uint32_t*>(codes + (i0 >> 3)) = h | hi << 16;
  } else {
    // (a coordinate past n has a = +0.0: its bit is 0)
    if (i0 < n) codes[i0 >> 3] = (uint8_t)(h & 0xFF);
    if (i0 + 8 < n) codes[(i0 >> 3) + 1] = (uint8_t)(h >> 8);
  }
}

// one client's sign bits of a lane's 16 coordinates: row + i0 / 8 has any alignment (a row starts at c ceil(n / 8)
// bytes).  fast: both bytes lie inside the row; else the bytes of the coordinates below n
__device__ __forceinline__ uint32_t load_signs(const uint8_t* __restrict__ row, uint32_t i0, uint32_t n, bool fast) {
  const uint32_t j0 = i0 >> 3;
  if (fast) {
    uint16_t h;
    __builtin_memcpy(&h, row + j0, 2);
    return h;
  }
  uint32_t h = 0;
  if (i0 < n) h = row[j0];
  if (i0 + 8 < n) h |= (uint32_t)row[j0 + 1] << 8;
  return h;
}

// acc[16] = the sequential sum over W clients of +-t_c from +0.0, t_c = weights[c] * scale[c] (one rounding, once per
// client), the sign bit xor-ed in; ws the weights' sum: sign_combine's arithmetic on the lane's 16 coordinates.  The
// loads of client c + 1 are issued before the adds of client c.  nbytes, nb: the row strides of codes and scales
__device__ __forceinline__ void sign_decode_sum16(const uint8_t* __restrict__ codes, const float* __restrict__ scales,
                                                  const float* __restrict__ wts, int W, size_t nbytes, size_t nb,
                                                  uint32_t i0, uint32_t blk, uint32_t n, bool fast, float (&acc)[16],
                                                  float& ws) {
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
  ws = 0.f;
  uint32_t cur = load_signs(codes, i0, n, fast);
  float sc = scales[blk];
  for (int c = 0; c < W; ++c) {
    uint32_t nxt = cur;
    float sn = sc;
    if (c + 1 < W) {  // issued before this client's adds
      nxt = load_signs(codes + (size_t)(c + 1) * nbytes, i0, n, fast);
      sn = scales[(size_t)(c + 1) * nb + blk];
    }
    const float w = wts[c];
    const uint32_t t = __float_as_uint(w * sc);
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = acc[e] + __uint_as_float(t ^ ((cur >> e & 1u) << 31));
    ws = ws + w;
    cur = nxt;
    sc = sn;
  }
}
