// Pieces of the transposed-read TN MFMA pipelines (gemm_wgrad.hip, text_head.hip): row-major
// tiles staged by glds with their 16-B chunks swizzled, fragments read back column-major with
// ds_read_b64_tr_b16 (gemm_wgrad.hip's header has the layout).  Each file keeps its own zero
// row: a __device__ array shared from a header would be one symbol per translation unit anyway.
#pragma once
#include "common.h"

// bank-conflict swizzle: 16-B chunk c of row r is stored at chunk c ^ swz(r)
static __device__ __forceinline__ int swz(int row) { return ((row & 3) | (((row >> 3) & 1) << 2)) << 1; }

// LDS byte offset (rows of `pitch` bytes) of this lane's 8 bytes for a transposed read of rows
// r0 + q (q = 0..3), columns col0 + 4p .. +3 (lane 4q+p of its 16-lane group)
static __device__ __forceinline__ uint32_t tr_off(int pitch, int r0, int col0, int q, int p) {
  const int c = (col0 >> 3) + (p >> 1);
  const int r = r0 + q;
  return (uint32_t)(r * pitch + ((c ^ swz(r)) << 4) + (p & 1) * 8);
}

// ds_read_b64_tr_b16 as opaque asm: a plain (builtin) LDS read after a glds into the same LDS
// object makes the compiler drain vmcnt first -- every in-flight stage -- which serialises the
// pipeline.  The reads' completion is then ours to wait for (LGKM_TIE8 and its kin).
static __device__ __forceinline__ s16x4 tr_read(uint32_t addr) {
  s16x4 v;
  asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(v) : "v"(addr));
  return v;
}

// a fragment = two ds_read_b64_tr_b16 four rows apart: the second at an immediate offset.
// `a` is early-clobber: the first read's destination must not be the address register the
// second read still needs (the return can land before a queued second read issues).
template <int OFF>
static __device__ __forceinline__ void tr_read2(uint32_t addr, s16x4& a, s16x4& b) {
  asm volatile("ds_read_b64_tr_b16 %0, %2\n\tds_read_b64_tr_b16 %1, %2 offset:%3"
               : "=&v"(a), "=v"(b)
               : "v"(addr), "n"(OFF));
}

#define LGKM_TIE8(r)                                                                                  \
  asm volatile("s_waitcnt lgkmcnt(0)"                                                                 \
               : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]), "+v"(r[4]), "+v"(r[5]), "+v"(r[6]), \
                 "+v"(r[7]))

static __device__ __forceinline__ bf16x8 join(s16x4 a, s16x4 b) {
  bf16x4 x = __builtin_bit_cast(bf16x4, a), y = __builtin_bit_cast(bf16x4, b);
  return bf16x8{x[0], x[1], x[2], x[3], y[0], y[1], y[2], y[3]};
}

// XCD-aware block order (bijective blockIdx remap): consecutive logical blocks -- the tiles
// that share a row panel -- run on one XCD's L2 (blocks go round-robin over the 8 XCDs)
static __device__ __forceinline__ int xcd_block(int bid, int nwg) {
  const int xcd = bid & 7, qq = nwg >> 3, rmd = nwg & 7;
  return (xcd < rmd ? xcd * (qq + 1) : rmd * (qq + 1) + (xcd - rmd) * qq) + (bid >> 3);
}
