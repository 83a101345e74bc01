// Diversity re-rank: Maximal Marginal Relevance over a candidate pool, one workgroup per user.
//
//   pool    ids [B, P] (slot j valid iff ids[b, j] >= 0; 0 <= id < N is trusted on valid slots), rel [B, P]
//   rhat_j  = (rel_j - rel_min) / (rel_max - rel_min) over the valid slots (1 when rel_max == rel_min)
//   g_ij    = sum_d table[id_i, d] * table[id_j, d]      fp32 operands, fp32 accumulate
//             (v_mfma_f32_16x16x4_f32, as topk_scores.hip: ranking is the output, so no bf16 rounding)
//   c_ij    = g_ij / (sqrt(g_ii) * sqrt(g_jj)); 0 unless g_ii, g_jj are finite and positive and g_ij finite
//   step t  picks the not-yet-picked valid slot with the largest
//             m_j = lam * rhat_j - (1 - lam) * max_{i picked} c_ij        (t = 0: lam * rhat_j)
//           a NaN m_j counts as -inf, ties go to the lowest pool position
//   output  ids / rel of the k picks in selection order ((-1, -inf) past the valid count) and
//           ild = mean of 1 - c_ij over the unordered pairs of picks (0 below two picks)
//
// mmr_rerank_kernel<PP> (P padded to PP in {16, 32, 64, 128}), 256 threads:
//   * gather: the pool's rows stream once through a two-stage LDS ring in chunks of 32 columns
//     (a stage is PP rows of 32 + 4 floats: the pad makes a 16-row b128 fragment read hit 16
//     distinct 16-byte slots; 36 KB for both stages at PP = 128).  All four waves load; the
//     global loads of chunk c + 1 are in flight while chunk c is multiplied; one barrier per chunk;
//   * Gram: wave w owns the 16-row tiles [w RT, w RT + RT) (RT = PP / 64, at least 1; with PP < 64
//     only PP / 16 waves multiply) against all PP / 16 column tiles: RT x PP / 16 accumulator
//     tiles of 4 VGPRs, 64 at PP = 128.  Both operands are fragments of the same staged image, and
//     MFMA step t of a 16-column group takes k = 16 g + 4 (lane >> 4) + t from both -- one fixed
//     k order for every pair, so g_ij depends on the two rows' values only (duplicate rows tie
//     bit for bit).  The P x P matrix never leaves the registers;
//   * norms: the diagonal goes through a PP-float LDS array once; accumulators become cosines in place;
//   * greedy loop: by symmetry column sel of the Gram holds c[row, sel] for a wave's own rows, in the
//     lanes with (lane & 15) == (sel & 15) of column tile sel >> 4 -- an unrolled select over the
//     compile-time tile index (no runtime register index, no private memory), one lane
//     broadcast per row register.  Each lane keeps the running max-similarity of its rows
//     (the 16 lanes of a (lane >> 4) group redundantly), forms m_j, and packs (m_j, position) into
//     one u64 key (topk_scores.hip's monotone map; 0 = no candidate); the key is reduced across
//     the wave, the four waves' winners meet in a parity-indexed LDS slot: one barrier per step;
//   * ild: every lane sums 1 - c over its accumulator elements with both slots picked and
//     row < column, in register order; a fixed shuffle tree, then the four waves in order.
// A user's outputs depend on nothing but the user's pool: bitwise independent of B, of the
// position in the batch and of the grid.  No atomics.
#include "common.h"
#include "launchers.h"

namespace {

typedef unsigned long long u64;

constexpr int MR_DC = 32;          // columns per staged chunk (two 16-column MFMA groups)
constexpr int MR_LD = MR_DC + 4;   // LDS row stride in floats

__device__ __forceinline__ u64 mr_key(float m, int pos) {
  m = m == m ? m : -INFINITY;                               // NaN ranks as -inf
  uint32_t u = __float_as_uint(m);
  u = u == 0x80000000u ? 0u : u;                            // -0 ranks as +0
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);           // monotone: larger m, larger u
  return ((u64)u << 32) | (uint32_t)(~(uint32_t)pos);       // lower position, larger key; never 0
}

__device__ __forceinline__ u64 mr_max(u64 a, u64 b) { return a > b ? a : b; }

__device__ __forceinline__ u64 mr_shfl_xor(u64 v, int j) {
  const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, j, 64);
  const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), j, 64);
  return ((u64)hi << 32) | lo;
}

// min / max that keep a NaN once they meet one (torch.amin / amax semantics)
__device__ __forceinline__ float mr_nanmin(float a, float b) { return (a < b || a != a) ? a : b; }
__device__ __forceinline__ float mr_nanmax(float a, float b) { return (a > b || a != a) ? a : b; }

template <int PP>
struct MrCfg {
  static constexpr int CT = PP / 16;                  // column tiles
  static constexpr int RT = PP >= 64 ? PP / 64 : 1;   // row tiles per wave
  static constexpr int AW = PP >= 64 ? 4 : PP / 16;   // waves that hold Gram rows
  static constexpr int NIT = PP >= 32 ? PP / 32 : 1;  // float4 loads per thread and chunk
};

// the global loads of chunk c (columns [32 c, 32 c + 32) of the thread's rows; columns >= D and
// empty slots zero): all issued before anything waits on them
template <int NIT>
__device__ __forceinline__ void mr_chunk_load(float4 (&st)[NIT], const float* const (&rp)[NIT], int c, int c4, int D) {
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int col = c * MR_DC + c4;
    st[it] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (rp[it] != nullptr && col < D) st[it] = *(const float4*)(rp[it] + col);
  }
}

template <int PP>
__global__ __launch_bounds__(256) void mmr_rerank_kernel(const float* __restrict__ table, const int* __restrict__ ids,
                                                         const float* __restrict__ rel, int* __restrict__ ids_out,
                                                         float* __restrict__ rel_out, float* __restrict__ ild, int N,
                                                         int P, int D, int k, float lam) {
  typedef MrCfg<PP> C;
  __shared__ __attribute__((aligned(16))) float stage[2][PP * MR_LD];
  __shared__ int s_id[PP];
  __shared__ float s_rel[PP];
  __shared__ float s_rhat[PP];
  __shared__ float s_diag[PP];
  __shared__ int s_pick[PP];
  __shared__ u64 s_key[2][4];
  __shared__ float s_red[4];
  __shared__ float s_mm[2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fq = lane >> 4;
  const size_t b = blockIdx.x;
  const int* idp = ids + b * P;
  const float* relp = rel + b * P;
  const bool active = wave < C::AW;

  // ---- the pool: ids, relevance, its min / max over the valid slots (wave 0)
  if (tid < PP) {
    s_id[tid] = tid < P ? idp[tid] : -1;
    s_rel[tid] = tid < P ? relp[tid] : 0.f;
    s_pick[tid] = 0;
  }
  if (wave == 0) {
    float mn = INFINITY, mx = -INFINITY;
#pragma unroll
    for (int h = 0; h < (PP + 63) / 64; ++h) {
      const int j = lane + 64 * h;
      if (j < P && idp[j] >= 0) {
        const float x = relp[j];
        mn = mr_nanmin(mn, x);
        mx = mr_nanmax(mx, x);
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      mn = mr_nanmin(mn, __shfl_xor(mn, o, 64));
      mx = mr_nanmax(mx, __shfl_xor(mx, o, 64));
    }
    if (lane == 0) {
      s_mm[0] = mn;
      s_mm[1] = mx;
    }
  }

  // ---- gather + Gram
  const int c4 = (tid & 7) * 4;
  const float* rp[C::NIT];
#pragma unroll
  for (int it = 0; it < C::NIT; ++it) {
    const int row = (tid + 256 * it) >> 3;
    const int id = row < P ? idp[row] : -1;
    rp[it] = id >= 0 ? table + (size_t)min(id, N - 1) * D : nullptr;
  }
  f32x4 acc[C::RT][C::CT];
#pragma unroll
  for (int rt = 0; rt < C::RT; ++rt)
#pragma unroll
    for (int ct = 0; ct < C::CT; ++ct) acc[rt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int NCH = (D + MR_DC - 1) / MR_DC, NG = (D + 15) / 16;
  float4 st[C::NIT];
  mr_chunk_load<C::NIT>(st, rp, 0, c4, D);
#pragma unroll
  for (int it = 0; it < C::NIT; ++it) {
    const int i = tid + 256 * it;
    if (i < PP * 8) *(float4*)(stage[0] + (i >> 3) * MR_LD + c4) = st[it];
  }
  __syncthreads();
  if (tid < PP) {
    const float mn = s_mm[0], mx = s_mm[1];
    s_rhat[tid] = mx == mn ? 1.f : (s_rel[tid] - mn) / (mx - mn);
  }
  for (int c = 0; c < NCH; ++c) {
    const int cur = c & 1;
    const bool more = c + 1 < NCH;
    if (more) mr_chunk_load<C::NIT>(st, rp, c + 1, c4, D);
    if (active) {
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        if (2 * c + g < NG) {  // wave-uniform
          const float* sp = stage[cur] + fr * MR_LD + 16 * g + 4 * fq;
          float4 bv[C::CT], av[C::RT];
#pragma unroll
          for (int ct = 0; ct < C::CT; ++ct) bv[ct] = *(const float4*)(sp + 16 * ct * MR_LD);
#pragma unroll
          for (int rt = 0; rt < C::RT; ++rt) av[rt] = *(const float4*)(sp + 16 * (wave * C::RT + rt) * MR_LD);
#pragma unroll
          for (int rt = 0; rt < C::RT; ++rt)
#pragma unroll
            for (int ct = 0; ct < C::CT; ++ct)
              acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[rt].x, bv[ct].x, acc[rt][ct], 0, 0, 0);
#pragma unroll
          for (int rt = 0; rt < C::RT; ++rt)
#pragma unroll
            for (int ct = 0; ct < C::CT; ++ct)
              acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[rt].y, bv[ct].y, acc[rt][ct], 0, 0, 0);
#pragma unroll
          for (int rt = 0; rt < C::RT; ++rt)
#pragma unroll
            for (int ct = 0; ct < C::CT; ++ct)
              acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[rt].z, bv[ct].z, acc[rt][ct], 0, 0, 0);
#pragma unroll
          for (int rt = 0; rt < C::RT; ++rt)
#pragma unroll
            for (int ct = 0; ct < C::CT; ++ct)
              acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[rt].w, bv[ct].w, acc[rt][ct], 0, 0, 0);
        }
      }
    }
    if (more) {
#pragma unroll
      for (int it = 0; it < C::NIT; ++it) {
        const int i = tid + 256 * it;
        if (i < PP * 8) *(float4*)(stage[cur ^ 1] + (i >> 3) * MR_LD + c4) = st[it];
      }
    }
    __syncthreads();
  }

  // ---- norms: accumulator element r of tile (rt, ct) is g[16 (wave RT + rt) + 4 fq + r][16 ct + fr]
  if (active) {
#pragma unroll
    for (int rt = 0; rt < C::RT; ++rt) {
      const int mt = wave * C::RT + rt;
#pragma unroll
      for (int ct = 0; ct < C::CT; ++ct) {
        if (ct == mt) {  // wave-uniform
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (fr == 4 * fq + r) s_diag[16 * mt + fr] = acc[rt][ct][r];
        }
      }
    }
  }
  __syncthreads();
  float rh[C::RT][4], ms[C::RT][4];
  unsigned alive = 0u, mine = 0u;  // bit 4 rt + r: the row is a live candidate / was picked
  if (active) {
    float sc[C::CT];
    bool okc[C::CT];
#pragma unroll
    for (int ct = 0; ct < C::CT; ++ct) {
      const float gjj = s_diag[16 * ct + fr];
      okc[ct] = gjj > 0.f && gjj < INFINITY;
      sc[ct] = sqrtf(gjj);
    }
#pragma unroll
    for (int rt = 0; rt < C::RT; ++rt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = 16 * (wave * C::RT + rt) + 4 * fq + r;
        const float gii = s_diag[j];
        const bool okr = gii > 0.f && gii < INFINITY;
        const float sr = sqrtf(gii);
#pragma unroll
        for (int ct = 0; ct < C::CT; ++ct) {
          const float g = acc[rt][ct][r];
          acc[rt][ct][r] = (okr && okc[ct] && fabsf(g) < INFINITY) ? g / (sr * sc[ct]) : 0.f;
        }
        rh[rt][r] = s_rhat[j];
        ms[rt][r] = 0.f;
        if (s_id[j] >= 0) alive |= 1u << (4 * rt + r);
      }
    }
  } else {
#pragma unroll
    for (int rt = 0; rt < C::RT; ++rt)
#pragma unroll
      for (int r = 0; r < 4; ++r) rh[rt][r] = ms[rt][r] = 0.f;
  }

  // ---- greedy selection
  const float oml = 1.f - lam;
  int np = 0;
  for (int t = 0; t < k; ++t) {
    u64 best = 0ull;
#pragma unroll
    for (int rt = 0; rt < C::RT; ++rt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = 16 * (wave * C::RT + rt) + 4 * fq + r;
        const float pen = t > 0 ? oml * ms[rt][r] : 0.f;
        const float m = lam * rh[rt][r] - pen;
        best = mr_max(best, (alive >> (4 * rt + r)) & 1u ? mr_key(m, j) : 0ull);
      }
    }
    best = mr_max(best, mr_shfl_xor(best, 16));
    best = mr_max(best, mr_shfl_xor(best, 32));
    if (lane == 0) s_key[t & 1][wave] = best;
    __syncthreads();
    const u64 win = mr_max(mr_max(s_key[t & 1][0], s_key[t & 1][1]), mr_max(s_key[t & 1][2], s_key[t & 1][3]));
    if (win == 0ull) break;  // block-uniform: every valid slot is taken
    const int sel = __builtin_amdgcn_readfirstlane((int)(~(uint32_t)win));
    np = t + 1;
    if (tid == 0) {
      ids_out[b * k + t] = s_id[sel];
      rel_out[b * k + t] = s_rel[sel];
      s_pick[sel] = 1;
    }
    const int stile = sel >> 4, src = (lane & 48) | (sel & 15);
#pragma unroll
    for (int rt = 0; rt < C::RT; ++rt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v = 0.f;
#pragma unroll
        for (int ct = 0; ct < C::CT; ++ct) v = ct == stile ? acc[rt][ct][r] : v;
        v = __shfl(v, src, 64);  // c[row, sel] from the lane that holds column sel
        ms[rt][r] = t > 0 ? fmaxf(ms[rt][r], v) : v;
        const int j = 16 * (wave * C::RT + rt) + 4 * fq + r;
        if (j == sel) {
          alive &= ~(1u << (4 * rt + r));
          mine |= 1u << (4 * rt + r);
        }
      }
    }
  }
  for (int e = np + tid; e < k; e += 256) {
    ids_out[b * k + e] = -1;
    rel_out[b * k + e] = -INFINITY;
  }

  // ---- intra-list diversity of the picks
  __syncthreads();
  float sum = 0.f;
  if (active) {
#pragma unroll
    for (int rt = 0; rt < C::RT; ++rt) {
#pragma unroll
      for (int ct = 0; ct < C::CT; ++ct) {
        const int col = 16 * ct + fr;
        const bool pc = s_pick[col] != 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int j = 16 * (wave * C::RT + rt) + 4 * fq + r;
          const bool on = ((mine >> (4 * rt + r)) & 1u) && pc && j < col;
          sum += on ? 1.f - acc[rt][ct][r] : 0.f;
        }
      }
    }
  }
  sum = wave_sum(sum);
  if (lane == 0) s_red[wave] = sum;
  __syncthreads();
  if (tid == 0) {
    const float tot = ((s_red[0] + s_red[1]) + s_red[2]) + s_red[3];
    ild[b] = np >= 2 ? tot / (float)(np * (np - 1) / 2) : 0.f;
  }
}

template <int PP>
void mr_launch(const float* table, const int* ids, const float* rel, int* ids_out, float* rel_out, float* ild, int B,
               int N, int P, int D, int k, float lam, hipStream_t s) {
  hipLaunchKernelGGL(mmr_rerank_kernel<PP>, dim3((unsigned)B), dim3(256), 0, s, table, ids, rel, ids_out, rel_out, ild,
                     N, P, D, k, lam);
}

}  // namespace

// 0 ok; 1 unsupported shape or lam; 2 misaligned table
extern "C" int fr_mmr_rerank(const float* table, const int* ids, const float* rel, int* ids_out, float* rel_out,
                             float* ild, long B, long N, int P, int D, int k, float lam, hipStream_t s) {
  if (!(B >= 1 && B < 2147483648L && N >= 1 && N < 2147483648L && P >= 1 && P <= 128 && k >= 1 && k <= P && D >= 4 &&
        D <= 512 && D % 4 == 0 && lam >= 0.f && lam <= 1.f))
    return 1;
  if (((uintptr_t)table) & 15) return 2;
  if (P <= 16)
    mr_launch<16>(table, ids, rel, ids_out, rel_out, ild, (int)B, (int)N, P, D, k, lam, s);
  else if (P <= 32)
    mr_launch<32>(table, ids, rel, ids_out, rel_out, ild, (int)B, (int)N, P, D, k, lam, s);
  else if (P <= 64)
    mr_launch<64>(table, ids, rel, ids_out, rel_out, ild, (int)B, (int)N, P, D, k, lam, s);
  else
    mr_launch<128>(table, ids, rel, ids_out, rel_out, ild, (int)B, (int)N, P, D, k, lam, s);
  return 0;
}
