// The exact retrieval kernels' arguments and their source for the shared scan (topk_scan.h): a query
// tile's wave against one split of the item table. Shared by retrieval.hip (k <= TT_TOPK_MAX_K, sorted
// partial lists) and topk_large.hip (k <= TT_TOPK_LARGE_MAX_K, pooled radix selection).
#pragma once

#include "topk_scan.h"

namespace tt {

struct TopkArgs {
  const void* q;
  const void* c;
  const float* bias;
  u64* ws;  // [S][M][k] keys, each list sorted descending, 0 = no entry (topk_large.hip: [S][M][2 k + 32] pools)
  int64_t ldq, ldc, M, N, per;  // per: items per split (a multiple of the chunk)
  int k, S, qtiles, q_bf16, c_bf16, c_vec;
};

// the FILT instantiations' arguments: allow is NULL or ceil(N / 32) words (bit n & 31 of word n >> 5:
// item n is eligible); excl_offsets is NULL or [M + 1] absolute offsets into excl_values, query m's
// segment ascending
struct TopkFiltArgs : TopkArgs {
  const uint32_t* allow;
  const int32_t* excl_values;
  const int64_t* excl_offsets;
};

// a workgroup's work unit for the shared scan (topk_scan.h): a query tile's wave against one split
template <int KS, bool FILT>
struct ExactSrc {
  using Sh = ScanShape<KS>;
  const std::conditional_t<FILT, TopkFiltArgs, TopkArgs>& a;
  int64_t m_wave;  // the wave's queries: m_wave + q, while < M
  u64* lists;
  int64_t n_beg, n_end;
  int nchunks;
  bool wave_excl;
  const int32_t* excl_values;
  bool raw_bf16;  // bf16 rows that 16-byte loads can fetch: staged as they are
  // staging: thread t holds 8-element groups g = t + TK_THREADS i of the chunk: item row g / GPR
  f32x4 rawf[Sh::GPT][2];
  bf16x8 rawb[Sh::GPT];
  uint32_t rawmask;

  __device__ __forceinline__ bool computes() const { return true; }
  __device__ __forceinline__ int64_t query(int q) const { return m_wave + q < a.M ? m_wave + q : -1; }
  __device__ __forceinline__ int index(int64_t n) const { return (int)n; }
  __device__ __forceinline__ bool has_list(int q) const { return m_wave + q < a.M; }
  __device__ __forceinline__ const int64_t* excl(int q) const { return a.excl_offsets + m_wave + q; }

  __device__ __forceinline__ void load_rows(int64_t n0, int tid) {
#pragma unroll
    for (int i = 0; i < Sh::GPT; ++i) {
      const int g = tid + TK_THREADS * i;
      const int row = g / Sh::GPR, kc = (g - row * Sh::GPR) * 8;
      const int64_t n = n0 + row;
      if (raw_bf16) {
        bf16x8 z;
#pragma unroll
        for (int j = 0; j < 8; ++j) z[j] = (__bf16)0.f;
        rawb[i] = n < n_end ? *reinterpret_cast<const bf16x8*>(reinterpret_cast<const unsigned short*>(a.c) + n * a.ldc + kc) : z;
      } else if (!a.c_bf16 && a.c_vec) {
        const f32x4* p = reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(a.c) + n * a.ldc + kc);
        rawf[i][0] = n < n_end ? p[0] : (f32x4)(0.f);
        rawf[i][1] = n < n_end ? p[1] : (f32x4)(0.f);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float x = 0.f;
          if (n < n_end) {
            const int64_t o = n * a.ldc + kc + j;
            x = a.c_bf16 ? __uint_as_float(((uint32_t) reinterpret_cast<const unsigned short*>(a.c)[o]) << 16)
                         : reinterpret_cast<const float*>(a.c)[o];
          }
          rawf[i][j >> 2][j & 3] = x;
        }
      }
    }
  }
  __device__ __forceinline__ void store_rows(__bf16* buf, int tid) const {
#pragma unroll
    for (int i = 0; i < Sh::GPT; ++i) {
      const int g = tid + TK_THREADS * i;
      const int row = g / Sh::GPR, kc = (g - row * Sh::GPR) * 8;
      bf16x8 o;
      if (raw_bf16) {
        o = rawb[i];
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (__bf16)rawf[i][j >> 2][j & 3];  // round-to-nearest-even
      }
      *reinterpret_cast<bf16x8*>(&buf[row * Sh::STRIDE + kc]) = o;
    }
  }
  // the chunk's words of `allow` (all ones where it is NULL), one thread per word. n0 is a multiple
  // of the chunk, the chunk of 32: the words are whole; those past the N items count as zero
  __device__ __forceinline__ void load_mask(int, int64_t n0, int tid) {
    if (tid < Sh::MW) {
      const int64_t wd = (n0 >> 5) + tid;
      rawmask = !a.allow ? 0xffffffffu : wd < ((a.N + 31) >> 5) ? a.allow[wd] : 0u;
    }
  }
  __device__ __forceinline__ void store_mask(uint32_t* words, int tid) const {
    if (tid < Sh::MW) words[tid] = rawmask;
  }
};

}  // namespace tt
