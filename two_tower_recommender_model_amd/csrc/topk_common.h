// Selection helpers shared by the exact top-k kernel (retrieval.hip) and the IVF list scan (ivf.hip):
// the 64-bit key order, the wave-level syncs, a wave's selection state in LDS, the rank-counting merge
// of a candidate buffer into a sorted partial list, and the exclusion-list drop.
#pragma once

#include "tt_common.h"

namespace tt {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef unsigned long long u64;

constexpr int TK_WAVES = 4;
constexpr int TK_THREADS = 64 * TK_WAVES;
constexpr int TK_QW = 32;               // queries per wave (2 MFMA tiles)
constexpr int TK_QB = TK_WAVES * TK_QW; // queries per workgroup
// items per staged chunk: one global round trip per chunk, so as many as keep two workgroups'
// LDS on a CU (E <= 64), else 64
constexpr int tk_chunk(int E) { return E <= 64 ? 128 : 64; }
constexpr int TK_CB = 32;               // candidate keys per query
constexpr int TK_MAX_SPLITS = 64;       // one lane per split in the merge kernel

__device__ __forceinline__ u64 make_key(float s, int n) {
  s += 0.f;  // -0 -> +0: equal scores, equal keys
  uint32_t u = __float_as_uint(s);
  u ^= (u & 0x80000000u) ? 0xffffffffu : 0x80000000u;
  return ((u64)u << 32) | (u64)(0xffffffffu - (uint32_t)n);
}
__device__ __forceinline__ float key_score(u64 k) {
  uint32_t u = (uint32_t)(k >> 32);
  u ^= (u & 0x80000000u) ? 0x80000000u : 0xffffffffu;
  return __uint_as_float(u);
}
__device__ __forceinline__ int key_index(u64 k) { return (int)(0xffffffffu - (uint32_t)k); }

// LDS only: a wave's LDS operations execute in program order, so this orders nothing in hardware and
// only keeps the compiler from moving LDS accesses across it (no wait for outstanding global loads)
__device__ __forceinline__ void lds_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// LDS (and the list's global words) written by some lanes of this wave, read by others
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

// one wave's selection state in LDS
struct WaveSel {
  u64* cbuf;    // [TK_QW][TK_CB]
  u64* lscr;    // [Sink::SCR] the sink's scratch: a list's copy [TT_TOPK_MAX_K], or a 256-bin histogram
  int* ccnt;    // [TK_QW] candidates buffered
  int* lcnt;    // [TK_QW] entries of the partial list (of the pool)
  float* thrs;  // [TK_QW] score of the list's k-th entry (-inf while shorter; +inf: no such query)
};

// buffer of wave-local query q -> its sorted partial list gl (k keys). New rank of a list entry =
// its index + the candidates above it; of a candidate = the list entries above it (binary search)
// + the candidates above it. Keys are distinct, so the ranks are; ranks >= k fall out. The buffer's
// unused slots hold 0, so the candidate loops run over all TK_CB slots, unrolled: their LDS reads
// pipeline (a loop over the count paid one LDS latency per candidate).
__device__ __noinline__ void topk_merge_query(const WaveSel w, int q, u64* gl, int k, int lane) {
  const int nc = w.ccnt[q], L = w.lcnt[q];
  const u64* cb = w.cbuf + q * TK_CB;
  // the stores of this list's previous merge (other lanes of this wave) have completed; the list
  // is read from L2 (agent-scope loads), where they went. The stores below are not waited for
  wave_sync();
  for (int i = lane; i < L; i += 64) w.lscr[i] = __hip_atomic_load(gl + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  lds_wave_sync();
  for (int i = lane; i < L; i += 64) {
    const u64 e = w.lscr[i];
    int rank = i;
#pragma unroll
    for (int c = 0; c < TK_CB; ++c) rank += cb[c] > e ? 1 : 0;  // unused slots hold 0: never above
    if (rank < k) {
      __hip_atomic_store(gl + rank, e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (rank == k - 1) w.thrs[q] = key_score(e);
    }
  }
  if (lane < nc) {
    const u64 e = cb[lane];
    int lo = 0, hi = L;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (w.lscr[mid] > e) lo = mid + 1; else hi = mid;
    }
    int rank = lo;
#pragma unroll
    for (int c = 0; c < TK_CB; ++c) rank += cb[c] > e ? 1 : 0;
    if (rank < k) {
      __hip_atomic_store(gl + rank, e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (rank == k - 1) w.thrs[q] = key_score(e);
    }
  }
  lds_wave_sync();
  if (lane < TK_CB) w.cbuf[q * TK_CB + lane] = 0ull;
  if (lane == 0) {
    w.lcnt[q] = min(k, L + nc);
    w.ccnt[q] = 0;
  }
  lds_wave_sync();
}

// wave-local query q's buffered candidates that are in the query's exclusion segment
// xv[xo[0], xo[1]) (ascending; only the segment is read) are dropped and the buffer is compacted
// (its order is free: the merge ranks by counting). One lane per buffered key (at most TK_CB = 32),
// so the binary searches' dependent loads run side by side. Returns the candidates left.
__device__ __noinline__ int topk_drop_excluded(const WaveSel w, int q, const int32_t* __restrict__ xv,
                                               const int64_t* __restrict__ xo, int lane) {
  const int nc = w.ccnt[q];
  const int64_t beg = xo[0], end = xo[1];
  if (end <= beg) return nc;
  u64* cb = w.cbuf + q * TK_CB;
  u64 e = 0ull;
  bool keep = false;
  if (lane < nc) {
    e = cb[lane];
    const int n = key_index(e);
    int64_t lo = beg, hi = end;
    while (lo < hi) {
      const int64_t mid = lo + ((hi - lo) >> 1);
      if (xv[mid] < n) lo = mid + 1; else hi = mid;
    }
    keep = !(lo < end && xv[lo] == n);
  }
  const u64 kept = __ballot(keep);
  const int nk = __popcll(kept);
  if (nk == nc) return nc;
  lds_wave_sync();  // every lane has read its key
  if (keep) cb[__popcll(kept & ((1ull << lane) - 1ull))] = e;  // places [0, nk)
  if (lane >= nk && lane < TK_CB) cb[lane] = 0ull;
  if (lane == 0) w.ccnt[q] = nk;
  lds_wave_sync();
  return nk;
}
}  // namespace tt
