// Exact top-k retrieval for k up to TT_TOPK_LARGE_MAX_K = 8192 on gfx950 (tt_topk_mips_large): the
// shared scan (topk_scan.h) of tt_topk_mips / tt_topk_mips_filtered with another sink. A sorted list
// per query does not stretch to thousands of keys (64 KB per list at k = 8192, O(k) rank counting per
// merge, k serial rounds in the split merge); here every (split, query) keeps an UNSORTED pool and
// prunes it by selecting its k-th key.
//
//   pool: CAP = 2 k + TK_CB keys in the workspace ([S][M][CAP]), touched by the owning wave only, no
//   atomics on it. A full candidate buffer is appended with one 8-byte store per lane. When the next
//   append would not fit, the wave prunes: a radix select of the k-th largest key (64-bit keys, MSB
//   first, 8-bit digits, a 256-bin histogram per wave in LDS where the list sink has its 2-KB strip),
//   then a front compaction in place that keeps the keys >= it. Keys are distinct, so exactly k
//   survive, and the k-th key's score is the query's new threshold (-inf until the first prune).
//   The select stops at the first digit that decides enough: during the scan a prune may keep up to
//   k / 8 keys more than k (those that share the k-th key's leading digits) and takes the score of
//   those digits, a lower bound of the k-th score, as the threshold; the flush prunes to exactly k.
//   The strict filter "score > threshold" loses nothing, as in the list sink: a split streams
//   ascending indices, so an equal score met later has a lower key than everything kept.
//
//   flush: drop excluded keys, append, prune once if the pool holds more than k, pad to k with key 0
//   ("no entry"). The pool's first k words are the split's result, in no order.
//
//   merge (one workgroup per query): radix select of the k-th key over the S pools' first k words,
//   gather of the survivors into the query's first pool behind its k result words, a bitonic sort in
//   LDS, ids / scores. A zero key becomes -1 / -inf.
//
// The score chain, the key order, the mask and the exclusion lists are the scan's, so the result is
// the unique one: bit-identical across runs and split counts, and to tt_topk_mips(_filtered) where
// both exist.
#include "tt_common.h"
#include "topk_exact.h"

namespace tt {

constexpr int TKL_THREADS = 1024;  // the merge kernel's workgroup

__host__ __device__ constexpr int64_t tkl_cap(int k) { return 2 * (int64_t)k + TK_CB; }

// One 8-bit digit of a radix select, the part after the histogram is filled: `need` is the rank
// (1-based, from the top) wanted among the keys that match the digits chosen so far, hist their
// counts by this digit. Returns the digit the wanted key has; `need` becomes its rank among the keys
// that share it, `bin` their number. Whole wave, lane l looks at bins 4 l .. 4 l + 3.
__device__ __forceinline__ int radix_pick(const uint32_t* hist, int& need, int& bin, int lane) {
  const uint32_t h0 = hist[4 * lane], h1 = hist[4 * lane + 1], h2 = hist[4 * lane + 2], h3 = hist[4 * lane + 3];
  const int sum = (int)(h0 + h1 + h2 + h3);
  int suf = sum;  // the keys in this lane's bins and in higher lanes'
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_down(suf, o, 64);
    if (lane + o < 64) suf += t;
  }
  int above = suf - sum, digit = 0, cnt = 0;
  const bool mine = above < need && need <= suf;
  if (mine) {
    if (need <= above + (int)h3) {
      digit = 4 * lane + 3;
      cnt = (int)h3;
    } else if (need <= above + (int)(h3 + h2)) {
      digit = 4 * lane + 2;
      cnt = (int)h2;
      above += (int)h3;
    } else if (need <= above + (int)(h3 + h2 + h1)) {
      digit = 4 * lane + 1;
      cnt = (int)h1;
      above += (int)(h3 + h2);
    } else {
      digit = 4 * lane;
      cnt = (int)h0;
      above += (int)(h3 + h2 + h1);
    }
  }
  // exactly one lane has it: at least `need` keys match the digits so far
  const int src = __builtin_ctzll(__ballot(mine) | (1ull << 63));
  need -= __shfl(above, src, 64);
  bin = __shfl(cnt, src, 64);
  return __shfl(digit, src, 64);
}

// one key of a radix pass into the histogram. Keys of one pass often share the digit (the scores'
// sign and exponent; equal scores): a wave whose matching keys all have the first one's digit adds
// their number once instead of serialising 64 LDS atomics on one bin
__device__ __forceinline__ void radix_count(uint32_t* hist, bool match, int digit, int lane) {
  const u64 mm = __ballot(match);
  if (mm == 0ull) return;
  const int d0 = __shfl(digit, __builtin_ctzll(mm), 64);
  if (__ballot(match && digit != d0) == 0ull) {
    if (lane == 0) atomicAdd(&hist[d0], (uint32_t)__popcll(mm));
  } else if (match) {
    atomicAdd(&hist[digit], 1u);
  }
}

// wave-local query q's pool (n > k keys, all distinct and non-zero) -> its largest keys in front, at
// least k and at most k + slack of them; returns their number. The select stops at the first digit
// after which the keys above the wanted key's bin and the bin together are no more than that: they
// are the keys >= `prefix`, the digits chosen so far with zeros below. With continuous scores that is
// after 3 or 4 of the 8 digits; slack = 0 (the flush) ends with exactly the k largest, if need be in
// the index digits. The threshold becomes the score of `prefix`, a lower bound of the k-th key's (the
// orderable bits below the chosen digits are zero), so the strict filter still loses nothing
__device__ __forceinline__ int topk_pool_prune(const WaveSel w, int q, u64* pool, int n, int k, int slack, int lane) {
  uint32_t* hist = reinterpret_cast<uint32_t*>(w.lscr);
  // the appended keys (other lanes' stores) have completed; the pool is read from L2, where they went
  wave_sync();
  u64 prefix = 0ull, himask = 0ull;
  int need = k;
#pragma unroll 1
  for (int shift = 56; shift >= 0; shift -= 8) {
#pragma unroll
    for (int i = 0; i < 4; ++i) hist[lane + 64 * i] = 0u;
    lds_wave_sync();
    for (int i0 = 0; i0 < n; i0 += 64) {
      const int i = i0 + lane;
      const u64 e = i < n ? __hip_atomic_load(pool + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
      radix_count(hist, i < n && (e & himask) == prefix, (int)(e >> shift) & 255, lane);
    }
    lds_wave_sync();
    int bin;
    const int digit = radix_pick(hist, need, bin, lane);
    lds_wave_sync();
    prefix |= (u64)digit << shift;
    himask |= 0xffull << shift;
    // k - need keys lie above the bin; the last digit's bins hold one key each
    if (k - need + bin <= k + slack) break;
  }
  // front compaction in place: a step's 64 keys are in registers before its stores, which go to
  // places at or below the ones it read
  int wr = 0;
  for (int i0 = 0; i0 < n; i0 += 64) {
    const int i = i0 + lane;
    const u64 e = i < n ? __hip_atomic_load(pool + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
    const bool keep = i < n && e >= prefix;
    const u64 kept = __ballot(keep);
    if (keep) __hip_atomic_store(pool + wr + __popcll(kept & ((1ull << lane) - 1ull)), e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    wr += __popcll(kept);
  }
  if (lane == 0) {
    const float t = key_score(prefix);  // NaN only where the k-th score is not finite: then no bound
    w.thrs[q] = t == t ? fmaxf(w.thrs[q], t) : w.thrs[q];
    w.lcnt[q] = wr;
  }
  lds_wave_sync();
  return wr;
}

// wave-local query q's buffered candidates -> its pool, after a prune (to k + k / 8 keys at the most:
// the slack saves about half of the select's passes and costs an eighth of the room) where they do not
// fit. `last` (the flush): the pool is then pruned to exactly k if it holds more. One function, not inlined,
// with both prunes inside it: a call from a called function would cost a scratch frame
__device__ __noinline__ void topk_pool_append(const WaveSel w, int q, u64* pool, int k, int lane, bool last) {
  const int nc = w.ccnt[q];
  int n = w.lcnt[q];
  if (n + nc > (int)tkl_cap(k)) n = topk_pool_prune(w, q, pool, n, k, k >> 3, lane);  // k + k / 8 + TK_CB <= CAP
  if (lane < nc && n + lane < (int)tkl_cap(k)) __hip_atomic_store(pool + n + lane, w.cbuf[q * TK_CB + lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  lds_wave_sync();
  if (lane < TK_CB) w.cbuf[q * TK_CB + lane] = 0ull;
  n += nc;
  if (lane == 0) {
    w.lcnt[q] = n;
    w.ccnt[q] = 0;
  }
  lds_wave_sync();
  if (last && n > k) topk_pool_prune(w, q, pool, n, k, 0, lane);
}

struct PoolSink {
  static constexpr int SCR = 128;  // 256 histogram bins of 4 bytes
  static __device__ __forceinline__ void absorb(const WaveSel w, int q, u64* lists, int k, int lane) {
    topk_pool_append(w, q, lists + (int64_t)q * tkl_cap(k), k, lane, false);
  }
  static __device__ __forceinline__ void flush(const WaveSel w, int q, u64* lists, int k, int lane) {
    u64* pool = lists + (int64_t)q * tkl_cap(k);
    topk_pool_append(w, q, pool, k, lane, true);
    for (int i = w.lcnt[q] + lane; i < k; i += 64) pool[i] = 0ull;
  }
};

template <int KS, bool BIAS, bool FILT>
__global__ void __launch_bounds__(TK_THREADS, 2)
    topk_large_kernel(const std::conditional_t<FILT, TopkFiltArgs, TopkArgs> a) {
  constexpr int TK_IC = ScanShape<KS>::IC;
  // the work units and their order are topk_mips_kernel's (retrieval.hip)
  const int logical = xcd_remap((int)blockIdx.x, (int)gridDim.x);
  const int split = logical / a.qtiles, qtile = logical - split * a.qtiles;
  const int64_t n_beg = (int64_t)split * a.per;
  const int64_t n_end = n_beg + a.per < a.N ? n_beg + a.per : a.N;
  const int nchunks = n_end > n_beg ? (int)((n_end - n_beg + TK_IC - 1) / TK_IC) : 0;
  const int64_t m_wave = (int64_t)qtile * TK_QB + (threadIdx.x >> 6) * TK_QW;
  bool wave_excl = false;
  const int32_t* excl_values = nullptr;
  if constexpr (FILT) {
    excl_values = a.excl_values;
    if (a.excl_offsets && m_wave < a.M) {
      const int64_t m_last = m_wave + TK_QW < a.M ? m_wave + TK_QW : a.M;
      wave_excl = __builtin_amdgcn_readfirstlane((int)(a.excl_offsets[m_last] > a.excl_offsets[m_wave])) != 0;
    }
  }
  // the wave's pools in [S][M][CAP]
  u64* lists = a.ws + ((int64_t)split * a.M + m_wave) * tkl_cap(a.k);
  if constexpr (FILT) asm volatile("" : "+v"(lists));
  ExactSrc<KS, FILT> s{a, m_wave, lists, n_beg, n_end, nchunks, wave_excl, excl_values, a.c_bf16 && a.c_vec};
  topk_scan_body<KS, BIAS, FILT, FILT, PoolSink>(s);
}

// ids / scores [k] of query blockIdx.x from its S pools' first k words
__global__ void __launch_bounds__(TKL_THREADS) topk_large_merge_kernel(u64* __restrict__ ws, int64_t M, int k, int S,
                                                                       int64_t* __restrict__ ids,
                                                                       float* __restrict__ scores) {
  // the sort's keys; the select's histogram and its few words lie in it, before it is filled
  __shared__ u64 sbuf[TT_TOPK_LARGE_MAX_K];
  uint32_t* hist = reinterpret_cast<uint32_t*>(sbuf);      // [256]
  int* sel = reinterpret_cast<int*>(sbuf) + 256;           // digit, need, stop
  const int tid = threadIdx.x, lane = tid & 63;
  const int64_t m = blockIdx.x;
  const int64_t cap = tkl_cap(k);
  const auto pool = [&](int s) { return ws + ((int64_t)s * M + m) * cap; };
  // the survivors' place: behind the k result words of the query's first pool (CAP - k >= k words)
  u64* surv = pool(0) + k;

  u64 kth = 0ull;  // the k-th key's leading digits, zeros below: exactly k words are >= it. S = 1: all
  if (S > 1) {
    u64 himask = 0ull;
    int need = k;
#pragma unroll 1
    for (int shift = 56; shift >= 0; shift -= 8) {
      if (tid < 256) hist[tid] = 0u;
      __syncthreads();
      for (int s = 0; s < S; ++s) {
        const u64* p = pool(s);
        for (int i0 = 0; i0 < k; i0 += TKL_THREADS) {  // whole waves: radix_count is a wave's
          const int i = i0 + tid;
          const u64 e = i < k ? p[i] : 0ull;
          radix_count(hist, i < k && (e & himask) == kth, (int)(e >> shift) & 255, lane);
        }
      }
      __syncthreads();
      if (tid < 64) {
        int bin;
        const int digit = radix_pick(hist, need, bin, lane);
        if (lane == 0) {
          sel[0] = digit;
          sel[1] = need;
          sel[2] = bin == need;  // the keys >= the digits so far are exactly k: topk_pool_prune's stop
        }
      }
      __syncthreads();
      kth |= (u64)sel[0] << shift;
      need = sel[1];
      himask |= 0xffull << shift;
      const bool stop = sel[2] != 0;
      __syncthreads();
      if (stop) break;
    }
  }

  // the survivors: the non-zero keys >= that (distinct: at most k), in any order
  int* cnt = reinterpret_cast<int*>(sbuf);
  if (tid == 0) *cnt = 0;
  __syncthreads();
  if (S > 1) {
    for (int s = 0; s < S; ++s) {
      const u64* p = pool(s);
      for (int i = tid; i < k; i += TKL_THREADS) {
        const u64 e = p[i];
        if (e != 0ull && e >= kth) {
          const int at = atomicAdd(cnt, 1);
          if (at < k) __hip_atomic_store(surv + at, e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
    }
  }
  __threadfence();
  __syncthreads();
  const int ns = S > 1 ? min(*cnt, k) : k;  // S = 1: the pool itself, its zeros sort last
  const u64* src = S > 1 ? surv : pool(0);
  int P = 64;
  while (P < k) P <<= 1;
  __syncthreads();
  for (int i = tid; i < P; i += TKL_THREADS)
    sbuf[i] = i < ns ? __hip_atomic_load(src + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
  __syncthreads();
  // bitonic sort, descending
  for (int len = 2; len <= P; len <<= 1) {
    for (int j = len >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (P >> 1); t += TKL_THREADS) {
        const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
        const u64 x = sbuf[lo], y = sbuf[hi];
        const bool desc = (lo & len) == 0;
        if ((x < y) == desc) {
          sbuf[lo] = y;
          sbuf[hi] = x;
        }
      }
      __syncthreads();
    }
  }
  for (int i = tid; i < k; i += TKL_THREADS) {
    const u64 e = sbuf[i];
    ids[m * k + i] = e ? (int64_t)key_index(e) : (int64_t)-1;
    scores[m * k + i] = e ? key_score(e) : -std::numeric_limits<float>::infinity();
  }
}

static int topk_large_auto_splits(int64_t M, int64_t N, int k) {
  // tt_topk_mips' occupancy aim (8 waves per CU when the queries alone do not give them), but a split
  // holds at least 4 k items: a split that cannot fill its pools past k prunes nothing and only
  // multiplies the pools and the merge's keys
  const int64_t qtiles = ceil_div(M, TK_QB);
  int64_t s = ceil_div(256 * (8 / TK_WAVES), qtiles);
  s = std::min<int64_t>(s, N / (4 * (int64_t)k));
  return (int)std::max<int64_t>(1, std::min<int64_t>(s, TK_MAX_SPLITS));
}

static const char* topk_large_check(int64_t M, int64_t N, int k, int splits) {
  if (M < 1 || M > (int64_t)1 << 30) return "M must be in [1, 2^30]";
  if (N < 1 || N >= (int64_t)1 << 31) return "N must be in [1, 2^31)";
  if (k < 1 || k > TT_TOPK_LARGE_MAX_K) return "k must be in [1, TT_TOPK_LARGE_MAX_K = 8192]";
  if (splits < 0 || splits > TK_MAX_SPLITS) return "splits must be 0 (chosen by the library) or in [1, 64]";
  return nullptr;
}

static size_t topk_large_ws(int64_t M, int k, int S) { return (size_t)S * (size_t)M * (size_t)tkl_cap(k) * 8; }

template <bool FILT>
static void topk_large_launch(const TopkFiltArgs& a, int E, int blocks, hipStream_t st) {
  const std::conditional_t<FILT, TopkFiltArgs, TopkArgs>& ka = a;
  topk_dispatch(E, a.bias != nullptr, [&](auto ks, auto bias) {
    hipLaunchKernelGGL((topk_large_kernel<decltype(ks)::value, decltype(bias)::value, FILT>), dim3(blocks),
                       dim3(TK_THREADS), 0, st, ka);
  });
}

}  // namespace tt

extern "C" {

size_t tt_topk_mips_large_workspace_bytes(int64_t M, int64_t N, int k, int splits) {
  if (tt::topk_large_check(M, N, k, splits)) return 0;
  return tt::topk_large_ws(M, k, splits ? splits : tt::topk_large_auto_splits(M, N, k));
}

int tt_topk_mips_large(const void* queries, int q_dtype, int64_t ldq, const void* items, int c_dtype, int64_t ldc,
                       const float* bias, int64_t M, int64_t N, int E, int k, int splits, const uint32_t* allow,
                       const int32_t* excl_values, const int64_t* excl_offsets, int64_t* ids, float* scores,
                       void* workspace, size_t ws_bytes, void* stream) {
  using namespace tt;
  const std::string fn = "tt_topk_mips_large";
  if (E < 32 || E > 128 || (E & 31)) return fail(TT_EINVAL, fn + ": E must be a multiple of 32 in [32, 128]");
  if (const char* msg = topk_large_check(M, N, k, splits)) return fail(TT_EINVAL, fn + ": " + msg);
  if ((q_dtype != TT_F32 && q_dtype != TT_BF16) || (c_dtype != TT_F32 && c_dtype != TT_BF16))
    return fail(TT_EINVAL, fn + ": q_dtype / c_dtype must be TT_F32 or TT_BF16");
  if (ldq < E || ldc < E) return fail(TT_EINVAL, fn + ": ldq / ldc must be >= E");
  if (!queries || !items || !ids || !scores || !workspace)
    return fail(TT_EINVAL, fn + ": null queries / items / ids / scores / workspace");
  if ((excl_values == nullptr) != (excl_offsets == nullptr))
    return fail(TT_EINVAL, fn + ": excl_values and excl_offsets must both be NULL or both be given");
  const int S = splits ? splits : topk_large_auto_splits(M, N, k);
  if (ws_bytes < topk_large_ws(M, k, S))
    return fail(TT_EINVAL, fn + ": ws_bytes is smaller than tt_topk_mips_large_workspace_bytes");
  const int64_t qtiles = ceil_div(M, TK_QB);

  TopkFiltArgs a{};
  a.q = queries;
  a.c = items;
  a.bias = bias;
  a.ws = reinterpret_cast<u64*>(workspace);
  a.ldq = ldq;
  a.ldc = ldc;
  a.M = M;
  a.N = N;
  a.per = ceil_div(ceil_div(N, S), tk_chunk(E)) * tk_chunk(E);
  a.k = k;
  a.S = S;
  a.qtiles = (int)qtiles;
  a.q_bf16 = q_dtype == TT_BF16;
  a.c_bf16 = c_dtype == TT_BF16;
  a.c_vec = (reinterpret_cast<uintptr_t>(items) & 15) == 0 && (ldc % (a.c_bf16 ? 8 : 4)) == 0;
  a.allow = allow;
  a.excl_values = excl_values;
  a.excl_offsets = excl_offsets;
  const int blocks = (int)(qtiles * S);
  hipStream_t st = as_stream(stream);
  if (allow || excl_offsets)
    topk_large_launch<true>(a, E, blocks, st);
  else
    topk_large_launch<false>(a, E, blocks, st);
  if (int rc = check_launch("tt_topk_mips_large")) return rc;
  hipLaunchKernelGGL(topk_large_merge_kernel, dim3((unsigned)M), dim3(TKL_THREADS), 0, st, a.ws, M, k, S, ids, scores);
  return check_launch("tt_topk_mips_large merge");
}

}  // extern "C"
