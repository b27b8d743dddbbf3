// IVF (inverted-file) approximate top-k retrieval on gfx950: tt_ivf_scan is the fine step, the top k
// of each query over the items of the lists it probes; tt_ivf_segment_mean is the deterministic
// centroid update of the k-means that builds the index. The coarse step ("nearest centroids of a
// query") is tt_topk_mips itself with the centroids as items.
//
// The index stores the item rows in list order (bf16, a list's rows contiguous, its original item
// indices `labels` ascending). A (query, probed list) PAIR is the unit of work: the pairs are grouped
// by list in the workspace (count, exclusive scan, scatter), so that a workgroup streams ONE list
// past a tile of up to 128 of the queries that probe it, through the shared scan (topk_scan.h); a
// pair's sorted partial list is the k keys at ws + p * k. Keys carry the ORIGINAL item index
// (labels[n], loaded in the candidate branch), so the order "higher score, then lower original
// index" and the exclusion lists work on item indices; labels ascend within a list, so the scan's
// strict compare against the threshold still loses nothing. A last kernel merges a query's up to 64
// partial lists (one lane per probe).
//
// The score of a pair is the same function of the two rows' bf16 values and the bias as in
// tt_topk_mips, and the result is unique under the total order: it is what tt_topk_mips_filtered
// returns when the query is denied every item outside its probed lists, bit for bit, whatever the
// order of the probes and the order of the pairs within a list.
//
// Nothing the device reads can send an access out of range: a probe outside [0, L) is no probe, a
// list that does not lie within the P rows is empty, and the grouping writes only slots it counted.
//
// The item mask (tt_ivf_scan_masked): a bit per PACKED row, row_allow, which tt_ivf_mask_lists makes
// from the mask over original item indices and the labels. A list begins at a multiple of 128, so a
// chunk's bits are whole aligned words: they are loaded with the chunk's other global loads and are
// the scan's row mask.
#include "tt_common.h"
#include "topk_scan.h"

namespace tt {

constexpr int IVF_MAX_PROBE = 64;       // one lane per probed list in the merge kernel
constexpr int64_t IVF_MAX_L = 1 << 20;  // the exclusive scan over the lists is one workgroup
constexpr int IVF_SCAN_THREADS = 1024;

// the workspace: the pairs' partial lists, then the grouping tables
struct IvfWs {
  u64* lists;           // [PN][k] keys, sorted descending, 0 = no entry; pair slot p's list at p * k
  int32_t* cnt;         // [L] pairs of a list
  int32_t* cursor;      // [L] next free place within the list's slots (follows cnt: zeroed together)
  int32_t* list_off;    // [L + 1] first slot of a list (exclusive scan of cnt)
  int32_t* tile_off;    // [L + 1] first workgroup of a list (exclusive scan of ceil(cnt / 128))
  int32_t* pair_query;  // [PN] slot -> query
  int32_t* slot_of;     // [PN] (query, probe column) -> slot, -1: no probe
};

static size_t ivf_ws_layout(int64_t PN, int k, int64_t L, void* base, IvfWs* w) {
  char* p = reinterpret_cast<char*>(base);
  size_t off = 0;
  const auto take = [&](size_t bytes) {
    char* r = p + off;
    off += bytes;
    return r;
  };
  IvfWs t;
  t.lists = reinterpret_cast<u64*>(take((size_t)PN * (size_t)k * 8));
  t.cnt = reinterpret_cast<int32_t*>(take((size_t)L * 4));
  t.cursor = reinterpret_cast<int32_t*>(take((size_t)L * 4));
  t.list_off = reinterpret_cast<int32_t*>(take((size_t)(L + 1) * 4));
  t.tile_off = reinterpret_cast<int32_t*>(take((size_t)(L + 1) * 4));
  t.pair_query = reinterpret_cast<int32_t*>(take((size_t)PN * 4));
  t.slot_of = reinterpret_cast<int32_t*>(take((size_t)PN * 4));
  if (w) *w = t;
  return align_up(off, 16);
}

// ---- grouping --------------------------------------------------------------------------------

__global__ void __launch_bounds__(256) ivf_count_kernel(const int32_t* __restrict__ probes, int64_t PN, int L,
                                                        int32_t* __restrict__ cnt) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= PN) return;
  const int l = probes[i];
  if ((uint32_t)l < (uint32_t)L) atomicAdd(cnt + l, 1);  // anything else, -1 included: no probe
}

// one workgroup: thread t owns lists [t * per, (t + 1) * per); its sums, a scan of the 1024 sums in LDS,
// then its lists' offsets
__global__ void __launch_bounds__(IVF_SCAN_THREADS) ivf_offsets_kernel(const int32_t* __restrict__ cnt, int L,
                                                                       int32_t* __restrict__ list_off,
                                                                       int32_t* __restrict__ tile_off) {
  __shared__ int s_pairs[IVF_SCAN_THREADS];
  __shared__ int s_tiles[IVF_SCAN_THREADS];
  const int tid = threadIdx.x;
  const int per = (L + IVF_SCAN_THREADS - 1) / IVF_SCAN_THREADS;
  const int lo = min(L, tid * per), hi = min(L, lo + per);
  int pairs = 0, tiles = 0;
  for (int i = lo; i < hi; ++i) {
    const int c = cnt[i];
    pairs += c;
    tiles += (c + TK_QB - 1) / TK_QB;
  }
  s_pairs[tid] = pairs;
  s_tiles[tid] = tiles;
  __syncthreads();
  for (int o = 1; o < IVF_SCAN_THREADS; o <<= 1) {
    const int vp = tid >= o ? s_pairs[tid - o] : 0;
    const int vt = tid >= o ? s_tiles[tid - o] : 0;
    __syncthreads();
    s_pairs[tid] += vp;
    s_tiles[tid] += vt;
    __syncthreads();
  }
  int ep = s_pairs[tid] - pairs, et = s_tiles[tid] - tiles;
  for (int i = lo; i < hi; ++i) {
    const int c = cnt[i];
    list_off[i] = ep;
    tile_off[i] = et;
    ep += c;
    et += (c + TK_QB - 1) / TK_QB;
  }
  if (tid == IVF_SCAN_THREADS - 1) {
    list_off[L] = s_pairs[tid];
    tile_off[L] = s_tiles[tid];
  }
}

// pair i = (query i / nprobe, probe column i % nprobe) -> a slot among its list's. The place within
// the list comes from an atomic, so it differs from run to run; the result does not depend on it:
// a pair's partial list is a function of the pair alone, and the merge of a query's lists is the
// unique top k under the total order.
__global__ void __launch_bounds__(256) ivf_scatter_kernel(const int32_t* __restrict__ probes, int64_t PN, int nprobe,
                                                          int L, const int32_t* __restrict__ list_off,
                                                          int32_t* __restrict__ cursor,
                                                          int32_t* __restrict__ pair_query,
                                                          int32_t* __restrict__ slot_of) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= PN) return;
  const int l = probes[i];
  int slot = -1;
  if ((uint32_t)l < (uint32_t)L) {
    slot = list_off[l] + atomicAdd(cursor + l, 1);  // < list_off[l + 1]: the same probes were counted
    pair_query[slot] = (int)(i / nprobe);
  }
  slot_of[i] = slot;
}

// ---- the list scan -----------------------------------------------------------------------------

struct IvfArgs {
  const void* q;
  const unsigned short* rows;  // [P][E] bf16
  const float* bias;           // [P] or NULL
  const int32_t* labels;       // [P]
  const int64_t* list_begin;   // [L]
  const int32_t* list_len;     // [L]
  const int32_t* list_off;
  const int32_t* tile_off;
  const int32_t* pair_query;
  u64* ws;
  const int32_t* excl_values;
  const int64_t* excl_offsets;
  int64_t ldq, M, P;
  int k, L, q_bf16;
};

// the MASK instantiations' arguments: ceil(P / 32) words, bit p & 31 of word p >> 5: row p is eligible
struct IvfMaskArgs : IvfArgs {
  const uint32_t* row_allow;
};

// a workgroup's work unit for the shared scan (topk_scan.h): a wave's pairs against their list
template <int KS, bool MASK>
struct IvfSrc {
  using Sh = ScanShape<KS>;
  const std::conditional_t<MASK, IvfMaskArgs, IvfArgs>& a;
  const int* qid;  // [TK_QW] the wave's pairs' queries, -1: no pair
  int pw;          // the wave's pairs: none in a tile's tail waves
  u64* lists;
  int64_t n_beg, n_end;
  int nchunks;
  bool wave_excl;
  const int32_t* excl_values;
  // MASK: thread t stages word t % MW of a chunk (every thread one, without a branch: the FILT
  // instantiations have no scalar register left for one more saved exec mask). Its index within the
  // list's words (n_beg is a multiple of 32) is clamped to the list's last word: a word that begins
  // at or past n_end is not read and counts as zero
  const uint32_t* mask_p;
  int mask_i, mask_last;
  // staging: thread t holds 8-element groups g = t + TK_THREADS i of the chunk: item row g / GPR.
  // The rows are bf16 already: 16-byte loads, stored as they are
  bf16x8 rawb[Sh::GPT];
  uint32_t rawmask;

  __device__ __forceinline__ bool computes() const { return pw > 0; }
  __device__ __forceinline__ int64_t query(int q) const { return qid[q]; }
  __device__ __forceinline__ int index(int64_t n) const { return a.labels[n]; }
  __device__ __forceinline__ bool has_list(int q) const { return q < pw; }
  __device__ __forceinline__ const int64_t* excl(int q) const { return a.excl_offsets + __builtin_amdgcn_readfirstlane(qid[q]); }

  __device__ __forceinline__ void load_rows(int64_t n0, int tid) {
#pragma unroll
    for (int i = 0; i < Sh::GPT; ++i) {
      const int g = tid + TK_THREADS * i;
      const int row = g / Sh::GPR, kc = (g - row * Sh::GPR) * 8;
      const int64_t n = n0 + row;
      bf16x8 z;
#pragma unroll
      for (int j = 0; j < 8; ++j) z[j] = (__bf16)0.f;
      rawb[i] = n < n_end ? *reinterpret_cast<const bf16x8*>(a.rows + n * Sh::E + kc) : z;
    }
  }
  __device__ __forceinline__ void store_rows(__bf16* buf, int tid) const {
#pragma unroll
    for (int i = 0; i < Sh::GPT; ++i) {
      const int g = tid + TK_THREADS * i;
      const int row = g / Sh::GPR, kc = (g - row * Sh::GPR) * 8;
      *reinterpret_cast<bf16x8*>(&buf[row * Sh::STRIDE + kc]) = rawb[i];
    }
  }
  __device__ __forceinline__ void load_mask(int c, int64_t, int) {
    const int wd = c * Sh::MW + mask_i;  // chunks are loaded only where len > 0: mask_last >= 0
    const uint32_t x = mask_p[min(wd, mask_last)];
    rawmask = wd <= mask_last ? x : 0u;
  }
  __device__ __forceinline__ void store_mask(uint32_t* words, int) const {
    words[mask_i] = rawmask;  // the threads of one word store the same value
  }
};

template <int KS, bool BIAS, bool FILT, bool MASK>
__global__ void __launch_bounds__(TK_THREADS, 2)
    ivf_scan_kernel(const std::conditional_t<MASK, IvfMaskArgs, IvfArgs> a) {
  constexpr int TK_IC = ScanShape<KS>::IC;
  __shared__ int qid_s[TK_WAVES][TK_QW];

  // the grid is an upper bound of the tiles; the tiles of one list are consecutive in the logical
  // order, which an XCD runs a contiguous part of: they share the list's rows through its L2
  const int b = xcd_remap((int)blockIdx.x, (int)gridDim.x);
  const int L = a.L;
  if (b >= a.tile_off[L]) return;
  int l = 0;
  {
    int lo = 0, hi = L;  // the list l with tile_off[l] <= b < tile_off[l + 1]
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (a.tile_off[mid + 1] <= b) lo = mid + 1; else hi = mid;
    }
    l = lo;
  }
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int p_beg = a.list_off[l] + (b - a.tile_off[l]) * TK_QB;
  const int p_end = min(a.list_off[l + 1], p_beg + TK_QB);
  const int p_wave = p_beg + wid * TK_QW;
  const int pw = max(0, min(TK_QW, p_end - p_wave));
  // a list that does not lie within the P rows is empty
  int64_t n_beg = a.list_begin[l];
  int len = a.list_len[l];
  if (len < 0 || n_beg < 0 || n_beg > a.P || (int64_t)len > a.P - n_beg) {
    n_beg = 0;
    len = 0;
  }
  // MASK: so is a list whose rows' bits are not whole words
  if constexpr (MASK) {
    if (n_beg & 31) {
      n_beg = 0;
      len = 0;
    }
  }

  int* qid = qid_s[wid];
  bool lane_excl = false;
  if (lane < TK_QW) {
    int m = lane < pw ? a.pair_query[p_wave + lane] : -1;
    if (m < 0 || m >= a.M) m = -1;
    qid[lane] = m;
    if constexpr (FILT) lane_excl = m >= 0 && a.excl_offsets[m + 1] > a.excl_offsets[m];
  }
  // FILT: does any of the wave's queries have a non-empty exclusion segment?
  const bool wave_excl = FILT && __ballot(lane_excl) != 0ull;
  // FILT + MASK: the exclusion values' address is held in vector registers, where the call of
  // topk_drop_excluded wants it anyway: with the mask the scalar registers do not suffice
  const int32_t* excl_values = a.excl_values;
  if constexpr (FILT && MASK) asm volatile("" : "+v"(excl_values));
  const uint32_t* mask_p = nullptr;
  if constexpr (MASK) {
    mask_p = a.row_allow + (n_beg >> 5);
    asm volatile("" : "+v"(mask_p));  // held in vector registers, for the same reason
  }
  wave_sync();

  IvfSrc<KS, MASK> s{a, qid, pw, a.ws + (int64_t)p_wave * a.k, n_beg, n_beg + len, (len + TK_IC - 1) / TK_IC,
                     wave_excl, excl_values, mask_p, tid & (ScanShape<KS>::MW - 1), (len - 1) >> 5};
  topk_scan_body<KS, BIAS, FILT, MASK>(s);
}

// ids / scores [M][k] from the sorted lists of each query's pairs: one wave per query, lane j walks
// the list of the query's probe column j (no list where the probe was no probe). The lists of
// distinct probes hold distinct items, so keys are distinct
__global__ void __launch_bounds__(TK_THREADS) ivf_merge_kernel(const u64* __restrict__ ws,
                                                               const int32_t* __restrict__ slot_of, int64_t M,
                                                               int nprobe, int k, int64_t* __restrict__ ids,
                                                               float* __restrict__ scores) {
  const int lane = threadIdx.x & 63;
  const int64_t m = (int64_t)blockIdx.x * TK_WAVES + (threadIdx.x >> 6);
  if (m >= M) return;
  const int slot = lane < nprobe ? slot_of[m * nprobe + lane] : -1;
  topk_merge_lists(ws + (int64_t)(slot >= 0 ? slot : 0) * k, slot >= 0, m, k, ids, scores);
}

template <bool FILT, bool MASK>
static void ivf_launch(const IvfMaskArgs& a, int E, unsigned blocks, hipStream_t st) {
  topk_dispatch(E, a.bias != nullptr, [&](auto ks, auto bias) {
    hipLaunchKernelGGL((ivf_scan_kernel<decltype(ks)::value, decltype(bias)::value, FILT, MASK>), dim3(blocks),
                       dim3(TK_THREADS), 0, st, a);
  });
}

static const char* ivf_check(int64_t M, int nprobe, int k, int64_t L) {
  if (M < 1) return "M must be >= 1";
  if (nprobe < 1 || nprobe > IVF_MAX_PROBE) return "nprobe must be in [1, 64]";
  if (k < 1 || k > TT_TOPK_MAX_K) return "k must be in [1, TT_TOPK_MAX_K = 256]";
  if (L < 1 || L > IVF_MAX_L) return "L must be in [1, 2^20]";
  if (M >= ((int64_t)1 << 31) / nprobe) return "M * nprobe must be < 2^31";
  return nullptr;
}

// ---- the item mask in list order ---------------------------------------------------------------

constexpr int IVF_MASK_LISTS_PER_WG = 32;  // one word of list_allow per workgroup

// row_allow: a lane per packed row, a wave per two words. Bit p = the row's label is an item in
// [0, N) whose bit in `allow` is set; rows past P are no rows. Every word is written.
__global__ void __launch_bounds__(256) ivf_row_allow_kernel(const uint32_t* __restrict__ allow, int64_t N,
                                                            const int32_t* __restrict__ labels, int64_t P,
                                                            uint32_t* __restrict__ row_allow) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool ok = false;
  if (p < P) {
    const int n = labels[p];
    if (n >= 0 && (int64_t)n < N) ok = (allow[n >> 5] >> (n & 31)) & 1u;
  }
  const u64 bits = __ballot(ok);
  const int lane = threadIdx.x & 63;
  const int64_t wd = (p >> 6) * 2 + (lane >> 5), words = (P + 31) >> 5;
  if ((lane & 31) == 0 && wd < words) row_allow[wd] = (uint32_t)(bits >> (lane & 32));
}

// list_eligible / list_allow from row_allow: a workgroup per 32 lists (one word of list_allow), each of
// its 4 waves counts 8 of them, a lane per word of the list's rows; integer sums, so any order gives
// the same count. A list that does not lie within the P rows has no eligible row (ivf_scan_kernel).
__global__ void __launch_bounds__(TK_THREADS) ivf_list_eligible_kernel(const uint32_t* __restrict__ row_allow,
                                                                       int64_t P,
                                                                       const int64_t* __restrict__ list_begin,
                                                                       const int32_t* __restrict__ list_len, int L,
                                                                       int32_t* __restrict__ list_eligible,
                                                                       uint32_t* __restrict__ list_allow) {
  __shared__ int cnt_s[IVF_MASK_LISTS_PER_WG];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  constexpr int PER_WAVE = IVF_MASK_LISTS_PER_WG / TK_WAVES;
  for (int i = 0; i < PER_WAVE; ++i) {
    const int j = wid * PER_WAVE + i;
    const int l = (int)blockIdx.x * IVF_MASK_LISTS_PER_WG + j;
    int cnt = 0;
    if (l < L) {
      int64_t beg = list_begin[l];
      int len = list_len[l];
      if (len < 0 || beg < 0 || beg > P || (int64_t)len > P - beg) len = 0;
      if (len > 0) {
        const int64_t end = beg + len;  // <= P: the words below are within ceil(P / 32)
        const int64_t w0 = beg >> 5, w1 = (end - 1) >> 5;
        for (int64_t wd = w0 + lane; wd <= w1; wd += 64) {
          uint32_t x = row_allow[wd];
          if (wd == w0) x &= 0xffffffffu << (beg & 31);
          if (wd == w1) x &= 0xffffffffu >> (31 - ((end - 1) & 31));
          cnt += __popc(x);
        }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
      if (lane == 0) list_eligible[l] = cnt;
    }
    if (lane == 0) cnt_s[j] = cnt;
  }
  __syncthreads();
  if (wid == 0) {
    const u64 bits = __ballot(lane < IVF_MASK_LISTS_PER_WG && cnt_s[lane & (IVF_MASK_LISTS_PER_WG - 1)] > 0);
    if (lane == 0) list_allow[blockIdx.x] = (uint32_t)bits;
  }
}

// ---- the centroid update -----------------------------------------------------------------------

// out[l] = mean of rows[order[i]], i in [seg[l], seg[l + 1]): one workgroup per segment, G = 256 / E
// row groups (group g sums the segment's positions g, g + G, ... in ascending order), the groups'
// sums added in ascending g, then one division: every element is summed in one fixed order
__global__ void __launch_bounds__(256) ivf_segment_mean_kernel(const void* __restrict__ rows, int is_bf16, int64_t ld,
                                                               int64_t n, int E, const int64_t* __restrict__ order,
                                                               const int64_t* __restrict__ seg,
                                                               float* __restrict__ out) {
  __shared__ float part[256];
  const int64_t l = blockIdx.x;
  int64_t beg = seg[l], end = seg[l + 1];
  if (beg < 0) beg = 0;
  if (end > n) end = n;
  if (end <= beg) return;  // an empty segment leaves out[l] as it is
  const int tid = threadIdx.x;
  const int cols = E < 256 ? E : 256, G = 256 / cols;
  const int grp = tid / cols, col = tid - grp * cols;
  for (int e0 = 0; e0 < E; e0 += cols) {
    const int e = e0 + col;
    float s = 0.f;
    if (grp < G && e < E) {
      for (int64_t i = beg + grp; i < end; i += G) {
        const int64_t r = order[i];
        if ((uint64_t)r >= (uint64_t)n) continue;  // no such row
        const int64_t o = r * ld + e;
        s += is_bf16 ? __uint_as_float(((uint32_t) reinterpret_cast<const unsigned short*>(rows)[o]) << 16)
                     : reinterpret_cast<const float*>(rows)[o];
      }
    }
    part[tid] = s;
    __syncthreads();
    if (grp == 0 && e < E) {
      float t = part[col];
      for (int g = 1; g < G; ++g) t += part[g * cols + col];
      out[l * E + e] = t / (float)(end - beg);
    }
    __syncthreads();
  }
}

}  // namespace tt

extern "C" {

size_t tt_ivf_scan_workspace_bytes(int64_t M, int nprobe, int k, int64_t L) {
  if (tt::ivf_check(M, nprobe, k, L)) return 0;
  return tt::ivf_ws_layout(M * nprobe, k, L, nullptr, nullptr);
}

}  // extern "C"

namespace tt {

// tt_ivf_scan (row_allow NULL, masked false) and tt_ivf_scan_masked
static int ivf_scan_impl(const char* name, bool masked, const void* queries, int q_dtype, int64_t ldq, int64_t M, int E,
                         const void* rows, const float* bias, const int32_t* labels, int64_t P,
                         const int64_t* list_begin, const int32_t* list_len, int64_t L, const int32_t* probes,
                         int nprobe, const int32_t* excl_values, const int64_t* excl_offsets,
                         const uint32_t* row_allow, int k, int64_t* ids, float* scores, void* workspace,
                         size_t ws_bytes, void* stream) {
  const std::string fn = std::string(name) + ": ";
  if (E < 32 || E > 128 || (E & 31)) return fail(TT_EINVAL, fn + "E must be a multiple of 32 in [32, 128]");
  if (const char* msg = ivf_check(M, nprobe, k, L)) return fail(TT_EINVAL, fn + msg);
  if (P < 1 || P >= (int64_t)1 << 31) return fail(TT_EINVAL, fn + "P must be in [1, 2^31)");
  if (q_dtype != TT_F32 && q_dtype != TT_BF16) return fail(TT_EINVAL, fn + "q_dtype must be TT_F32 or TT_BF16");
  if (ldq < E) return fail(TT_EINVAL, fn + "ldq must be >= E");
  if (!queries || !rows || !labels || !list_begin || !list_len || !probes || !ids || !scores || !workspace)
    return fail(TT_EINVAL, fn + "null queries / rows / labels / list_begin / list_len / probes / ids / scores / workspace");
  if (masked && !row_allow) return fail(TT_EINVAL, fn + "null row_allow");
  if ((excl_values == nullptr) != (excl_offsets == nullptr))
    return fail(TT_EINVAL, fn + "excl_values and excl_offsets must both be NULL or both be given");
  if (reinterpret_cast<uintptr_t>(rows) & 15) return fail(TT_EINVAL, fn + "rows must be 16-byte aligned");
  const int64_t PN = M * nprobe;
  IvfWs w;
  if (ws_bytes < ivf_ws_layout(PN, k, L, workspace, &w))
    return fail(TT_EINVAL, fn + "ws_bytes is smaller than tt_ivf_scan_workspace_bytes");
  hipStream_t st = as_stream(stream);

  // grouping: count, scan, scatter
  if (hipMemsetAsync(w.cnt, 0, (size_t)L * 8, st) != hipSuccess) return check_launch((fn + "memset").c_str());
  const unsigned pblocks = (unsigned)ceil_div(PN, 256);
  hipLaunchKernelGGL(ivf_count_kernel, dim3(pblocks), dim3(256), 0, st, probes, PN, (int)L, w.cnt);
  hipLaunchKernelGGL(ivf_offsets_kernel, dim3(1), dim3(IVF_SCAN_THREADS), 0, st, w.cnt, (int)L, w.list_off, w.tile_off);
  hipLaunchKernelGGL(ivf_scatter_kernel, dim3(pblocks), dim3(256), 0, st, probes, PN, nprobe, (int)L, w.list_off,
                     w.cursor, w.pair_query, w.slot_of);
  if (int rc = check_launch((fn + "grouping").c_str())) return rc;

  IvfMaskArgs a{};
  a.q = queries;
  a.rows = reinterpret_cast<const unsigned short*>(rows);
  a.bias = bias;
  a.labels = labels;
  a.list_begin = list_begin;
  a.list_len = list_len;
  a.list_off = w.list_off;
  a.tile_off = w.tile_off;
  a.pair_query = w.pair_query;
  a.ws = w.lists;
  a.excl_values = excl_values;
  a.excl_offsets = excl_offsets;
  a.ldq = ldq;
  a.M = M;
  a.P = P;
  a.k = k;
  a.L = (int)L;
  a.q_bf16 = q_dtype == TT_BF16;
  a.row_allow = row_allow;
  // an upper bound of sum_l ceil(cnt_l / 128): full tiles, plus one partial tile per probed list
  const unsigned blocks = (unsigned)(ceil_div(PN, TK_QB) + std::min<int64_t>(L, PN));
  if (masked) {
    if (excl_offsets)
      ivf_launch<true, true>(a, E, blocks, st);
    else
      ivf_launch<false, true>(a, E, blocks, st);
  } else {
    if (excl_offsets)
      ivf_launch<true, false>(a, E, blocks, st);
    else
      ivf_launch<false, false>(a, E, blocks, st);
  }
  if (int rc = check_launch((fn + "list scan").c_str())) return rc;
  hipLaunchKernelGGL(ivf_merge_kernel, dim3((unsigned)ceil_div(M, TK_WAVES)), dim3(TK_THREADS), 0, st, w.lists,
                     w.slot_of, M, nprobe, k, ids, scores);
  return check_launch((fn + "merge").c_str());
}

}  // namespace tt

extern "C" {

int tt_ivf_scan(const void* queries, int q_dtype, int64_t ldq, int64_t M, int E, const void* rows, const float* bias,
                const int32_t* labels, int64_t P, const int64_t* list_begin, const int32_t* list_len, int64_t L,
                const int32_t* probes, int nprobe, const int32_t* excl_values, const int64_t* excl_offsets, int k,
                int64_t* ids, float* scores, void* workspace, size_t ws_bytes, void* stream) {
  return tt::ivf_scan_impl("tt_ivf_scan", false, queries, q_dtype, ldq, M, E, rows, bias, labels, P, list_begin,
                           list_len, L, probes, nprobe, excl_values, excl_offsets, nullptr, k, ids, scores, workspace,
                           ws_bytes, stream);
}

int tt_ivf_scan_masked(const void* queries, int q_dtype, int64_t ldq, int64_t M, int E, const void* rows,
                       const float* bias, const int32_t* labels, int64_t P, const int64_t* list_begin,
                       const int32_t* list_len, int64_t L, const int32_t* probes, int nprobe,
                       const int32_t* excl_values, const int64_t* excl_offsets, const uint32_t* row_allow, int k,
                       int64_t* ids, float* scores, void* workspace, size_t ws_bytes, void* stream) {
  return tt::ivf_scan_impl("tt_ivf_scan_masked", true, queries, q_dtype, ldq, M, E, rows, bias, labels, P, list_begin,
                           list_len, L, probes, nprobe, excl_values, excl_offsets, row_allow, k, ids, scores, workspace,
                           ws_bytes, stream);
}

int tt_ivf_mask_lists(const uint32_t* allow, int64_t N, const int32_t* labels, int64_t P, const int64_t* list_begin,
                      const int32_t* list_len, int64_t L, uint32_t* row_allow, uint32_t* list_allow,
                      int32_t* list_eligible, void* stream) {
  using namespace tt;
  const std::string fn = "tt_ivf_mask_lists: ";
  if (N < 1 || N >= (int64_t)1 << 31) return fail(TT_EINVAL, fn + "N must be in [1, 2^31)");
  if (P < 1 || P >= (int64_t)1 << 31) return fail(TT_EINVAL, fn + "P must be in [1, 2^31)");
  if (L < 1 || L > IVF_MAX_L) return fail(TT_EINVAL, fn + "L must be in [1, 2^20]");
  if (!allow || !labels || !list_begin || !list_len || !row_allow || !list_allow || !list_eligible)
    return fail(TT_EINVAL, fn + "null allow / labels / list_begin / list_len / row_allow / list_allow / list_eligible");
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(ivf_row_allow_kernel, dim3((unsigned)ceil_div(P, 256)), dim3(256), 0, st, allow, N, labels, P,
                     row_allow);
  hipLaunchKernelGGL(ivf_list_eligible_kernel, dim3((unsigned)ceil_div(L, IVF_MASK_LISTS_PER_WG)), dim3(TK_THREADS), 0,
                     st, row_allow, P, list_begin, list_len, (int)L, list_eligible, list_allow);
  return check_launch("tt_ivf_mask_lists");
}

int tt_ivf_segment_mean(const void* rows, int dtype, int64_t ld, int64_t n, int E, const int64_t* order,
                        const int64_t* seg_offsets, int64_t L, float* out, void* stream) {
  using namespace tt;
  const std::string fn = "tt_ivf_segment_mean: ";
  if (dtype != TT_F32 && dtype != TT_BF16) return fail(TT_EINVAL, fn + "dtype must be TT_F32 or TT_BF16");
  if (E < 1 || E > 4096) return fail(TT_EINVAL, fn + "E must be in [1, 4096]");
  if (ld < E) return fail(TT_EINVAL, fn + "ld must be >= E");
  if (n < 1) return fail(TT_EINVAL, fn + "n must be >= 1");
  if (L < 1 || L > IVF_MAX_L) return fail(TT_EINVAL, fn + "L must be in [1, 2^20]");
  if (!rows || !order || !seg_offsets || !out) return fail(TT_EINVAL, fn + "null rows / order / seg_offsets / out");
  hipLaunchKernelGGL(ivf_segment_mean_kernel, dim3((unsigned)L), dim3(256), 0, as_stream(stream), rows,
                     dtype == TT_BF16 ? 1 : 0, ld, n, E, order, seg_offsets, out);
  return check_launch("tt_ivf_segment_mean");
}

}  // extern "C"
