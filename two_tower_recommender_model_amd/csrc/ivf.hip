// IVF (inverted-file) approximate top-k retrieval on gfx950: tt_ivf_scan is the fine step, the top k
// of each query over the items of the lists it probes; tt_ivf_segment_mean is the deterministic
// centroid update of the k-means that builds the index. The coarse step ("nearest centroids of a
// query") is tt_topk_mips itself with the centroids as items.
//
// The index stores the item rows in list order (bf16, a list's rows contiguous, its original item
// indices `labels` ascending). A (query, probed list) PAIR is the unit of work: the pairs are grouped
// by list in the workspace (count, exclusive scan, scatter), so that a workgroup streams ONE list
// past a tile of up to 128 of the queries that probe it. From there it is the exact kernel's
// structure (retrieval.hip): each wave's 32 queries as MFMA B fragments in registers, the list's
// rows through double-buffered LDS chunks, v_mfma_f32_16x16x32_bf16 in ascending k-steps from a zero
// accumulator, + bias, the max3 + max + compare filter, a 32-key candidate buffer per query and the
// rank-counting merge into the pair's sorted partial list (k keys at ws + p * k). Keys carry the
// ORIGINAL item index (labels[n], loaded in the candidate branch), so the order "higher score, then
// lower original index" and the exclusion lists work on item indices; labels ascend within a list,
// so the strict compare against the threshold still loses nothing. A last kernel merges a query's
// up to 64 partial lists (one lane per probe, k rounds of a wave-wide max).
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
// chunk's bits are whole aligned words: they are loaded with the chunk's other global loads, staged
// beside its bias, read with the tile's other LDS reads and ANDed into the candidate test, as the
// exact kernel does with its mask. A denied row never enters a candidate buffer.
#include "tt_common.h"
#include "topk_common.h"

#include <limits>

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

template <int KS, bool BIAS, bool FILT, bool MASK>
__global__ void __launch_bounds__(TK_THREADS, 2)
    ivf_scan_kernel(const std::conditional_t<MASK, IvfMaskArgs, IvfArgs> a) {
  constexpr int E = KS * 32, STRIDE = E + 8, GPR = E / 8;  // GPR: 8-element groups per item row
  constexpr int TK_IC = tk_chunk(E);
  constexpr int GPT = TK_IC * GPR / TK_THREADS;             // groups per thread
  __shared__ __attribute__((aligned(16))) __bf16 items[2][TK_IC * STRIDE];
  __shared__ __attribute__((aligned(16))) float bias_s[2][TK_IC];
  __shared__ uint32_t mask_s[2][4];  // MASK: the chunk's TK_IC / 32 mask words (no LDS without MASK)
  __shared__ u64 cbuf_s[TK_WAVES][TK_QW * TK_CB];
  __shared__ u64 lscr_s[TK_WAVES][TT_TOPK_MAX_K];
  __shared__ int ccnt_s[TK_WAVES][TK_QW];
  __shared__ int lcnt_s[TK_WAVES][TK_QW];
  __shared__ float thrs_s[TK_WAVES][TK_QW];
  __shared__ int qid_s[TK_WAVES][TK_QW];  // the wave's pairs' queries, -1: no pair

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
  const int pw = max(0, min(TK_QW, p_end - p_wave));  // the wave's pairs: none in a tile's tail waves
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
  const int64_t n_end = n_beg + len;
  const int nchunks = (len + TK_IC - 1) / TK_IC;
  const int k = a.k;

  const WaveSel w{cbuf_s[wid], lscr_s[wid], ccnt_s[wid], lcnt_s[wid], thrs_s[wid]};
  int* qid = qid_s[wid];
  for (int i = lane; i < TK_QW * TK_CB; i += 64) w.cbuf[i] = 0ull;
  bool lane_excl = false;
  if (lane < TK_QW) {
    int m = lane < pw ? a.pair_query[p_wave + lane] : -1;
    if (m < 0 || m >= a.M) m = -1;
    qid[lane] = m;
    w.ccnt[lane] = 0;
    w.lcnt[lane] = 0;
    w.thrs[lane] = m >= 0 ? -std::numeric_limits<float>::infinity() : std::numeric_limits<float>::infinity();
    if constexpr (FILT) lane_excl = m >= 0 && a.excl_offsets[m + 1] > a.excl_offsets[m];
  }
  // FILT: does any of the wave's queries have a non-empty exclusion segment?
  const bool wave_excl = FILT && __ballot(lane_excl) != 0ull;
  // FILT + MASK: the exclusion values' address is held in vector registers, where the call of
  // topk_drop_excluded wants it anyway: with the mask the scalar registers do not suffice
  const int32_t* excl_values = a.excl_values;
  if constexpr (FILT && MASK) asm volatile("" : "+v"(excl_values));
  wave_sync();

  // the wave's queries as B operands: lane l holds query (l & 15), k = 32 ks + 8 (l >> 4) + j
  bf16x8 qf[2][KS];
  float thr[2];
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    const int64_t m = qid[qt * 16 + (lane & 15)];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      bf16x8 f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float x = 0.f;
        if (m >= 0) {
          const int64_t o = m * a.ldq + ks * 32 + (lane >> 4) * 8 + j;
          x = a.q_bf16 ? __uint_as_float(((uint32_t) reinterpret_cast<const unsigned short*>(a.q)[o]) << 16)
                       : reinterpret_cast<const float*>(a.q)[o];
        }
        f[j] = (__bf16)x;
      }
      qf[qt][ks] = f;
    }
    thr[qt] = m >= 0 ? -std::numeric_limits<float>::infinity() : std::numeric_limits<float>::infinity();
  }

  // staging: thread t holds 8-element groups g = t + TK_THREADS i of the chunk: item row g / GPR.
  // The rows are bf16 already: 16-byte loads, stored as they are
  bf16x8 rawb[GPT];
  float rawbias = 0.f;
  uint32_t rawmask = 0u;
  // MASK: thread t stages word t % (TK_IC / 32) of a chunk (every thread one, without a branch: the
  // FILT instantiations have no scalar register left for one more saved exec mask). Its index within
  // the list's words (n_beg is a multiple of 32) is clamped to the list's last word: a word that
  // begins at or past n_end is not read and counts as zero
  constexpr int MW = TK_IC / 32;
  const int mask_i = tid & (MW - 1), mask_last = (len - 1) >> 5;
  const uint32_t* mask_p = nullptr;
  if constexpr (MASK) {
    mask_p = a.row_allow + (n_beg >> 5);
    asm volatile("" : "+v"(mask_p));  // held in vector registers, for the same reason
  }
  auto load_chunk = [&](int c) {
    const int64_t n0 = n_beg + (int64_t)c * TK_IC;
#pragma unroll
    for (int i = 0; i < GPT; ++i) {
      const int g = tid + TK_THREADS * i;
      const int row = g / GPR, kc = (g - row * GPR) * 8;
      const int64_t n = n0 + row;
      bf16x8 z;
#pragma unroll
      for (int j = 0; j < 8; ++j) z[j] = (__bf16)0.f;
      rawb[i] = n < n_end ? *reinterpret_cast<const bf16x8*>(a.rows + n * E + kc) : z;
    }
    if (BIAS && tid < TK_IC) rawbias = n0 + tid < n_end ? a.bias[n0 + tid] : 0.f;
    if constexpr (MASK) {
      const int wd = c * MW + mask_i;  // load_chunk runs only where len > 0: mask_last >= 0
      const uint32_t x = mask_p[min(wd, mask_last)];
      rawmask = wd <= mask_last ? x : 0u;
    }
  };
  auto store_chunk = [&](int buf) {
#pragma unroll
    for (int i = 0; i < GPT; ++i) {
      const int g = tid + TK_THREADS * i;
      const int row = g / GPR, kc = (g - row * GPR) * 8;
      *reinterpret_cast<bf16x8*>(&items[buf][row * STRIDE + kc]) = rawb[i];
    }
    if (BIAS && tid < TK_IC) bias_s[buf][tid] = rawbias;
    if constexpr (MASK) {
      mask_s[buf][mask_i] = rawmask;  // the threads of one word store the same value
    }
  };

  if (nchunks > 0) {
    load_chunk(0);
    store_chunk(0);
  }
  __syncthreads();

  for (int c = 0; c < nchunks; ++c) {
    const int buf = c & 1;
    if (c + 1 < nchunks) load_chunk(c + 1);
    const int64_t n0 = n_beg + (int64_t)c * TK_IC;
    // a wave with no pairs only helps to stage
    if (pw > 0) {
#pragma unroll 1
      for (int it = 0; it < TK_IC / 16; ++it) {
        bf16x8 af[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
          af[ks] = *reinterpret_cast<const bf16x8*>(&items[buf][(it * 16 + (lane & 15)) * STRIDE + ks * 32 + (lane >> 4) * 8]);
        f32x4 bv = (f32x4)(0.f);
        if (BIAS) bv = *reinterpret_cast<const f32x4*>(&bias_s[buf][it * 16 + (lane >> 4) * 4]);
        // MASK: the chunk's mask word it >> 1, read with the tile's other LDS reads: not one more
        // latency inside the candidate branch
        uint32_t mword = 0u;
        if constexpr (MASK) mword = mask_s[buf][it >> 1];
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) {
          f32x4 acc = (f32x4)(0.f);
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[ks], qf[qt][ks], acc, 0, 0, 0);
          if (BIAS) acc += bv;
          const float mx = fmaxf(fmaxf(acc[0], acc[1]), fmaxf(acc[2], acc[3]));
          if (__ballot(mx > thr[qt]) != 0ull) {
            // candidates of this tile, decided against the threshold as it stood before the tile;
            // rows past the list's end (its padding, the next list) are cut here
            const int q = qt * 16 + (lane & 15);
            const int64_t nb = n0 + it * 16 + (lane >> 4) * 4;
            bool pass[4];
            int cnt = 0;
            // MASK: the lane's 4 rows are bits (it & 1) * 16 + (lane >> 4) * 4 + r of the word. The
            // empty asm keeps the shift and the bit tests here, out of the tiles without candidates
            // (retrieval.hip)
            uint32_t mbits = 0xfu;
            if constexpr (MASK) {
              uint32_t mw = mword;
              asm volatile("" : "+v"(mw));
              mbits = mw >> ((it & 1) * 16 + (lane >> 4) * 4);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              pass[r] = acc[r] > thr[qt] && nb + r < n_end;
              if constexpr (MASK) pass[r] = pass[r] && ((mbits >> r) & 1u);
              cnt += pass[r] ? 1 : 0;
            }
            const int c16 = __shfl_xor(cnt, 16, 64);
            const int c32 = __shfl_xor(cnt + c16, 32, 64);
            const int tot = cnt + c16 + c32;
            const int ex = ((lane & 16) ? c16 : 0) + ((lane & 32) ? c32 : 0);
            int base = w.ccnt[q];
            // first merge the buffers they do not fit in
            u64 need = __ballot(lane < 16 && base + tot > TK_CB);
            const bool merged = need != 0ull;
            while (need) {
              const int qi = qt * 16 + __builtin_ctzll(need);
              need &= need - 1;
              if constexpr (FILT) {
                if (wave_excl) {
                  const int mq = __builtin_amdgcn_readfirstlane(qid[qi]);
                  if (topk_drop_excluded(w, qi, excl_values, a.excl_offsets + mq, lane) == 0)
                    continue;  // nothing left to merge, and the buffer is empty
                }
              }
              topk_merge_query(w, qi, a.ws + (int64_t)(p_wave + qi) * k, k, lane);
            }
            if (merged) base = w.ccnt[q];
            int slot = base + ex;
            // the key carries the item's original index
#pragma unroll
            for (int r = 0; r < 4; ++r)
              if (pass[r]) w.cbuf[q * TK_CB + slot++] = make_key(acc[r], a.labels[nb + r]);
            if (lane < 16 && tot > 0) w.ccnt[q] = base + tot;
            lds_wave_sync();
            if (merged) thr[qt] = w.thrs[q];
          }
        }
      }
    }
    if (c + 1 < nchunks) store_chunk(buf ^ 1);
    __syncthreads();
  }

  // flush the buffers; pad the lists shorter than k
#pragma unroll 1
  for (int q = 0; q < pw; ++q) {
    u64* gl = a.ws + (int64_t)(p_wave + q) * k;
    if constexpr (FILT) {
      if (w.ccnt[q] > 0 && wave_excl) {
        const int mq = __builtin_amdgcn_readfirstlane(qid[q]);
        if (mq >= 0) topk_drop_excluded(w, q, excl_values, a.excl_offsets + mq, lane);
      }
    }
    if (w.ccnt[q] > 0) topk_merge_query(w, q, gl, k, lane);
    for (int i = w.lcnt[q] + lane; i < k; i += 64) gl[i] = 0ull;
  }
}

// ids / scores [M][k] from the sorted lists of each query's pairs: one wave per query, lane j walks
// the list of the query's probe column j (no list where the probe was no probe); k rounds of a
// wave-wide max over the heads. The lists of distinct probes hold distinct items, so keys are distinct
__global__ void __launch_bounds__(TK_THREADS) ivf_merge_kernel(const u64* __restrict__ ws,
                                                               const int32_t* __restrict__ slot_of, int64_t M,
                                                               int nprobe, int k, int64_t* __restrict__ ids,
                                                               float* __restrict__ scores) {
  const int lane = threadIdx.x & 63;
  const int64_t m = (int64_t)blockIdx.x * TK_WAVES + (threadIdx.x >> 6);
  if (m >= M) return;
  const int slot = lane < nprobe ? slot_of[m * nprobe + lane] : -1;
  const u64* base = ws + (int64_t)(slot >= 0 ? slot : 0) * k;
  int p = 0;
  u64 head = slot >= 0 ? base[0] : 0ull;
  for (int i = 0; i < k; ++i) {
    u64 mx = head;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const u64 t = __shfl_xor(mx, o, 64);
      mx = t > mx ? t : mx;
    }
    if (lane == 0) {
      ids[m * k + i] = mx ? (int64_t)key_index(mx) : (int64_t)-1;
      scores[m * k + i] = mx ? key_score(mx) : -std::numeric_limits<float>::infinity();
    }
    if (mx != 0ull && head == mx) {
      ++p;
      head = p < k ? base[p] : 0ull;
    }
  }
}

template <int KS, bool FILT, bool MASK>
static void ivf_launch(const IvfMaskArgs& a, unsigned blocks, hipStream_t st) {
  if (a.bias)
    hipLaunchKernelGGL((ivf_scan_kernel<KS, true, FILT, MASK>), dim3(blocks), dim3(TK_THREADS), 0, st, a);
  else
    hipLaunchKernelGGL((ivf_scan_kernel<KS, false, FILT, MASK>), dim3(blocks), dim3(TK_THREADS), 0, st, a);
}

template <bool FILT, bool MASK>
static void ivf_launch_e(const IvfMaskArgs& a, int E, unsigned blocks, hipStream_t st) {
  switch (E / 32) {
    case 1: ivf_launch<1, FILT, MASK>(a, blocks, st); break;
    case 2: ivf_launch<2, FILT, MASK>(a, blocks, st); break;
    case 3: ivf_launch<3, FILT, MASK>(a, blocks, st); break;
    default: ivf_launch<4, FILT, MASK>(a, blocks, st); break;
  }
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
      ivf_launch_e<true, true>(a, E, blocks, st);
    else
      ivf_launch_e<false, true>(a, E, blocks, st);
  } else {
    if (excl_offsets)
      ivf_launch_e<true, false>(a, E, blocks, st);
    else
      ivf_launch_e<false, false>(a, E, blocks, st);
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
