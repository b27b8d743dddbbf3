// The scan shared by the exact top-k kernel (retrieval.hip) and the IVF list scan (ivf.hip): the
// scores of a wave's 32 queries against a stream of item rows on bf16 MFMA
// (v_mfma_f32_16x16x32_bf16, fp32 accumulate) with the selection fused behind it, so a score leaves
// the registers only when it is a candidate. Also the merge of a query's sorted partial lists and the
// launchers' dispatch over E and the bias.
//
//   256 threads; each wave owns 32 queries (2 tiles of 16) whose fragments stay in registers as the
//   MFMA's B operand; the workgroup stages chunks of 128 rows (64 when E > 64) of its item range
//   through LDS (bf16, double-buffered, the next chunk's global loads in flight during the compute,
//   one barrier per chunk) as the A operand. Accumulator layout: lane l holds query l & 15 against
//   rows (l >> 4) * 4 + r, so the running k-th-best threshold of a tile is ONE register per lane and
//   the filter is max3 + max + compare per 4 scores.
//
// Every entry (score, index) is one 64-bit key whose unsigned order is the total order "higher
// score first, equal scores by lower index": key = orderable(score) << 32 | ~index. A score that
// beats its query's threshold is appended to the query's candidate buffer in LDS (32 keys); a
// buffer that the next tile's candidates do not fit in is merged into the query's sorted partial
// list (k keys, in the workspace, read and written by the owning wave only) by rank counting,
// which raises the threshold. A source streams its rows in ascending index order, so "score >
// threshold" (strict) loses nothing: an equal score met later has a higher index than everything in
// the list.
//
// The score of a pair is the MFMA chain over E in ascending k-steps from a zero accumulator, then
// + bias: a function of the two rows' bf16 values and the row's bias only, so the result (unique
// under the total order) is bit-identical across runs, sources, tilings and split counts.
//
// MASK: a bit per row, shared by all queries, is staged per chunk (whole aligned words) and decides,
// with the threshold, what becomes a candidate: a denied row never enters a buffer. EXCL: a query's
// exclusion list (ascending item indices) is tested where it is cheap: not per candidate, but when
// the query's candidate buffer is about to be merged into its list (topk_drop_excluded: one lane
// per buffered key, a binary search each). Thresholds rise only in a merge and the final flush merges
// too, so an excluded key never raises a threshold, never enters a list and never displaces an
// eligible item; all it costs is its place in the buffer until the next merge.
//
// Where a full buffer goes is the scan's sink (ListSink below: the sorted partial list just described;
// PoolSink in topk_large.hip: an unsorted pool pruned by radix selection, for k up to 8192). The scan,
// the candidate path, the mask and the exclusion drop are the same for both.
//
// A source (ExactSrc in topk_exact.h, IvfSrc in ivf.hip) describes a workgroup's work unit:
//   a                     the kernel's arguments: q, ldq, q_bf16, bias, k, excl_offsets
//   n_beg, n_end, nchunks the item range [n_beg, n_end) and its chunks
//   computes()            false: the wave has no queries and only helps to stage
//   query(q)              the query of wave-local query q, -1: none
//   has_list(q), lists    q has a partial list (the wave's first so many have), at lists + q * k
//                         (the sink's layout: PoolSink's pools are 2 k + 32 keys apart)
//   wave_excl             EXCL: some query of the wave has a non-empty exclusion segment
//   excl_values, excl(q)  EXCL: the exclusion lists' values; q's two offsets into them
//   index(n)              the item index that row n's key carries
//   load_rows / store_rows   a chunk's rows: global -> the thread's registers -> LDS (bf16)
//   load_mask / store_mask   MASK: the same for the chunk's mask words
#pragma once

#include "topk_common.h"

#include <limits>
#include <type_traits>

namespace tt {

// the staged chunk of rows of E = 32 KS elements
template <int KS>
struct ScanShape {
  static constexpr int E = KS * 32, STRIDE = E + 8;  // STRIDE: a row in LDS
  static constexpr int GPR = E / 8;                  // 8-element groups per item row
  static constexpr int IC = tk_chunk(E);             // rows per chunk
  static constexpr int GPT = IC * GPR / TK_THREADS;  // groups per thread
  static constexpr int MW = IC / 32;                 // mask words per chunk
};

// The sink of the scan: what happens to a query's full candidate buffer (absorb: the buffer is empty
// afterwards and thrs[q] holds the new threshold) and what the final flush leaves in the workspace.
// `lists` is the wave's first query's storage. SCR: the 8-byte words of per-wave LDS scratch it
// needs (WaveSel::lscr). ListSink keeps a sorted list of k keys per query (k <= TT_TOPK_MAX_K);
// topk_large.hip has the sink for larger k
struct ListSink {
  static constexpr int SCR = TT_TOPK_MAX_K;
  static __device__ __forceinline__ void absorb(const WaveSel w, int q, u64* lists, int k, int lane) {
    topk_merge_query(w, q, lists + (int64_t)q * k, k, lane);
  }
  // merge what is buffered; pad a list shorter than k
  static __device__ __forceinline__ void flush(const WaveSel w, int q, u64* lists, int k, int lane) {
    u64* gl = lists + (int64_t)q * k;
    if (w.ccnt[q] > 0) topk_merge_query(w, q, gl, k, lane);
    for (int i = w.lcnt[q] + lane; i < k; i += 64) gl[i] = 0ull;
  }
};

template <int KS, bool BIAS, bool EXCL, bool MASK, class Sink = ListSink, class Src>
__device__ __forceinline__ void topk_scan_body(Src& s) {
  constexpr int STRIDE = ScanShape<KS>::STRIDE, TK_IC = ScanShape<KS>::IC;
  __shared__ __attribute__((aligned(16))) __bf16 items[2][TK_IC * STRIDE];
  __shared__ __attribute__((aligned(16))) float bias_s[2][TK_IC];
  __shared__ uint32_t mask_s[2][ScanShape<KS>::MW];  // MASK only (no LDS without it)
  __shared__ u64 cbuf_s[TK_WAVES][TK_QW * TK_CB];
  __shared__ u64 lscr_s[TK_WAVES][Sink::SCR];
  __shared__ int ccnt_s[TK_WAVES][TK_QW];
  __shared__ int lcnt_s[TK_WAVES][TK_QW];
  __shared__ float thrs_s[TK_WAVES][TK_QW];

  const auto& a = s.a;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int64_t n_beg = s.n_beg, n_end = s.n_end;
  const int nchunks = s.nchunks;
  const int k = a.k;

  const WaveSel w{cbuf_s[wid], lscr_s[wid], ccnt_s[wid], lcnt_s[wid], thrs_s[wid]};
  for (int i = lane; i < TK_QW * TK_CB; i += 64) w.cbuf[i] = 0ull;
  if (lane < TK_QW) {
    w.ccnt[lane] = 0;
    w.lcnt[lane] = 0;
    w.thrs[lane] = s.query(lane) >= 0 ? -std::numeric_limits<float>::infinity() : std::numeric_limits<float>::infinity();
  }

  // the wave's queries as B operands: lane l holds query (l & 15), k = 32 ks + 8 (l >> 4) + j
  bf16x8 qf[2][KS];
  float thr[2];
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    const int64_t m = s.query(qt * 16 + (lane & 15));
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
  wave_sync();

  float rawbias = 0.f;
  auto load_chunk = [&](int c) {
    const int64_t n0 = n_beg + (int64_t)c * TK_IC;
    s.load_rows(n0, tid);
    if (BIAS && tid < TK_IC) rawbias = n0 + tid < n_end ? a.bias[n0 + tid] : 0.f;
    if constexpr (MASK) s.load_mask(c, n0, tid);
  };
  auto store_chunk = [&](int buf) {
    s.store_rows(items[buf], tid);
    if (BIAS && tid < TK_IC) bias_s[buf][tid] = rawbias;
    if constexpr (MASK) s.store_mask(mask_s[buf], tid);
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
    if (s.computes()) {
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
            // rows past the range's end (zero rows, padding, another list) are cut here
            const int q = qt * 16 + (lane & 15);
            const int64_t nb = n0 + it * 16 + (lane >> 4) * 4;
            bool pass[4];
            int cnt = 0;
            // MASK: the lane's 4 rows are bits (it & 1) * 16 + (lane >> 4) * 4 + r of the word. The
            // empty asm keeps the shift and the bit tests here: the compiler otherwise hoists them
            // (9 VALU instructions) into every tile, candidates or not
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
            // the tile's candidates per query (its 4 lanes l, l ^ 16, l ^ 32, l ^ 48: at most 16) and
            // this lane's place among them
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
              if constexpr (EXCL) {
                if (s.wave_excl) {
                  if (topk_drop_excluded(w, qi, s.excl_values, s.excl(qi), lane) == 0)
                    continue;  // nothing left to merge, and the buffer is empty
                }
              }
              Sink::absorb(w, qi, s.lists, k, lane);
            }
            if (merged) base = w.ccnt[q];
            int slot = base + ex;
#pragma unroll
            for (int r = 0; r < 4; ++r)
              if (pass[r]) w.cbuf[q * TK_CB + slot++] = make_key(acc[r], s.index(nb + r));
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

  // flush the buffers
#pragma unroll 1
  for (int q = 0; q < TK_QW; ++q) {
    if (!s.has_list(q)) break;
    if constexpr (EXCL) {
      if (w.ccnt[q] > 0 && s.wave_excl) {
        if (s.query(q) >= 0) topk_drop_excluded(w, q, s.excl_values, s.excl(q), lane);
      }
    }
    Sink::flush(w, q, s.lists, k, lane);
  }
}

// ids / scores [k] of query m from its sorted partial lists, one wave: lane j walks its list `base`
// (k keys; `has` false: no list), k rounds of a wave-wide max over the heads. Keys of distinct lists
// are distinct
__device__ __forceinline__ void topk_merge_lists(const u64* __restrict__ base, bool has, int64_t m, int k,
                                                 int64_t* __restrict__ ids, float* __restrict__ scores) {
  const int lane = threadIdx.x & 63;
  int p = 0;
  u64 head = has ? base[0] : 0ull;
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

// f(KS, BIAS) with E / 32 and "a bias is given" as integral constants: the launchers' kernel choice
template <class F>
static void topk_dispatch(int E, bool bias, F f) {
  const auto with_ks = [&](auto ks) {
    if (bias)
      f(ks, std::true_type{});
    else
      f(ks, std::false_type{});
  };
  switch (E / 32) {
    case 1: with_ks(std::integral_constant<int, 1>{}); break;
    case 2: with_ks(std::integral_constant<int, 2>{}); break;
    case 3: with_ks(std::integral_constant<int, 3>{}); break;
    default: with_ks(std::integral_constant<int, 4>{}); break;
  }
}

}  // namespace tt
