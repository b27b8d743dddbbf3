// Exact top-k maximum-inner-product retrieval on gfx950 (tt_topk_mips): the scores of a query
// tile against a stream of items on bf16 MFMA (v_mfma_f32_16x16x32_bf16, fp32 accumulate) with the
// selection fused behind it, so a score leaves the registers only when it is a candidate.
// Replaces the vector-index query loop of 04_evaluate_retrieval.py:131-153.
//
//   grid = query tiles (128 queries) x item splits; 256 threads, each wave owns 32 queries
//   (2 tiles of 16) whose fragments stay in registers as the MFMA's B operand; the workgroup stages
//   chunks of 128 items (64 when E > 64) of its split through LDS (converted to bf16 once,
//   double-buffered, the next chunk's global loads in flight during the compute, one barrier per
//   chunk) as the A operand. Accumulator layout: lane l holds query l & 15 against items
//   (l >> 4) * 4 + r, so the running k-th-best threshold of a tile is ONE register per lane and the
//   filter is max3 + max + compare per 4 scores.
//
// Every entry (score, index) is one 64-bit key whose unsigned order is the total order "higher
// score first, equal scores by lower index": key = orderable(score) << 32 | ~index. A score that
// beats its query's threshold is appended to the query's candidate buffer in LDS (32 keys); a
// buffer that the next tile's candidates do not fit in is merged into the query's sorted partial
// list (k keys, in the workspace, read and written by the owning wave only) by rank counting,
// which raises the threshold. Items are streamed in ascending index order, so "score > threshold"
// (strict) loses nothing: an equal score met later has a higher index than everything in the list.
// A second kernel merges the S splits' sorted lists of a query (one lane per split, k rounds of a
// wave-wide max).
//
// The score of a pair is the MFMA chain over E in ascending k-steps from a zero accumulator, then
// + bias: a function of the two rows' bf16 values and bias[n] only, so the result (unique under the
// total order) is bit-identical across runs, M, N and split counts.
//
// tt_topk_mips_filtered runs the FILT instantiations of the same kernel: the top k over each query's
// ELIGIBLE items. The item mask shared by all queries (a bit per item) is staged per chunk beside the
// bias and decides, with the threshold, what becomes a candidate. A query's exclusion list (ascending
// item indices) is tested where it is cheap: not per candidate, but when the query's candidate
// buffer is about to be merged into its list (topk_drop_excluded: one lane per buffered key, a binary
// search each). Thresholds rise only in a merge and the final flush merges too, so an excluded key
// never raises a threshold, never enters a list and never displaces an eligible item; all it costs
// is its place in the buffer until the next merge. The unfiltered instantiations are unchanged.
#include "tt_common.h"
#include "topk_common.h"

#include <limits>
#include <type_traits>

namespace tt {

struct TopkArgs {
  const void* q;
  const void* c;
  const float* bias;
  u64* ws;  // [S][M][k] keys, each list sorted descending, 0 = no entry
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

template <int KS, bool BIAS, bool FILT>
__global__ void __launch_bounds__(TK_THREADS, 2)
    topk_mips_kernel(const std::conditional_t<FILT, TopkFiltArgs, TopkArgs> a) {
  constexpr int E = KS * 32, STRIDE = E + 8, GPR = E / 8;  // GPR: 8-element groups per item row
  constexpr int TK_IC = tk_chunk(E);
  constexpr int GPT = TK_IC * GPR / TK_THREADS;             // groups per thread
  __shared__ __attribute__((aligned(16))) __bf16 items[2][TK_IC * STRIDE];
  // FILT: the chunk's TK_IC / 32 mask words follow its bias
  __shared__ __attribute__((aligned(16))) float bias_s[2][TK_IC + (FILT ? TK_IC / 32 : 0)];
  __shared__ u64 cbuf_s[TK_WAVES][TK_QW * TK_CB];
  __shared__ u64 lscr_s[TK_WAVES][TT_TOPK_MAX_K];
  __shared__ int ccnt_s[TK_WAVES][TK_QW];
  __shared__ int lcnt_s[TK_WAVES][TK_QW];
  __shared__ float thrs_s[TK_WAVES][TK_QW];

  // workgroups of one item split are consecutive in the logical order, and an XCD runs a contiguous
  // part of it: the split's item stream is read from HBM once and shared through that XCD's L2
  const int logical = xcd_remap((int)blockIdx.x, (int)gridDim.x);
  const int split = logical / a.qtiles, qtile = logical - split * a.qtiles;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int64_t n_beg = (int64_t)split * a.per;
  const int64_t n_end = n_beg + a.per < a.N ? n_beg + a.per : a.N;
  const int nchunks = n_end > n_beg ? (int)((n_end - n_beg + TK_IC - 1) / TK_IC) : 0;
  const int64_t m_wave = (int64_t)qtile * TK_QB + wid * TK_QW;
  const int k = a.k;

  const WaveSel w{cbuf_s[wid], lscr_s[wid], ccnt_s[wid], lcnt_s[wid], thrs_s[wid]};
  for (int i = lane; i < TK_QW * TK_CB; i += 64) w.cbuf[i] = 0ull;
  if (lane < TK_QW) {
    w.ccnt[lane] = 0;
    w.lcnt[lane] = 0;
    w.thrs[lane] = m_wave + lane < a.M ? -std::numeric_limits<float>::infinity() : std::numeric_limits<float>::infinity();
  }
  // FILT: does any of the wave's queries have a non-empty exclusion segment (offsets never decrease)?
  // Where none has, the merges go as in the unfiltered kernel, without the look at the offsets
  bool wave_excl = false;
  if constexpr (FILT) {
    if (a.excl_offsets && m_wave < a.M) {
      const int64_t m_last = m_wave + TK_QW < a.M ? m_wave + TK_QW : a.M;
      wave_excl = __builtin_amdgcn_readfirstlane((int)(a.excl_offsets[m_last] > a.excl_offsets[m_wave])) != 0;
    }
  }

  // the wave's queries as B operands: lane l holds query (l & 15), k = 32 ks + 8 (l >> 4) + j
  bf16x8 qf[2][KS];
  float thr[2];
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    const int64_t m = m_wave + qt * 16 + (lane & 15);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      bf16x8 f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float x = 0.f;
        if (m < a.M) {
          const int64_t o = m * a.ldq + ks * 32 + (lane >> 4) * 8 + j;
          x = a.q_bf16 ? __uint_as_float(((uint32_t) reinterpret_cast<const unsigned short*>(a.q)[o]) << 16)
                       : reinterpret_cast<const float*>(a.q)[o];
        }
        f[j] = (__bf16)x;
      }
      qf[qt][ks] = f;
    }
    thr[qt] = m < a.M ? -std::numeric_limits<float>::infinity() : std::numeric_limits<float>::infinity();
  }
  wave_sync();

  // staging: thread t holds 8-element groups g = t + TK_THREADS i of the chunk: item row g / GPR
  const bool raw_bf16 = a.c_bf16 && a.c_vec;
  f32x4 rawf[GPT][2];
  bf16x8 rawb[GPT];
  float rawbias = 0.f;
  uint32_t rawmask = 0u;
  auto load_chunk = [&](int c) {
    const int64_t n0 = n_beg + (int64_t)c * TK_IC;
#pragma unroll
    for (int i = 0; i < GPT; ++i) {
      const int g = tid + TK_THREADS * i;
      const int row = g / GPR, kc = (g - row * GPR) * 8;
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
    if (BIAS && tid < TK_IC) rawbias = n0 + tid < n_end ? a.bias[n0 + tid] : 0.f;
    if constexpr (FILT) {
      // n0 is a multiple of the chunk, the chunk of 32: the chunk's words are whole
      if (tid < TK_IC / 32) {
        const int64_t wd = (n0 >> 5) + tid;
        rawmask = !a.allow ? 0xffffffffu : wd < ((a.N + 31) >> 5) ? a.allow[wd] : 0u;
      }
    }
  };
  auto store_chunk = [&](int buf) {
#pragma unroll
    for (int i = 0; i < GPT; ++i) {
      const int g = tid + TK_THREADS * i;
      const int row = g / GPR, kc = (g - row * GPR) * 8;
      bf16x8 o;
      if (raw_bf16) {
        o = rawb[i];
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (__bf16)rawf[i][j >> 2][j & 3];  // round-to-nearest-even
      }
      *reinterpret_cast<bf16x8*>(&items[buf][row * STRIDE + kc]) = o;
    }
    if (BIAS && tid < TK_IC) bias_s[buf][tid] = rawbias;
    if constexpr (FILT) {
      if (tid < TK_IC / 32) *reinterpret_cast<uint32_t*>(&bias_s[buf][TK_IC + tid]) = rawmask;
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
#pragma unroll 1
    for (int it = 0; it < TK_IC / 16; ++it) {
      bf16x8 af[KS];
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
        af[ks] = *reinterpret_cast<const bf16x8*>(&items[buf][(it * 16 + (lane & 15)) * STRIDE + ks * 32 + (lane >> 4) * 8]);
      f32x4 bv = (f32x4)(0.f);
      if (BIAS) bv = *reinterpret_cast<const f32x4*>(&bias_s[buf][it * 16 + (lane >> 4) * 4]);
      // FILT: the chunk's mask word it >> 1, read with the tile's other LDS reads: not one more
      // latency inside the candidate branch
      uint32_t mword = 0u;
      if constexpr (FILT) mword = *reinterpret_cast<const uint32_t*>(&bias_s[buf][TK_IC + (it >> 1)]);
#pragma unroll
      for (int qt = 0; qt < 2; ++qt) {
        f32x4 acc = (f32x4)(0.f);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[ks], qf[qt][ks], acc, 0, 0, 0);
        if (BIAS) acc += bv;
        const float mx = fmaxf(fmaxf(acc[0], acc[1]), fmaxf(acc[2], acc[3]));
        if (__ballot(mx > thr[qt]) != 0ull) {
          // candidates of this tile, decided against the threshold as it stood before the tile
          const int q = qt * 16 + (lane & 15);
          const int64_t nb = n0 + it * 16 + (lane >> 4) * 4;
          bool pass[4];
          int cnt = 0;
          // FILT: the lane's 4 items are bits (it & 1) * 16 + (lane >> 4) * 4 + r of the word. The
          // empty asm keeps the shift and the bit tests here: the compiler otherwise hoists them
          // (9 VALU instructions) into every tile, candidates or not
          uint32_t mbits = 0xfu;
          if constexpr (FILT) {
            uint32_t mw = mword;
            asm volatile("" : "+v"(mw));
            mbits = mw >> ((it & 1) * 16 + (lane >> 4) * 4);
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            pass[r] = acc[r] > thr[qt] && nb + r < n_end;
            if constexpr (FILT) pass[r] = pass[r] && ((mbits >> r) & 1u);
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
            if constexpr (FILT) {
              if (wave_excl && topk_drop_excluded(w, qi, a.excl_values, a.excl_offsets + m_wave + qi, lane) == 0)
                continue;  // nothing left to merge, and the buffer is empty
            }
            topk_merge_query(w, qi, a.ws + ((int64_t)split * a.M + m_wave + qi) * k, k, lane);
          }
          if (merged) base = w.ccnt[q];
          int slot = base + ex;
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (pass[r]) w.cbuf[q * TK_CB + slot++] = make_key(acc[r], (int)(nb + r));
          if (lane < 16 && tot > 0) w.ccnt[q] = base + tot;
          lds_wave_sync();
          if (merged) thr[qt] = w.thrs[q];
        }
      }
    }
    if (c + 1 < nchunks) store_chunk(buf ^ 1);
    __syncthreads();
  }

  // flush the buffers; pad the lists shorter than k
#pragma unroll 1
  for (int q = 0; q < TK_QW; ++q) {
    if (m_wave + q >= a.M) break;
    u64* gl = a.ws + ((int64_t)split * a.M + m_wave + q) * k;
    if constexpr (FILT) {
      if (w.ccnt[q] > 0 && wave_excl) topk_drop_excluded(w, q, a.excl_values, a.excl_offsets + m_wave + q, lane);
    }
    if (w.ccnt[q] > 0) topk_merge_query(w, q, gl, k, lane);
    for (int i = w.lcnt[q] + lane; i < k; i += 64) gl[i] = 0ull;
  }
}

// ids / scores [M][k] from the S sorted lists of each query: one wave per query, lane j walks
// split j's list; k rounds of a wave-wide max over the heads
__global__ void __launch_bounds__(TK_THREADS) topk_merge_kernel(const u64* __restrict__ ws, int64_t M, int k, int S,
                                                                int64_t* __restrict__ ids, float* __restrict__ scores) {
  const int lane = threadIdx.x & 63;
  const int64_t m = (int64_t)blockIdx.x * TK_WAVES + (threadIdx.x >> 6);
  if (m >= M) return;
  const u64* base = ws + ((int64_t)(lane < S ? lane : 0) * M + m) * k;
  int p = 0;
  u64 head = lane < S ? base[0] : 0ull;
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

static int topk_auto_splits(int64_t M, int64_t N) {
  // 8 waves per CU (every workgroup resident at once) when the queries alone do not give them: every split
  // starts its thresholds afresh, so more splits than that only add candidates; a split keeps
  // >= 512 items
  const int64_t qtiles = ceil_div(M, TK_QB);
  int64_t s = ceil_div(256 * (8 / TK_WAVES), qtiles);
  s = std::min<int64_t>(s, ceil_div(N, 512));
  return (int)std::max<int64_t>(1, std::min<int64_t>(s, TK_MAX_SPLITS));
}

static const char* topk_check(int64_t M, int64_t N, int k, int splits) {
  if (M < 1 || M > (int64_t)1 << 30) return "M must be in [1, 2^30]";
  if (N < 1 || N >= (int64_t)1 << 31) return "N must be in [1, 2^31)";
  if (k < 1 || k > TT_TOPK_MAX_K) return "k must be in [1, TT_TOPK_MAX_K = 256]";
  if (splits < 0 || splits > TK_MAX_SPLITS) return "splits must be 0 (chosen by the library) or in [1, 64]";
  return nullptr;
}

template <int KS, bool FILT>
static void topk_launch(const TopkFiltArgs& a, int blocks, hipStream_t st) {
  const std::conditional_t<FILT, TopkFiltArgs, TopkArgs>& ka = a;
  if (a.bias)
    hipLaunchKernelGGL((topk_mips_kernel<KS, true, FILT>), dim3(blocks), dim3(TK_THREADS), 0, st, ka);
  else
    hipLaunchKernelGGL((topk_mips_kernel<KS, false, FILT>), dim3(blocks), dim3(TK_THREADS), 0, st, ka);
}

template <bool FILT>
static void topk_launch_e(const TopkFiltArgs& a, int E, int blocks, hipStream_t st) {
  switch (E / 32) {
    case 1: topk_launch<1, FILT>(a, blocks, st); break;
    case 2: topk_launch<2, FILT>(a, blocks, st); break;
    case 3: topk_launch<3, FILT>(a, blocks, st); break;
    default: topk_launch<4, FILT>(a, blocks, st); break;
  }
}

// both entry points: `fn_name` prefixes the messages, `fn_merge` names the second launch; the FILT
// kernel runs when a filter is given
static int topk_run(const char* fn_name, const char* fn_merge, const void* queries, int q_dtype, int64_t ldq,
                    const void* items, int c_dtype, int64_t ldc, const float* bias, int64_t M, int64_t N, int E, int k,
                    int splits, const uint32_t* allow, const int32_t* excl_values, const int64_t* excl_offsets,
                    int64_t* ids, float* scores, void* workspace, size_t ws_bytes, void* stream) {
  const auto fn = [fn_name] { return std::string(fn_name); };  // built for a message only
  if (E < 32 || E > 128 || (E & 31)) return fail(TT_EINVAL, fn() + ": E must be a multiple of 32 in [32, 128]");
  if (const char* msg = topk_check(M, N, k, splits)) return fail(TT_EINVAL, fn() + ": " + msg);
  if ((q_dtype != TT_F32 && q_dtype != TT_BF16) || (c_dtype != TT_F32 && c_dtype != TT_BF16))
    return fail(TT_EINVAL, fn() + ": q_dtype / c_dtype must be TT_F32 or TT_BF16");
  if (ldq < E || ldc < E) return fail(TT_EINVAL, fn() + ": ldq / ldc must be >= E");
  if (!queries || !items || !ids || !scores || !workspace)
    return fail(TT_EINVAL, fn() + ": null queries / items / ids / scores / workspace");
  if ((excl_values == nullptr) != (excl_offsets == nullptr))
    return fail(TT_EINVAL, fn() + ": excl_values and excl_offsets must both be NULL or both be given");
  const int S = splits ? splits : topk_auto_splits(M, N);
  if (ws_bytes < (size_t)S * (size_t)M * (size_t)k * 8)
    return fail(TT_EINVAL, fn() + ": ws_bytes is smaller than tt_topk_mips_workspace_bytes");
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
  // 16-B loads of an item row's 8-element groups need the base and the row stride aligned
  a.c_vec = (reinterpret_cast<uintptr_t>(items) & 15) == 0 && (ldc % (a.c_bf16 ? 8 : 4)) == 0;
  a.allow = allow;
  a.excl_values = excl_values;
  a.excl_offsets = excl_offsets;
  const int blocks = (int)(qtiles * S);
  hipStream_t st = as_stream(stream);
  if (allow || excl_offsets)
    topk_launch_e<true>(a, E, blocks, st);
  else
    topk_launch_e<false>(a, E, blocks, st);
  if (int rc = check_launch(fn_name)) return rc;
  hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)ceil_div(M, TK_WAVES)), dim3(TK_THREADS), 0, st, a.ws, M, k, S,
                     ids, scores);
  return check_launch(fn_merge);
}

}  // namespace tt

extern "C" {

size_t tt_topk_mips_workspace_bytes(int64_t M, int64_t N, int k, int splits) {
  if (tt::topk_check(M, N, k, splits)) return 0;
  const int S = splits ? splits : tt::topk_auto_splits(M, N);
  return (size_t)S * (size_t)M * (size_t)k * 8;
}

int tt_topk_mips(const void* queries, int q_dtype, int64_t ldq, const void* items, int c_dtype, int64_t ldc,
                 const float* bias, int64_t M, int64_t N, int E, int k, int splits, int64_t* ids, float* scores,
                 void* workspace, size_t ws_bytes, void* stream) {
  return tt::topk_run("tt_topk_mips", "tt_topk_mips merge", queries, q_dtype, ldq, items, c_dtype, ldc, bias, M, N, E, k,
                      splits, nullptr, nullptr, nullptr, ids, scores, workspace, ws_bytes, stream);
}

int tt_topk_mips_filtered(const void* queries, int q_dtype, int64_t ldq, const void* items, int c_dtype, int64_t ldc,
                          const float* bias, int64_t M, int64_t N, int E, int k, int splits, const uint32_t* allow,
                          const int32_t* excl_values, const int64_t* excl_offsets, int64_t* ids, float* scores,
                          void* workspace, size_t ws_bytes, void* stream) {
  return tt::topk_run("tt_topk_mips_filtered", "tt_topk_mips_filtered merge", queries, q_dtype, ldq, items, c_dtype, ldc,
                      bias, M, N, E, k, splits, allow, excl_values, excl_offsets, ids, scores, workspace, ws_bytes, stream);
}

}  // extern "C"
