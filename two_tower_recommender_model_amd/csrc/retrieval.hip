// Exact top-k maximum-inner-product retrieval on gfx950 (tt_topk_mips): the shared scan
// (topk_scan.h: the scores of a query tile against a stream of items on bf16 MFMA, the selection
// fused behind them) over the whole item table. Replaces the vector-index query loop of
// 04_evaluate_retrieval.py:131-153.
//
//   grid = query tiles (128 queries) x item splits; a workgroup streams its split's items (f32 or
//   bf16, converted to bf16 once on the way into LDS) past its query tile and leaves each query's
//   sorted partial list in the workspace ([S][M][k]). A second kernel merges the S splits' lists of
//   a query (one lane per split).
//
// tt_topk_mips_filtered runs the FILT instantiations: the top k over each query's ELIGIBLE items,
// with the item mask (`allow`, a bit per item) as the scan's row mask and the queries' exclusion
// lists. The unfiltered instantiations carry neither.
#include "tt_common.h"
#include "topk_exact.h"

namespace tt {

template <int KS, bool BIAS, bool FILT>
__global__ void __launch_bounds__(TK_THREADS, 2)
    topk_mips_kernel(const std::conditional_t<FILT, TopkFiltArgs, TopkArgs> a) {
  constexpr int TK_IC = ScanShape<KS>::IC;
  // workgroups of one item split are consecutive in the logical order, and an XCD runs a contiguous
  // part of it: the split's item stream is read from HBM once and shared through that XCD's L2
  const int logical = xcd_remap((int)blockIdx.x, (int)gridDim.x);
  const int split = logical / a.qtiles, qtile = logical - split * a.qtiles;
  const int64_t n_beg = (int64_t)split * a.per;
  const int64_t n_end = n_beg + a.per < a.N ? n_beg + a.per : a.N;
  const int nchunks = n_end > n_beg ? (int)((n_end - n_beg + TK_IC - 1) / TK_IC) : 0;
  const int64_t m_wave = (int64_t)qtile * TK_QB + (threadIdx.x >> 6) * TK_QW;
  // FILT: does any of the wave's queries have a non-empty exclusion segment (offsets never decrease)?
  // Where none has, the merges go as in the unfiltered kernel, without the look at the offsets
  bool wave_excl = false;
  const int32_t* excl_values = nullptr;
  if constexpr (FILT) {
    excl_values = a.excl_values;
    if (a.excl_offsets && m_wave < a.M) {
      const int64_t m_last = m_wave + TK_QW < a.M ? m_wave + TK_QW : a.M;
      wave_excl = __builtin_amdgcn_readfirstlane((int)(a.excl_offsets[m_last] > a.excl_offsets[m_wave])) != 0;
    }
  }
  // the wave's lists in [S][M][k]. FILT: the address is held in vector registers (as m_wave is): left
  // to itself the compiler keeps its scalar part in 5 more scalar registers across the scan, which
  // these instantiations do not have
  u64* lists = a.ws + ((int64_t)split * a.M + m_wave) * a.k;
  if constexpr (FILT) asm volatile("" : "+v"(lists));
  ExactSrc<KS, FILT> s{a, m_wave, lists, n_beg, n_end, nchunks, wave_excl, excl_values, a.c_bf16 && a.c_vec};
  topk_scan_body<KS, BIAS, FILT, FILT>(s);
}

// ids / scores [M][k] from the S sorted lists of each query: one wave per query, lane j walks
// split j's list
__global__ void __launch_bounds__(TK_THREADS) topk_merge_kernel(const u64* __restrict__ ws, int64_t M, int k, int S,
                                                                int64_t* __restrict__ ids, float* __restrict__ scores) {
  const int lane = threadIdx.x & 63;
  const int64_t m = (int64_t)blockIdx.x * TK_WAVES + (threadIdx.x >> 6);
  if (m >= M) return;
  topk_merge_lists(ws + ((int64_t)(lane < S ? lane : 0) * M + m) * k, lane < S, m, k, ids, scores);
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

template <bool FILT>
static void topk_launch(const TopkFiltArgs& a, int E, int blocks, hipStream_t st) {
  const std::conditional_t<FILT, TopkFiltArgs, TopkArgs>& ka = a;
  topk_dispatch(E, a.bias != nullptr, [&](auto ks, auto bias) {
    hipLaunchKernelGGL((topk_mips_kernel<decltype(ks)::value, decltype(bias)::value, FILT>), dim3(blocks),
                       dim3(TK_THREADS), 0, st, ka);
  });
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
    topk_launch<true>(a, E, blocks, st);
  else
    topk_launch<false>(a, E, blocks, st);
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
