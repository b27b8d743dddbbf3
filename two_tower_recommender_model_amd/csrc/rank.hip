// Full-catalogue target ranks on gfx950 (tt_target_ranks): for every (query, target item) pair the
// number of the query's eligible items that precede the target in the retrieval kernels' total order
// ("higher score first, equal scores by lower index"), without selecting a top-k list: no candidate
// buffers, no partial lists, no merges, no k-sized workspace. The rank is the target's column in
// tt_topk_mips_filtered's list for any k above it, so recall@k / nDCG@k for every k, MRR and the mean
// rank follow from one pass over the item table.
//
// Four launches on the caller's stream, nothing read back by the host:
//   1. rank_slabs_kernel   a query's T_m targets become ceil(T_m / 8) "virtual queries": the same
//                          query row with a slab of at most 8 targets (count, exclusive scan, fill;
//                          one workgroup). The same for the exclusion segments, in slabs of 16. The
//                          slab counts stay on the device; the later grids are sized to their bound
//                          and a workgroup past the count exits.
//   2. rank_pair_kernel    the scores of the (query, target) pairs and of every query's exclusion
//                          items: a wave holds up to 16 pairs as row i / column i of one 16x16 MFMA
//                          tile (the item row gathered as the A operand, its query as the B operand,
//                          the rounding and the chain of the scan) and keeps the tile's diagonal. The
//                          chain's output depends on its own row and column only, so these are the
//                          bits the scan computes for the pair wherever the row sits in a chunk.
//   3. rank_scan_kernel    the scan of topk_scan.h (256 threads, a wave's 32 virtual queries as B
//                          fragments, item chunks double-buffered through LDS by ExactSrc's loaders,
//                          bias and mask words staged with the chunk) with counters behind the MFMA
//                          in place of the selection: a lane holds its virtual query's 8 thresholds,
//                          target indices and counters and adds "this score precedes that target"
//                          for its 4 scores of a tile (over the 1, 2, 4 or 8 slots that the wave's
//                          queries use). Per-split partial counts go to [S][T_cap].
//   4. rank_finish_kernel  per target: the sum over the splits, minus the items of the query's
//                          exclusion segment that the scan counted (in range, allowed, distinct,
//                          preceding the target); -1 / -inf for an ineligible target.
//
// The compare of the scan's common path is one float compare per (score, target): items stream in
// ascending index order, so before the target's own row "precedes" is s >= t, after it s > t, and
// s >= t is s > pred(t) with pred(t) the next float below t (f32 denormals are kept: the kernels run
// in the default mode, and an MFMA result is never flushed). A lane's threshold per target starts as
// pred(t) and becomes t in the one 16-row tile that holds the target's row; that tile (found per
// chunk as a bit per tile) takes the exact path with the index rule.
#include "tt_common.h"
#include "topk_exact.h"

namespace tt {

constexpr int RK_R = 8;          // targets per virtual query: a lane's registers
constexpr int RK_XR = 16;        // exclusion items per slab: one pair tile
constexpr int RK_SLAB_THREADS = 1024;

struct RankSlab {
  int64_t first;  // position of the slab's first value
  int32_t q;      // its query
  int32_t n;      // values in the slab: 1..R
};

struct RankArgs {
  const void* q;
  const void* c;
  const float* bias;
  const int32_t* tv;
  const int64_t* to;
  const uint32_t* allow;
  const int32_t* xv;
  const int64_t* xo;
  int64_t* ranks;
  float* scores;
  // workspace
  int32_t* hdr;  // [0]: target slabs, [1]: exclusion slabs
  RankSlab* tslab;
  RankSlab* xslab;
  float* tscore;   // [T_cap] the targets' scores, +inf: index outside [0, N)
  float* xscore;   // [L_cap] the exclusion items' scores
  uint32_t* part;  // [S][T_cap] per-split counts
  int64_t ldq, ldc, M, N, per, T_cap, L_cap;
  int S, vtiles, tvmax, xvmax, q_bf16, c_bf16, c_vec, tblocks;
};

// query m's segment [beg, beg + n) of a jagged list of `cap` values; offsets that decrease or leave
// [0, cap] give an empty one
__device__ __forceinline__ int64_t rank_segment(const int64_t* __restrict__ off, int64_t m, int64_t cap, int64_t& beg) {
  const int64_t b = off[m], e = off[m + 1];
  beg = b;
  return (b >= 0 && e >= b && e <= cap) ? e - b : 0;
}

// workgroup 0: the target slabs, workgroup 1: the exclusion slabs. Thread t takes a contiguous run of
// queries: count, exclusive scan over the threads, fill. Slabs past the bound (overlapping segments:
// the sum of the lengths may exceed cap) are dropped
__global__ void __launch_bounds__(RK_SLAB_THREADS) rank_slabs_kernel(const RankArgs a) {
  __shared__ int64_t s_cnt[RK_SLAB_THREADS];
  const bool x = blockIdx.x != 0;
  const int64_t* off = x ? a.xo : a.to;
  const int64_t cap = x ? a.L_cap : a.T_cap;
  const int R = x ? RK_XR : RK_R;
  RankSlab* slabs = x ? a.xslab : a.tslab;
  const int64_t vmax = x ? a.xvmax : a.tvmax;
  const int tid = threadIdx.x;
  const int64_t per = (a.M + RK_SLAB_THREADS - 1) / RK_SLAB_THREADS;
  const int64_t lo = min(a.M, tid * per), hi = min(a.M, lo + per);
  int64_t mine = 0, beg;
  for (int64_t m = lo; m < hi; ++m) mine += (rank_segment(off, m, cap, beg) + R - 1) / R;
  s_cnt[tid] = mine;
  __syncthreads();
  for (int o = 1; o < RK_SLAB_THREADS; o <<= 1) {
    const int64_t v = tid >= o ? s_cnt[tid - o] : 0;
    __syncthreads();
    s_cnt[tid] += v;
    __syncthreads();
  }
  int64_t at = s_cnt[tid] - mine;
  for (int64_t m = lo; m < hi && at < vmax; ++m) {
    const int64_t n = rank_segment(off, m, cap, beg);
    for (int64_t i = 0; i < n && at < vmax; i += R, ++at) slabs[at] = RankSlab{beg + i, (int32_t)m, (int32_t)min((int64_t)R, n - i)};
  }
  if (tid == RK_SLAB_THREADS - 1) a.hdr[x ? 1 : 0] = (int32_t)min(s_cnt[tid], vmax);
}

// a row's 8 elements k0 .. k0 + 7 as a bf16 fragment: fp32 rounded to nearest-even (store_rows'
// conversion), bf16 taken as it is; `row` < 0: zeros
__device__ __forceinline__ bf16x8 rank_frag(const void* base, bool bf16, int64_t row, int64_t ld, int k0) {
  bf16x8 f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float x = 0.f;
    if (row >= 0) {
      const int64_t o = row * ld + k0 + j;
      x = bf16 ? __uint_as_float(((uint32_t) reinterpret_cast<const unsigned short*>(base)[o]) << 16)
               : reinterpret_cast<const float*>(base)[o];
    }
    f[j] = (__bf16)x;
  }
  return f;
}

// workgroups [0, tblocks): the target slabs, two per wave; the others: the exclusion slabs, one per
// wave. Pair i of the wave is row i (the item) and column i (its query) of one MFMA tile
template <int KS, bool BIAS>
__global__ void __launch_bounds__(TK_THREADS) rank_pair_kernel(const RankArgs a) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const bool x = (int)blockIdx.x >= a.tblocks;
  const int R = x ? RK_XR : RK_R;
  const int64_t wave = (int64_t)(x ? (int)blockIdx.x - a.tblocks : (int)blockIdx.x) * TK_WAVES + wid;
  const int V = a.hdr[x ? 1 : 0];
  const int64_t v0 = wave * (16 / R);
  if (v0 >= V) return;
  const RankSlab* slabs = x ? a.xslab : a.tslab;
  const int32_t* values = x ? a.xv : a.tv;
  float* out = x ? a.xscore : a.tscore;

  const int i = lane & 15;
  const int64_t v = v0 + i / R;
  const int j = i % R;
  int64_t pos = -1, m = -1, n = -1;
  if (v < V) {
    const RankSlab sl = slabs[v];
    if (j < sl.n) {
      pos = sl.first + j;
      m = sl.q;
      n = values[pos];
    }
  }
  const bool in_range = n >= 0 && n < a.N;
  if (!in_range) n = -1;
  f32x4 acc = (f32x4)(0.f);
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const int k0 = ks * 32 + (lane >> 4) * 8;
    const bf16x8 af = rank_frag(a.c, a.c_bf16, n, a.ldc, k0);
    const bf16x8 qf = rank_frag(a.q, a.q_bf16, n >= 0 ? m : -1, a.ldq, k0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, qf, acc, 0, 0, 0);
  }
  // the diagonal: row i is register i & 3 of the lanes with lane >> 4 == i >> 2
  if (pos >= 0 && (lane >> 4) == (i >> 2)) {
    const int r = i & 3;
    float s = r == 0 ? acc[0] : r == 1 ? acc[1] : r == 2 ? acc[2] : acc[3];
    if (BIAS && in_range) s += a.bias[n];
    out[pos] = in_range ? s : std::numeric_limits<float>::infinity();
  }
}

// the next float below a finite t (t normalised: no -0), and its inverse (which gives -0 for +0:
// equal in every compare)
__device__ __forceinline__ float rank_pred(float t) {
  const uint32_t u = __float_as_uint(t);
  return __uint_as_float(t > 0.f ? u - 1u : t < 0.f ? u + 1u : 0x80000001u);
}
__device__ __forceinline__ float rank_succ(float p) {
  const uint32_t u = __float_as_uint(p);
  return __uint_as_float((u & 0x80000000u) ? u - 1u : u + 1u);
}

template <int KS, bool BIAS>
__global__ void __launch_bounds__(TK_THREADS, 2) rank_scan_kernel(const RankArgs a) {
  using Sh = ScanShape<KS>;
  constexpr int STRIDE = Sh::STRIDE, IC = Sh::IC;
  __shared__ __attribute__((aligned(16))) __bf16 items[2][IC * STRIDE];
  __shared__ __attribute__((aligned(16))) float bias_s[2][IC];
  __shared__ uint32_t mask_s[2][Sh::MW];

  // as topk_mips_kernel: the workgroups of one item split are consecutive in the logical order
  const int logical = xcd_remap((int)blockIdx.x, (int)gridDim.x);
  const int split = logical / a.vtiles, vtile = logical - split * a.vtiles;
  const int V = a.hdr[0];
  if ((int64_t)vtile * TK_QB >= V) return;  // the whole workgroup: the grid is sized to the bound of V
  const int64_t n_beg = (int64_t)split * a.per;
  const int64_t n_end = n_beg + a.per < a.N ? n_beg + a.per : a.N;
  const int nchunks = n_end > n_beg ? (int)((n_end - n_beg + IC - 1) / IC) : 0;

  TopkFiltArgs fa{};
  fa.c = a.c;
  fa.ldc = a.ldc;
  fa.N = a.N;
  fa.c_bf16 = a.c_bf16;
  fa.c_vec = a.c_vec;
  fa.allow = a.allow;
  ExactSrc<KS, true> s{fa, 0, nullptr, n_beg, n_end, nchunks, false, nullptr, a.c_bf16 && a.c_vec};

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int64_t v_wave = (int64_t)vtile * TK_QB + wid * TK_QW;
  const bool computes = v_wave < V;  // else the wave only helps to stage
  constexpr float INF = std::numeric_limits<float>::infinity();

  // the wave's virtual queries: lane l holds query (l & 15) of tile qt as the B operand, and that
  // query's targets: index ti (0xffffffff: none), the running threshold thr (pred(t) of the target's score t
  // until the stream has passed row ti, then t; +inf: no target) and the count
  bf16x8 qf[2][KS];
  float thr[2][RK_R], tmin[2];
  uint32_t ti[2][RK_R], cnt[2][RK_R];
  int live = 0;  // the most targets any of the wave's queries has: the slots the scan compares
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    const int64_t v = v_wave + qt * 16 + (lane & 15);
    RankSlab sl{0, -1, 0};
    if (v < V) sl = a.tslab[v];
#pragma unroll
    for (int j = 1; j <= RK_R; ++j)
      if (__ballot(sl.n >= j) != 0ull) live = live > j ? live : j;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) qf[qt][ks] = rank_frag(a.q, a.q_bf16, sl.q, a.ldq, ks * 32 + (lane >> 4) * 8);
    tmin[qt] = INF;
#pragma unroll
    for (int j = 0; j < RK_R; ++j) {
      float ts = INF;
      int idx = -1;
      if (j < sl.n) {
        ts = a.tscore[sl.first + j] + 0.f;  // -0 -> +0, as make_key
        if (ts != INF) idx = a.tv[sl.first + j];
      }
      ti[qt][j] = (uint32_t)idx;
      cnt[qt][j] = 0u;
      const float lo = ts != INF ? rank_pred(ts) : INF;
      thr[qt][j] = idx >= n_beg ? lo : ts;
      tmin[qt] = fminf(tmin[qt], lo);
    }
  }

  float rawbias = 0.f;
  auto load_chunk = [&](int c) {
    const int64_t n0 = n_beg + (int64_t)c * IC;
    s.load_rows(n0, tid);
    if (BIAS && tid < IC) rawbias = n0 + tid < n_end ? a.bias[n0 + tid] : 0.f;
    s.load_mask(c, n0, tid);
    // rows at and past n_end (zero rows, another split's) are denied here, so the mask alone decides
    if (tid < Sh::MW) {
      const int64_t left = n_end - (n0 + 32 * tid);
      if (left < 32) s.rawmask &= left > 0 ? (1u << left) - 1u : 0u;
    }
  };
  auto store_chunk = [&](int buf) {
    s.store_rows(items[buf], tid);
    if (BIAS && tid < IC) bias_s[buf][tid] = rawbias;
    s.store_mask(mask_s[buf], tid);
  };

  if (nchunks > 0) {
    load_chunk(0);
    store_chunk(0);
  }
  __syncthreads();

  for (int c = 0; c < nchunks; ++c) {
    const int buf = c & 1;
    if (c + 1 < nchunks) load_chunk(c + 1);
    const int64_t n0 = n_beg + (int64_t)c * IC;
    if (computes) {
      // bit `it` of hit[qt]: tile `it` of this chunk holds the row of one of the lane's targets
      uint32_t hit[2];
#pragma unroll
      for (int qt = 0; qt < 2; ++qt) {
        hit[qt] = 0u;
#pragma unroll
        for (int j = 0; j < RK_R; ++j) {
          const uint32_t d = ti[qt][j] - (uint32_t)n0;  // indices and rows are below 2^31 + IC
          if (d < (uint32_t)IC) hit[qt] |= 1u << (d >> 4);
        }
      }
      // the chunk's tiles, comparing the first NL target slots: those past `live` hold +inf in every
      // lane (leave-one-out evaluation has one target a query). One copy of the loop per slot count:
      // chosen inside the loop, per tile, the full 8 slots ran 9 to 15 % slower
      const auto tiles = [&](auto nl) {
        constexpr int NL = decltype(nl)::value;
#pragma unroll 1
        for (int it = 0; it < IC / 16; ++it) {
          bf16x8 af[KS];
#pragma unroll
          for (int ks = 0; ks < KS; ++ks)
            af[ks] = *reinterpret_cast<const bf16x8*>(&items[buf][(it * 16 + (lane & 15)) * STRIDE + ks * 32 + (lane >> 4) * 8]);
          f32x4 bv = (f32x4)(0.f);
          if (BIAS) bv = *reinterpret_cast<const f32x4*>(&bias_s[buf][it * 16 + (lane >> 4) * 4]);
          // the tile's 16 mask bits (wave-uniform), all set in the common case
          const uint32_t m16 = (mask_s[buf][it >> 1] >> ((it & 1) * 16)) & 0xffffu;
          const bool all_rows = __builtin_amdgcn_readfirstlane(m16) == 0xffffu;
#pragma unroll
          for (int qt = 0; qt < 2; ++qt) {
            f32x4 acc = (f32x4)(0.f);
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[ks], qf[qt][ks], acc, 0, 0, 0);
            if (BIAS) acc += bv;
            // nothing of the tile reaches the lowest of the lanes' thresholds: no count changes. (A
            // tile with a target's row holds its score, which is above pred(t))
            const float mx = fmaxf(fmaxf(acc[0], acc[1]), fmaxf(acc[2], acc[3]));
            if (__ballot(mx > tmin[qt]) == 0ull) continue;
            if (!all_rows) {
              const uint32_t mb = m16 >> ((lane >> 4) * 4);
#pragma unroll
              for (int r = 0; r < 4; ++r) acc[r] = ((mb >> r) & 1u) ? acc[r] : -INF;  // precedes no finite target
            }
            if (__ballot((hit[qt] >> it) & 1u) == 0ull) {
#pragma unroll
              for (int j = 0; j < NL; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) cnt[qt][j] += acc[r] > thr[qt][j] ? 1u : 0u;
            } else {
              // the exact rule. thr is t where an earlier tile held the target's row, else pred(t); a
              // target whose row this tile holds goes on with t
              const uint32_t tile_beg = (uint32_t)n0 + it * 16;
              const uint32_t nb = tile_beg + (lane >> 4) * 4;
#pragma unroll
              for (int j = 0; j < NL; ++j) {
                const uint32_t tij = ti[qt][j];
                const float tj = tij < tile_beg ? thr[qt][j] : rank_succ(thr[qt][j]);
#pragma unroll
                for (int r = 0; r < 4; ++r) cnt[qt][j] += ((acc[r] > tj) | ((acc[r] == tj) & (nb + r < tij))) ? 1u : 0u;
                if (tij < tile_beg + 16) thr[qt][j] = tj;
              }
            }
          }
        }
      };
      using std::integral_constant;
      if (live > 4)
        tiles(integral_constant<int, RK_R>{});
      else if (live > 2)
        tiles(integral_constant<int, 4>{});
      else if (live > 1)
        tiles(integral_constant<int, 2>{});
      else
        tiles(integral_constant<int, 1>{});
    }
    if (c + 1 < nchunks) store_chunk(buf ^ 1);
    __syncthreads();
  }

  // a query's counts are spread over its 4 lanes (4 rows of a tile each)
  if (computes) {
    uint32_t* part = a.part + (int64_t)split * a.T_cap;
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
      const int64_t v = v_wave + qt * 16 + (lane & 15);
      RankSlab sl{0, -1, 0};
      if (v < V) sl = a.tslab[v];
#pragma unroll
      for (int j = 0; j < RK_R; ++j) {
        uint32_t cj = cnt[qt][j];
        cj += __shfl_xor(cj, 16, 64);
        cj += __shfl_xor(cj, 32, 64);
        if (lane < 16 && j < sl.n) part[sl.first + j] = cj;
      }
    }
  }
}

__device__ __forceinline__ bool rank_allowed(const uint32_t* __restrict__ allow, int64_t n) {
  return !allow || ((allow[n >> 5] >> (n & 31)) & 1u);
}

// one thread per target of a slab
__global__ void __launch_bounds__(256) rank_finish_kernel(const RankArgs a) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t v = g / RK_R;
  const int j = (int)(g - v * RK_R);
  if (v >= a.hdr[0]) return;
  const RankSlab sl = a.tslab[v];
  if (j >= sl.n) return;
  const int64_t pos = sl.first + j;
  const int64_t tn = a.tv[pos];
  const float ts = a.tscore[pos] + 0.f;  // -0 -> +0: the bits a key holds
  bool ok = tn >= 0 && tn < a.N;
  ok = ok && rank_allowed(a.allow, tn);
  int64_t rank = 0;
  if (ok) {
    for (int sp = 0; sp < a.S; ++sp) rank += a.part[(int64_t)sp * a.T_cap + pos];
    if (a.xo) {
      int64_t beg;
      const int64_t n = rank_segment(a.xo, sl.q, a.L_cap, beg);
      const u64 tkey = make_key(ts, (int)tn);
      int64_t prev = -1;
      for (int64_t e = beg; e < beg + n; ++e) {
        const int64_t xn = a.xv[e];
        if (xn == tn) ok = false;
        // what the scan counted of the segment: once per distinct item (the segment ascends)
        if (xn != prev && xn >= 0 && xn < a.N && rank_allowed(a.allow, xn) && make_key(a.xscore[e], (int)xn) > tkey) --rank;
        prev = xn;
      }
    }
  }
  a.ranks[pos] = ok ? rank : -1;
  if (a.scores) a.scores[pos] = ok ? ts : -std::numeric_limits<float>::infinity();
}

static const char* rank_check(int64_t M, int64_t N, int64_t T_cap, int64_t L_cap, int splits) {
  if (M < 1 || M > (int64_t)1 << 30) return "M must be in [1, 2^30]";
  if (N < 1 || N >= (int64_t)1 << 31) return "N must be in [1, 2^31)";
  if (T_cap < 0 || T_cap >= (int64_t)1 << 31) return "T_cap must be in [0, 2^31)";
  if (L_cap < 0 || L_cap >= (int64_t)1 << 31) return "L_cap must be in [0, 2^31)";
  if (splits < 0 || splits > TK_MAX_SPLITS) return "splits must be 0 (chosen by the library) or in [1, 64]";
  return nullptr;
}

static int rank_auto_splits(int64_t M, int64_t T_cap, int64_t N) {
  // topk_auto_splits' aim (every workgroup resident at once, a split keeps >= 512 items) over the
  // virtual-query tiles that M queries with T_cap targets have at least
  const int64_t vtiles = ceil_div(std::max<int64_t>(M, ceil_div(T_cap, RK_R)), TK_QB);
  int64_t s = ceil_div(256 * (8 / TK_WAVES), vtiles);
  s = std::min<int64_t>(s, ceil_div(N, 512));
  return (int)std::max<int64_t>(1, std::min<int64_t>(s, TK_MAX_SPLITS));
}

// the workspace: the slab counts, the two slab tables, the two score arrays, the partial counts
struct RankWs {
  size_t hdr, tslab, xslab, tscore, xscore, part, bytes;
  int64_t tvmax, xvmax;
};
static RankWs rank_ws(int64_t M, int64_t T_cap, int64_t L_cap, int S) {
  RankWs w{};
  w.tvmax = ceil_div(T_cap, RK_R) + M;
  w.xvmax = L_cap > 0 ? ceil_div(L_cap, RK_XR) + M : 0;
  size_t o = 0;
  const auto take = [&](size_t n) {
    const size_t at = o;
    o += align_up(n, 256);
    return at;
  };
  w.hdr = take(2 * sizeof(int32_t));
  w.tslab = take((size_t)w.tvmax * sizeof(RankSlab));
  w.xslab = take((size_t)w.xvmax * sizeof(RankSlab));
  w.tscore = take((size_t)T_cap * 4);
  w.xscore = take((size_t)L_cap * 4);
  w.part = take((size_t)S * (size_t)T_cap * 4);
  w.bytes = o;
  return w;
}

}  // namespace tt

extern "C" {

size_t tt_target_ranks_workspace_bytes(int64_t M, int64_t N, int64_t T_cap, int64_t L_cap, int splits) {
  if (tt::rank_check(M, N, T_cap, L_cap, splits)) return 0;
  const int S = splits ? splits : tt::rank_auto_splits(M, T_cap, N);
  return tt::rank_ws(M, T_cap, L_cap, S).bytes;
}

int tt_target_ranks(const void* queries, int q_dtype, int64_t ldq, const void* items, int c_dtype, int64_t ldc,
                    const float* bias, int64_t M, int64_t N, int E, const int32_t* target_values,
                    const int64_t* target_offsets, int64_t T_cap, const uint32_t* allow, const int32_t* excl_values,
                    const int64_t* excl_offsets, int64_t L_cap, int splits, int64_t* ranks, float* scores, void* workspace,
                    size_t ws_bytes, void* stream) {
  using namespace tt;
  const std::string fn = "tt_target_ranks: ";
  if (E < 32 || E > 128 || (E & 31)) return fail(TT_EINVAL, fn + "E must be a multiple of 32 in [32, 128]");
  if (const char* msg = rank_check(M, N, T_cap, L_cap, splits)) return fail(TT_EINVAL, fn + msg);
  if ((q_dtype != TT_F32 && q_dtype != TT_BF16) || (c_dtype != TT_F32 && c_dtype != TT_BF16))
    return fail(TT_EINVAL, fn + "q_dtype / c_dtype must be TT_F32 or TT_BF16");
  if (ldq < E || ldc < E) return fail(TT_EINVAL, fn + "ldq / ldc must be >= E");
  if ((excl_values == nullptr) != (excl_offsets == nullptr))
    return fail(TT_EINVAL, fn + "excl_values and excl_offsets must both be NULL or both be given");
  if (!excl_values && L_cap != 0) return fail(TT_EINVAL, fn + "L_cap must be 0 without exclusion lists");
  if (!queries || !items || !target_offsets || !ranks || !workspace || (T_cap > 0 && !target_values))
    return fail(TT_EINVAL, fn + "null queries / items / target_values / target_offsets / ranks / workspace");
  const int S = splits ? splits : rank_auto_splits(M, T_cap, N);
  const RankWs w = rank_ws(M, T_cap, L_cap, S);
  if (ws_bytes < w.bytes) return fail(TT_EINVAL, fn + "ws_bytes is smaller than tt_target_ranks_workspace_bytes");
  if (T_cap == 0) return TT_OK;  // no targets: nothing is written
  const bool excl = excl_offsets && L_cap > 0;

  char* base = reinterpret_cast<char*>(workspace);
  RankArgs a{};
  a.q = queries;
  a.c = items;
  a.bias = bias;
  a.tv = target_values;
  a.to = target_offsets;
  a.allow = allow;
  a.xv = excl ? excl_values : nullptr;
  a.xo = excl ? excl_offsets : nullptr;
  a.ranks = ranks;
  a.scores = scores;
  a.hdr = reinterpret_cast<int32_t*>(base + w.hdr);
  a.tslab = reinterpret_cast<RankSlab*>(base + w.tslab);
  a.xslab = reinterpret_cast<RankSlab*>(base + w.xslab);
  a.tscore = reinterpret_cast<float*>(base + w.tscore);
  a.xscore = reinterpret_cast<float*>(base + w.xscore);
  a.part = reinterpret_cast<uint32_t*>(base + w.part);
  a.ldq = ldq;
  a.ldc = ldc;
  a.M = M;
  a.N = N;
  a.per = ceil_div(ceil_div(N, S), tk_chunk(E)) * tk_chunk(E);
  a.T_cap = T_cap;
  a.L_cap = excl ? L_cap : 0;
  a.S = S;
  a.vtiles = (int)ceil_div(w.tvmax, TK_QB);
  a.tvmax = (int)w.tvmax;
  a.xvmax = excl ? (int)w.xvmax : 0;
  a.q_bf16 = q_dtype == TT_BF16;
  a.c_bf16 = c_dtype == TT_BF16;
  a.c_vec = (reinterpret_cast<uintptr_t>(items) & 15) == 0 && (ldc % (a.c_bf16 ? 8 : 4)) == 0;
  a.tblocks = (int)ceil_div(ceil_div(w.tvmax, 16 / RK_R), TK_WAVES);
  if ((int64_t)a.vtiles * S > 0x7fffffff) return fail(TT_EINVAL, fn + "too many targets for one call");
  const int xblocks = excl ? (int)ceil_div(w.xvmax, TK_WAVES) : 0;

  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(rank_slabs_kernel, dim3(excl ? 2 : 1), dim3(RK_SLAB_THREADS), 0, st, a);
  if (int rc = check_launch("tt_target_ranks slabs")) return rc;
  topk_dispatch(E, bias != nullptr, [&](auto ks, auto b) {
    hipLaunchKernelGGL((rank_pair_kernel<decltype(ks)::value, decltype(b)::value>), dim3(a.tblocks + xblocks),
                       dim3(TK_THREADS), 0, st, a);
  });
  if (int rc = check_launch("tt_target_ranks pair scores")) return rc;
  topk_dispatch(E, bias != nullptr, [&](auto ks, auto b) {
    hipLaunchKernelGGL((rank_scan_kernel<decltype(ks)::value, decltype(b)::value>), dim3(a.vtiles * S),
                       dim3(TK_THREADS), 0, st, a);
  });
  if (int rc = check_launch("tt_target_ranks scan")) return rc;
  hipLaunchKernelGGL(rank_finish_kernel, dim3((unsigned)ceil_div(w.tvmax * RK_R, 256)), dim3(256), 0, st, a);
  return check_launch("tt_target_ranks finish");
}

}  // extern "C"
