// The row-owned T1 of the fused tower step (tower.hip): tower_rows_kernel and its launch.
#include "tower_common.h"

namespace tt {

// ---------------------------------------------------------------------------------------------
// T1, row-owned form (tower_rows_kernel): the production shape — both towers over 128-wide
// single-hot rows gathered from the tables, layers [128, 64]. One workgroup of 4 compute waves (and
// the image wave, which fills the LDS weight image while the ids and rows come in) per 32
// batch rows; wave w < 4 runs tower t = w >> 1 over rows 16 (w & 1) .. + 15 of the tile through the
// whole chain (gather, both layers, logit, dZ1, dZ0, dX, the in-place row-wise Adagrad) with every
// activation in registers: three barriers (the weight image landed; the towers' outputs exchanged
// for the logit; the workgroup's bias / loss partials combined), no LDS round trip between layers.
//
// Every product is computed transposed, Z^T = W A^T: the weights are the MFMA A operand (M = the
// layer's output features, from an LDS image of both towers' bf16 weights, 96 KB, copied whole by
// LDS-DMA), the wave's 16 batch rows are N. The M rows of every tile are PERMUTED (rk_perm): row
// rho of M-tile mt is feature 32 (mt >> 1) + 8 (rho >> 2) + 4 (mt & 1) + (rho & 3), so a lane's
// result values of the tile pair (2 s, 2 s + 1) are features 32 s + 8 q .. + 7 of its batch row n
// (q = lane >> 4, n = lane & 15) — exactly the B operand of the next product's k-step s, and two
// 16-B pieces of the row (the gathered fp32 row is loaded straight into that layout, and dX comes
// out in it: the row-wise Adagrad updates the row from registers). Forward A fragments are one
// ds_read_b128 per lane (W [out][in] image, conflict-free under rk_swz); backward ones (W^T) two
// ds_read_b64_tr_b16 from the same image (2-way: the minimum with a fixed 8-B half per read).
// The T1 -> T2 operand strips (tile-major, strip_at) go through a per-wave LDS transpose; the bias
// partials are fp32 column sums (a DPP transpose-reduce over the wave's 16 rows, then the two row
// halves in order): the tail launch and T3 read the same buffers as with tower_l2_kernel.
// The weight image's layout (RK_IN .. rk_off) is in tower_common.h: T3 writes the image.

// four compute waves (threads 0 .. 255: everything indexed by threadIdx.x is theirs) and the image
// wave (wave 4), which only copies the image into LDS and keeps the barrier count
constexpr int RK_THREADS = 320;
__device__ __forceinline__ int rk_perm(int mt, int rho) {
  return 32 * (mt >> 1) + 8 * (rho >> 2) + 4 * (mt & 1) + (rho & 3);
}
// A fragment (M-tile mt, k-step s) of W from its image ([M][K] rows): lane (rho, q) holds
// W[rk_perm(mt, rho)][32 s + 8 q .. + 7]
__device__ __forceinline__ bf16x8 rk_afwd(const char* img, int mt, int s, int rho, int q) {
  return *reinterpret_cast<const bf16x8*>(img + rk_off(rk_perm(mt, rho), 32 * s + 8 * q));
}
// A fragment (M-tile mt, k-step s) of W^T from the image of W ([K][M] rows): lane 4 q' + p of the
// 16-lane group q addresses image row 32 s + 8 q + q' (+ 4) at the 4 contiguous features
// rk_perm(mt, 4 p .. 4 p + 3); lane rho receives feature rk_perm(mt, rho) at those rows
__device__ __forceinline__ bf16x8 rk_abwd(const char* img, int mt, int s, int lane) {
  const int q = lane >> 4, qq = (lane >> 2) & 3, p = lane & 3;
  const int row = 32 * s + 8 * q + qq;
  const int col = 32 * (mt >> 1) + 8 * p + 4 * (mt & 1);
  const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(img + rk_off(row, col)));
  const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(img + rk_off(row + 4, col)));
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}
__device__ __forceinline__ bf16x8 rk_pack(const f32x4& a, const f32x4& b) {
  bf16x8 v;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    v[j] = (__bf16)a[j];
    v[4 + j] = (__bf16)b[j];
  }
  return v;
}
// the A fragments (M-tiles mt < MT) of k-step s of a product, issued into one register set
template <int MT, bool BWD>
__device__ __forceinline__ void rk_frags(bf16x8 (&f)[8], const char* img, int s, int lane) {
  const int n = lane & 15, q = lane >> 4;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) f[mt] = BWD ? rk_abwd(img, mt, s, lane) : rk_afwd(img, mt, s, n, q);
}
// acc[mt] (mt < MT) = sum over k-steps s < S of A(mt, s) x b[s], as one link of the fragment
// pipeline that runs through all the products of the chain: the product's k-step 0 is already in
// flight in fa[0] when it starts (rk_frags, issued by the product before it), the fragments of
// k-step s + 1 are read into the other register set before k-step s's MFMAs issue, and in front
// of its last k-step's MFMAs the product issues the NEXT product's k-step 0 (next(set): the weight
// fragments depend on the image only, never on an activation; S is even, so that set is fa[0]
// again). No product starts with an LDS round trip of its own, and none waits behind the
// epilogue of the one before. fill(s) is vector work without LDS reads that runs beside k-step
// s's MFMAs, behind the reads' issue (the bias column sums under the LDS-bound backward products)
template <int MT, int S, bool BWD, typename Next, typename Fill>
__device__ __forceinline__ void rk_gemm(f32x4 (&acc)[8], bf16x8 (&fa)[2][8], const char* img, const bf16x8 (&b)[4],
                                        int lane, Next next, Fill fill) {
  static_assert(S % 2 == 0, "the next product's k-step 0 goes to set 0");
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) acc[mt] = (f32x4)(0.f);
#pragma unroll
  for (int s = 0; s < S; ++s) {
    if (s + 1 < S) rk_frags<MT, BWD>(fa[(s + 1) & 1], img, s + 1, lane);
    else next(fa[(s + 1) & 1]);
    __builtin_amdgcn_sched_barrier(0);
    fill(s);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
      acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[s & 1][mt], b[s], acc[mt], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
  }
}
// lane value from lane ^ X of its 16-lane row (X in {1, 2, 4, 8}) by DPP
template <int X>
__device__ __forceinline__ float rk_xor(float v) {
  if constexpr (X == 1) return dpp_f<0xB1>(v);   // quad_perm [1, 0, 3, 2]
  if constexpr (X == 2) return dpp_f<0x4E>(v);   // quad_perm [2, 3, 0, 1]
  if constexpr (X == 4) return dpp_f<0x1B>(dpp_f<0x141>(v));  // row_half_mirror, then quad reversal
  return dpp_f<0x128>(v);                        // row_ror 8
}
// column sums over the 16 lanes of each 16-lane row: NV values per lane in, NV / 16 out; after it,
// lane n holds the sums of values k = (NV / 16) n + i, i < NV / 16 (halving at lane bits 3, 2, 1, 0)
template <int X, int H>  // the live values v[0, 2 H) -> v[0, H)
__device__ __forceinline__ void rk_halve(float* v, int n) {
  const bool up = (n & X) != 0;
#pragma unroll
  for (int i = 0; i < H; ++i) {
    const float keep = up ? v[H + i] : v[i], send = up ? v[i] : v[H + i];
    v[i] = keep + rk_xor<X>(send);
  }
}
// one level l of the four (lane bit 3 - l), in order: the caller spreads them over the k-steps of a
// product
template <int NV>
__device__ __forceinline__ void rk_colsum_level(float (&v)[NV], int n, int l) {
  static_assert(NV == 32 || NV == 16, "column sum of 32 or 16 values per lane");
  if (l == 0) rk_halve<8, NV / 2>(v, n);
  else if (l == 1) rk_halve<4, NV / 4>(v, n);
  else if (l == 2) rk_halve<2, NV / 8>(v, n);
  else rk_halve<1, NV / 16>(v, n);
}
// row-major operand strip ([Bp][nf] bf16, what the tail's wgrad_lds_block_rm reads): lane (q, n)
// stores its 16-B pieces (features 32 s + 8 q .. + 7) of batch row m; a wave instruction writes 16
// whole 64-B row segments
// (every row of the tile, dead rows of a ragged tile included: the strips hold Bp rows, the tail
// reads the first B; no branch around the stores, which would make later load waits count
// conservatively)
template <int NS>
__device__ __forceinline__ void rk_strip(const bf16x8 (&v)[4], __bf16* row, int q) {
#pragma unroll
  for (int s = 0; s < NS; ++s) *reinterpret_cast<bf16x8*>(row + 32 * s + 8 * q) = v[s];
}

// direct exchange (tt_peer_direct_t): where send-buffer row `row` lands (the destination block's
// mapped receive buffer); a uniform loop with scalar kernarg loads selects the block
__device__ __forceinline__ char* px_row(const tt_peer_direct_t& x, int64_t row, int64_t row_bytes) {
  char* base = reinterpret_cast<char*>(x.row0[0]);
  int64_t f0 = 0;
#pragma unroll
  for (int q = 1; q < TT_PEER_MAXW; ++q) {
    if (q < x.W && row >= x.first_row[q]) {
      base = reinterpret_cast<char*>(x.row0[q]);
      f0 = x.first_row[q];
    }
  }
  return base + (row - f0) * row_bytes;
}
// the copy fields split over the grid: workgroup b takes 16-B units [b per, (b + 1) per) of their
// concatenation (d ascending); unit u of this thread -> (src, dst), or false past the end
__device__ __forceinline__ bool px_copy_unit(const tt_peer_direct_t& x, int64_t u, const uint4*& src, uint4*& dst) {
  int64_t pre = 0;
  bool hit = false;
#pragma unroll
  for (int q = 0; q < TT_PEER_MAXW; ++q) {
    const int64_t n = q < x.W ? x.copy_len[q] >> 4 : 0;
    if (!hit && u >= pre && u < pre + n) {
      src = reinterpret_cast<const uint4*>(x.copy_src[q]) + (u - pre);
      dst = reinterpret_cast<uint4*>(x.copy_dst[q]) + (u - pre);
      hit = true;
    }
    pre += n;
  }
  return hit;
}
__device__ __forceinline__ int64_t px_copy_units(const tt_peer_direct_t& x) {
  int64_t n = 0;
#pragma unroll
  for (int q = 0; q < TT_PEER_MAXW; ++q) n += q < x.W ? x.copy_len[q] >> 4 : 0;
  return n;
}

// raw 4- or 8-byte element i of an id / label column: the conversion is left to the caller, so a
// dtype branch does not put a wait for the load right behind it (the loads of a prologue all issue
// before the first wait)
struct RkRaw {
  uint32_t lo, hi;
};
__device__ __forceinline__ RkRaw rk_raw(const void* p, bool wide, int64_t i) {
  RkRaw r;
  if (wide) {
    const uint2 v = reinterpret_cast<const uint2*>(p)[i];
    r.lo = v.x;
    r.hi = v.y;
  } else {
    r.lo = reinterpret_cast<const uint32_t*>(p)[i];
    r.hi = 0u;
  }
  return r;
}
__device__ __forceinline__ int64_t rk_id(RkRaw r, bool wide) {
  return wide ? (int64_t)(((uint64_t)r.hi << 32) | r.lo) : (int64_t)(int32_t)r.lo;
}
__device__ __forceinline__ float rk_label(RkRaw r, int dt) {
  if (dt == TT_I32) return (float)(int32_t)r.lo;
  if (dt == TT_I64) return (float)(int64_t)(((uint64_t)r.hi << 32) | r.lo);
  return __uint_as_float(r.lo);
}
// N per-lane values (addresses, row indices) pinned in VGPRs at one point: everything they depend
// on (a batch of shuffles or LDS reads) is issued and waited for once in front of it, where the
// compiler would otherwise interleave each value's wait with its use
template <int N, typename T>
__device__ __forceinline__ void rk_pin(T (&p)[N]) {
  static_assert(N == 2 || N == 4 || N == 8, "2, 4 or 8 values");
  if constexpr (N == 8)
    asm volatile("" : "+v"(p[0]), "+v"(p[1]), "+v"(p[2]), "+v"(p[3]), "+v"(p[4]), "+v"(p[5]), "+v"(p[6]), "+v"(p[7]));
  else if constexpr (N == 4)
    asm volatile("" : "+v"(p[0]), "+v"(p[1]), "+v"(p[2]), "+v"(p[3]));
  else
    asm volatile("" : "+v"(p[0]), "+v"(p[1]));
}
// EXPERIMENT (TT_T1_DEBUG bit 8): lane 0 of each wave at point k: stamps[8192 + (wg * 16 + k) * 9 + wave]
#if TT_EXPERIMENTS
#define RK_STAMP(k) \
  do { if (a.stamps && lane == 0) a.stamps[8192 + ((int64_t)blockIdx.x * 16 + (k)) * 9 + wid] = (int64_t)__builtin_amdgcn_s_memrealtime(); } while (0)
// extra points in wave slots 4 .. 7
#define RK_STAMP2(k) \
  do { if (a.stamps && lane == 0) a.stamps[8192 + ((int64_t)blockIdx.x * 16 + (k)) * 9 + 4 + wid] = (int64_t)__builtin_amdgcn_s_memrealtime(); } while (0)
// the image wave's points (0 start, 1 DMAs issued, 2 landed, 3 past barrier 1) in wave slot 8
#define RK_STAMP_IMG(k) \
  do { if (a.stamps && lane == 0) a.stamps[8192 + ((int64_t)blockIdx.x * 16 + (k)) * 9 + 8] = (int64_t)__builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define RK_STAMP(k) do { } while (0)
#define RK_STAMP2(k) do { } while (0)
#define RK_STAMP_IMG(k) do { } while (0)
#endif

// IDX: the sharded step's form (tt_tower_fwd_bwd_indexed2_bf16): tower t's input row m is bf16 row
// gpos[t][m] of gsrc[t] (-1: zeros; the rows an owner returned, dense), its dX goes to fp32 row
// gpos_out[t][m] of gdst[t]; no in-place update, no insert
// IN: the input width (128 or 64: config 2's D = 64; the first layer then has 2 k-steps and dX 4
// M-tiles, the rows are 256 B)
// POOL: the input rows are the pooled matrix's (tower t's row m at a.pooled + m ldp + in_col[t]:
// the multi-hot path's T1 after tt_pooled_fwd), no ids, no dedup
template <bool UPD, bool IDX, int IN, bool POOL = false>
__device__ __forceinline__ void tower_rows_body(const TowerArgs& a) {
  static_assert(IN == 128 || IN == 64, "row-owned T1: inputs of 128 or 64");
  static_assert(!POOL || (!UPD && !IDX), "pooled input: the plain T1 only");
  constexpr int NI = IN / 32;   // layer-0 k-steps (B-operand pieces xb[s], s < NI)
  constexpr int MTI = IN / 16;  // dX M-tiles (row pieces xv[mt], mt < MTI)
  __shared__ __attribute__((aligned(16))) char wimg[RK_IMG];         // both towers' W0, W1 (rk_off)
  __shared__ __attribute__((aligned(16))) float xo[2][2][16 * 64];  // tower outputs per (tower, row half)
  __shared__ float bsum[2][RK_W0 + RK_W1];                          // row half 1's bias partials
  __shared__ __attribute__((aligned(16))) float lrow[TR];           // row losses
  __shared__ __attribute__((aligned(16))) float xr[4][16 * IN];     // per wave: its 16 gathered rows
                                                                    // (fp32, 16-B chunk c of row n at c ^ n)
  const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  typedef __attribute__((address_space(3))) void lds_void;
  typedef __attribute__((address_space(1))) void glb_void;
  // ---- the image wave (wave 4 of RK_THREADS): the whole weight image -> LDS by LDS-DMA, 1 KB per
  // wave instruction (the global image is in the LDS layout, rk_off: a straight copy). The image
  // does not depend on the ids, and vmcnt is per wave: the compute waves' id / row waits never
  // count these DMAs, and nothing of the image passes through their registers. The wave then only
  // keeps the workgroup's barrier count (three, as every path of the compute waves)
  if (wid == 4) {
    RK_STAMP_IMG(0);
    if (!TDBG(16)) {  // EXPERIMENT (timing only): no image fill
#pragma unroll
      for (int k = 0; k < RK_IMG / 1024; ++k)
        __builtin_amdgcn_global_load_lds((glb_void*)(a.wimg + k * 1024 + lane * 16), (lds_void*)(wimg + k * 1024), 16, 0, 0);
    }
    RK_STAMP_IMG(1);
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): the image landed
    RK_STAMP_IMG(2);
    __syncthreads();  // barrier 1: the image landed
    RK_STAMP_IMG(3);
    __syncthreads();  // barrier 2: the towers' outputs exchanged
    __syncthreads();  // barrier 3: the bias / loss partials combined
    return;
  }
  const int t = wid >> 1, h = wid & 1, q = lane >> 4, n = lane & 15;
  // ---- the entry batch (RkCommon line 0, the tower's line 0): every scalar the id, claim, label,
  // bias and row-DMA addresses need, loaded together and held at once: one wait in front of the
  // first vector load (left at their uses, each field is a scalar round trip of its own, the
  // modulus inside its branch)
  const RkCommon& C = a.rk.c;
  const RkTower& T = a.rk.tw[t];  // t is wave-uniform: one scalar offset selects the record
  const int64_t B = C.B;
  const void* const labels = C.labels;
  const int label_dtype = C.label_dtype, gid_dtype = C.gid_dtype;
  const void* const idcol = T.idcol;
  const void* const tab0 = T.tab;
  const int64_t gmod = T.gmod;
  const float* const b0p = T.b0;
  const float* const b1p = T.b1;
  const int32_t* const claim = T.claim;
  const int32_t* const pos_out = T.pos_out;
  const int64_t pstride = T.rstride;
  const int nwg = C.nwg;
  if (UPD) asm volatile("" ::"s"(nwg), "s"(B), "s"(labels), "s"(label_dtype), "s"(gid_dtype), "s"(idcol), "s"(tab0), "s"(gmod), "s"(b0p), "s"(b1p), "s"(claim));
  else if (IDX) asm volatile("" ::"s"(nwg), "s"(B), "s"(labels), "s"(label_dtype), "s"(idcol), "s"(tab0), "s"(b0p), "s"(b1p), "s"(pos_out));
  else if (POOL) asm volatile("" ::"s"(nwg), "s"(B), "s"(labels), "s"(label_dtype), "s"(tab0), "s"(b0p), "s"(b1p), "s"(pstride));
  else asm volatile("" ::"s"(nwg), "s"(B), "s"(labels), "s"(label_dtype), "s"(gid_dtype), "s"(idcol), "s"(tab0), "s"(gmod), "s"(b0p), "s"(b1p));
  // the tile: XCD x runs tiles [x n / 8, (x + 1) n / 8) (xcd_remap), so the 256-row slices the
  // tail's T2 tiles read (also placed a contiguous 1/8 per XCD) were written through that XCD's L2
  // (the grid size from the record: the launch's own copy is a scalar load, and a wait, of its own)
  const int tile = xcd_remap((int)blockIdx.x, nwg);
  const int64_t m0 = (int64_t)tile * TR, m = m0 + 16 * h + n;
  const bool live = m < B;
  RK_STAMP(0);
  // ---- 0. loads in dependency order (vmcnt retires in issue order: a wait for a load also waits
  // for everything issued before it): the ids, the label, the biases (raw: no conversion between
  // them); the row (the weight image is the image wave's, above)
  const bool wide = gid_dtype == TT_I64;
  const int64_t mc = live ? m : 0;  // dead rows of a ragged tile read row 0 of every column
  RkRaw id_raw{0u, 0u}, pout_raw{0u, 0u};
  if (IDX) {
    id_raw.lo = (uint32_t) reinterpret_cast<const int32_t*>(idcol)[mc];
    pout_raw.lo = pos_out ? (uint32_t)pos_out[mc] : id_raw.lo;
  } else if (!POOL) {
    id_raw = rk_raw(idcol, wide, mc);
  }
  // UPD: the claim of this row's lookup in the batch's completed dedup table (no dependency: issued
  // beside the id, so the slot word's load can follow the row DMA instead of stalling the chain after
  // layer 1 for a whole memory round trip)
  int32_t cl = -1;
  if (UPD) cl = claim[mc];
  const RkRaw lab_raw = rk_raw(labels, label_dtype == TT_I64, mc);
  f32x4 b0v[8], b1v[4];
  auto load_biases = [&]() {
#pragma unroll
    for (int mt = 0; mt < 8; ++mt) b0v[mt] = *reinterpret_cast<const f32x4*>(b0p + 32 * (mt >> 1) + 8 * q + 4 * (mt & 1));
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) b1v[mt] = *reinterpret_cast<const f32x4*>(b1p + 32 * (mt >> 1) + 8 * q + 4 * (mt & 1));
  };
  // (with an LDS-DMA in flight the compiler waits vmcnt(0) at the first use of any load, so in
  // these waves the ids must land before the first row DMA is issued: no DMA of the image here)
  load_biases();
  __builtin_amdgcn_sched_barrier(0);
  // direct exchange: this workgroup's first share of the copy region (exchange A's keys), loaded
  // now beside the prologue's loads, stored at the end (the rest of a large share there too)
  uint4 cpv = make_uint4(0u, 0u, 0u, 0u);
  uint4* cpd = nullptr;
  int64_t cp_per = 0, cp_end = 0;
  if constexpr (IDX) {
    if (a.xd.W) {
      const int64_t tot = px_copy_units(a.xd);
      cp_per = (tot + gridDim.x - 1) / gridDim.x;
      cp_end = min(tot, ((int64_t)blockIdx.x + 1) * cp_per);
      const int64_t u = (int64_t)blockIdx.x * cp_per + threadIdx.x;
      const uint4* cps;
      if (u < cp_end && px_copy_unit(a.xd, u, cps, cpd)) cpv = *cps;
      else cpd = nullptr;
    }
  }
  int64_t r;  // the row's index in its source (table row / returned-rows buffer row), -1: zeros
  if (POOL) {
    r = live ? m : -1;
  } else if (IDX) {
    r = live ? (int64_t)(int32_t)id_raw.lo : -1;
  } else {
    const int64_t id = live ? rk_id(id_raw, wide) : 0;
    r = id != 0 ? py_mod64(id, gmod) : -1;
  }
  const float* tab = reinterpret_cast<const float*>(tab0);
  const int64_t rstride = POOL ? pstride : IN;  // floats between consecutive source rows
  // the wave's 16 rows -> LDS by LDS-DMA, two whole 512-B rows per wave instruction (two TLB pages
  // per instruction, full lines; a lane-per-row-piece register gather touches 16 rows per
  // instruction): lane l of instruction i carries 16-B chunk (l & 31) ^ row of row 2 i + (l >> 5),
  // so that the B-layout reads below are conflict-free; rows without an id read table row 0
  // (ignored)
  RK_STAMP2(4);  // EXPERIMENT: the ids landed (r is computed), in front of the row-index shuffles
  __builtin_amdgcn_sched_barrier(0);
  float* xw = xr[wid];
  // (IN = 64: four 256-B rows per instruction)
  constexpr int CPR = IDX ? IN / 8 : IN / 4;  // 16-B chunks per row (chunk swizzle: c ^ (row & (CPR - 1)))
  constexpr int RPI = 64 / CPR;               // rows per wave instruction
  constexpr int NDMA = 16 / RPI;              // wave instructions for the 16 rows
  // every row-index shuffle first, all addresses held at once (rk_pin), then the DMAs back to
  // back: one LDS round trip between "ids landed" and "rows issued", not one per instruction
  if (IDX) {
    // bf16 rows (2 IN bytes): lane l carries 16-B chunk (l % CPR) ^ row of row RPI i + l / CPR
    const int rr0 = lane / CPR, pc = lane % CPR;
    const char* src0 = reinterpret_cast<const char*>(tab0);
    const char* src[NDMA];
    int64_t rid[NDMA];
#pragma unroll
    for (int i = 0; i < NDMA; ++i) rid[i] = __shfl((long long)r, RPI * i + rr0, 64);
    rk_pin<NDMA>(rid);
#pragma unroll
    for (int i = 0; i < NDMA; ++i) {
      const int row = RPI * i + rr0;
      src[i] = src0 + (rid[i] >= 0 ? rid[i] : 0) * (IN * 2) + 16 * (pc ^ (row & (CPR - 1)));
    }
    rk_pin<NDMA>(src);
#pragma unroll
    for (int i = 0; i < NDMA; ++i)
      __builtin_amdgcn_global_load_lds((glb_void*)src[i], (lds_void*)(reinterpret_cast<char*>(xw) + i * 1024), 16, 0, 0);
  } else {
    const int rr0 = lane / CPR, pc = lane % CPR;
    const float* src[NDMA];
    int64_t rid[NDMA];
#pragma unroll
    for (int i = 0; i < NDMA; ++i) rid[i] = __shfl((long long)r, RPI * i + rr0, 64);
    rk_pin<NDMA>(rid);
#pragma unroll
    for (int i = 0; i < NDMA; ++i) {
      const int row = RPI * i + rr0;
      src[i] = tab + (rid[i] >= 0 ? rid[i] : 0) * rstride + 4 * (pc ^ row);
    }
    rk_pin<NDMA>(src);
#pragma unroll
    for (int i = 0; i < NDMA; ++i)
      if (!TDBG(32))  // EXPERIMENT (timing only, garbage rows): no row gather
        __builtin_amdgcn_global_load_lds((glb_void*)src[i], (lds_void*)(xw + i * 256), 16, 0, 0);
  }
  __builtin_amdgcn_sched_barrier(0);
  // the classic step's insert of this batch's lookups (T1 with a dedup workspace): the claiming
  // CAS now, the deferred finish at the end (lane q == 0 of each row)
  DdPend pend;
  pend.key = DD_EMPTY;
  const int32_t li = (int32_t)(t * B + m);
  if (!UPD && a.dd_on && q == 0 && live) {
    const uint64_t key = r >= 0 ? (((uint64_t)(t ? a.dd_table[1] : a.dd_table[0]) << DD_TABLE_SHIFT) | (uint64_t)r)
                                : DD_EMPTY;
    dd_insert_begin(a.dd, key, li, pend);
  }
  RK_STAMP(1);
  // ---- the late batch (the rest of RkCommon line 0, the tower's line 1 up to the state): the strip
  // bases, the slots, the state, grad_scale — issued behind the row DMAs, so their round trip runs
  // inside the wait for the rows (the pin behind that wait only keeps the loads in this block)
  const int in_max = C.in_max;
  const float grad_scale = C.grad_scale, fB = C.fB;
  DSlot* const slots = C.slots;
  __bf16* const xt_t = T.xt;
  __bf16* const act_t = T.act0;
  const float* const us_t = T.us;
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): the rows (LDS-DMA) and the small loads
  if (UPD) asm volatile("" ::"s"(in_max), "s"(grad_scale), "s"(fB), "s"(slots), "s"(xt_t), "s"(act_t), "s"(us_t));
  else asm volatile("" ::"s"(in_max), "s"(grad_scale), "s"(fB), "s"(xt_t), "s"(act_t));
  RK_STAMP(2);
  // this lane's row in the B layout: xv[mt] = features 32 (mt >> 1) + 8 q + 4 (mt & 1) .. + 3 (fp32).
  // In front of barrier 1: only this wave reads these rows, and its own vmcnt(0) above is all the
  // ordering an LDS-DMA asks of its issuing wave, so the LDS round trip and the converts run inside
  // the wait for the image instead of at the head of the chain. (Not the X strip's stores: in front
  // of the barrier they share the vector memory path with the image wave's DMAs and held the image
  // back 0.4-0.56 us, profiles/r11_t1_chain_stamps.log)
  f32x4 xv[8];
  bf16x8 xb[4];
  if (IDX) {  // the bf16 B operand straight from the returned rows
#pragma unroll
    for (int s2 = 0; s2 < NI; ++s2) {
      const bf16x8 v = *reinterpret_cast<const bf16x8*>(reinterpret_cast<const char*>(xw) + n * (IN * 2) +
                                                         16 * ((4 * s2 + q) ^ (n & (CPR - 1))));
      xb[s2] = r >= 0 ? v : (bf16x8)(__bf16)0.f;
    }
  } else {
#pragma unroll
    for (int mt = 0; mt < MTI; ++mt) {
      const int c = 8 * (mt >> 1) + 2 * q + (mt & 1);
      const f32x4 v = *reinterpret_cast<const f32x4*>(xw + n * IN + 4 * (c ^ n));
      xv[mt] = r >= 0 ? v : (f32x4)(0.f);
    }
#pragma unroll
    for (int s2 = 0; s2 < NI; ++s2) xb[s2] = rk_pack(xv[2 * s2], xv[2 * s2 + 1]);
  }
  // (the strip row's address in vector registers from here: its scalars end in front of the
  // barrier; typed as a global pointer, since one that went through the pin as a generic pointer
  // is stored through with flat instructions, which turn every counted LDS wait into a full one)
  typedef __attribute__((address_space(1))) bf16x8 glb_bf16x8;
  glb_bf16x8* xrow = (glb_bf16x8*)(xt_t + m * in_max);
  asm volatile("" : "+v"(xrow));
  __builtin_amdgcn_sched_barrier(0);
  __syncthreads();  // barrier 1: the image wave's DMAs landed before it arrived
  RK_STAMP(3);
  // ---- the fragment pipeline starts: layer 0's k-step 0, the first thing issued behind barrier 1
  // and never in front of it (the LDS still holds the previous launch's image there: the previous
  // step's weights, stale by one Adam step, returned without a stall)
  const char* img0 = wimg + t * RK_IMG_T;
  const char* img1 = img0 + RK_W0 * 256;
  bf16x8 fa[2][8];
  rk_frags<8, false>(fa[0], img0, 0, lane);
  __builtin_amdgcn_sched_barrier(0);
  // the T1 -> T2 strip of X (row-major), fire-and-forget: issued before the layer's MFMAs so the
  // stores drain under them (likewise h's after layer 0, the dZ strips before dX)
  if (!TDBG(512)) {  // (TDBG: timing only)
#pragma unroll
    for (int s = 0; s < NI; ++s) xrow[4 * s + q] = xb[s];  // rk_strip's stores
  }
  // UPD, past barrier 1 (nothing waits on these until the row update; the claim landed with the id,
  // so neither waits for a round trip here): the slot word (its low half holds the lookup count:
  // DD_CNT_BITS < 32, little-endian) and the row's state — unconditional loads at clamped indices
  // (a branch around a load pulls its first use, and the wait for it, into the branch); the state
  // is used only for a single-lookup row. Issued before the row DMA, the two random loads held the
  // DMA's issue back 1.4 us (profiles/r05_t1_claim_ab.log)
  uint32_t word = 0u;
  float s_old = 0.f;
  if (UPD) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {  // the table's hot-row count for the tail (dd_update_block)
      int32_t* const ctr = C.ctr;
      const int32_t nh = ctr[0];
      ctr[2] = nh;
      ctr[0] = 0;
    }
    word = reinterpret_cast<const uint32_t*>(&slots[cl >= 0 ? cl : 0].word)[0];
    s_old = us_t[r >= 0 ? r : 0];
  }
  __builtin_amdgcn_sched_barrier(0);
  auto no_fill = [](int) {};
  // ---- 1. layer 0: h^T = relu(W0 X^T + b0), 8 M-tiles x 4 k-steps (then W1's k-step 0)
  f32x4 acc[8];
  rk_gemm<8, NI, false>(acc, fa, img0, xb, lane, [&](bf16x8(&f)[8]) { rk_frags<4, false>(f, img1, 0, lane); }, no_fill);
  RK_STAMP(4);
  bf16x8 hb[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    f32x4 u0, u1;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      u0[j] = fmaxf(acc[2 * s][j] + b0v[2 * s][j], 0.f);
      u1[j] = fmaxf(acc[2 * s + 1][j] + b0v[2 * s + 1][j], 0.f);
    }
    hb[s] = rk_pack(u0, u1);
  }
  if (!TDBG(256)) rk_strip<4>(hb, act_t + m * MAXW, q);
  // ---- 2. layer 1: out^T = relu(W1 h^T + b1) (fp32), 4 M-tiles x 4 k-steps; exchanged in LDS
  // (then dZ0's k-step 0, W1^T: the exchange, barrier 2, the logit, the BCE and dZ1 run under it)
  f32x4 uo[4];
  rk_gemm<4, 4, false>(acc, fa, img1, hb, lane, [&](bf16x8(&f)[8]) { rk_frags<8, true>(f, img1, 0, lane); }, no_fill);
  // ---- the update batch (the rest of the tower's line 1, the table rows, RkCommon line 1): issued
  // here, so that barrier 2's full LDS wait, which the exchange pays anyway, covers their round
  // trip. Scalar loads return out of order: one in flight turns every counted LDS wait of a product
  // into a full one, so none is outstanding between barrier 2 and the end of dX (the pin behind the
  // barrier keeps the loads here instead of at their uses, the list's inside its branch). The
  // gradient rows and the logits come with it, except with UPD, which has no scalar register to
  // spare across the backward products and fetches them under the write-back's one LDS wait; the
  // bias and loss partials' bases come under barrier 3's wait in every form
  __bf16* const dzt0_t = T.dzt0;
  __bf16* const dzt1_t = T.dzt1;
  float* const uw_t = T.uw;
  const float ulr = C.ulr, ueps = C.ueps;
  const int nseg = C.nseg;
  float* grow_t = nullptr;
  float* prow_t = nullptr;
  int64_t ldp = 0;
  float* logits = nullptr;
  if constexpr (!UPD) {
    grow_t = T.grow;
    prow_t = T.prow;
    ldp = C.ldp;
    logits = C.logits;
  }
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) uo[mt] = acc[mt];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) {
#pragma unroll
    for (int j = 0; j < 4; ++j) uo[mt][j] = fmaxf(uo[mt][j] + b1v[mt][j], 0.f);
    const int c = 8 * (mt >> 1) + 2 * q + (mt & 1);  // 16-B chunk of the 64-float row
    *reinterpret_cast<f32x4*>(&xo[t][h][n * 64 + ((c ^ n) << 2)]) = uo[mt];
  }
  RK_STAMP(5);
  RK_STAMP(6);
  __syncthreads();
  if (UPD) asm volatile("" ::"s"(dzt0_t), "s"(dzt1_t), "s"(uw_t), "s"(ulr), "s"(ueps), "s"(nseg));
  else asm volatile("" ::"s"(dzt0_t), "s"(dzt1_t), "s"(grow_t), "s"(prow_t), "s"(ldp), "s"(logits));
  RK_STAMP(7);
  // ---- 3. logit (both towers compute it: the same products in the same order), BCE, dlogit
  f32x4 vo[4];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) {
    const int c = 8 * (mt >> 1) + 2 * q + (mt & 1);
    vo[mt] = *reinterpret_cast<const f32x4*>(&xo[t ^ 1][h][n * 64 + ((c ^ n) << 2)]);
  }
  // the summation tree of tower_l2_kernel's logit (bit-identical logits): per group of 4 columns
  // an fma chain from 0, groups g = 16 s' + ... combined at group bits 0 (in lane), 1 (lanes ^ 16),
  // 2 (lanes ^ 32), 3 (in lane); uo[mt] holds group 8 (mt >> 1) + 2 q + (mt & 1)
  float gs[4];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) {
    float e = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) e = fmaf(uo[mt][j], vo[mt][j], e);
    gs[mt] = e;
  }
  float c0 = gs[0] + gs[1], c1 = gs[2] + gs[3];
  c0 += __shfl_xor(c0, 16, 64);
  c1 += __shfl_xor(c1, 16, 64);
  c0 += __shfl_xor(c0, 32, 64);
  c1 += __shfl_xor(c1, 32, 64);
  const float d = c0 + c1;
  float lo = 0.f, dl = 0.f;
  if (live) {
    const float x = d, y = rk_label(lab_raw, label_dtype);
    const float e = __expf(-fabsf(x));
    const float l1p = e < 1e-4f ? e * (1.f - 0.5f * e) : __logf(1.f + e);
    const float lsig = fminf(x, 0.f) - l1p;
    lo = (1.f - y) * x - lsig;
    const float rc = __builtin_amdgcn_rcpf(1.f + e);
    dl = ((x >= 0.f ? rc : e * rc) - y) * (grad_scale / fB);
  }
  // (the row half, the tower and the lane per lane from here on, each from a thread index the
  // compiler cannot share between its uses: the wave-uniform copies and the lane masks shared with
  // the prologue would hold scalar registers from the entry to the end, and the chain has none to
  // spare. Tower 0's lanes q == 0: thread index bits 7, 5 and 4 clear)
  auto tid = [] {
    uint32_t v = threadIdx.x;
    asm volatile("" : "+v"(v));
    return v;
  };
  const int hv = (int)(tid() >> 6) & 1;
  if ((tid() & 0xB0u) == 0u) lrow[16 * hv + n] = lo;
  // ---- 4. dZ1 = dlogit * other * (self > 0) (fp32: bias sums; bf16: the next product, the strip)
  float z1[16];
  bf16x8 z1b[4];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int j = 0; j < 4; ++j) z1[4 * mt + j] = live && uo[mt][j] > 0.f ? dl * vo[mt][j] : 0.f;
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    bf16x8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (__bf16)z1[8 * s + j];
    z1b[s] = v;
  }
  // ---- 5. dZ0^T = (W1^T dZ1^T) * (h > 0): 8 M-tiles x 2 k-steps
  RK_STAMP(8);
  // (then dX's k-step 0, W0^T). The backward products are LDS-bound and leave the vector ALU idle:
  // db1's column sums over the wave's rows (two of rk_colsum's four levels per k-step) run beside
  // this product's MFMAs, db0's beside dX's, each long before the barrier that combines them
  rk_gemm<8, 2, true>(acc, fa, img1, z1b, lane, [&](bf16x8(&f)[8]) { rk_frags<MTI, true>(f, img0, 0, lane); },
                      [&](int s) {
                        rk_colsum_level<16>(z1, n, 2 * s);
                        rk_colsum_level<16>(z1, n, 2 * s + 1);  // lane n: k = n
                      });
  float z0[32];
  bf16x8 z0b[4];
#pragma unroll
  for (int mt = 0; mt < 8; ++mt)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      z0[4 * mt + j] = live && (float)hb[mt >> 1][4 * (mt & 1) + j] > 0.f ? acc[mt][j] : 0.f;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    bf16x8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (__bf16)z0[8 * s + j];
    z0b[s] = v;
  }
  // the dZ strips (T1 -> T2), issued here so they drain beside dX and the row update instead of at
  // the kernel's end
  if (!TDBG(512)) rk_strip<2>(z1b, dzt1_t + m * MAXW, q);
  if (!TDBG(128)) rk_strip<4>(z0b, dzt0_t + m * MAXW, q);
  // ---- 6. dX^T = W0^T dZ0^T: 8 M-tiles x 4 k-steps; acc[mt] = dX features of xv[mt]
  RK_STAMP(9);
  // (the last product: nothing to prefetch; one level of db0's column sums per k-step)
  rk_gemm<MTI, 4, true>(acc, fa, img0, z0b, lane, [](bf16x8(&)[8]) {},
                        [&](int s) { rk_colsum_level<32>(z0, n, s); });  // lane n: k = 2 n + i, i < 2 (k = 4 mt + j)
  // row half 1's bias partials at once (a dead wave's are exact zeros: every z of a dead row is 0.f);
  // feature of value k = 4 mt + j: 32 (mt >> 1) + 8 q + 4 (mt & 1) + j
  auto feat = [&](int k) { return 32 * ((k >> 2) >> 1) + 8 * q + 4 * ((k >> 2) & 1) + (k & 3); };
  if (hv == 1) {
    bsum[t][feat(2 * n)] = z0[0];
    bsum[t][feat(2 * n + 1)] = z0[1];
    bsum[t][RK_W0 + feat(n)] = z1[0];
  }
  RK_STAMP(10);
  // ---- 7. the row: UPD + looked up once -> row-wise Adagrad in place (the K3 update's arithmetic and
  // summation tree: feature groups of 4 combined at group bits 4, 3 (in lane), 2, 1 (lanes ^ 32,
  // ^ 16), 0 (in lane)); otherwise dX -> the pooled gradient (and the gathered row, pooled_out)
  float* grow = nullptr;
  bool store_dx;
  if (IDX) {  // dX -> the requester's gradient row in the send buffer (none for a zero row)
    const int32_t po = (int32_t)pout_raw.lo;
    store_dx = r >= 0 && po >= 0;
    grow = grow_t + (int64_t)(store_dx ? po : 0) * IN;
    if (a.xd.W) grow = reinterpret_cast<float*>(px_row(a.xd, store_dx ? po : 0, IN * 4));
  } else {
    store_dx = live;
  }
  if (UPD) {
    // (the list's base from the line nseg brought into the scalar cache: past the products, under
    // the wait of the shuffles below)
    int32_t* const multi = C.multi;
    __builtin_amdgcn_sched_barrier(0);
    float e2[2];
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      // IN = 64: K3's first level (group bit 4) adds zeros, which is exact: only bit 3 remains
      const float s0 = rw_sq4(acc[0 + hh]), s1 = rw_sq4(acc[2 + hh]);
      float c2;
      if constexpr (IN == 128) {
        const float s2 = rw_sq4(acc[4 + hh]), s3 = rw_sq4(acc[6 + hh]);
        c2 = (s0 + s2) + (s1 + s3);
      } else {
        c2 = s0 + s1;
      }
      c2 += __shfl_xor(c2, 32, 64);
      c2 += __shfl_xor(c2, 16, 64);
      e2[hh] = c2;
    }
    asm volatile("" ::"s"(multi));
    RK_STAMP2(0);
    const float sq = e2[0] + e2[1];
    const float snew = rw_state(s_old, sq, IN);
    const float step = rw_step(snew, ulr, ueps);
    float* us_w;
    const uint32_t cnt = word & (uint32_t)DD_CNT_MASK;
    const bool single = r >= 0 && cl >= 0 && cnt == 1u;
    {
      // this wave's rows looked up 2..DD_INL times (their claiming lookups): the tail's list role
      // updates them (segment = the wave; plain stores, the count written every step)
      const bool mul = q == 0 && r >= 0 && cl >= 0 && cnt >= 2u && cnt <= (uint32_t)DD_INL;
      const uint64_t bal = __ballot(mul);
      const int seg = tile * 4 + wid;
      if (seg < nseg) {  // [count, slots...] (DD_SEGW): the list role reads count + 3 slots at once
        if (mul) multi[(int64_t)seg * DD_SEGW + 1 + __popcll(bal & ((1ull << lane) - 1))] = cl;
        if (lane == 0) multi[(int64_t)seg * DD_SEGW] = __popcll(bal);
      }
    }
    // the updated rows go back through the wave's LDS rows (same chunk swizzle) and out as two
    // whole rows per store instruction, as they came in
#pragma unroll
    for (int mt = 0; mt < MTI; ++mt) {
      const int c = 8 * (mt >> 1) + 2 * q + (mt & 1);
      *reinterpret_cast<f32x4*>(xw + n * IN + 4 * (c ^ n)) = rw_apply(xv[mt], acc[mt], step);
    }
    RK_STAMP2(1);
    asm volatile("" ::: "memory");  // LDS is in order per wave: only the compiler must not reorder
    {
      const int wl = (int)(tid() & 63u);
      const int rr0 = wl / CPR, pc = wl % CPR;
      float* wtab = uw_t;
      // as a batch: every shuffle (the row's index where it is updated here, -1 elsewhere: one
      // value carries the index and the predicate), every LDS read, one wait; then the stores under
      // their predicates, with no LDS instruction and no wait between them
      const int64_t rsend = single ? r : -1;
      int64_t rid[NDMA];
      f32x4 w[NDMA];
      grow_t = T.grow;
      prow_t = T.prow;
      ldp = C.ldp;
      logits = C.logits;
      // the state's base again, through a tower index the compiler cannot match with the entry's:
      // held from the late batch to here it costs the chain the scalar pair it does not have
      int tw = t;
      asm volatile("" : "+s"(tw));
      us_w = const_cast<float*>(a.rk.tw[tw].us);
#pragma unroll
      for (int i = 0; i < NDMA; ++i) rid[i] = __shfl((long long)rsend, RPI * i + rr0, 64);
#pragma unroll
      for (int i = 0; i < NDMA; ++i) w[i] = *reinterpret_cast<const f32x4*>(xw + (RPI * i + rr0) * IN + 4 * pc);
      rk_pin<NDMA>(rid);
      rk_pin<NDMA>(w);
      asm volatile("" ::"s"(grow_t), "s"(prow_t), "s"(ldp), "s"(logits), "s"(us_w));
#pragma unroll
      for (int i = 0; i < NDMA; ++i) {
        const int row = RPI * i + rr0;
        if (__builtin_expect(rid[i] >= 0, 1)) *reinterpret_cast<f32x4*>(wtab + rid[i] * IN + 4 * (pc ^ row)) = w[i];
      }
    }
    RK_STAMP2(2);
    if (single) {
      if (q == 0) {
        us_w[r] = snew;
        slots[cl].word = DD_EMPTY;  // free: nothing else of the step reads a single slot
      }
      store_dx = prow_t != nullptr;  // dX only for inspection
    }
  }
  if (!IDX) grow = grow_t + m * ldp;  // (store_dx: live rows only)
  if (store_dx) {
#pragma unroll
    for (int mt = 0; mt < MTI; ++mt)
      *reinterpret_cast<f32x4*>(grow + 32 * (mt >> 1) + 8 * q + 4 * (mt & 1)) = acc[mt];
  }
  RK_STAMP2(3);
  if ((tid() & 0xB0u) == 0u && live) logits[m] = d;  // after the row update (see rk_strip)
  if (!IDX && !POOL && prow_t && live) {
    float* prow = prow_t + m * ldp;
#pragma unroll
    for (int mt = 0; mt < MTI; ++mt) *reinterpret_cast<f32x4*>(prow + 32 * (mt >> 1) + 8 * q + 4 * (mt & 1)) = xv[mt];
  }
  RK_STAMP(11);
  // ---- 8. bias partials (the wave's column sums from under the backward products: row half 0 +
  // row half 1); the loss partial (the tile's 32 row losses in order)
  RK_STAMP(12);
  float* const db0_t = T.db0;
  float* const db1_t = T.db1;
  float* const loss_part = C.loss_part;
  __builtin_amdgcn_sched_barrier(0);
  RK_STAMP(13);
  __syncthreads();
  asm volatile("" ::"s"(db0_t), "s"(db1_t), "s"(loss_part));
  RK_STAMP(14);
  if (hv == 0) {
    float* db0 = db0_t + (int64_t)tile * MAXW;  // by tile: T2 sums them in tile order
    float* db1 = db1_t + (int64_t)tile * MAXW;
    db0[feat(2 * n)] = z0[0] + bsum[t][feat(2 * n)];
    db0[feat(2 * n + 1)] = z0[1] + bsum[t][feat(2 * n + 1)];
    db1[feat(n)] = z1[0] + bsum[t][RK_W0 + feat(n)];
    if (tid() == 0u) {
      // the 32 row losses as one batch of reads and one wait, then the adds in the order i = 0 .. 31
      f32x4 lv[TR / 4];
#pragma unroll
      for (int i = 0; i < TR / 4; ++i) lv[i] = reinterpret_cast<const f32x4*>(lrow)[i];
      rk_pin<TR / 4>(lv);
      float p = 0.f;
#pragma unroll
      for (int i = 0; i < TR; ++i) p += lv[i >> 2][i & 3];
      loss_part[tile] = p;
    }
  }
  // every row's overflow entry is written (EMPTY for a dropped id or a dead row of a ragged tile):
  // the resolver reads all 64 entries of the group
  if (!UPD && a.dd_on && q == 0) dd_insert_defer_finish_at(a.dd, pend, li, tile, 16 * wid + n);
  if constexpr (IDX) {
    if (cpd) *cpd = cpv;
    if (a.xd.W) {  // a share past 256 units (not at the sharded steps' sizes)
      for (int64_t u = (int64_t)blockIdx.x * cp_per + threadIdx.x + 256; u < cp_end; u += 256) {
        const uint4* s2;
        uint4* d2;
        if (px_copy_unit(a.xd, u, s2, d2)) *d2 = *s2;
      }
    }
    // the exchange's epoch advances with its producer (a consumer that signals / waits in-launch
    // reads it after this kernel's boundary)
    if (a.xd.epoch && blockIdx.x == 0 && threadIdx.x == 0)
      __hip_atomic_fetch_add(a.xd.epoch, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  RK_STAMP(15);
}
template <bool UPD, bool IDX = false, int IN = 128, bool POOL = false>
__global__ void __launch_bounds__(RK_THREADS) tower_rows_kernel(TowerArgs a) {
  tower_rows_body<UPD, IDX, IN, POOL>(a);
}

// the row-owned T1's argument front from the filled TowerArgs (gather, indexed or pooled input)
static void rk_front(TowerArgs& a, bool pool) {
  RkCommon& c = a.rk.c;
  c.B = a.B;
  c.labels = a.labels;
  c.label_dtype = a.label_dtype;
  c.gid_dtype = a.gid_dtype;
  c.grad_scale = a.grad_scale;
  c.in_max = (int32_t)a.in_max;
  c.slots = a.dd.slots;
  c.ctr = a.dd.ctr;
  c.ulr = a.ulr;
  c.nwg = a.nwg;
  c.fB = (float)a.B;
  c.ueps = a.ueps;
  c.ldp = a.ldp;
  c.multi = a.dd.multi;
  c.logits = a.logits;
  c.loss_part = a.loss_part;
  c.nseg = a.dd.nseg;
  const bool idx = a.gpos[0] != nullptr;
  for (int t = 0; t < 2; ++t) {
    RkTower& w = a.rk.tw[t];
    w.idcol = idx ? static_cast<const void*>(a.gpos[t]) : a.gcol[t];
    w.tab = idx ? static_cast<const void*>(a.gsrc[t]) : pool ? static_cast<const void*>(a.pooled + a.s.in_col[t]) : a.gtab[t];
    w.gmod = a.gmod[t];
    w.b0 = a.params + a.boff[t][0];
    w.b1 = a.params + a.boff[t][1];
    w.claim = a.uw[0] ? a.dd.claim + (int64_t)t * a.B : nullptr;
    w.pos_out = a.gpos_out[0] ? a.gpos_out[t] : nullptr;
    w.rstride = a.ldp;
    w.xt = a.xt + (int64_t)t * a.in_max * a.Bp;
    w.act0 = a.act + ((int64_t)t * MAXL + 0) * MAXW * a.Bp;
    w.dzt0 = a.dzt + ((int64_t)t * MAXL + 0) * MAXW * a.Bp;
    w.dzt1 = a.dzt + ((int64_t)t * MAXL + 1) * MAXW * a.Bp;
    w.us = a.us[t];
    w.uw = a.uw[t];
    w.grow = idx ? a.gdst[t] : a.gpooled + a.s.in_col[t];
    w.prow = a.pooled_out ? a.pooled_out + a.s.in_col[t] : nullptr;
    w.db0 = a.dbpart + ((int64_t)t * MAXL + 0) * a.nwg * MAXW;
    w.db1 = a.dbpart + ((int64_t)t * MAXL + 1) * a.nwg * MAXW;
  }
}

// the row-owned T1 for a filled TowerArgs (an L.rows shape): single-hot ids with or without the
// in-place update, bf16 rows by position, or the pooled matrix
int launch_t1_rows(TowerArgs& a, void* stream) {
  const dim3 g(a.nwg), b(RK_THREADS);
  const bool in64 = a.s.in_dim[0] == 64;
  if (!a.gcol[0] && !a.gpos[0]) {  // pooled input (the multi-hot path after tt_pooled_fwd)
    rk_front(a, true);
    in64 ? tower_rows_kernel<false, false, 64, true><<<g, b, 0, as_stream(stream)>>>(a)
         : tower_rows_kernel<false, false, 128, true><<<g, b, 0, as_stream(stream)>>>(a);
    return check_launch("tower_rows_pooled");
  }
  rk_front(a, false);
  if (a.gpos[0])
    in64 ? tower_rows_kernel<false, true, 64><<<g, b, 0, as_stream(stream)>>>(a)
         : tower_rows_kernel<false, true, 128><<<g, b, 0, as_stream(stream)>>>(a);
  else if (a.uw[0])
    in64 ? tower_rows_kernel<true, false, 64><<<g, b, 0, as_stream(stream)>>>(a)
         : tower_rows_kernel<true, false, 128><<<g, b, 0, as_stream(stream)>>>(a);
  else
    in64 ? tower_rows_kernel<false, false, 64><<<g, b, 0, as_stream(stream)>>>(a)
         : tower_rows_kernel<false, false, 128><<<g, b, 0, as_stream(stream)>>>(a);
  return check_launch(a.uw[0] ? "tower_rows_gather_update" : "tower_rows_gather");
}

}  // namespace tt
