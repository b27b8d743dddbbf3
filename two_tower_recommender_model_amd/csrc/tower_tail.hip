// What runs behind T1 in the fused tower step (tower.hip): T2 (the dW tiles), the next batch's insert
// role, T3 (reduce, Adam, the weight copies), the kernels that combine them with the row-wise Adagrad
// and the sharded step's roles, their arguments and launches.
#include "tower_common.h"

namespace tt {

// ---------------------------------------------------------------------------------------------
// T3: reduce + Adam + bf16 weight copies

// One segment of the flat parameter vector, W or b of (t, l), is a 16-B record, so the table is four
// 64-B lines that t3_seg fetches two at a time (every offset is far below 2^31: the shape limits
// bound P at 2 (1024 x 128 + 3 x 128 x 128 + 4 x 128)). A vector type: the records are pinned in
// SGPRs, four registers each.
//   .x  first element in params (INT32_MAX: unused record, never selected)
//   .y  W: element offset in the bf16 copies
//   .z  n | k << 16 (b: k = 1)
//   .w  isw | t << 1 | l << 2
typedef uint32_t t3_u32x4 __attribute__((ext_vector_type(4)));
constexpr int T3_NSEG = 2 * 2 * MAXL;

struct alignas(64) UpdateArgs {
  // line 0: all that stands in front of update_block's first slab, parameter and moment loads
  float* params;
  float* exp_avg;
  float* exp_avg_sq;
  const float* slab;
  const float* adam_pre;  // nullable: step size / sqrt(bias correction 2) precomputed by T2 (which
                          // also advanced step_state): no pow() and no arrival ticket here
  const float* grads_in;  // nullable: take the gradient from here (data-parallel: all-reduced)
  int32_t P;
  int S;
  int do_adam;
  int nseg;
  // lines 1..4: the segment table, ascending offsets; two layers' eight records are lines 1..2
  t3_u32x4 seg[T3_NSEG];
  const float* dbpart;
  int nwg;
  __bf16* wb;
  __bf16* wtb;
  __bf16* wbf;
  __bf16* wtbf;
  int skip_plain;  // wb / wtb unused by this shape's T1 (tower_l2_kernel): not written
  float lr, beta1, beta2, eps, wd;
  int64_t* step_state;
  float* grads_out;  // nullable: the reduced gradient (tests / inspection)
  // data-parallel towers without an all-reduce launch (pipelined sharded step): grads_out is
  // written out_copies times (stride out_stride, scaled by out_scale: one copy per destination
  // rank of the exchange), and grads_in is the fixed-order sum of in_srcs vectors (stride in_stride)
  int out_copies;
  int64_t out_stride;
  int64_t out_off[16];  // with out_copies > 1: element offset of copy q (explicit, out_stride unused)
  float out_scale;
  int in_srcs;
  int64_t in_stride;
  char* wimg;  // nullable: the row-owned T1's weight image (rk_off), written beside the other copies
  PxWait wt;   // W > 0: every workgroup waits for the exchange that brought grads_in (workgroup 0 signals)
#if TT_EXPERIMENTS
  int64_t* stamps;  // EXPERIMENT (TT_RING_STAMPS): [workgroups][4] s_memrealtime per phase
#endif
};
// T3's workgroup size: every launch of update_block is 256 wide (a constant, so that no load of the
// launch dimensions stands in front of the slab loads); the experiment build also tries 128
#if TT_EXPERIMENTS
#define T3_BLOCK ((int)blockDim.x)
#else
#define T3_BLOCK 256
#endif
#if TT_EXPERIMENTS
#define T3_STAMP(k) \
  do { if (a.stamps && threadIdx.x == 0 && bid < 512) a.stamps[(int64_t)bid * 4 + (k)] = (int64_t)__builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define T3_STAMP(k) do { } while (0)
#endif

// one parameter's segment (W or b of tower t, layer l): per-lane compares and selects over the
// table held in SGPRs — no load and no branch per segment. update_block calls this behind its slab
// loads, which need no segment. A per-lane index into the kernarg table would be a chain of
// dependent vector loads from the kernarg segment (several us per launch); a scalar load per
// segment inside `if (i >= off[q])` was about twenty serial scalar round trips in front of the
// slab loads.
struct T3Seg {
  int64_t soff = 0, swc = 0;
  int sisw = 0, sk = 1, sn = 1, st_ = 0, sl_ = 0;
};
__device__ __forceinline__ T3Seg t3_seg(const UpdateArgs& a, int64_t i, int nseg) {
  // the last record at or below i wins (ascending offsets); unused records hold INT32_MAX (i < P)
  const int32_t ii = (int32_t)i;
  int32_t off = 0, wc = 0;
  uint32_t nk = 1u | 1u << 16, meta = 0;
  // eight records (two 64-B lines) at a time: their scalar loads issued together, one wait (the
  // empty asm holds all eight in SGPRs at once; left alone they load and wait line by line)
  const auto half = [&](int q0) {
    t3_u32x4 r[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) r[q] = a.seg[q0 + q];
    asm volatile("" ::"s"(r[0]), "s"(r[1]), "s"(r[2]), "s"(r[3]), "s"(r[4]), "s"(r[5]), "s"(r[6]), "s"(r[7]));
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const bool c = ii >= (int32_t)r[q].x;
      off = c ? (int32_t)r[q].x : off;
      wc = c ? (int32_t)r[q].y : wc;
      nk = c ? r[q].z : nk;
      meta = c ? r[q].w : meta;
    }
  };
  half(0);
  if (nseg > 8) half(8);  // three or four layers
  T3Seg g;
  g.soff = off;
  g.swc = wc;
  g.sisw = (int)(meta & 1u);
  g.st_ = (int)(meta >> 1 & 1u);
  g.sl_ = (int)(meta >> 2);
  g.sn = (int)(nk & 0xffffu);
  g.sk = (int)(nk >> 16);
  return g;
}

// after the gradient g of parameter i (value p): gradient copies, Adam, the bf16 copies T1 reads
__device__ __forceinline__ void t3_apply(const UpdateArgs& a, int64_t i, const T3Seg& sg, float p, float m,
                                         float v0, float g, float step_size, float bc2_sqrt, bool adam) {
  // no fma contraction: the contraction choice would otherwise depend on the inlining context (T3,
  // the sharded step's launch G), and every form must give the same bits
#pragma clang fp contract(off)
  const int64_t e = i - sg.soff;
  if (a.grads_out) {
    if (a.out_copies <= 1) {
      a.grads_out[i] = g;
    } else {
      const float gs = g * a.out_scale;
      for (int q = 0; q < a.out_copies; ++q) a.grads_out[a.out_off[q] + i] = gs;
    }
  }
  if (adam) {
    if (a.wd != 0.f) g = g + a.wd * p;
    m = m + (1.f - a.beta1) * (g - m);
    const float v = v0 * a.beta2 + (1.f - a.beta2) * g * g;
    const float denom = sqrtf(v) / bc2_sqrt + a.eps;
    p = p + (-step_size) * m / denom;
    a.exp_avg[i] = m;
    a.exp_avg_sq[i] = v;
    a.params[i] = p;
  }
  if (sg.sisw) {
    const int K = sg.sk, N = sg.sn;
    const int64_t n = e / K, k = e - n * K;
    if (!a.skip_plain) {
      a.wb[sg.swc + e] = (__bf16)p;
      a.wtb[sg.swc + k * N + n] = (__bf16)p;
    }
    a.wbf[sg.swc + frag_off((int)n, (int)k, K)] = (__bf16)p;   // W as [N][K]
    a.wtbf[sg.swc + frag_off((int)k, (int)n, N)] = (__bf16)p;  // W^T as [K][N]
    if (a.wimg)  // the row-owned T1's image: W [out][in], 256-B swizzled rows, W1 after W0
      *reinterpret_cast<__bf16*>(a.wimg + sg.st_ * RK_IMG_T + sg.sl_ * (RK_W0 * 256) + rk_off((int)n, (int)k)) = (__bf16)p;
  }
}

// ---------------------------------------------------------------------------------------------
// T2: dW_(t,l)[n][k] = sum_m dZ_(t,l)[m][n] * A_(t,l)[m][k], A = X (l=0) or act_(t,l-1)


struct WgradArgs {
  const __bf16* xt;
  const __bf16* act;
  const __bf16* dzt;
  float* slab;  // [S][P]
  int64_t P;
  int64_t B;
  int64_t in_max;
  int64_t Bp;      // strip rows per block (strip_at)
  int S;
  int64_t mslice;  // rows per slice (multiple of 32)
  int ntiles;
  int64_t woff[2][MAXL];
  int64_t boff[2][MAXL];
  int32_t K[2][MAXL];  // layer input width
  int32_t width[MAXL];
  int L;
  const float* dbpart;
  int nwg;
  const float* loss_part;  // [nwg] T1 partials
  float* loss;             // nullable
  int nbias;
  int64_t tiles_off;       // byte offset of the tile list in the workspace (host side)
  // Adam's per-step scalars for the T3 that follows (nullable): t = ++step_state[0];
  // adam_pre = {lr / (1 - beta1^t), sqrt(1 - beta2^t)} — one thread, once, instead of every T3
  // thread evaluating pow() and an arrival ticket advancing the counter
  int64_t* step_state;
  float* adam_pre;
  float lr, beta1, beta2;
  // staged path (every K <= 128): tiles of T2_NT dW rows x the whole K, (t, l, n0) per tile
  int lds;
  int rm;  // row-major operand strips ([Bp][features], the row-owned T1's shape): wgrad_lds_block_rm
  int32_t t2_code[16];  // t | l << 4 | n0 << 8
#if TT_EXPERIMENTS
  int64_t* stamps;      // EXPERIMENT (TT_T2_STAMPS): [workgroups][8] s_memrealtime per phase
#endif
  DedupWs dd;           // tt_tower_wgrad_pre with a dedup workspace: the first n_res workgroups
  int n_res;            //   finish T1's deferred inserts (dd_resolve_block)
};

#if TT_EXPERIMENTS
#define T2_STAMP(k) \
  do { if (a.stamps && threadIdx.x == 0) a.stamps[(int64_t)blockIdx.x * 8 + (k)] = (int64_t)__builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define T2_STAMP(k) do { } while (0)
#endif

// the staged T2's LDS (T2_NT, T2_MB, T2_PF and what they mean: tower_common.h)
constexpr int T2_STR = T2_MB + 8;                      // bf16 LDS row stride (80 B: conflict-free b128)
constexpr int T2_ROWS = T2_NT + MAXW;                  // Z rows [0, 64) + A rows [64, 64 + K)
constexpr int T2_LDS = 2 * T2_ROWS * T2_STR * 2;       // bytes (30,720)
constexpr int T2_RED = 3 * 64 * 16 * 4;                // bytes of the register-path reduction
constexpr int T2R_STR = 208;                           // bf16 per LDS row of a row-major chunk (416 B)
constexpr int T2R_RING = 3;                            // chunk buffers of the row-major full-pass ring
constexpr int T2R_LDS = T2R_RING * TR * T2R_STR * 2;   // bytes (39,936)
constexpr int T2_SMEM0 = T2_LDS > T2_RED ? T2_LDS : T2_RED;
constexpr int T2_SMEM1 = T2_SMEM0 > T2R_LDS ? T2_SMEM0 : T2R_LDS;
constexpr int T2_SMEM = T2_SMEM1 > DD_SMEM ? T2_SMEM1 : DD_SMEM;  // the combined launch shares it with dedup.h


__device__ __forceinline__ void wgrad_lds_block(const WgradArgs& a, int lb, char* smem) {
  __bf16* buf = reinterpret_cast<__bf16*>(smem);
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int r = lane & 15, q = lane >> 4;
  // lb is workgroup-uniform: readfirstlane keeps the tile lookup a scalar kernarg load (a VGPR index
  // would be a vector load from the kernarg segment, a dependent hop before the first operand load)
  const int s = __builtin_amdgcn_readfirstlane(lb / a.ntiles), ti = __builtin_amdgcn_readfirstlane(lb % a.ntiles);
  T2_STAMP(0);
  const int code = a.t2_code[ti];
  const int t = code & 15, l = (code >> 4) & 15, n0 = code >> 8;
  const int K = a.K[t][l];
  const int NT = min(T2_NT, a.width[l] - n0);  // 64, or 32 for the last tile of a width % 64 layer
  const int64_t B = a.B;
  const __bf16* Z = a.dzt + ((int64_t)t * MAXL + l) * MAXW * a.Bp;  // strip blocks (strip_at)
  const __bf16* A = l == 0 ? a.xt + (int64_t)t * a.in_max * a.Bp : a.act + ((int64_t)t * MAXL + l - 1) * MAXW * a.Bp;
  const int64_t anf = l == 0 ? a.in_max : MAXW;
  const int64_t mb = (int64_t)s * a.mslice;
  const int64_t me = min(mb + a.mslice, B);
  // loader: 4 threads per 64-B operand row segment (32 batch rows), 64 rows per pass; row i's
  // chunk at batch row m (a multiple of 32) starts at src[i] + (m / 32) * tstr[i]
  const int seg = (tid & 3) * 8, frow = tid >> 2;
  const __bf16* src[3];
  int64_t tstr[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int f = frow + 64 * i;
    src[i] = f < T2_NT ? (f < NT ? Z + ((int64_t)(n0 + f) << 5) : nullptr)
                       : (f - T2_NT < K ? A + ((int64_t)(f - T2_NT) << 5) : nullptr);
    tstr[i] = (f < T2_NT ? (int64_t)MAXW : anf) << 5;
  }
  const int nh = wid >> 1, kh = wid & 1;  // wave: dW rows [32 nh, +32) x columns [64 kh, +64)
  f32x4 acc[2][4];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4)(0.f);
  for (int64_t p0 = mb; p0 < me; p0 += T2_PF * T2_MB) {
    bf16x8 ld[T2_PF][3];
#pragma unroll
    for (int c = 0; c < T2_PF; ++c) {
      const int64_t m = p0 + c * T2_MB + seg;  // B % 8 == 0: a segment is wholly in or out
#pragma unroll
      for (int i = 0; i < 3; ++i)
        ld[c][i] = (src[i] && m < me) ? *reinterpret_cast<const bf16x8*>(src[i] + (m >> 5) * tstr[i] + seg)
                                      : (bf16x8)(__bf16)0.f;
    }
#pragma unroll
    for (int c = 0; c < T2_PF; ++c) {
      if (p0 + c * T2_MB >= me) break;  // uniform: the slice's tail
      __bf16* d = buf + (c & 1) * T2_ROWS * T2_STR;
#pragma unroll
      for (int i = 0; i < 3; ++i)
        if (src[i]) *reinterpret_cast<bf16x8*>(d + (frow + 64 * i) * T2_STR + seg) = ld[c][i];
      __syncthreads();  // one barrier per chunk: buffer c & 1 was last read two chunks ago
      if (c == 0 && p0 == mb) T2_STAMP(1);
      bf16x8 fa[2], fb[4];
#pragma unroll
      for (int i = 0; i < 2; ++i) fa[i] = *reinterpret_cast<const bf16x8*>(d + (nh * 32 + i * 16 + r) * T2_STR + q * 8);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        fb[j] = *reinterpret_cast<const bf16x8*>(d + (T2_NT + kh * 64 + j * 16 + r) * T2_STR + q * 8);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (nh * 32 + i * 16 < NT && kh * 64 + j * 16 < K)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
    }
  }
  T2_STAMP(2);
  // C[n][k]: row n = 4q + rr, column k = r of each 16 x 16 block
  float* dst = a.slab + (int64_t)s * a.P + a.woff[t][l];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (nh * 32 + i * 16 < NT && kh * 64 + j * 16 < K)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const int n = n0 + nh * 32 + i * 16 + q * 4 + rr;
          const int k = kh * 64 + j * 16 + r;
          dst[(int64_t)n * K + k] = acc[i][j][rr];
        }
  T2_STAMP(3);
}

// staged T2 over ROW-MAJOR operand strips ([Bp][features] bf16: what the row-owned T1 and the
// fixed-shape tower_l2_kernel write for the [128, 64] towers over 128-wide inputs): a chunk of 32 batch
// rows x [T2_NT dZ features | K layer-input features] goes to LDS as 32 rows at a 416-B stride
// (whole 16-B pieces of rows, three loads per thread as in wgrad_lds_block), and the fragments are
// transposed reads (ds_read_b64_tr_b16). K-slot (q, j) of every fragment is chunk row
// 4 q + (j & 3) + 16 (j >> 2): the 32 lanes of a read then address 8 consecutive rows, which the
// 416-B stride (= 160 mod 256) spreads over all 64 banks.
// The first pass of a slice, when it holds all 256 rows of a full tile, runs t2r_full_pass (pipelined
// over a ring of T2R_RING chunk buffers, no predicate); every other pass runs the general loop in
// wgrad_lds_block_rm (two buffers, a chunk at a time, rows and features predicated). Later passes of
// a slice of more than 256 rows stay on the general loop: pipelined, their accumulators live across
// the pass loop beside the 24 loads and two fragment sets do not fit the tail's 168 registers
static_assert(T2R_LDS <= T2_SMEM, "the row-major staged chunks fit the tail's LDS");
__device__ __forceinline__ bf16x8 t2r_frag(const __bf16* d, int col0, int lane) {
  const int q = lane >> 4, qq = (lane >> 2) & 3, p = lane & 3;
  const __bf16* base = d + (4 * q + qq) * T2R_STR + col0 + 4 * p;
  const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)base);
  const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(base + 16 * T2R_STR));
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}
// The FIRST pass of a slice in wgrad_lds_block_rm when it is full: all T2_PF chunks inside the slice and every piece inside the
// tile (NT = 64, K = 64 or 128), so nothing is zeroed and nothing is predicated: no MFMA behind an
// exec-mask branch. Chunk c lives in ring buffer c % T2R_RING. Iteration c issues chunk c + 1's
// fragment reads and chunk c + 2's LDS writes in among chunk c's MFMAs (the sched_group_barriers
// pin that interleave), then the chunk's one barrier: the reads of chunk c + 1 were issued a whole
// MFMA group before they are waited for, and the MFMAs of chunk c are in flight at the barrier.
// Buffer (c + 2) % 3 was last read for chunk c - 1, by reads every wave completed before the
// barrier of iteration c - 1. `more` (another pass follows, which restarts at buffers 0 and 1 =
// chunks 6 and 7 here) keeps the barrier behind chunk 6's MFMAs; the last pass drops it.
// Every accumulator takes the MFMAs of the general loop, same operands, same chunk order.
// ACT = false: a wave whose 64 dW columns lie past K (kh = 1 at K = 64) stages and joins the
// barriers only. Chunk 0 accumulates onto a literal zero: acc need not be set by the caller (32
// zeroed registers would otherwise live beside the 24 loads in flight).
// The sched_barriers keep the MFMAs, which are free to cross an s_barrier, in their own chunk.
template <bool ACT>
__device__ __forceinline__ void t2r_full_pass(const WgradArgs& a, bool more, const bf16x8 (&ld)[T2_PF][3],
                                              __bf16* buf, int lw0, int lw1, int lw2, int nh, int kh, int lane,
                                              f32x4 (&acc)[2][4]) {
  auto stage = [&](int c) {
    __bf16* d = buf + (c % T2R_RING) * TR * T2R_STR;
    *reinterpret_cast<bf16x8*>(d + lw0) = ld[c][0];
    *reinterpret_cast<bf16x8*>(d + lw1) = ld[c][1];
    *reinterpret_cast<bf16x8*>(d + lw2) = ld[c][2];
  };
  auto frags = [&](int c, bf16x8 (&f)[6]) {
    const __bf16* d = buf + (c % T2R_RING) * TR * T2R_STR;
#pragma unroll
    for (int i = 0; i < 2; ++i) f[i] = t2r_frag(d, nh * 32 + i * 16, lane);
#pragma unroll
    for (int j = 0; j < 4; ++j) f[2 + j] = t2r_frag(d, T2_NT + kh * 64 + j * 16, lane);
  };
  bf16x8 f[2][6];
  stage(0);
  stage(1);
  __syncthreads();
  T2_STAMP(1);
  if (ACT) frags(0, f[0]);
#pragma unroll
  for (int c = 0; c < T2_PF; ++c) {
    __builtin_amdgcn_sched_barrier(0);
    if (c + 2 < T2_PF) stage(c + 2);
    if (ACT && c + 1 < T2_PF) frags(c + 1, f[(c + 1) & 1]);
    if (ACT) {
      // j outside i: a B fragment is dead after its two MFMAs, the next chunk's reuses its registers
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 2; ++i)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f[c & 1][i], f[c & 1][2 + j],
                                                              c == 0 ? (f32x4)(0.f) : acc[i][j], 0, 0, 0);
      if (c + 1 < T2_PF) {
        if (c + 2 < T2_PF) __builtin_amdgcn_sched_group_barrier(0x200, 3, 0);  // the 3 DS writes
        __builtin_amdgcn_sched_group_barrier(0x8, 1, 0);  // 1 MFMA
#pragma unroll
        for (int k = 0; k < 6; ++k) {
          __builtin_amdgcn_sched_group_barrier(0x8, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);  // 2 DS reads: one fragment
        }
        __builtin_amdgcn_sched_group_barrier(0x8, 1, 0);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    if (c + 2 < T2_PF || (c + 2 == T2_PF && more)) __syncthreads();
  }
}
__device__ __forceinline__ void wgrad_lds_block_rm(const WgradArgs& a, int lb, char* smem) {
  __bf16* buf = reinterpret_cast<__bf16*>(smem);
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, q = lane >> 4;
  const int s = __builtin_amdgcn_readfirstlane(lb / a.ntiles), ti = __builtin_amdgcn_readfirstlane(lb % a.ntiles);
  T2_STAMP(0);
  const int code = a.t2_code[ti];
  const int t = code & 15, l = (code >> 4) & 15, n0 = code >> 8;
  const int K = a.K[t][l];
  const int NT = min(T2_NT, a.width[l] - n0);
  const int64_t B = a.B;
  const __bf16* Z = a.dzt + ((int64_t)t * MAXL + l) * MAXW * a.Bp;  // [Bp][MAXW]
  const __bf16* A = l == 0 ? a.xt + (int64_t)t * a.in_max * a.Bp : a.act + ((int64_t)t * MAXL + l - 1) * MAXW * a.Bp;
  const int64_t anf = l == 0 ? a.in_max : MAXW;
  const int64_t mb = (int64_t)s * a.mslice;
  const int64_t me = min(mb + a.mslice, B);
  // loader: piece 0 = dZ row tid >> 3, features n0 + 8 (tid & 7); pieces 1, 2 = layer-input row
  // idx >> 4, features 8 (idx & 15), idx = tid + 256 (i - 1); LDS column of a piece: dZ at 0, layer
  // input at T2_NT. Uniform block bases + 32-bit per-thread byte offsets (one address VGPR per load
  // of the 24 in flight: the tail kernel's roles share its register allocation)
  const char* zb = reinterpret_cast<const char*>(Z);
  const char* ab = reinterpret_cast<const char*>(A);
  const int prow0 = tid >> 3, prow1 = tid >> 4, prow2 = (tid + 256) >> 4;
  const bool ok0 = 8 * (tid & 7) < NT, ok1 = 8 * (tid & 15) < K, ok2 = 8 * ((tid + 256) & 15) < K;
  const uint32_t zstr = MAXW * 2, astr = (uint32_t)anf * 2;  // bytes per strip row
  const uint32_t zo = (uint32_t)(mb + prow0) * zstr + (uint32_t)(n0 + 8 * (tid & 7)) * 2;
  const uint32_t ao1 = (uint32_t)(mb + prow1) * astr + (uint32_t)(8 * (tid & 15)) * 2;
  const uint32_t ao2 = (uint32_t)(mb + prow2) * astr + (uint32_t)(8 * ((tid + 256) & 15)) * 2;
  const int lw0 = prow0 * T2R_STR + 8 * (tid & 7);
  const int lw1 = prow1 * T2R_STR + T2_NT + 8 * (tid & 15);
  const int lw2 = prow2 * T2R_STR + T2_NT + 8 * ((tid + 256) & 15);
  const int nh = wid >> 1, kh = wid & 1;  // wave: dW rows [32 nh, +32) x columns [64 kh, +64)
  f32x4 acc[2][4];
  auto zero_acc = [&]() {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4)(0.f);
  };
  // full tile (wave-uniform, from scalar kernel arguments): every piece of every thread is inside it
  const bool full_tile = NT == T2_NT && (K == 64 || K == MAXW);
  constexpr int64_t PASS = T2_PF * T2_MB;
  // the loads of a full pass of a full tile (the pipelined, branch-free loop takes them). A piece
  // past K (the upper half of a row at K = 64) rereads the slice's first row, as in the general
  // loop; it lands in LDS columns that only the idle waves' fragments would cover
  auto full_loads = [&](int64_t p0, bf16x8 (&ld)[T2_PF][3]) {
    const uint32_t dr = (uint32_t)(p0 - mb);
#pragma unroll
    for (int c = 0; c < T2_PF; ++c) {
      const uint32_t rc = dr + c * T2_MB;
      ld[c][0] = *reinterpret_cast<const bf16x8*>(zb + zo + rc * zstr);
      ld[c][1] = *reinterpret_cast<const bf16x8*>(ab + ao1 + (ok1 ? rc * astr : 0u));
      ld[c][2] = *reinterpret_cast<const bf16x8*>(ab + ao2 + (ok2 ? rc * astr : 0u));
    }
  };
  int64_t p0 = mb;
  if (full_tile && mb + PASS <= me) {  // the first pass is full (at the north star: the only pass)
    bf16x8 ld[T2_PF][3];
    full_loads(p0, ld);
    T2_STAMP(4);  // operand loads issued
    const bool more = mb + PASS < me;
    if (kh * 64 < K) {
      t2r_full_pass<true>(a, more, ld, buf, lw0, lw1, lw2, nh, kh, lane, acc);
    } else {
      zero_acc();
      t2r_full_pass<false>(a, more, ld, buf, lw0, lw1, lw2, nh, kh, lane, acc);
    }
    p0 += PASS;
  } else {
    zero_acc();
  }
  for (; p0 < me; p0 += PASS) {
    bf16x8 ld[T2_PF][3];
    const uint32_t dr = (uint32_t)(p0 - mb);  // rows into the slice
    // every load unconditional (an invalid piece reads the slice's first row and is zeroed after):
    // loads behind branches make the compiler wait for ALL of them (vmcnt(0)) before chunk 0's
    // LDS write; straight-line loads let chunk c wait for its own three only
    bool okc[T2_PF][3];
#pragma unroll
    for (int c = 0; c < T2_PF; ++c) {
      const uint32_t rc = dr + c * T2_MB;
      const int64_t mrow = p0 + c * T2_MB;
      okc[c][0] = ok0 && mrow + prow0 < me;
      okc[c][1] = ok1 && mrow + prow1 < me;
      okc[c][2] = ok2 && mrow + prow2 < me;
      ld[c][0] = *reinterpret_cast<const bf16x8*>(zb + zo + (okc[c][0] ? rc * zstr : 0u));
      ld[c][1] = *reinterpret_cast<const bf16x8*>(ab + ao1 + (okc[c][1] ? rc * astr : 0u));
      ld[c][2] = *reinterpret_cast<const bf16x8*>(ab + ao2 + (okc[c][2] ? rc * astr : 0u));
    }
    if (p0 == mb) T2_STAMP(4);  // operand loads issued
#pragma unroll
    for (int c = 0; c < T2_PF; ++c) {
      if (p0 + c * T2_MB >= me) break;  // uniform: the slice's tail
      __bf16* d = buf + (c & 1) * TR * T2R_STR;
      // pieces outside the tile's features land in LDS columns no fragment of this tile reads
#pragma unroll
      for (int i = 0; i < 3; ++i)
        if (!okc[c][i]) ld[c][i] = (bf16x8)(__bf16)0.f;
      *reinterpret_cast<bf16x8*>(d + lw0) = ld[c][0];
      *reinterpret_cast<bf16x8*>(d + lw1) = ld[c][1];
      *reinterpret_cast<bf16x8*>(d + lw2) = ld[c][2];
      __syncthreads();  // one barrier per chunk: buffer c & 1 was last read two chunks ago
      if (c == 0 && p0 == mb) T2_STAMP(1);
      bf16x8 fa[2], fb[4];
#pragma unroll
      for (int i = 0; i < 2; ++i) fa[i] = t2r_frag(d, nh * 32 + i * 16, lane);
#pragma unroll
      for (int j = 0; j < 4; ++j) fb[j] = t2r_frag(d, T2_NT + kh * 64 + j * 16, lane);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (nh * 32 + i * 16 < NT && kh * 64 + j * 16 < K)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
    }
  }
  T2_STAMP(2);
  float* dst = a.slab + (int64_t)s * a.P + a.woff[t][l];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (nh * 32 + i * 16 < NT && kh * 64 + j * 16 < K)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const int n = n0 + nh * 32 + i * 16 + q * 4 + rr;
          const int k = kh * 64 + j * 16 + r;
          dst[(int64_t)n * K + k] = acc[i][j][rr];
        }
  T2_STAMP(3);
}

__device__ __forceinline__ void wgrad_block(const WgradArgs& a, const WgradTile* __restrict__ tiles, int bid,
                                            char* smem) {
  // workgroups [0, ntiles * S): one (32x32 tile of dW, batch slice) each, its 4 waves on 4
  // consecutive quarters of the slice, reduced through LDS in wave order -> one slab row.
  // Workgroups beyond: one wave per bias output (+ one for the loss).
  float (*red)[64 * 16] = reinterpret_cast<float (*)[64 * 16]>(smem);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int64_t nwg_tiles = (int64_t)a.ntiles * a.S;
  if ((int64_t)bid >= nwg_tiles) {
    T2_STAMP(0);
    // bias gradient of one output n of (t, l): sum of the T1 workgroups' partials, lanes strided
    // over workgroups, then a fixed butterfly -> slab[0]
    int64_t b = ((int64_t)bid - nwg_tiles) * 4 + wid;
    if (b == a.nbias) {  // the scalar loss: T1's per-workgroup partials in a fixed order
      b = -1;            // (no bias output below)
      if (a.loss) {
        float s = 0.f;
        for (int w0 = 0; w0 < a.nwg; w0 += 512) {
          float v[8];
#pragma unroll
          for (int k = 0; k < 8; ++k) v[k] = w0 + k * 64 + lane < a.nwg ? a.loss_part[w0 + k * 64 + lane] : 0.f;
#pragma unroll
          for (int k = 0; k < 8; ++k) s += v[k];
        }
        s = wave_sum(s);
        if (lane == 0) a.loss[0] = s / (float)a.B;
      }
      if (a.adam_pre && lane == 0) {
        const int64_t t_step = a.step_state[0] + 1;
        a.step_state[0] = t_step;
        const double bc1 = 1.0 - pow((double)a.beta1, (double)t_step);
        const double bc2 = 1.0 - pow((double)a.beta2, (double)t_step);
        a.adam_pre[0] = (float)((double)a.lr / bc1);
        a.adam_pre[1] = (float)sqrt(bc2);
      }
    }
    for (int t = 0; t < 2; ++t)
      for (int l = 0; l < a.L; ++l) {
        if (b >= 0 && b < a.width[l]) {
          const float* dbp = a.dbpart + ((int64_t)t * MAXL + l) * a.nwg * MAXW + b;
          // 8 independent loads per lane in flight per round (not one dependent load per add)
          float s = 0.f;
          for (int w0 = 0; w0 < a.nwg; w0 += 512) {
            float v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
              const int w = w0 + k * 64 + lane;
              v[k] = w < a.nwg ? dbp[(int64_t)w * MAXW] : 0.f;
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) s += v[k];
          }
          s = wave_sum(s);
          if (lane == 0) a.slab[a.boff[t][l] + b] = s;
        }
        if (b >= 0) b -= a.width[l];
      }
    T2_STAMP(3);
    return;
  }
  // XCD-aware placement: a contiguous 1/8 of the (slice, tile) list — whole slices, whose tiles
  // re-read the same operand strips — on one XCD and its L2
  const int lb = xcd_remap(bid, (int)nwg_tiles);
  if (a.lds && a.rm) {
    wgrad_lds_block_rm(a, lb, smem);
    return;
  }
  if (a.lds) {
    wgrad_lds_block(a, lb, smem);
    return;
  }
  const int s = (int)(lb / a.ntiles);
  const WgradTile tl = tiles[lb % a.ntiles];
  const int64_t B = a.B;
  const __bf16* Z = a.dzt + ((int64_t)tl.t * MAXL + tl.l) * MAXW * a.Bp;  // strip blocks (strip_at)
  const __bf16* A = tl.l == 0 ? a.xt + (int64_t)tl.t * a.in_max * a.Bp
                              : a.act + ((int64_t)tl.t * MAXL + tl.l - 1) * MAXW * a.Bp;
  const int64_t anf = tl.l == 0 ? a.in_max : MAXW;
  const int64_t mw = a.mslice / 4;
  int64_t mb = (int64_t)s * a.mslice + wid * mw;
  int64_t me = mb + mw;
  if (mb > B) mb = B;
  if (me > B) me = B;
  f32x4 acc[2][2];
  for (int i = 0; i < 2; ++i)
    for (int j = 0; j < 2; ++j) acc[i][j] = (f32x4)(0.f);
  // feature row bases in the tile-major strips; batch row o of a row: + (o / 32) * nf * 32 + o % 32
  const __bf16* z0 = Z + ((int64_t)(tl.n0 + r) << 5);
  const __bf16* z1 = Z + ((int64_t)(tl.n0 + 16 + r) << 5);
  const __bf16* a0 = A + ((int64_t)(tl.k0 + r) << 5);
  const __bf16* a1 = A + ((int64_t)(tl.k0 + 16 + r) << 5);
  auto zo = [&](int64_t o) { return (((o >> 5) * MAXW) << 5) + (o & 31); };
  auto ao = [&](int64_t o) { return (((o >> 5) * anf) << 5) + (o & 31); };
  int64_t m = mb;
  // 4 k-steps per iteration: their 16 fragment loads are issued before the first MFMA
  for (; m + 128 <= me; m += 128) {
    bf16x8 fa0[4], fa1[4], fb0[4], fb1[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t o = m + 32 * u + q * 8;
      fa0[u] = *reinterpret_cast<const bf16x8*>(z0 + zo(o));
      fa1[u] = *reinterpret_cast<const bf16x8*>(z1 + zo(o));
      fb0[u] = *reinterpret_cast<const bf16x8*>(a0 + ao(o));
      fb1[u] = *reinterpret_cast<const bf16x8*>(a1 + ao(o));
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa0[u], fb0[u], acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa0[u], fb1[u], acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa1[u], fb0[u], acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa1[u], fb1[u], acc[1][1], 0, 0, 0);
    }
  }
  for (; m + 32 <= me; m += 32) {
    const int64_t o = m + q * 8;
    const bf16x8 fa0 = *reinterpret_cast<const bf16x8*>(z0 + zo(o));
    const bf16x8 fa1 = *reinterpret_cast<const bf16x8*>(z1 + zo(o));
    const bf16x8 fb0 = *reinterpret_cast<const bf16x8*>(a0 + ao(o));
    const bf16x8 fb1 = *reinterpret_cast<const bf16x8*>(a1 + ao(o));
    acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa0, fb0, acc[0][0], 0, 0, 0);
    acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa0, fb1, acc[0][1], 0, 0, 0);
    acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa1, fb0, acc[1][0], 0, 0, 0);
    acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa1, fb1, acc[1][1], 0, 0, 0);
  }
  if (m < me) {  // ragged tail (B % 32 != 0): zero-padded fragments
    bf16x8 fa0, fa1, fb0, fb1;
    for (int j = 0; j < 8; ++j) {
      const int64_t mm = m + q * 8 + j;
      const bool ok = mm < me;
      fa0[j] = ok ? z0[zo(mm)] : (__bf16)0.f;
      fa1[j] = ok ? z1[zo(mm)] : (__bf16)0.f;
      fb0[j] = ok ? a0[ao(mm)] : (__bf16)0.f;
      fb1[j] = ok ? a1[ao(mm)] : (__bf16)0.f;
    }
    acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa0, fb0, acc[0][0], 0, 0, 0);
    acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa0, fb1, acc[0][1], 0, 0, 0);
    acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa1, fb0, acc[1][0], 0, 0, 0);
    acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa1, fb1, acc[1][1], 0, 0, 0);
  }
  // fixed-order reduction of the 4 waves' tiles: wave 0 adds waves 1, 2, 3 in that order
  if (wid > 0) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) red[wid - 1][((i * 2 + j) * 4 + rr) * 64 + lane] = acc[i][j][rr];
  }
  __syncthreads();
  if (wid > 0) return;
#pragma unroll
  for (int w = 0; w < 3; ++w)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) acc[i][j][rr] += red[w][((i * 2 + j) * 4 + rr) * 64 + lane];
  // C[n][k]: row = n (4q + rr), col = k (r)
  const int K = a.K[tl.t][tl.l];
  float* dst = a.slab + (int64_t)s * a.P + a.woff[tl.t][tl.l];
  for (int i = 0; i < 2; ++i)
    for (int j = 0; j < 2; ++j)
      for (int rr = 0; rr < 4; ++rr) {
        const int n = tl.n0 + i * 16 + q * 4 + rr;
        const int k = tl.k0 + j * 16 + r;
        dst[(int64_t)n * K + k] = acc[i][j][rr];
      }
}

__global__ void __launch_bounds__(256) tower_wgrad_kernel(WgradArgs a, const WgradTile* __restrict__ tiles) {
  __shared__ __attribute__((aligned(16))) char smem[T2_SMEM];
  // resolver workgroups first (their probe chains are the longest dependent work of the launch);
  // n_res % 8 == 0 keeps the tiles' XCD placement
  if ((int)blockIdx.x < a.n_res)
    dd_resolve_block(a.dd, (int)blockIdx.x, a.n_res);
  else
    wgrad_block(a, tiles, (int)blockIdx.x - a.n_res, smem);
}

// T2 + the embedding path's fused row-wise Adagrad (dedup.h) in ONE launch: workgroups
// [0, n_t2) are T2's, the rest run dd_update_block. Both read only what T1 wrote, so one launch
// boundary (and no cross-stream join) separates them from T1, and the MFMA/L2-bound tiles overlap
// the HBM-bound row updates on the same CUs.
__global__ void __launch_bounds__(256) tower_wgrad_dedup_kernel(WgradArgs a, const WgradTile* __restrict__ tiles,
                                                                DdUpdateArgs d, int n_t2) {
  __shared__ __attribute__((aligned(16))) char smem[T2_SMEM];
  if ((int)blockIdx.x < n_t2)
    wgrad_block(a, tiles, (int)blockIdx.x, smem);
  else
    dd_update_block(d, (int)blockIdx.x - n_t2, smem);
}

// Pipelined fused step: T2 with the NEXT batch's dedup insert as extra workgroups (one wave per
// 64 lookups i = t * B + m: one returning CAS each, lookups that lost it deferred to the next
// launch's resolver), so T1 of the next step finds a complete table and updates the rows looked up
// once in place (tower_rows_kernel<UPD = true>).
struct InsertArgs {
  const void* col[2];
  int64_t mod[2];
  int32_t tab[2];
  int id_dtype;
  int64_t B;
  DedupWs dd;
  int xcd_wpt;  // > 0: insert_next_full_block files by T1 tile class (ins_lookup), this many workgroups
                // per (XCD class, tower); 0: 256 consecutive lookups per workgroup
};
// lookup of thread tid in insert workgroup blk (blk < 2B / 256). xcd_wpt > 0 (B % 2048 == 0): the
// workgroup takes only rows of the T1 tiles (32 rows each) that run on its own XCD (blk % 8): T1
// places tiles [c B / 256, (c + 1) B / 256) on XCD c (xcd_remap), so the next batch's ids and the
// claims T1 reads first are in that XCD's L2 when its T1 tile starts (plain loads and stores keep
// their lines there). Lookup order is irrelevant to the results: every row's lookups are summed in
// ascending lookup order whatever their slot positions.
__device__ __forceinline__ int64_t ins_lookup(const InsertArgs& ins, int blk, int tid) {
  if (ins.xcd_wpt <= 0) return (int64_t)blk * 256 + tid;
  const int c = blk & 7, j = blk >> 3;
  const int t = j / ins.xcd_wpt, qi = j - t * ins.xcd_wpt;
  // T1 tile b runs on XCD c for b in [c B / 256, (c + 1) B / 256) (tower_rows_body's xcd_remap)
  const int64_t b = (int64_t)c * (ins.B / 256) + 8 * qi + (tid >> 5);
  return (int64_t)t * ins.B + 32 * b + (tid & 31);
}

__device__ __forceinline__ void insert_next_block(const InsertArgs& ins, int blk) {
  const int lane = threadIdx.x & 63;
  const int64_t grp = (int64_t)blk * 4 + (threadIdx.x >> 6);
  const int64_t i = grp * 64 + lane;
  DdPend p;
  p.key = DD_EMPTY;
  if (i < 2 * ins.B) {
    const int t = i >= ins.B;
    const int64_t m = i - (t ? ins.B : 0);
    const int64_t id = load_id(t ? ins.col[1] : ins.col[0], ins.id_dtype, m);
    const uint64_t key = id != 0 ? (((uint64_t)(t ? ins.tab[1] : ins.tab[0]) << DD_TABLE_SHIFT) |
                                    (uint64_t)py_mod64(id, t ? ins.mod[1] : ins.mod[0]))
                                 : DD_EMPTY;
    dd_insert_begin(ins.dd, key, (int32_t)i, p);
  }
  if (grp < ins.dd.ovf_groups) dd_insert_defer_finish(ins.dd, p, (int32_t)(i < 2 * ins.B ? i : 0), (int)grp);
}

// EXPERIMENT (TT_RING_STAMPS): s_memrealtime of wave 0 at the start / end of each workgroup's role
#if TT_EXPERIMENTS
#define RING_STAMP(p, k) \
  do { if ((p) && threadIdx.x == 0 && blockIdx.x < 2048) (p)[(int64_t)blockIdx.x * 2 + (k)] = (int64_t)__builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define RING_STAMP(p, k) do { (void)(p); } while (0)
#endif

__global__ void __launch_bounds__(256) tower_wgrad_insert_kernel(WgradArgs a, const WgradTile* __restrict__ tiles,
                                                                 InsertArgs ins, int n_t2, int64_t* stamps) {
  __shared__ __attribute__((aligned(16))) char smem[T2_SMEM];
  RING_STAMP(stamps, 0);
  if ((int)blockIdx.x < n_t2)
    wgrad_block(a, tiles, (int)blockIdx.x, smem);
  else
    insert_next_block(ins, (int)blockIdx.x - n_t2);
  RING_STAMP(stamps, 1);
}

// Pipelined sharded step, launch U (after exchange A brought the gradient rows of batch i and the
// ids of batch i+1): T2 of batch i (weight-gradient tiles, bias sums, loss) beside the owner's
// row-wise Adagrad of batch i's rows and the count pass of batch i+2's route — all three read only
// what T1 and the exchange wrote, so the tower weight gradients overlap the embedding update.
// n_dd > 0: the owner's update workgroups come FIRST in the grid (they carry the launch's longest
// chain, claim -> slot -> rows -> stores; dispatched behind the T2 tiles, the last of them started
// ~4.5 us late), then the T2 tiles, then the route count
__global__ void __launch_bounds__(256, 3) tower_wgrad_route_rowwise_kernel(WgradArgs a, const WgradTile* __restrict__ tiles,
                                                                        RouteArgs r, DdUpdateArgs d, int n_t2,
                                                                        int n_cnt, int n_dd, PxWait w) {
  __shared__ __attribute__((aligned(16))) char smem[T2_SMEM];
  int b = (int)blockIdx.x;
  if (w.W) {
    // in-launch exchange A: workgroup 0 signals; it and the owner's update workgroups (the only
    // readers of the received blocks) wait — workgroup 0 always, so a rank with no update
    // workgroups still holds launch G back until every peer consumed its exchange-B buffer
    if (b == 0) px_signal(w);
    if (b == 0 || (n_dd > 0 ? b < n_dd : b >= n_t2 + n_cnt)) px_wait(w);
  }
  if (n_dd > 0) {
    if (b < n_dd) {
      dd_update_block(d, b, smem);
      return;
    }
    b -= n_dd;
    if (b >= n_t2 + n_cnt) return;
  }
  if (b < n_t2) {
    wgrad_block(a, tiles, b, smem);
  } else if (b < n_t2 + n_cnt) {
    const int j = b - n_t2;
    route_count_block(r, j % r.nblk, j / r.nblk, reinterpret_cast<int (*)[RT_MAXW]>(smem));
  } else {
    dd_update_block(d, b - n_t2 - n_cnt, smem);
  }
}

// REMAP: the parameter blocks a contiguous 1/8 per XCD (xcd_remap of workgroup b of nblocks)
template <bool REMAP = false>
__device__ __forceinline__ void update_block(const UpdateArgs& a, int b, int nblocks) {
  // The entry batch: every scalar in front of the first slab load (UpdateArgs' line 0, the wait
  // flag, the launch dimensions), one group of scalar loads with one wait. The empty asm pins them
  // in SGPRs and, as its outputs, keeps every use below it: a use scheduled between two of the
  // loads costs a wait of its own (scalar loads return out of order, so any wait is for all), and
  // left alone the compiler sinks each load into the branch that uses it, a serial round trip each.
  const float* params = a.params;
  const float* exp_avg = a.exp_avg;
  const float* exp_avg_sq = a.exp_avg_sq;
  const float* slab = a.slab;
  const float* adam_pre = a.adam_pre;
  const float* grads_in = a.grads_in;
  const float* grads_out = a.grads_out;
  int64_t P = a.P;
  int S = a.S, do_adam = a.do_adam, nseg = a.nseg, wt_w = a.wt.W;
  asm volatile(""
               : "+s"(P), "+s"(S), "+s"(do_adam), "+s"(nseg), "+s"(wt_w), "+s"(nblocks)
               : "s"(slab), "s"(adam_pre), "s"(grads_in), "s"(params), "s"(exp_avg), "s"(exp_avg_sq), "s"(grads_out));
  const int bid = REMAP ? xcd_remap(b, nblocks) : b;
  T3_STAMP(0);
  if (wt_w) {
    if (bid == 0) px_signal(a.wt);
    px_wait(a.wt);
  }
  const int64_t i = (int64_t)bid * T3_BLOCK + threadIdx.x;
  int64_t t_step = 0;
  float step_size = 0.f, bc2_sqrt = 1.f;
  // (T2's precomputed Adam scalars are loaded below, behind the slab loads: in front of them the
  // slab loads would wait out that load's latency first)
  const bool pre = do_adam && adam_pre;
  if (do_adam && !pre) {
    t_step = a.step_state[0] + 1;
    const double bc1 = 1.0 - pow((double)a.beta1, (double)t_step);
    const double bc2 = 1.0 - pow((double)a.beta2, (double)t_step);
    step_size = (float)((double)a.lr / bc1);
    bc2_sqrt = (float)sqrt(bc2);
  }
  if (i < P) {
    // a round's 32 slab loads all in flight (one memory latency per 32 slabs, not per load); the
    // sum keeps the sequential order s = 0, 1, ... A round is one basic block: the loads past S - 1
    // read slab S - 1 again (the same cache line) and their values are not added, where a branch
    // per load would end the block and put a wait for every earlier load at the join.
    float sv[32];
    const auto slab_issue = [&](int s0) {
#pragma unroll
      for (int u = 0; u < 32; ++u)  // S P < 2^31: a scalar base per slab, the lane's offset shared by all
        sv[u] = (slab + (uint32_t)(s0 + u < S ? s0 + u : S - 1) * (uint32_t)P)[(uint32_t)i];
    };
    const auto slab_sum = [&](int s0, float g) {
#pragma unroll
      for (int u = 0; u < 32; ++u) g = s0 + u < S ? g + sv[u] : g;
      return g;
    };
    // the moments' addresses without a branch (no Adam: the parameter again, value unused)
    const float* const mp = do_adam ? exp_avg : params;
    const float* const vp = do_adam ? exp_avg_sq : params;
    // and Adam's scalars' (no precomputed pair: the first two parameters, values unused)
    const float* const sp = pre ? adam_pre : params;
    float g = 0.f, p, m, v, pre0, pre1;
    const auto state_issue = [&]() { p = params[i], m = mp[i], v = vp[i], pre0 = sp[0], pre1 = sp[1]; };
    T3Seg sg;
    if (!grads_in && (do_adam || grads_out)) {
      // The first round's loads wait for nothing but the entry batch. A bias element (its gradient
      // is slab 0's alone, reduced over the T1 workgroups by T2's bias waves) issues the same loads
      // and keeps the first, so which segment a lane is in is not needed yet: the segment table's
      // scalar loads and the select run while the slab, parameter and moment loads are in flight.
      slab_issue(0);
      state_issue();
      sg = t3_seg(a, i, nseg);
      // (the select stands in front of the sum: the first addend passes through the asm with it)
      asm volatile("" : "+v"(sv[0]) : "v"(sg.soff), "v"(sg.swc), "v"(sg.sisw), "v"(sg.sk), "v"(sg.sn), "v"(sg.st_), "v"(sg.sl_));
      const float gb = sv[0];
      g = slab_sum(0, g);
      for (int s0 = 32; s0 < S; s0 += 32) {
        slab_issue(s0);
        g = slab_sum(s0, g);
      }
      g = sg.sisw ? g : gb;
    } else {
      if (grads_in) {
        g = grads_in[i];
        for (int q = 1; q < a.in_srcs; ++q) g += grads_in[(int64_t)q * a.in_stride + i];
      }
      state_issue();
      sg = t3_seg(a, i, nseg);
    }
    if (!do_adam) m = 0.f, v = 0.f;
    if (pre) step_size = pre0, bc2_sqrt = pre1;
    T3_STAMP(1);
    t3_apply(a, i, sg, p, m, v, g, step_size, bc2_sqrt, do_adam);
    T3_STAMP(2);
  }
  if (do_adam && !pre) {
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned* counter = reinterpret_cast<unsigned*>(a.step_state + 1);
      const unsigned prev = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (prev == (unsigned)nblocks - 1) {
        __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(reinterpret_cast<unsigned long long*>(a.step_state), (unsigned long long)t_step,
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
}

// the parameter blocks a contiguous 1/8 per XCD (xcd_remap; every parameter's update is independent
// of its workgroup): -0.45 us a step at the north star against blockIdx order, same box
// (profiles/r06y2_ab_t3_by_xcd.log)
__global__ void __launch_bounds__(256) tower_update_kernel(UpdateArgs a) {
  update_block<true>(a, (int)blockIdx.x, (int)gridDim.x);
}

// Pipelined sharded step, launch G (after launch U updated this rank's rows): the owner's gather of
// batch i+1's rows (bf16, into exchange B's row blocks, filing batch i+1's dedup table), the tower
// gradient of batch i x 1/W into exchange B's tower block of every destination (slab reduction, no
// Adam), and the place pass of batch i+2's route.
__global__ void __launch_bounds__(256) tower_grads_place_gather_kernel(UpdateArgs a, RouteArgs r, GatherSegArgs g,
                                                                       int n_upd, int n_place) {
  __shared__ int base[RT_MAXW];
  __shared__ int wc[RT_BLOCK / 64][RT_MAXW];
  const int b = (int)blockIdx.x;
  if (g.epoch && b == 0 && threadIdx.x == 0)  // exchange B's epoch advances with its producer
    __hip_atomic_fetch_add(g.epoch, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (b < n_upd) {
    update_block<true>(a, b, n_upd);  // a contiguous 1/8 per XCD, as T3
  } else if (b < n_upd + n_place) {
    const int j = b - n_upd;
    route_place_block<true>(r, j % r.nblk, j / r.nblk, base, wc);
  } else {
    shard_gather_block(g, b - n_upd - n_place);
  }
}

// K3 of the pipelined fused step: resolver workgroups for the NEXT batch's deferred inserts, then
// the update of this batch's rows looked up more than once (skip_single), then T3
constexpr int K3_RES_WGS = 32;
__global__ void __launch_bounds__(256) tower_update_dedup_resolve_kernel(UpdateArgs a, DdUpdateArgs d, DedupWs next,
                                                                         int n_dd, int64_t* stamps) {
  __shared__ __attribute__((aligned(16))) char smem[DD_SMEM];
  const int bid = (int)blockIdx.x;
  RING_STAMP(stamps, 0);
  if (bid < K3_RES_WGS)
    dd_resolve_block(next, bid, K3_RES_WGS);
  else if (bid < K3_RES_WGS + n_dd)
    dd_update_block(d, bid - K3_RES_WGS, smem);
  else
    update_block(a, bid - K3_RES_WGS - n_dd, (int)gridDim.x - K3_RES_WGS - n_dd);
  RING_STAMP(stamps, 1);
}

// The pipelined fused step's backward tail, one launch: T2 (weight gradients, bias sums, loss,
// Adam scalars) + the NEXT batch's complete insert (probing in place: its latency hides behind the
// tiles, so no deferral and no resolver launch) + the update of this batch's rows looked up more
// than once. The three roles read only what T1 (or the previous step) wrote; T3 follows as its own
// launch (it needs every T2 slab: in-launch, that hand-off across the 8 XCDs' L2s cost more than
// the launch boundary it saves — DESIGN.md section 5).
// the NEXT batch's lookups, INS_PT per thread, inserted completely (probing in place). The
// workgroup's repeated keys are merged in LDS first: one leader per key claims or joins the key's
// slot with the group's count in ONE global atomic and hands each member its position (base +
// rank in the group) — at skewed ids a hot row costs one atomic per workgroup, not one per lookup
// (the update sums a row's lookups in lookup order whatever the positions: the same results).
#ifndef TT_INS_PT
#define TT_INS_PT 1
#endif
constexpr int INS_PT = TT_INS_PT;  // lookups per thread (1: 256 per workgroup, 64 workgroups at the
                                   // north star; 2 measured 0.3-0.4 µs slower per step, scripts/r04_inspt.sh)
constexpr int INS_HS = 1024;  // LDS hash slots per 512 lookups
static_assert(INS_HS * (8 + 3 * 4) <= T2_SMEM, "the insert role's LDS hash fits the tail's LDS");
__device__ __forceinline__ void insert_next_full_block(const InsertArgs& ins, int blk, char* smem) {
  unsigned long long* hk = reinterpret_cast<unsigned long long*>(smem);  // [INS_HS] keys
  int* hc = reinterpret_cast<int*>(smem + 8 * INS_HS);                   // [INS_HS] group counts
  int* hb = hc + INS_HS;                                                 // [INS_HS] group base position
  int* hg = hb + INS_HS;                                                 // [INS_HS] global slot
  const DedupWs& ws = ins.dd;
  for (int q = threadIdx.x; q < INS_HS; q += 256) {
    hk[q] = DD_EMPTY;
    hc[q] = 0;
  }
  int64_t iv[INS_PT];
  uint64_t key[INS_PT];
#pragma unroll
  for (int u = 0; u < INS_PT; ++u) {
    const int64_t i = INS_PT == 1 ? ins_lookup(ins, blk, (int)threadIdx.x)
                                  : ((int64_t)blk * INS_PT + u) * 256 + threadIdx.x;
    iv[u] = i;
    key[u] = DD_EMPTY;
    if (i < 2 * ins.B) {
      const int t = i >= ins.B;
      const int64_t m = i - (t ? ins.B : 0);
      const int64_t id = load_id(t ? ins.col[1] : ins.col[0], ins.id_dtype, m);
      if (id != 0)
        key[u] = ((uint64_t)(t ? ins.tab[1] : ins.tab[0]) << DD_TABLE_SHIFT) |
                 (uint64_t)py_mod64(id, t ? ins.mod[1] : ins.mod[0]);
      ws.lkey[i] = key[u];
    }
  }
  __syncthreads();
  int hl[INS_PT], rank[INS_PT];
#pragma unroll
  for (int u = 0; u < INS_PT; ++u) {
    hl[u] = -1;
    rank[u] = 0;
    if (key[u] != DD_EMPTY) {
      unsigned h = (unsigned)dd_mix64(key[u]) & (INS_HS - 1);
      while (true) {
        const unsigned long long prev = atomicCAS(&hk[h], (unsigned long long)DD_EMPTY, (unsigned long long)key[u]);
        if (prev == DD_EMPTY || prev == key[u]) break;
        h = (h + 1) & (INS_HS - 1);
      }
      hl[u] = (int)h;
      rank[u] = atomicAdd(&hc[h], 1);
    }
  }
  __syncthreads();
  // each group's leader: one claiming CAS (with the group's count) or one add of it
  const uint64_t mask = (uint64_t)ws.cap - 1;
#pragma unroll
  for (int u = 0; u < INS_PT; ++u) {
    if (hl[u] >= 0 && rank[u] == 0) {
      const uint64_t c = (uint64_t)hc[hl[u]];
      uint64_t g = dd_mix64(key[u]) & mask;
      int base;
      while (true) {
        unsigned long long* w = reinterpret_cast<unsigned long long*>(&ws.slots[g].word);
        const unsigned long long prev =
            atomicCAS(w, (unsigned long long)DD_EMPTY, (unsigned long long)((key[u] << DD_CNT_BITS) | c));
        if (prev == DD_EMPTY) {
          base = 0;
          break;
        }
        if ((prev >> DD_CNT_BITS) == key[u]) {
          base = (int)(atomicAdd(w, (unsigned long long)c) & DD_CNT_MASK);
          break;
        }
        g = (g + 1) & mask;
      }
      hb[hl[u]] = base;
      hg[hl[u]] = (int)g;
    }
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < INS_PT; ++u) {
    const int64_t i = iv[u];
    if (i >= 2 * ins.B) continue;
    if (hl[u] < 0) {
      ws.claim[i] = -1;
      continue;
    }
    const int k = hb[hl[u]] + rank[u], h = hg[hl[u]];
    ws.claim[i] = k == 0 ? h : -1;
    if (k < DD_INL) {
      ws.slots[h].item[k] = (int32_t)i;
    } else if (k == DD_INL) {
      const int q = atomicAdd(&ws.ctr[0], 1);
      if (q < ws.hot_cap) {
        ws.hot[q] = h;
        ws.hkey[q] = key[u];
      }
    }
  }
}

template <bool LIST>
__global__ void __launch_bounds__(256, 3) tower_tail_kernel(WgradArgs a2, const WgradTile* __restrict__ tiles,
                                                         InsertArgs ins, DdUpdateArgs d, int n_ins, int n_t2,
                                                         int64_t* stamps) {
  __shared__ __attribute__((aligned(16))) char smem[T2_SMEM];
  int b = (int)blockIdx.x;
  RING_STAMP(stamps, 0);
  if (b < n_ins)
    insert_next_full_block(ins, b, smem);
  else if ((b -= n_ins) < n_t2)
    wgrad_block(a2, tiles, b, smem);  // n_ins % 8 == 0: b keeps the XCD placement of wgrad_block
  else
    dd_update_block<LIST>(d, b - n_t2, smem);
  RING_STAMP(stamps, 1);
}

// T3 + the embedding path's fused row-wise Adagrad (dedup.h) in ONE launch: workgroups [0, n_dd)
// run dd_update_block (its slot workgroups fit one round of resident waves), the rest T3 (Adam with
// T2's precomputed scalars). T2 runs alone before it with the registers and LDS it needs.
__global__ void __launch_bounds__(256) tower_update_dedup_kernel(UpdateArgs a, DdUpdateArgs d, int n_dd) {
  __shared__ __attribute__((aligned(16))) char smem[DD_SMEM];
  if ((int)blockIdx.x < n_dd)
    dd_update_block(d, (int)blockIdx.x, smem);
  else
    update_block(a, (int)blockIdx.x - n_dd, (int)gridDim.x - n_dd);
}

// the NEXT batch's insert role (WGRAD | INSERT, and the ring tail WGRAD | INSERT | ADAGRAD): its checks
// and arguments; the dedup workspace holds both towers' B lookups
static int insert_args(const tt_insert_role_t& in, int64_t B, const char* what, InsertArgs& ins) {
  const std::string w(what);
  if (!in.next_cols || !in.num_embeddings || !in.dedup_tables || !in.next_dedup_ws)
    return fail(TT_EINVAL, w + ": null pointer");
  if (in.id_dtype != TT_I32 && in.id_dtype != TT_I64) return fail(TT_EINVAL, w + ": ids must be int32/int64");
  if (int rc = check_dedup_ws(in.next_dedup_ws, in.dedup_ws_bytes, in.dedup_max_lookups, 2 * B, what, true)) return rc;
  for (int t = 0; t < 2; ++t) {
    if (!in.next_cols[t] || in.num_embeddings[t] < 1 || in.num_embeddings[t] >= (1ll << DD_TABLE_SHIFT) ||
        in.dedup_tables[t] < 0 || in.dedup_tables[t] >= TT_MAX_TABLES)
      return fail(TT_EINVAL, "tower insert: bad column / table");
    ins.col[t] = in.next_cols[t];
    ins.mod[t] = in.num_embeddings[t];
    ins.tab[t] = in.dedup_tables[t];
  }
  ins.id_dtype = in.id_dtype;
  ins.B = B;
  // tile-class filing (ins_lookup): 2B / 256 workgroups, B / 2048 of them per (class, tower)
  ins.xcd_wpt = (INS_PT == 1 && B % 2048 == 0) ? (int)(B / 2048) : 0;
  dedup_layout(in.next_dedup_ws, in.dedup_max_lookups, &ins.dd);
  return TT_OK;
}

// T2 arguments from the shape + workspace + WGRAD role (shared by every launch that runs T2); hands
// back the layout it computed and *wgs = T2's workgroup count
static int wgrad_args(const tt_tower_shape_t* shape, int64_t B, void* workspace, size_t ws_bytes,
                      const tt_wgrad_role_t& w, WgradArgs& a, int64_t* wgs, TowerLayout& L) {
  int rc = tower_ws_layout(shape, B, workspace, ws_bytes, &L);
  if (rc) return rc;
  char* ws = reinterpret_cast<char*>(workspace);
  a.xt = reinterpret_cast<const __bf16*>(ws + L.o_xt);
  a.act = reinterpret_cast<const __bf16*>(ws + L.o_act);
  a.dzt = reinterpret_cast<const __bf16*>(ws + L.o_dzt);
  a.slab = reinterpret_cast<float*>(ws + L.o_slab);
  a.P = L.P;
  a.B = B;
  a.in_max = L.in_max;
  a.Bp = L.Bp;
  a.S = L.S;
  a.mslice = L.mslice;
  a.ntiles = L.ntiles;
  for (int t = 0; t < 2; ++t)
    for (int l = 0; l < MAXL; ++l) {
      a.woff[t][l] = L.woff[t][l];
      a.boff[t][l] = L.boff[t][l];
      a.K[t][l] = L.K[t][l];
    }
  int nbias = 0;
  for (int l = 0; l < shape->L; ++l) {
    a.width[l] = shape->width[l];
    nbias += 2 * shape->width[l];
  }
  a.L = shape->L;
  a.dbpart = reinterpret_cast<const float*>(ws + L.o_dbpart);
  a.nwg = L.nwg;
  a.loss_part = reinterpret_cast<const float*>(ws + L.o_losspart);
  a.loss = w.loss;
  a.nbias = nbias;
  a.tiles_off = (int64_t)L.o_tiles;
#if TT_EXPERIMENTS
  if (getenv("TT_T2_STAMPS")) a.stamps = reinterpret_cast<int64_t*>(ws + L.o_dbg);
#endif
  a.lds = L.lds;
  a.rm = L.rows;
  for (int i = 0; i < 16; ++i) {
    a.t2_code[i] = L.t2_code[i];
  }
  if (w.adam_step_state) {  // the loss wave advances Adam's step and writes its scalars for T3
    a.step_state = w.adam_step_state;
    a.adam_pre = reinterpret_cast<float*>(ws + L.o_counter);
    a.lr = w.adam_lr;
    a.beta1 = w.adam_beta1;
    a.beta2 = w.adam_beta2;
  }
  *wgs = (int64_t)L.ntiles * L.S + ceil_div(nbias + 1, 4);
  return TT_OK;
}

// the tile list of the register-path T2 in the workspace (tt_tower_workspace_init uploaded it)
static const WgradTile* wgrad_tiles(void* workspace, const WgradArgs& a) {
  return reinterpret_cast<const WgradTile*>(reinterpret_cast<char*>(workspace) + a.tiles_off);
}

int fused_wgrad_adagrad(const tt_launch_plan_t& p, void* stream) {
  WgradArgs a{};
  int64_t wgs = 0;
  TowerLayout L;
  int rc = wgrad_args(p.shape, p.B, p.workspace, p.ws_bytes, p.wgrad, a, &wgs, L);
  if (rc) return rc;
  DdUpdateArgs d{};
  int64_t dd_grid = 0;
  if ((rc = dedup_update_args(p.adagrad, d, &dd_grid))) return rc;
  if (wgs + dd_grid > INT32_MAX) return fail(TT_EINVAL, "tower_wgrad_rowwise_adagrad: grid too large");
  tower_wgrad_dedup_kernel<<<dim3((unsigned)(wgs + dd_grid)), dim3(256), 0, as_stream(stream)>>>(
      a, wgrad_tiles(p.workspace, a), d, (int)wgs);
  return check_launch("tower_wgrad_rowwise_adagrad");
}

// what a T3 launch takes beside its UPDATE role (named at each call site; declaration order)
struct T3Opts {
  int64_t* step_state = nullptr;     // Adam's step counter, advanced by T3 itself (tt_adam_step's) ...
  float lr = 0.f;                    // ... and its learning rate
  int do_adam = 0;
  const float* grads_in = nullptr;   // the gradient to apply instead of T2's partials: in_srcs blocks,
  int in_srcs = 1;                   // in_stride floats apart, summed in ascending order
  int64_t in_stride = 0;
  bool adam_pre = false;             // Adam's step scalars are in the workspace (a WGRAD role wrote them)
  const DdUpdateArgs* dd = nullptr;  // the row-wise Adagrad update's workgroups in front (UPDATE | ADAGRAD)
  int64_t dd_grid = 0;
  const tt_peer_wait_t* wait = nullptr;
};

// the replicated form's output (UPDATE.replicated = 1): checked by its two launches before anything else
static int replicated_check(const tt_update_role_t& u) {
  if (!u.base || !u.offsets || u.copies < 1 || u.copies > 16) return fail(TT_EINVAL, "tower_grads_replicated: bad output");
  return TT_OK;
}

// T3 arguments (shared by every T3 launch form); hands back the layout, *grid = T3's workgroup count
static int t3_args(const tt_tower_shape_t* shape, int64_t B, void* workspace, size_t ws_bytes,
                   const tt_update_role_t& u, const T3Opts& o, UpdateArgs& a, int64_t* grid, TowerLayout& L) {
  int rc = tower_ws_layout(shape, B, workspace, ws_bytes, &L);
  if (rc) return rc;
  const bool rep = u.replicated != 0;  // no Adam: the gradient x scale to base + offsets[q]
  if (!u.params || (o.do_adam && (!u.exp_avg || !u.exp_avg_sq || (!o.step_state && !o.adam_pre))))
    return fail(TT_EINVAL, "tower: null pointer");
  if (rep && u.copies > 16) return fail(TT_EINVAL, "tower: at most 16 gradient copies");
  char* ws = reinterpret_cast<char*>(workspace);
  a = UpdateArgs{};
  a.params = u.params;
  a.exp_avg = rep ? nullptr : u.exp_avg;
  a.exp_avg_sq = rep ? nullptr : u.exp_avg_sq;
  a.slab = reinterpret_cast<const float*>(ws + L.o_slab);
  a.dbpart = reinterpret_cast<const float*>(ws + L.o_dbpart);
  a.P = (int32_t)L.P;
  a.S = L.S;
  a.nwg = L.nwg;
  // the segment records' fields and update_block's 32-bit slab offsets (the shape limits keep far below)
  if ((int64_t)L.S * L.P >= INT32_MAX / 4 || L.PW >= INT32_MAX)
    return fail(TT_EINVAL, "tower: parameter vector too long for the segment table");
  int sg = 0;
  const auto rec = [&](int64_t off, int64_t wc, int n, int k, int isw, int t, int l) {
    a.seg[sg++] = t3_u32x4{(uint32_t)off, (uint32_t)wc, (uint32_t)n | (uint32_t)k << 16,
                           (uint32_t)isw | (uint32_t)t << 1 | (uint32_t)l << 2};
  };
  for (int t = 0; t < 2; ++t)
    for (int l = 0; l < shape->L; ++l) {
      rec(L.woff[t][l], L.wcoff[t][l], shape->width[l], L.K[t][l], 1, t, l);
      rec(L.boff[t][l], 0, shape->width[l], 1, 0, t, l);
    }
  a.nseg = sg;
  while (sg < T3_NSEG) rec(INT32_MAX, 0, 1, 1, 0, 0, 0);  // never selected
  a.wb = reinterpret_cast<__bf16*>(ws + L.o_wb);
  a.wtb = reinterpret_cast<__bf16*>(ws + L.o_wtb);
  a.wbf = reinterpret_cast<__bf16*>(ws + L.o_wbf);
  a.wtbf = reinterpret_cast<__bf16*>(ws + L.o_wtbf);
  a.wimg = L.rows ? ws + L.o_wimg : nullptr;
  // the plain [out][in] / [in][out] bf16 copies are read only by tower_fwd_bwd_kernel, which
  // launch_t1 uses for shapes other than two layers over inputs <= 128 wide
  a.skip_plain = shape->L == 2 && shape->in_dim[0] <= 128 && shape->in_dim[1] <= 128 &&
                 !(shape->flags & TT_TOWER_GENERAL_T1);
  a.lr = o.lr;
  // (the replicated form reads none of Adam's constants: fixed values, whatever the role holds)
  a.beta1 = rep ? 0.9f : u.beta1; a.beta2 = rep ? 0.999f : u.beta2; a.eps = rep ? 1e-8f : u.eps;
  a.wd = rep ? 0.f : u.weight_decay;
  a.step_state = o.step_state;
  a.do_adam = o.do_adam;
  a.grads_out = rep ? u.base : u.grads_out;
  a.grads_in = o.grads_in;
  a.adam_pre = o.adam_pre ? reinterpret_cast<const float*>(ws + L.o_counter) : nullptr;
  // one copy takes the multi-copy path too (scale applied): give it two identical copies
  a.out_copies = !rep ? 1 : u.copies == 1 ? 2 : u.copies;
  for (int q = 0; rep && u.offsets && q < a.out_copies; ++q) a.out_off[q] = u.offsets[q < u.copies ? q : 0];
  a.out_scale = rep ? u.scale : 1.f;
  a.in_srcs = o.in_srcs;
  a.in_stride = o.in_stride;
  *grid = ceil_div(L.P, 256);
  return TT_OK;
}

static int launch_t3(const tt_tower_shape_t* shape, int64_t B, void* workspace, size_t ws_bytes,
                     const tt_update_role_t& u, const T3Opts& o, void* stream) {
  UpdateArgs a;
  int64_t g3 = 0;
  TowerLayout L;
  int rc = t3_args(shape, B, workspace, ws_bytes, u, o, a, &g3, L);
  if (rc) return rc;
  if ((rc = peer_wait_args(o.wait, a.wt, "tower_update"))) return rc;
  if (o.dd) {
    if (o.dd_grid + g3 > INT32_MAX) return fail(TT_EINVAL, "tower_update_rowwise_adagrad: grid too large");
    tower_update_dedup_kernel<<<dim3((unsigned)(o.dd_grid + g3)), dim3(256), 0, as_stream(stream)>>>(a, *o.dd,
                                                                                                      (int)o.dd_grid);
    return check_launch("tower_update_rowwise_adagrad");
  }
#if TT_EXPERIMENTS
  if (getenv("TT_RING_STAMPS"))  // workgroups [0, 512) stamp
    a.stamps = reinterpret_cast<int64_t*>(reinterpret_cast<char*>(workspace) + L.o_dbg) + 6144;
#endif
  int bs = 256;
#if TT_EXPERIMENTS
  if (const char* e = getenv("TT_T3_BLOCK")) bs = atoi(e) == 128 ? 128 : 256;  // EXPERIMENT
#endif
  tower_update_kernel<<<dim3((unsigned)ceil_div(a.P, (int64_t)bs)), dim3(bs), 0, as_stream(stream)>>>(a);
  return check_launch("tower_update");
}

// the Adam form of the UPDATE role from an export's arguments
static tt_update_role_t adam_role(float* params, float* exp_avg, float* exp_avg_sq, float eps, float beta1,
                                  float beta2, float weight_decay, float* grads_out) {
  tt_update_role_t u{};
  u.params = params, u.exp_avg = exp_avg, u.exp_avg_sq = exp_avg_sq;
  u.eps = eps, u.beta1 = beta1, u.beta2 = beta2, u.weight_decay = weight_decay, u.grads_out = grads_out;
  return u;
}

int fused_update_adagrad(const tt_launch_plan_t& p, void* stream) {
  // the towers' checks come before the ADAGRAD role's (launch_t3 repeats them, at no cost that matters)
  TowerLayout L;
  int rc = tower_ws_layout(p.shape, p.B, p.workspace, p.ws_bytes, &L);
  if (rc) return rc;
  DdUpdateArgs d{};
  int64_t dd_grid = 0;
  if ((rc = dedup_update_args(p.adagrad, d, &dd_grid))) return rc;
  return launch_t3(p.shape, p.B, p.workspace, p.ws_bytes, p.update,
                   {.do_adam = 1, .adam_pre = true, .dd = &d, .dd_grid = dd_grid}, stream);
}

// the next batch's route of the fused launches (as tt_shard_route_segs; never an empty batch)
static int fused_route_args(const tt_launch_plan_t& p, RouteArgs& r) {
  if (p.B < 1) return fail(TT_EINVAL, "route: bad batch / segment capacity");
  return route_args(p.route, p.B, RT_SEGS, "route", r);
}

int fused_wgrad_route_count_adagrad(const tt_launch_plan_t& p, void* stream) {
  if (!p.wgrad.adam_step_state) return fail(TT_EINVAL, "tower_wgrad_route_rowwise: null Adam step state");
  PxWait pw;
  if (int rc = peer_wait_args(p.wait, pw, "tower_wgrad_route_rowwise")) return rc;
  WgradArgs a{};
  int64_t wgs = 0;
  TowerLayout L;
  int rc = wgrad_args(p.shape, p.B, p.workspace, p.ws_bytes, p.wgrad, a, &wgs, L);
  if (rc) return rc;
  RouteArgs r{};
  if ((rc = fused_route_args(p, r))) return rc;
  DdUpdateArgs d{};
  int64_t dd_grid = 0;
  if ((rc = dedup_update_args(p.adagrad, d, &dd_grid))) return rc;
  const int64_t n_cnt = (int64_t)r.nblk * r.F;
  if (wgs + n_cnt + dd_grid > INT32_MAX) return fail(TT_EINVAL, "tower_wgrad_route_rowwise: grid too large");
  d.xcd = d.hot_wgs % 8 == 0 ? 1 : 0;  // the owner's update workgroups first (dd_first): slot role aligned
#if TT_EXPERIMENTS
  static const bool dd_first = !getenv("TT_U_DD_FIRST") || atoi(getenv("TT_U_DD_FIRST")) != 0;  // A/B switch
#else
  constexpr bool dd_first = true;
#endif
  tower_wgrad_route_rowwise_kernel<<<dim3((unsigned)(wgs + n_cnt + dd_grid)), dim3(256), 0, as_stream(stream)>>>(
      a, wgrad_tiles(p.workspace, a), r, d, (int)wgs, (int)n_cnt, dd_first ? (int)dd_grid : 0, pw);
  return check_launch("tower_wgrad_route_count_rowwise_adagrad");
}

int fused_route_count_adagrad(const tt_launch_plan_t& p, void* stream) {
  PxWait pw;
  if (int rc = peer_wait_args(p.wait, pw, "shard_route_count_rowwise_adagrad")) return rc;
  // launch U of the pipelined sharded step without its T2 tiles (those run on a parallel branch of
  // the step graph, beside exchange A): the owner's update workgroups first, then the route count
  RouteArgs r{};
  int rc = fused_route_args(p, r);
  if (rc) return rc;
  DdUpdateArgs d{};
  int64_t dd_grid = 0;
  if ((rc = dedup_update_args(p.adagrad, d, &dd_grid))) return rc;
  const int64_t n_cnt = (int64_t)r.nblk * r.F;
  if (n_cnt + dd_grid > INT32_MAX) return fail(TT_EINVAL, "shard_route_count_rowwise_adagrad: grid too large");
  d.xcd = d.hot_wgs % 8 == 0 ? 1 : 0;  // the owner's update workgroups first: slot role aligned
  WgradArgs a{};
  tower_wgrad_route_rowwise_kernel<<<dim3((unsigned)(n_cnt + dd_grid)), dim3(256), 0, as_stream(stream)>>>(
      a, nullptr, r, d, 0, (int)n_cnt, (int)dd_grid, pw);
  return check_launch("shard_route_count_rowwise_adagrad");
}

int fused_grads_route_place_gather(const tt_launch_plan_t& p, void* stream) {
  if (!p.update.params) return fail(TT_EINVAL, "tower_grads_replicated: bad output");
  int rc = replicated_check(p.update);
  if (rc) return rc;
  RouteArgs r{};
  if ((rc = fused_route_args(p, r))) return rc;
  GatherSegArgs g{};
  if ((rc = gather_segs_args(p.gather, r.F, r.W, g))) return rc;
  UpdateArgs a;
  int64_t g3 = 0;
  TowerLayout L;
  if ((rc = t3_args(p.shape, p.B, p.workspace, p.ws_bytes, p.update, {}, a, &g3, L))) return rc;
  const int64_t n_place = (int64_t)r.nblk * r.F, n_gather = ceil_div(ceil_div((int64_t)r.W * g.S, GS_SL), 8);
  if (g3 + n_place + n_gather > INT32_MAX) return fail(TT_EINVAL, "tower_grads_place_gather: grid too large");
  tower_grads_place_gather_kernel<<<dim3((unsigned)(g3 + n_place + n_gather)), dim3(256), 0, as_stream(stream)>>>(
      a, r, g, (int)g3, (int)n_place);
  return check_launch("tower_grads_replicated_route_place_gather");
}

int fused_wgrad_insert(const tt_launch_plan_t& p, void* stream) {
  if (!p.wgrad.adam_step_state) return fail(TT_EINVAL, "tower_wgrad_pre_insert: null pointer");
  InsertArgs ins{};
  int rc = insert_args(p.insert, p.B, "tower_wgrad_pre_insert", ins);
  if (rc) return rc;
  WgradArgs a{};
  int64_t wgs = 0;
  TowerLayout L;
  if ((rc = wgrad_args(p.shape, p.B, p.workspace, p.ws_bytes, p.wgrad, a, &wgs, L))) return rc;
  const int64_t n_ins = ceil_div(ceil_div(2 * p.B, 64), 4);  // 4 waves of 64 lookups per workgroup
  int64_t* stamps = TT_EXPERIMENTS && getenv("TT_RING_STAMPS") ? reinterpret_cast<int64_t*>(reinterpret_cast<char*>(p.workspace) + L.o_dbg) + 4096 : nullptr;
  tower_wgrad_insert_kernel<<<dim3((unsigned)(wgs + n_ins)), dim3(256), 0, as_stream(stream)>>>(
      a, wgrad_tiles(p.workspace, a), ins, (int)wgs, stamps);
  return check_launch("tower_wgrad_pre_insert");
}

int fused_update_adagrad_resolve(const tt_launch_plan_t& p, void* stream) {
  void* next_dedup_ws = p.resolve.dedup_ws;  // bytes / max lookups: the ADAGRAD role's
  if (!next_dedup_ws || (reinterpret_cast<uintptr_t>(next_dedup_ws) & 63))
    return fail(TT_EINVAL, "tower_update_resolve: next dedup workspace null / misaligned");
  DdUpdateArgs d{};
  int64_t dd_grid = 0;
  int rc = dedup_update_args(p.adagrad, d, &dd_grid);
  if (rc) return rc;
  d.skip_single = 1;
  DedupWs next;
  dedup_layout(next_dedup_ws, p.adagrad.dedup_max_lookups, &next);
  UpdateArgs a;
  int64_t g3 = 0;
  TowerLayout L;
  if ((rc = t3_args(p.shape, p.B, p.workspace, p.ws_bytes, p.update, {.do_adam = 1, .adam_pre = true}, a, &g3, L)))
    return rc;
  int64_t* stamps = TT_EXPERIMENTS && getenv("TT_RING_STAMPS") ? reinterpret_cast<int64_t*>(reinterpret_cast<char*>(p.workspace) + L.o_dbg) + 6144 : nullptr;
  if (stamps && (K3_RES_WGS + dd_grid + g3 > 1024 || L.nwg > 256)) stamps = nullptr;
  tower_update_dedup_resolve_kernel<<<dim3((unsigned)(K3_RES_WGS + dd_grid + g3)), dim3(256), 0,
                                      as_stream(stream)>>>(a, d, next, (int)dd_grid, stamps);
  return check_launch("tower_update_pre_rowwise_adagrad_resolve");
}

int fused_wgrad_insert_adagrad(const tt_launch_plan_t& p, void* stream) {
  if (!p.wgrad.adam_step_state) return fail(TT_EINVAL, "tower_tail: null pointer");
  const int64_t B = p.B;
  tt_adagrad_role_t g = p.adagrad;
  g.B = B;  // the ring tail's lookups per feature are the plan's B (tt_launch: adagrad.B is 0 or B)
  tt_insert_role_t in = p.insert;
  in.dedup_ws_bytes = g.dedup_ws_bytes, in.dedup_max_lookups = g.dedup_max_lookups;  // one size: the ADAGRAD role's
  InsertArgs ins{};
  int rc = insert_args(in, B, "tower_tail", ins);
  if (rc) return rc;
  WgradArgs a2{};
  int64_t wgs = 0;
  TowerLayout L;
  if ((rc = wgrad_args(p.shape, B, p.workspace, p.ws_bytes, p.wgrad, a2, &wgs, L))) return rc;
  char* ws = reinterpret_cast<char*>(p.workspace);
  DdUpdateArgs d{};
  int64_t dd_grid = 0;
  if ((rc = dedup_update_args(g, d, &dd_grid))) return rc;
  d.skip_single = 1;
  bool list = L.rows && L.lds;  // the row-owned T1 listed the multi-lookup rows and freed the single slots
#if TT_EXPERIMENTS
  if (const char* e = getenv("TT_MULTI_LIST")) list = list && e[0] != '0';  // EXPERIMENT: A/B
  if (const char* e = getenv("TT_EXP_SKIP")) d.exp_skip = atoi(e);
#endif
  // the list role scans at most 2048 segments (B <= 16384); past that the slot role walks every
  // claiming lookup (T1 still freed the single slots: their words read EMPTY there)
  list = list && L.nwg * 4 <= std::min<int64_t>(d.ws.nseg, 2048);
  if (list) {
    d.multi_nseg = (int)(L.nwg * 4);
    // a workgroup's share of the listed slots <= 256 (at most lookups / 2 slots are listed)
    int64_t nlb = std::max<int64_t>(8, ceil_div(2 * B, 512) * 4);
#if TT_EXPERIMENTS
    if (const char* e = getenv("TT_LIST_WGS")) nlb = std::max(nlb, (int64_t)atoi(e));  // EXPERIMENT
#endif
    d.slot_hw = nlb * 8;
    dd_grid = d.hot_wgs + nlb;
  }
  const int64_t n_ins = ceil_div(ceil_div(2 * B, 256 * INS_PT), 8) * 8;  // INS_PT lookups per thread; % 8 == 0
  int64_t* stamps = TT_EXPERIMENTS && getenv("TT_RING_STAMPS") ? reinterpret_cast<int64_t*>(ws + L.o_dbg) + 4096 : nullptr;
  if (stamps && L.nwg > 256) stamps = nullptr;
  // the list role (the ring) in a kernel of its own code: no slot-role instructions in its footprint
  auto kern = list ? tower_tail_kernel<true> : tower_tail_kernel<false>;
  kern<<<dim3((unsigned)(n_ins + wgs + dd_grid)), dim3(256), 0, as_stream(stream)>>>(
      a2, wgrad_tiles(p.workspace, a2), ins, d, (int)n_ins, (int)wgs, stamps);
  return check_launch("tower_wgrad_pre_insert_rowwise_adagrad");
}

}  // namespace tt

using namespace tt;

extern "C" {

int tt_tower_wgrad(const tt_tower_shape_t* shape, int64_t B, float* loss, void* workspace, size_t ws_bytes,
                   void* stream) {
  tt_wgrad_role_t w{};
  w.loss = loss;
  WgradArgs a{};
  int64_t wgs = 0;
  TowerLayout L;
  int rc = wgrad_args(shape, B, workspace, ws_bytes, w, a, &wgs, L);
  if (rc) return rc;
  tower_wgrad_kernel<<<dim3((unsigned)wgs), dim3(256), 0, as_stream(stream)>>>(a, wgrad_tiles(workspace, a));
  return check_launch("tower_wgrad");
}

int tt_tower_wgrad_pre(const tt_tower_shape_t* shape, int64_t B, float* loss, void* workspace, size_t ws_bytes,
                       int64_t* adam_step_state, float adam_lr, float adam_beta1, float adam_beta2, void* dedup_ws,
                       size_t dedup_ws_bytes, int64_t dedup_max_lookups, void* stream) {
  if (!adam_step_state) return fail(TT_EINVAL, "tower_wgrad_pre: null Adam step state");
  const tt_wgrad_role_t w{loss, adam_step_state, adam_lr, adam_beta1, adam_beta2};
  WgradArgs a{};
  int64_t wgs = 0;
  TowerLayout L;
  int rc = wgrad_args(shape, B, workspace, ws_bytes, w, a, &wgs, L);
  if (rc) return rc;
  if (dedup_ws) {
    if ((rc = check_dedup_ws(dedup_ws, dedup_ws_bytes, dedup_max_lookups, 1, "tower_wgrad_pre", true))) return rc;
    dedup_layout(dedup_ws, dedup_max_lookups, &a.dd);
    a.n_res = 64;
    wgs += a.n_res;
  }
  tower_wgrad_kernel<<<dim3((unsigned)wgs), dim3(256), 0, as_stream(stream)>>>(a, wgrad_tiles(workspace, a));
  return check_launch("tower_wgrad_pre");
}

int tt_tower_update(const tt_tower_shape_t* shape, int64_t B, float* params, float* exp_avg, float* exp_avg_sq,
                    float lr, float beta1, float beta2, float eps, float weight_decay, int64_t* step_state,
                    int do_adam, float* grads_out, void* workspace, size_t ws_bytes, void* stream) {
  return launch_t3(shape, B, workspace, ws_bytes,
                   adam_role(params, exp_avg, exp_avg_sq, eps, beta1, beta2, weight_decay, grads_out),
                   {.step_state = step_state, .lr = lr, .do_adam = do_adam}, stream);
}

int tt_tower_update_pre(const tt_tower_shape_t* shape, int64_t B, float* params, float* exp_avg, float* exp_avg_sq,
                        float eps, float beta1, float beta2, float weight_decay, float* grads_out, void* workspace,
                        size_t ws_bytes, void* stream) {
  return launch_t3(shape, B, workspace, ws_bytes,
                   adam_role(params, exp_avg, exp_avg_sq, eps, beta1, beta2, weight_decay, grads_out),
                   {.do_adam = 1, .adam_pre = true}, stream);
}

int tt_tower_adam_grads(const tt_tower_shape_t* shape, int64_t B, float* params, const float* grads,
                        float* exp_avg, float* exp_avg_sq, float lr, float beta1, float beta2, float eps,
                        float weight_decay, int64_t* step_state, void* workspace, size_t ws_bytes, void* stream) {
  if (!grads) return fail(TT_EINVAL, "tower_adam_grads: null gradient");
  return launch_t3(shape, B, workspace, ws_bytes,
                   adam_role(params, exp_avg, exp_avg_sq, eps, beta1, beta2, weight_decay, nullptr),
                   {.step_state = step_state, .lr = lr, .do_adam = 1, .grads_in = grads}, stream);
}

int tt_tower_grads_replicated(const tt_tower_shape_t* shape, int64_t B, float* params, float* base, int copies,
                              const int64_t* offsets, float scale, void* workspace, size_t ws_bytes, void* stream) {
  tt_update_role_t u{};
  u.params = params, u.replicated = 1, u.copies = copies, u.base = base, u.offsets = offsets, u.scale = scale;
  if (int rc = replicated_check(u)) return rc;
  for (int q = 0; q < copies; ++q)
    if (offsets[q] < 0) return fail(TT_EINVAL, "tower_grads_replicated: negative offset");
  return launch_t3(shape, B, workspace, ws_bytes, u, {}, stream);
}

int tt_tower_adam_pre_grads_sum(const tt_tower_shape_t* shape, int64_t B, float* params, const float* grads, int nsrc,
                                int64_t src_stride, float* exp_avg, float* exp_avg_sq, float eps, float beta1,
                                float beta2, float weight_decay, void* workspace, size_t ws_bytes,
                                const tt_peer_wait_t* wait, void* stream) {
  TowerLayout L;
  int rc = tower_ws_layout(shape, B, workspace, ws_bytes, &L);
  if (rc) return rc;
  if (!grads || nsrc < 1 || (nsrc > 1 && src_stride < L.P)) return fail(TT_EINVAL, "tower_adam_pre_grads_sum: bad gradient");
  if (wait && wait->W != nsrc) return fail(TT_EINVAL, "tower_adam_pre_grads_sum: wait.W must be nsrc");
  return launch_t3(shape, B, workspace, ws_bytes,
                   adam_role(params, exp_avg, exp_avg_sq, eps, beta1, beta2, weight_decay, nullptr),
                   {.do_adam = 1, .grads_in = grads, .in_srcs = nsrc, .in_stride = src_stride, .adam_pre = true,
                    .wait = wait},
                   stream);
}

}  // extern "C"
