// What the units of the fused tower step share (tower.hip: the stages, the workspace layout, the T1
// exports and tt_launch; tower_t1.hip: the general and the two-layer T1; tower_rows.hip: the
// row-owned T1; tower_tail.hip: T2, the insert role, T3 and their launches): the tile constants, the
// T1 kernel arguments, the weight-image layout that T3 writes and the row-owned T1 reads, the
// workspace layout, and the host functions one unit calls in another.
#pragma once

#include "tt_common.h"
#include "dedup.h"
#include "shard.h"

namespace tt {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;

constexpr int TR = 32;                // rows per workgroup
constexpr int MAXW = 128;             // max layer width
constexpr int XCH = 128;              // input columns per chunk
constexpr int LSTR = MAXW + 8;        // bf16 LDS row stride (272 B: conflict-light ds_read_b128)
constexpr int FSTR = MAXW + 4;        // fp32 LDS row stride
constexpr int MAXL = 4;

// T1 -> T2 operand strips (X^T, activations, dZ^T; bf16), tile-major: element (feature f, batch
// row m) of a strip block with nf features sits at ((m / 32) * nf + f) * 32 + m % 32, blocks of
// nf x Bp elements (Bp = B rounded up to 32). One T1 workgroup's 32-row tile of a block is one
// contiguous run (whole cache lines written once), and a T2 chunk of 32 rows x 16 features is 1 KB
// contiguous (a full-rate load per wave instruction) instead of 16 scattered 64-B pieces.
__device__ __forceinline__ int64_t strip_at(int64_t f, int64_t m, int64_t nf) {
  return (((m >> 5) * nf + f) << 5) + (m & 31);
}

// The row-owned T1's argument front (tower_rows_body), built by launch_t1_rows (rk_front): what its
// compute waves read, laid out by WHEN they read it, so that each phase's scalar loads are one batch
// of whole 64-B lines of the kernel-argument segment with one wait (as UpdateArgs for T3). A wave
// reads the common record and its tower's record, selected by one wave-uniform offset: everything
// per tower (pointers advanced to the tower's block, offsets folded in) is precomputed on the host.
struct alignas(64) RkTower {
  // line 0, the entry batch: all that the id, claim, bias and row-DMA addresses need
  const void* idcol;       // gcol[t]; IDX: gpos[t]
  const void* tab;         // gtab[t]; IDX: gsrc[t]; POOL: pooled + in_col[t]
  int64_t gmod;
  const float* b0;         // params + boff[t][0]
  const float* b1;         // params + boff[t][1]
  const int32_t* claim;    // UPD: dd.claim + t B
  const int32_t* pos_out;  // IDX: gpos_out[t], null: the input row's index
  int64_t rstride;         // POOL: floats between source rows (ldp)
  // line 1: the strips and the row's state (the late batch, behind the row DMAs), the dZ strips
  // and the gradient rows (the update batch, in front of the dZ0 product)
  __bf16* xt;              // xt + t in_max Bp
  __bf16* act0;            // act + (t MAXL + 0) MAXW Bp
  float* us;               // UPD: us[t]
  __bf16* dzt0;            // dzt + (t MAXL + 0) MAXW Bp
  __bf16* dzt1;            // dzt + (t MAXL + 1) MAXW Bp
  float* grow;             // gpooled + in_col[t]; IDX: gdst[t]
  float* prow;             // pooled_out + in_col[t], null without pooled_out
  int64_t pad1_;
  // line 2: the table rows (update batch: it brings the line in), the bias partials (epilogue)
  float* uw;               // UPD: uw[t]
  float* db0;              // dbpart + (t MAXL + 0) nwg MAXW
  float* db1;              // dbpart + (t MAXL + 1) nwg MAXW
  int64_t pad2_[5];
};
struct alignas(64) RkCommon {
  // line 0: entry (B .. gid_dtype), the late batch (the rest)
  int64_t B;
  const void* labels;
  int32_t label_dtype;
  int32_t gid_dtype;
  float grad_scale;
  int32_t in_max;
  DSlot* slots;            // UPD: dd.slots
  int32_t* ctr;            // UPD: dd.ctr
  float ulr, ueps;
  int32_t nwg;             // the grid (the tile's XCD placement needs it at entry)
  float fB;                // (float)B, for the late batch: B itself need not live up to the logit
  // line 1: the update batch and the epilogue
  int64_t ldp;
  int32_t* multi;          // UPD: dd.multi
  float* logits;
  float* loss_part;
  int32_t nseg;            // UPD: dd.nseg
  int32_t pad1_[7];
};
struct RkFront {
  RkCommon c;
  RkTower tw[2];
};
static_assert(sizeof(RkTower) == 192 && sizeof(RkCommon) == 128, "whole 64-B lines");

struct alignas(64) TowerArgs {
  RkFront rk;  // first: 64-B aligned in the kernel-argument segment
  tt_tower_shape_t s;
  int64_t B;
  const float* pooled;  // [B, ldp]
  int64_t ldp;
  float* gpooled;       // [B, ldp] (tower-input columns written)
  const float* params;  // flat fp32 (bias read from here)
  const __bf16* wb;     // bf16 W  [out][in] per (t,l), flat like params' W blocks
  const __bf16* wtb;    // bf16 W^T [in][out]
  const __bf16* wbf;    // the same two copies in MFMA B-fragment order (frag_off): every fragment
  const __bf16* wtbf;   //   load of a wave is 1 KB contiguous (full 128-B lines, one request each)
  int64_t woff[2][MAXL];  // element offset of W_(t,l) in params
  int64_t boff[2][MAXL];  // element offset of b_(t,l) in params
  int64_t wcoff[2][MAXL]; // element offset of W_(t,l) in the bf16 copies
  const void* labels;
  int label_dtype;
  float grad_scale;
  float* logits;
  // T1 -> T2 buffers
  __bf16* xt;           // [2] blocks of in_max x Bp (strip_at)
  __bf16* act;          // [2][MAXL][MAXW][B]  (layer-l OUTPUT, transposed; layers 0..L-2 used)
  __bf16* dzt;          // [2][MAXL][MAXW][B]
  float* dbpart;        // [2][MAXL][nwg][MAXW]
  float* loss_part;     // [nwg]
  int64_t in_max;
  int64_t Bp;           // strip rows per block (B rounded up to 32)
  int nwg;
  // fused single-hot gather (tt_tower_fwd_bwd_gather): tower t's input row m is table row
  // (gcol[t][m] mod gmod[t]) of gtab[t] (zeros for id 0) instead of pooled row m
  const void* gcol[2];
  const float* gtab[2];
  int64_t gmod[2];
  int gid_dtype;
  float* pooled_out;    // nullable: the gathered rows are also written here (ld = ldp)
  // dedup insert of the gathered lookups (lookup i = t * B + m, key = dd_table[t] << 40 | row)
  DedupWs dd;
  int dd_on;
  int dd_table[2];
  // indexed gather (sharded step, tt_tower_fwd_bwd_indexed): tower t's input row m is row
  // gpos[t][m] of gsrc[t] ([*][in_dim[t]] fp32; -1 -> zeros) and its dX row goes to row gpos[t][m]
  // of gdst[t] instead of gpooled
  const int32_t* gpos[2];
  const float* gsrc[2];  // fp32 rows, or bf16 rows when gsrc_bf16 (the same bf16 values T1 computes on)
  float* gdst[2];
  const int32_t* gpos_out[2];  // nullable: dX row index in gdst (units of in_dim floats) when it differs
                               // from the input row (the pipelined sharded step's packed send buffer)
  int gsrc_bf16;
  // in-place row-wise Adagrad of the rows looked up ONCE in the step (the pipelined fused step,
  // tower_rows_kernel<UPD = true>): `dd` is this batch's dedup table, completed before T1 (by the
  // previous step's T2 / K3); a kept lookup whose slot count is 1 updates its row and state here from
  // its dX (the same arithmetic as the K3 update: rw_* helpers); the others leave dX for K3
  float* uw[2];  // tower t's table rows (writable; == gtab[t])
  float* us[2];  // tower t's table row-wise state
  float ulr, ueps;
  const void* reserved_[2];  // unused (once the classic T1's next-batch id columns): keeps the later kernarg offsets
  // multi-hot EBC forward fused in (tt_tower_fwd_bwd_kjt, tower_l2_kernel<..., MH = true>): tower
  // t's input row m is the SUM of rows values[moff[t][m] .. moff[t][m + 1]) of gtab[t] (gmod[t]
  // rows: an id >= gmod[t] reads row 0, never out of bounds)
  const void* mval;
  const int32_t* moff[2];
  // multi-feature indexed rows (sharded step with several single-hot features per tower,
  // tt_tower_fwd_bwd_indexed_multi_bf16; the general kernel): input column k of tower t is column
  // k % iD of bf16 row ipos[(ifeat0[t] + k / iD) * B + m] of isrc (-1 -> zeros), and dX column k
  // goes to column k % iD of row ipos_out[same] of idst (-1: not written)
  const int32_t* ipos;
  const int32_t* ipos_out;
  const __bf16* isrc;
  float* idst;
  int ifeat0[2];
  int iD;
  // the row-owned T1 (tower_rows_kernel): both towers' bf16 weight image, the LDS layout (rk_off)
  const char* wimg;
  // indexed2 with a direct exchange (W > 0): dX rows go to the destinations' mapped receive buffers
  // (px_row) and the copy fields' bytes travel beside them (px_copy_*); W = 0: gdst as above
  tt_peer_direct_t xd;
#if TT_EXPERIMENTS
  int dbg;  // EXPERIMENT: 1 skip T2 operand stores, 2 skip dX stores, 4 gather row 0 only, 8 stamps
  int64_t* stamps;  // EXPERIMENT: [nwg][16] s_memrealtime per phase (thread 0)
#endif
};
#if TT_EXPERIMENTS
#define TDBG(bit) ((a.dbg & (bit)) != 0)
#else
#define TDBG(bit) false
#endif
// EXPERIMENT (TT_T1_DEBUG bit 64 with 8): lane 0 of every wave at its arrival at barrier k (1..7),
// at its start (0) and its end (8): [nwg][16][9] after the 8192 stamps of the other launches
#if TT_EXPERIMENTS
#define T1_WSTAMP(k) \
  do { if (a.stamps && (a.dbg & 64) && lane == 0) a.stamps[8192 + ((int64_t)blockIdx.x * 16 + (k)) * 9 + wid] = (int64_t)__builtin_amdgcn_s_memrealtime(); } while (0)
#define T1_STAMP(k) \
  do { if (a.stamps && threadIdx.x == 0) a.stamps[(int64_t)blockIdx.x * 16 + (k)] = (int64_t)__builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define T1_WSTAMP(k) do { } while (0)
#define T1_STAMP(k) do { } while (0)
#endif

__device__ __forceinline__ float lbl(const void* p, int dt, int64_t i) {
  if (dt == TT_I32) return (float)reinterpret_cast<const int32_t*>(p)[i];
  if (dt == TT_I64) return (float)reinterpret_cast<const int64_t*>(p)[i];
  return reinterpret_cast<const float*>(p)[i];
}

// B-fragment order of a [N][K] matrix (K % 32 == 0): the 16 x 32 fragment (n-tile nt, k-step s) is
// 64 lanes x 8 contiguous elements, lane q * 16 + r holding row nt * 16 + r, columns s * 32 + q * 8 ..
__host__ __device__ __forceinline__ int64_t frag_off(int n, int k, int K) {
  return ((int64_t)((n >> 4) * (K >> 5) + (k >> 5)) * 64 + ((k & 31) >> 3) * 16 + (n & 15)) * 8 + (k & 7);
}

// lane value from another lane of its 16-lane row by DPP (no LDS round trip: ds_bpermute is one)
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), CTRL, 0xF, 0xF, true));
}

typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;

// the row-owned T1's shape and its bf16 weight image (tower_rows.hip reads it, T3's t3_apply writes it)
constexpr int RK_IN = 128, RK_W0 = 128, RK_W1 = 64;
constexpr int RK_IMG_T = (RK_W0 + RK_W1) * 256;  // bytes per tower: W0 [128][128], then W1 [64][128]
constexpr int RK_IMG = 2 * RK_IMG_T;             // 98,304 B
// 16-B chunk swizzle of image row `row` (256-B rows): b128 reads of 16 permuted rows x one chunk
// and transposed reads of 8 rows x 4 chunks (two 16-lane groups) hit distinct banks
__host__ __device__ __forceinline__ int rk_swz(int row) {
  return (row & 3) | (((row & 1) | (((row >> 3) & 1) << 1)) << 2);
}
__host__ __device__ __forceinline__ int rk_off(int row, int col) {  // byte offset of bf16 element (row, col)
  return row * 256 + (((col >> 3) ^ rk_swz(row)) << 4) + ((col & 7) << 1);
}

// staged T2 (wgrad_lds_block): a workgroup owns T2_NT rows x all K columns of one dW over a batch
// slice. The slice is read in passes of T2_PF chunks of T2_MB rows; ALL loads of a pass are issued
// up front (T2_PF x 3 x 16 B per thread in flight: one memory latency per pass, not one per chunk),
// then each chunk (T2_NT rows of dZ^T + K rows of A^T, bf16) goes through LDS (double-buffered, one
// barrier per chunk) where the 4 waves share it
constexpr int T2_NT = 64;
constexpr int T2_MB = 32;                              // batch rows per staged chunk (one k-step)
constexpr int T2_PF = 8;                               // chunks per pass (256 rows)
// a tile of the register-path T2's list in the workspace (tt_tower_workspace_init uploads it)
struct WgradTile {
  int32_t t, l, n0, k0;
};

// the parameter vector, T2's tiling and the workspace carve of a shape and batch (tower.hip)
struct TowerLayout {
  int64_t P;         // dense params
  int64_t PW;        // weight elements (bf16 copies)
  int64_t woff[2][MAXL], boff[2][MAXL], wcoff[2][MAXL];
  int32_t K[2][MAXL];
  int64_t in_max;
  int64_t Bp;        // strip rows per block (B rounded up to 32)
  int nwg;
  int S;
  int64_t mslice;
  int ntiles;
  int lds;  // staged T2 (wgrad_lds_block)
  int32_t t2_code[16];
  int rows;  // the row-owned T1 (tower_rows_kernel) serves this shape's single-hot gather launches
  // workspace carve (bytes)
  size_t o_xt, o_act, o_dzt, o_dbpart, o_slab, o_losspart, o_counter, o_wb, o_wtb, o_wbf, o_wtbf, o_wimg, o_tiles, o_dbg, total;
};

// what every T1 export hands on as it got it: the towers' parameters, the labels, the outputs
struct T1Common {
  const float* params;
  const void* labels;
  int label_dtype;
  float grad_scale;
  float* logits;
  void* workspace;
  size_t ws_bytes;
  void* stream;
};

// host functions that one unit defines and another calls: internal to the library
#pragma GCC visibility push(hidden)
// tower.hip
int tower_layout(const tt_tower_shape_t* s, int64_t B, TowerLayout* lay);
int tower_ws_layout(const tt_tower_shape_t* s, int64_t B, const void* workspace, size_t ws_bytes, TowerLayout* lay);
// tower_t1.hip, tower_rows.hip: the launch of a TowerArgs that launch_t1 (tower.hip) checked and filled
int launch_t1_classic(const TowerArgs& a, void* stream);
int launch_t1_rows(TowerArgs& a, void* stream);
// tower_tail.hip: the fused launches behind tt_launch (tower.hip)
int fused_wgrad_adagrad(const tt_launch_plan_t& p, void* stream);
int fused_update_adagrad(const tt_launch_plan_t& p, void* stream);
int fused_wgrad_route_count_adagrad(const tt_launch_plan_t& p, void* stream);
int fused_route_count_adagrad(const tt_launch_plan_t& p, void* stream);
int fused_grads_route_place_gather(const tt_launch_plan_t& p, void* stream);
int fused_wgrad_insert(const tt_launch_plan_t& p, void* stream);
int fused_update_adagrad_resolve(const tt_launch_plan_t& p, void* stream);
int fused_wgrad_insert_adagrad(const tt_launch_plan_t& p, void* stream);
#pragma GCC visibility pop

}  // namespace tt
