// Fused two-tower MLP step on gfx950 bf16 MFMA (v_mfma_f32_16x16x32_bf16, fp32 accumulate).
//
// Replaces ~9 per-layer launches of the towers (torchrec MLP = Linear + ReLU on every layer,
// 03_model_training.py:411-412), the dot + BCE head (:452-453) and Adam (:826-829) with three:
//
//  T1 tower_fwd_bwd   one 256-thread workgroup per 32 rows: both towers' forward through all layers
//                     (activations stay in LDS), logits + BCE + dlogit, the backward through all
//                     layers down to dX, written straight into the pooled-embedding gradient
//                     [B, sum D] that the fused row-wise Adagrad consumes. It also stores, for T2,
//                     the layer inputs and the dZ of every layer TRANSPOSED ([feature][row], bf16),
//                     and per-workgroup bias-gradient partials (fp32).
//  T2 tower_wgrad     dW = dZ^T A over all rows: one wave per (32x32 tile, row slice), fragments
//                     loaded straight from the transposed bf16 buffers (16 B per lane, no LDS),
//                     partial tiles into fp32 slabs.
//  T3 tower_update    per parameter: fixed-order sum of the slabs / bias partials, Adam
//                     (torch.optim.Adam formula), and the bf16 weight copies T1 reads next step
//                     (W [out][in] for the forward, W^T [in][out] for the backward).
// Every reduction is in a fixed order: bitwise reproducible, independent of XCD placement.
//
// MFMA 16x16x32 operand maps (lane l, element j < 8): A[l&15][8(l>>4)+j], B[8(l>>4)+j][l&15];
// result C[4(l>>4)+r][l&15], r < 4.
//
// This file: the workspace layout, the T1 entry points (launch_t1: checks, arguments, the choice of
// kernel family) and tt_launch. The kernels and their launches: tower_t1.hip (the general and the
// two-layer T1), tower_rows.hip (the row-owned T1), tower_tail.hip (T2, the insert role, T3); what
// they share: tower_common.h.
#include <vector>

#include "tower_common.h"

namespace tt {

int tower_layout(const tt_tower_shape_t* s, int64_t B, TowerLayout* lay) {
  if (!s) return fail(TT_EINVAL, "tower: null shape");
  if (s->L < 1 || s->L > MAXL) return fail(TT_EINVAL, "tower: 1..4 layers supported");
  if (B < 8 || B % 8) return fail(TT_EINVAL, "tower: B must be a positive multiple of 8");
  if (s->flags & ~TT_TOWER_GENERAL_T1) return fail(TT_EINVAL, "tower: unknown shape flags");
  for (int l = 0; l < s->L; ++l)
    if (s->width[l] < 16 || s->width[l] > MAXW || s->width[l] % 32)
      return fail(TT_EINVAL, "tower: layer widths must be multiples of 32 in [32, 128]");
  for (int t = 0; t < 2; ++t) {
    if (s->in_dim[t] < 32 || s->in_dim[t] > 1024 || s->in_dim[t] % 32)
      return fail(TT_EINVAL, "tower: input widths must be multiples of 32 in [32, 1024]");
    if (s->in_col[t] < 0 || s->in_col[t] % 4) return fail(TT_EINVAL, "tower: input column must be >= 0, % 4 == 0");
  }
  TowerLayout L{};
  int64_t o = 0, w = 0;
  for (int t = 0; t < 2; ++t) {
    int k = s->in_dim[t];
    for (int l = 0; l < s->L; ++l) {
      L.woff[t][l] = o;
      L.wcoff[t][l] = w;
      L.K[t][l] = k;
      o += (int64_t)s->width[l] * k;
      w += (int64_t)s->width[l] * k;
      L.boff[t][l] = o;
      o += s->width[l];
      k = s->width[l];
    }
  }
  L.P = o;
  L.PW = w;
  L.in_max = std::max(s->in_dim[0], s->in_dim[1]);
  L.nwg = (int)ceil_div(B, TR);
  int nt = 0;
  L.lds = L.in_max <= MAXW;
  if (L.lds) {
    // staged T2: tiles of 64 dW rows x all K
    for (int t = 0; t < 2; ++t)
      for (int l = 0; l < s->L; ++l)
        for (int n0 = 0; n0 < s->width[l]; n0 += T2_NT) {
          L.t2_code[nt] = t | l << 4 | n0 << 8;
          ++nt;
        }
    // slices of whole passes (256 rows), at most 64 (the slab depth T3 reduces over)
    const int64_t pass = T2_PF * T2_MB;
    int64_t passes = 1;  // per slice
#if TT_EXPERIMENTS
    if (const char* e = getenv("TT_T2_SLICE_PASSES")) passes = std::max(1, atoi(e));  // EXPERIMENT
#endif
    const int64_t S = std::min<int64_t>(64, ceil_div(B, pass * passes));
    L.mslice = ceil_div(ceil_div(B, S), pass) * pass;
    L.S = (int)ceil_div(B, L.mslice);
  } else {
    for (int t = 0; t < 2; ++t)
      for (int l = 0; l < s->L; ++l) nt += (s->width[l] / 32) * (L.K[t][l] / 32);
    // slices (one T2 workgroup each per tile, 4 waves of mslice/4 rows): aim for ~400 workgroups,
    // >= 512 rows per slice; the slice count is also the slab depth T3 reduces over
    int64_t S = std::max<int64_t>(1, 400 / std::max(1, nt));
    S = std::min<int64_t>(S, std::max<int64_t>(1, ceil_div(B, 512)));
    S = std::min<int64_t>(S, 64);
    L.S = (int)S;
    L.mslice = ceil_div(ceil_div(B, S), 128) * 128;
  }
  L.ntiles = nt;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    size_t r = off;
    off += align_up(bytes, 256);
    return r;
  };
  L.Bp = ceil_div(B, 32) * 32;
  L.o_xt = take(2 * (size_t)L.in_max * L.Bp * 2);
  L.o_act = take(2 * (size_t)MAXL * MAXW * L.Bp * 2);
  L.o_dzt = take(2 * (size_t)MAXL * MAXW * L.Bp * 2);
  L.o_dbpart = take(2 * (size_t)MAXL * L.nwg * MAXW * 4);
  L.o_slab = take((size_t)L.S * L.P * 4);
  L.o_losspart = take((size_t)L.nwg * 4);
  L.o_counter = take(64);
  L.o_wb = take((size_t)L.PW * 2);
  L.o_wtb = take((size_t)L.PW * 2);
  L.o_wbf = take((size_t)L.PW * 2);
  L.o_wtbf = take((size_t)L.PW * 2);
  L.rows = s->L == 2 && s->in_dim[0] == s->in_dim[1] && (s->in_dim[0] == RK_IN || s->in_dim[0] == 64) &&
           s->width[0] == RK_W0 && s->width[1] == RK_W1 && !(s->flags & TT_TOWER_GENERAL_T1);
  L.o_wimg = take(L.rows ? (size_t)RK_IMG : 0);
  L.o_tiles = take((size_t)nt * sizeof(WgradTile));
  L.o_dbg = take((size_t)(std::max<int64_t>(L.nwg * 2, 1024) * 8 + L.nwg * 16 * 9) * sizeof(int64_t));
  L.total = off;
  *lay = L;
  return TT_OK;
}

// the layout of a caller's workspace: the shape checks, then the workspace's size
int tower_ws_layout(const tt_tower_shape_t* s, int64_t B, const void* workspace, size_t ws_bytes,
                    TowerLayout* lay) {
  int rc = tower_layout(s, B, lay);
  if (rc) return rc;
  if (!workspace || ws_bytes < lay->total) return fail(TT_ECAPACITY, "tower: workspace too small");
  return TT_OK;
}

// shared by every T1 export: checks, T1 arguments, launch
static int launch_t1(const tt_tower_shape_t* shape, int64_t B, TowerArgs& a, const float* pooled, int64_t ldp,
                     float* gpooled, const T1Common& c) {
  const float* params = c.params;
  const void* labels = c.labels;
  const int label_dtype = c.label_dtype;
  const float grad_scale = c.grad_scale;
  float* logits = c.logits;
  void* workspace = c.workspace;
  const size_t ws_bytes = c.ws_bytes;
  void* stream = c.stream;
  TowerLayout L;
  int rc = tower_ws_layout(shape, B, workspace, ws_bytes, &L);
  if (rc) return rc;
  if ((!pooled && !a.gcol[0] && !a.gpos[0] && !a.mval && !a.ipos) || (!gpooled && !a.gpos[0] && !a.ipos) || !params ||
      !labels || !logits)
    return fail(TT_EINVAL, "tower: null pointer");
  if (label_dtype != TT_I32 && label_dtype != TT_I64 && label_dtype != TT_F32)
    return fail(TT_EINVAL, "tower: labels must be int32/int64/float32");
  if (ldp % 4 || (reinterpret_cast<uintptr_t>(pooled) & 15) || (reinterpret_cast<uintptr_t>(gpooled) & 15) ||
      (reinterpret_cast<uintptr_t>(a.pooled_out) & 15))
    return fail(TT_EINVAL, "tower: pooled rows and their gradient must be 16-B aligned");
  for (int t = 0; t < 2; ++t)
    if (shape->in_col[t] + shape->in_dim[t] > ldp) return fail(TT_EINVAL, "tower: input columns exceed the pooled row");
  char* ws = reinterpret_cast<char*>(workspace);
  a.s = *shape;
  a.B = B;
  a.pooled = pooled;
  a.ldp = ldp;
  a.gpooled = gpooled;
  a.params = params;
  a.wb = reinterpret_cast<const __bf16*>(ws + L.o_wb);
  a.wtb = reinterpret_cast<const __bf16*>(ws + L.o_wtb);
  a.wbf = reinterpret_cast<const __bf16*>(ws + L.o_wbf);
  a.wtbf = reinterpret_cast<const __bf16*>(ws + L.o_wtbf);
  for (int t = 0; t < 2; ++t)
    for (int l = 0; l < MAXL; ++l) {
      a.woff[t][l] = L.woff[t][l];
      a.boff[t][l] = L.boff[t][l];
      a.wcoff[t][l] = L.wcoff[t][l];
    }
  a.labels = labels;
  a.label_dtype = label_dtype;
  a.grad_scale = grad_scale;
  a.logits = logits;
  a.xt = reinterpret_cast<__bf16*>(ws + L.o_xt);
  a.act = reinterpret_cast<__bf16*>(ws + L.o_act);
  a.dzt = reinterpret_cast<__bf16*>(ws + L.o_dzt);
  a.dbpart = reinterpret_cast<float*>(ws + L.o_dbpart);
  a.loss_part = reinterpret_cast<float*>(ws + L.o_losspart);
  a.in_max = L.in_max;
  a.Bp = L.Bp;
  a.nwg = L.nwg;
#if TT_EXPERIMENTS
  if (const char* e = getenv("TT_T1_DEBUG")) a.dbg = atoi(e);
  if (a.dbg & 8) a.stamps = reinterpret_cast<int64_t*>(ws + L.o_dbg);
#endif
  const bool two = shape->L == 2 && shape->in_dim[0] <= 128 && shape->in_dim[1] <= 128;
  if ((a.gcol[0] || a.gpos[0]) && !two)
    return fail(TT_EINVAL, "tower: the fused gather needs 2 layers and inputs <= 128 wide");
  // TT_TOWER_GENERAL_T1 shapes keep tile-major operand strips for T2 (a.rm = L.rows is false for
  // them): only the general indexed kernel writes that layout for every shape, so every other T1
  // entry point refuses the flag rather than hand T2 strips in a layout it does not read
  if ((shape->flags & TT_TOWER_GENERAL_T1) && !a.ipos)
    return fail(TT_EINVAL, "tower: TT_TOWER_GENERAL_T1 shapes run T1 through tt_tower_fwd_bwd_indexed_multi only");
  // the row-owned T1 runs the L.rows shapes for every input but three: several features per tower
  // (ipos), multi-hot bags (mval) and fp32 rows by position (gpos without gsrc_bf16) are the classic
  // T1's, as is every other shape
  const bool rows = L.rows && !a.ipos && !a.mval && (!a.gpos[0] || a.gsrc_bf16);
  if (rows) {
    a.wimg = ws + L.o_wimg;
    return launch_t1_rows(a, stream);
  }
  // the in-place update exists in the row-owned T1 alone
  if (a.uw[0]) return fail(TT_EINVAL, "tower_gather_update: shapes in {64, 128} x [128, 64] only");
  return launch_t1_classic(a, stream);
}

}  // namespace tt

using namespace tt;

extern "C" {

int64_t tt_tower_num_params(const tt_tower_shape_t* shape) {
  TowerLayout L;
  if (tower_layout(shape, 8, &L)) return -1;
  return L.P;
}

size_t tt_tower_workspace_bytes(const tt_tower_shape_t* shape, int64_t B) {
  TowerLayout L;
  if (tower_layout(shape, B, &L)) return 0;
  return L.total;
}

int tt_tower_workspace_init(const tt_tower_shape_t* shape, int64_t B, void* workspace, size_t ws_bytes,
                            void* stream) {
  TowerLayout L;
  int rc = tower_ws_layout(shape, B, workspace, ws_bytes, &L);
  if (rc) return rc;
  hipStream_t st = as_stream(stream);
  char* ws = reinterpret_cast<char*>(workspace);
  if (hipMemsetAsync(ws, 0, L.total, st) != hipSuccess) return fail(TT_EINVAL, "tower: memset failed");
  if (L.lds) return hipStreamSynchronize(st) == hipSuccess ? TT_OK : fail(TT_EINVAL, "tower: init sync failed");
  // the tile list of the register-path T2 (host-built, copied once)
  std::vector<WgradTile> tiles;
  for (int t = 0; t < 2; ++t)
    for (int l = 0; l < shape->L; ++l)
      for (int n0 = 0; n0 < shape->width[l]; n0 += 32)
        for (int k0 = 0; k0 < L.K[t][l]; k0 += 32) tiles.push_back({t, l, n0, k0});
  if (hipMemcpyAsync(ws + L.o_tiles, tiles.data(), tiles.size() * sizeof(WgradTile), hipMemcpyHostToDevice, st) !=
      hipSuccess)
    return fail(TT_EINVAL, "tower: tile upload failed");
  return hipStreamSynchronize(st) == hipSuccess ? TT_OK : fail(TT_EINVAL, "tower: init sync failed");
}

int tt_tower_fwd_bwd(const tt_tower_shape_t* shape, int64_t B, const float* pooled, int64_t ldp, float* gpooled,
                     const float* params, const void* labels, int label_dtype, float grad_scale, float* logits,
                     void* workspace, size_t ws_bytes, void* stream) {
  TowerArgs a{};
  return launch_t1(shape, B, a, pooled, ldp, gpooled,
                   {params, labels, label_dtype, grad_scale, logits, workspace, ws_bytes, stream});
}

int tt_tower_fwd_bwd_gather(const tt_tower_shape_t* shape, int64_t B, const void* const* cols, int id_dtype,
                            const int64_t* num_embeddings, const float* const* table_rows, float* pooled_out,
                            int64_t ldp, float* gpooled, const float* params, const void* labels, int label_dtype,
                            float grad_scale, float* logits, const int32_t* dedup_tables, void* dedup_ws,
                            size_t dedup_ws_bytes, int64_t dedup_max_lookups, void* workspace, size_t ws_bytes,
                            void* stream) {
  if (!cols || !num_embeddings || !table_rows) return fail(TT_EINVAL, "tower_gather: null pointer");
  if (id_dtype != TT_I32 && id_dtype != TT_I64) return fail(TT_EINVAL, "tower_gather: ids must be int32/int64");
  TowerArgs a{};
  for (int t = 0; t < 2; ++t) {
    if (!cols[t] || !table_rows[t] || num_embeddings[t] < 1) return fail(TT_EINVAL, "tower_gather: bad column");
    if (reinterpret_cast<uintptr_t>(table_rows[t]) & 15) return fail(TT_EINVAL, "tower_gather: rows not 16-B aligned");
    a.gcol[t] = cols[t];
    a.gtab[t] = table_rows[t];
    a.gmod[t] = num_embeddings[t];
  }
  a.gid_dtype = id_dtype;
  a.pooled_out = pooled_out;
  if (dedup_ws) {
    if (!dedup_tables) return fail(TT_EINVAL, "tower_gather: dedup needs the key table of each tower");
    if (int rc = check_dedup_ws(dedup_ws, dedup_ws_bytes, dedup_max_lookups, 2 * B, "tower_gather", true)) return rc;
    for (int t = 0; t < 2; ++t) {
      if (dedup_tables[t] < 0 || dedup_tables[t] >= TT_MAX_TABLES || num_embeddings[t] >= (1ll << DD_TABLE_SHIFT))
        return fail(TT_EINVAL, "tower_gather: bad dedup table");
      a.dd_table[t] = dedup_tables[t];
    }
    dedup_layout(dedup_ws, dedup_max_lookups, &a.dd);
    a.dd_on = 1;
  }
  return launch_t1(shape, B, a, nullptr, ldp, gpooled,
                   {params, labels, label_dtype, grad_scale, logits, workspace, ws_bytes, stream});
}

int tt_tower_fwd_bwd_kjt(const tt_tower_shape_t* shape, int64_t B, const void* values, int id_dtype,
                         const int32_t* offsets, const int64_t* num_rows, const float* const* table_rows,
                         float* pooled_out, int64_t ldp, float* gpooled, const float* params, const void* labels,
                         int label_dtype, float grad_scale, float* logits, void* workspace, size_t ws_bytes,
                         void* stream) {
  if (!values || !offsets || !num_rows || !table_rows) return fail(TT_EINVAL, "tower_fwd_bwd_kjt: null pointer");
  if (id_dtype != TT_I32 && id_dtype != TT_I64) return fail(TT_EINVAL, "tower_fwd_bwd_kjt: ids must be int32/int64");
  TowerArgs a{};
  for (int t = 0; t < 2; ++t) {
    if (!table_rows[t] || num_rows[t] < 1) return fail(TT_EINVAL, "tower_fwd_bwd_kjt: bad table");
    if (reinterpret_cast<uintptr_t>(table_rows[t]) & 15)
      return fail(TT_EINVAL, "tower_fwd_bwd_kjt: rows not 16-B aligned");
    a.gtab[t] = table_rows[t];
    a.gmod[t] = num_rows[t];
    a.moff[t] = offsets + (int64_t)t * B;  // key-major: tower t's bags follow the previous key's B
  }
  a.mval = values;
  a.gid_dtype = id_dtype;
  a.pooled_out = pooled_out;
  return launch_t1(shape, B, a, nullptr, ldp, gpooled,
                   {params, labels, label_dtype, grad_scale, logits, workspace, ws_bytes, stream});
}

static int tower_indexed(const tt_tower_shape_t* shape, int64_t B, const int32_t* const* pos,
                         const float* const* rows_in, float* const* grad_rows_out, const T1Common& c, int bf16_rows) {
  if (!pos || !rows_in || !grad_rows_out) return fail(TT_EINVAL, "tower_indexed: null pointer");
  TowerArgs a{};
  a.gsrc_bf16 = bf16_rows;
  for (int t = 0; t < 2; ++t) {
    if (!pos[t] || !rows_in[t] || !grad_rows_out[t]) return fail(TT_EINVAL, "tower_indexed: null pointer");
    if ((reinterpret_cast<uintptr_t>(rows_in[t]) & 15) || (reinterpret_cast<uintptr_t>(grad_rows_out[t]) & 15))
      return fail(TT_EINVAL, "tower_indexed: rows not 16-B aligned");
    a.gpos[t] = pos[t];
    a.gsrc[t] = rows_in[t];
    a.gdst[t] = grad_rows_out[t];
  }
  return launch_t1(shape, B, a, nullptr,
                   std::max(shape->in_col[0] + shape->in_dim[0], shape->in_col[1] + shape->in_dim[1]), nullptr, c);
}

int tt_tower_fwd_bwd_indexed(const tt_tower_shape_t* shape, int64_t B, const int32_t* const* pos,
                             const float* const* rows_in, float* const* grad_rows_out, const float* params,
                             const void* labels, int label_dtype, float grad_scale, float* logits, void* workspace,
                             size_t ws_bytes, void* stream) {
  return tower_indexed(shape, B, pos, rows_in, grad_rows_out,
                       {params, labels, label_dtype, grad_scale, logits, workspace, ws_bytes, stream}, 0);
}

int tt_tower_fwd_bwd_indexed_bf16(const tt_tower_shape_t* shape, int64_t B, const int32_t* const* pos,
                                  const void* const* rows_in, float* const* grad_rows_out, const float* params,
                                  const void* labels, int label_dtype, float grad_scale, float* logits,
                                  void* workspace, size_t ws_bytes, void* stream) {
  return tower_indexed(shape, B, pos, reinterpret_cast<const float* const*>(rows_in), grad_rows_out,
                       {params, labels, label_dtype, grad_scale, logits, workspace, ws_bytes, stream}, 1);
}

int tt_tower_fwd_bwd_gather_update(const tt_tower_shape_t* shape, int64_t B, const void* const* cols, int id_dtype,
                                   const int64_t* num_embeddings, float* const* table_rows, float* const* table_state,
                                   float* pooled_out, int64_t ldp, float* gpooled, const float* params,
                                   const void* labels, int label_dtype, float grad_scale, float* logits, float lr,
                                   float eps, void* dedup_ws, size_t dedup_ws_bytes, int64_t dedup_max_lookups,
                                   const void* const* next_cols, void* workspace, size_t ws_bytes, void* stream) {
  if (!cols || !num_embeddings || !table_rows || !table_state || !dedup_ws)
    return fail(TT_EINVAL, "tower_gather_update: null pointer");
  if (id_dtype != TT_I32 && id_dtype != TT_I64) return fail(TT_EINVAL, "tower_gather_update: ids must be int32/int64");
  if (int rc = check_dedup_ws(dedup_ws, dedup_ws_bytes, dedup_max_lookups, 2 * B, "tower_gather_update", true)) return rc;
  TowerArgs a{};
  for (int t = 0; t < 2; ++t) {
    if (!cols[t] || !table_rows[t] || !table_state[t] || num_embeddings[t] < 1)
      return fail(TT_EINVAL, "tower_gather_update: bad column");
    if (reinterpret_cast<uintptr_t>(table_rows[t]) & 15) return fail(TT_EINVAL, "tower_gather_update: rows not 16-B aligned");
    a.gcol[t] = cols[t];
    a.gtab[t] = table_rows[t];
    a.gmod[t] = num_embeddings[t];
    a.uw[t] = table_rows[t];
    a.us[t] = table_state[t];
    // next_cols is checked and otherwise not read
    if (next_cols && !next_cols[t]) return fail(TT_EINVAL, "tower_gather_update: null next column");
  }
  a.gid_dtype = id_dtype;
  a.pooled_out = pooled_out;
  a.ulr = lr;
  a.ueps = eps;
  dedup_layout(dedup_ws, dedup_max_lookups, &a.dd);
  return launch_t1(shape, B, a, nullptr, ldp, gpooled,
                   {params, labels, label_dtype, grad_scale, logits, workspace, ws_bytes, stream});
}

int tt_tower_fwd_bwd_indexed_multi_bf16(const tt_tower_shape_t* shape, int64_t B, int D, const int32_t* pos_in,
                                        const int32_t* pos_out, const void* rows_in, float* grad_rows_out,
                                        const float* params, const void* labels, int label_dtype, float grad_scale,
                                        float* logits, void* workspace, size_t ws_bytes, void* stream) {
  if (!shape || !pos_in || !pos_out || !rows_in || !grad_rows_out)
    return fail(TT_EINVAL, "tower_indexed_multi: null pointer");
  if (D < 16 || D > 128 || D % 16 || XCH % D)
    return fail(TT_EINVAL, "tower_indexed_multi: feature dim must be 16..128, a multiple of 16 dividing 128");
  for (int t = 0; t < 2; ++t)
    if (shape->in_dim[t] % D) return fail(TT_EINVAL, "tower_indexed_multi: tower input not a multiple of D");
  if (shape->in_col[0] != 0 || shape->in_col[1] != shape->in_dim[0])
    return fail(TT_EINVAL, "tower_indexed_multi: query features first, then candidate features");
  if ((reinterpret_cast<uintptr_t>(rows_in) & 7) || (reinterpret_cast<uintptr_t>(grad_rows_out) & 3))
    return fail(TT_EINVAL, "tower_indexed_multi: rows not aligned");
  if (shape->L == 2 && shape->in_dim[0] <= 128 && shape->in_dim[1] <= 128 && !(shape->flags & TT_TOWER_GENERAL_T1))
    return fail(TT_EINVAL, "tower_indexed_multi: set TT_TOWER_GENERAL_T1 in the shape (T3 must keep the general "
                           "T1's weight copies)");
  TowerArgs a{};
  a.ipos = pos_in;
  a.ipos_out = pos_out;
  a.isrc = reinterpret_cast<const __bf16*>(rows_in);
  a.idst = grad_rows_out;
  a.ifeat0[0] = 0;
  a.ifeat0[1] = shape->in_dim[0] / D;
  a.iD = D;
  return launch_t1(shape, B, a, nullptr, shape->in_dim[0] + shape->in_dim[1], nullptr,
                   {params, labels, label_dtype, grad_scale, logits, workspace, ws_bytes, stream});
}

int tt_tower_fwd_bwd_indexed2_bf16(const tt_tower_shape_t* shape, int64_t B, const int32_t* const* pos_in,
                                   const int32_t* const* pos_out, const void* const* rows_in,
                                   float* const* grad_rows_out, const float* params, const void* labels,
                                   int label_dtype, float grad_scale, float* logits, void* workspace, size_t ws_bytes,
                                   const tt_peer_direct_t* direct, void* stream) {
  if (!pos_in || !pos_out || !rows_in || !grad_rows_out) return fail(TT_EINVAL, "tower_indexed2: null pointer");
  TowerArgs a{};
  if (direct) {
    if (int rc = peer_direct_check(*direct, "tower_indexed2")) return rc;
    if (grad_rows_out[0] != grad_rows_out[1])
      return fail(TT_EINVAL, "tower_indexed2: a direct exchange takes one send buffer (grad_rows_out[0] == [1])");
    a.xd = *direct;
  }
  a.gsrc_bf16 = 1;
  for (int t = 0; t < 2; ++t) {
    if (!pos_in[t] || !pos_out[t] || !rows_in[t] || !grad_rows_out[t]) return fail(TT_EINVAL, "tower_indexed2: null pointer");
    if ((reinterpret_cast<uintptr_t>(rows_in[t]) & 15) || (reinterpret_cast<uintptr_t>(grad_rows_out[t]) & 15))
      return fail(TT_EINVAL, "tower_indexed2: rows not 16-B aligned");
    a.gpos[t] = pos_in[t];
    a.gpos_out[t] = pos_out[t];
    a.gsrc[t] = reinterpret_cast<const float*>(rows_in[t]);
    a.gdst[t] = grad_rows_out[t];
  }
  return launch_t1(shape, B, a, nullptr,
                   std::max(shape->in_col[0] + shape->in_dim[0], shape->in_col[1] + shape->in_dim[1]), nullptr,
                   {params, labels, label_dtype, grad_scale, logits, workspace, ws_bytes, stream});
}

// ---- launch plans (include/tt_mi355x.h): the multi-role fused launches behind one entry point ----
int tt_launch(const tt_launch_plan_t* p, void* stream) {
  if (!p) return fail(TT_EINVAL, "launch: null plan");
  const tt_update_role_t& u = p->update;
  const tt_insert_role_t& in = p->insert;
  const tt_adagrad_role_t& g = p->adagrad;
  auto need_multi = [&](int want) {
    return g.multi_only == want ? TT_OK
                                : fail(TT_EINVAL, want ? "launch: this plan updates only rows looked up more than once "
                                                         "(adagrad.multi_only = 1)"
                                                       : "launch: this plan updates every row (adagrad.multi_only = 0)");
  };
  // the in-launch exchange wait is launch U's alone
  if (p->wait && p->roles != (TT_ROLE_WGRAD | TT_ROLE_ROUTE_COUNT | TT_ROLE_ADAGRAD) &&
      p->roles != (TT_ROLE_ROUTE_COUNT | TT_ROLE_ADAGRAD))
    return fail(TT_EINVAL, "launch: only launch U (ROUTE_COUNT | ADAGRAD [| WGRAD]) takes a wait");
  auto adam_mode = [&]() {
    return u.replicated ? fail(TT_EINVAL, "launch: this plan's UPDATE role runs Adam (update.replicated = 0)") : TT_OK;
  };
  int rc = TT_OK;
  switch (p->roles) {
    case TT_ROLE_WGRAD | TT_ROLE_INSERT | TT_ROLE_ADAGRAD:
      if ((rc = need_multi(1))) return rc;
      // the ring tail's lookups per feature are the plan's B (the tower batch): a different
      // adagrad.B is a caller error, not something to ignore
      if (g.B && g.B != p->B) return fail(TT_EINVAL, "launch: this plan's ADAGRAD role uses the plan's B (adagrad.B = 0 or B)");
      if ((in.dedup_ws_bytes && in.dedup_ws_bytes != g.dedup_ws_bytes) ||
          (in.dedup_max_lookups && in.dedup_max_lookups != g.dedup_max_lookups))
        return fail(TT_EINVAL, "launch: the ring's two dedup workspaces have one size (the ADAGRAD role's)");
      return fused_wgrad_insert_adagrad(*p, stream);
    case TT_ROLE_WGRAD | TT_ROLE_INSERT:
      return fused_wgrad_insert(*p, stream);
    case TT_ROLE_UPDATE | TT_ROLE_ADAGRAD | TT_ROLE_RESOLVE:
      if ((rc = need_multi(1)) || (rc = adam_mode())) return rc;
      return fused_update_adagrad_resolve(*p, stream);
    case TT_ROLE_WGRAD | TT_ROLE_ADAGRAD:
      if ((rc = need_multi(0))) return rc;
      return fused_wgrad_adagrad(*p, stream);
    case TT_ROLE_UPDATE | TT_ROLE_ADAGRAD:
      if ((rc = need_multi(0)) || (rc = adam_mode())) return rc;
      return fused_update_adagrad(*p, stream);
    case TT_ROLE_WGRAD | TT_ROLE_ROUTE_COUNT | TT_ROLE_ADAGRAD:
      if ((rc = need_multi(0))) return rc;
      return fused_wgrad_route_count_adagrad(*p, stream);
    case TT_ROLE_ROUTE_COUNT | TT_ROLE_ADAGRAD:
      if ((rc = need_multi(0))) return rc;
      return fused_route_count_adagrad(*p, stream);
    case TT_ROLE_UPDATE | TT_ROLE_ROUTE_PLACE | TT_ROLE_GATHER:
      if (!u.replicated) return fail(TT_EINVAL, "launch: launch G's UPDATE role writes the replicated gradient "
                                                "(update.replicated = 1)");
      return fused_grads_route_place_gather(*p, stream);
    default:
      return fail(TT_EINVAL, "launch: no fused launch runs this set of roles (see tt_launch_plan_t)");
  }
}

}  // extern "C"
