// Fused tower inference on gfx950 (tt_tower_embed): table rows (a range or an id list) through the
// whole tower MLP (Linear + ReLU on every layer) in one launch, result in fp32 or bf16.
//
// The arithmetic is gemm.hip's bf16 forward chain, layer by layer: X and W rounded to bf16 by the same
// (__bf16) conversion, v_mfma_f32_16x16x32_bf16 over K in ascending steps of 32 from a zero accumulator
// with the activation row in the A position and the weight row in the B position, bias added in fp32,
// fmaxf(x, 0), and the fp32 activation rounded to bf16 where the next layer's tt_linear_fwd would round
// it on load. An output element depends on its own row and its own weight row only, so the bits do not
// depend on M, on the tile a row lands in or on how the row was addressed.
//
// Shape of the launch: a persistent grid, one workgroup of up to 8 waves per CU (two where the LDS
// image is small). Each workgroup converts the whole tower's weights to bf16 once into an LDS image
// ([n][K + 8] per layer: k contiguous, so a B fragment is one 16-B ds_read; the 16-B pad spreads the 16
// rows of a fragment over the banks) and the biases to an fp32 image beside it. After that one barrier
// the waves are independent: a wave owns tiles of 32 rows (two 16-row MFMA row tiles, so every weight
// fragment read feeds two MFMAs) and strides over them. Per tile:
//   1. the tile's rows, loaded with whole-row coalesced 16-B loads into registers one tile ahead (the
//      loads of tile t + 1 are in flight under the MFMAs of tile t), are rounded to bf16 into the
//      wave's LDS buffer ([32][maxw + 8] bf16);
//   2. per layer all A fragments of the wave's rows are read into registers, then per 32 output columns
//      the weight fragments stream from the image through 4 independent accumulators, and the epilogue
//      writes the bf16 activation back into the same buffer in the C layout (col = lane & 15,
//      row = (lane >> 4) * 4 + r), which is the next layer's A image. In place is safe: the A fragments
//      are in registers before the first write, and a wave's LDS operations execute in order;
//   3. the last layer's epilogue writes the result into the buffer in the output type (fp32 rows of
//      N + 4 floats, or the bf16 activation image as it stands), and the wave copies whole rows to
//      ``out`` with 16-B stores.
// No workspace, no workgroup barrier inside the loop, no atomics but the bad-row count.
#include "tt_common.h"

namespace tt {
namespace embed {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;

constexpr int MAXL = 4;
constexpr int MAXW = 128;         // widest layer (and in_dim)
constexpr int ROWS = 32;          // rows of a wave's tile: two MFMA row tiles
constexpr int PAD = 8;            // bf16 elements (16 B) after every LDS row
constexpr int LDS_BYTES = 163840; // 160 KiB per CU
constexpr int NUM_CU = 256;
constexpr int BIAS_BYTES = MAXL * MAXW * 4;

struct Args {
  const float* table;
  int64_t ld, num_rows;
  const void* rows;
  int64_t first_row, M, tiles;
  const float* W[MAXL];
  const float* bias[MAXL];
  void* out;
  int64_t ldo;
  int32_t* bad_rows;
  int32_t width[MAXL];
  int32_t woff[MAXL];  // byte offset of layer l's weight image
  int32_t L, row_i64, out_bf16;
  int32_t bias_off;    // byte offset of the bias image; the waves' buffers follow it
  int32_t abytes;      // bytes of a wave's buffer
  int32_t astride;     // its row stride as an activation image, in bf16 elements
};

struct Plan {
  int waves, lds, bias_off, abytes, astride;
  int woff[MAXL];
};

static bool in_range(int in_dim, int L, const int32_t* widths) {
  if (L < 1 || L > MAXL || !widths) return false;
  if (in_dim < 32 || in_dim > MAXW || in_dim % 32) return false;
  for (int l = 0; l < L; ++l)
    if (widths[l] < 32 || widths[l] > MAXW || widths[l] % 32) return false;
  return true;
}

// The LDS plan: the weight images, the bias image, then as many wave buffers (8, 4, 2 or 1) as fit.
// A wave's buffer holds its 32 rows as a bf16 activation image of the widest layer, or the fp32
// result rows where those are larger.
static bool make_plan(int in_dim, int L, const int32_t* widths, bool out_f32, Plan& p) {
  if (!in_range(in_dim, L, widths)) return false;
  int off = 0, maxw = in_dim, k = in_dim;
  for (int l = 0; l < L; ++l) {
    p.woff[l] = off;
    off += widths[l] * (k + PAD) * 2;
    k = widths[l];
    maxw = std::max(maxw, k);
  }
  p.bias_off = off;
  off += BIAS_BYTES;
  p.astride = maxw + PAD;
  p.abytes = ROWS * std::max(p.astride * 2, out_f32 ? (widths[L - 1] + 4) * 4 : 0);
  for (int w = 8; w >= 1; w >>= 1)
    if (off + w * p.abytes <= LDS_BYTES) {
      p.waves = w;
      p.lds = off + w * p.abytes;
      return true;
    }
  return false;
}

// The rows of tile t into registers: chunk c = i * 64 + lane of the tile's [32][in_dim / 4] 16-B chunks,
// so a wave instruction reads whole consecutive rows. Lane l < 32 resolves row l's index; a row
// outside the table (or past M) reads as zeros and never forms an address.
template <int KS0>
__device__ __forceinline__ void load_rows(const Args& a, int64_t t, int lane, f32x4 (&x)[KS0 * 4], int& bad) {
  constexpr int CPR = KS0 * 8;
  const int64_t m = t * ROWS + (lane & 31);
  int64_t r = -1;
  if (m < a.M) {
    if (a.rows)
      r = a.row_i64 ? reinterpret_cast<const int64_t*>(a.rows)[m] : (int64_t) reinterpret_cast<const int32_t*>(a.rows)[m];
    else
      r = a.first_row + m;
    if ((uint64_t)r >= (uint64_t)a.num_rows) {
      r = -1;
      if (lane < 32) ++bad;
    }
  }
#pragma unroll
  for (int i = 0; i < KS0 * 4; ++i) {
    const int c = i * 64 + lane;
    const int row = c / CPR, cc = c % CPR;
    const int64_t rr = __shfl(r, row, 64);
    f32x4 v = (f32x4)(0.f);
    if (rr >= 0) v = *reinterpret_cast<const f32x4*>(a.table + rr * a.ld + cc * 4);
    x[i] = v;
  }
}

// One layer on the wave's 32 rows. ``buf`` holds the bf16 input image ([32][astride]); the result goes
// back into it as the bf16 image (F32OUT = false) or as fp32 rows of N + 4 floats (F32OUT = true).
template <int KS, bool F32OUT>
__device__ __forceinline__ void layer(const char* wimg, const float* bimg, bool has_bias, int N, char* buf, int astride,
                                      int lane) {
  constexpr int WS = KS * 32 + PAD;
  const __bf16* A = reinterpret_cast<const __bf16*>(buf) + (lane & 15) * astride + (lane >> 4) * 8;
  bf16x8 af[2][KS];
#pragma unroll
  for (int rt = 0; rt < 2; ++rt)
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) af[rt][ks] = *reinterpret_cast<const bf16x8*>(A + rt * 16 * astride + ks * 32);
  const __bf16* Wl = reinterpret_cast<const __bf16*>(wimg) + (lane & 15) * WS + (lane >> 4) * 8;
  for (int n0 = 0; n0 < N; n0 += 32) {
    f32x4 acc[2][2];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[rt][j] = (f32x4)(0.f);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const bf16x8 b0 = *reinterpret_cast<const bf16x8*>(Wl + n0 * WS + ks * 32);
      const bf16x8 b1 = *reinterpret_cast<const bf16x8*>(Wl + (n0 + 16) * WS + ks * 32);
#pragma unroll
      for (int rt = 0; rt < 2; ++rt) {
        acc[rt][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[rt][ks], b0, acc[rt][0], 0, 0, 0);
        acc[rt][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[rt][ks], b1, acc[rt][1], 0, 0, 0);
      }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = n0 + j * 16 + (lane & 15);
      const float bv = bimg[col];
#pragma unroll
      for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = rt * 16 + (lane >> 4) * 4 + r;
          float v = acc[rt][j][r];
          if (has_bias) v += bv;
          v = fmaxf(v, 0.f);
          if (F32OUT)
            reinterpret_cast<float*>(buf)[row * (N + 4) + col] = v;
          else
            reinterpret_cast<__bf16*>(buf)[row * astride + col] = (__bf16)v;
        }
    }
  }
}

template <bool F32OUT>
__device__ __forceinline__ void layer_k(int ks, const char* wimg, const float* bimg, bool has_bias, int N, char* buf,
                                        int astride, int lane) {
  switch (ks) {
    case 1: layer<1, F32OUT>(wimg, bimg, has_bias, N, buf, astride, lane); break;
    case 2: layer<2, F32OUT>(wimg, bimg, has_bias, N, buf, astride, lane); break;
    case 3: layer<3, F32OUT>(wimg, bimg, has_bias, N, buf, astride, lane); break;
    default: layer<4, F32OUT>(wimg, bimg, has_bias, N, buf, astride, lane); break;
  }
}

template <int KS0>
__global__ void __launch_bounds__(512) tower_embed_kernel(Args a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;

  // the tower's weights, bf16, and its biases, once per workgroup
  {
    int K = KS0 * 32;
    for (int l = 0; l < a.L; ++l) {
      const int N = a.width[l], kc = K >> 3, total = N * kc;
      const float* W = a.W[l];
      __bf16* img = reinterpret_cast<__bf16*>(smem + a.woff[l]);
      const bool al = (reinterpret_cast<uintptr_t>(W) & 15) == 0;
      for (int i = tid; i < total; i += blockDim.x) {
        const int n = i / kc, c = i - n * kc;
        const float* s = W + n * K + c * 8;
        float v[8];
        if (al) {
          const f32x4 x0 = reinterpret_cast<const f32x4*>(s)[0], x1 = reinterpret_cast<const f32x4*>(s)[1];
          v[0] = x0[0]; v[1] = x0[1]; v[2] = x0[2]; v[3] = x0[3];
          v[4] = x1[0]; v[5] = x1[1]; v[6] = x1[2]; v[7] = x1[3];
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] = s[j];
        }
        bf16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (__bf16)v[j];
        *reinterpret_cast<bf16x8*>(img + n * (K + PAD) + c * 8) = o;
      }
      float* bimg = reinterpret_cast<float*>(smem + a.bias_off) + l * MAXW;
      const float* b = a.bias[l];
      for (int i = tid; i < N; i += blockDim.x) bimg[i] = b ? b[i] : 0.f;
      K = N;
    }
  }
  __syncthreads();

  char* buf = smem + a.bias_off + BIAS_BYTES + wave * a.abytes;
  const int astride = a.astride;
  const int NL = a.width[a.L - 1];
  // the copy-out's walk over the result's 16-B chunks: chunk c = lane, lane + 64, ... of [32][cpr]
  const int cpr = a.out_bf16 ? NL >> 3 : NL >> 2;
  const int sstride = a.out_bf16 ? astride * 2 : (NL + 4) * 4;  // bytes of a staged result row
  const int cq = 64 / cpr, crem = 64 - cq * cpr, crow0 = lane / cpr, ccc0 = lane - crow0 * cpr;
  const int64_t obytes = a.ldo * (a.out_bf16 ? 2 : 4);

  const int64_t GW = (int64_t)gridDim.x * nw;
  int64_t t = (int64_t)blockIdx.x * nw + wave;
  f32x4 x[KS0 * 4];
  int bad = 0;
  if (t < a.tiles) load_rows<KS0>(a, t, lane, x, bad);
  while (t < a.tiles) {
    // the rows, bf16, into the wave's buffer
#pragma unroll
    for (int i = 0; i < KS0 * 4; ++i) {
      constexpr int CPR = KS0 * 8;
      const int c = i * 64 + lane;
      const int row = c / CPR, cc = c % CPR;
      bf16x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = (__bf16)x[i][j];
      *reinterpret_cast<bf16x4*>(reinterpret_cast<__bf16*>(buf) + row * astride + cc * 4) = o;
    }
    __builtin_amdgcn_wave_barrier();
    // the next tile's rows: in flight under this tile's MFMAs
    const int64_t tn = t + GW;
    if (tn < a.tiles) load_rows<KS0>(a, tn, lane, x, bad);

    int ks = KS0;
    for (int l = 0; l < a.L; ++l) {
      const int N = a.width[l];
      const char* wimg = smem + a.woff[l];
      const float* bimg = reinterpret_cast<const float*>(smem + a.bias_off) + l * MAXW;
      const bool hb = a.bias[l] != nullptr;
      if (l == a.L - 1 && !a.out_bf16) {
        if (l == 0)
          layer<KS0, true>(wimg, bimg, hb, N, buf, astride, lane);
        else
          layer_k<true>(ks, wimg, bimg, hb, N, buf, astride, lane);
      } else {
        if (l == 0)
          layer<KS0, false>(wimg, bimg, hb, N, buf, astride, lane);
        else
          layer_k<false>(ks, wimg, bimg, hb, N, buf, astride, lane);
      }
      ks = N >> 5;
      __builtin_amdgcn_wave_barrier();
    }

    // whole result rows to ``out``
    {
      int row = crow0, cc = ccc0;
      char* o = reinterpret_cast<char*>(a.out);
      for (int c = lane; c < ROWS * cpr; c += 64) {
        const int64_t m = t * ROWS + row;
        if (m < a.M)
          *reinterpret_cast<f32x4*>(o + m * obytes + cc * 16) = *reinterpret_cast<const f32x4*>(buf + row * sstride + cc * 16);
        cc += crem;
        row += cq;
        if (cc >= cpr) {
          cc -= cpr;
          ++row;
        }
      }
    }
    __builtin_amdgcn_wave_barrier();
    t = tn;
  }
  if (a.bad_rows) {
    const int n = wave_sum_i(bad);
    if (lane == 0 && n) atomicAdd(a.bad_rows, n);
  }
}

template <int KS0>
static int launch(const Args& a, const Plan& p, unsigned blocks, hipStream_t st) {
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(&tower_embed_kernel<KS0>),
                          hipFuncAttributeMaxDynamicSharedMemorySize, p.lds) != hipSuccess)
    return fail(TT_EINVAL, "tt_tower_embed: the LDS image was refused");
  tower_embed_kernel<KS0><<<dim3(blocks), dim3(p.waves * 64), p.lds, st>>>(a);
  return check_launch("tt_tower_embed");
}

}  // namespace embed
}  // namespace tt

using namespace tt;
using namespace tt::embed;

extern "C" {

int tt_tower_embed_supported(int in_dim, int L, const int32_t* widths) {
  Plan p;
  // the fp32 result needs the larger wave buffer: a shape runs with either result type or not at all
  return make_plan(in_dim, L, widths, true, p) ? 1 : 0;
}

int tt_tower_embed(const float* table, int64_t ld, int64_t num_rows, int in_dim, const void* rows, int row_dtype,
                   int64_t first_row, int64_t M, int L, const int32_t* widths, const float* const* W,
                   const float* const* bias, void* out, int out_dtype, int64_t ldo, int32_t* bad_rows, void* stream) {
  const std::string fn = "tt_tower_embed: ";
  if (L < 1 || L > MAXL) return fail(TT_EINVAL, fn + "L must be 1..4");
  if (!table || !widths || !W || !out) return fail(TT_EINVAL, fn + "table, widths, W and out must not be null");
  if (in_dim < 32 || in_dim > MAXW || in_dim % 32) return fail(TT_EINVAL, fn + "in_dim must be a multiple of 32 in [32, 128]");
  for (int l = 0; l < L; ++l) {
    if (widths[l] < 32 || widths[l] > MAXW || widths[l] % 32)
      return fail(TT_EINVAL, fn + "every width must be a multiple of 32 in [32, 128]");
    if (!W[l]) return fail(TT_EINVAL, fn + "W[l] is null");
  }
  if (M < 0) return fail(TT_EINVAL, fn + "M must be >= 0");
  if (num_rows < 1) return fail(TT_EINVAL, fn + "num_rows must be >= 1");
  if (ld < in_dim || (ld & 3) || (reinterpret_cast<uintptr_t>(table) & 15))
    return fail(TT_EINVAL, fn + "ld must be >= in_dim and a multiple of 4, table 16-B aligned");
  if (out_dtype != TT_F32 && out_dtype != TT_BF16) return fail(TT_EINVAL, fn + "out_dtype must be TT_F32 or TT_BF16");
  const bool f32 = out_dtype == TT_F32;
  if (ldo < widths[L - 1] || (ldo & (f32 ? 3 : 7)) || (reinterpret_cast<uintptr_t>(out) & 15))
    return fail(TT_EINVAL, fn + "ldo must be >= the last width with 16-B aligned rows (a multiple of 4 fp32 / 8 bf16 "
                                "elements), out 16-B aligned");
  if (rows) {
    if (row_dtype != TT_I32 && row_dtype != TT_I64) return fail(TT_EINVAL, fn + "row_dtype must be TT_I32 or TT_I64");
    if (first_row != 0) return fail(TT_EINVAL, fn + "first_row must be 0 with a row list");
  } else if (first_row < 0 || first_row > num_rows || M > num_rows - first_row) {
    return fail(TT_EINVAL, fn + "the row range [first_row, first_row + M) must lie in [0, num_rows)");
  }
  Plan p;
  if (!tt_tower_embed_supported(in_dim, L, widths) || !make_plan(in_dim, L, widths, f32, p))
    return fail(TT_EINVAL, fn + "unsupported shape (tt_tower_embed_supported): the weight image does not fit in LDS "
                                "beside a wave's row tile");
  if (M == 0) return TT_OK;

  Args a{};
  a.table = table; a.ld = ld; a.num_rows = num_rows;
  a.rows = rows; a.row_i64 = row_dtype == TT_I64;
  a.first_row = first_row; a.M = M; a.tiles = ceil_div(M, ROWS);
  for (int l = 0; l < L; ++l) {
    a.W[l] = W[l];
    a.bias[l] = bias ? bias[l] : nullptr;
    a.width[l] = widths[l];
    a.woff[l] = p.woff[l];
  }
  a.out = out; a.ldo = ldo; a.out_bf16 = f32 ? 0 : 1;
  a.bad_rows = bad_rows;
  a.L = L; a.bias_off = p.bias_off; a.abytes = p.abytes; a.astride = p.astride;
  const int per_cu = p.lds * 2 <= LDS_BYTES ? 2 : 1;
  const unsigned blocks = (unsigned)std::min<int64_t>(ceil_div(a.tiles, p.waves), (int64_t)NUM_CU * per_cu);
  hipStream_t st = as_stream(stream);
  switch (in_dim >> 5) {
    case 1: return launch<1>(a, p, blocks, st);
    case 2: return launch<2>(a, p, blocks, st);
    case 3: return launch<3>(a, p, blocks, st);
    default: return launch<4>(a, p, blocks, st);
  }
}

}  // extern "C"
