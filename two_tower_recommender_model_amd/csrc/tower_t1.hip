// The classic T1 of the fused tower step (tower.hip): the general kernel (tower_fwd_bwd_kernel: any
// depth and width, several features per tower), the two-layer kernel (tower_l2_kernel) and their launch.
#include "tower_common.h"

namespace tt {

// acc[mt][j] += A(lds, rows 16*mt..) x B(global bf16, k-major rows) over K (multiple of 32)
// B fragment: lane reads 8 consecutive k of "column" n from a [n][k]-layout matrix (ldb elems).
__device__ __forceinline__ void mma_lds_global(f32x4 (&acc)[2][2], const __bf16* As, int lda_s,
                                               const __bf16* Bg, int64_t ldb, int K, int n0a, int n0b,
                                               bool has_b) {
  // K <= 128 (4 k-steps): every B fragment (weights, L2-resident) is issued before the first
  // MFMA so the GEMM pays one L2 round trip, not one per k-step.
  const int lane = threadIdx.x & 63;
  const int r = lane & 15, q = lane >> 4;
  const int nk = K >> 5;
  bf16x8 b0[4], b1[4];
  const __bf16* p0 = Bg + (int64_t)(n0a + r) * ldb + q * 8;
  const __bf16* p1 = Bg + (int64_t)(n0b + r) * ldb + q * 8;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    if (s < nk) {
      b0[s] = *reinterpret_cast<const bf16x8*>(p0 + s * 32);
      if (has_b) b1[s] = *reinterpret_cast<const bf16x8*>(p1 + s * 32);
    }
  }
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    if (s < nk) {
      const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(As + r * lda_s + s * 32 + q * 8);
      const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(As + (16 + r) * lda_s + s * 32 + q * 8);
      acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b0[s], acc[0][0], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b0[s], acc[1][0], 0, 0, 0);
      if (has_b) {
        acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b1[s], acc[0][1], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b1[s], acc[1][1], 0, 0, 0);
      }
    }
  }
}

__global__ void __launch_bounds__(256) tower_fwd_bwd_kernel(TowerArgs a) {
  // LDS: X chunk, activations per (tower, layer) bf16, last-layer outputs fp32, dZ ping-pong
  __shared__ __attribute__((aligned(16))) __bf16 xs[TR * LSTR];
  __shared__ __attribute__((aligned(16))) __bf16 acts[2][MAXL][TR * LSTR];
  __shared__ __attribute__((aligned(16))) float outf[2][TR * FSTR];
  __shared__ __attribute__((aligned(16))) __bf16 dz[2][TR * LSTR];
  __shared__ float dlog[TR];
  __shared__ float lpart[TR];

  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int r16 = lane & 15, q4 = lane >> 4;
  const int64_t B = a.B;
  const int64_t m0 = (int64_t)blockIdx.x * TR;
  const int L = a.s.L;

  // ================= forward, both towers =================
  for (int t = 0; t < 2; ++t) {
    const int in = a.s.in_dim[t];
    for (int l = 0; l < L; ++l) {
      const int N = a.s.width[l];
      const int K = l == 0 ? in : a.s.width[l - 1];
      const int ntile = N / 16;
      // this wave's n-tiles: wid and wid + 4
      const bool h0 = wid < ntile, h1 = wid + 4 < ntile;
      f32x4 acc[2][2];
      for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2; ++j) acc[i][j] = (f32x4)(0.f);
      const __bf16* Wg = a.wb + a.wcoff[t][l];
      if (l == 0) {
        for (int k0 = 0; k0 < K; k0 += XCH) {
          const int kc = min(XCH, K - k0);
          // stage X[m0.., in_col + k0 ..] fp32 -> bf16 LDS, and X^T to global for T2
          for (int e = threadIdx.x; e < TR * (kc / 4); e += 256) {
            const int row = e / (kc / 4), c4 = (e % (kc / 4)) * 4;
            const int64_t gm = m0 + row;
            bf16x4 bv;
            if (a.ipos) {  // the feature's row as returned by its owner (bf16, what T1 computes on)
              const int kk = k0 + c4, f = a.ifeat0[t] + kk / a.iD;
              const int32_t p = gm < B ? a.ipos[(int64_t)f * B + gm] : -1;
              bv = p >= 0 ? *reinterpret_cast<const bf16x4*>(a.isrc + (int64_t)p * a.iD + kk % a.iD)
                          : (bf16x4)(__bf16)0.f;
            } else {
              f32x4 v = (f32x4)(0.f);
              if (gm < B) v = *reinterpret_cast<const f32x4*>(a.pooled + gm * a.ldp + a.s.in_col[t] + k0 + c4);
              bv[0] = (__bf16)v[0]; bv[1] = (__bf16)v[1]; bv[2] = (__bf16)v[2]; bv[3] = (__bf16)v[3];
            }
            *reinterpret_cast<bf16x4*>(xs + row * LSTR + c4) = bv;
          }
          __syncthreads();
          // X^T [t][k][B]: thread -> (k, 8 consecutive rows)
          for (int e = threadIdx.x; e < kc * (TR / 8); e += 256) {
            const int k = e / (TR / 8), rb = (e % (TR / 8)) * 8;
            bf16x8 v;
            for (int j = 0; j < 8; ++j) v[j] = xs[(rb + j) * LSTR + k];
            const int64_t gm = m0 + rb;
            __bf16* dst = a.xt + (int64_t)t * a.in_max * a.Bp + strip_at(k0 + k, gm, a.in_max);
            if (gm + 8 <= B) {
              *reinterpret_cast<bf16x8*>(dst) = v;
            } else {
              for (int j = 0; j < 8; ++j)
                if (gm + j < B) dst[j] = v[j];
            }
          }
          if (h0) mma_lds_global(acc, xs, LSTR, Wg + k0, K, kc, wid * 16, (wid + 4) * 16, h1);
          __syncthreads();
        }
      } else {
        if (h0) mma_lds_global(acc, acts[t][l - 1], LSTR, Wg, K, K, wid * 16, (wid + 4) * 16, h1);
      }
      // epilogue: bias + relu -> LDS (bf16; fp32 too for the last layer), act^T -> global
      const float* bias = a.params + a.boff[t][l];
      for (int j = 0; j < 2; ++j) {
        if (!(j == 0 ? h0 : h1)) continue;
        const int col = (wid + 4 * j) * 16 + r16;
        const float bv = bias[col];
        for (int i = 0; i < 2; ++i) {
          bf16x4 pk;
          for (int rr = 0; rr < 4; ++rr) {
            const int row = i * 16 + q4 * 4 + rr;
            const float v = fmaxf(acc[i][j][rr] + bv, 0.f);
            acts[t][l][row * LSTR + col] = (__bf16)v;
            pk[rr] = (__bf16)v;
            if (l == L - 1) outf[t][row * FSTR + col] = v;
          }
          if (l < L - 1) {
            const int64_t gm = m0 + i * 16 + q4 * 4;
            __bf16* dst = a.act + ((int64_t)t * MAXL + l) * MAXW * a.Bp + strip_at(col, gm, MAXW);
            if (gm + 4 <= B) {
              *reinterpret_cast<bf16x4*>(dst) = pk;
            } else {
              for (int rr = 0; rr < 4; ++rr)
                if (gm + rr < B) dst[rr] = pk[rr];
            }
          }
        }
      }
      __syncthreads();
    }
  }

  // ================= logits, BCE, dlogit =================
  const int NL = a.s.width[L - 1];
  {
    // 8 threads per row
    const int row = threadIdx.x >> 3, sub = threadIdx.x & 7;
    float d = 0.f;
    for (int c = sub; c < NL; c += 8) d += outf[0][row * FSTR + c] * outf[1][row * FSTR + c];
    d += __shfl_xor(d, 1, 64);
    d += __shfl_xor(d, 2, 64);
    d += __shfl_xor(d, 4, 64);
    const int64_t gm = m0 + row;
    float lo = 0.f, dl = 0.f;
    if (gm < B) {
      const float x = d, y = lbl(a.labels, a.label_dtype, gm);
      const float lsig = fminf(x, 0.f) - log1pf(expf(-fabsf(x)));
      lo = (1.f - y) * x - lsig;
      dl = (1.f / (1.f + expf(-x)) - y) / (float)B * a.grad_scale;
      if (sub == 0) a.logits[gm] = x;
    }
    if (sub == 0) {
      dlog[row] = dl;
      lpart[row] = lo;
    }
  }
  __syncthreads();

  // ================= backward, tower by tower =================
  for (int t = 0; t < 2; ++t) {
    // dZ_{L-1} = dlogit * other * (self > 0): thread -> (8 consecutive rows, column), fp32
    {
      const float* self_ = outf[t];
      const float* other = outf[1 - t];
      float* dbp = a.dbpart + (((int64_t)t * MAXL + (L - 1)) * a.nwg + blockIdx.x) * MAXW;
      for (int c = threadIdx.x >> 2; c < NL; c += 64) {
        const int rb = (threadIdx.x & 3) * 8;
        bf16x8 v;
        float s = 0.f;
        for (int j = 0; j < 8; ++j) {
          const int row = rb + j;
          float z = self_[row * FSTR + c] > 0.f ? dlog[row] * other[row * FSTR + c] : 0.f;
          if (m0 + row >= B) z = 0.f;
          s += z;
          v[j] = (__bf16)z;
          dz[0][row * LSTR + c] = (__bf16)z;
        }
        // bias-grad partial: 4 threads per column, fixed order
        s += __shfl_xor(s, 1, 64);
        s += __shfl_xor(s, 2, 64);
        if ((threadIdx.x & 3) == 0) dbp[c] = s;
        const int64_t gm = m0 + rb;
        __bf16* dst = a.dzt + ((int64_t)t * MAXL + (L - 1)) * MAXW * a.Bp + strip_at(c, gm, MAXW);
        if (gm + 8 <= B) {
          *reinterpret_cast<bf16x8*>(dst) = v;
        } else {
          for (int j = 0; j < 8; ++j)
            if (gm + j < B) dst[j] = v[j];
        }
      }
    }
    __syncthreads();
    int cur = 0;
    for (int l = L - 1; l >= 1; --l) {
      // dA_{l-1} = dZ_l W_l : [TR, K=width[l]] x [width[l], width[l-1]], B from W^T [in][out]
      const int Kd = a.s.width[l];
      const int N = a.s.width[l - 1];
      const int ntile = N / 16;
      const bool h0 = wid < ntile, h1 = wid + 4 < ntile;
      f32x4 acc[2][2];
      for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2; ++j) acc[i][j] = (f32x4)(0.f);
      if (h0) mma_lds_global(acc, dz[cur], LSTR, a.wtb + a.wcoff[t][l], Kd, Kd, wid * 16, (wid + 4) * 16, h1);
      // dZ_{l-1} = dA * (act_{l-1} > 0)
      float* dbp = a.dbpart + (((int64_t)t * MAXL + (l - 1)) * a.nwg + blockIdx.x) * MAXW;
      for (int j = 0; j < 2; ++j) {
        if (!(j == 0 ? h0 : h1)) continue;
        const int col = (wid + 4 * j) * 16 + r16;
        float s = 0.f;
        for (int i = 0; i < 2; ++i) {
          bf16x4 pk;
          for (int rr = 0; rr < 4; ++rr) {
            const int row = i * 16 + q4 * 4 + rr;
            float z = (float)acts[t][l - 1][row * LSTR + col] > 0.f ? acc[i][j][rr] : 0.f;
            if (m0 + row >= B) z = 0.f;
            s += z;
            pk[rr] = (__bf16)z;
            dz[cur ^ 1][row * LSTR + col] = (__bf16)z;
          }
          const int64_t gm = m0 + i * 16 + q4 * 4;
          __bf16* dst = a.dzt + ((int64_t)t * MAXL + (l - 1)) * MAXW * a.Bp + strip_at(col, gm, MAXW);
          if (gm + 4 <= B) {
            *reinterpret_cast<bf16x4*>(dst) = pk;
          } else {
            for (int rr = 0; rr < 4; ++rr)
              if (gm + rr < B) dst[rr] = pk[rr];
          }
        }
        s += __shfl_xor(s, 16, 64);
        s += __shfl_xor(s, 32, 64);
        if (q4 == 0) dbp[col] = s;
      }
      __syncthreads();
      cur ^= 1;
    }
    // dX = dZ_0 W_0 : [TR, width[0]] x [width[0], in] -> fp32 into the pooled gradient
    {
      const int in = a.s.in_dim[t];
      const int Kd = a.s.width[0];
      const __bf16* WT = a.wtb + a.wcoff[t][0];  // [in][width0]
      for (int c0 = 0; c0 < in; c0 += XCH) {
        const int nc = min(XCH, in - c0);
        const int ntile = nc / 16;
        const bool h0 = wid < ntile, h1 = wid + 4 < ntile;
        f32x4 acc[2][2];
        for (int i = 0; i < 2; ++i)
          for (int j = 0; j < 2; ++j) acc[i][j] = (f32x4)(0.f);
        if (h0) mma_lds_global(acc, dz[cur], LSTR, WT, Kd, Kd, c0 + wid * 16, c0 + (wid + 4) * 16, h1);
        for (int j = 0; j < 2; ++j) {
          if (!(j == 0 ? h0 : h1)) continue;
          const int col = c0 + (wid + 4 * j) * 16 + r16;
          if (a.ipos) {  // dX column -> the lookup's gradient row in the exchange buffer
            const int f = a.ifeat0[t] + col / a.iD, cc = col % a.iD;
            for (int i = 0; i < 2; ++i)
              for (int rr = 0; rr < 4; ++rr) {
                const int64_t gm = m0 + i * 16 + q4 * 4 + rr;
                const int32_t p = gm < B ? a.ipos_out[(int64_t)f * B + gm] : -1;
                if (p >= 0) a.idst[(int64_t)p * a.iD + cc] = acc[i][j][rr];
              }
            continue;
          }
          for (int i = 0; i < 2; ++i)
            for (int rr = 0; rr < 4; ++rr) {
              const int64_t gm = m0 + i * 16 + q4 * 4 + rr;
              if (gm < B) a.gpooled[gm * a.ldp + a.s.in_col[t] + col] = acc[i][j][rr];
            }
        }
      }
    }
    __syncthreads();
  }

  // loss: per-workgroup partial; T2 sums the partials in a fixed order (no cross-workgroup
  // hand-off inside T1: a release fence here costs more than the rest of the epilogue)
  if (threadIdx.x == 0) {
    float p = 0.f;
    for (int i = 0; i < TR; ++i) p += lpart[i];
    a.loss_part[blockIdx.x] = p;
  }
}

// ---------------------------------------------------------------------------------------------
// T1 fast path: two layers per tower, every width <= 128. 512 threads: waves 0-3 run the query
// tower, waves 4-7 the candidate tower, in lockstep. Every weight fragment a wave needs for the
// whole step (fwd L0, fwd L1, bwd L1, bwd L0: up to 32 x 16 B per lane) is issued at kernel
// entry together with the X rows, so the only global round trip on the chain is X itself; the rest
// is LDS + MFMA.

struct Frags {
  bf16x8 f[4][2];
};

// fragments of W (fragment-major copy, see frag_off): one 1-KB contiguous load per (tile, k-step)
__device__ __forceinline__ void load_frags(Frags& fr, const __bf16* Wf, int ld, int K, int N, int w4) {
  const int lane = threadIdx.x & 63;
  const int nk = K >> 5, nt = N >> 4;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int tile = w4 + 4 * j;
#pragma unroll
    for (int s = 0; s < 4; ++s)
      if (tile < nt && s < nk)
        fr.f[s][j] = *reinterpret_cast<const bf16x8*>(Wf + ((int64_t)(tile * nk + s) * 64 + lane) * 8);
  }
}

__device__ __forceinline__ void mma_frags(f32x4 (&acc)[2][2], const __bf16* As, const Frags& fr, int K, int N,
                                          int w4) {
  const int lane = threadIdx.x & 63;
  const int r = lane & 15, q = lane >> 4;
  const int nk = K >> 5, nt = N >> 4;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = (f32x4)(0.f);
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    if (s < nk) {
      const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(As + r * LSTR + s * 32 + q * 8);
      const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(As + (16 + r) * LSTR + s * 32 + q * 8);
#pragma unroll
      for (int j = 0; j < 2; ++j)
        if (w4 + 4 * j < nt) {
          acc[0][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, fr.f[s][j], acc[0][j], 0, 0, 0);
          acc[1][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, fr.f[s][j], acc[1][j], 0, 0, 0);
        }
    }
  }
}

// T1's W0 image in LDS: [hidden unit][input column] bf16 in 256-B rows whose 16-B chunks are
// XOR-swizzled by row (CDNA4 guide T10, layout (b)). Layer 0 takes its W0 fragments from global
// memory and files them here; the dX product reads the SAME image transposed
// (ds_read_b64_tr_b16) instead of loading a second, transposed copy of W0 from global memory.
__device__ __forceinline__ int w0_off(int row, int ch) {  // byte offset of 16-B chunk ch of row
  return 256 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3)));
}

// f0 (B fragments of W0 as layer 0 reads it: lane r + 16 q of fragment (k-step s, tile j) holds
// W0[tile * 16 + r][s * 32 + 8 q .. + 7], one 16-B chunk) -> the image
__device__ __forceinline__ void w0_image_store(char* img, const Frags& f0, int K, int N, int w4) {
  const int lane = threadIdx.x & 63;
  const int r = lane & 15, q = lane >> 4;
  const int nk = K >> 5, nt = N >> 4;
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int s = 0; s < 4; ++s)
      if (w4 + 4 * j < nt && s < nk)
        *reinterpret_cast<bf16x8*>(img + w0_off((w4 + 4 * j) * 16 + r, 4 * s + q)) = f0.f[s][j];
}

// acc = A (LDS rows, K = W0 columns) x W0 (the image, [K = hidden][N = input]): the B fragment of
// (k-step s, n-tile nt) is B[s * 32 + 8 q + e][nt * 16 + r] = image[row s * 32 + 8 q + e][col nt * 16 + r],
// two transposed reads of 4 image rows x 16 columns each (lane 4 q' + p of a 16-lane group
// addresses row q', columns 4 p .. 4 p + 3; lane i receives column i). Every lane of the wave
// executes the reads (wave-uniform conditions only: the read needs a full EXEC mask).
__device__ __forceinline__ void mma_w0_tr(f32x4 (&acc)[2][2], const __bf16* As, const char* img, int K, int N,
                                          int w4) {
  const int lane = threadIdx.x & 63;
  const int r = lane & 15, q = lane >> 4;
  const int qq = (lane & 15) >> 2, p = lane & 3;
  const int nk = K >> 5, nt = N >> 4;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = (f32x4)(0.f);
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    if (s < nk) {
      const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(As + r * LSTR + s * 32 + q * 8);
      const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(As + (16 + r) * LSTR + s * 32 + q * 8);
#pragma unroll
      for (int j = 0; j < 2; ++j)
        if (w4 + 4 * j < nt) {
          const int row = s * 32 + 8 * q + qq, ch = 2 * (w4 + 4 * j) + (p >> 1);
          const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
              (lds_bf16x4*)(img + w0_off(row, ch) + 8 * (p & 1)));
          const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
              (lds_bf16x4*)(img + w0_off(row + 4, ch) + 8 * (p & 1)));
          const bf16x8 b = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
          acc[0][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b, acc[0][j], 0, 0, 0);
          acc[1][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b, acc[1][j], 0, 0, 0);
        }
    }
  }
}

// sum over each 16-lane row, every lane of the row receives it: quad_perm [1,0,3,2], quad_perm
// [2,3,0,1], row_half_mirror, row_mirror (each step adds the mirrored partner's partial sum, so
// partners compute identical values)
__device__ __forceinline__ float row16_sum(float v) {
  v += dpp_f<0xB1>(v);
  v += dpp_f<0x4E>(v);
  v += dpp_f<0x141>(v);
  v += dpp_f<0x140>(v);
  return v;
}

// 4 consecutive rows r0.. of one strip feature (tile-local row r0, nval valid rows in the tile)
__device__ __forceinline__ void store_t4(__bf16* dst, const bf16x4& pk, int r0, int nval) {
  if (r0 + 4 <= nval) {
    *reinterpret_cast<bf16x4*>(dst) = pk;
  } else {
    for (int rr = 0; rr < 4; ++rr)
      if (r0 + rr < nval) dst[rr] = pk[rr];
  }
}

// Multi-hot EBC forward inside T1 (MH): thread tt of tower t's 256-thread group owns the float4
// column c4 of rows (tt + 256 i) / LPR, i < NXV, as the single-hot gather does. The LPR lanes of a
// row group walk the concatenation of their NXV bags (bag order kept inside each bag) in chunks of
// LPR ids, one coalesced id read per chunk (the next chunk's ids in flight beside this chunk's
// rows), ids broadcast by lane shuffles, R rows in flight per lane whatever the bag lengths. Each
// bag's rows are added in bag order starting from zero: the fp32 sums are bit-identical to
// tt_pooled_fwd (SUM) of the same bag.
template <int IN_>
__device__ __forceinline__ void mh_gather(const TowerArgs& a, int t, int tt, int64_t m0, int64_t B,
                                          f32x4 (&xv)[4]) {
  constexpr int LPR = IN_ / 4;   // lanes per row: 32 (D 128) or 16 (D 64)
  constexpr int NXV = IN_ / 32;  // rows (bags) per thread: 4 or 2
  constexpr int R = IN_ == 128 ? 16 : 8;  // rows in flight per lane (D 64: 8, no spills)
  static_assert(LPR % R == 0, "a chunk is a whole number of rounds");
  const int lane = threadIdx.x & 63;
  const int lg = lane & (LPR - 1), gb = lane & ~(LPR - 1);
  const float* tab = t ? a.gtab[1] : a.gtab[0];
  const int32_t* off = t ? a.moff[1] : a.moff[0];
  const uint64_t nrows = (uint64_t)(t ? a.gmod[1] : a.gmod[0]);
  const float* colp = tab + lg * 4;
  int s[NXV], p[NXV + 1];
  p[0] = 0;
#pragma unroll
  for (int i = 0; i < NXV; ++i) {
    const int64_t gm = m0 + (tt + 256 * i) / LPR;
    s[i] = 0;
    int n = 0;
    if (gm < B) {
      s[i] = off[gm];
      n = off[gm + 1] - s[i];
    }
    p[i + 1] = p[i] + n;
    xv[i] = (f32x4)(0.f);
  }
  const int total = p[NXV];
  // combined position k (< total) -> element offset of its table row (an id >= rows reads row 0)
  auto row_at = [&](int k) -> int64_t {
    int si = s[0], pi = 0;
#pragma unroll
    for (int i = 1; i < NXV; ++i)
      if (k >= p[i]) {
        si = s[i];
        pi = p[i];
      }
    const int64_t id = load_id(a.mval, a.gid_dtype, (int64_t)si + (k - pi));
    return (uint64_t)id < nrows ? id * IN_ : 0;
  };
  int64_t nxt = lg < total ? row_at(lg) : 0;
  for (int k0 = 0; __ballot(k0 < total) != 0; k0 += LPR) {
    const int64_t cur = nxt;
    if (k0 + LPR + lg < total) nxt = row_at(k0 + LPR + lg);
#pragma unroll
    for (int k = 0; k < LPR; k += R) {
      if (__ballot(k0 + k < total) == 0) break;
      f32x4 r[R];
#pragma unroll
      for (int u = 0; u < R; ++u) {
        const int64_t o = __shfl((long long)cur, gb + k + u, 64);
        r[u] = k0 + k + u < total ? *reinterpret_cast<const f32x4*>(colp + o) : (f32x4)(0.f);
      }
#pragma unroll
      for (int u = 0; u < R; ++u) {
        const int kk = k0 + k + u;
#pragma unroll
        for (int i = 0; i < NXV; ++i)
          if (kk >= p[i] && kk < p[i + 1]) xv[i] += r[u];
      }
    }
  }
}

// IN_/W0_/W1_: compile-time tower input width and layer widths (0 = read from the shape at run
// time). With them fixed every fragment load is unconditional, so the waitcnt that guards X (issued
// first) does not also wait for the weight fragments issued behind it.
// 8 compute waves + 1 dedup wave; the compute path has exactly T1_BARRIERS __syncthreads
constexpr int T1_THREADS = 576;
constexpr int T1_BARRIERS = 7;

// R16: indexed rows arrive as bf16 (sharded step, tt_tower_fwd_bwd_indexed_bf16); its own
// instantiation, so the other modes' code and registers are untouched.
template <int IN_, int W0_, int W1_, bool R16 = false, bool MH = false>
__global__ void __launch_bounds__(T1_THREADS) tower_l2_kernel(TowerArgs a) {
  __shared__ __attribute__((aligned(16))) __bf16 xs[2][TR * LSTR];   // X, later dZ0
  __shared__ __attribute__((aligned(16))) __bf16 hs[2][TR * LSTR];   // hidden activation (bf16)
  __shared__ __attribute__((aligned(16))) __bf16 dzs[2][TR * LSTR];  // dZ1
  __shared__ __attribute__((aligned(16))) float outf[2][TR * FSTR];  // tower outputs, later dX (fp32)
  __shared__ float dlog[TR];
  __shared__ float lpart[TR];
  __shared__ __attribute__((aligned(16))) char w0img[2][128 * 256];  // W0 image (w0_off), per tower

  // wid via readfirstlane: the compiler then knows t (below) is wave-uniform and reads a.gcol[t],
  // a.gtab[t], ... with scalar loads (a per-lane index into the kernarg arrays is a vector load from
  // the kernarg segment: one more dependent memory hop in front of the row gather)
  const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // the [128, 64] towers over 64- or 128-wide inputs write ROW-MAJOR operand strips ([Bp][features], as the
  // row-owned T1 does; the tail reads them with wgrad_lds_block_rm): copies of the LDS tiles
  constexpr bool RM = (IN_ == 128 || IN_ == 64) && W0_ == 128 && W1_ == 64;
  auto rm_copy = [&](const __bf16* tile, __bf16* dst, int nchunk, int ld, int nval_) {
    // tile: TR rows at LSTR; dst: row 0 of the tile in a [Bp][ld] strip; nchunk 16-B pieces per row
    const int tt_ = threadIdx.x & 255;
    for (int idx = tt_; idx < TR * nchunk; idx += 256) {
      const int row = idx / nchunk, ch = idx % nchunk;
      if (row < nval_)
        *reinterpret_cast<bf16x8*>(dst + (int64_t)row * ld + ch * 8) = *reinterpret_cast<const bf16x8*>(tile + row * LSTR + ch * 8);
    }
  };
  if (wid == 8) {
    // ---- the dedup wave: files this workgroup's 2 x TR lookups (gather + dedup) into the hash
    // table; its CAS round trips count only in ITS vmcnt, so the 8 compute waves never wait on
    // them. It passes the compute waves' barriers (T1_BARRIERS, all unconditional) in step.
    const int tq = lane / TR, row = lane % TR;
    const int64_t gm = (int64_t)xcd_remap((int)blockIdx.x, (int)gridDim.x) * TR + row;
    const bool own = a.dd_on && gm < a.B;
    DdPend p;
    if (own) {
      // per-lane tower: select between the two towers' kernel arguments (no dynamic kernarg index)
      const int64_t id = load_id(tq ? a.gcol[1] : a.gcol[0], a.gid_dtype, gm);
      const int64_t mod = tq ? a.gmod[1] : a.gmod[0];
      const uint64_t tab = (uint64_t)(tq ? a.dd_table[1] : a.dd_table[0]);
      const uint64_t key = id != 0 ? ((tab << DD_TABLE_SHIFT) | (uint64_t)py_mod64(id, mod)) : DD_EMPTY;
      dd_insert_begin(a.dd, key, (int32_t)(tq * a.B + gm), p);
    } else {
      p.key = DD_EMPTY;
    }
    // the CAS results are needed only after two barriers (about half the compute chain later); a
    // lookup that did not claim a free slot is deferred to the next launch's resolver instead of
    // probing here (dd_insert_defer_finish): this wave's tail is one atomic round trip
    __syncthreads();
    __syncthreads();
    if (a.dd_on) dd_insert_defer_finish(a.dd, p, (int32_t)(tq * a.B + gm), xcd_remap((int)blockIdx.x, (int)gridDim.x));
#if TT_EXPERIMENTS
    if (a.stamps && lane == 0) a.stamps[(int64_t)blockIdx.x * 16 + 8] = (int64_t)__builtin_amdgcn_s_memrealtime();
#endif
#pragma unroll 1
    for (int k = 2; k < T1_BARRIERS; ++k) __syncthreads();
    return;
  }
  const int t = wid >> 2, w4 = wid & 3;
  T1_STAMP(0);
  T1_WSTAMP(0);
  const int tt = threadIdx.x & 255;  // thread index inside the tower group
  const int r16 = lane & 15, q4 = lane >> 4;
  const int64_t B = a.B;
  // the tile: a contiguous 1/8 per XCD (xcd_remap), as tower_rows_body; per-tile partials by tile
  const int tl2 = xcd_remap((int)blockIdx.x, (int)gridDim.x);
  const int64_t m0 = (int64_t)tl2 * TR;
  const int nval = (int)min((int64_t)TR, B - m0);  // valid rows of this tile (32-bit row tests)
  // this tile's run of each T1 -> T2 strip (tile-major, strip_at): wave-uniform bases, so a
  // store's address is base + (feature * TR + row) in 32 bits
  const int64_t tile_el = (int64_t)tl2 * TR;
  __bf16* const xt_tile = a.xt + (int64_t)t * a.in_max * a.Bp + tile_el * a.in_max;
  __bf16* const act_tile = a.act + ((int64_t)t * MAXL + 0) * MAXW * a.Bp + tile_el * MAXW;
  __bf16* const dz0_tile = a.dzt + ((int64_t)t * MAXL + 0) * MAXW * a.Bp + tile_el * MAXW;
  __bf16* const dz1_tile = a.dzt + ((int64_t)t * MAXL + 1) * MAXW * a.Bp + tile_el * MAXW;
  float* const db0 = a.dbpart + (((int64_t)t * MAXL + 0) * a.nwg + tl2) * MAXW;
  float* const db1 = a.dbpart + (((int64_t)t * MAXL + 1) * a.nwg + tl2) * MAXW;
  const int in = IN_ ? IN_ : a.s.in_dim[t];
  const int W0 = W0_ ? W0_ : a.s.width[0];
  const int W1 = W1_ ? W1_ : a.s.width[1];

  // ---- 0. everything this wave will read from global: X rows first (the chain waits on them),
  // then every weight fragment of the step in order of use, then the biases
  f32x4 xv[4];
  bf16x4 xb[4];  // R16: the bf16 rows as loaded (T1 stores bf16 to LDS anyway: no widening)
  const int nxv = in / 32;  // f32x4 loads per thread: TR rows x in/4 vectors over 256 threads
  const bool gather = a.gcol[t] != nullptr;
  const bool indexed = a.gpos[t] != nullptr;
  const int incol = a.s.in_col[t];  // read once, before any store (no vmcnt waits mid-chain)
  int32_t rpos[4];                   // indexed: the dX row of each xv (gpos_out, else its input row)
#pragma unroll
  for (int i = 0; i < 4; ++i) rpos[i] = -1;
  if constexpr (MH) {
    mh_gather<IN_>(a, t, tt, m0, B, xv);
  } else if (gather || indexed) {
    // single-hot: the embedding row itself (EBC forward fused in); id 0 -> empty bag -> zeros.
    // Indexed rows may be bf16 (tt_tower_fwd_bwd_indexed_bf16): byte offsets with the element size
    const bool r16 = R16;
    const char* src[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      src[i] = nullptr;
      rpos[i] = -1;
      if (i < nxv) {
        const int e = tt + 256 * i;
        const int row = e / (in / 4), c4 = (e % (in / 4)) * 4;
        const int64_t gm = m0 + row;
        if (gm < B) {
          if (indexed) {
            const int32_t pin = a.gpos[t][gm];
            rpos[i] = pin >= 0 && a.gpos_out[t] ? a.gpos_out[t][gm] : pin;
            if (pin >= 0)
              src[i] = reinterpret_cast<const char*>(a.gsrc[t]) + ((int64_t)pin * in + c4) * (r16 ? 2 : 4);
          } else {
            const int64_t id = TDBG(32) ? 1 : load_id(a.gcol[t], a.gid_dtype, gm);
            if (id != 0)
              src[i] = reinterpret_cast<const char*>(a.gtab[t] + (TDBG(4) ? 0 : py_mod64(id, a.gmod[t])) * in + c4);
          }
        }
      }
    }
    if (r16) {
#pragma unroll
      for (int i = 0; i < 4; ++i) xb[i] = src[i] ? *reinterpret_cast<const bf16x4*>(src[i]) : (bf16x4)(__bf16)0.f;
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) xv[i] = src[i] ? *reinterpret_cast<const f32x4*>(src[i]) : (f32x4)(0.f);
    }
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      xv[i] = (f32x4)(0.f);
      if (i < nxv) {
        const int e = tt + 256 * i;
        const int row = e / (in / 4), c4 = (e % (in / 4)) * 4;
        const int64_t gm = m0 + row;
        if (gm < B) xv[i] = *reinterpret_cast<const f32x4*>(a.pooled + gm * a.ldp + incol + c4);
      }
    }
  }
  Frags f0, f1, g1;
  if (TDBG(16)) {
    for (int s_ = 0; s_ < 4; ++s_) for (int j_ = 0; j_ < 2; ++j_) { f0.f[s_][j_] = (bf16x8)(__bf16)0.f; f1.f[s_][j_] = f0.f[s_][j_]; g1.f[s_][j_] = f0.f[s_][j_]; }
  } else {
  load_frags(f0, a.wbf + a.wcoff[t][0], in, in, W0, w4);      // W0 [W0][in]
  load_frags(f1, a.wbf + a.wcoff[t][1], W0, W0, W1, w4);      // W1 [W1][W0]
  load_frags(g1, a.wtbf + a.wcoff[t][1], W1, W1, W0, w4);     // W1^T [W0][W1]
  }
  float bias0[2], bias1[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int c = (w4 + 4 * j) * 16 + r16;
    bias0[j] = c < W0 ? a.params[a.boff[t][0] + c] : 0.f;
    bias1[j] = c < W1 ? a.params[a.boff[t][1] + c] : 0.f;
  }
  // the label of the row this thread scores in phase 3 (loaded now: no global load after the CAS)
  const int64_t lrow = m0 + (threadIdx.x >> 4);
  const float ylab = lrow < B ? lbl(a.labels, a.label_dtype, lrow) : 0.f;
  const float gscale = a.grad_scale / (float)B;

#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (i < nxv) {
      const int e = tt + 256 * i;
      const int row = e / (in / 4), c4 = (e % (in / 4)) * 4;
      bf16x4 bv;
      if (R16) {
        bv = xb[i];
      } else {
        bv[0] = (__bf16)xv[i][0]; bv[1] = (__bf16)xv[i][1]; bv[2] = (__bf16)xv[i][2]; bv[3] = (__bf16)xv[i][3];
      }
      *reinterpret_cast<bf16x4*>(xs[t] + row * LSTR + c4) = bv;
      const int64_t gm = m0 + row;
      if (!R16 && a.pooled_out && gm < B)
        *reinterpret_cast<f32x4*>(a.pooled_out + gm * a.ldp + incol + c4) = xv[i];
    }
  }
  // vmcnt(0) while only this wave's loads are outstanding (X, weight fragments, biases, label; the
  // fragments and biases come from L2 right behind X). Without it the compiler's merge of the
  // label-dtype branches leaves the biases "pending", and their first use in phase 1 becomes a
  // vmcnt(0) issued AFTER phase 1's strip stores: a wait for HBM store acknowledgements mid-chain.
  __builtin_amdgcn_s_waitcnt(0x0F70);
  T1_WSTAMP(1);
  __syncthreads();
  T1_STAMP(1);
  // X^T for T2's dW0 (fire-and-forget stores). A 16-lane group takes a block of 16 columns x 8
  // rows of X with two transposed LDS reads (ds_read_b64_tr_b16: lane 4 q' + p addresses row q',
  // columns 4 p .. 4 p + 3 of a 4-row block; lane i receives column i): lane i then holds rows
  // r0 .. r0 + 7 of column c0 + i, one 16-B strip store. Every lane executes the reads (full EXEC):
  // groups past the last block read block 0 and store nothing.
  if (RM) {
    rm_copy(xs[t], a.xt + (int64_t)t * a.in_max * a.Bp + m0 * a.in_max, IN_ / 8, (int)a.in_max, nval);
  } else if (!TDBG(1)) {
    const int g16 = lane >> 4, i16 = lane & 15, qq = i16 >> 2, pp = i16 & 3;
    const int nblk = (in / 16) * (TR / 8);  // blocks of 16 columns x 8 rows
    for (int b0 = w4 * 4; b0 < nblk; b0 += 16) {  // wave-uniform
      const int b = b0 + g16;
      const bool own = b < nblk;
      const int cb = own ? b % (in / 16) : 0, r0 = own ? (b / (in / 16)) * 8 : 0;
      const __bf16* src = xs[t] + (r0 + qq) * LSTR + cb * 16 + 4 * pp;
      const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)src);
      const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(src + 4 * LSTR));
      const bf16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
      if (own) {
        __bf16* dst = xt_tile + (cb * 16 + i16) * TR + r0;
        if (r0 + 8 <= nval) {
          *reinterpret_cast<bf16x8*>(dst) = v;
        } else {
          for (int j = 0; j < 8; ++j)
            if (r0 + j < nval) dst[j] = v[j];
        }
      }
    }
  }
  T1_WSTAMP(11);
  f32x4 acc[2][2];
  // ---- 1. layer 0: h = relu(X W0^T + b0)
  mma_frags(acc, xs[t], f0, in, W0, w4);
  T1_WSTAMP(12);
  w0_image_store(w0img[t], f0, in, W0, w4);  // read back transposed by the dX product (phase 6)
  T1_WSTAMP(13);
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    if (w4 + 4 * j >= W0 / 16) continue;
    const int col = (w4 + 4 * j) * 16 + r16;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      bf16x4 pk;
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int row = i * 16 + q4 * 4 + rr;
        const float v = fmaxf(acc[i][j][rr] + bias0[j], 0.f);
        pk[rr] = (__bf16)v;
        hs[t][row * LSTR + col] = pk[rr];
      }
      const int r0 = i * 16 + q4 * 4;
      if (!RM && !TDBG(1)) store_t4(act_tile + col * TR + r0, pk, r0, nval);
    }
  }
  T1_WSTAMP(2);
  __syncthreads();
  T1_STAMP(2);
  if (RM) rm_copy(hs[t], a.act + ((int64_t)t * MAXL + 0) * MAXW * a.Bp + m0 * MAXW, W0_ / 8, MAXW, nval);
  // ---- 2. layer 1: out = relu(h W1^T + b1) (fp32)
  mma_frags(acc, hs[t], f1, W0, W1, w4);
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    if (w4 + 4 * j >= W1 / 16) continue;
    const int col = (w4 + 4 * j) * 16 + r16;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int row = i * 16 + q4 * 4 + rr;
        outf[t][row * FSTR + col] = fmaxf(acc[i][j][rr] + bias1[j], 0.f);
      }
  }
  T1_WSTAMP(3);
  __syncthreads();
  T1_STAMP(3);
  // ---- 3. logits, BCE, dlogit: 16 threads per row
  {
    // 16 lanes per row, 4 consecutive columns per lane (one 16-B LDS read per tower), DPP sum
    // over the row's lanes; BCE from one exp, one log and one reciprocal (hardware
    // transcendentals, ~1 ulp) — the phase is one dependent chain per wave, so its length is its
    // instruction count
    const int row = threadIdx.x >> 4, sub = threadIdx.x & 15;
    float d = 0.f;
    for (int c = sub * 4; c < W1; c += 64) {
      const f32x4 u = *reinterpret_cast<const f32x4*>(&outf[0][row * FSTR + c]);
      const f32x4 v = *reinterpret_cast<const f32x4*>(&outf[1][row * FSTR + c]);
      d = fmaf(u[0], v[0], d);
      d = fmaf(u[1], v[1], d);
      d = fmaf(u[2], v[2], d);
      d = fmaf(u[3], v[3], d);
    }
    d = row16_sum(d);
    const int64_t gm = m0 + row;
    float lo = 0.f, dl = 0.f;
    if (gm < B) {
      const float x = d, y = ylab;
      const float e = __expf(-fabsf(x));  // exp(-|x|) in (0, 1]
      const float l1p = e < 1e-4f ? e * (1.f - 0.5f * e) : __logf(1.f + e);
      const float lsig = fminf(x, 0.f) - l1p;  // log(sigmoid(x))
      lo = (1.f - y) * x - lsig;
      const float rc = __builtin_amdgcn_rcpf(1.f + e);
      dl = ((x >= 0.f ? rc : e * rc) - y) * gscale;  // (sigmoid(x) - y) * grad_scale / B
      if (sub == 0) a.logits[gm] = x;
    }
    if (sub == 0) {
      dlog[row] = dl;
      lpart[row] = lo;
    }
  }
  T1_WSTAMP(4);
  __syncthreads();
  T1_STAMP(4);
  // ---- 4. dZ1 = dlogit * other * (self > 0): thread -> (column, 8 consecutive rows)
  for (int c = tt >> 2; c < W1; c += 64) {
    const int rb = (tt & 3) * 8;
    bf16x8 v;
    float s = 0.f, zz[8];
    for (int j = 0; j < 8; ++j) {
      const int row = rb + j;
      float z = outf[t][row * FSTR + c] > 0.f ? dlog[row] * outf[1 - t][row * FSTR + c] : 0.f;
      if (row >= nval) z = 0.f;
      zz[j] = z;
      s += z;
      v[j] = (__bf16)z;
      dzs[t][row * LSTR + c] = v[j];
    }
    if (RM) {
      // the row-owned T1's tree (rk_colsum, then the two 16-row halves): rows paired at row bits
      // 3 (the quad partner ^ 1), 2, 1, 0 (in thread), then the halves (quad partner ^ 2)
#pragma unroll
      for (int j = 0; j < 8; ++j) zz[j] += dpp_f<0xB1>(zz[j]);
#pragma unroll
      for (int j = 0; j < 4; ++j) zz[j] += zz[j + 4];
      zz[0] += zz[2];
      zz[1] += zz[3];
      s = zz[0] + zz[1];
      s += dpp_f<0x4E>(s);
    } else {
      s += dpp_f<0xB1>(s);  // the 4 lanes of a column are one quad: xor 1, then xor 2
      s += dpp_f<0x4E>(s);
    }
    if ((tt & 3) == 0) db1[c] = s;
    __bf16* dst = dz1_tile + c * TR + rb;
    if (RM || TDBG(1)) {
    } else if (rb + 8 <= nval) {
      *reinterpret_cast<bf16x8*>(dst) = v;
    } else {
      for (int j = 0; j < 8; ++j)
        if (rb + j < nval) dst[j] = v[j];
    }
  }
  T1_WSTAMP(5);
  __syncthreads();
  T1_STAMP(5);
  if (RM) rm_copy(dzs[t], a.dzt + ((int64_t)t * MAXL + 1) * MAXW * a.Bp + m0 * MAXW, W1_ / 8, MAXW, nval);
  // ---- 5. dZ0 = (dZ1 W1) * (h > 0)  -> xs (X is no longer needed)
  mma_frags(acc, dzs[t], g1, W1, W0, w4);
  T1_WSTAMP(14);
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    if (w4 + 4 * j >= W0 / 16) continue;
    const int col = (w4 + 4 * j) * 16 + r16;
    float s = 0.f, hsum[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      bf16x4 pk;
      float zz[4];
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int row = i * 16 + q4 * 4 + rr;
        float z = (float)hs[t][row * LSTR + col] > 0.f ? acc[i][j][rr] : 0.f;
        if (row >= nval) z = 0.f;
        zz[rr] = z;
        s += z;
        pk[rr] = (__bf16)z;
        xs[t][row * LSTR + col] = pk[rr];
      }
      if (RM) {
        // the row-owned T1's tree over the 16-row half i: row bits 3 (lanes ^ 32), 2 (^ 16), 1, 0
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) zz[rr] += __shfl_xor(zz[rr], 32, 64);
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) zz[rr] += __shfl_xor(zz[rr], 16, 64);
        hsum[i] = (zz[0] + zz[2]) + (zz[1] + zz[3]);
      }
      const int r0 = i * 16 + q4 * 4;
      if (!RM && !TDBG(1)) store_t4(dz0_tile + col * TR + r0, pk, r0, nval);
    }
    if (RM) {
      s = hsum[0] + hsum[1];
    } else {
      s += __shfl_xor(s, 16, 64);
      s += __shfl_xor(s, 32, 64);
    }
    if (q4 == 0) db0[col] = s;
  }
  T1_WSTAMP(6);
  __syncthreads();
  T1_STAMP(6);
  if (RM) rm_copy(xs[t], a.dzt + ((int64_t)t * MAXL + 0) * MAXW * a.Bp + m0 * MAXW, W0_ / 8, MAXW, nval);
  // ---- 6. dX = dZ0 W0 -> LDS (outf is free since phase 4) -> pooled gradient, whole rows
  mma_w0_tr(acc, xs[t], w0img[t], W0, in, w4);
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    if (w4 + 4 * j >= in / 16) continue;
    const int col = (w4 + 4 * j) * 16 + r16;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) outf[t][(i * 16 + q4 * 4 + rr) * FSTR + col] = acc[i][j][rr];
  }
  // ---- 7. loss: per-workgroup partial (T2 sums the partials in a fixed order)
  if (threadIdx.x == 0) {
    float p = 0.f;
    for (int i = 0; i < TR; ++i) p += lpart[i];
    a.loss_part[tl2] = p;
  }
  T1_WSTAMP(7);
  __syncthreads();
  T1_STAMP(7);
  T1_WSTAMP(9);
  // ---- 8. dX from LDS
  f32x4 gq[4];
  float* dstq[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    dstq[i] = nullptr;
    gq[i] = (f32x4)(0.f);
    if (i < nxv) {
      const int e = tt + 256 * i;
      const int row = e / (in / 4), c4 = (e % (in / 4)) * 4;
      const int64_t gm = m0 + row;
      if (gm < B) {
        if (indexed)
          dstq[i] = rpos[i] >= 0 ? a.gdst[t] + (int64_t)rpos[i] * in + c4 : nullptr;
        else
          dstq[i] = a.gpooled + gm * a.ldp + incol + c4;
      }
      gq[i] = *reinterpret_cast<const f32x4*>(&outf[t][row * FSTR + c4]);
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (i < nxv && dstq[i] && !TDBG(2)) *reinterpret_cast<f32x4*>(dstq[i]) = gq[i];
  T1_WSTAMP(8);
  T1_STAMP(15);
}

// the classic T1 for a filled TowerArgs: the general kernel for several features per tower and for
// shapes that are not two layers over inputs <= 128 wide, else tower_l2_kernel, at the compile-time
// shapes or with run-time widths
int launch_t1_classic(const TowerArgs& a, void* stream) {
  const int i0 = a.s.in_dim[0], i1 = a.s.in_dim[1], w0 = a.s.width[0], w1 = a.s.width[1];
  const dim3 g(a.nwg), b512(T1_THREADS);
  const bool two = a.s.L == 2 && i0 <= 128 && i1 <= 128;
  if (a.ipos) {  // several features per tower: the general kernel (any width, chunks of 128 columns)
    tower_fwd_bwd_kernel<<<g, dim3(256), 0, as_stream(stream)>>>(a);
    return check_launch("tower_fwd_bwd_indexed_multi");
  }
  if (a.mval) {  // multi-hot EBC forward fused in: compile-time shapes only
    if (two && i0 == 128 && i1 == 128 && w0 == 128 && w1 == 64)
      tower_l2_kernel<128, 128, 64, false, true><<<g, b512, 0, as_stream(stream)>>>(a);
    else if (two && i0 == 64 && i1 == 64 && w0 == 128 && w1 == 64)
      tower_l2_kernel<64, 128, 64, false, true><<<g, b512, 0, as_stream(stream)>>>(a);
    else
      return fail(TT_EINVAL, "tower_fwd_bwd_kjt: shapes in {64, 128} x [128, 64] only");
    return check_launch("tower_fwd_bwd_kjt");
  }
  if (two && a.gsrc_bf16)
    tower_l2_kernel<0, 0, 0, true><<<g, b512, 0, as_stream(stream)>>>(a);
  else if (two && i0 == 128 && i1 == 128 && w0 == 128 && w1 == 64)
    tower_l2_kernel<128, 128, 64><<<g, b512, 0, as_stream(stream)>>>(a);
  else if (two && i0 == 64 && i1 == 64 && w0 == 128 && w1 == 64)
    tower_l2_kernel<64, 128, 64><<<g, b512, 0, as_stream(stream)>>>(a);
  else if (two)
    tower_l2_kernel<0, 0, 0><<<g, b512, 0, as_stream(stream)>>>(a);
  else
    tower_fwd_bwd_kernel<<<g, dim3(256), 0, as_stream(stream)>>>(a);
  return check_launch("tower_fwd_bwd");
}

}  // namespace tt
