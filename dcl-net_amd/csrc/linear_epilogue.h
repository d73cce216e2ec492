// linear_epilogue.h -- the epilogues that the two GEMM cores (linear_dma.hip: fp32 MFMA; linear_split.hip: split bf16) share.
// A wave holds MB x NB accumulator blocks of 32 x 32 (mfma_tile.h: rowmap); `a` is the core's argument struct (LinDmaArgs /
// LinSplitArgs: the epilogue fields have the same names in both); (r, h) = (lane & 31, lane >> 5).  What differs between
// the cores -- barriers, the sum over waves, where a row's dot product goes -- stays in the kernels.
#pragma once
#include "mfma_tile.h"

namespace {

// EPI 0:  y = act(acc + bias).  wrow0 / wcol0: the wave's first row / column of y; whole (workgroup-uniform): an interior tile,
// no per-element checks.  NT: non-temporal stores on the whole-tile path.
template <bool NT, int MB, int NB, class Args>
__device__ __forceinline__ void lin_epi_store(const f32x16 (&acc)[MB][NB], const Args &a, bool whole, int wrow0, int wcol0, int r, int h) {
  float *__restrict__ y = a.y;
  float bias[NB];
#pragma unroll
  for (int n = 0; n < NB; ++n) {
    const int co = wcol0 + n * 32 + r;
    bias[n] = (a.bias && co < a.N) ? a.bias[co] : 0.0f;
  }
  if (whole) {
#pragma unroll
    for (int m = 0; m < MB; ++m)
#pragma unroll
      for (int n = 0; n < NB; ++n) {
        float *yp = y + (size_t)(wrow0 + m * 32 + 4 * h) * a.ldy + (wcol0 + n * 32 + r);
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          float v = acc[m][n][e] + bias[n];
          if (a.relu) v = fmaxf(v, 0.0f);
          if constexpr (NT) __builtin_nontemporal_store(v, yp + (size_t)rowmap(e, 0) * a.ldy);
          else yp[(size_t)rowmap(e, 0) * a.ldy] = v;
        }
      }
  } else {
#pragma unroll
    for (int m = 0; m < MB; ++m)
#pragma unroll
      for (int n = 0; n < NB; ++n) {
        const int co = wcol0 + n * 32 + r;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int orow = wrow0 + m * 32 + rowmap(e, h);
          float v = acc[m][n][e] + bias[n];
          if (a.relu) v = fmaxf(v, 0.0f);
          if (orow < a.M && co < a.N) y[(size_t)orow * a.ldy + co] = v;
        }
      }
  }
}

// EPI 4 (split core):  y = act(acc + bias + sum over the folded levels l, ascending, and i = 0, 1, 2 of fw[l][row][i] * G_l[fi[l][row][i]][col])
// -- one fmaf chain per output in exactly that order, so the bits are the same on every run.  The read-out's deep levels enter the
// first disengage layer this way: G_l = F_l W[col_l ...] has a few thousand rows (a few hundred per crop: they stay in the L2 of
// the XCD that owns the row block), and three fused multiply-adds on its rows replace the level's K columns of the big GEMM.
// rw: the wave's 64 rows x kFoldMax levels x 8 dwords in LDS, {w0, w1, w2, -, i0, i1, i2, -} per row and level (staged by the
// kernel).  A row's weights and indices are uniform over a lane half: LDS broadcasts; a load covers 128 contiguous bytes of one row
// of G_l per lane half, the shape of the stores.
// The loads are what the epilogue waits for (a row's twelve per level, issued and awaited row by row, made it a chain of 64 L2
// round trips per tile), so it is a software pipeline in straight-line code: a step = 24 loads (one row of two levels, two rows of
// one), the next step's loads are issued before this step's sums and stores, and nothing is predicated -- NFOLD and WHOLE are
// template arguments, and a ragged tile loads from its last valid column (rows >= M carry a valid row's indices) and only
// predicates its stores.
constexpr int kFoldMax = 2;
template <bool NT, int NFOLD, bool WHOLE, int MB, int NB, class Args>
__device__ __forceinline__ void lin_epi_gather_store(const f32x16 (&acc)[MB][NB], const Args &a, const float *rw, int wrow0, int wcol0,
                                                     int r, int h) {
  static_assert(NFOLD >= 1 && NFOLD <= kFoldMax, "folded levels");
  constexpr int RS = NFOLD == 1 ? 2 : 1, STEPS = MB * 16 / RS;             // rows per step; steps
  float *__restrict__ y = a.y;
  float bias[NB];
  int gcol[NB];
  bool cok[NB];
#pragma unroll
  for (int n = 0; n < NB; ++n) {
    const int co = wcol0 + n * 32 + r;
    cok[n] = WHOLE || co < a.N;
    bias[n] = (a.bias && cok[n]) ? a.bias[co] : 0.0f;
    gcol[n] = WHOLE ? co : min(co, a.N - 1);
  }
  float q[2][RS][NFOLD][3][NB], wq[2][RS][NFOLD][3];
  auto fetch = [&](int s, int buf) {
#pragma unroll
    for (int j = 0; j < RS; ++j) {
      const int t = s * RS + j, rl = (t >> 4) * 32 + rowmap(t & 15, h);
#pragma unroll
      for (int l = 0; l < NFOLD; ++l) {
        const float4 w4 = *reinterpret_cast<const float4 *>(rw + (l * 64 + rl) * 8);
        const int4 i4 = *reinterpret_cast<const int4 *>(rw + (l * 64 + rl) * 8 + 4);
        const int rows3[3] = {i4.x, i4.y, i4.z};
        wq[buf][j][l][0] = w4.x; wq[buf][j][l][1] = w4.y; wq[buf][j][l][2] = w4.z;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          const float *__restrict__ g = a.G[l] + (size_t)rows3[i] * a.ldg[l];
#pragma unroll
          for (int n = 0; n < NB; ++n) q[buf][j][l][i][n] = g[gcol[n]];
        }
      }
    }
  };
  fetch(0, 0);
#pragma unroll
  for (int s = 0; s < STEPS; ++s) {
    if (s + 1 < STEPS) fetch(s + 1, (s + 1) & 1);
#pragma unroll
    for (int j = 0; j < RS; ++j) {
      const int t = s * RS + j, m = t >> 4, e = t & 15;
      const int orow = wrow0 + m * 32 + rowmap(e, h);
#pragma unroll
      for (int n = 0; n < NB; ++n) {
        float v = acc[m][n][e] + bias[n];
#pragma unroll
        for (int l = 0; l < NFOLD; ++l)
#pragma unroll
          for (int i = 0; i < 3; ++i) v = __fmaf_rn(wq[s & 1][j][l][i], q[s & 1][j][l][i][n], v);
        if (a.relu) v = fmaxf(v, 0.0f);
        float *yp = y + (size_t)orow * a.ldy + (wcol0 + n * 32 + r);
        if constexpr (WHOLE) {
          if constexpr (NT) __builtin_nontemporal_store(v, yp);
          else *yp = v;
        } else {
          if (orow < a.M && cok[n]) *yp = v;
        }
      }
    }
  }
}

// EPI 1:  a wave's weighted column sums  sum over its 32 MB rows j of  w[j] * act(acc[j][c] + bias[c])  -- in registers, one
// fmaf chain per lane half over its rows in register order, then half 0 + half 1 -- written by lane half 0 to red_row[column
// inside the tile].  wts: the tile's row weights in LDS; wrow / wcol: the wave's first row / column INSIDE the tile; col0: the
// tile's first column.  (The kernel adds the waves of a column in wave order behind a barrier.)
template <int MB, int NB, class Args>
__device__ __forceinline__ void lin_epi_colsum(const f32x16 (&acc)[MB][NB], const Args &a, const float *wts, float *red_row, int wrow,
                                               int col0, int wcol, int r, int h) {
  const float *wl = wts + wrow + 4 * h;
#pragma unroll
  for (int n = 0; n < NB; ++n) {
    const int cl = wcol + n * 32 + r, co = col0 + cl;
    const float bias = (a.bias && co < a.N) ? a.bias[co] : 0.0f;
    float s = 0.0f;
#pragma unroll
    for (int m = 0; m < MB; ++m)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const float4 w4 = *reinterpret_cast<const float4 *>(wl + m * 32 + 8 * g4);    // rows 8 g4 + 4 h + 0..3 = e 4 g4 .. + 3
        const float wv[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float v = acc[m][n][4 * g4 + j] + bias;
          if (a.relu) v = fmaxf(v, 0.0f);
          s = __fmaf_rn(v, wv[j], s);
        }
      }
    s += __shfl_xor(s, 32, 64);
    if (h == 0) red_row[cl] = s;
  }
}

// EPI 2:  row dot (the confidence regressor's last two layers, models/DCL_Net.py:115-126: ... -> 128 -> 1):
//     sum_c relu(acc[row][c] + bias[c]) * w3[c]
// per lane an fmaf chain over its column blocks, then a butterfly over the 32 lanes of a half wave; every lane of the half
// ends with the sum and calls row_value(row, sum).  wrow0: the wave's first row, in the numbering row_value wants; wcol0: the
// wave's first column of the layer.
template <int MB, int NB, class Args, class F>
__device__ __forceinline__ void lin_epi_rowdot(const f32x16 (&acc)[MB][NB], const Args &a, int wrow0, int wcol0, int r, int h, F &&row_value) {
  float w3c[NB], bias[NB];
#pragma unroll
  for (int n = 0; n < NB; ++n) {
    const int co = wcol0 + n * 32 + r;
    bias[n] = (a.bias && co < a.N) ? a.bias[co] : 0.0f;
    w3c[n] = co < a.N ? a.roww[(size_t)co * a.w_stride] : 0.0f;
  }
#pragma unroll
  for (int m = 0; m < MB; ++m)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      float sdot = 0.0f;
#pragma unroll
      for (int n = 0; n < NB; ++n) sdot = __fmaf_rn(fmaxf(acc[m][n][e] + bias[n], 0.0f), w3c[n], sdot);
#pragma unroll
      for (int d = 16; d >= 1; d >>= 1) sdot += __shfl_xor(sdot, d, 64);
      row_value(wrow0 + m * 32 + rowmap(e, h), sdot);
    }
}

}  // namespace
