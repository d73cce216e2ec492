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
