// bn_relu.h -- the arithmetic and the summation orders of the train-mode BatchNorm + ReLU on the (V, C) row-major feature
// matrix of a sparse tensor (bn_relu.hip), shared by the kernels and their host twins: every routine here is
// __host__ __device__, and the library is built with -ffp-contract=off, so the operations below are the operations executed,
// in this order, on either side.
//
// PINNED ORDER of the four per-channel sums (sum x, sum x^2 forward; sum dy, sum dy xhat backward).  It is a function of
// (V, C) alone: not of the grid, not of a pointer's alignment, not of which load path ran.  All of it in float64.
//
//   chunks   the V rows are cut into chunks of kBnRows = DCL_BN_ROWS rows (the last one may be short).
//   groups   the C channels are cut into groups of kBnVec = 4 adjacent channels (the last one may be short): G = ceil(C / 4).
//   slots    inside a chunk a channel has S = bn_slots(C) slots: S = 256 / min(G, 16), rounded down.  Slot s takes the chunk's
//            rows s, s + S, s + 2 S, ... ascending, each sum from +0.0:
//              a1 = a1 + (double)v;   a2 = a2 + (double)v * (double)w      (v = w = x forward; v = dy, w = xhat backward)
//            The float64 product of two floats is exact.  A slot without a row stays +0.0.
//   chunk    the S slot values are added ascending from +0.0: p = (((0 + slot 0) + slot 1) + ...) + slot S-1.
//   finish   the chunks' values are added ascending from +0.0: sum = ((0 + p_0) + p_1) + ...
// A 16-byte aligned matrix with C % 4 == 0 is read four floats at a time, any other float by float: a lane owns the same
// (slot, group) either way, so the accumulators see the same elements in the same order.  No atomics anywhere.
//
// Element-wise arithmetic, fp32, every operation rounded as written:
//   xhat = (x - mean) * invstd;  y = xhat * gamma + beta;  z = y > 0 ? y : 0   (relu = 0: z = y)
//   dy = (relu == 0 || y > 0) ? g : 0;  a = gamma * invstd;  dx = a * ((dy - mb) - xhat * mg)
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/dclnet_hip.h"

#define BN_HD __host__ __device__ __forceinline__

constexpr int kBnRows = DCL_BN_ROWS;                // rows per chunk of the sums
constexpr int kBnVec = 4;                           // channels per group = floats per vector access
constexpr int kBnThreads = 256;                     // lanes of a workgroup = (slot, group) pairs of its channel tile
constexpr int kBnTileGroups = 16;                   // groups (of four channels) per workgroup: a channel tile is 64 channels
constexpr int kBnBatch = 8;                         // sums: rows a lane loads before it adds them (geometry only, no order)
constexpr int kBnRowsPerLane = 8;                   // element-wise kernels: rows per lane (geometry only, no order)
constexpr int kBnFinCh = 8;                         // finish: channels per workgroup (geometry only)
constexpr int kBnFinBatch = 256;                    // finish: chunks staged per batch (geometry only: the order is ascending)

BN_HD bool bn_aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }
BN_HD int bn_groups(int C) { return (C + kBnVec - 1) / kBnVec; }
BN_HD int bn_tile_groups(int C) { return bn_groups(C) < kBnTileGroups ? bn_groups(C) : kBnTileGroups; }   // groups a workgroup covers
BN_HD int bn_tiles(int C) { return (bn_groups(C) + kBnTileGroups - 1) / kBnTileGroups; }
BN_HD int bn_slots(int C) { return kBnThreads / bn_tile_groups(C); }
static inline long long bn_nchunks(long long V) { return (V + kBnRows - 1) / kBnRows; }

BN_HD float bn_xhat(float x, float mean, float invstd) { return (x - mean) * invstd; }
BN_HD float bn_y(float xhat, float gamma, float beta) { return xhat * gamma + beta; }
BN_HD float bn_z(float y, int relu) { return (!relu || y > 0.0f) ? y : 0.0f; }
BN_HD float bn_dy(float y, float g, int relu) { return (!relu || y > 0.0f) ? g : 0.0f; }
BN_HD float bn_dx(float a, float dy, float mb, float xhat, float mg) { return a * ((dy - mb) - xhat * mg); }

// the per-channel constants of a group of up to four channels, loaded once per lane
struct BnGroup {
  float mean[kBnVec], invstd[kBnVec], gamma[kBnVec], beta[kBnVec];
};
BN_HD void bn_load_group(BnGroup &k, const float *mean, const float *invstd, const float *gamma, const float *beta, int c0,
                         int nch) {
#pragma unroll
  for (int q = 0; q < kBnVec; ++q) {
    const int c = q < nch ? c0 + q : c0;             // a channel that does not exist repeats the group's first: never used
    k.mean[q] = mean[c];
    k.invstd[q] = invstd[c];
    k.gamma[q] = gamma[c];
    k.beta[q] = beta[c];
  }
}

// four adjacent floats of a row: one 16-byte access, or float by float (nch < 4: the group's last channels do not exist)
template <bool VEC>
BN_HD void bn_load4(const float *p, int nch, float *v) {
  if (VEC) {
    const float4 f = *reinterpret_cast<const float4 *>(p);
    v[0] = f.x, v[1] = f.y, v[2] = f.z, v[3] = f.w;
  } else {
#pragma unroll
    for (int q = 0; q < kBnVec; ++q) v[q] = q < nch ? p[q] : 0.0f;
  }
}
template <bool VEC>
BN_HD void bn_store4(float *p, int nch, const float *v) {
  if (VEC) {
    *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int q = 0; q < kBnVec; ++q)
      if (q < nch) p[q] = v[q];
  }
}

// ---- the sums of one slot of one chunk ---------------------------------------------------------------------------------------
// xg = &x[chunk's first row][group's first channel], C the row pitch, rows s, s + S, ... < nrows; a1 / a2 continue.  kBnBatch
// rows are loaded before the first is added, so that a lane's loads are in flight together; a row beyond the chunk is read
// from the chunk's last row instead (an address that exists, no branch around the load) and is not added.  The additions
// keep the rows' ascending order: the batch is geometry only.
template <bool VEC>
BN_HD void bn_stat_slot(const float *xg, int C, int nrows, int s, int S, int nch, double *a1, double *a2) {
  for (int r = s; r < nrows; r += kBnBatch * S) {
    float v[kBnBatch][kBnVec];
#pragma unroll
    for (int u = 0; u < kBnBatch; ++u) {
      const int ru = r + u * S;
      bn_load4<VEC>(xg + (size_t)(ru < nrows ? ru : nrows - 1) * C, nch, v[u]);
    }
#pragma unroll
    for (int u = 0; u < kBnBatch; ++u) {
      const bool live = r + u * S < nrows;
#pragma unroll
      for (int q = 0; q < kBnVec; ++q) {
        const double d = (double)v[u][q];
        a1[q] = live ? a1[q] + d : a1[q];
        a2[q] = live ? a2[q] + d * d : a2[q];
      }
    }
  }
}
// the backward's: a1 += dy, a2 += dy * xhat, with y recomputed as the forward formed it (the same bits, hence the same mask)
template <bool VEC>
BN_HD void bn_bwd_slot(const float *xg, const float *gg, int C, int nrows, int s, int S, int nch, const BnGroup &k, int relu,
                       double *a1, double *a2) {
  for (int r = s; r < nrows; r += kBnBatch * S) {
    float v[kBnBatch][kBnVec], g[kBnBatch][kBnVec];
#pragma unroll
    for (int u = 0; u < kBnBatch; ++u) {
      const int ru = r + u * S;
      const size_t off = (size_t)(ru < nrows ? ru : nrows - 1) * C;
      bn_load4<VEC>(xg + off, nch, v[u]);
      bn_load4<VEC>(gg + off, nch, g[u]);
    }
#pragma unroll
    for (int u = 0; u < kBnBatch; ++u) {
      const bool live = r + u * S < nrows;
#pragma unroll
      for (int q = 0; q < kBnVec; ++q) {
        const float xh = bn_xhat(v[u][q], k.mean[q], k.invstd[q]);
        const float dy = bn_dy(bn_y(xh, k.gamma[q], k.beta[q]), g[u][q], relu);
        a1[q] = live ? a1[q] + (double)dy : a1[q];
        a2[q] = live ? a2[q] + (double)dy * (double)xh : a2[q];
      }
    }
  }
}

// values `pitch` doubles apart, added ascending onto s: the slots of a chunk and the chunks of a channel, both from +0.0
BN_HD double bn_ordered_sum_from(double s, const double *p, size_t pitch, int n) {
#pragma unroll 16
  for (int i = 0; i < n; ++i) s = s + p[(size_t)i * pitch];
  return s;
}
BN_HD double bn_ordered_sum(const double *p, size_t pitch, int n) { return bn_ordered_sum_from(0.0, p, pitch, n); }

// ---- what the finish makes of a channel's two sums ---------------------------------------------------------------------------
BN_HD void bn_finish_stats(double s1, double s2, long long V, float eps, float momentum, float *running_mean,
                           float *running_var, float *mean, float *invstd) {
  const double m = s1 / (double)V;
  double var = s2 / (double)V - m * m;
  var = var > 0.0 ? var : 0.0;                       // also turns a NaN into 0: nothing is promised for non-finite inputs
  const float mf = (float)m;
  *mean = mf;
  *invstd = (float)(1.0 / sqrt(var + (double)eps));
  if (running_mean) {
    const float unbiased = (float)(var * (double)V / (double)(V - 1));
    const float keep = 1.0f - momentum;
    *running_mean = keep * *running_mean + momentum * mf;
    *running_var = keep * *running_var + momentum * unbiased;
  }
}
BN_HD void bn_finish_bwd(double s1, double s2, long long V, float *dgamma, float *dbeta, float *mb, float *mg) {
  if (dgamma) {
    *dbeta = (float)s1;
    *dgamma = (float)s2;
  }
  *mb = (float)(s1 / (double)V);
  *mg = (float)(s2 / (double)V);
}
