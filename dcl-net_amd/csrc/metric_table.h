// metric_table.h -- what the ADD(-S) distance kernels (metric.hip, metric_table.hip) and the evaluation tables' update
// (metric_table.hip and its host twin metric_table_host.cpp) share: the per-(pose, object) arithmetic of a 256-point slice,
// and ONE crop's step of a table -- so the trajectory kernel has dcl_add_s's bits and the device table the host twin's.
#pragma once
#include "common.h"
#include <math.h>

// -------------------------------------------------------------------------------------------- one crop into one table entry
// The entries class c owns at step t, in registers (the kernel) or locals (the twin).
struct DclTableAcc {
  double n, m, sd, c2, mx;        // DCL_TABLE_ADDS: sums[t][c][0..3], maxd[t][c]
  int64_t num, suc;               // DCL_TABLE_LM / _LMO: counts[t][c][0..1]
};

// include/dclnet_hip.h pins this: every comparison in double on the exactly converted fp32 distance; NaN / inf take the
// branches the comparisons take; valid == 0 is AddsTable.add(c, inf) / dropped (LM) / LmoTable.add_lost.  A row with
// valid < 0 is not a crop (padding): the callers skip it before this step, so `valid` here is valid > 0.
__host__ __device__ inline void dcl_table_step(int mode, bool valid, float df, double diam, DclTableAcc &a) {
  const double d = (double)df;
  if (mode == DCL_TABLE_ADDS) {
    a.n += 1.0;
    if (!valid) return;
    if (d <= 0.1) {
      a.m += 1.0;
      a.sd += d;
      a.mx = d > a.mx ? d : a.mx;
    }
    if (d < 0.02) a.c2 += 1.0;
    return;
  }
  if (!valid) {
    if (mode == DCL_TABLE_LMO) a.num += 1;
    return;
  }
  a.num += 1;
  if (d < diam) a.suc += 1;
}

__host__ __device__ inline void dcl_table_load(int mode, size_t e, const double *sums, const double *maxd, const int64_t *counts,
                                               DclTableAcc &a) {
  a.n = a.m = a.sd = a.c2 = a.mx = 0.0;
  a.num = a.suc = 0;
  if (mode == DCL_TABLE_ADDS) {
    a.n = sums[e * 4]; a.m = sums[e * 4 + 1]; a.sd = sums[e * 4 + 2]; a.c2 = sums[e * 4 + 3];
    a.mx = maxd[e];
  } else {
    a.num = counts[e * 2]; a.suc = counts[e * 2 + 1];
  }
}

__host__ __device__ inline void dcl_table_store(int mode, size_t e, const DclTableAcc &a, double *sums, double *maxd,
                                                int64_t *counts) {
  if (mode == DCL_TABLE_ADDS) {
    sums[e * 4] = a.n; sums[e * 4 + 1] = a.m; sums[e * 4 + 2] = a.sd; sums[e * 4 + 3] = a.c2;
    maxd[e] = a.mx;
  } else {
    counts[e * 2] = a.num; counts[e * 2 + 1] = a.suc;
  }
}

// the refusals both tabulation entries make before any work
#define DCL_TABLE_CHECK_ARGS()                                                                                          \
  do {                                                                                                                  \
    DCL_CHECK_ARG(mode == DCL_TABLE_ADDS || mode == DCL_TABLE_LM || mode == DCL_TABLE_LMO);                             \
    DCL_CHECK_ARG(T >= 1 && b >= 0 && C >= 1 && C <= (1 << 20));                                                        \
    DCL_CHECK_ARG(bad && (mode == DCL_TABLE_ADDS ? (sums && maxd) : (counts && diameter)));                             \
  } while (0)

// ------------------------------------------------------------------------------------------ a 256-point slice of one object
#if defined(__HIPCC__)
__device__ __forceinline__ void adds_pose_point(const float *R, const float *t, float x, float y, float z, float &ox, float &oy,
                                                float &oz) {
  // row-vector form of bmm(cld, R^T) + t: out[c] = x*R[c][0] + y*R[c][1] + z*R[c][2] + t[c]
  ox = __fmaf_rn(z, R[2], __fmaf_rn(y, R[1], x * R[0])) + t[0];
  oy = __fmaf_rn(z, R[5], __fmaf_rn(y, R[4], x * R[3])) + t[1];
  oz = __fmaf_rn(z, R[8], __fmaf_rn(y, R[7], x * R[6])) + t[2];
}

// the object's cloud posed by the ground truth into LDS gt[P][3] (the caller's barrier follows)
__device__ __forceinline__ void adds_stage_gt(int P, const float *C, const float *R2, const float *t2, float *gt, int tid) {
  for (int j = tid; j < P; j += 256) {
    float x, y, z;
    adds_pose_point(R2, t2, C[j * 3], C[j * 3 + 1], C[j * 3 + 2], x, y, z);
    gt[j * 3] = x; gt[j * 3 + 1] = y; gt[j * 3 + 2] = z;
  }
}

// the slice's sums of point distances under NP poses at once: pose k is (R1 + k * sR, t1 + k * st); lane tid holds point
// i = slice * 256 + tid.  The NP poses share every read of the staged cloud and run as NP independent minimum chains; each
// chain is the one-pose arithmetic in the one-pose order, so a pose's sum does not depend on NP.  All 256 lanes call it; the
// results are the workgroup's sums on lane 0.  red[4 * NP] is reused by the next call: a barrier goes between two calls.
template <int NP>
__device__ __forceinline__ void adds_slice_sums(int P, int i, const float *C, const float *R1, const float *t1, size_t sR, size_t st,
                                                const float *gt, bool nearest, float *red, int tid, float (&sum)[NP]) {
  float best[NP];
#pragma unroll
  for (int k = 0; k < NP; ++k) best[k] = 0.0f;
  if (i < P) {
    const float cx = C[i * 3], cy = C[i * 3 + 1], cz = C[i * 3 + 2];
    float px[NP], py[NP], pz[NP], m[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) {
      adds_pose_point(R1 + k * sR, t1 + k * st, cx, cy, cz, px[k], py[k], pz[k]);
      m[k] = INFINITY;
    }
    if (nearest) {                                                    // ADD-S: nearest gt point; ADD: the corresponding one
      for (int j = 0; j < P; ++j) {
        const float gx = gt[j * 3], gy = gt[j * 3 + 1], gz = gt[j * 3 + 2];
#pragma unroll
        for (int k = 0; k < NP; ++k) {
          const float dx = px[k] - gx, dy = py[k] - gy, dz = pz[k] - gz;
          m[k] = fminf(m[k], __fmaf_rn(dz, dz, __fmaf_rn(dy, dy, dx * dx)));
        }
      }
    } else {
      const float gx = gt[i * 3], gy = gt[i * 3 + 1], gz = gt[i * 3 + 2];
#pragma unroll
      for (int k = 0; k < NP; ++k) {
        const float dx = px[k] - gx, dy = py[k] - gy, dz = pz[k] - gz;
        m[k] = __fmaf_rn(dz, dz, __fmaf_rn(dy, dy, dx * dx));
      }
    }
#pragma unroll
    for (int k = 0; k < NP; ++k) best[k] = sqrtf(m[k]);
  }
#pragma unroll
  for (int k = 0; k < NP; ++k) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) best[k] += __shfl_xor(best[k], d, 64);
    if ((tid & 63) == 0) red[k * 4 + (tid >> 6)] = best[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NP; ++k) sum[k] = (red[k * 4] + red[k * 4 + 1]) + (red[k * 4 + 2] + red[k * 4 + 3]);
}
#endif
