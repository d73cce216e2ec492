// conf_pool_pm.h -- the summation orders of the point-major confidence pooling and its gradient (conf_pool_pm.hip), shared by
// the kernels and their host twins: every routine here is __host__ __device__, and the library is built with
// -ffp-contract=off, so the operations below are the operations executed, in this order, on either side.
//
// Per crop: F1 (n1, C), F2 (n2, C) point-major (a point's channels are contiguous), w and conf rows of L = n1 + n2 values
// (direction 1 first).
//
// PINNED ORDERS.  Each is a function of C, n1, n2 alone: not of b, not of the grid, not of a row's alignment.
//
//   pooled[c]   a sum over the points.  Each direction's rows are cut into chunks of kCppRows = DCL_POOL_PM_ROWS rows (a
//               direction's last chunk may be short; a chunk never spans both directions).  A chunk of a channel is ONE fmaf
//               chain from +0, rows ascending:
//                 p = fmaf(w[j], F[j][c], p)   for j = first row of the chunk, ..., its last row.
//               The chunks are then added ascending, F1's chunks before F2's, starting from the first chunk's value:
//               pooled = ((p_0 + p_1) + p_2) + ...   Every channel has its own chains, so four channels per lane (16-byte
//               aligned rows) and one channel per lane give the same bits.
//
//   d[j]        = sum over channels of g_pooled[c] F[j][c], a dot along the point's own row: the row has kCpgSlots = 256 slots,
//               slot k runs ONE fmaf chain from +0 over channels k, k + 256, k + 512, ... < C ascending; a lane folds its four
//               slots 4l .. 4l+3 as (s0 + s1) + (s2 + s3); the 64 lane values are folded by the butterfly with strides 32, 16,
//               ..., 1 -- the fold and the butterfly of the channel-major pooling (conf_pool_grad.h).  An aligned row is read
//               four floats at a time, any other float by float: the slots see the same elements in the same order.
//
//   dot, ds[j], dlogit[j]   conf_pool_grad.h's, by its routines (cpg_dot_lane, the 256-lane tree, cpg_dlogit).
//   dF[j][c]    = g_pooled[c] * w[j]
// No atomics anywhere.
#pragma once
#include "conf_pool_grad.h"

#ifndef DCL_POOL_PM_ROWS
#define DCL_POOL_PM_ROWS 64                         // -DDCL_POOL_PM_ROWS=n: another build to measure against (tools/bench_conf_pool_pm.py --lib)
#endif
constexpr int kCppRows = DCL_POOL_PM_ROWS;          // rows per fmaf chain of pooled
constexpr int kCppColLanes = 16;                    // lanes across one chunk's columns (geometry only, no order)
constexpr int kCppCols = kCppColLanes * kCpgVec;    // 64 channels per workgroup of the pooling
constexpr int kCppGroups = 64;                      // chunks a workgroup of the pooling works on at a time (geometry only)

CPG_HD int cpp_nchunks(int n) { return (n + kCppRows - 1) / kCppRows; }

// ---- pooled: one chunk's chain of one channel ----------------------------------------------------------------------------------
// Fcol = &F[j0][c] of the crop's direction, C its row pitch, w = &w[j0] of the direction's block; rows j0 .. j0 + rows - 1
CPG_HD float cpp_pool_chain(const float *Fcol, size_t C, const float *w, int rows) {
  float acc = 0.0f;
#pragma unroll 8
  for (int r = 0; r < rows; ++r) acc = fmaf(w[r], Fcol[(size_t)r * C], acc);
  return acc;
}
// the same chains for four adjacent channels of 16-byte aligned rows
CPG_HD void cpp_pool_chain4(const float *Fcol, size_t C, const float *w, int rows, float *acc) {
  acc[0] = acc[1] = acc[2] = acc[3] = 0.0f;
#pragma unroll 8
  for (int r = 0; r < rows; ++r) {
    const float4 f = *reinterpret_cast<const float4 *>(Fcol + (size_t)r * C);
    const float wr = w[r];
    acc[0] = fmaf(wr, f.x, acc[0]);
    acc[1] = fmaf(wr, f.y, acc[1]);
    acc[2] = fmaf(wr, f.z, acc[2]);
    acc[3] = fmaf(wr, f.w, acc[3]);
  }
}

// chunk q of a crop (q counts F1's chunks, then F2's): its direction, first row and length
struct CppChunk {
  int dir, j0, rows;
};
CPG_HD CppChunk cpp_chunk(int q, int n1, int n2) {
  const int q1 = cpp_nchunks(n1);
  CppChunk k;
  k.dir = q >= q1;
  k.j0 = (k.dir ? q - q1 : q) * kCppRows;
  const int n = k.dir ? n2 : n1;
  k.rows = n - k.j0 < kCppRows ? n - k.j0 : kCppRows;
  return k;
}

// ---- d: lane `lane`'s four slots of one row's dot with g ------------------------------------------------------------------------
// F: the row (C floats), g: the crop's g_pooled.  VEC: four floats at a time (both pointers 16-byte aligned, C % 4 == 0).
template <bool VEC>
CPG_HD void cpp_dot_lane(const float *F, const float *g, int C, int lane, float *acc) {
  acc[0] = acc[1] = acc[2] = acc[3] = 0.0f;
  if (VEC) {
#pragma unroll 4
    for (int c = kCpgVec * lane; c < C; c += kCpgSlots) {
      const float4 f = *reinterpret_cast<const float4 *>(F + c);
      const float4 x = *reinterpret_cast<const float4 *>(g + c);
      acc[0] = fmaf(x.x, f.x, acc[0]);
      acc[1] = fmaf(x.y, f.y, acc[1]);
      acc[2] = fmaf(x.z, f.z, acc[2]);
      acc[3] = fmaf(x.w, f.w, acc[3]);
    }
  } else {
    for (int c = kCpgVec * lane; c < C; c += kCpgSlots) {
#pragma unroll
      for (int q = 0; q < kCpgVec; ++q)
        if (c + q < C) acc[q] = fmaf(g[c + q], F[c + q], acc[q]);
    }
  }
}
