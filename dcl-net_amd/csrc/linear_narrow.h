// linear_narrow.h -- the summation orders of the narrow per-point layer and its gradients (linear_narrow.hip), shared by the
// kernels and their host twins: every routine here is __host__ __device__, and the library is built with -ffp-contract=off,
// so the operations below are the operations executed, in this order, on either side.
//
// x (M, K) with a row pitch, W (N, K) as the convolution registers it, g and y (M, N) dense, N <= kLnMaxN.
//
// PINNED ORDERS.  Each is a function of (M, K, N) alone: not of the grid, of x's pitch or of a pointer's alignment.
//
//   y[m][j]     a dot along the row.  The row has kLnSlots = 64 slots, slot k = 4 l + e of lane l < 16.  Slot k runs ONE fmaf
//               chain from +0 over the columns k, k + 64, k + 128, ... < K ascending:
//                 s = fmaf(x[m][c], W[j][c], s).
//               A column that does not exist adds nothing.  A lane folds its four slots as (s0 + s1) + (s2 + s3); the 16 lane
//               values are folded by a butterfly with strides 8, 4, 2, 1 (v[l] = v[l] + v[l ^ stride], all lanes at once);
//               y = v + bias[j] when there is a bias.  Every output j has its own slots: x is read once for all N of them.
//
//   dx[m][k]    ONE fmaf chain from +0 over the outputs, j ascending:  d = fmaf(g[m][j], W[j][k], d).
//
//   dW[j][k]    the rows are cut into chunks of kLnRows = DCL_NARROW_ROWS rows (the last may be short).  A chunk of an element is
//               ONE fmaf chain from +0, rows ascending:  p = fmaf(g[m][j], x[m][k], p).  The chunks are then added ascending,
//               starting from the first chunk's value:  dW = ((p_0 + p_1) + p_2) + ...
//   db[j]       the same chunks; inside a chunk p = p + g[m][j] from +0, rows ascending; the chunks as for dW.
//
// Every element of dx, dW and db has its own chain, so four columns per lane (16-byte accesses) and one float at a time give
// the same bits.  No atomics anywhere.
#pragma once
#include "conf_pool_grad.h"                          // CPG_HD, cpg_aligned16

constexpr int kLnMaxN = DCL_NARROW_MAX_N;            // widest layer served
constexpr int kLnRows = DCL_NARROW_ROWS;             // rows per fmaf chain of dW / db
constexpr int kLnLanes = 16;                         // lanes per row of the forward dot
constexpr int kLnVec = 4;                            // slots per lane = floats per vector access
constexpr int kLnSlots = kLnLanes * kLnVec;          // 64 slots per row

// four adjacent floats at p, of which `have` exist (the others read as +0 and feed chains that are never stored).
// VEC: one 16-byte access (p aligned, have >= 4).
template <bool VEC>
CPG_HD float4 ln_load4(const float *p, int have) {
  if (VEC) return *reinterpret_cast<const float4 *>(p);
  float4 v;
  v.x = have > 0 ? p[0] : 0.0f;
  v.y = have > 1 ? p[1] : 0.0f;
  v.z = have > 2 ? p[2] : 0.0f;
  v.w = have > 3 ? p[3] : 0.0f;
  return v;
}
template <bool VEC>
CPG_HD void ln_store4(float *p, int have, float4 v) {
  if (VEC) {
    *reinterpret_cast<float4 *>(p) = v;
    return;
  }
  if (have > 0) p[0] = v.x;
  if (have > 1) p[1] = v.y;
  if (have > 2) p[2] = v.z;
  if (have > 3) p[3] = v.w;
}

// ---- y: lane `lane`'s four slots of one row against each of the N weight rows -----------------------------------------------
// x: the row (K floats), W (N, K); acc[j][e]: slot 4 lane + e of output j.  NMAX >= N bounds the unrolled loop over the outputs.
template <bool VEC, int NMAX>
CPG_HD void ln_row_lane(const float *x, const float *W, int K, int N, int lane, float (*acc)[kLnVec]) {
#pragma unroll
  for (int j = 0; j < NMAX; ++j) acc[j][0] = acc[j][1] = acc[j][2] = acc[j][3] = 0.0f;
  for (int c = kLnVec * lane; c < K; c += kLnSlots) {
    const int have = K - c;
    const float4 a = ln_load4<VEC>(x + c, have);
#pragma unroll
    for (int j = 0; j < NMAX; ++j)
      if (j < N) {
        const float4 w = ln_load4<VEC>(W + (size_t)j * K + c, have);
        acc[j][0] = fmaf(a.x, w.x, acc[j][0]);
        if (have > 1) acc[j][1] = fmaf(a.y, w.y, acc[j][1]);
        if (have > 2) acc[j][2] = fmaf(a.z, w.z, acc[j][2]);
        if (have > 3) acc[j][3] = fmaf(a.w, w.w, acc[j][3]);
      }
  }
}
CPG_HD float ln_lane_fold(const float *acc) { return (acc[0] + acc[1]) + (acc[2] + acc[3]); }
// the butterfly over the 16 lane values, as the kernel's shuffles run it
inline float ln_butterfly_host(float *v) {
  for (int s = kLnLanes / 2; s >= 1; s >>= 1) {
    float t[kLnLanes];
    for (int l = 0; l < kLnLanes; ++l) t[l] = v[l] + v[l ^ s];
    for (int l = 0; l < kLnLanes; ++l) v[l] = t[l];
  }
  return v[0];
}

// ---- dx, dW, db: one thread's share of one chunk ---------------------------------------------------------------------------------
// The thread owns the columns k .. k + 3 (`have` of them exist) of the rows m0 .. m0 + rows - 1.  dx (dense, pitch K) gets its
// rows' elements; pw[j] and pb[j] get the chunk's partial of dW[j][k ..] and (first column only) db[j].  dx NULL: not written;
// sums == false: the partials are not formed.
template <bool VEC, int NMAX>
CPG_HD void ln_bwd_chunk(const float *x, long long pitch, const float *W, const float *g, int K, int N, long long m0, int rows, int k,
                         float *dx, bool sums, float4 *pw, float *pb) {
  const int have = K - k;
  constexpr int kInFlight = NMAX <= 4 ? 16 : 4;
  float4 w[NMAX];
#pragma unroll
  for (int j = 0; j < NMAX; ++j) {
    w[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (j < N && dx) w[j] = ln_load4<VEC>(W + (size_t)j * K + k, have);
    pw[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    pb[j] = 0.0f;
  }
  // kInFlight rows at a time: their loads are all issued before the first store, since a chunk is walked by one thread and only
  // its own loads overlap (the rows' chains are continued in row order all the same)
  for (int r0 = 0; r0 < rows; r0 += kInFlight) {
    float4 a[kInFlight];
    float gv[kInFlight][NMAX];
#pragma unroll
    for (int u = 0; u < kInFlight; ++u) {
      const bool live = r0 + u < rows;
      const size_t m = (size_t)(m0 + r0 + (live ? u : 0));
#pragma unroll
      for (int j = 0; j < NMAX; ++j) gv[u][j] = live && j < N ? g[m * N + j] : 0.0f;
      a[u] = live && sums ? ln_load4<VEC>(x + m * (size_t)pitch + k, have) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < kInFlight; ++u) {
      const bool live = r0 + u < rows;
      const size_t m = (size_t)(m0 + r0 + u);
      if (live && dx) {
        float4 d = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int j = 0; j < NMAX; ++j)
          if (j < N) {
            d.x = fmaf(gv[u][j], w[j].x, d.x);
            d.y = fmaf(gv[u][j], w[j].y, d.y);
            d.z = fmaf(gv[u][j], w[j].z, d.z);
            d.w = fmaf(gv[u][j], w[j].w, d.w);
          }
        ln_store4<VEC>(dx + m * K + k, have, d);
      }
      if (live && sums) {
#pragma unroll
        for (int j = 0; j < NMAX; ++j)
          if (j < N) {
            pw[j].x = fmaf(gv[u][j], a[u].x, pw[j].x);
            pw[j].y = fmaf(gv[u][j], a[u].y, pw[j].y);
            pw[j].z = fmaf(gv[u][j], a[u].z, pw[j].z);
            pw[j].w = fmaf(gv[u][j], a[u].w, pw[j].w);
            pb[j] = pb[j] + gv[u][j];
          }
      }
    }
  }
}

CPG_HD long long ln_nchunks(long long M) { return (M + kLnRows - 1) / kLnRows; }
// one chunk's partials: dW (N K floats) then db (N floats), padded to whole 16-byte vectors
CPG_HD long long ln_part_floats(int K, int N) { return ((long long)N * K + N + 3) / 4 * 4; }
