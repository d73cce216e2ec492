// conf_pool_grad.h -- the summation orders of the channel-major confidence pooling and its gradient (conf_pool_grad.hip),
// shared by the kernels and their host twins: every routine here is __host__ __device__, and the library is built with
// -ffp-contract=off, so the operations below are the operations executed, in this order, on either side.
//
// Per crop: F1 (C, n1), F2 (C, n2) channel-major, w and conf rows of L = n1 + n2 values (direction 1 first).
//
// PINNED ORDERS.  Each is a function of C, n1, n2 alone: not of b, not of the grid, not of a row's alignment.
//
//   pooled[c]   one wave of kCpgLanes = 64 lanes per (crop, channel) row; lane l owns kCpgVec = 4 accumulators, so a row has
//               kCpgSlots = 256 slots, slot k = 4 l + q.  Slot k runs ONE fmaf chain from +0:
//                 slot = fmaf(w[j], F1[c][j], slot)       for j = k, k + 256, k + 512, ... < n1 ascending, then
//                 slot = fmaf(w[n1 + j], F2[c][j], slot)  for j = k, k + 256, ...          < n2 ascending.
//               An element that does not exist adds nothing (no fmaf of zeros).  A lane folds its four slots as
//               (s0 + s1) + (s2 + s3); the 64 lane values are folded by a butterfly with strides 32, 16, ..., 1
//               (v[l] = v[l] + v[l ^ stride], all lanes at once).  A 16-byte aligned row is read four floats at a time, any
//               other row float by float: the slots see the same elements in the same order either way.
//
//   d[j]        = sum over channels of g_pooled[c] F[c][j].  The channels are cut into chunks of kCpgChunk = 256 (the last one
//               may be short).  Chunk q of column j is ONE fmaf chain from +0, channels ascending:
//                 p_q = fmaf(g_pooled[c], F[c][j], p_q)   for c = 256 q, ..., min(256 q + 255, C - 1).
//               The chunks are then added ascending, starting from chunk 0's value: d = ((p_0 + p_1) + p_2) + ...
//               Every column has its own chains, so four columns per lane (aligned rows) and one column per lane give the
//               same bits.
//
//   dot         = sum over j of w[j] d[j]: kCpgDotLanes = 256 lanes per crop; lane l runs acc = fmaf(w[j], d[j], acc) from +0
//               for j = l, l + 256, ... < L ascending; the 256 accumulators are folded by a tree with strides 128, 64, ..., 1
//               (slot l += slot l + stride for l < stride).
//
//   ds[j]       = fmaf(w[j], d[j] - dot, g_conf[j])   (g_conf NULL: w[j] * (d[j] - dot))
//   dlogit[j]   = (ds[j] * s) * (1 - s),  s = conf[j]
//   dF[c][j]    = g_pooled[c] * w[j]
// No atomics anywhere.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#define CPG_HD __host__ __device__ __forceinline__

constexpr int kCpgLanes = 64;                       // lanes per row of the pooling
constexpr int kCpgVec = 4;                          // accumulators per lane = floats per vector access
constexpr int kCpgSlots = kCpgLanes * kCpgVec;      // 256 slots per row
#ifndef DCL_CPG_CHUNK
#define DCL_CPG_CHUNK 256                           // -DDCL_CPG_CHUNK=n: another build to measure against (tools/bench_conf_pool.py --lib)
#endif
constexpr int kCpgChunk = DCL_CPG_CHUNK;            // channels per fmaf chain of d
constexpr int kCpgDotLanes = 256;                   // lanes of the per-crop dot
constexpr int kCpgTile = 256 * kCpgVec;             // columns per workgroup of the d / dF kernels (geometry only, no order)

CPG_HD bool cpg_aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// ---- pooled: lane `lane`'s share of one direction of one row, continued on acc[4] -------------------------------------------
// F: the row (n floats), w: the direction's block of the crop's weights.  VEC: take whole 256-column blocks four floats at a
// time (both pointers 16-byte aligned); the last, partial block is always taken float by float.
template <bool VEC>
CPG_HD void cpg_pool_lane(const float *F, const float *w, int n, int lane, float *acc) {
  const int nfull = n / kCpgSlots * kCpgSlots;
  int j = kCpgVec * lane;
  if (VEC) {
#pragma unroll 4
    for (; j < nfull; j += kCpgSlots) {
      const float4 f = *reinterpret_cast<const float4 *>(F + j);
      const float4 x = *reinterpret_cast<const float4 *>(w + j);
      acc[0] = fmaf(x.x, f.x, acc[0]);
      acc[1] = fmaf(x.y, f.y, acc[1]);
      acc[2] = fmaf(x.z, f.z, acc[2]);
      acc[3] = fmaf(x.w, f.w, acc[3]);
    }
  } else {
#pragma unroll 4
    for (; j < nfull; j += kCpgSlots) {
#pragma unroll
      for (int q = 0; q < kCpgVec; ++q) acc[q] = fmaf(w[j + q], F[j + q], acc[q]);
    }
  }
#pragma unroll
  for (int q = 0; q < kCpgVec; ++q)
    if (j + q < n) acc[q] = fmaf(w[j + q], F[j + q], acc[q]);
}

CPG_HD float cpg_pool_lane_fold(const float *acc) { return (acc[0] + acc[1]) + (acc[2] + acc[3]); }

// the host's copy of the butterfly over the 64 lane values (the kernel does it with cross-lane moves)
inline float cpg_pool_butterfly_host(float *v) {
  float t[kCpgLanes];
  for (int s = kCpgLanes / 2; s >= 1; s >>= 1) {
    for (int l = 0; l < kCpgLanes; ++l) t[l] = v[l] + v[l ^ s];
    for (int l = 0; l < kCpgLanes; ++l) v[l] = t[l];
  }
  return v[0];
}

// ---- d: one chunk's chain of one column ---------------------------------------------------------------------------------------
// Fcol = &F[c0][j] of the crop's direction, n its row pitch, g the crop's g_pooled; channels c0 .. c1 - 1
CPG_HD float cpg_d_chain(const float *Fcol, size_t n, const float *g, int c0, int c1) {
  float acc = 0.0f;
#pragma unroll 8
  for (int c = c0; c < c1; ++c) acc = fmaf(g[c], Fcol[(size_t)(c - c0) * n], acc);
  return acc;
}
// the same chains for four adjacent columns of 16-byte aligned rows
CPG_HD void cpg_d_chain4(const float *Fcol, size_t n, const float *g, int c0, int c1, float *acc) {
  acc[0] = acc[1] = acc[2] = acc[3] = 0.0f;
#pragma unroll 8
  for (int c = c0; c < c1; ++c) {
    const float4 f = *reinterpret_cast<const float4 *>(Fcol + (size_t)(c - c0) * n);
    const float gc = g[c];
    acc[0] = fmaf(gc, f.x, acc[0]);
    acc[1] = fmaf(gc, f.y, acc[1]);
    acc[2] = fmaf(gc, f.z, acc[2]);
    acc[3] = fmaf(gc, f.w, acc[3]);
  }
}

// chunks added ascending, from chunk 0's value; part = &partial[chunk 0][j], pitch = floats between chunks
CPG_HD float cpg_d_fold(const float *part, size_t pitch, int nchunks) {
  float d = part[0];
#pragma unroll 8
  for (int q = 1; q < nchunks; ++q) d = d + part[(size_t)q * pitch];
  return d;
}

// ---- dot, ds, dlogit ----------------------------------------------------------------------------------------------------------
CPG_HD float cpg_dot_lane(const float *w, const float *d, int L, int lane) {
  float acc = 0.0f;
#pragma unroll 8
  for (int j = lane; j < L; j += kCpgDotLanes) acc = fmaf(w[j], d[j], acc);
  return acc;
}

inline float cpg_dot_tree_host(float *slot) {
  for (int s = kCpgDotLanes / 2; s >= 1; s >>= 1)
    for (int l = 0; l < s; ++l) slot[l] += slot[l + s];
  return slot[0];
}

CPG_HD float cpg_dlogit(float w, float d, float dot, const float *g_conf_j, float s) {
  const float ds = g_conf_j ? fmaf(w, d - dot, *g_conf_j) : w * (d - dot);
  return (ds * s) * (1.0f - s);
}

static inline int cpg_nchunks(int c) { return (c + kCpgChunk - 1) / kCpgChunk; }

// ---- the per-crop rest (dot, ds, dlogit), shared with the point-major pooling (conf_pool_pm.hip) ------------------------------
// host: one crop's rows of w, d, conf, g_conf (may be NULL) and of the two outputs
inline void cpg_logits_crop_host(int n1, int n2, const float *w, const float *d, const float *conf, const float *g_conf,
                                 float *dlogit1, float *dlogit2) {
  const int L = n1 + n2;
  float slot[kCpgDotLanes];
  for (int l = 0; l < kCpgDotLanes; ++l) slot[l] = cpg_dot_lane(w, d, L, l);
  const float dot = cpg_dot_tree_host(slot);
  for (int j = 0; j < L; ++j) {
    const float v = cpg_dlogit(w[j], d[j], dot, g_conf ? g_conf + j : nullptr, conf[j]);
    if (j < n1) dlogit1[j] = v;
    else dlogit2[j - n1] = v;
  }
}
// device: launches k_cpg_logits (conf_pool_grad.hip), one workgroup per crop, on `stream` (a hipStream_t).  part: the chunks'
// partials of d, (b, nchunks, L), folded into d first; NULL: d (b, L) holds its values already.
void cpg_launch_logits(int b, int n1, int n2, int nchunks, const float *conf, const float *w, const float *part, float *d,
                       const float *g_conf, float *dlogit1, float *dlogit2, void *stream);
