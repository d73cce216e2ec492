// chamfer.hip -- both-direction nearest-neighbour (Chamfer) distances of the training losses, with a deterministic backward.
//
// models/DCL_Net.py:306-312 (`CD_Dis`) takes min over both axes of a materialised (b, n, m) Euclidean matrix built from a
// (b, n, m, 3) difference tensor, and autograd keeps both.  Here, as in metric.hip, a lane keeps its own point in registers
// and scans the opposite cloud from LDS; nothing of size n*m exists in either pass.
//
// Forward, one launch: workgroup = (crop, slice of 256 points, direction), one point per lane (DESIGN.md section 9 says why
// not more).  The opposite cloud is staged in tiles of kTile points, padded to 16 B per point, so that the scan reads one
// point with one wide read at a wave-uniform address (a broadcast: no bank conflicts) and m is not limited by LDS.  The
// minimum is taken on squared distances fma(dz,dz, fma(dy,dy, dx*dx)) in ascending index order with strict '<' (lowest
// index wins a tie); sqrt once at the end.
//
// Backward, one launch: workgroup = (crop, slice of 256 output points, side).  With u(p,t) = (p-t)/|p-t| (0 at distance 0)
//   grad_pred[i]   =  g_pt[i] u(p_i, t_idx_pt[i]) + sum_{j asc, idx_tp[j]=i} g_tp[j] u(p_i, t_j)
//   grad_target[j] = -g_tp[j] u(p_idx_tp[j], t_j) - sum_{i asc, idx_pt[i]=j} g_pt[i] u(p_i, t_j)
// and -u(p,t) = u(t,p) exactly, so both sides are the same sum  g_own u(own, nearest) + sum g_opp u(own, opp)  over the
// opposite points that chose this one.  The lane that owns an output point adds its own term first and then scans the
// opposite INDEX array (staged in LDS, four per wide read, an integer compare each) in ascending order; the opposite point
// and its upstream gradient sit next to it in LDS for the few matches.  No float atomics, no workspace, no workgroup waits
// on another: the same inputs give the same bits.
#include "common.h"
#include <math.h>

namespace {

constexpr int kThreads = 256;
constexpr int kTile = 1024;        // opposite points per LDS tile: 16 KiB (forward), 20 KiB (backward)

// which (crop, slice, side) a workgroup of a two-sided launch is: side A owns slices [0, slices_a) of every crop
struct Slot {
  int crop, slice;
  bool side_a;
};
__device__ __forceinline__ Slot decode_slot(int slices_a, int slices_b) {
  const int per_crop = slices_a + slices_b;
  Slot s;
  s.crop = blockIdx.x / per_crop;
  s.slice = blockIdx.x - s.crop * per_crop;
  s.side_a = s.slice < slices_a;
  if (!s.side_a) s.slice -= slices_a;
  return s;
}

__global__ __launch_bounds__(kThreads) void k_chamfer_fwd(int n, int m, const float *__restrict__ pred,
                                                          const float *__restrict__ target,
                                                          const int32_t *__restrict__ active, float *__restrict__ dist_pt,
                                                          int32_t *__restrict__ idx_pt, float *__restrict__ dist_tp,
                                                          int32_t *__restrict__ idx_tp, int slices_pt, int slices_tp) {
  __shared__ float4 tile[kTile];                         // [x, y, z, -] of the opposite cloud
  const Slot s = decode_slot(slices_pt, slices_tp);
  const int n_own = s.side_a ? n : m, n_opp = s.side_a ? m : n;
  const float *own = (s.side_a ? pred : target) + (size_t)s.crop * n_own * 3;
  const float *opp = (s.side_a ? target : pred) + (size_t)s.crop * n_opp * 3;
  float *dist = (s.side_a ? dist_pt : dist_tp) + (size_t)s.crop * n_own;
  int32_t *idx = (s.side_a ? idx_pt : idx_tp) + (size_t)s.crop * n_own;
  const int tid = threadIdx.x, i = s.slice * kThreads + tid;
  if (active && active[s.crop] == 0) {                   // workgroup-uniform: no distance work for this crop
    if (i < n_own) { dist[i] = 0.0f; idx[i] = -1; }
    return;
  }
  const int ic = min(i, n_own - 1);                      // lanes past the end scan a copy of the last point and write nothing
  const float px = own[ic * 3], py = own[ic * 3 + 1], pz = own[ic * 3 + 2];
  float best = INFINITY;
  int bi = 0;
  for (int t0 = 0; t0 < n_opp; t0 += kTile) {
    const int cnt = min(kTile, n_opp - t0);
    if (t0) __syncthreads();                             // the previous tile has been read by every wave
    for (int j = tid; j < cnt; j += kThreads) {
      const float *c = opp + (size_t)(t0 + j) * 3;
      tile[j] = make_float4(c[0], c[1], c[2], 0.0f);
    }
    __syncthreads();
#pragma unroll 8
    for (int j = 0; j < cnt; ++j) {
      const float4 t = tile[j];                          // wave-uniform address: one broadcast 16-byte read
      const float dx = px - t.x, dy = py - t.y, dz = pz - t.z;
      const float d2 = __fmaf_rn(dz, dz, __fmaf_rn(dy, dy, dx * dx));
      if (d2 < best) { best = d2; bi = t0 + j; }
    }
  }
  if (i < n_own) { dist[i] = sqrtf(best); idx[i] = bi; }
}

// acc += (g / |o - c|) (o - c), nothing at distance 0
__device__ __forceinline__ void add_term(float &ax, float &ay, float &az, float g, float ox, float oy, float oz, float cx,
                                         float cy, float cz) {
  const float dx = ox - cx, dy = oy - cy, dz = oz - cz;
  const float r = sqrtf(__fmaf_rn(dz, dz, __fmaf_rn(dy, dy, dx * dx)));
  const float w = r > 0.0f ? g / r : 0.0f;
  ax = __fmaf_rn(w, dx, ax); ay = __fmaf_rn(w, dy, ay); az = __fmaf_rn(w, dz, az);
}

__global__ __launch_bounds__(kThreads) void k_chamfer_bwd(int n, int m, const float *__restrict__ pred,
                                                          const float *__restrict__ target,
                                                          const int32_t *__restrict__ active,
                                                          const int32_t *__restrict__ idx_pt,
                                                          const int32_t *__restrict__ idx_tp, const float *__restrict__ g_pt,
                                                          const float *__restrict__ g_tp, float *__restrict__ grad_pred,
                                                          float *__restrict__ grad_target, int slices_p, int slices_t) {
  __shared__ float4 tq[kTile];                           // [x, y, z, upstream gradient] of the opposite points
  __shared__ int4 ti[kTile / 4];                         // their nearest-neighbour indices, four per read
  const Slot s = decode_slot(slices_p, slices_t);
  const int n_own = s.side_a ? n : m, n_opp = s.side_a ? m : n;
  const size_t own0 = (size_t)s.crop * n_own, opp0 = (size_t)s.crop * n_opp;
  const float *own = (s.side_a ? pred : target) + own0 * 3, *opp = (s.side_a ? target : pred) + opp0 * 3;
  const int32_t *idx_own = (s.side_a ? idx_pt : idx_tp) + own0, *idx_opp = (s.side_a ? idx_tp : idx_pt) + opp0;
  const float *g_own = (s.side_a ? g_pt : g_tp) + own0, *g_opp = (s.side_a ? g_tp : g_pt) + opp0;
  float *grad = (s.side_a ? grad_pred : grad_target) + own0 * 3;
  const int tid = threadIdx.x, i = s.slice * kThreads + tid;
  if (active && active[s.crop] == 0) {                   // workgroup-uniform
    if (i < n_own) { grad[i * 3] = 0.0f; grad[i * 3 + 1] = 0.0f; grad[i * 3 + 2] = 0.0f; }
    return;
  }
  // lanes past the end take part in the staging and the barriers only: they have no term of their own, match no index
  // (every index is < n_own) and write nothing
  const int ic = min(i, n_own - 1);
  const float ox = own[ic * 3], oy = own[ic * 3 + 1], oz = own[ic * 3 + 2];
  float ax = 0.0f, ay = 0.0f, az = 0.0f;
  const int k = idx_own[ic];
  if (i < n_own && (unsigned)k < (unsigned)n_opp) add_term(ax, ay, az, g_own[ic], ox, oy, oz, opp[k * 3], opp[k * 3 + 1], opp[k * 3 + 2]);
  int32_t *ti1 = reinterpret_cast<int32_t *>(ti);
  for (int t0 = 0; t0 < n_opp; t0 += kTile) {
    const int cnt = min(kTile, n_opp - t0), cnt4 = (cnt + 3) & ~3;
    if (t0) __syncthreads();
    for (int j = tid; j < cnt4; j += kThreads) {
      if (j < cnt) {
        const float *c = opp + (size_t)(t0 + j) * 3;
        tq[j] = make_float4(c[0], c[1], c[2], g_opp[t0 + j]);
        ti1[j] = idx_opp[t0 + j];
      } else {
        ti1[j] = -1;                                     // the ragged end of the last group of four matches nobody
      }
    }
    __syncthreads();
#pragma unroll 2
    for (int j = 0; j < cnt4; j += 4) {
      const int4 v = ti[j >> 2];
      if (v.x == i) { const float4 c = tq[j]; add_term(ax, ay, az, c.w, ox, oy, oz, c.x, c.y, c.z); }
      if (v.y == i) { const float4 c = tq[j + 1]; add_term(ax, ay, az, c.w, ox, oy, oz, c.x, c.y, c.z); }
      if (v.z == i) { const float4 c = tq[j + 2]; add_term(ax, ay, az, c.w, ox, oy, oz, c.x, c.y, c.z); }
      if (v.w == i) { const float4 c = tq[j + 3]; add_term(ax, ay, az, c.w, ox, oy, oz, c.x, c.y, c.z); }
    }
  }
  if (i < n_own) { grad[i * 3] = ax; grad[i * 3 + 1] = ay; grad[i * 3 + 2] = az; }
}

}  // namespace

DCL_API int dcl_chamfer_fwd(int b, int n, int m, const float *pred, const float *target, const int32_t *active,
                            float *dist_pt, int32_t *idx_pt, float *dist_tp, int32_t *idx_tp, dclStream_t stream) {
  DCL_CHECK_ARG(b >= 0 && n >= 1 && m >= 1);
  if (b == 0) return 0;
  DCL_CHECK_ARG(pred && target && dist_pt && idx_pt && dist_tp && idx_tp);
  DCL_CHECK_ARG((long long)b * n * 3 <= INT32_MAX && (long long)b * m * 3 <= INT32_MAX);
  hipStream_t s = (hipStream_t)stream;
  const int spt = dcl_div_up(n, kThreads), stp = dcl_div_up(m, kThreads);
  hipLaunchKernelGGL(k_chamfer_fwd, dim3(b * (spt + stp)), dim3(kThreads), 0, s, n, m, pred, target, active, dist_pt, idx_pt,
                     dist_tp, idx_tp, spt, stp);
  DCL_LAUNCH_CHECK();
  return 0;
}

DCL_API int dcl_chamfer_bwd(int b, int n, int m, const float *pred, const float *target, const int32_t *active,
                            const int32_t *idx_pt, const int32_t *idx_tp, const float *g_pt, const float *g_tp,
                            float *grad_pred, float *grad_target, dclStream_t stream) {
  DCL_CHECK_ARG(b >= 0 && n >= 1 && m >= 1);
  DCL_CHECK_ARG(grad_pred || grad_target);
  if (b == 0) return 0;
  DCL_CHECK_ARG(pred && target && idx_pt && idx_tp && g_pt && g_tp);
  DCL_CHECK_ARG((long long)b * n * 3 <= INT32_MAX && (long long)b * m * 3 <= INT32_MAX);
  const int sp = grad_pred ? dcl_div_up(n, kThreads) : 0, st = grad_target ? dcl_div_up(m, kThreads) : 0;
  hipLaunchKernelGGL(k_chamfer_bwd, dim3(b * (sp + st)), dim3(kThreads), 0, (hipStream_t)stream, n, m, pred, target, active,
                     idx_pt, idx_tp, g_pt, g_tp, grad_pred, grad_target, sp, st);
  DCL_LAUNCH_CHECK();
  return 0;
}
