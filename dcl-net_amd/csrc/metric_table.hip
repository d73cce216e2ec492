// metric_table.hip -- ADD(-S) over a pose trajectory and the device-resident evaluation tables (include/dclnet_hip.h:
// "device-resident eval tables").
//
// k_adds_traj_partial: metric.hip's slice kernel with the pose loop inside -- a workgroup owns an (object, 256-point slice),
// stages the ground-truth-posed cloud in LDS ONCE and walks the T poses of the trajectory, three per scan of the staged
// cloud: independent minimum chains that share every LDS read (scoring every refine iteration otherwise re-poses, re-stages
// and re-scans the same cloud T times, one dependent chain per lane).  The slice arithmetic is metric_table.h's, shared with
// k_adds_partial, so dis[t] has dcl_add_s's bits.
// k_metric_tabulate: one block row per step t, lane c owns class c; the block stages a chunk of crops (distance, class,
// valid) in LDS -- finishing the distances from the slice sums in the fused form -- and every lane walks the chunk in
// ascending crop order, updating its own registers; plain per-lane stores at the end.  No atomics: the same bits every run.
#include "common.h"
#include "metric_table.h"
#include <math.h>

namespace {

constexpr int kTabChunk = 1024;   // crops staged per pass: 12 KiB of LDS
constexpr int kTrajPoses = 3;     // poses a workgroup scores per scan of its staged cloud

template <int NP>
__device__ __forceinline__ void traj_group(int P, int i, const float *C, const float *R1, const float *t1, size_t sR, size_t st,
                                           const float *gt, bool nearest, float *red, int tid, float *out, size_t so) {
  float sum[NP];
  adds_slice_sums<NP>(P, i, C, R1, t1, sR, st, gt, nearest, red, tid, sum);
  if (tid == 0) {
#pragma unroll
    for (int k = 0; k < NP; ++k) out[k * so] = sum[k];
  }
}

__global__ __launch_bounds__(256) void k_adds_traj_partial(int T, int b, int P, int n_clouds, const float *__restrict__ cld,
                                                           const int32_t *__restrict__ cls, const float *__restrict__ Rp,
                                                           const float *__restrict__ tp, const float *__restrict__ Rg,
                                                           const float *__restrict__ tg, const int32_t *__restrict__ valid,
                                                           float *__restrict__ partial, int nslices,
                                                           const int32_t *__restrict__ sym, int all_mode) {
  extern __shared__ float gt[];                 // [P][3] posed by the ground truth
  __shared__ float red[4 * kTrajPoses];
  const int obj = blockIdx.y, slice = blockIdx.x, tid = threadIdx.x;
  if (valid && valid[obj] <= 0) return;         // workgroup-uniform: no work, the poses are not read (0: no crop, < 0: padding)
  const int cloud = cls ? cls[obj] : obj;
  if ((unsigned)cloud >= (unsigned)n_clouds) return;
  const float *C = cld + (size_t)cloud * P * 3;
  adds_stage_gt(P, C, Rg + obj * 9, tg + obj * 3, gt, tid);
  __syncthreads();
  const bool nearest = sym ? sym[obj] != 0 : all_mode != 0;
  const int i = slice * 256 + tid;
  const size_t sR = (size_t)b * 9, st = (size_t)b * 3;
  for (int t0 = 0; t0 < T; t0 += kTrajPoses) {  // kTrajPoses poses share every read of the staged cloud
    const float *R1 = Rp + ((size_t)t0 * b + obj) * 9, *t1 = tp + ((size_t)t0 * b + obj) * 3;
    float *out = partial + ((size_t)t0 * b + obj) * nslices + slice;
    const size_t so = (size_t)b * nslices;
    const int np = T - t0 < kTrajPoses ? T - t0 : kTrajPoses;       // workgroup-uniform
    if (np == 3) traj_group<3>(P, i, C, R1, t1, sR, st, gt, nearest, red, tid, out, so);
    else if (np == 2) traj_group<2>(P, i, C, R1, t1, sR, st, gt, nearest, red, tid, out, so);
    else traj_group<1>(P, i, C, R1, t1, sR, st, gt, nearest, red, tid, out, so);
    __syncthreads();                            // red[] is rewritten by the next group
  }
}

__device__ __forceinline__ bool crop_has_distance(const int32_t *valid, const int32_t *cloud, bool by_cloud, int n_clouds, int i) {
  if (valid && valid[i] <= 0) return false;
  return !by_cloud || (unsigned)(cloud ? cloud[i] : i) < (unsigned)n_clouds;
}

// k_adds_finish's sum: the slices in ascending order, then / P
__device__ __forceinline__ float finish_distance(const float *partial, size_t e, int nslices, int P) {
  float s = 0.0f;
  for (int k = 0; k < nslices; ++k) s += partial[e * nslices + k];
  return s / (float)P;
}

__global__ void k_adds_traj_finish(int T, int b, int P, int n_clouds, int nslices, const float *__restrict__ partial,
                                   const int32_t *__restrict__ cls, const int32_t *__restrict__ valid, float *__restrict__ dis) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, t = blockIdx.y;
  if (i >= b) return;
  const size_t e = (size_t)t * b + i;
  dis[e] = crop_has_distance(valid, cls, true, n_clouds, i) ? finish_distance(partial, e, nslices, P) : INFINITY;
}

// partial != nullptr: the fused form -- the distances are finished here (and written to dis_out when it is given);
// otherwise they are read from dis_in.
__global__ __launch_bounds__(1024) void k_metric_tabulate(int mode, int b, int C, int P, int n_clouds, int nslices,
                                                          const float *__restrict__ partial, const float *__restrict__ dis_in,
                                                          float *__restrict__ dis_out, const int32_t *__restrict__ cloud,
                                                          const int32_t *__restrict__ cls, const int32_t *__restrict__ valid,
                                                          const double *__restrict__ diameter, double *__restrict__ sums,
                                                          double *__restrict__ maxd, int64_t *__restrict__ counts,
                                                          int32_t *__restrict__ bad) {
  __shared__ float s_d[kTabChunk];
  __shared__ int32_t s_c[kTabChunk];
  __shared__ int32_t s_v[kTabChunk];            // bit 0: valid, bit 1: raises bad (a cloud index out of range), bit 2: padding
  const int t = blockIdx.x, c = blockIdx.y * blockDim.x + threadIdx.x;
  const bool mine = c < C;
  const size_t ent = (size_t)t * C + (mine ? c : 0);
  DclTableAcc a;
  dcl_table_load(mode, ent, sums, maxd, counts, a);
  const double diam = (mode != DCL_TABLE_ADDS && mine) ? diameter[c] : 0.0;
  bool saw_bad = false;
  for (int base = 0; base < b; base += kTabChunk) {
    const int n = b - base < kTabChunk ? b - base : kTabChunk;
    for (int k = threadIdx.x; k < n; k += blockDim.x) {
      const int i = base + k;
      const size_t e = (size_t)t * b + i;
      const int32_t v = valid ? valid[i] : 1;
      const bool ok = v > 0;
      int flags = ok ? 1 : (v < 0 ? 4 : 0);      // valid < 0: not a crop -- no entry and no flag is touched for it
      float d;
      if (partial) {
        const bool has = crop_has_distance(valid, cloud, true, n_clouds, i);
        d = has ? finish_distance(partial, e, nslices, P) : INFINITY;
        if (ok && !has) flags |= 2;
        if (dis_out && blockIdx.y == 0) dis_out[e] = d;
      } else {
        d = dis_in[e];
      }
      s_d[k] = d;
      s_c[k] = cls[i];
      s_v[k] = flags;
    }
    __syncthreads();
    if (mine) {
      for (int k = 0; k < n; ++k) {             // ascending crop order: the pinned summation order of sum D
        const int cc = s_c[k], f = s_v[k];
        if (f & 4) continue;
        if ((unsigned)cc >= (unsigned)C || (f & 2)) saw_bad = true;
        if (cc == c) dcl_table_step(mode, (f & 1) != 0, s_d[k], diam, a);
      }
    }
    __syncthreads();
  }
  if (mine) dcl_table_store(mode, ent, a, sums, maxd, counts);
  if (saw_bad && c == 0) bad[0] = 1;            // every step's lane 0 stores the same value; never read here
}

int traj_check(int T, int b, int P, int n_clouds, int all_mode) {
  DCL_CHECK_ARG(T >= 1 && b >= 0 && P > 0 && (size_t)P * 12 <= 150 * 1024 && n_clouds >= 0 && (all_mode == 0 || all_mode == 1));
  return 0;
}

void launch_traj_partial(int T, int b, int P, int n_clouds, const float *cld, const int32_t *cls, const int32_t *sym,
                         int all_mode, const float *R_pred, const float *t_pred, const float *R_gt, const float *t_gt,
                         const int32_t *valid, float *partial, hipStream_t s) {
  const int nslices = dcl_div_up(P, 256);
  const size_t lds = (size_t)P * 12;
  if (lds > 48 * 1024)
    (void)hipFuncSetAttribute((const void *)k_adds_traj_partial, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(k_adds_traj_partial, dim3(nslices, b), dim3(256), lds, s, T, b, P, n_clouds, cld, cls, R_pred, t_pred, R_gt,
                     t_gt, valid, partial, nslices, sym, all_mode);
}

void launch_tabulate(int mode, int T, int b, int C, int P, int n_clouds, const float *partial, const float *dis_in,
                     float *dis_out, const int32_t *cloud, const int32_t *cls, const int32_t *valid, const double *diameter,
                     double *sums, double *maxd, int64_t *counts, int32_t *bad, hipStream_t s) {
  const int block = C >= 1024 ? 1024 : dcl_div_up(C, 64) * 64;      // lane c owns class c: enough waves for C
  hipLaunchKernelGGL(k_metric_tabulate, dim3(T, dcl_div_up(C, block)), dim3(block), 0, s, mode, b, C, P, n_clouds,
                     partial ? dcl_div_up(P, 256) : 0, partial, dis_in, dis_out, cloud, cls, valid, diameter, sums, maxd, counts,
                     bad);
}

}  // namespace

DCL_API int dcl_add_traj(int T, int b, int P, int n_clouds, const float *cld, const int32_t *cls, const int32_t *sym,
                         int all_mode, const float *R_pred, const float *t_pred, const float *R_gt, const float *t_gt,
                         const int32_t *valid, float *partial_scratch, float *dis, dclStream_t stream) {
  if (int rc = traj_check(T, b, P, n_clouds, all_mode)) return rc;
  if (b == 0) return 0;
  DCL_CHECK_ARG(cld && R_pred && t_pred && R_gt && t_gt && partial_scratch && dis && b <= 65535 && T <= 65535);
  DCL_CHECK_ARG(cls || n_clouds >= b);
  hipStream_t s = (hipStream_t)stream;
  launch_traj_partial(T, b, P, n_clouds, cld, cls, sym, all_mode, R_pred, t_pred, R_gt, t_gt, valid, partial_scratch, s);
  hipLaunchKernelGGL(k_adds_traj_finish, dim3(dcl_div_up(b, 64), T), dim3(64), 0, s, T, b, P, n_clouds, dcl_div_up(P, 256),
                     partial_scratch, cls, valid, dis);
  DCL_LAUNCH_CHECK();
  return 0;
}

DCL_API int dcl_metric_tabulate(int mode, int T, int b, int C, const float *dis, const int32_t *cls, const int32_t *valid,
                                const double *diameter, double *sums, double *maxd, int64_t *counts, int32_t *bad,
                                dclStream_t stream) {
  DCL_TABLE_CHECK_ARGS();
  if (b == 0) return 0;
  DCL_CHECK_ARG(dis && cls && T <= (1 << 20));
  launch_tabulate(mode, T, b, C, 0, 0, nullptr, dis, nullptr, nullptr, cls, valid, diameter, sums, maxd, counts, bad,
                  (hipStream_t)stream);
  DCL_LAUNCH_CHECK();
  return 0;
}

DCL_API int dcl_add_tabulate(int mode, int T, int b, int P, int n_clouds, int C, const float *cld, const int32_t *cloud,
                             const int32_t *cls, const int32_t *sym, int all_mode, const float *R_pred, const float *t_pred,
                             const float *R_gt, const float *t_gt, const int32_t *valid, const double *diameter,
                             float *partial_scratch, float *dis, double *sums, double *maxd, int64_t *counts, int32_t *bad,
                             dclStream_t stream) {
  if (int rc = traj_check(T, b, P, n_clouds, all_mode)) return rc;
  DCL_TABLE_CHECK_ARGS();
  if (b == 0) return 0;
  DCL_CHECK_ARG(cld && cls && R_pred && t_pred && R_gt && t_gt && partial_scratch && b <= 65535 && T <= 65535);
  DCL_CHECK_ARG(cloud || n_clouds >= b);
  hipStream_t s = (hipStream_t)stream;
  launch_traj_partial(T, b, P, n_clouds, cld, cloud, sym, all_mode, R_pred, t_pred, R_gt, t_gt, valid, partial_scratch, s);
  launch_tabulate(mode, T, b, C, P, n_clouds, partial_scratch, nullptr, dis, cloud, cls, valid, diameter, sums, maxd, counts,
                  bad, s);
  DCL_LAUNCH_CHECK();
  return 0;
}
