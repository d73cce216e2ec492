// objective.hip -- the training objective between net(data) and loss.backward() (models/DCL_Net.py:264-304,
// models/refiner.py:101-125) on the device: the rigid transforms that pose the template and canonicalise the observed points,
// the per-point loss terms with their ordered sums packed into one (5,) tensor, and every gradient.  objective.h holds the
// arithmetic and the pinned reduction order; the *_host entry points run the same routines on host pointers.
//
// MI355X mapping.  Everything here is a few hundred KB per call and launch-bound, so the aim is few launches, not bandwidth:
//   k_rigid_points      one lane per point, 256 per workgroup: 3 loads, 12 uniform loads (R, t: scalar loads), 3 stores.
//   k_rigid_points_bwd  one workgroup per crop (the pinned order): lane l walks points l, l+256, ..., writes g_pts as it goes,
//                       keeps 12 accumulators (g_R, g_t) and folds them through 12 KiB of LDS, strides 128 .. 1.
//   k_objective_crop    one workgroup per crop, the same walk and fold over 5 accumulators; writes L and the crop's 5 sums.
//   k_objective_final   one wave: lane k < 5 adds column k over the crops in ascending order, lane 0 writes packed.
//   k_objective_bwd     one lane per point, no reduction: 4 gradients and 6 Chamfer-distance gradients in one launch; the
//                       weights are formed from the device (5,) upstream gradient by every lane (5 uniform loads).
// No float atomics, no workgroup waits on another, nothing read back: the same inputs give the same bits.
#include "common.h"
#include "objective.h"

namespace {

__global__ __launch_bounds__(kObjLanes) void k_rigid_points(int n, const float *__restrict__ pts, const float *__restrict__ R,
                                                            const float *__restrict__ t, int inverse, float *__restrict__ out) {
  const int crop = blockIdx.y, i = blockIdx.x * kObjLanes + threadIdx.x;
  if (i >= n) return;
  const size_t o = ((size_t)crop * n + i) * 3;
  float r[3];
  obj_rigid_point(R + (size_t)crop * 9, t + (size_t)crop * 3, inverse, pts + o, r);
  out[o] = r[0]; out[o + 1] = r[1]; out[o + 2] = r[2];
}

// slot[k][lane] folded with strides 128 .. 1; on return slot[k][0] holds the sum for every k < K (all lanes must call)
template <int K>
__device__ __forceinline__ void fold(float (*slot)[kObjLanes], const float *acc, int tid) {
#pragma unroll
  for (int k = 0; k < K; ++k) slot[k][tid] = acc[k];
  for (int s = kObjLanes / 2; s >= 1; s >>= 1) {
    __syncthreads();
    if (tid < s) {
#pragma unroll
      for (int k = 0; k < K; ++k) slot[k][tid] += slot[k][tid + s];
    }
  }
  __syncthreads();
}

__global__ __launch_bounds__(kObjLanes) void k_rigid_points_bwd(int n, const float *__restrict__ pts,
                                                                const float *__restrict__ R, const float *__restrict__ t,
                                                                int inverse, const float *__restrict__ g_out,
                                                                float *__restrict__ g_R, float *__restrict__ g_t,
                                                                float *__restrict__ g_pts) {
  __shared__ float slot[12][kObjLanes];
  const int crop = blockIdx.x, tid = threadIdx.x;
  float acc[12];
  obj_rigid_lane_grad(n, pts, R, t, inverse, g_out, g_pts, crop, tid, acc);
  fold<12>(slot, acc, tid);
  if (tid < 9) g_R[(size_t)crop * 9 + tid] = slot[tid][0];
  else if (tid < 12) g_t[(size_t)crop * 3 + tid - 9] = slot[tid][0];
}

__global__ __launch_bounds__(kObjLanes) void k_objective_crop(ObjArgs a, float *__restrict__ crop_sums) {
  __shared__ float slot[kObjSums][kObjLanes];
  const int crop = blockIdx.x, tid = threadIdx.x;
  float acc[kObjSums];
  obj_lane_fwd(a, crop, tid, acc);
  fold<kObjSums>(slot, acc, tid);
  if (tid < kObjSums) crop_sums[(size_t)crop * kObjSums + tid] = slot[tid][0];
}

__global__ __launch_bounds__(64) void k_objective_final(int b, int n, int full, const float *__restrict__ crop_sums,
                                                        float *__restrict__ packed) {
  __shared__ float tot[kObjSums];
  const int tid = threadIdx.x;
  if (tid < kObjSums) tot[tid] = obj_column_sum(crop_sums, b, tid);
  __syncthreads();
  if (tid == 0) obj_finalize(tot, b, n, full, packed);
}

__global__ __launch_bounds__(kObjLanes) void k_objective_bwd(ObjArgs a) {
  const int crop = blockIdx.y, i = blockIdx.x * kObjLanes + threadIdx.x;
  if (i < a.n) obj_point_bwd(a, crop, i);
}

int rigid_check(int b, int n, const void *pts, const void *R, const void *t, int inverse, const void *a,
                const void *c, const void *d) {
  if (!(b >= 0 && n >= 1 && (inverse == 0 || inverse == 1))) return 1;
  if (b == 0) return 0;
  if (!(pts && R && t && a && c && d)) return 1;
  if ((long long)b * n * 3 > INT32_MAX || b > 65535) return 1;
  return 0;
}

// fills ObjArgs and validates one forward or backward call; returns 0 when the arguments are good
int objective_args(ObjArgs &a, int b, int n, const float *posed, const float *posed_gt, const float *Yc,
                   const float *cano_pred, const float *cano_gt, const float *Xo, const float *conf, const float *sym,
                   const float *cd_pose_pt, const float *cd_pose_tp, const float *cd_Xo_pt, const float *cd_Xo_tp,
                   const float *cd_Yc_pt, const float *cd_Yc_tp, const float *L, bool need_cd) {
  // the backward does not read the Chamfer halves (their gradients depend on sym alone): it passes its L in their place
  const void *opt[] = {Yc, cano_pred, cano_gt, Xo, conf, L, need_cd ? cd_Xo_pt : L, need_cd ? cd_Xo_tp : L,
                       need_cd ? cd_Yc_pt : L, need_cd ? cd_Yc_tp : L};
  int have = 0;
  for (const void *p : opt) have += p != nullptr;
  if (have != 0 && have != 10) return 1;                 // a partial set of the optional arrays
  if (!(posed && posed_gt && sym)) return 1;
  if (need_cd && !(cd_pose_pt && cd_pose_tp)) return 1;
  if ((long long)b * n * 3 > INT32_MAX || b > 65535) return 1;
  a = ObjArgs{};
  a.b = b; a.n = n; a.full = have != 0;
  a.posed = posed; a.posed_gt = posed_gt; a.Yc = Yc; a.cano_pred = cano_pred; a.cano_gt = cano_gt; a.Xo = Xo;
  a.conf = conf; a.sym = sym;
  a.cd_pose_pt = cd_pose_pt; a.cd_pose_tp = cd_pose_tp; a.cd_Xo_pt = cd_Xo_pt; a.cd_Xo_tp = cd_Xo_tp;
  a.cd_Yc_pt = cd_Yc_pt; a.cd_Yc_tp = cd_Yc_tp;
  return 0;
}

int objective_bwd_outputs(ObjArgs &a, const float *g_packed, float *g_posed, float *g_Xo, float *g_Yc, float *g_conf,
                          float *g_cd_pose_pt, float *g_cd_pose_tp, float *g_cd_Xo_pt, float *g_cd_Xo_tp,
                          float *g_cd_Yc_pt, float *g_cd_Yc_tp) {
  if (!(g_packed && g_posed && g_cd_pose_pt && g_cd_pose_tp)) return 1;
  const void *opt[] = {g_Xo, g_Yc, g_conf, g_cd_Xo_pt, g_cd_Xo_tp, g_cd_Yc_pt, g_cd_Yc_tp};
  int have = 0;
  for (const void *p : opt) have += p != nullptr;
  if (have != (a.full ? 7 : 0)) return 1;                // the optional outputs go with the optional inputs
  a.g_packed = g_packed; a.g_posed = g_posed; a.g_Xo = g_Xo; a.g_Yc = g_Yc; a.g_conf = g_conf;
  a.g_cd_pose_pt = g_cd_pose_pt; a.g_cd_pose_tp = g_cd_pose_tp; a.g_cd_Xo_pt = g_cd_Xo_pt; a.g_cd_Xo_tp = g_cd_Xo_tp;
  a.g_cd_Yc_pt = g_cd_Yc_pt; a.g_cd_Yc_tp = g_cd_Yc_tp;
  return 0;
}

}  // namespace

#define OBJ_IN_PARAMS                                                                                                      \
  int b, int n, const float *posed, const float *posed_gt, const float *Yc, const float *cano_pred, const float *cano_gt,   \
      const float *Xo, const float *conf, const float *sym
#define OBJ_IN_NAMES b, n, posed, posed_gt, Yc, cano_pred, cano_gt, Xo, conf, sym
#define OBJ_CD_PARAMS                                                                                                      \
  const float *cd_pose_pt, const float *cd_pose_tp, const float *cd_Xo_pt, const float *cd_Xo_tp, const float *cd_Yc_pt,    \
      const float *cd_Yc_tp
#define OBJ_CD_NAMES cd_pose_pt, cd_pose_tp, cd_Xo_pt, cd_Xo_tp, cd_Yc_pt, cd_Yc_tp
#define OBJ_NO_CD nullptr, nullptr, nullptr, nullptr, nullptr, nullptr
#define OBJ_BWD_OUT_PARAMS                                                                                                 \
  const float *g_packed, float *g_posed, float *g_Xo, float *g_Yc, float *g_conf, float *g_cd_pose_pt, float *g_cd_pose_tp, \
      float *g_cd_Xo_pt, float *g_cd_Xo_tp, float *g_cd_Yc_pt, float *g_cd_Yc_tp
#define OBJ_BWD_OUT_NAMES \
  g_packed, g_posed, g_Xo, g_Yc, g_conf, g_cd_pose_pt, g_cd_pose_tp, g_cd_Xo_pt, g_cd_Xo_tp, g_cd_Yc_pt, g_cd_Yc_tp

DCL_API int dcl_rigid_points(int b, int n, const float *pts, const float *R, const float *t, int inverse, float *out,
                             dclStream_t stream) {
  DCL_CHECK_ARG(rigid_check(b, n, pts, R, t, inverse, out, out, out) == 0);
  if (b == 0) return 0;
  hipLaunchKernelGGL(k_rigid_points, dim3(dcl_div_up(n, kObjLanes), b), dim3(kObjLanes), 0, (hipStream_t)stream, n, pts, R, t,
                     inverse, out);
  DCL_LAUNCH_CHECK();
  return 0;
}

DCL_API int dcl_rigid_points_host(int b, int n, const float *pts, const float *R, const float *t, int inverse, float *out) {
  DCL_CHECK_ARG(rigid_check(b, n, pts, R, t, inverse, out, out, out) == 0);
  for (int c = 0; c < b; ++c)
    for (int i = 0; i < n; ++i) {
      const size_t o = ((size_t)c * n + i) * 3;
      obj_rigid_point(R + (size_t)c * 9, t + (size_t)c * 3, inverse, pts + o, out + o);
    }
  return 0;
}

DCL_API int dcl_rigid_points_bwd(int b, int n, const float *pts, const float *R, const float *t, int inverse,
                                 const float *g_out, float *g_R, float *g_t, float *g_pts, dclStream_t stream) {
  DCL_CHECK_ARG(rigid_check(b, n, pts, R, t, inverse, g_out, g_R, g_t) == 0);
  if (b == 0) return 0;
  hipLaunchKernelGGL(k_rigid_points_bwd, dim3(b), dim3(kObjLanes), 0, (hipStream_t)stream, n, pts, R, t, inverse, g_out, g_R,
                     g_t, g_pts);
  DCL_LAUNCH_CHECK();
  return 0;
}

DCL_API int dcl_rigid_points_bwd_host(int b, int n, const float *pts, const float *R, const float *t, int inverse,
                                      const float *g_out, float *g_R, float *g_t, float *g_pts) {
  DCL_CHECK_ARG(rigid_check(b, n, pts, R, t, inverse, g_out, g_R, g_t) == 0);
  static thread_local float slot[12][kObjLanes];
  for (int c = 0; c < b; ++c) {
    for (int l = 0; l < kObjLanes; ++l) {
      float acc[12];
      obj_rigid_lane_grad(n, pts, R, t, inverse, g_out, g_pts, c, l, acc);
      for (int k = 0; k < 12; ++k) slot[k][l] = acc[k];
    }
    for (int k = 0; k < 9; ++k) g_R[(size_t)c * 9 + k] = obj_tree_host(slot[k]);
    for (int k = 0; k < 3; ++k) g_t[(size_t)c * 3 + k] = obj_tree_host(slot[9 + k]);
  }
  return 0;
}

DCL_API int dcl_pose_objective_fwd(OBJ_IN_PARAMS, OBJ_CD_PARAMS, float *L, float *crop_sums, float *packed, dclStream_t stream) {
  DCL_CHECK_ARG(b >= 0 && n >= 1);
  if (b == 0) return 0;
  ObjArgs a;
  DCL_CHECK_ARG(objective_args(a, OBJ_IN_NAMES, OBJ_CD_NAMES, L, true) == 0 && crop_sums && packed);
  a.L = L;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_objective_crop, dim3(b), dim3(kObjLanes), 0, s, a, crop_sums);
  hipLaunchKernelGGL(k_objective_final, dim3(1), dim3(64), 0, s, b, n, a.full, (const float *)crop_sums, packed);
  DCL_LAUNCH_CHECK();
  return 0;
}

DCL_API int dcl_pose_objective_fwd_host(OBJ_IN_PARAMS, OBJ_CD_PARAMS, float *L, float *crop_sums, float *packed) {
  DCL_CHECK_ARG(b >= 0 && n >= 1);
  if (b == 0) return 0;
  ObjArgs a;
  DCL_CHECK_ARG(objective_args(a, OBJ_IN_NAMES, OBJ_CD_NAMES, L, true) == 0 && crop_sums && packed);
  a.L = L;
  static thread_local float slot[kObjSums][kObjLanes];
  for (int c = 0; c < b; ++c) {
    for (int l = 0; l < kObjLanes; ++l) {
      float acc[kObjSums];
      obj_lane_fwd(a, c, l, acc);
      for (int k = 0; k < kObjSums; ++k) slot[k][l] = acc[k];
    }
    for (int k = 0; k < kObjSums; ++k) crop_sums[(size_t)c * kObjSums + k] = obj_tree_host(slot[k]);
  }
  float tot[kObjSums];
  for (int k = 0; k < kObjSums; ++k) tot[k] = obj_column_sum(crop_sums, b, k);
  obj_finalize(tot, b, n, a.full, packed);
  return 0;
}

DCL_API int dcl_pose_objective_bwd(OBJ_IN_PARAMS, const float *L, OBJ_BWD_OUT_PARAMS, dclStream_t stream) {
  DCL_CHECK_ARG(b >= 0 && n >= 1);
  if (b == 0) return 0;
  ObjArgs a;
  DCL_CHECK_ARG(objective_args(a, OBJ_IN_NAMES, OBJ_NO_CD, L, false) == 0);
  DCL_CHECK_ARG(objective_bwd_outputs(a, OBJ_BWD_OUT_NAMES) == 0);
  a.Lr = L;
  hipLaunchKernelGGL(k_objective_bwd, dim3(dcl_div_up(n, kObjLanes), b), dim3(kObjLanes), 0, (hipStream_t)stream, a);
  DCL_LAUNCH_CHECK();
  return 0;
}

DCL_API int dcl_pose_objective_bwd_host(OBJ_IN_PARAMS, const float *L, OBJ_BWD_OUT_PARAMS) {
  DCL_CHECK_ARG(b >= 0 && n >= 1);
  if (b == 0) return 0;
  ObjArgs a;
  DCL_CHECK_ARG(objective_args(a, OBJ_IN_NAMES, OBJ_NO_CD, L, false) == 0);
  DCL_CHECK_ARG(objective_bwd_outputs(a, OBJ_BWD_OUT_NAMES) == 0);
  a.Lr = L;
  for (int c = 0; c < b; ++c)
    for (int i = 0; i < n; ++i) obj_point_bwd(a, c, i);
  return 0;
}
