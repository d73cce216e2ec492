// metric.hip -- fused ADD-S / ADD distances (the step right after the forward in the eval harness).
//
// LineMOD variant (tools/test_LM.py:123-135): non-symmetric objects use ADD = mean_i |pred_i - gt_i| (corresponding
// points), symmetric ones ADD-S; `sym` selects per object inside the same launch (workgroup-uniform branch).
//
// tools/test_YCBV_stage1.py:186-189 poses the class cloud (2620 points) by the predicted and by the ground-truth pose and
// takes mean_i min_j |pred_i - gt_j| through a materialised (b, P, P, 3) difference tensor: 82 MB per object.
// Here one workgroup per (object, 256-point slice of i): the gt-posed cloud is staged once per workgroup in LDS
// (P*12 B = 31 KB), every lane keeps one pred point in registers and scans the LDS copy (broadcast reads), the
// per-point minima are reduced in the workgroup and accumulated per object in fixed slice order by a second tiny
// kernel (deterministic).  sqrt is applied to the minimum squared distance (monotone, same argmin as min of norms).
#include "common.h"
#include "metric_table.h"
#include <math.h>

namespace {

__global__ __launch_bounds__(256) void k_adds_partial(int P, const float *__restrict__ cld, const int32_t *__restrict__ cls,
                                                      const float *__restrict__ Rp, const float *__restrict__ tp,
                                                      const float *__restrict__ Rg, const float *__restrict__ tg,
                                                      float *__restrict__ partial, int nslices,
                                                      const int32_t *__restrict__ sym, int all_mode) {
  extern __shared__ float gt[];                 // [P][3] posed by the ground truth
  __shared__ float red[4];
  const int obj = blockIdx.y, slice = blockIdx.x, tid = threadIdx.x;
  const float *C = cld + (size_t)(cls ? cls[obj] : obj) * P * 3;
  // (the slice's arithmetic lives in metric_table.h: the trajectory kernel of metric_table.hip calls the same functions)
  adds_stage_gt(P, C, Rg + obj * 9, tg + obj * 3, gt, tid);
  __syncthreads();
  const bool nearest = sym ? sym[obj] != 0 : all_mode != 0;
  float sum[1];
  adds_slice_sums<1>(P, slice * 256 + tid, C, Rp + obj * 9, tp + obj * 3, 0, 0, gt, nearest, red, tid, sum);
  if (tid == 0) partial[(size_t)obj * nslices + slice] = sum[0];
}

__global__ void k_adds_finish(int b, int P, int nslices, const float *__restrict__ partial, float *__restrict__ out) {
  const int obj = blockIdx.x * blockDim.x + threadIdx.x;
  if (obj >= b) return;
  float s = 0.0f;
  for (int k = 0; k < nslices; ++k) s += partial[(size_t)obj * nslices + k];
  out[obj] = s / (float)P;
}

}  // namespace

static int add_launch(int b, int P, const float *cld, const int32_t *cls, const float *R_pred, const float *t_pred,
                      const float *R_gt, const float *t_gt, float *partial_scratch, float *out, const int32_t *sym,
                      int all_mode, dclStream_t stream);

DCL_API int dcl_add_s(int b, int P, const float *cld, const int32_t *cls, const float *R_pred, const float *t_pred,
                      const float *R_gt, const float *t_gt, float *partial_scratch, float *out, dclStream_t stream) {
  return add_launch(b, P, cld, cls, R_pred, t_pred, R_gt, t_gt, partial_scratch, out, nullptr, 1, stream);
}

DCL_API int dcl_add(int b, int P, const float *cld, const int32_t *cls, const float *R_pred, const float *t_pred,
                    const float *R_gt, const float *t_gt, float *partial_scratch, float *out, dclStream_t stream) {
  return add_launch(b, P, cld, cls, R_pred, t_pred, R_gt, t_gt, partial_scratch, out, nullptr, 0, stream);
}

DCL_API int dcl_add_by_symmetry(int b, int P, const float *cld, const int32_t *cls, const int32_t *sym_flag,
                                const float *R_pred, const float *t_pred, const float *R_gt, const float *t_gt,
                                float *partial_scratch, float *out, dclStream_t stream) {
  DCL_CHECK_ARG(sym_flag || b == 0);
  return add_launch(b, P, cld, cls, R_pred, t_pred, R_gt, t_gt, partial_scratch, out, sym_flag, 0, stream);
}

static int add_launch(int b, int P, const float *cld, const int32_t *cls, const float *R_pred, const float *t_pred,
                      const float *R_gt, const float *t_gt, float *partial_scratch, float *out, const int32_t *sym,
                      int all_mode, dclStream_t stream) {
  DCL_CHECK_ARG(b >= 0 && P > 0 && (size_t)P * 12 <= 150 * 1024);
  if (b == 0) return 0;
  DCL_CHECK_ARG(cld && R_pred && t_pred && R_gt && t_gt && partial_scratch && out && b <= 65535);
  hipStream_t s = (hipStream_t)stream;
  const int nslices = dcl_div_up(P, 256);
  const size_t lds = (size_t)P * 12;
  if (lds > 48 * 1024)
    (void)hipFuncSetAttribute((const void *)k_adds_partial, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(k_adds_partial, dim3(nslices, b), dim3(256), lds, s, P, cld, cls, R_pred, t_pred, R_gt, t_gt,
                     partial_scratch, nslices, sym, all_mode);
  hipLaunchKernelGGL(k_adds_finish, dim3(dcl_div_up(b, 64)), dim3(64), 0, s, b, P, nslices, partial_scratch, out);
  DCL_LAUNCH_CHECK();
  return 0;
}
