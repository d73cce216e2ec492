// rotation_grad.hip -- the gradient of ortho9d2matrix (models/DCL_Net.py:15-36): dcl_ortho9d_bwd and its host twin.
//
// R = U' V'^T is the rotation nearest the normalised axes M (its polar factor, with the reflection folded into the third
// singular value).  For G = dL/dR the gradient with respect to M is U' Y V'^T with Y_ij = (B_ij - B_ji) / (s'_i + s'_j),
// B = U'^T G V' (ortho9d.h: ortho9d_grad, which also chains through the normalisation).  Differentiating the SVD's U and V
// apart, as autograd does with the torch composition, divides by s_i^2 - s_j^2 instead -- zero for orthonormal axes, which is
// where a trained rotation head lives.
//
// MI355X mapping.  One lane per crop, 64 per workgroup, like k_ortho9d: a batch is tens of crops, the work per crop a
// handful of 3x3 Jacobi sweeps in fp64, so the launch is latency and nothing else.  The factors are recomputed from o9 (the
// forward saves nothing else); a lane reads its 18 floats and writes the 9 it alone owns -- no atomics, no workspace, no
// LDS, the same bits on every call.
#include "common.h"
#include "ortho9d.h"

namespace {

__global__ __launch_bounds__(64) void k_ortho9d_bwd(int b, const float *__restrict__ o9, const float *__restrict__ grad_R,
                                                    float *__restrict__ grad_o9) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < b) ortho9d_grad(o9 + (size_t)i * 9, grad_R + (size_t)i * 9, grad_o9 + (size_t)i * 9);
}

}  // namespace

DCL_API int dcl_ortho9d_bwd(int b, const float *o9, const float *grad_R, float *grad_o9, dclStream_t stream) {
  DCL_CHECK_ARG(b >= 0);
  if (b == 0) return 0;
  DCL_CHECK_ARG(o9 && grad_R && grad_o9);
  hipLaunchKernelGGL(k_ortho9d_bwd, dim3(dcl_div_up(b, 64)), dim3(64), 0, (hipStream_t)stream, b, o9, grad_R, grad_o9);
  DCL_LAUNCH_CHECK();
  return 0;
}

// the same routine on host pointers (tests of the mathematics on machines without a GPU; no GPU call is made)
DCL_API int dcl_ortho9d_bwd_host(int b, const float *o9, const float *grad_R, float *grad_o9) {
  DCL_CHECK_ARG(b >= 0);
  if (b == 0) return 0;
  DCL_CHECK_ARG(o9 && grad_R && grad_o9);
  for (int i = 0; i < b; ++i) ortho9d_grad(o9 + (size_t)i * 9, grad_R + (size_t)i * 9, grad_o9 + (size_t)i * 9);
  return 0;
}
