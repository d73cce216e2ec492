// refine_pose.h -- the arithmetic of the eval refine loop's device form (dense.hip: k_refine_first, k_heads_l1_tiles,
// k_heads_l23_compose), shared by the kernels and their host twins: every routine here is __host__ __device__, and the library
// is built with -ffp-contract=off, so the operations below are the operations executed, in this order, on either side.
#pragma once
#include <math.h>
#include <stddef.h>

#include "objective.h"

// one channel of the refiner's first shared layer on a canonicalised point (x, y, z): k_affine3_relu's chain,
// (x Wx + y Wy) + z Wz as fmas, then the constant term, then ReLU
OBJ_HD float refine_first_channel(float x, float y, float z, float wx, float wy, float wz, float a) {
  return fmaxf(fmaf(z, wz, fmaf(y, wy, x * wx)) + a, 0.0f);
}

// channels 4 q .. 4 q + 3 of row `row` (crop = row / n): cur = R^T (p - t) (obj_rigid_point, inverse form), never stored
OBJ_HD void refine_first_quad(const float *Rc, const float *tc, const float *p, const float *W3, int c, int q, const float *term4,
                              float *out4) {
  float cur[3];
  obj_rigid_point(Rc, tc, 1, p, cur);
#pragma unroll
  for (int j = 0; j < 4; ++j)
    out4[j] = refine_first_channel(cur[0], cur[1], cur[2], W3[4 * q + j], W3[c + 4 * q + j], W3[2 * c + 4 * q + j], term4[j]);
}

// pose composition of one crop, row-major: R_out = R dR, t_out = R dt + t, each dot product as
// fmaf(R_i2, d_2, fmaf(R_i1, d_1, R_i0 * d_0)).  Either output (with its delta) may be NULL: the rotation and the translation
// workgroup of a crop each form their own.
OBJ_HD void pose_compose(const float *R, const float *t, const float *dR, const float *dt, float *R_out, float *t_out) {
  if (R_out) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j)
        R_out[3 * i + j] = fmaf(R[3 * i + 2], dR[6 + j], fmaf(R[3 * i + 1], dR[3 + j], R[3 * i] * dR[j]));
  }
  if (t_out) {
#pragma unroll
    for (int i = 0; i < 3; ++i) t_out[i] = fmaf(R[3 * i + 2], dt[2], fmaf(R[3 * i + 1], dt[1], R[3 * i] * dt[0])) + t[i];
  }
}

// x[ch] of one crop from the pooling's T tile partials (rows of `pitch` floats): one ascending chain from tile 0
OBJ_HD float tile_chain(const float *part_ch, int T, size_t pitch) {
  float acc = part_ch[0];
  for (int s = 1; s < T; ++s) acc = acc + part_ch[(size_t)s * pitch];
  return acc;
}
