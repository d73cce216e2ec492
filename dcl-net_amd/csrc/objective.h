// objective.h -- the per-point arithmetic and the reduction order of the training objective (objective.hip), shared by the
// kernels and their host twins: every routine here is __host__ __device__, and the library is built with -ffp-contract=off,
// so the operations below are the operations executed, in this order, on either side.
//
// Squared distance: fmaf(dz,dz, fmaf(dy,dy, dx*dx)) of fp32 differences, sqrtf once (chamfer.hip's association).
//
// PINNED ORDER of every per-crop sum (rigid-points gradient, objective): one workgroup of kObjLanes = 256 lanes per crop;
// lane l adds the terms of points l, l + 256, l + 512, ... in ascending order into its own accumulator, starting from 0;
// the 256 accumulators are then folded by a tree with strides 128, 64, ..., 1 (slot l += slot l + stride for l < stride).
// Crops are added afterwards in ascending crop order, starting from 0.  No float atomics anywhere.
//
// conf <= 0 is NOT guarded: logf and the division give what torch.log and its backward give (nan / -inf / inf).
// sym is the float multiplier of the formula (1 - sym and sym both appear); the error bounds quoted in DESIGN.md hold for the
// flags the loaders produce, 0 and 1.
#pragma once
#include <math.h>
#include <stddef.h>

#define OBJ_HD __host__ __device__ __forceinline__

constexpr int kObjLanes = 256;
// per-crop sums: [pose, Xo, Yc, conf over the Xo half of the row, conf over the Yc half]
constexpr int kObjSums = 5;

// ---- rigid transform of one point -------------------------------------------------------------------------------------
// inverse == 0: o = R p + t, row r as fmaf(R_r2,p_2, fmaf(R_r1,p_1, R_r0*p_0)) + t_r
// inverse == 1: o = R^T (p - t), q = p - t, column c as fmaf(R_2c,q_2, fmaf(R_1c,q_1, R_0c*q_0))
OBJ_HD void obj_rigid_point(const float *R, const float *t, int inverse, const float *p, float *o) {
  if (!inverse) {
    const float p0 = p[0], p1 = p[1], p2 = p[2];
#pragma unroll
    for (int r = 0; r < 3; ++r) o[r] = fmaf(R[3 * r + 2], p2, fmaf(R[3 * r + 1], p1, R[3 * r] * p0)) + t[r];
  } else {
    const float q0 = p[0] - t[0], q1 = p[1] - t[1], q2 = p[2] - t[2];
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = fmaf(R[6 + c], q2, fmaf(R[3 + c], q1, R[c] * q0));
  }
}

// One point's share of the gradient: acc[0..8] is g_R (row-major), acc[9..11] is g_t; gp (3 floats, may be NULL) is g_p.
// inverse == 0: g_R[r][c] = fmaf(g_r, p_c, g_R[r][c]);  g_t[r] += g_r;                 g_p = R^T g
// inverse == 1: g_R[r][c] = fmaf(q_r, g_c, g_R[r][c]);  g_t[r] -= (R g)_r;             g_p = R g      (q = p - t)
// with (R^T g)_c = fmaf(R_2c,g_2, fmaf(R_1c,g_1, R_0c*g_0)) and (R g)_r = fmaf(R_r2,g_2, fmaf(R_r1,g_1, R_r0*g_0)).
OBJ_HD void obj_rigid_point_grad(const float *R, const float *t, int inverse, const float *p, const float *g, float *acc,
                                 float *gp) {
  const float g0 = g[0], g1 = g[1], g2 = g[2];
  if (!inverse) {
    const float gg[3] = {g0, g1, g2};
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[3 * r + c] = fmaf(gg[r], p[c], acc[3 * r + c]);
      acc[9 + r] += gg[r];
    }
    if (gp) {
#pragma unroll
      for (int c = 0; c < 3; ++c) gp[c] = fmaf(R[6 + c], g2, fmaf(R[3 + c], g1, R[c] * g0));
    }
  } else {
    const float q[3] = {p[0] - t[0], p[1] - t[1], p[2] - t[2]};
    const float gg[3] = {g0, g1, g2};
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[3 * r + c] = fmaf(q[r], gg[c], acc[3 * r + c]);
      const float gq = fmaf(R[3 * r + 2], g2, fmaf(R[3 * r + 1], g1, R[3 * r] * g0));
      acc[9 + r] -= gq;
      if (gp) gp[r] = gq;
    }
  }
}

// what lane `lane` of crop `crop`'s workgroup accumulates: points lane, lane + 256, ... ascending
OBJ_HD void obj_rigid_lane_grad(int n, const float *pts, const float *R, const float *t, int inverse, const float *g_out,
                                float *g_pts, int crop, int lane, float *acc) {
  const float *Rc = R + (size_t)crop * 9, *tc = t + (size_t)crop * 3;
#pragma unroll
  for (int k = 0; k < 12; ++k) acc[k] = 0.0f;
  for (int i = lane; i < n; i += kObjLanes) {
    const size_t o = ((size_t)crop * n + i) * 3;
    obj_rigid_point_grad(Rc, tc, inverse, pts + o, g_out + o, acc, g_pts ? g_pts + o : nullptr);
  }
}

// ---- the objective ----------------------------------------------------------------------------------------------------
// d = a - b (three differences, kept for the backward form), returns |a - b|
OBJ_HD float obj_dist(const float *a, const float *b, float *d) {
  d[0] = a[0] - b[0]; d[1] = a[1] - b[1]; d[2] = a[2] - b[2];
  return sqrtf(fmaf(d[2], d[2], fmaf(d[1], d[1], d[0] * d[0])));
}

// everything one call reads and writes; the optional set (Yc .. cd_Yc_tp, L and their gradients) is all there or all NULL
struct ObjArgs {
  int b, n, full;
  const float *posed, *posed_gt, *Yc, *cano_pred, *cano_gt, *Xo, *conf, *sym;
  const float *cd_pose_pt, *cd_pose_tp, *cd_Xo_pt, *cd_Xo_tp, *cd_Yc_pt, *cd_Yc_tp;
  float *L;                         // forward: written;  backward: read (through Lr)
  const float *Lr, *g_packed;
  float *g_posed, *g_Xo, *g_Yc, *g_conf, *g_cd_pose_pt, *g_cd_pose_tp, *g_cd_Xo_pt, *g_cd_Xo_tp, *g_cd_Yc_pt, *g_cd_Yc_tp;
};

// Per-point terms of crop `crop` with s = sym[crop], cd(a, b) = 0.5f * (a + b) of the two Chamfer halves:
//   pose_i = (1 - s) * |posed_i - posed_gt_i| + s * cd_pose_i
//   LXo_i  = (1 - s) * |Xo_i - cano_gt_i|  + (0.5f * s) * (cd_Xo_i + |Xo_i - cano_pred_i|)
//   LYc_i  = (1 - s) * |Yc_i - posed_gt_i| + (0.5f * s) * (cd_Yc_i + |Yc_i - posed_i|)
//   conf terms: LXo_i * conf[i] - 0.01f * logf(conf[i])  and  LYc_i * conf[n + i] - 0.01f * logf(conf[n + i])
// L[crop][i] = LXo_i, L[crop][n + i] = LYc_i.  acc[kObjSums] gets this lane's sums (order: see the top of the file).
OBJ_HD void obj_lane_fwd(const ObjArgs &a, int crop, int lane, float *acc) {
  const int n = a.n;
  const float s = a.sym[crop], s1 = 1.0f - s, sh = 0.5f * s;
  float d[3];
#pragma unroll
  for (int k = 0; k < kObjSums; ++k) acc[k] = 0.0f;
  for (int i = lane; i < n; i += kObjLanes) {
    const size_t r = (size_t)crop * n + i, o = r * 3;
    acc[0] += s1 * obj_dist(a.posed + o, a.posed_gt + o, d) + s * (0.5f * (a.cd_pose_pt[r] + a.cd_pose_tp[r]));
    if (!a.full) continue;
    const float lxo = s1 * obj_dist(a.Xo + o, a.cano_gt + o, d) +
                      sh * (0.5f * (a.cd_Xo_pt[r] + a.cd_Xo_tp[r]) + obj_dist(a.Xo + o, a.cano_pred + o, d));
    const float lyc = s1 * obj_dist(a.Yc + o, a.posed_gt + o, d) +
                      sh * (0.5f * (a.cd_Yc_pt[r] + a.cd_Yc_tp[r]) + obj_dist(a.Yc + o, a.posed + o, d));
    const size_t jx = (size_t)crop * 2 * n + i, jy = jx + n;
    a.L[jx] = lxo;
    a.L[jy] = lyc;
    acc[1] += lxo;
    acc[2] += lyc;
    const float cx = a.conf[jx], cy = a.conf[jy];
    acc[3] += lxo * cx - 0.01f * logf(cx);
    acc[4] += lyc * cy - 0.01f * logf(cy);
  }
}

// column k of the (b, kObjSums) per-crop sums, crops ascending from 0
OBJ_HD float obj_column_sum(const float *crop_sums, int b, int k) {
  float tot = 0.0f;
  for (int c = 0; c < b; ++c) tot += crop_sums[(size_t)c * kObjSums + k];
  return tot;
}

// packed = [loss_pose, loss_Xo, loss_Yc, loss_conf, loss_all] from the five column sums:
//   loss_pose = tot0 / (b n), loss_Xo = tot1 / (b n), loss_Yc = tot2 / (b n), loss_conf = (tot3 + tot4) / (2 b n)
//   loss_all = ((loss_pose + 5 * loss_Xo) + loss_Yc) + loss_conf;   pose-only form: [loss_pose, 0, 0, 0, loss_pose]
OBJ_HD void obj_finalize(const float *tot, int b, int n, int full, float *packed) {
  const float np = (float)((double)b * n), nc = (float)(2.0 * b * n);
  const float pose = tot[0] / np;
  packed[0] = pose;
  if (!full) {
    packed[1] = 0.0f; packed[2] = 0.0f; packed[3] = 0.0f; packed[4] = pose;
    return;
  }
  const float xo = tot[1] / np, yc = tot[2] / np, cf = (tot[3] + tot[4]) / nc;
  packed[1] = xo; packed[2] = yc; packed[3] = cf;
  packed[4] = ((pose + 5.0f * xo) + yc) + cf;
}

// Backward.  With g = the upstream gradient of packed, the weights (formed here, on the device, per lane):
//   W_pose = (g0 + g4) / (b n), W_Xo = fmaf(5, g4, g1) / (b n), W_Yc = (g2 + g4) / (b n), W_conf = (g3 + g4) / (2 b n)
// and per point, with u_k(a, b) = (k / |a - b|) (a - b), 0 at distance 0 (torch.norm's subgradient):
//   g_posed_i = u_{W_pose (1-s)}(posed_i, posed_gt_i)                       (the detached uses of posed give nothing)
//   g_Xo_i    = u_{W_Xo (1-s)}(Xo_i, cano_gt_i)  + u_{W_Xo 0.5 s}(Xo_i, cano_pred_i)      second term folded in by fmaf
//   g_Yc_i    = u_{W_Yc (1-s)}(Yc_i, posed_gt_i) + u_{W_Yc 0.5 s}(Yc_i, posed_i)
//   g_conf_j  = W_conf * (L_j - 0.01f / conf_j)                                            (L is detached in the formula)
//   g_cd_pose_{pt,tp}_i = (W_pose s) * 0.5,  g_cd_Xo_{pt,tp}_i = (W_Xo 0.5 s) * 0.5,  g_cd_Yc_{pt,tp}_i = (W_Yc 0.5 s) * 0.5
OBJ_HD void obj_scaled_unit(float k, const float *a, const float *b, float *w, float *d) {
  const float r = obj_dist(a, b, d);
  *w = r > 0.0f ? k / r : 0.0f;
}

OBJ_HD void obj_point_bwd(const ObjArgs &a, int crop, int i) {
  const int n = a.n;
  const float np = (float)((double)a.b * n), nc = (float)(2.0 * a.b * n);
  const float *g = a.g_packed;
  const float s = a.sym[crop], s1 = 1.0f - s, sh = 0.5f * s;
  const size_t r = (size_t)crop * n + i, o = r * 3;
  float w, d[3];
  const float Wp = (g[0] + g[4]) / np;
  obj_scaled_unit(Wp * s1, a.posed + o, a.posed_gt + o, &w, d);
  a.g_posed[o] = w * d[0]; a.g_posed[o + 1] = w * d[1]; a.g_posed[o + 2] = w * d[2];
  const float gcp = (Wp * s) * 0.5f;
  a.g_cd_pose_pt[r] = gcp; a.g_cd_pose_tp[r] = gcp;
  if (!a.full) return;
  const float Wx = fmaf(5.0f, g[4], g[1]) / np, Wy = (g[2] + g[4]) / np, Wc = (g[3] + g[4]) / nc;
  float w2, d2[3];
  obj_scaled_unit(Wx * s1, a.Xo + o, a.cano_gt + o, &w, d);
  obj_scaled_unit(Wx * sh, a.Xo + o, a.cano_pred + o, &w2, d2);
#pragma unroll
  for (int c = 0; c < 3; ++c) a.g_Xo[o + c] = fmaf(w2, d2[c], w * d[c]);
  obj_scaled_unit(Wy * s1, a.Yc + o, a.posed_gt + o, &w, d);
  obj_scaled_unit(Wy * sh, a.Yc + o, a.posed + o, &w2, d2);
#pragma unroll
  for (int c = 0; c < 3; ++c) a.g_Yc[o + c] = fmaf(w2, d2[c], w * d[c]);
  const float gcx = (Wx * sh) * 0.5f, gcy = (Wy * sh) * 0.5f;
  a.g_cd_Xo_pt[r] = gcx; a.g_cd_Xo_tp[r] = gcx;
  a.g_cd_Yc_pt[r] = gcy; a.g_cd_Yc_tp[r] = gcy;
  const size_t jx = (size_t)crop * 2 * n + i, jy = jx + n;
  a.g_conf[jx] = Wc * (a.Lr[jx] - 0.01f / a.conf[jx]);
  a.g_conf[jy] = Wc * (a.Lr[jy] - 0.01f / a.conf[jy]);
}

// the host's copy of the fold: strides 128 .. 1 over kObjLanes slots (the kernels do the same through LDS)
inline float obj_tree_host(float *slot) {
  for (int s = kObjLanes / 2; s >= 1; s >>= 1)
    for (int l = 0; l < s; ++l) slot[l] += slot[l + s];
  return slot[0];
}
