// ortho9d.h -- the factors of ortho9d2matrix (models/DCL_Net.py:15-36), shared by the projection (dense.hip: ortho9d_one) and its
// gradient (rotation_grad.hip), on the device and on the host.
//
// M = the three raw axes, each divided by (|r| + 1e-8) in fp32, as columns.  One-sided Jacobi SVD in fp64 (the reference calls a
// batched LAPACK/MAGMA gesdd, ms-scale latency): M V = U Sigma, columns sorted by descending singular value.  The projection is
//     R = u1 v1^T + u2 v2^T + det(V) (u1 x u2) v3^T = U' V'^T,   U' = [u1, u2, u1 x u2],  V' = [v1, v2, det(V) v3],
// both proper rotations (sign-ambiguity free), and M = U' diag(s1, s2, s3') V'^T with the SIGNED s3' = det(V) (u1 x u2) . (M v3).
// Every translation unit that includes this is built with -ffp-contract=off: the operations and their order below are the bits
// of dcl_ortho9d_to_matrix.
#pragma once
#include <math.h>

struct Ortho9dFactors {
  double u1[3], u2[3], u3[3];      // U' by columns; u2 (and u3) are NaN where the second singular value is exactly 0
  double v1[3], v2[3], v3[3];      // V by columns, sorted; V' = [v1, v2, detV * v3]
  double detV;                     // +1 or -1
  double s1, s2, s3;               // singular values, descending, all >= 0
  double a3[3];                    // M v3 (the unnormalised third left vector): s3' = detV * (u3 . a3)
  float len[3], mag[3];            // per raw axis: |r| and |r| + 1e-8 (fp32, utils/transform3D.py:18-20)
};

// o9: the crop's nine values, axis c at o9[3c .. 3c+2].  At most 30 sweeps.
__host__ __device__ inline void ortho9d_factors(const float *__restrict__ o9, Ortho9dFactors &f) {
  double A[3][3], V[3][3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float x = o9[c * 3], y = o9[c * 3 + 1], z = o9[c * 3 + 2];
    const float len = sqrtf((x * x + y * y) + z * z);
    const float mag = len + 1e-8f;                                  // utils/transform3D.py:18-20 (fp32)
    f.len[c] = len; f.mag[c] = mag;
    A[0][c] = (double)(x / mag); A[1][c] = (double)(y / mag); A[2][c] = (double)(z / mag);
#pragma unroll
    for (int r = 0; r < 3; ++r) V[r][c] = r == c ? 1.0 : 0.0;
  }
  for (int sweep = 0; sweep < 30; ++sweep) {
    double off = 0.0;
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int q = p + 1; q < 3; ++q) {
        double alpha = 0, beta = 0, gamma = 0;
#pragma unroll
        for (int r = 0; r < 3; ++r) { alpha += A[r][p] * A[r][p]; beta += A[r][q] * A[r][q]; gamma += A[r][p] * A[r][q]; }
        off = fmax(off, fabs(gamma) / sqrt(alpha * beta + 1e-300));
        if (fabs(gamma) < 1e-300) continue;
        const double zeta = (beta - alpha) / (2.0 * gamma);
        const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          const double ap = A[r][p], aq = A[r][q];
          A[r][p] = cs * ap - sn * aq; A[r][q] = sn * ap + cs * aq;
          const double vp = V[r][p], vq = V[r][q];
          V[r][p] = cs * vp - sn * vq; V[r][q] = sn * vp + cs * vq;
        }
      }
    if (off < 1e-15) break;
  }
  // sort the three (column of A, column of V) pairs by descending singular value with explicit swaps -- no
  // dynamically indexed local arrays, so the kernels need no scratch memory
  double a0[3] = {A[0][0], A[1][0], A[2][0]}, a1[3] = {A[0][1], A[1][1], A[2][1]}, a2[3] = {A[0][2], A[1][2], A[2][2]};
  double v0[3] = {V[0][0], V[1][0], V[2][0]}, v1[3] = {V[0][1], V[1][1], V[2][1]}, v2[3] = {V[0][2], V[1][2], V[2][2]};
  double s0 = sqrt(a0[0] * a0[0] + a0[1] * a0[1] + a0[2] * a0[2]);
  double s1 = sqrt(a1[0] * a1[0] + a1[1] * a1[1] + a1[2] * a1[2]);
  double s2 = sqrt(a2[0] * a2[0] + a2[1] * a2[1] + a2[2] * a2[2]);
#define DCL_SWAP_COLS(sa, sb, aa, ab, va, vb)                                  \
  if (sa < sb) {                                                               \
    double t_ = sa; sa = sb; sb = t_;                                          \
    for (int r_ = 0; r_ < 3; ++r_) {                                           \
      t_ = aa[r_]; aa[r_] = ab[r_]; ab[r_] = t_;                               \
      t_ = va[r_]; va[r_] = vb[r_]; vb[r_] = t_;                               \
    }                                                                          \
  }
  DCL_SWAP_COLS(s0, s1, a0, a1, v0, v1)
  DCL_SWAP_COLS(s1, s2, a1, a2, v1, v2)
  DCL_SWAP_COLS(s0, s1, a0, a1, v0, v1)
#undef DCL_SWAP_COLS
#pragma unroll
  for (int r = 0; r < 3; ++r) { f.u1[r] = a0[r] / s0; f.u2[r] = a1[r] / s1; }
  f.u3[0] = f.u1[1] * f.u2[2] - f.u1[2] * f.u2[1];
  f.u3[1] = f.u1[2] * f.u2[0] - f.u1[0] * f.u2[2];
  f.u3[2] = f.u1[0] * f.u2[1] - f.u1[1] * f.u2[0];
  f.detV = v0[0] * (v1[1] * v2[2] - v1[2] * v2[1]) - v0[1] * (v1[0] * v2[2] - v1[2] * v2[0]) +
           v0[2] * (v1[0] * v2[1] - v1[1] * v2[0]);
#pragma unroll
  for (int r = 0; r < 3; ++r) { f.v1[r] = v0[r]; f.v2[r] = v1[r]; f.v3[r] = v2[r]; f.a3[r] = a2[r]; }
  f.s1 = s0; f.s2 = s1; f.s3 = s2;
}

// R (3,3) row-major = U' V'^T, rounded to fp32
__host__ __device__ inline void ortho9d_compose(const Ortho9dFactors &f, float *__restrict__ R) {
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c)
      R[r * 3 + c] = (float)(f.u1[r] * f.v1[c] + f.u2[r] * f.v2[c] + f.detV * f.u3[r] * f.v3[c]);
}

// The gradient of R = ortho9d2matrix(o9) for one crop: G = dL/dR (3,3) row-major -> out = dL/do9 (9), in fp64, rounded once.
//   B = U'^T G V',  Y_ij = (B_ij - B_ji) / (s'_i + s'_j) (i != j; 0 where |s'_i + s'_j| <= 1e-12 s1),  dL/dM = U' Y V'^T,
// then through the normalisation of every raw axis r with g = its column of dL/dM:
//   dL/dr = g / mag - r (r . g) / (|r| mag^2)          (second term 0 where |r| = 0).
// The denominators are sums of singular values (about 2 for near-orthonormal axes), where differentiating U and V apart
// divides by differences of their squares.  A non-finite o9 or G gives nine NaN.  Rank-deficient M (parallel or zero axes)
// leaves U' incomplete; any orthonormal completion serves, since the terms it could change are the guarded ones or multiply
// a zero singular value's direction that the projection itself does not define -- the outputs stay finite.
__host__ __device__ inline void ortho9d_grad(const float *__restrict__ o9, const float *__restrict__ G, float *__restrict__ out) {
  bool finite = true;
#pragma unroll
  for (int k = 0; k < 9; ++k) finite = finite && isfinite(o9[k]) && isfinite(G[k]);
  if (!finite) {
#pragma unroll
    for (int k = 0; k < 9; ++k) out[k] = NAN;
    return;
  }
  Ortho9dFactors f;
  ortho9d_factors(o9, f);
  double u1[3] = {f.u1[0], f.u1[1], f.u1[2]}, u2[3] = {f.u2[0], f.u2[1], f.u2[2]}, u3[3] = {f.u3[0], f.u3[1], f.u3[2]};
  if (!(f.s1 > 0.0)) { u1[0] = 1.0; u1[1] = 0.0; u1[2] = 0.0; }                   // M = 0
  if (!(f.s2 > 0.0)) {                                                            // rank <= 1: u2 = any unit vector across u1
    const double ax = fabs(u1[0]), ay = fabs(u1[1]), az = fabs(u1[2]);
    const bool kx = ax <= ay && ax <= az, ky = !kx && ay <= az;                   // the axis u1 leans on least
    const double d = kx ? u1[0] : ky ? u1[1] : u1[2];
    double w[3] = {(kx ? 1.0 : 0.0) - d * u1[0], (ky ? 1.0 : 0.0) - d * u1[1], ((kx || ky) ? 0.0 : 1.0) - d * u1[2]};
    const double n = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
#pragma unroll
    for (int r = 0; r < 3; ++r) u2[r] = w[r] / n;
    u3[0] = u1[1] * u2[2] - u1[2] * u2[1];
    u3[1] = u1[2] * u2[0] - u1[0] * u2[2];
    u3[2] = u1[0] * u2[1] - u1[1] * u2[0];
  }
  const double U[3][3] = {{u1[0], u2[0], u3[0]}, {u1[1], u2[1], u3[1]}, {u1[2], u2[2], u3[2]}};          // U[r][i]
  const double V[3][3] = {{f.v1[0], f.v2[0], f.detV * f.v3[0]}, {f.v1[1], f.v2[1], f.detV * f.v3[1]},
                          {f.v1[2], f.v2[2], f.detV * f.v3[2]}};                                         // V[c][j]
  const double sg[3] = {f.s1, f.s2, f.detV * (u3[0] * f.a3[0] + u3[1] * f.a3[1] + u3[2] * f.a3[2])};
  double T[3][3], B[3][3], Y[3][3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int j = 0; j < 3; ++j) T[r][j] = (double)G[r * 3] * V[0][j] + (double)G[r * 3 + 1] * V[1][j] + (double)G[r * 3 + 2] * V[2][j];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) B[i][j] = U[0][i] * T[0][j] + U[1][i] * T[1][j] + U[2][i] * T[2][j];
  const double tiny = 1e-12 * f.s1;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double den = sg[i] + sg[j];
      Y[i][j] = (i == j || fabs(den) <= tiny) ? 0.0 : (B[i][j] - B[j][i]) / den;
    }
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int j = 0; j < 3; ++j) T[r][j] = U[r][0] * Y[0][j] + U[r][1] * Y[1][j] + U[r][2] * Y[2][j];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    double g[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) g[r] = T[r][0] * V[c][0] + T[r][1] * V[c][1] + T[r][2] * V[c][2];       // dL/dM[r][c]
    const double x = o9[c * 3], y = o9[c * 3 + 1], z = o9[c * 3 + 2];
    const double len = f.len[c], mag = f.mag[c];
    const double k = len > 0.0 ? (x * g[0] + y * g[1] + z * g[2]) / (len * mag * mag) : 0.0;
    out[c * 3] = (float)(g[0] / mag - x * k);
    out[c * 3 + 1] = (float)(g[1] / mag - y * k);
    out[c * 3 + 2] = (float)(g[2] / mag - z * k);
  }
}
