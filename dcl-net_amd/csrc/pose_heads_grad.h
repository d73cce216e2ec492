// pose_heads_grad.h -- the summation orders of the two pose heads in training (pose_heads_grad.hip), shared by the kernels and
// their host twins: every routine here is __host__ __device__, and the library is built with -ffp-contract=off, so the
// operations below are the operations executed, in this order, on either side.
//
// A head is three layers, z = in W^T + bias with W (O, Kd) as the convolution registers it, ReLU behind the first two.
//
// PINNED ORDERS.  Each is a function of the layer widths alone: not of b, of the grid or of which outputs are asked for.
//
//   z[r][o]      a dot along the row of `in`: 256 slots, slot k = 4 l + e of lane l < 64 runs ONE fmaf chain from +0 over the
//                columns k, k + 256, k + 512, k + 768 < Kd ascending, s = fmaf(in[r][c], W[o][c], s); a lane folds its slots as
//                (s0 + s1) + (s2 + s3); the 64 lane values by a butterfly with strides 32, 16, ..., 1; z = v + bias[o];
//                h = z > 0 ? z : 0 behind the first two layers.
//   dW[o][k]     ONE fmaf chain from +0, rows ascending:  p = fmaf(dz[r][o], in[r][k], p).
//   db[o]        p = p + dz[r][o] from +0, rows ascending.
//   d in[r][k]   the layer's outputs are cut into chunks of kPhChunk = DCL_POSE_TRAIN_CHUNK outputs (the last may be short); a
//                chunk is ONE fmaf chain from +0, outputs ascending:  p = fmaf(dz[r][o], W[o][k], p); the chunks are added
//                ascending from the first chunk's value.  Layers 2 and 3: dz_below = h_below > 0 ? that sum : 0.  Layer 1:
//                dx = R + T, the rotation head's sum and the translation head's, each formed as above.
// A row's values depend on that row alone (dW, db aside): a crop gives the same o9, t3 and dx bits alone as inside a batch.
#pragma once
#include "conf_pool_grad.h"                          // CPG_HD, cpg_aligned16

constexpr int kPhMaxWidth = DCL_POSE_TRAIN_MAX_WIDTH;   // widest layer input (the W row of an output lives in a wave's registers)
constexpr int kPhMaxOut = DCL_POSE_TRAIN_MAX_OUT;       // widest last layer
constexpr int kPhChunk = DCL_POSE_TRAIN_CHUNK;          // outputs per fmaf chain of an input gradient
constexpr int kPhLanes = 64, kPhVec = 4, kPhSlots = kPhLanes * kPhVec;
constexpr int kPhSteps = kPhMaxWidth / kPhSlots;        // 4 columns steps of 256

CPG_HD int ph_nchunks(int O) { return (O + kPhChunk - 1) / kPhChunk; }

// z: lane `lane`'s four slots of one row's dot with one weight row (Kd a multiple of 4)
CPG_HD void ph_dot_lane(const float *in, const float *w, int Kd, int lane, float *acc) {
  acc[0] = acc[1] = acc[2] = acc[3] = 0.0f;
  for (int c = kPhVec * lane; c < Kd; c += kPhSlots) {
#pragma unroll
    for (int e = 0; e < kPhVec; ++e) acc[e] = fmaf(in[c + e], w[c + e], acc[e]);
  }
}
CPG_HD float ph_lane_fold(const float *acc) { return (acc[0] + acc[1]) + (acc[2] + acc[3]); }
inline float ph_butterfly_host(float *v) {
  for (int s = kPhLanes / 2; s >= 1; s >>= 1) {
    float t[kPhLanes];
    for (int l = 0; l < kPhLanes; ++l) t[l] = v[l] + v[l ^ s];
    for (int l = 0; l < kPhLanes; ++l) v[l] = t[l];
  }
  return v[0];
}
