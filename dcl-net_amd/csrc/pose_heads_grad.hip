// pose_heads_grad.hip -- the two pose heads (rotation 1024 -> 512 -> 128 -> 9, translation ... -> 3) on the b pooled rows of a
// training step, forward and backward (models/DCL_Net.py, models/refiner.py: train_heads = "kernels"; autograd.PoseHeadsFn).
// The weights are read as the convolutions register them, (out, in): nothing is folded or transposed per step.  Both heads
// share every launch (grid dimension y = head):
//   k_ph_fwd        one launch per layer: a wave holds the weight rows of two outputs in registers and walks the b rows, eight
//                   at a time, so a weight matrix is read once per launch whatever b is
//   k_ph_bwd_layer  one launch per layer, from that layer's dz alone: dW and db (a wave per four outputs x 256 columns, rows
//                   ascending) and the chunk partials of the input gradient (the weight tile of a chunk staged once in LDS)
//   k_ph_bwd_sum    adds a layer's chunk partials in order and applies the ReLU mask of the stored activation below (layer 1:
//                   adds the two heads' sums into dx)
// Forward 3 launches, backward at most 6.  pose_heads_grad.h pins every summation order and is shared with the *_host entry
// points.  No atomics.  The eval kernels (dense.hip: k_heads_l1 / k_heads_l23) use folded, transposed weights and other slice
// orders: train-mode values are NOT their bits.
#include <vector>

#include "common.h"
#include "pose_heads_grad.h"

namespace {

struct PhFwdArgs {
  const float *in[2], *W[2], *bias[2];
  float *out[2];
  int O[2];
};
constexpr int kFwdOut = 2;                                    // outputs per wave of the forward
constexpr int kFwdRows = 8;                                   // rows whose loads and butterflies a wave keeps in flight

__device__ __forceinline__ float4 ph_zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }

__global__ __launch_bounds__(256) void k_ph_fwd(PhFwdArgs a, int b, int Kd, int relu) {
  const int head = blockIdx.y, lane = threadIdx.x & (kPhLanes - 1), wave = threadIdx.x / kPhLanes;
  const int O = a.O[head];
  const int o0 = ((int)blockIdx.x * 4 + wave) * kFwdOut;
  if (o0 >= O) return;                                       // whole waves leave; no barrier below
  const float *__restrict__ W = a.W[head];
  const float *__restrict__ in = a.in[head];
  const float *__restrict__ bias = a.bias[head];
  float *__restrict__ out = a.out[head];
  float4 w[kFwdOut][kPhSteps];
#pragma unroll
  for (int i = 0; i < kFwdOut; ++i)
#pragma unroll
    for (int q = 0; q < kPhSteps; ++q) {
      const int c = kPhVec * lane + kPhSlots * q;
      w[i][q] = o0 + i < O && c < Kd ? *reinterpret_cast<const float4 *>(W + (size_t)(o0 + i) * Kd + c) : ph_zero4();
    }
  // eight rows at a time: a wave walks the rows alone, so their loads are issued together and their butterflies run side by
  // side, stride by stride (a row past the end is a row of zeros that is not stored)
  for (int r0 = 0; r0 < b; r0 += kFwdRows) {
    float4 xv[kFwdRows][kPhSteps];
#pragma unroll
    for (int u = 0; u < kFwdRows; ++u)
#pragma unroll
      for (int q = 0; q < kPhSteps; ++q) {
        const int c = kPhVec * lane + kPhSlots * q;
        xv[u][q] = r0 + u < b && c < Kd ? *reinterpret_cast<const float4 *>(in + (size_t)(r0 + u) * Kd + c) : ph_zero4();
      }
    float v[kFwdRows][kFwdOut];
#pragma unroll
    for (int u = 0; u < kFwdRows; ++u)
#pragma unroll
      for (int i = 0; i < kFwdOut; ++i) {
        float acc[kPhVec] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int q = 0; q < kPhSteps; ++q)
          if (kPhVec * lane + kPhSlots * q < Kd) {           // a column that does not exist adds nothing
            acc[0] = fmaf(xv[u][q].x, w[i][q].x, acc[0]);
            acc[1] = fmaf(xv[u][q].y, w[i][q].y, acc[1]);
            acc[2] = fmaf(xv[u][q].z, w[i][q].z, acc[2]);
            acc[3] = fmaf(xv[u][q].w, w[i][q].w, acc[3]);
          }
        v[u][i] = ph_lane_fold(acc);
      }
#pragma unroll
    for (int s = kPhLanes / 2; s >= 1; s >>= 1)
#pragma unroll
      for (int u = 0; u < kFwdRows; ++u)
#pragma unroll
        for (int i = 0; i < kFwdOut; ++i) v[u][i] = v[u][i] + __shfl_xor(v[u][i], s, kPhLanes);
    // lane 2 u + i stores row r0 + u of output o0 + i
    float mine = 0.0f;
#pragma unroll
    for (int u = 0; u < kFwdRows; ++u)
#pragma unroll
      for (int i = 0; i < kFwdOut; ++i) mine = lane == kFwdOut * u + i ? v[u][i] : mine;
    const int u = lane / kFwdOut, i = lane % kFwdOut;
    if (lane < kFwdRows * kFwdOut && r0 + u < b && o0 + i < O) {
      const float z = mine + bias[o0 + i];
      out[(size_t)(r0 + u) * O + o0 + i] = relu ? (z > 0.0f ? z : 0.0f) : z;
    }
  }
}

struct PhBwdArgs {
  const float *W[2];       // (O, Kd)
  const float *dz[2];      // (b, O), NULL = all zero
  const float *in[2];      // (b, Kd): the layer's input
  float *dW[2], *db[2];    // NULL = not wanted
  float *part[2];          // (chunks, b, Kd): the chunk partials of the input gradient, NULL = not wanted
  int O[2];
};
constexpr int kBwdOut = 4;                                    // outputs per wave of the dW part

// blocks [0, nA): dW / db, a wave per (four outputs, 256 columns); blocks [nA, ..): a workgroup per (chunk of outputs, 256 columns)
__global__ __launch_bounds__(256) void k_ph_bwd_layer(PhBwdArgs a, int b, int Kd, int ktiles, int nA) {
  __shared__ float4 sW[kPhChunk][kPhLanes];
  const int head = blockIdx.y, lane = threadIdx.x & (kPhLanes - 1), wave = threadIdx.x / kPhLanes;
  const int O = a.O[head];
  const float *__restrict__ dz = a.dz[head];
  if ((int)blockIdx.x < nA) {
    const int wid = (int)blockIdx.x * 4 + wave;
    const int o0 = wid / ktiles * kBwdOut, kt = wid % ktiles;
    float *__restrict__ dW = a.dW[head];
    float *__restrict__ db = a.db[head];
    if (o0 >= O || (!dW && !db)) return;                     // whole waves leave; no barrier on this side
    const float *__restrict__ in = a.in[head];
    const int c = kt * kPhSlots + kPhVec * lane;
    float4 acc[kBwdOut];
    float accb[kBwdOut];
#pragma unroll
    for (int i = 0; i < kBwdOut; ++i) acc[i] = ph_zero4(), accb[i] = 0.0f;
#pragma unroll 8
    for (int r = 0; r < b; ++r) {
      const float4 xv = c < Kd ? *reinterpret_cast<const float4 *>(in + (size_t)r * Kd + c) : ph_zero4();
#pragma unroll
      for (int i = 0; i < kBwdOut; ++i) {
        const float d = dz && o0 + i < O ? dz[(size_t)r * O + o0 + i] : 0.0f;
        acc[i].x = fmaf(d, xv.x, acc[i].x);
        acc[i].y = fmaf(d, xv.y, acc[i].y);
        acc[i].z = fmaf(d, xv.z, acc[i].z);
        acc[i].w = fmaf(d, xv.w, acc[i].w);
        accb[i] = accb[i] + d;
      }
    }
    if (dW && c < Kd) {
#pragma unroll
      for (int i = 0; i < kBwdOut; ++i)
        if (o0 + i < O) *reinterpret_cast<float4 *>(dW + (size_t)(o0 + i) * Kd + c) = acc[i];
    }
    if (db && kt == 0 && lane < kBwdOut && o0 + lane < O) {
      float v = accb[0];
#pragma unroll
      for (int i = 1; i < kBwdOut; ++i) v = lane == i ? accb[i] : v;
      db[o0 + lane] = v;
    }
    return;
  }
  const int idx = (int)blockIdx.x - nA;
  const int kt = idx % ktiles, q = idx / ktiles, o0 = q * kPhChunk;
  float *__restrict__ part = a.part[head];
  if (o0 >= O || !part) return;                              // the whole workgroup leaves, before the barrier
  const int no = O - o0 < kPhChunk ? O - o0 : kPhChunk;
  const float *__restrict__ W = a.W[head];
  for (int f = threadIdx.x; f < kPhChunk * kPhLanes; f += 256) {
    const int row = f / kPhLanes, c4 = f % kPhLanes, c = kt * kPhSlots + kPhVec * c4;
    sW[row][c4] = row < no && c < Kd ? *reinterpret_cast<const float4 *>(W + (size_t)(o0 + row) * Kd + c) : ph_zero4();
  }
  __syncthreads();
  const int c = kt * kPhSlots + kPhVec * lane;
  if (c >= Kd) return;
  for (int r = wave; r < b; r += 4) {
    float4 p = ph_zero4();
    for (int o = 0; o < no; ++o) {
      const float d = dz ? dz[(size_t)r * O + o0 + o] : 0.0f;
      const float4 wv = sW[o][lane];
      p.x = fmaf(d, wv.x, p.x);
      p.y = fmaf(d, wv.y, p.y);
      p.z = fmaf(d, wv.z, p.z);
      p.w = fmaf(d, wv.w, p.w);
    }
    *reinterpret_cast<float4 *>(part + ((size_t)q * b + r) * Kd + c) = p;
  }
}

__device__ __forceinline__ float4 ph_chunk_sum(const float *__restrict__ part, int nch, size_t slab, size_t at) {
  float4 t = *reinterpret_cast<const float4 *>(part + at);   // the first chunk's value starts the sum
  for (int q = 1; q < nch; ++q) {
    const float4 u = *reinterpret_cast<const float4 *>(part + (size_t)q * slab + at);
    t.x = t.x + u.x, t.y = t.y + u.y, t.z = t.z + u.z, t.w = t.w + u.w;
  }
  return t;
}

// n4 = b Kd / 4 vectors.  add_heads == 0 (grid y = head): out[head] = mask[head] > 0 ? the head's chunk sum : 0.
// add_heads == 1: out0 = head 0's chunk sum + head 1's.
__global__ __launch_bounds__(256) void k_ph_bwd_sum(const float *__restrict__ part0, const float *__restrict__ part1, int nch0,
                                                    int nch1, long long n4, const float *__restrict__ mask0,
                                                    const float *__restrict__ mask1, float *__restrict__ out0,
                                                    float *__restrict__ out1, int add_heads) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const size_t at = (size_t)i * kPhVec, slab = (size_t)n4 * kPhVec;
  if (add_heads) {
    const float4 R = ph_chunk_sum(part0, nch0, slab, at), T = ph_chunk_sum(part1, nch1, slab, at);
    *reinterpret_cast<float4 *>(out0 + at) = make_float4(R.x + T.x, R.y + T.y, R.z + T.z, R.w + T.w);
    return;
  }
  const int head = blockIdx.y;
  float4 t = ph_chunk_sum(head ? part1 : part0, head ? nch1 : nch0, slab, at);
  const float4 m = *reinterpret_cast<const float4 *>((head ? mask1 : mask0) + at);
  t.x = m.x > 0.0f ? t.x : 0.0f;
  t.y = m.y > 0.0f ? t.y : 0.0f;
  t.z = m.z > 0.0f ? t.z : 0.0f;
  t.w = m.w > 0.0f ? t.w : 0.0f;
  *reinterpret_cast<float4 *>((head ? out1 : out0) + at) = t;
}

inline bool ph_width_ok(int d) { return d >= kPhVec && d <= kPhMaxWidth && (d & 3) == 0; }
inline bool ph_dims_ok(int b, int d0, int d1, int d2, int n_rot, int n_trans) {
  return b >= 0 && ph_width_ok(d0) && ph_width_ok(d1) && ph_width_ok(d2) && n_rot >= 1 && n_rot <= kPhMaxOut && n_trans >= 1 &&
         n_trans <= kPhMaxOut;
}
inline long long ph_max(long long a, long long b) { return a > b ? a : b; }
// floats of one head's chunk partials, the largest of the three layers
inline long long ph_part_floats(int b, int d0, int d1, int d2, int n_rot, int n_trans) {
  const long long l3 = (long long)ph_nchunks(n_rot > n_trans ? n_rot : n_trans) * d2, l2 = (long long)ph_nchunks(d2) * d1,
                  l1 = (long long)ph_nchunks(d1) * d0;
  return (long long)b * ph_max(l3, ph_max(l2, l1));
}
inline long long ph_ws_floats(int b, int d0, int d1, int d2, int n_rot, int n_trans) {
  return 2 * ((long long)b * d2 + (long long)b * d1 + ph_part_floats(b, d0, d1, d2, n_rot, n_trans));
}
// the sum kernel's grid counts b Kd / 4 vectors in blocks of 256
inline bool ph_grid_ok(int b, int d0, int d1, int d2) { return (long long)b * kPhMaxWidth / 4 / 256 + 1 <= INT32_MAX; }
inline bool ph_aligned(const void *a, const void *b = nullptr, const void *c = nullptr, const void *d = nullptr) {
  return cpg_aligned16(a) && cpg_aligned16(b) && cpg_aligned16(c) && cpg_aligned16(d);
}

// one layer of the backward: dW / db of both heads and, if `below`, the input gradient's chunk partials and their sum
inline void ph_launch_layer(PhBwdArgs a, int b, int Kd, bool below, const float *mask0, const float *mask1, float *out0, float *out1,
                            int add_heads, hipStream_t s) {
  const int ktiles = dcl_div_up(Kd, kPhSlots), maxO = a.O[0] > a.O[1] ? a.O[0] : a.O[1];
  const bool sums = a.dW[0] || a.dW[1] || a.db[0] || a.db[1];
  const int nA = sums ? dcl_div_up((long long)ktiles * dcl_div_up(maxO, kBwdOut), 4) : 0;
  const int nB = below ? ktiles * ph_nchunks(maxO) : 0;
  if (!below) a.part[0] = a.part[1] = nullptr;
  if (nA + nB > 0) hipLaunchKernelGGL(k_ph_bwd_layer, dim3((unsigned)(nA + nB), 2), dim3(256), 0, s, a, b, Kd, ktiles, nA);
  if (below) {
    const long long n4 = (long long)b * Kd / kPhVec;
    hipLaunchKernelGGL(k_ph_bwd_sum, dim3((unsigned)((n4 + 255) / 256), add_heads ? 1 : 2), dim3(256), 0, s, a.part[0], a.part[1],
                       ph_nchunks(a.O[0]), ph_nchunks(a.O[1]), n4, mask0, mask1, out0, out1, add_heads);
  }
}

// ---- host twins' pieces --------------------------------------------------------------------------------------------------------
void ph_layer_fwd_host(int b, int Kd, int O, const float *in, const float *W, const float *bias, int relu, float *out) {
  for (size_t r = 0; r < (size_t)b; ++r)
    for (int o = 0; o < O; ++o) {
      float v[kPhLanes];
      for (int lane = 0; lane < kPhLanes; ++lane) {
        float acc[kPhVec];
        ph_dot_lane(in + r * Kd, W + (size_t)o * Kd, Kd, lane, acc);
        v[lane] = ph_lane_fold(acc);
      }
      const float z = ph_butterfly_host(v) + bias[o];
      out[r * O + o] = relu ? (z > 0.0f ? z : 0.0f) : z;
    }
}
// dz NULL = all zero.  din: (b, Kd) the chunk-ordered input gradient, or NULL
void ph_layer_bwd_host(int b, int Kd, int O, const float *W, const float *dz, const float *in, float *dW, float *db, float *din) {
  auto d = [&](size_t r, int o) { return dz ? dz[r * O + o] : 0.0f; };
  for (int o = 0; o < O; ++o) {
    if (dW)
      for (int k = 0; k < Kd; ++k) {
        float p = 0.0f;
        for (size_t r = 0; r < (size_t)b; ++r) p = fmaf(d(r, o), in[r * Kd + k], p);
        dW[(size_t)o * Kd + k] = p;
      }
    if (db) {
      float p = 0.0f;
      for (size_t r = 0; r < (size_t)b; ++r) p = p + d(r, o);
      db[o] = p;
    }
  }
  if (din)
    for (size_t r = 0; r < (size_t)b; ++r)
      for (int k = 0; k < Kd; ++k) {
        float total = 0.0f;
        for (int q = 0; q < ph_nchunks(O); ++q) {
          const int o1 = (q + 1) * kPhChunk < O ? (q + 1) * kPhChunk : O;
          float p = 0.0f;
          for (int o = q * kPhChunk; o < o1; ++o) p = fmaf(d(r, o), W[(size_t)o * Kd + k], p);
          total = q == 0 ? p : total + p;
        }
        din[r * Kd + k] = total;
      }
}

}  // namespace

DCL_API int dcl_pose_heads_train_fwd(int b, int d0, int d1, int d2, int n_rot, int n_trans, const float *x, const float *rW0,
                                     const float *rb0, const float *rW1, const float *rb1, const float *rW2, const float *rb2,
                                     const float *tW0, const float *tb0, const float *tW1, const float *tb1, const float *tW2,
                                     const float *tb2, float *h1, float *h2, float *o9, float *t3, dclStream_t stream) {
  DCL_CHECK_ARG(ph_dims_ok(b, d0, d1, d2, n_rot, n_trans));
  if (b == 0) return 0;
  DCL_CHECK_ARG(x && rW0 && rb0 && rW1 && rb1 && rW2 && rb2 && tW0 && tb0 && tW1 && tb1 && tW2 && tb2 && h1 && h2 && o9 && t3);
  DCL_CHECK_ARG(ph_aligned(x, h1, h2) && ph_aligned(rW0, rW1, rW2) && ph_aligned(tW0, tW1, tW2));
  hipStream_t s = (hipStream_t)stream;
  float *h1t = h1 + (size_t)b * d1, *h2t = h2 + (size_t)b * d2;
  const PhFwdArgs l1 = {{x, x}, {rW0, tW0}, {rb0, tb0}, {h1, h1t}, {d1, d1}};
  const PhFwdArgs l2 = {{h1, h1t}, {rW1, tW1}, {rb1, tb1}, {h2, h2t}, {d2, d2}};
  const PhFwdArgs l3 = {{h2, h2t}, {rW2, tW2}, {rb2, tb2}, {o9, t3}, {n_rot, n_trans}};
  const int per = 4 * kFwdOut, n3 = n_rot > n_trans ? n_rot : n_trans;
  hipLaunchKernelGGL(k_ph_fwd, dim3((unsigned)dcl_div_up(d1, per), 2), dim3(256), 0, s, l1, b, d0, 1);
  hipLaunchKernelGGL(k_ph_fwd, dim3((unsigned)dcl_div_up(d2, per), 2), dim3(256), 0, s, l2, b, d1, 1);
  hipLaunchKernelGGL(k_ph_fwd, dim3((unsigned)dcl_div_up(n3, per), 2), dim3(256), 0, s, l3, b, d2, 0);
  DCL_LAUNCH_CHECK();
  return 0;
}

DCL_API int dcl_pose_heads_train_fwd_host(int b, int d0, int d1, int d2, int n_rot, int n_trans, const float *x, const float *rW0,
                                          const float *rb0, const float *rW1, const float *rb1, const float *rW2,
                                          const float *rb2, const float *tW0, const float *tb0, const float *tW1,
                                          const float *tb1, const float *tW2, const float *tb2, float *h1, float *h2, float *o9,
                                          float *t3) {
  DCL_CHECK_ARG(ph_dims_ok(b, d0, d1, d2, n_rot, n_trans));
  if (b == 0) return 0;
  DCL_CHECK_ARG(x && rW0 && rb0 && rW1 && rb1 && rW2 && rb2 && tW0 && tb0 && tW1 && tb1 && tW2 && tb2 && h1 && h2 && o9 && t3);
  float *h1t = h1 + (size_t)b * d1, *h2t = h2 + (size_t)b * d2;
  ph_layer_fwd_host(b, d0, d1, x, rW0, rb0, 1, h1);
  ph_layer_fwd_host(b, d0, d1, x, tW0, tb0, 1, h1t);
  ph_layer_fwd_host(b, d1, d2, h1, rW1, rb1, 1, h2);
  ph_layer_fwd_host(b, d1, d2, h1t, tW1, tb1, 1, h2t);
  ph_layer_fwd_host(b, d2, n_rot, h2, rW2, rb2, 0, o9);
  ph_layer_fwd_host(b, d2, n_trans, h2t, tW2, tb2, 0, t3);
  return 0;
}

DCL_API int dcl_pose_heads_train_bwd_ws_bytes(int b, int d0, int d1, int d2, int n_rot, int n_trans, int64_t *bytes_host) {
  DCL_CHECK_ARG(ph_dims_ok(b, d0, d1, d2, n_rot, n_trans) && bytes_host);
  *bytes_host = (int64_t)sizeof(float) * ph_ws_floats(b, d0, d1, d2, n_rot, n_trans);
  return 0;
}

#define PH_GRADS d_rW0, d_rb0, d_rW1, d_rb1, d_rW2, d_rb2, d_tW0, d_tb0, d_tW1, d_tb1, d_tW2, d_tb2

DCL_API int dcl_pose_heads_train_bwd(int b, int d0, int d1, int d2, int n_rot, int n_trans, const float *x, const float *rW0,
                                     const float *rW1, const float *rW2, const float *tW0, const float *tW1, const float *tW2,
                                     const float *h1, const float *h2, const float *g_o9, const float *g_t3, float *dx,
                                     float *d_rW0, float *d_rb0, float *d_rW1, float *d_rb1, float *d_rW2, float *d_rb2,
                                     float *d_tW0, float *d_tb0, float *d_tW1, float *d_tb1, float *d_tW2, float *d_tb2, void *ws,
                                     int64_t ws_bytes, dclStream_t stream) {
  DCL_CHECK_ARG(ph_dims_ok(b, d0, d1, d2, n_rot, n_trans));
  if (b == 0) return 0;
  DCL_CHECK_ARG(x && rW0 && rW1 && rW2 && tW0 && tW1 && tW2 && h1 && h2 && (g_o9 || g_t3));
  float *const grads[12] = {PH_GRADS};
  bool any = dx != nullptr;
  for (float *p : grads) any = any || p;
  DCL_CHECK_ARG(any && ph_grid_ok(b, d0, d1, d2));
  DCL_CHECK_ARG(ws && ws_bytes >= (int64_t)sizeof(float) * ph_ws_floats(b, d0, d1, d2, n_rot, n_trans));
  DCL_CHECK_ARG(ph_aligned(x, h1, h2, ws) && ph_aligned(rW0, rW1, rW2, dx) && ph_aligned(tW0, tW1, tW2) &&
                ph_aligned(d_rW0, d_rW1, d_rW2) && ph_aligned(d_tW0, d_tW1, d_tW2));
  hipStream_t s = (hipStream_t)stream;
  const float *h1t = h1 + (size_t)b * d1, *h2t = h2 + (size_t)b * d2;
  float *dz2 = (float *)ws, *dz2t = dz2 + (size_t)b * d2;
  float *dz1 = dz2t + (size_t)b * d2, *dz1t = dz1 + (size_t)b * d1;
  float *part = dz1t + (size_t)b * d1, *partt = part + ph_part_floats(b, d0, d1, d2, n_rot, n_trans);
  const bool need1 = dx || d_rW0 || d_rb0 || d_tW0 || d_tb0;                 // layer 1 has work: dz1 is needed
  const bool need2 = need1 || d_rW1 || d_rb1 || d_tW1 || d_tb1;              // layer 2 has work: dz2 is needed
  const PhBwdArgs l3 = {{rW2, tW2}, {g_o9, g_t3}, {h2, h2t}, {d_rW2, d_tW2}, {d_rb2, d_tb2}, {part, partt}, {n_rot, n_trans}};
  ph_launch_layer(l3, b, d2, need2, h2, h2t, dz2, dz2t, 0, s);
  if (need2) {
    const PhBwdArgs l2 = {{rW1, tW1}, {dz2, dz2t}, {h1, h1t}, {d_rW1, d_tW1}, {d_rb1, d_tb1}, {part, partt}, {d2, d2}};
    ph_launch_layer(l2, b, d1, need1, h1, h1t, dz1, dz1t, 0, s);
  }
  if (need1) {
    const PhBwdArgs l1 = {{rW0, tW0}, {dz1, dz1t}, {x, x}, {d_rW0, d_tW0}, {d_rb0, d_tb0}, {part, partt}, {d1, d1}};
    ph_launch_layer(l1, b, d0, dx != nullptr, nullptr, nullptr, dx, nullptr, 1, s);
  }
  DCL_LAUNCH_CHECK();
  return 0;
}

DCL_API int dcl_pose_heads_train_bwd_host(int b, int d0, int d1, int d2, int n_rot, int n_trans, const float *x, const float *rW0,
                                          const float *rW1, const float *rW2, const float *tW0, const float *tW1,
                                          const float *tW2, const float *h1, const float *h2, const float *g_o9,
                                          const float *g_t3, float *dx, float *d_rW0, float *d_rb0, float *d_rW1, float *d_rb1,
                                          float *d_rW2, float *d_rb2, float *d_tW0, float *d_tb0, float *d_tW1, float *d_tb1,
                                          float *d_tW2, float *d_tb2) {
  DCL_CHECK_ARG(ph_dims_ok(b, d0, d1, d2, n_rot, n_trans));
  if (b == 0) return 0;
  DCL_CHECK_ARG(x && rW0 && rW1 && rW2 && tW0 && tW1 && tW2 && h1 && h2 && (g_o9 || g_t3));
  float *const grads[12] = {PH_GRADS};
  bool any = dx != nullptr;
  for (float *p : grads) any = any || p;
  DCL_CHECK_ARG(any && ph_grid_ok(b, d0, d1, d2));
  const size_t B = (size_t)b;
  const float *W0[2] = {rW0, tW0}, *W1[2] = {rW1, tW1}, *W2[2] = {rW2, tW2}, *g[2] = {g_o9, g_t3};
  float *dW0[2] = {d_rW0, d_tW0}, *db0[2] = {d_rb0, d_tb0}, *dW1[2] = {d_rW1, d_tW1}, *db1[2] = {d_rb1, d_tb1};
  float *dW2[2] = {d_rW2, d_tW2}, *db2[2] = {d_rb2, d_tb2};
  const int n3[2] = {n_rot, n_trans};
  std::vector<float> dz2(B * d2), dz1(B * d1), dxh[2];
  for (int head = 0; head < 2; ++head) {
    const float *h1h = h1 + head * B * d1, *h2h = h2 + head * B * d2;
    ph_layer_bwd_host(b, d2, n3[head], W2[head], g[head], h2h, dW2[head], db2[head], dz2.data());
    for (size_t i = 0; i < dz2.size(); ++i) dz2[i] = h2h[i] > 0.0f ? dz2[i] : 0.0f;
    ph_layer_bwd_host(b, d1, d2, W1[head], dz2.data(), h1h, dW1[head], db1[head], dz1.data());
    for (size_t i = 0; i < dz1.size(); ++i) dz1[i] = h1h[i] > 0.0f ? dz1[i] : 0.0f;
    if (dx) dxh[head].resize(B * d0);
    ph_layer_bwd_host(b, d0, d1, W0[head], dz1.data(), x, dW0[head], db0[head], dx ? dxh[head].data() : nullptr);
  }
  if (dx)
    for (size_t i = 0; i < B * d0; ++i) dx[i] = dxh[0][i] + dxh[1][i];
  return 0;
}
