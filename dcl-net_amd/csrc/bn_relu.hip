// bn_relu.hip -- train-mode BatchNorm1d + ReLU on the (V, C) row-major feature matrix of a sparse tensor, with its gradient
// (models/Modules.py: BasicBlock_SPCONV with norm_form = "fused"; autograd.BnReluFn).  Five streaming kernels:
//   k_bn_sums<.., false>  per-chunk float64 partials of sum x, sum x^2: a workgroup per (chunk of kBnRows rows, tile of 64 channels)
//   k_bn_sums<.., true>   the same walk for sum dy, sum dy xhat, the mask recomputed from x
//   k_bn_finish           per channel: the chunks' partials added ascending (staged through LDS in batches), then mean / invstd
//                         and the running statistics, or dgamma / dbeta and the two means the dx pass needs
//   k_bn_apply            z = relu(xhat gamma + beta)
//   k_bn_dx               dx = a ((dy - mb) - xhat mg); may write over g
// Bandwidth-bound: no MFMA, no LDS staging of x.  bn_relu.h pins the arithmetic and every summation order and is shared with
// the *_host entry points, which run the same routines on host pointers.  Element offsets are 64-bit.
#include <vector>

#include "common.h"
#include "bn_relu.h"

#ifndef DCL_BN_NT
#define DCL_BN_NT 0                                  // -DDCL_BN_NT=1: z and dx leave as non-temporal stores (a build to measure against)
#endif

namespace {

typedef float bn_f4 __attribute__((ext_vector_type(4)));

template <bool VEC>
__device__ __forceinline__ void bn_store4_dev(float *p, int nch, const float *v) {
#if DCL_BN_NT
  if (VEC) {
    bn_f4 f = {v[0], v[1], v[2], v[3]};
    __builtin_nontemporal_store(f, reinterpret_cast<bn_f4 *>(p));
    return;
  }
#endif
  bn_store4<VEC>(p, nch, v);
}

// which (slot, group) a lane is: blockIdx.y numbers the channel tiles of kBnTileGroups groups
struct BnLane {
  int Gp, S, s, grp;
  bool live;
};
__device__ __forceinline__ BnLane bn_lane(int C) {
  BnLane l;
  l.Gp = bn_tile_groups(C);
  l.S = bn_slots(C);
  l.s = (int)threadIdx.x / l.Gp;
  l.grp = (int)blockIdx.y * kBnTileGroups + (int)threadIdx.x % l.Gp;
  l.live = l.s < l.S && l.grp < bn_groups(C);
  return l;
}

template <bool VEC, bool BWD>
__global__ __launch_bounds__(kBnThreads) void k_bn_sums(long long V, int C, const float *__restrict__ x,
                                                        const float *__restrict__ g, const float *__restrict__ mean,
                                                        const float *__restrict__ invstd, const float *__restrict__ gamma,
                                                        const float *__restrict__ beta, int relu, double *__restrict__ part) {
  __shared__ double red[kBnThreads * 2 * kBnVec];
  const BnLane l = bn_lane(C);
  const long long row0 = (long long)blockIdx.x * kBnRows;
  const int nrows = V - row0 < kBnRows ? (int)(V - row0) : kBnRows;
  double *prow = part + (size_t)blockIdx.x * 2 * C;
  double a1[kBnVec] = {0.0, 0.0, 0.0, 0.0}, a2[kBnVec] = {0.0, 0.0, 0.0, 0.0};
  if (l.live) {
    const int c0 = l.grp * kBnVec, nch = C - c0 < kBnVec ? C - c0 : kBnVec;
    const size_t off = (size_t)row0 * C + c0;
    if (BWD) {
      BnGroup k;
      bn_load_group(k, mean, invstd, gamma, beta, c0, nch);
      bn_bwd_slot<VEC>(x + off, g + off, C, nrows, l.s, l.S, nch, k, relu, a1, a2);
    } else {
      bn_stat_slot<VEC>(x + off, C, nrows, l.s, l.S, nch, a1, a2);
    }
  }
  double *mine = red + (size_t)threadIdx.x * 2 * kBnVec;
#pragma unroll
  for (int q = 0; q < kBnVec; ++q) mine[q] = a1[q], mine[kBnVec + q] = a2[q];
  __syncthreads();
  // a lane per channel of the tile: its S slots sit Gp lanes apart
  const int t = threadIdx.x, c = (int)blockIdx.y * kBnTileGroups * kBnVec + t;
  if (t < l.Gp * kBnVec && c < C) {
    const double *first = red + (size_t)(t / kBnVec) * 2 * kBnVec + (t % kBnVec);
    prow[c] = bn_ordered_sum(first, (size_t)l.Gp * 2 * kBnVec, l.S);
    prow[C + c] = bn_ordered_sum(first + kBnVec, (size_t)l.Gp * 2 * kBnVec, l.S);
  }
}

// mode 0: mean / invstd (o0, o1) and the running statistics; mode 1: dgamma / dbeta (o0, o1; both may be NULL) and mb / mg
// (o2, o3).  A workgroup owns kBnFinCh channels and walks the chunks in batches of kBnFinBatch staged in LDS, all of a
// batch's loads in flight together.  A channel's two chains -- dependent float64 additions, ascending chunk order whatever
// the batch size -- run in lanes of two different waves, reading their terms from LDS sixteen at a time.
constexpr int kFinLoads = kBnFinBatch * 2 * kBnFinCh / kBnThreads;
static_assert(kFinLoads * kBnThreads == kBnFinBatch * 2 * kBnFinCh, "a batch is a whole number of loads per lane");
__global__ __launch_bounds__(kBnThreads) void k_bn_finish(int mode, long long V, int C, int nchunks,
                                                          const double *__restrict__ part, float eps, float momentum,
                                                          float *running_mean, float *running_var, float *o0, float *o1,
                                                          float *o2, float *o3) {
  __shared__ double st[kBnFinBatch * 2 * kBnFinCh + 2 * kBnFinCh];
  double *fin = st + kBnFinBatch * 2 * kBnFinCh;             // the finished sums: [which][channel]
  const int tid = threadIdx.x, c0 = blockIdx.x * kBnFinCh;
  const int which = tid / 64, lc = tid % 64;                 // waves 0 and 1 hold the chains of the first and the second sum
  const bool chain = which < 2 && lc < kBnFinCh && c0 + lc < C;
  double sum = 0.0;
  for (int q0 = 0; q0 < nchunks; q0 += kBnFinBatch) {
    const int nb = nchunks - q0 < kBnFinBatch ? nchunks - q0 : kBnFinBatch;
    // kFinLoads loads per lane, none behind a branch: a chunk or a channel that does not exist reads the last one that does,
    // and no chain reads what it left in st
    double v[kFinLoads];
#pragma unroll
    for (int u = 0; u < kFinLoads; ++u) {
      const int i = tid + u * kBnThreads;
      const int q = q0 + i / (2 * kBnFinCh), ch = c0 + (i % kBnFinCh);
      v[u] = part[(size_t)(q < nchunks ? q : nchunks - 1) * 2 * C + (size_t)((i / kBnFinCh) & 1) * C + (ch < C ? ch : C - 1)];
    }
#pragma unroll
    for (int u = 0; u < kFinLoads; ++u) st[tid + u * kBnThreads] = v[u];
    __syncthreads();
    if (chain) sum = bn_ordered_sum_from(sum, st + which * kBnFinCh + lc, 2 * kBnFinCh, nb);
    __syncthreads();                                         // st is refilled by the next batch
  }
  if (chain) fin[which * kBnFinCh + lc] = sum;
  __syncthreads();
  const int c = c0 + tid;
  if (tid < kBnFinCh && c < C) {
    const double s1 = fin[tid], s2 = fin[kBnFinCh + tid];
    if (mode == 0)
      bn_finish_stats(s1, s2, V, eps, momentum, running_mean ? running_mean + c : nullptr,
                      running_mean ? running_var + c : nullptr, o0 + c, o1 + c);
    else
      bn_finish_bwd(s1, s2, V, o0 ? o0 + c : nullptr, o0 ? o1 + c : nullptr, o2 + c, o3 + c);
  }
}

// The element-wise pair: a workgroup owns S * kBnRowsPerLane rows of a channel tile, a lane the rows s, s + S, ... of them in
// its group's four channels.  All of a lane's loads are issued before the first is used; FULL = no row of the workgroup is beyond V.
template <bool VEC, bool FULL>
__device__ __forceinline__ void bn_apply_lane(const float *xg, float *zg, int C, long long rows_left, int S, int nch,
                                              const BnGroup &k, int relu) {
  float v[kBnRowsPerLane][kBnVec];
#pragma unroll
  for (int i = 0; i < kBnRowsPerLane; ++i)
    if (FULL || (long long)i * S < rows_left) bn_load4<VEC>(xg + (size_t)i * S * C, nch, v[i]);
#pragma unroll
  for (int i = 0; i < kBnRowsPerLane; ++i)
    if (FULL || (long long)i * S < rows_left) {
#pragma unroll
      for (int q = 0; q < kBnVec; ++q)
        v[i][q] = bn_z(bn_y(bn_xhat(v[i][q], k.mean[q], k.invstd[q]), k.gamma[q], k.beta[q]), relu);
      bn_store4_dev<VEC>(zg + (size_t)i * S * C, nch, v[i]);
    }
}

template <bool VEC>
__global__ __launch_bounds__(kBnThreads) void k_bn_apply(long long V, int C, const float *x, const float *__restrict__ mean,
                                                         const float *__restrict__ invstd, const float *__restrict__ gamma,
                                                         const float *__restrict__ beta, int relu, float *z) {
  const BnLane l = bn_lane(C);
  const long long row0 = (long long)blockIdx.x * l.S * kBnRowsPerLane + l.s;      // the lane's first row
  const bool full = (long long)(blockIdx.x + 1) * l.S * kBnRowsPerLane <= V;
  if (!l.live || row0 >= V) return;                          // no barrier below
  const int c0 = l.grp * kBnVec, nch = C - c0 < kBnVec ? C - c0 : kBnVec;
  BnGroup k;
  bn_load_group(k, mean, invstd, gamma, beta, c0, nch);
  const size_t off = (size_t)row0 * C + c0;
  if (full) bn_apply_lane<VEC, true>(x + off, z + off, C, 0, l.S, nch, k, relu);
  else bn_apply_lane<VEC, false>(x + off, z + off, C, V - row0, l.S, nch, k, relu);
}

template <bool VEC, bool FULL>
__device__ __forceinline__ void bn_dx_lane(const float *xg, const float *gg, float *dxg, int C, long long rows_left, int S,
                                           int nch, const BnGroup &k, const float *mb, const float *mg, int relu) {
  float v[kBnRowsPerLane][kBnVec], g[kBnRowsPerLane][kBnVec];
#pragma unroll
  for (int i = 0; i < kBnRowsPerLane; ++i)
    if (FULL || (long long)i * S < rows_left) {
      bn_load4<VEC>(xg + (size_t)i * S * C, nch, v[i]);
      bn_load4<VEC>(gg + (size_t)i * S * C, nch, g[i]);
    }
#pragma unroll
  for (int i = 0; i < kBnRowsPerLane; ++i)
    if (FULL || (long long)i * S < rows_left) {
#pragma unroll
      for (int q = 0; q < kBnVec; ++q) {
        const float xh = bn_xhat(v[i][q], k.mean[q], k.invstd[q]);
        const float dy = bn_dy(bn_y(xh, k.gamma[q], k.beta[q]), g[i][q], relu);
        v[i][q] = bn_dx(k.gamma[q] * k.invstd[q], dy, mb[q], xh, mg[q]);
      }
      bn_store4_dev<VEC>(dxg + (size_t)i * S * C, nch, v[i]);
    }
}

// dx may be g: a lane reads its own elements of g before it writes them, and no other lane touches them
template <bool VEC>
__global__ __launch_bounds__(kBnThreads) void k_bn_dx(long long V, int C, const float *x, const float *g,
                                                      const float *__restrict__ mean, const float *__restrict__ invstd,
                                                      const float *__restrict__ gamma, const float *__restrict__ beta,
                                                      const float *__restrict__ mbv, const float *__restrict__ mgv, int relu,
                                                      float *dx) {
  const BnLane l = bn_lane(C);
  const long long row0 = (long long)blockIdx.x * l.S * kBnRowsPerLane + l.s;
  const bool full = (long long)(blockIdx.x + 1) * l.S * kBnRowsPerLane <= V;
  if (!l.live || row0 >= V) return;
  const int c0 = l.grp * kBnVec, nch = C - c0 < kBnVec ? C - c0 : kBnVec;
  BnGroup k;
  bn_load_group(k, mean, invstd, gamma, beta, c0, nch);
  float mb[kBnVec], mg[kBnVec];
#pragma unroll
  for (int q = 0; q < kBnVec; ++q) mb[q] = mbv[q < nch ? c0 + q : c0], mg[q] = mgv[q < nch ? c0 + q : c0];
  const size_t off = (size_t)row0 * C + c0;
  if (full) bn_dx_lane<VEC, true>(x + off, g + off, dx + off, C, 0, l.S, nch, k, mb, mg, relu);
  else bn_dx_lane<VEC, false>(x + off, g + off, dx + off, C, V - row0, l.S, nch, k, mb, mg, relu);
}

inline int64_t bn_ws_bytes(long long V, int c) {             // the chunks' partials (float64), then mb and mg (fp32)
  return (int64_t)bn_nchunks(V) * 2 * c * (int64_t)sizeof(double) + 2 * (int64_t)c * (int64_t)sizeof(float);
}
inline long long bn_elem_blocks(long long V, int c) {
  const long long per = (long long)bn_slots(c) * kBnRowsPerLane;
  return (V + per - 1) / per;
}
inline bool bn_dims_ok(long long V, int c) { return V >= 0 && c >= 1 && V != 1; }
inline bool bn_grid_ok(long long V, int c) {
  return bn_nchunks(V) <= INT32_MAX && bn_elem_blocks(V, c) <= INT32_MAX && bn_tiles(c) <= 65535;
}
inline bool bn_ws_ok(const void *ws, int64_t ws_bytes, long long V, int c) {
  return ws && ((uintptr_t)ws & 7) == 0 && ws_bytes >= bn_ws_bytes(V, c);
}
inline bool bn_flag(int v) { return v == 0 || v == 1; }

// the chunk partials of a host matrix, then the channel sums, in the kernels' order
template <bool BWD>
void bn_sums_host(long long V, int c, const float *x, const float *g, const float *mean, const float *invstd,
                  const float *gamma, const float *beta, int relu, std::vector<double> &s1, std::vector<double> &s2) {
  const int G = bn_groups(c), S = bn_slots(c);
  const long long nchunks = bn_nchunks(V);
  std::vector<double> part((size_t)nchunks * 2 * c), slot((size_t)S * 2 * kBnVec);
  for (long long ch = 0; ch < nchunks; ++ch) {
    const long long row0 = ch * kBnRows;
    const int nrows = V - row0 < kBnRows ? (int)(V - row0) : kBnRows;
    for (int grp = 0; grp < G; ++grp) {
      const int c0 = grp * kBnVec, nch = c - c0 < kBnVec ? c - c0 : kBnVec;
      const size_t off = (size_t)row0 * c + c0;
      BnGroup k;
      if (BWD) bn_load_group(k, mean, invstd, gamma, beta, c0, nch);
      for (int s = 0; s < S; ++s) {
        double *a = slot.data() + (size_t)s * 2 * kBnVec;
        for (int q = 0; q < 2 * kBnVec; ++q) a[q] = 0.0;
        if (BWD) bn_bwd_slot<false>(x + off, g + off, c, nrows, s, S, nch, k, relu, a, a + kBnVec);
        else bn_stat_slot<false>(x + off, c, nrows, s, S, nch, a, a + kBnVec);
      }
      for (int q = 0; q < nch; ++q) {
        part[(size_t)ch * 2 * c + c0 + q] = bn_ordered_sum(slot.data() + q, 2 * kBnVec, S);
        part[(size_t)ch * 2 * c + c + c0 + q] = bn_ordered_sum(slot.data() + kBnVec + q, 2 * kBnVec, S);
      }
    }
  }
  s1.resize(c), s2.resize(c);
  for (int ch = 0; ch < c; ++ch) {
    s1[ch] = bn_ordered_sum(part.data() + ch, (size_t)2 * c, (int)nchunks);
    s2[ch] = bn_ordered_sum(part.data() + c + ch, (size_t)2 * c, (int)nchunks);
  }
}

}  // namespace

DCL_API int dcl_bn_relu_ws_bytes(int64_t rows, int c, int64_t *bytes_host) {
  DCL_CHECK_ARG(bn_dims_ok(rows, c) && bytes_host);
  *bytes_host = rows == 0 ? 0 : bn_ws_bytes(rows, c);
  return 0;
}

#define BN_FWD_ARGS_OK                                                                                                   \
  (x && gamma && beta && mean && invstd && z && (running_mean != nullptr) == (running_var != nullptr) && bn_flag(relu) && \
   eps >= 0.0f && momentum >= 0.0f && momentum <= 1.0f && bn_grid_ok(rows, c))
#define BN_BWD_ARGS_OK                                                                                             \
  (x && gamma && beta && mean && invstd && g && (dgamma != nullptr) == (dbeta != nullptr) && (dx || dgamma) && \
   bn_flag(relu) && bn_grid_ok(rows, c))

DCL_API int dcl_bn_relu_fwd(int64_t rows, int c, const float *x, const float *gamma, const float *beta, float eps,
                            float momentum, float *running_mean, float *running_var, float *mean, float *invstd, float *z,
                            int relu, void *ws, int64_t ws_bytes, dclStream_t stream) {
  DCL_CHECK_ARG(bn_dims_ok(rows, c));
  if (rows == 0) return 0;
  DCL_CHECK_ARG(BN_FWD_ARGS_OK && bn_ws_ok(ws, ws_bytes, rows, c));
  hipStream_t s = (hipStream_t)stream;
  const int nchunks = (int)bn_nchunks(rows);
  double *part = (double *)ws;
  const bool vec = (c & 3) == 0 && bn_aligned16(x), vecz = vec && bn_aligned16(z);
  const float *none = nullptr;
  if (vec)
    hipLaunchKernelGGL((k_bn_sums<true, false>), dim3(nchunks, bn_tiles(c)), dim3(kBnThreads), 0, s, (long long)rows, c, x, none, none,
                       none, none, none, 0, part);
  else
    hipLaunchKernelGGL((k_bn_sums<false, false>), dim3(nchunks, bn_tiles(c)), dim3(kBnThreads), 0, s, (long long)rows, c, x, none, none,
                       none, none, none, 0, part);
  float *nof = nullptr;
  hipLaunchKernelGGL(k_bn_finish, dim3(dcl_div_up(c, kBnFinCh)), dim3(kBnThreads), 0, s, 0, (long long)rows, c, nchunks,
                     (const double *)part, eps, momentum, running_mean, running_var, mean, invstd, nof, nof);
  const dim3 grid((unsigned)bn_elem_blocks(rows, c), bn_tiles(c));
  if (vecz)
    hipLaunchKernelGGL((k_bn_apply<true>), grid, dim3(kBnThreads), 0, s, (long long)rows, c, x, (const float *)mean,
                       (const float *)invstd, gamma, beta, relu, z);
  else
    hipLaunchKernelGGL((k_bn_apply<false>), grid, dim3(kBnThreads), 0, s, (long long)rows, c, x, (const float *)mean,
                       (const float *)invstd, gamma, beta, relu, z);
  DCL_LAUNCH_CHECK();
  return 0;
}

DCL_API int dcl_bn_relu_bwd(int64_t rows, int c, const float *x, const float *gamma, const float *beta, const float *mean,
                            const float *invstd, const float *g, int relu, float *dx, float *dgamma, float *dbeta, void *ws,
                            int64_t ws_bytes, dclStream_t stream) {
  DCL_CHECK_ARG(bn_dims_ok(rows, c));
  if (rows == 0) return 0;
  DCL_CHECK_ARG(BN_BWD_ARGS_OK && bn_ws_ok(ws, ws_bytes, rows, c));
  hipStream_t s = (hipStream_t)stream;
  const int nchunks = (int)bn_nchunks(rows);
  double *part = (double *)ws;
  float *mb = (float *)(part + (size_t)nchunks * 2 * c), *mg = mb + c;
  const bool vec = (c & 3) == 0 && bn_aligned16(x) && bn_aligned16(g);
  if (vec)
    hipLaunchKernelGGL((k_bn_sums<true, true>), dim3(nchunks, bn_tiles(c)), dim3(kBnThreads), 0, s, (long long)rows, c, x, g, mean, invstd,
                       gamma, beta, relu, part);
  else
    hipLaunchKernelGGL((k_bn_sums<false, true>), dim3(nchunks, bn_tiles(c)), dim3(kBnThreads), 0, s, (long long)rows, c, x, g, mean, invstd,
                       gamma, beta, relu, part);
  float *nof = nullptr;
  hipLaunchKernelGGL(k_bn_finish, dim3(dcl_div_up(c, kBnFinCh)), dim3(kBnThreads), 0, s, 1, (long long)rows, c, nchunks,
                     (const double *)part, 0.0f, 0.0f, nof, nof, dgamma, dbeta, mb, mg);
  if (dx) {
    const dim3 grid((unsigned)bn_elem_blocks(rows, c), bn_tiles(c));
    if (vec && bn_aligned16(dx))
      hipLaunchKernelGGL((k_bn_dx<true>), grid, dim3(kBnThreads), 0, s, (long long)rows, c, x, g, mean, invstd, gamma, beta,
                         (const float *)mb, (const float *)mg, relu, dx);
    else
      hipLaunchKernelGGL((k_bn_dx<false>), grid, dim3(kBnThreads), 0, s, (long long)rows, c, x, g, mean, invstd, gamma, beta,
                         (const float *)mb, (const float *)mg, relu, dx);
  }
  DCL_LAUNCH_CHECK();
  return 0;
}

DCL_API int dcl_bn_relu_fwd_host(int64_t rows, int c, const float *x, const float *gamma, const float *beta, float eps,
                                 float momentum, float *running_mean, float *running_var, float *mean, float *invstd, float *z,
                                 int relu) {
  DCL_CHECK_ARG(bn_dims_ok(rows, c));
  if (rows == 0) return 0;
  DCL_CHECK_ARG(BN_FWD_ARGS_OK);
  std::vector<double> s1, s2;
  bn_sums_host<false>(rows, c, x, nullptr, nullptr, nullptr, nullptr, nullptr, 0, s1, s2);
  for (int ch = 0; ch < c; ++ch)
    bn_finish_stats(s1[ch], s2[ch], rows, eps, momentum, running_mean ? running_mean + ch : nullptr,
                    running_mean ? running_var + ch : nullptr, mean + ch, invstd + ch);
  for (long long r = 0; r < rows; ++r)
    for (int ch = 0; ch < c; ++ch) {
      const size_t i = (size_t)r * c + ch;
      z[i] = bn_z(bn_y(bn_xhat(x[i], mean[ch], invstd[ch]), gamma[ch], beta[ch]), relu);
    }
  return 0;
}

DCL_API int dcl_bn_relu_bwd_host(int64_t rows, int c, const float *x, const float *gamma, const float *beta, const float *mean,
                                 const float *invstd, const float *g, int relu, float *dx, float *dgamma, float *dbeta) {
  DCL_CHECK_ARG(bn_dims_ok(rows, c));
  if (rows == 0) return 0;
  DCL_CHECK_ARG(BN_BWD_ARGS_OK);
  std::vector<double> s1, s2;
  bn_sums_host<true>(rows, c, x, g, mean, invstd, gamma, beta, relu, s1, s2);
  std::vector<float> mb(c), mg(c);
  for (int ch = 0; ch < c; ++ch)
    bn_finish_bwd(s1[ch], s2[ch], rows, dgamma ? dgamma + ch : nullptr, dgamma ? dbeta + ch : nullptr, &mb[ch], &mg[ch]);
  if (dx)
    for (long long r = 0; r < rows; ++r)
      for (int ch = 0; ch < c; ++ch) {
        const size_t i = (size_t)r * c + ch;
        const float xh = bn_xhat(x[i], mean[ch], invstd[ch]);
        const float dy = bn_dy(bn_y(xh, gamma[ch], beta[ch]), g[i], relu);
        dx[i] = bn_dx(gamma[ch] * invstd[ch], dy, mb[ch], xh, mg[ch]);
      }
  return 0;
}
