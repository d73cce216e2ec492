// conf_pool_grad.hip -- the confidence-weighted pooling that ends stage 1's dense half, on channel-major activations, with
// its gradient (models/DCL_Net.py: conf_1 ... F_p_wei on the module path; autograd.ConfPoolFn).  conf and w come from
// dcl_conf_softmax (dense.hip); this file holds the three streaming kernels and the small per-crop one:
//   k_cpg_pool    pooled (b, C): one wave per (crop, channel) row, F1's row then F2's against w
//   k_cpg_d       per-chunk partials of d (b, L): F read once, coalesced along the points, reduced over kCpgChunk channels
//   k_cpg_logits  per crop: chunks folded into d, dot = sum w d, dlogit1 / dlogit2
//   k_cpg_dF      dF1 / dF2 = g_pooled[c] * w[j], a pure streaming write
// Bandwidth-bound (half a flop per byte): no MFMA, no LDS staging of F.  conf_pool_grad.h pins every summation order and is
// shared with the *_host entry points, which run the same routines on host pointers.  Element offsets are 64-bit.
#include <vector>

#include "common.h"
#include "conf_pool_grad.h"

namespace {

constexpr int kPoolRowsPerBlock = 256 / kCpgLanes;

__global__ __launch_bounds__(256) void k_cpg_pool(long long rows, int C, int n1, int n2, const float *__restrict__ w,
                                                  const float *__restrict__ F1, const float *__restrict__ F2,
                                                  float *__restrict__ pooled) {
  const int lane = threadIdx.x & (kCpgLanes - 1), wave = threadIdx.x / kCpgLanes;
  const long long row = (long long)blockIdx.x * kPoolRowsPerBlock + wave;
  if (row >= rows) return;                                   // whole waves leave; no workgroup barrier below
  const long long crop = row / C;
  const float *w1 = w + (size_t)crop * ((size_t)n1 + n2), *w2 = w1 + n1;
  const float *r1 = F1 + (size_t)row * n1, *r2 = F2 + (size_t)row * n2;
  float acc[kCpgVec] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (cpg_aligned16(r1) && cpg_aligned16(w1)) cpg_pool_lane<true>(r1, w1, n1, lane, acc);
  else cpg_pool_lane<false>(r1, w1, n1, lane, acc);
  if (cpg_aligned16(r2) && cpg_aligned16(w2)) cpg_pool_lane<true>(r2, w2, n2, lane, acc);
  else cpg_pool_lane<false>(r2, w2, n2, lane, acc);
  float v = cpg_pool_lane_fold(acc);
#pragma unroll
  for (int s = kCpgLanes / 2; s >= 1; s >>= 1) v = v + __shfl_xor(v, s, kCpgLanes);
  if (lane == 0) pooled[row] = v;
}

// which (crop, chunk, direction, tile) a workgroup of the d / dF kernels owns: tiles fastest, then chunks, then crops
struct CpgWork {
  long long crop;
  int chunk, dir, tile;
};
__device__ __forceinline__ CpgWork cpg_work(int tiles1, int tiles2, int nchunks) {
  long long blk = blockIdx.x;
  const int tiles = tiles1 + tiles2;
  const int t = (int)(blk % tiles);
  blk /= tiles;
  CpgWork k;
  k.chunk = (int)(blk % nchunks);
  k.crop = blk / nchunks;
  k.dir = t >= tiles1;
  k.tile = k.dir ? t - tiles1 : t;
  return k;
}

__global__ __launch_bounds__(256) void k_cpg_d(int C, int n1, int n2, int tiles1, int tiles2, int nchunks,
                                               const float *__restrict__ F1, const float *__restrict__ F2,
                                               const float *__restrict__ g_pooled, float *__restrict__ part) {
  const CpgWork k = cpg_work(tiles1, tiles2, nchunks);
  const int n = k.dir ? n2 : n1;
  const size_t L = (size_t)n1 + n2;
  const float *F = k.dir ? F2 : F1;
  const int c0 = k.chunk * kCpgChunk, c1 = min(c0 + kCpgChunk, C);
  const float *Fc = F + ((size_t)k.crop * C + c0) * n;
  const float *g = g_pooled + (size_t)k.crop * C;
  float *prow = part + ((size_t)k.crop * nchunks + k.chunk) * L + (k.dir ? n1 : 0);
  if ((n & 3) == 0 && cpg_aligned16(F)) {                    // every row of this direction starts on 16 bytes
    const int j = k.tile * kCpgTile + kCpgVec * (int)threadIdx.x;
    if (j < n) {
      float acc[kCpgVec];
      cpg_d_chain4(Fc + j, (size_t)n, g, c0, c1, acc);
#pragma unroll
      for (int q = 0; q < kCpgVec; ++q) prow[j + q] = acc[q];
    }
  } else {
#pragma unroll
    for (int q = 0; q < kCpgVec; ++q) {
      const int j = k.tile * kCpgTile + q * 256 + (int)threadIdx.x;
      if (j < n) prow[j] = cpg_d_chain(Fc + j, (size_t)n, g, c0, c1);
    }
  }
}

// kDFRows channels per workgroup: geometry only (dF has no sum), so it does not follow kCpgChunk
constexpr int kDFRows = 64;
__global__ __launch_bounds__(256) void k_cpg_dF(int C, int n1, int n2, int tiles1, int tiles2, int ngroups,
                                                const float *__restrict__ w, const float *__restrict__ g_pooled,
                                                float *__restrict__ dF1, float *__restrict__ dF2) {
  const CpgWork k = cpg_work(tiles1, tiles2, ngroups);
  const int n = k.dir ? n2 : n1;
  const size_t L = (size_t)n1 + n2;
  float *dF = k.dir ? dF2 : dF1;
  const int c0 = k.chunk * kDFRows, c1 = min(c0 + kDFRows, C);
  float *dFc = dF + ((size_t)k.crop * C + c0) * n;
  const float *g = g_pooled + (size_t)k.crop * C;
  const float *wrow = w + (size_t)k.crop * L + (k.dir ? n1 : 0);
  if ((n & 3) == 0 && cpg_aligned16(dF)) {
    const int j = k.tile * kCpgTile + kCpgVec * (int)threadIdx.x;
    if (j < n) {
      const float w0 = wrow[j], w1 = wrow[j + 1], w2 = wrow[j + 2], w3 = wrow[j + 3];
#pragma unroll 8
      for (int c = c0; c < c1; ++c) {
        const float gc = g[c];
        *reinterpret_cast<float4 *>(dFc + (size_t)(c - c0) * n + j) = make_float4(gc * w0, gc * w1, gc * w2, gc * w3);
      }
    }
  } else {
#pragma unroll
    for (int q = 0; q < kCpgVec; ++q) {
      const int j = k.tile * kCpgTile + q * 256 + (int)threadIdx.x;
      if (j < n) {
        const float wj = wrow[j];
#pragma unroll 8
        for (int c = c0; c < c1; ++c) dFc[(size_t)(c - c0) * n + j] = g[c] * wj;
      }
    }
  }
}

// One workgroup of kLogitThreads per crop.  The fold of the chunks and the last pass are per column (any thread may take any
// column); the dot is the pinned one: its kCpgDotLanes lanes are the first 256 threads.
constexpr int kLogitThreads = 1024;
__global__ __launch_bounds__(kLogitThreads) void k_cpg_logits(int n1, int n2, int nchunks, const float *__restrict__ conf,
                                                               const float *__restrict__ w, const float *__restrict__ part,
                                                               float *d, const float *__restrict__ g_conf,
                                                               float *__restrict__ dlogit1, float *__restrict__ dlogit2) {
  __shared__ float red[kCpgDotLanes];
  const int tid = threadIdx.x, L = n1 + n2;
  const size_t crop = blockIdx.x, row = crop * (size_t)L;
  const float *wr = w + row, *pr = part ? part + crop * (size_t)nchunks * L : nullptr;
  float *dr = d + row;
  if (part)                                                  // NULL: the caller left d's values in place (conf_pool_pm.hip)
    for (int j = tid; j < L; j += kLogitThreads) dr[j] = cpg_d_fold(pr + j, (size_t)L, nchunks);
  __syncthreads();                                          // d goes through memory: the dot's lanes read other threads' columns
  if (tid < kCpgDotLanes) red[tid] = cpg_dot_lane(wr, dr, L, tid);
  __syncthreads();
  for (int s = kCpgDotLanes / 2; s >= 1; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  const float dot = red[0];
  for (int j = tid; j < L; j += kLogitThreads) {
    const float v = cpg_dlogit(wr[j], dr[j], dot, g_conf ? g_conf + row + j : nullptr, conf[row + j]);
    if (j < n1) dlogit1[crop * (size_t)n1 + j] = v;
    else dlogit2[crop * (size_t)n2 + (j - n1)] = v;
  }
}

inline int cpg_tiles(int n) { return (n + kCpgTile - 1) / kCpgTile; }
inline long long cpg_ws_floats(int b, int c, int n1, int n2) {
  return (long long)b * ((long long)n1 + n2) * (cpg_nchunks(c) + 1);     // the chunks' partials, then d
}
inline bool cpg_dims_ok(int b, int c, int n1, int n2) { return b >= 0 && c >= 1 && n1 >= 1 && n2 >= 1; }
// the d / dF launches count (crop, chunk, tile) workgroups in one grid dimension; L itself is an int in the kernels
inline bool cpg_grid_ok(int b, int c, int n1, int n2) {
  return (long long)n1 + n2 <= INT32_MAX &&
         (long long)b * cpg_nchunks(c) * (cpg_tiles(n1) + cpg_tiles(n2)) <= INT32_MAX &&
         (long long)b * dcl_div_up(c, kDFRows) * (cpg_tiles(n1) + cpg_tiles(n2)) <= INT32_MAX && (long long)b * c <= INT32_MAX;
}
inline bool cpg_bwd_outputs_ok(const float *dlogit1, const float *dlogit2, const float *dF1, const float *dF2) {
  return (dlogit1 != nullptr) == (dlogit2 != nullptr) && (dF1 != nullptr) == (dF2 != nullptr) && (dlogit1 || dF1);
}

}  // namespace

void cpg_launch_logits(int b, int n1, int n2, int nchunks, const float *conf, const float *w, const float *part, float *d,
                       const float *g_conf, float *dlogit1, float *dlogit2, void *stream) {
  hipLaunchKernelGGL(k_cpg_logits, dim3(b), dim3(kLogitThreads), 0, (hipStream_t)stream, n1, n2, nchunks, conf, w, part, d, g_conf,
                     dlogit1, dlogit2);
}

DCL_API int dcl_conf_pool_cm_fwd(int b, int c, int n1, int n2, const float *w, const float *F1, const float *F2,
                                 float *pooled, dclStream_t stream) {
  DCL_CHECK_ARG(cpg_dims_ok(b, c, n1, n2));
  if (b == 0) return 0;
  DCL_CHECK_ARG(w && F1 && F2 && pooled && cpg_grid_ok(b, c, n1, n2));
  const long long rows = (long long)b * c;
  hipLaunchKernelGGL(k_cpg_pool, dim3(dcl_div_up(rows, kPoolRowsPerBlock)), dim3(256), 0, (hipStream_t)stream, rows, c, n1, n2,
                     w, F1, F2, pooled);
  DCL_LAUNCH_CHECK();
  return 0;
}

DCL_API int dcl_conf_pool_cm_fwd_host(int b, int c, int n1, int n2, const float *w, const float *F1, const float *F2,
                                      float *pooled) {
  DCL_CHECK_ARG(cpg_dims_ok(b, c, n1, n2));
  if (b == 0) return 0;
  DCL_CHECK_ARG(w && F1 && F2 && pooled && cpg_grid_ok(b, c, n1, n2));
  for (long long row = 0; row < (long long)b * c; ++row) {
    const float *w1 = w + (size_t)(row / c) * ((size_t)n1 + n2);
    float v[kCpgLanes];
    for (int lane = 0; lane < kCpgLanes; ++lane) {
      float acc[kCpgVec] = {0.0f, 0.0f, 0.0f, 0.0f};
      cpg_pool_lane<false>(F1 + (size_t)row * n1, w1, n1, lane, acc);
      cpg_pool_lane<false>(F2 + (size_t)row * n2, w1 + n1, n2, lane, acc);
      v[lane] = cpg_pool_lane_fold(acc);
    }
    pooled[row] = cpg_pool_butterfly_host(v);
  }
  return 0;
}

DCL_API int dcl_conf_pool_cm_bwd_ws_bytes(int b, int c, int n1, int n2, int64_t *bytes_host) {
  DCL_CHECK_ARG(cpg_dims_ok(b, c, n1, n2) && bytes_host);
  *bytes_host = (int64_t)sizeof(float) * cpg_ws_floats(b, c, n1, n2);
  return 0;
}

DCL_API int dcl_conf_pool_cm_bwd(int b, int c, int n1, int n2, const float *conf, const float *w, const float *F1,
                                 const float *F2, const float *g_pooled, const float *g_conf, float *dlogit1, float *dlogit2,
                                 float *dF1, float *dF2, void *ws, int64_t ws_bytes, dclStream_t stream) {
  DCL_CHECK_ARG(cpg_dims_ok(b, c, n1, n2));
  if (b == 0) return 0;
  DCL_CHECK_ARG(conf && w && F1 && F2 && g_pooled && cpg_bwd_outputs_ok(dlogit1, dlogit2, dF1, dF2) &&
                cpg_grid_ok(b, c, n1, n2));
  // the scratch holds the partials of d and d itself: only the logits' gradient needs it
  DCL_CHECK_ARG(!dlogit1 || (ws && ws_bytes >= (int64_t)sizeof(float) * cpg_ws_floats(b, c, n1, n2)));
  hipStream_t s = (hipStream_t)stream;
  const int nchunks = cpg_nchunks(c), t1 = cpg_tiles(n1), t2 = cpg_tiles(n2);
  const dim3 grid((unsigned)((long long)b * nchunks * (t1 + t2)));
  if (dlogit1) {
    float *part = (float *)ws, *d = part + (size_t)b * nchunks * ((size_t)n1 + n2);
    hipLaunchKernelGGL(k_cpg_d, grid, dim3(256), 0, s, c, n1, n2, t1, t2, nchunks, F1, F2, g_pooled, part);
    cpg_launch_logits(b, n1, n2, nchunks, conf, w, part, d, g_conf, dlogit1, dlogit2, s);
  }
  if (dF1) {
    const int ngroups = dcl_div_up(c, kDFRows);
    hipLaunchKernelGGL(k_cpg_dF, dim3((unsigned)((long long)b * ngroups * (t1 + t2))), dim3(256), 0, s, c, n1, n2, t1, t2, ngroups,
                       w, g_pooled, dF1, dF2);
  }
  DCL_LAUNCH_CHECK();
  return 0;
}

DCL_API int dcl_conf_pool_cm_bwd_host(int b, int c, int n1, int n2, const float *conf, const float *w, const float *F1,
                                      const float *F2, const float *g_pooled, const float *g_conf, float *dlogit1,
                                      float *dlogit2, float *dF1, float *dF2) {
  DCL_CHECK_ARG(cpg_dims_ok(b, c, n1, n2));
  if (b == 0) return 0;
  DCL_CHECK_ARG(conf && w && F1 && F2 && g_pooled && cpg_bwd_outputs_ok(dlogit1, dlogit2, dF1, dF2) &&
                cpg_grid_ok(b, c, n1, n2));
  const int nchunks = cpg_nchunks(c), L = n1 + n2;
  std::vector<float> part((size_t)nchunks * L), d((size_t)L);
  for (int crop = 0; crop < b; ++crop) {
    const float *g = g_pooled + (size_t)crop * c, *wr = w + (size_t)crop * L;
    if (dlogit1) {
      for (int q = 0; q < nchunks; ++q) {
        const int c0 = q * kCpgChunk, c1 = c0 + kCpgChunk < c ? c0 + kCpgChunk : c;
        for (int j = 0; j < L; ++j) {
          const float *Fcol = j < n1 ? F1 + ((size_t)crop * c + c0) * n1 + j : F2 + ((size_t)crop * c + c0) * n2 + (j - n1);
          part[(size_t)q * L + j] = cpg_d_chain(Fcol, (size_t)(j < n1 ? n1 : n2), g, c0, c1);
        }
      }
      for (int j = 0; j < L; ++j) d[j] = cpg_d_fold(part.data() + j, (size_t)L, nchunks);
      cpg_logits_crop_host(n1, n2, wr, d.data(), conf + (size_t)crop * L, g_conf ? g_conf + (size_t)crop * L : nullptr,
                           dlogit1 + (size_t)crop * n1, dlogit2 + (size_t)crop * n2);
    }
    if (dF1)
      for (int ch = 0; ch < c; ++ch) {
        float *o1 = dF1 + ((size_t)crop * c + ch) * n1, *o2 = dF2 + ((size_t)crop * c + ch) * n2;
        for (int j = 0; j < n1; ++j) o1[j] = g[ch] * wr[j];
        for (int j = 0; j < n2; ++j) o2[j] = g[ch] * wr[n1 + j];
      }
  }
  return 0;
}
