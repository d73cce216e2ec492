// conf_pool_pm.hip -- the confidence-weighted pooling that ends stage 1's dense half, on POINT-major activations, with its
// gradient (models/DCL_Net.py: train_dense = "point_major"; autograd.ConfPoolPmFn).  F1 (b n1, C), F2 (b n2, C): a point's
// channels are contiguous.  conf and w come from dcl_conf_softmax (dense.hip); this file holds three streaming kernels, the
// per-crop rest is conf_pool_grad.hip's k_cpg_logits:
//   k_cpp_pool   pooled (b, C): a workgroup per (crop, 64 channels); 16 lanes read 256 bytes of a row, a group of 16 lanes runs
//                one chunk of DCL_POOL_PM_ROWS rows, 64 groups at a time; the chunks meet in LDS and are added in order
//   k_cpp_d      d (b, L): one wave per row, the row's dot with g_pooled
//   k_cpp_dF     dF1 / dF2 = g_pooled[c] * w[j], a pure streaming write, whole rows, g_pooled held in registers
// Bandwidth-bound (half a flop per byte): no MFMA, no LDS staging of F.  conf_pool_pm.h pins every summation order and is
// shared with the *_host entry points, which run the same routines on host pointers.  Element offsets are 64-bit.
#include <vector>

#include "common.h"
#include "conf_pool_pm.h"

namespace {

constexpr int kPoolThreads = kCppGroups * kCppColLanes;      // 1024

__global__ __launch_bounds__(kPoolThreads) void k_cpp_pool(int C, int n1, int n2, int coltiles, const float *__restrict__ w,
                                                           const float *__restrict__ F1, const float *__restrict__ F2,
                                                           float *__restrict__ pooled) {
  __shared__ float part[kCppGroups][kCppCols];
  const int tid = threadIdx.x, grp = tid / kCppColLanes, cl = tid % kCppColLanes;
  const size_t crop = blockIdx.x / coltiles;
  const int c0 = (int)(blockIdx.x % coltiles) * kCppCols;     // the workgroup's first channel
  const int c = c0 + kCpgVec * cl;                            // this lane's first channel
  const float *wr = w + crop * ((size_t)n1 + n2);
  const int Q = cpp_nchunks(n1) + cpp_nchunks(n2);
  const bool vec1 = (C & 3) == 0 && cpg_aligned16(F1), vec2 = (C & 3) == 0 && cpg_aligned16(F2);
  float total = 0.0f;
  for (int q0 = 0; q0 < Q; q0 += kCppGroups) {
    const int q = q0 + grp;
    if (q < Q && c < C) {
      const CppChunk k = cpp_chunk(q, n1, n2);
      const float *Fc = (k.dir ? F2 + (crop * n2 + k.j0) * (size_t)C : F1 + (crop * n1 + k.j0) * (size_t)C) + c;
      const float *wc = wr + (k.dir ? n1 : 0) + k.j0;
      float acc[kCpgVec];
      if (k.dir ? vec2 : vec1) {
        cpp_pool_chain4(Fc, (size_t)C, wc, k.rows, acc);
      } else {
#pragma unroll
        for (int v = 0; v < kCpgVec; ++v) acc[v] = c + v < C ? cpp_pool_chain(Fc + v, (size_t)C, wc, k.rows) : 0.0f;
      }
#pragma unroll
      for (int v = 0; v < kCpgVec; ++v) part[grp][kCpgVec * cl + v] = acc[v];
    }
    __syncthreads();
    if (tid < kCppCols && c0 + tid < C) {
      const int nq = min(kCppGroups, Q - q0);
      int k = 0;
      if (q0 == 0) total = part[k++][tid];                    // the first chunk's value starts the sum
      for (; k < nq; ++k) total = total + part[k][tid];
    }
    __syncthreads();
  }
  if (tid < kCppCols && c0 + tid < C) pooled[crop * C + c0 + tid] = total;
}

constexpr int kDRowsPerWave = 4;
constexpr int kDRowsPerBlock = 4 * kDRowsPerWave;             // 256 threads = 4 waves

// one direction: rows = b n rows of F (rows, C); row r is point r % n of crop r / n and goes to d[crop][off + point]
__global__ __launch_bounds__(256) void k_cpp_d(long long rows, int C, int n, int L, int off, const float *__restrict__ F,
                                               const float *__restrict__ g_pooled, float *__restrict__ d) {
  const int lane = threadIdx.x & (kCpgLanes - 1), wave = threadIdx.x / kCpgLanes;
  const long long r0 = ((long long)blockIdx.x * 4 + wave) * kDRowsPerWave;
  const bool vec = (C & 3) == 0 && cpg_aligned16(F) && cpg_aligned16(g_pooled);
  float v[kDRowsPerWave];
#pragma unroll
  for (int i = 0; i < kDRowsPerWave; ++i) {
    const long long r = r0 + i;
    v[i] = 0.0f;
    if (r < rows) {                                          // wave-uniform
      const float *Fr = F + (size_t)r * C, *g = g_pooled + (size_t)(r / n) * C;
      float acc[kCpgVec];
      if (vec) cpp_dot_lane<true>(Fr, g, C, lane, acc);
      else cpp_dot_lane<false>(Fr, g, C, lane, acc);
      v[i] = cpg_pool_lane_fold(acc);
    }
  }
#pragma unroll
  for (int i = 0; i < kDRowsPerWave; ++i) {
#pragma unroll
    for (int s = kCpgLanes / 2; s >= 1; s >>= 1) v[i] = v[i] + __shfl_xor(v[i], s, kCpgLanes);
  }
  if (lane < kDRowsPerWave && r0 + lane < rows) {
    const long long r = r0 + lane;
    float out = v[0];
#pragma unroll
    for (int i = 1; i < kDRowsPerWave; ++i) out = lane == i ? v[i] : out;
    d[(size_t)(r / n) * L + off + (r % n)] = out;
  }
}

// one direction: dF (b n, C) = g_pooled[crop][c] * w[crop][off + point].  A wave owns kDFRowsPerWave rows of one crop and keeps
// its channels' g_pooled in registers across them (1024 channels per pass): nothing but w is read per row.  Geometry only.
constexpr int kDFRowsPerWave = 32;
constexpr int kDFRowsPerBlock = 4 * kDFRowsPerWave;
constexpr int kDFPass = 4;                                    // float4 per lane and pass
__global__ __launch_bounds__(256) void k_cpp_dF(int C, int n, int L, int off, int nblk, const float *__restrict__ w,
                                                const float *__restrict__ g_pooled, float *__restrict__ dF) {
  const int lane = threadIdx.x & (kCpgLanes - 1), wave = threadIdx.x / kCpgLanes;
  const size_t crop = blockIdx.x / nblk;
  const int j0 = (int)(blockIdx.x % nblk) * kDFRowsPerBlock + wave * kDFRowsPerWave;
  if (j0 >= n) return;                                       // whole waves leave; no barrier below
  const int j1 = min(j0 + kDFRowsPerWave, n);
  const float *g = g_pooled + crop * C, *wr = w + crop * L + off;
  float *o = dF + crop * n * (size_t)C;
  if ((C & 3) == 0 && cpg_aligned16(dF) && cpg_aligned16(g_pooled)) {
    for (int c0 = kCpgVec * lane; c0 < C; c0 += kDFPass * kCpgSlots) {
      float4 x[kDFPass];
#pragma unroll
      for (int q = 0; q < kDFPass; ++q)
        x[q] = c0 + q * kCpgSlots < C ? *reinterpret_cast<const float4 *>(g + c0 + q * kCpgSlots) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 2
      for (int j = j0; j < j1; ++j) {
        const float wj = wr[j];
        float *row = o + (size_t)j * C + c0;
#pragma unroll
        for (int q = 0; q < kDFPass; ++q)
          if (c0 + q * kCpgSlots < C)
            *reinterpret_cast<float4 *>(row + q * kCpgSlots) = make_float4(x[q].x * wj, x[q].y * wj, x[q].z * wj, x[q].w * wj);
      }
    }
  } else {
    for (int j = j0; j < j1; ++j) {
      const float wj = wr[j];
      for (int c = lane; c < C; c += kCpgLanes) o[(size_t)j * C + c] = g[c] * wj;
    }
  }
}

inline long long cpp_row_blocks(long long rows) { return (rows + kDRowsPerBlock - 1) / kDRowsPerBlock; }
inline int cpp_coltiles(int c) { return (c + kCppCols - 1) / kCppCols; }
inline long long cpp_ws_floats(int b, int n1, int n2) { return (long long)b * ((long long)n1 + n2); }      // d
inline bool cpp_dims_ok(int b, int c, int n1, int n2) { return b >= 0 && c >= 1 && n1 >= 1 && n2 >= 1; }
// one grid dimension counts the pooling's (crop, channel tile) workgroups and the row kernels' row blocks; L is an int
inline bool cpp_grid_ok(int b, int c, int n1, int n2) {
  const long long nmax = n1 > n2 ? n1 : n2;
  return (long long)n1 + n2 <= INT32_MAX && (long long)b * cpp_coltiles(c) <= INT32_MAX &&
         cpp_row_blocks((long long)b * nmax) <= INT32_MAX;
}
inline bool cpp_bwd_outputs_ok(const float *dlogit1, const float *dlogit2, const float *dF1, const float *dF2) {
  return (dlogit1 != nullptr) == (dlogit2 != nullptr) && (dF1 != nullptr) == (dF2 != nullptr) && (dlogit1 || dF1);
}
inline dim3 cpp_row_grid(long long rows) { return dim3((unsigned)cpp_row_blocks(rows)); }

}  // namespace

DCL_API int dcl_conf_pool_pm_fwd(int b, int c, int n1, int n2, const float *w, const float *F1, const float *F2,
                                 float *pooled, dclStream_t stream) {
  DCL_CHECK_ARG(cpp_dims_ok(b, c, n1, n2));
  if (b == 0) return 0;
  DCL_CHECK_ARG(w && F1 && F2 && pooled && cpp_grid_ok(b, c, n1, n2));
  const int coltiles = cpp_coltiles(c);
  hipLaunchKernelGGL(k_cpp_pool, dim3((unsigned)((long long)b * coltiles)), dim3(kPoolThreads), 0, (hipStream_t)stream, c, n1, n2,
                     coltiles, w, F1, F2, pooled);
  DCL_LAUNCH_CHECK();
  return 0;
}

DCL_API int dcl_conf_pool_pm_fwd_host(int b, int c, int n1, int n2, const float *w, const float *F1, const float *F2,
                                      float *pooled) {
  DCL_CHECK_ARG(cpp_dims_ok(b, c, n1, n2));
  if (b == 0) return 0;
  DCL_CHECK_ARG(w && F1 && F2 && pooled && cpp_grid_ok(b, c, n1, n2));
  const int Q = cpp_nchunks(n1) + cpp_nchunks(n2);
  for (size_t crop = 0; crop < (size_t)b; ++crop) {
    const float *wr = w + crop * ((size_t)n1 + n2);
    for (int ch = 0; ch < c; ++ch) {
      float total = 0.0f;
      for (int q = 0; q < Q; ++q) {
        const CppChunk k = cpp_chunk(q, n1, n2);
        const float *Fc = (k.dir ? F2 + (crop * n2 + k.j0) * (size_t)c : F1 + (crop * n1 + k.j0) * (size_t)c) + ch;
        const float p = cpp_pool_chain(Fc, (size_t)c, wr + (k.dir ? n1 : 0) + k.j0, k.rows);
        total = q == 0 ? p : total + p;
      }
      pooled[crop * c + ch] = total;
    }
  }
  return 0;
}

DCL_API int dcl_conf_pool_pm_bwd_ws_bytes(int b, int c, int n1, int n2, int64_t *bytes_host) {
  DCL_CHECK_ARG(cpp_dims_ok(b, c, n1, n2) && bytes_host);
  *bytes_host = (int64_t)sizeof(float) * cpp_ws_floats(b, n1, n2);
  return 0;
}

DCL_API int dcl_conf_pool_pm_bwd(int b, int c, int n1, int n2, const float *conf, const float *w, const float *F1,
                                 const float *F2, const float *g_pooled, const float *g_conf, float *dlogit1, float *dlogit2,
                                 float *dF1, float *dF2, void *ws, int64_t ws_bytes, dclStream_t stream) {
  DCL_CHECK_ARG(cpp_dims_ok(b, c, n1, n2));
  if (b == 0) return 0;
  DCL_CHECK_ARG(conf && w && F1 && F2 && g_pooled && cpp_bwd_outputs_ok(dlogit1, dlogit2, dF1, dF2) &&
                cpp_grid_ok(b, c, n1, n2));
  // the scratch holds d: only the logits' gradient needs it
  DCL_CHECK_ARG(!dlogit1 || (ws && ws_bytes >= (int64_t)sizeof(float) * cpp_ws_floats(b, n1, n2)));
  hipStream_t s = (hipStream_t)stream;
  const int L = n1 + n2;
  const long long rows1 = (long long)b * n1, rows2 = (long long)b * n2;
  if (dlogit1) {
    float *d = (float *)ws;
    hipLaunchKernelGGL(k_cpp_d, cpp_row_grid(rows1), dim3(256), 0, s, rows1, c, n1, L, 0, F1, g_pooled, d);
    hipLaunchKernelGGL(k_cpp_d, cpp_row_grid(rows2), dim3(256), 0, s, rows2, c, n2, L, n1, F2, g_pooled, d);
    cpg_launch_logits(b, n1, n2, 1, conf, w, nullptr, d, g_conf, dlogit1, dlogit2, s);
  }
  if (dF1) {
    const int nblk1 = dcl_div_up(n1, kDFRowsPerBlock), nblk2 = dcl_div_up(n2, kDFRowsPerBlock);
    hipLaunchKernelGGL(k_cpp_dF, dim3((unsigned)((long long)b * nblk1)), dim3(256), 0, s, c, n1, L, 0, nblk1, w, g_pooled, dF1);
    hipLaunchKernelGGL(k_cpp_dF, dim3((unsigned)((long long)b * nblk2)), dim3(256), 0, s, c, n2, L, n1, nblk2, w, g_pooled, dF2);
  }
  DCL_LAUNCH_CHECK();
  return 0;
}

DCL_API int dcl_conf_pool_pm_bwd_host(int b, int c, int n1, int n2, const float *conf, const float *w, const float *F1,
                                      const float *F2, const float *g_pooled, const float *g_conf, float *dlogit1,
                                      float *dlogit2, float *dF1, float *dF2) {
  DCL_CHECK_ARG(cpp_dims_ok(b, c, n1, n2));
  if (b == 0) return 0;
  DCL_CHECK_ARG(conf && w && F1 && F2 && g_pooled && cpp_bwd_outputs_ok(dlogit1, dlogit2, dF1, dF2) &&
                cpp_grid_ok(b, c, n1, n2));
  const int L = n1 + n2;
  std::vector<float> d((size_t)L);
  for (size_t crop = 0; crop < (size_t)b; ++crop) {
    const float *g = g_pooled + crop * c, *wr = w + crop * L;
    if (dlogit1) {
      for (int j = 0; j < L; ++j) {
        const float *Fr = j < n1 ? F1 + (crop * n1 + j) * (size_t)c : F2 + (crop * n2 + (j - n1)) * (size_t)c;
        float v[kCpgLanes];
        for (int lane = 0; lane < kCpgLanes; ++lane) {
          float acc[kCpgVec];
          cpp_dot_lane<false>(Fr, g, c, lane, acc);
          v[lane] = cpg_pool_lane_fold(acc);
        }
        d[j] = cpg_pool_butterfly_host(v);
      }
      cpg_logits_crop_host(n1, n2, wr, d.data(), conf + crop * L, g_conf ? g_conf + crop * L : nullptr, dlogit1 + crop * n1,
                           dlogit2 + crop * n2);
    }
    if (dF1)
      for (int j = 0; j < L; ++j) {
        float *o = j < n1 ? dF1 + (crop * n1 + j) * (size_t)c : dF2 + (crop * n2 + (j - n1)) * (size_t)c;
        for (int ch = 0; ch < c; ++ch) o[ch] = g[ch] * wr[j];
      }
  }
  return 0;
}
