// linear_narrow.hip -- a per-point linear layer with very few output columns (the last layers of stage 1's per-point heads: 1 or
// 3 columns over 32 768 and more rows), forward and backward, for the training path (models/DCL_Net.py: train_heads = "kernels";
// autograd.NarrowLinearFn).  y (M, N) = x (M, K) W^T + bias with W (N, K) as the convolution registers it: no transposed copy.
//   k_ln_fwd     16 lanes read a row of x 16 bytes each and hold one accumulator set per output: x is read once
//                (k_ln_fwd_small, K <= 256 and N <= 4: the lanes' share of W in registers, four rows' loads in flight)
//   k_ln_bwd     one pass over x and g: a thread owns four columns of a chunk of DCL_NARROW_ROWS rows, writes its rows' dx (a
//                pure stream, W's columns held in registers) and carries the chunk's dW / db chains; the partials go to scratch
//   k_ln_finish  adds the chunks' partials in ascending order (they meet in LDS, 512 chunks a round)
// Bandwidth-bound (2 N flop per 4 bytes of x): no MFMA.  linear_narrow.h pins every summation order and is shared with the
// *_host entry points, which run the same routines on host pointers.  No atomics.  Element offsets are 64-bit.
#include <vector>

#include "common.h"
#include "linear_narrow.h"

namespace {

constexpr int kFwdRowsPerGroup = 4;                           // rows a group of 16 lanes takes, one after the other
constexpr int kFwdGroups = 256 / kLnLanes;                    // 16 groups per workgroup
constexpr int kFwdRowsPerBlock = kFwdGroups * kFwdRowsPerGroup;

template <bool VEC, int NMAX>
__global__ __launch_bounds__(256) void k_ln_fwd(long long M, int K, int N, const float *__restrict__ x, long long pitch,
                                                const float *__restrict__ W, const float *__restrict__ bias,
                                                float *__restrict__ y) {
  const int lane = threadIdx.x & (kLnLanes - 1), grp = threadIdx.x / kLnLanes;
  const long long r0 = ((long long)blockIdx.x * kFwdGroups + grp) * kFwdRowsPerGroup;
  for (int i = 0; i < kFwdRowsPerGroup; ++i) {
    const long long r = r0 + i;
    const bool live = r < M;                                  // the same for the 16 lanes of a group
    float acc[NMAX][kLnVec];
    float v[NMAX];
    if (live) {
      ln_row_lane<VEC, NMAX>(x + (size_t)r * (size_t)pitch, W, K, N, lane, acc);
#pragma unroll
      for (int j = 0; j < NMAX; ++j) v[j] = ln_lane_fold(acc[j]);
    } else {
#pragma unroll
      for (int j = 0; j < NMAX; ++j) v[j] = 0.0f;
    }
#pragma unroll
    for (int j = 0; j < NMAX; ++j)
      if (j < N) {
#pragma unroll
        for (int s = kLnLanes / 2; s >= 1; s >>= 1) v[j] = v[j] + __shfl_xor(v[j], s, kLnLanes);
      }
    if (live && lane < N) {
      float out = v[0];
#pragma unroll
      for (int j = 1; j < NMAX; ++j) out = lane == j ? v[j] : out;
      if (bias) out = out + bias[lane];
      y[(size_t)r * N + lane] = out;
    }
  }
}

// The same rows, slots and chains for K <= kLnSmallK and at most four outputs: a lane's columns are the same in every row, so
// its share of W stays in registers, and the loads of a group's four rows are issued together.
constexpr int kSmallSteps = 4;
constexpr int kLnSmallK = kSmallSteps * kLnSlots;             // 256
template <bool VEC, int NMAX>
__global__ __launch_bounds__(256) void k_ln_fwd_small(long long M, int K, int N, const float *__restrict__ x, long long pitch,
                                                      const float *__restrict__ W, const float *__restrict__ bias,
                                                      float *__restrict__ y) {
  const int lane = threadIdx.x & (kLnLanes - 1), grp = threadIdx.x / kLnLanes;
  const long long r0 = ((long long)blockIdx.x * kFwdGroups + grp) * kFwdRowsPerGroup;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 w[NMAX][kSmallSteps], a[kFwdRowsPerGroup][kSmallSteps];
#pragma unroll
  for (int s = 0; s < kSmallSteps; ++s) {
    const int c = kLnVec * lane + kLnSlots * s;
#pragma unroll
    for (int j = 0; j < NMAX; ++j) w[j][s] = j < N && c < K ? ln_load4<VEC>(W + (size_t)j * K + c, K - c) : zero;
#pragma unroll
    for (int i = 0; i < kFwdRowsPerGroup; ++i)
      a[i][s] = r0 + i < M && c < K ? ln_load4<VEC>(x + (size_t)(r0 + i) * (size_t)pitch + c, K - c) : zero;
  }
#pragma unroll
  for (int i = 0; i < kFwdRowsPerGroup; ++i) {
    float v[NMAX];
#pragma unroll
    for (int j = 0; j < NMAX; ++j) {
      float acc[kLnVec] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int s = 0; s < kSmallSteps; ++s) {
        const int have = K - (kLnVec * lane + kLnSlots * s);  // a column that does not exist adds nothing
        if (have > 0) acc[0] = fmaf(a[i][s].x, w[j][s].x, acc[0]);
        if (have > 1) acc[1] = fmaf(a[i][s].y, w[j][s].y, acc[1]);
        if (have > 2) acc[2] = fmaf(a[i][s].z, w[j][s].z, acc[2]);
        if (have > 3) acc[3] = fmaf(a[i][s].w, w[j][s].w, acc[3]);
      }
      v[j] = ln_lane_fold(acc);
#pragma unroll
      for (int st = kLnLanes / 2; st >= 1; st >>= 1) v[j] = v[j] + __shfl_xor(v[j], st, kLnLanes);
    }
    if (r0 + i < M && lane < N) {
      float out = v[0];
#pragma unroll
      for (int j = 1; j < NMAX; ++j) out = lane == j ? v[j] : out;
      if (bias) out = out + bias[lane];
      y[(size_t)(r0 + i) * N + lane] = out;
    }
  }
}

template <bool VEC, int NMAX>
__global__ __launch_bounds__(256) void k_ln_bwd(long long M, int K, int N, int K4, long long nchunks, long long pfloats,
                                                const float *__restrict__ x, long long pitch, const float *__restrict__ W,
                                                const float *__restrict__ g, float *__restrict__ dx, float *__restrict__ part) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long q = t / K4;
  if (q >= nchunks) return;
  const int k = (int)(t % K4) * kLnVec;
  const long long m0 = q * kLnRows;
  const int rows = (int)(M - m0 < kLnRows ? M - m0 : kLnRows);
  float4 pw[NMAX];
  float pb[NMAX];
  ln_bwd_chunk<VEC, NMAX>(x, pitch, W, g, K, N, m0, rows, k, dx, part != nullptr, pw, pb);
  if (part) {
    float *p = part + (size_t)q * (size_t)pfloats;
#pragma unroll
    for (int j = 0; j < NMAX; ++j)
      if (j < N) {
        ln_store4<VEC>(p + (size_t)j * K + k, K - k, pw[j]);
        if (k == 0) p[(size_t)N * K + j] = pb[j];
      }
  }
}

constexpr int kFinCols = 16;                                  // elements of dW | db per workgroup of the finish
constexpr int kFinGroups = 64, kFinPer = 8;                   // 64 groups of 16 lanes fetch 8 chunks each: 512 chunks a round
constexpr int kFinRound = kFinGroups * kFinPer;
constexpr int kFinBatch = 16;
__global__ __launch_bounds__(kFinCols *kFinGroups) void k_ln_finish(long long nchunks, int NK, int E, long long pfloats,
                                                                     const float *__restrict__ part, float *__restrict__ dW,
                                                                     float *__restrict__ db) {
  __shared__ float s[kFinRound][kFinCols];
  const int col = threadIdx.x % kFinCols, grp = threadIdx.x / kFinCols;
  const int e = blockIdx.x * kFinCols + col;                  // < E + 15: an int, E <= 16 K + 16
  float total = 0.0f;
  float nxt[kFinPer];
  auto fetch = [&](long long q0) {
#pragma unroll
    for (int u = 0; u < kFinPer; ++u) {
      const long long q = q0 + grp * kFinPer + u;
      nxt[u] = q < nchunks && e < E ? part[(size_t)q * (size_t)pfloats + e] : 0.0f;
    }
  };
  fetch(0);
  for (long long q0 = 0; q0 < nchunks; q0 += kFinRound) {
#pragma unroll
    for (int u = 0; u < kFinPer; ++u) s[grp * kFinPer + u][col] = nxt[u];
    __syncthreads();
    if (q0 + kFinRound < nchunks) fetch(q0 + kFinRound);      // the next round's loads fly while this round is added
    if (grp == 0 && e < E) {
      const int nq = (int)(nchunks - q0 < kFinRound ? nchunks - q0 : kFinRound);
      int k = 0;
      if (q0 == 0) total = s[k++][col];                       // the first chunk's value starts the sum
      for (; k + kFinBatch <= nq; k += kFinBatch) {           // sixteen LDS reads in flight, added in order
        float t[kFinBatch];
#pragma unroll
        for (int u = 0; u < kFinBatch; ++u) t[u] = s[k + u][col];
#pragma unroll
        for (int u = 0; u < kFinBatch; ++u) total = total + t[u];
      }
      for (; k < nq; ++k) total = total + s[k][col];
    }
    __syncthreads();
  }
  if (grp == 0 && e < E) {
    if (e < NK) {
      if (dW) dW[e] = total;
    } else if (db) {
      db[e - NK] = total;
    }
  }
}

inline bool ln_dims_ok(long long M, int K, int N) { return M >= 0 && K >= 1 && N >= 1 && N <= kLnMaxN; }
// one grid dimension counts the forward's row blocks and the backward's (chunk, four columns) threads
inline bool ln_grid_ok(long long M, int K) {
  const long long K4 = ((long long)K + kLnVec - 1) / kLnVec;
  return (M + kFwdRowsPerBlock - 1) / kFwdRowsPerBlock <= INT32_MAX && ((long long)K + 1) * kLnMaxN + kFinCols <= INT32_MAX &&
         ln_nchunks(M) <= (INT64_MAX / 4) / K4 && (ln_nchunks(M) * K4 + 255) / 256 <= INT32_MAX;
}
inline bool ln_pitch_ok(long long M, int K, long long pitch) { return pitch >= K || M <= 1; }
inline long long ln_ws_floats(long long M, int K, int N) { return ln_nchunks(M) * ln_part_floats(K, N); }

#define LN_DISPATCH(kernel, vec, N, ...)                                                      \
  do {                                                                                       \
    if (vec) {                                                                               \
      if ((N) == 1) hipLaunchKernelGGL((kernel<true, 1>), __VA_ARGS__);                      \
      else if ((N) <= 4) hipLaunchKernelGGL((kernel<true, 4>), __VA_ARGS__);                 \
      else hipLaunchKernelGGL((kernel<true, kLnMaxN>), __VA_ARGS__);                         \
    } else {                                                                                 \
      if ((N) == 1) hipLaunchKernelGGL((kernel<false, 1>), __VA_ARGS__);                     \
      else if ((N) <= 4) hipLaunchKernelGGL((kernel<false, 4>), __VA_ARGS__);                \
      else hipLaunchKernelGGL((kernel<false, kLnMaxN>), __VA_ARGS__);                        \
    }                                                                                        \
  } while (0)

}  // namespace

DCL_API int dcl_linear_narrow_fwd(int64_t M, int K, int N, const float *x, int64_t x_pitch, const float *W, const float *bias,
                                  float *y, dclStream_t stream) {
  DCL_CHECK_ARG(ln_dims_ok(M, K, N));
  if (M == 0) return 0;
  DCL_CHECK_ARG(x && W && y && ln_pitch_ok(M, K, x_pitch) && ln_grid_ok(M, K));
  const bool vec = (K & 3) == 0 && (x_pitch & 3) == 0 && cpg_aligned16(x) && cpg_aligned16(W);
  const dim3 grid((unsigned)((M + kFwdRowsPerBlock - 1) / kFwdRowsPerBlock));
  if (K <= kLnSmallK && N <= 4) {
    if (vec && N == 1) hipLaunchKernelGGL((k_ln_fwd_small<true, 1>), grid, dim3(256), 0, (hipStream_t)stream, (long long)M, K, N, x, (long long)x_pitch, W, bias, y);
    else if (vec) hipLaunchKernelGGL((k_ln_fwd_small<true, 4>), grid, dim3(256), 0, (hipStream_t)stream, (long long)M, K, N, x, (long long)x_pitch, W, bias, y);
    else if (N == 1) hipLaunchKernelGGL((k_ln_fwd_small<false, 1>), grid, dim3(256), 0, (hipStream_t)stream, (long long)M, K, N, x, (long long)x_pitch, W, bias, y);
    else hipLaunchKernelGGL((k_ln_fwd_small<false, 4>), grid, dim3(256), 0, (hipStream_t)stream, (long long)M, K, N, x, (long long)x_pitch, W, bias, y);
  } else {
    LN_DISPATCH(k_ln_fwd, vec, N, grid, dim3(256), 0, (hipStream_t)stream, (long long)M, K, N, x, (long long)x_pitch, W, bias, y);
  }
  DCL_LAUNCH_CHECK();
  return 0;
}

DCL_API int dcl_linear_narrow_fwd_host(int64_t M, int K, int N, const float *x, int64_t x_pitch, const float *W,
                                       const float *bias, float *y) {
  DCL_CHECK_ARG(ln_dims_ok(M, K, N));
  if (M == 0) return 0;
  DCL_CHECK_ARG(x && W && y && ln_pitch_ok(M, K, x_pitch) && ln_grid_ok(M, K));
  for (size_t m = 0; m < (size_t)M; ++m) {
    float v[kLnMaxN][kLnLanes];
    for (int lane = 0; lane < kLnLanes; ++lane) {
      float acc[kLnMaxN][kLnVec];
      ln_row_lane<false, kLnMaxN>(x + m * (size_t)x_pitch, W, K, N, lane, acc);
      for (int j = 0; j < N; ++j) v[j][lane] = ln_lane_fold(acc[j]);
    }
    for (int j = 0; j < N; ++j) {
      const float out = ln_butterfly_host(v[j]);
      y[m * N + j] = bias ? out + bias[j] : out;
    }
  }
  return 0;
}

DCL_API int dcl_linear_narrow_bwd_ws_bytes(int64_t M, int K, int N, int64_t *bytes_host) {
  DCL_CHECK_ARG(ln_dims_ok(M, K, N) && bytes_host && ln_grid_ok(M, K));
  *bytes_host = (int64_t)sizeof(float) * ln_ws_floats(M, K, N);
  return 0;
}

DCL_API int dcl_linear_narrow_bwd(int64_t M, int K, int N, const float *x, int64_t x_pitch, const float *W, const float *g,
                                  float *dx, float *dW, float *db, void *ws, int64_t ws_bytes, dclStream_t stream) {
  DCL_CHECK_ARG(ln_dims_ok(M, K, N));
  if (M == 0) return 0;
  DCL_CHECK_ARG(x && W && g && (dx || dW || db) && ln_pitch_ok(M, K, x_pitch) && ln_grid_ok(M, K));
  const bool sums = dW || db;                                // the scratch holds the chunks' partials: only dW / db need it
  DCL_CHECK_ARG(!sums || (ws && ws_bytes >= (int64_t)sizeof(float) * ln_ws_floats(M, K, N)));
  hipStream_t s = (hipStream_t)stream;
  float *part = sums ? (float *)ws : nullptr;
  const int K4 = (K + kLnVec - 1) / kLnVec;
  const long long nchunks = ln_nchunks(M), pfloats = ln_part_floats(K, N);
  const bool vec = (K & 3) == 0 && (x_pitch & 3) == 0 && cpg_aligned16(x) && cpg_aligned16(W) && cpg_aligned16(dx) &&
                   cpg_aligned16(part);
  const dim3 grid((unsigned)((nchunks * K4 + 255) / 256));
  LN_DISPATCH(k_ln_bwd, vec, N, grid, dim3(256), 0, s, (long long)M, K, N, K4, nchunks, pfloats, x, (long long)x_pitch, W, g, dx,
              part);
  if (sums) {
    const int NK = N * K, E = NK + N;
    hipLaunchKernelGGL(k_ln_finish, dim3((unsigned)dcl_div_up(E, kFinCols)), dim3(kFinCols * kFinGroups), 0, s, nchunks, NK, E,
                       pfloats, part, dW, db);
  }
  DCL_LAUNCH_CHECK();
  return 0;
}

DCL_API int dcl_linear_narrow_bwd_host(int64_t M, int K, int N, const float *x, int64_t x_pitch, const float *W, const float *g,
                                       float *dx, float *dW, float *db) {
  DCL_CHECK_ARG(ln_dims_ok(M, K, N));
  if (M == 0) return 0;
  DCL_CHECK_ARG(x && W && g && (dx || dW || db) && ln_pitch_ok(M, K, x_pitch) && ln_grid_ok(M, K));
  const bool sums = dW || db;
  const long long nchunks = ln_nchunks(M);
  std::vector<float> tw((size_t)N * K), tb((size_t)N);
  for (long long q = 0; q < nchunks; ++q) {
    const long long m0 = q * kLnRows;
    const int rows = (int)(M - m0 < kLnRows ? M - m0 : kLnRows);
    for (int k = 0; k < K; k += kLnVec) {
      float4 pw[kLnMaxN];
      float pb[kLnMaxN];
      ln_bwd_chunk<false, kLnMaxN>(x, x_pitch, W, g, K, N, m0, rows, k, dx, sums, pw, pb);
      if (!sums) continue;
      for (int j = 0; j < N; ++j) {
        const float p[kLnVec] = {pw[j].x, pw[j].y, pw[j].z, pw[j].w};
        for (int e = 0; e < kLnVec && k + e < K; ++e) {
          float &t = tw[(size_t)j * K + k + e];
          t = q == 0 ? p[e] : t + p[e];
        }
        if (k == 0) tb[j] = q == 0 ? pb[j] : tb[j] + pb[j];
      }
    }
  }
  if (dW)
    for (size_t i = 0; i < tw.size(); ++i) dW[i] = tw[i];
  if (db)
    for (int j = 0; j < N; ++j) db[j] = tb[j];
  return 0;
}
