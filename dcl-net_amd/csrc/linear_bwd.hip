// linear_bwd.hip -- the training side of a per-point Linear + ReLU stack (the stage-2 refiner's MLP_share): the weight-gradient
// GEMM and the ReLU mask with the bias gradient.  The input gradients are plain GEMMs of the forward core (dcl_linear_dma_fwd
// with the registered (out, in) weight as its (K x N) matrix), so nothing else is needed to train such a stack on the library's
// own kernels.
//
// dcl_linear_wgrad: dW[p][q] = sum_j a[j][p] b[j][q] (a = dZ (M x P), b = the layer input (M x Q), both row-major).
//   * v_mfma_f32_32x32x2_f32 in its transposed-A form: lane l of BOTH operands holds element [row j0 + (l >> 5)][col c0 + (l & 31)],
//     so row-major slabs of a and b go to LDS as they lie and feed the pipe without a transpose; exact fp32, one rounding per
//     product, an output element is ONE accumulator fed by the rows in ascending order.
//   * the M rows are cut into splits of DCL_WGRAD_ROWS rows (a function of M alone); a workgroup owns one (P, Q) tile of one
//     split -- its 4 waves tile (P, Q), never the rows -- and writes partial[split]; k_split_sum adds the splits ascending.
//     No float atomics, no workgroup waits on another: the same operands give the same bits on every call.
//   * one kernel body for every shape: loads are guarded and zero-filled (a zero row or column adds +0 to an accumulator, which
//     changes no bit), the 16-byte vector load is only a fast path for aligned bases and pitches, and the order of the arithmetic
//     never depends on pitches or alignment.  Two instantiations differ in the tile only: 128 x 128 (2 x 2 waves of 64 x 64) and
//     128 x 32 (4 x 1 waves of 32 x 32) for Q <= 32 (the xyz block, Q = 3).
// dcl_relu_bwd: dz = h > 0 ? g : 0 (or the pooled last layer's roww[j] * gpool[crop][p]) with db[p] = sum_j dz[j][p]: lanes run
//   over columns (a row's loads are coalesced); a workgroup owns 64 columns of one split, its four waves stream the rows through
//   LDS in chunks and one lane per column adds them in ascending order with one FLOAT64 accumulator that is rounded to fp32 once
//   per split (a single fp32 chain over 512 masked gradients of mixed sign missed the project's float64 rule on the network's own
//   operands, tests/test_gpu_step_replay.py); k_split_sum adds the splits ascending.
#include "common.h"
#include "mfma_tile.h"

namespace {

constexpr int kWgKC = 16;            // rows per LDS slab (8 MFMA k-steps)
constexpr int kWgPad = 32;           // slab row pitch = tile width + 32 floats: the two lane halves (rows j, j + 1) hit different banks
constexpr int kWgThreads = 256;

// 4 consecutive floats of row `row`, columns c .. c + 3 of a (rows x cols) row-major matrix with pitch ld; 0 outside
__device__ __forceinline__ float4 wg_load4(const float *m, int64_t ld, int64_t row, int64_t row_hi, int c, int cols, bool vec_ok) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (row >= row_hi || c >= cols) return v;
  const float *p = m + (size_t)row * (size_t)ld + c;
  if (vec_ok && c + 3 < cols) return *reinterpret_cast<const float4 *>(p);
  v.x = p[0];
  if (c + 1 < cols) v.y = p[1];
  if (c + 2 < cols) v.z = p[2];
  if (c + 3 < cols) v.w = p[3];
  return v;
}

// one operand's slab of kWgKC rows x W columns: global -> registers (prefetch) and registers -> LDS
template <int W>
struct WgSlab {
  static constexpr int kItems = kWgKC * W / 4;                                 // float4 items
  static constexpr int kPer = (kItems + kWgThreads - 1) / kWgThreads;
  static constexpr int kPitch = W + kWgPad;
  float4 r[kPer];
  __device__ __forceinline__ void fetch(const float *m, int64_t ld, int64_t j0, int64_t row_hi, int c0, int cols, bool vec_ok) {
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
      const int item = threadIdx.x + i * kWgThreads;
      const int row = item / (W / 4), c4 = (item - row * (W / 4)) * 4;
      r[i] = item < kItems ? wg_load4(m, ld, j0 + row, row_hi, c0 + c4, cols, vec_ok) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  __device__ __forceinline__ void put(float *lds) const {
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
      const int item = threadIdx.x + i * kWgThreads;
      const int row = item / (W / 4), c4 = (item - row * (W / 4)) * 4;
      if (item < kItems) *reinterpret_cast<float4 *>(lds + row * kPitch + c4) = r[i];
    }
  }
};

// WP x WQ waves (= 4), each TP x TQ accumulator tiles of 32 x 32: the workgroup's tile is (32 WP TP) x (32 WQ TQ)
template <int WP, int WQ, int TP, int TQ>
__global__ __launch_bounds__(kWgThreads) void k_linear_wgrad(const float *__restrict__ a, int64_t lda, const float *__restrict__ b,
                                                             int64_t ldb, int M, int P, int Q, int tiles_p, int tiles_q,
                                                             float *__restrict__ partial) {
  static_assert(WP * WQ * 64 == kWgThreads, "four waves");
  constexpr int BP = 32 * WP * TP, BQ = 32 * WQ * TQ;
  constexpr int PA = BP + kWgPad, PB = BQ + kWgPad;
  __shared__ __attribute__((aligned(16))) float As[2][kWgKC * PA];
  __shared__ __attribute__((aligned(16))) float Bs[2][kWgKC * PB];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
  const int wp = wave / WQ, wq = wave - wp * WQ;
  // workgroup -> (split, tile): the tiles of one split are neighbours, so they read the same rows of a and b together
  const int tiles = tiles_p * tiles_q;
  const int split = blockIdx.x / tiles, tile = blockIdx.x - split * tiles;
  const int tp = tile / tiles_q, tq = tile - tp * tiles_q;
  const int p0 = tp * BP, q0 = tq * BQ;
  const int64_t row_lo = (int64_t)split * DCL_WGRAD_ROWS;
  const int64_t row_hi = row_lo + DCL_WGRAD_ROWS < (int64_t)M ? row_lo + DCL_WGRAD_ROWS : (int64_t)M;
  const bool vec_a = (((size_t)a & 15) == 0) && (lda & 3) == 0, vec_b = (((size_t)b & 15) == 0) && (ldb & 3) == 0;

  f32x16 acc[TP][TQ];
#pragma unroll
  for (int i = 0; i < TP; ++i)
#pragma unroll
    for (int j = 0; j < TQ; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;

  WgSlab<BP> sa;
  WgSlab<BQ> sb;
  const int nchunks = (int)((row_hi - row_lo + kWgKC - 1) / kWgKC);
  sa.fetch(a, lda, row_lo, row_hi, p0, P, vec_a);
  sb.fetch(b, ldb, row_lo, row_hi, q0, Q, vec_b);
  sa.put(As[0]);
  sb.put(Bs[0]);
  __syncthreads();
  for (int c = 0; c < nchunks; ++c) {
    const int cur = c & 1;
    if (c + 1 < nchunks) {                                   // the next slab's loads fly during this slab's MFMAs
      const int64_t j0 = row_lo + (int64_t)(c + 1) * kWgKC;
      sa.fetch(a, lda, j0, row_hi, p0, P, vec_a);
      sb.fetch(b, ldb, j0, row_hi, q0, Q, vec_b);
    }
    const float *A = As[cur] + h * PA + wp * (32 * TP) + r;
    const float *B = Bs[cur] + h * PB + wq * (32 * TQ) + r;
#pragma unroll
    for (int s = 0; s < kWgKC / 2; ++s) {                    // k-step s: rows 2s (lanes 0..31) and 2s + 1 (lanes 32..63), ascending
      float av[TP], bv[TQ];
#pragma unroll
      for (int i = 0; i < TP; ++i) av[i] = A[2 * s * PA + 32 * i];
#pragma unroll
      for (int j = 0; j < TQ; ++j) bv[j] = B[2 * s * PB + 32 * j];
#pragma unroll
      for (int i = 0; i < TP; ++i)
#pragma unroll
        for (int j = 0; j < TQ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[j], acc[i][j], 0, 0, 0);
    }
    if (c + 1 < nchunks) {                                   // (the other buffer: last read before the previous barrier)
      sa.put(As[cur ^ 1]);
      sb.put(Bs[cur ^ 1]);
    }
    __syncthreads();
  }
  // accumulator register e of lane half h: output row rowmap(e, h), column lane & 31
  float *out = partial + (size_t)split * (size_t)P * (size_t)Q;
#pragma unroll
  for (int i = 0; i < TP; ++i)
#pragma unroll
    for (int j = 0; j < TQ; ++j) {
      const int q = q0 + wq * (32 * TQ) + 32 * j + r;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int p = p0 + wp * (32 * TP) + 32 * i + rowmap(e, h);
        if (p < P && q < Q) out[(size_t)p * Q + q] = acc[i][j][e];
      }
    }
}

// out[p][q] (pitch ldo) = partial[0][p][q] + partial[1][p][q] + ... in split order (nsplit == 0: +0)
__global__ __launch_bounds__(256) void k_split_sum(const float *__restrict__ partial, int nsplit, int P, int Q,
                                                   float *__restrict__ out, int64_t ldo) {
  const size_t n = (size_t)P * (size_t)Q;
  for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (size_t)gridDim.x * blockDim.x) {
    float s = nsplit > 0 ? partial[t] : 0.0f;
    for (int z = 1; z < nsplit; ++z) s = s + partial[(size_t)z * n + t];
    const size_t p = t / (size_t)Q, q = t - p * (size_t)Q;
    out[p * (size_t)ldo + q] = s;
  }
}

constexpr int kRbCols = 64;        // columns of a workgroup's strip
constexpr int kRbRows = 64;        // rows per chunk: 16 lanes x float4 cover a row of the strip, 256 threads 16 rows, 4 rows each
constexpr int kRbThreads = 256;

__device__ __forceinline__ void rb_store4(float *m, int64_t ld, int64_t row, int64_t row_hi, int c, int cols, bool vec_ok, float4 v) {
  if (row >= row_hi || c >= cols) return;
  float *p = m + (size_t)row * (size_t)ld + c;
  if (vec_ok && c + 3 < cols) {
    *reinterpret_cast<float4 *>(p) = v;
    return;
  }
  p[0] = v.x;
  if (c + 1 < cols) p[1] = v.y;
  if (c + 2 < cols) p[2] = v.z;
  if (c + 3 < cols) p[3] = v.w;
}
__device__ __forceinline__ bool rb_vec_ok(const void *p, int64_t ld) { return (((size_t)p & 15) == 0) && (ld & 3) == 0; }

// One workgroup per (strip of 64 columns, split); g == nullptr: the pooled form.  All four waves load, mask and store chunks of
// 64 rows (coalesced 256-byte row pieces, many in flight) and leave the chunk's dz in LDS; wave 0, one lane per column, then
// adds the chunk's rows to its float64 accumulator in ascending order -- the bias gradient's pinned chain -- while the other waves are
// already loading the next chunk (two LDS buffers, one barrier per chunk).  dz may be g (first form) or h (pooled form): a
// thread reads an element before it writes it and touches no other thread's, so no pointer here is __restrict__.
__global__ __launch_bounds__(kRbThreads) void k_relu_bwd(const float *h, int64_t ldh, const float *g, int64_t ldg,
                                                         const float *roww, const float *gpool, int64_t ldgp, int rows_per_crop,
                                                         int M, int P, float *dz, int64_t lddz, float *partial) {
  __shared__ __attribute__((aligned(16))) float tile[2][kRbRows * kRbCols];
  const int t = threadIdx.x, c4 = (t & 15) * 4, r0 = t >> 4;
  const int p0 = blockIdx.x * kRbCols, c = p0 + c4;
  const int split = blockIdx.y;
  const int64_t row_lo = (int64_t)split * DCL_WGRAD_ROWS;
  const int64_t row_hi = row_lo + DCL_WGRAD_ROWS < (int64_t)M ? row_lo + DCL_WGRAD_ROWS : (int64_t)M;
  const bool vh = rb_vec_ok(h, ldh), vg = g ? rb_vec_ok(g, ldg) : rb_vec_ok(gpool, ldgp), vz = rb_vec_ok(dz, lddz);
  const int nchunks = (int)((row_hi - row_lo + kRbRows - 1) / kRbRows);
  double acc = 0.0;
  for (int ch = 0; ch < nchunks; ++ch) {
    const int64_t j0 = row_lo + (int64_t)ch * kRbRows;
    float4 hv[kRbRows / 16], gv[kRbRows / 16];
#pragma unroll
    for (int i = 0; i < kRbRows / 16; ++i) {
      const int64_t j = j0 + r0 + 16 * i;
      hv[i] = wg_load4(h, ldh, j, row_hi, c, P, vh);
      if (g) {
        gv[i] = wg_load4(g, ldg, j, row_hi, c, P, vg);
      } else {
        const bool in = j < row_hi;
        const float w = in ? roww[j] : 0.0f;
        const float4 gp = wg_load4(gpool, ldgp, in ? j / rows_per_crop : 0, in ? INT64_MAX : 0, c, P, vg);
        gv[i] = make_float4(__fmul_rn(w, gp.x), __fmul_rn(w, gp.y), __fmul_rn(w, gp.z), __fmul_rn(w, gp.w));
      }
    }
    float *T = tile[ch & 1];
#pragma unroll
    for (int i = 0; i < kRbRows / 16; ++i) {
      const int64_t j = j0 + r0 + 16 * i;
      float4 d;                                              // (rows and columns outside the problem were loaded as h = 0: d = 0)
      d.x = hv[i].x > 0.0f ? gv[i].x : 0.0f;
      d.y = hv[i].y > 0.0f ? gv[i].y : 0.0f;
      d.z = hv[i].z > 0.0f ? gv[i].z : 0.0f;
      d.w = hv[i].w > 0.0f ? gv[i].w : 0.0f;
      rb_store4(dz, lddz, j, row_hi, c, P, vz, d);
      *reinterpret_cast<float4 *>(T + (r0 + 16 * i) * kRbCols + c4) = d;
    }
    __syncthreads();
    if (t < kRbCols) {
      const int n = row_hi - j0 < kRbRows ? (int)(row_hi - j0) : kRbRows;
#pragma unroll 8
      for (int r = 0; r < n; ++r) acc = acc + (double)T[r * kRbCols + t];      // rows ascending, one float64 accumulator
    }
  }
  if (t < kRbCols && p0 + t < P) partial[(size_t)split * P + p0 + t] = (float)acc;      // one rounding per split
}

bool aligned4(const void *p) { return ((size_t)p & 3) == 0; }

}  // namespace

// dW (P x Q, pitch lddw) = the nsplit partial results added in ascending split order (k_split_sum); nsplit == 0 zero-fills.  Shared
// with the split-bf16 weight gradient (linear_wgrad_split.hip): one kernel adds the splits of both.
int dcl_internal_split_sum(const float *partial, int nsplit, int P, int Q, float *dW, int64_t lddw, hipStream_t s) {
  hipLaunchKernelGGL(k_split_sum, dim3(dcl_grid_1d((long long)P * Q, 256)), dim3(256), 0, s, partial, nsplit, P, Q, dW, lddw);
  DCL_LAUNCH_CHECK();
  return 0;
}

DCL_API int dcl_linear_wgrad_splits(int M, int32_t *splits_host) {
  DCL_CHECK_ARG(M >= 0 && splits_host);
  const int s = dcl_div_up(M, DCL_WGRAD_ROWS);
  *splits_host = s < 1 ? 1 : s;
  return 0;
}

DCL_API int dcl_linear_wgrad(const float *a, int64_t lda, const float *b, int64_t ldb, int M, int P, int Q, float *partial,
                             float *dW, int64_t lddw, dclStream_t stream) {
  DCL_CHECK_ARG(M >= 0 && P >= 1 && Q >= 1 && lda >= P && ldb >= Q && lddw >= Q);
  DCL_CHECK_ARG(dW && partial && aligned4(dW) && aligned4(partial));
  DCL_CHECK_ARG(M == 0 || (a && b && aligned4(a) && aligned4(b)));
  hipStream_t s = (hipStream_t)stream;
  int splits = 0;
  if (M > 0) {
    (void)dcl_linear_wgrad_splits(M, &splits);
    if (Q <= 32) {
      const int tiles_p = dcl_div_up(P, 128), tiles_q = 1;
      DCL_CHECK_ARG((long long)tiles_p * tiles_q * splits < (1ll << 31));
      hipLaunchKernelGGL((k_linear_wgrad<4, 1, 1, 1>), dim3(tiles_p * tiles_q * splits), dim3(kWgThreads), 0, s, a, lda, b, ldb, M,
                         P, Q, tiles_p, tiles_q, partial);
    } else {
      const int tiles_p = dcl_div_up(P, 128), tiles_q = dcl_div_up(Q, 128);
      DCL_CHECK_ARG((long long)tiles_p * tiles_q * splits < (1ll << 31));
      hipLaunchKernelGGL((k_linear_wgrad<2, 2, 2, 2>), dim3(tiles_p * tiles_q * splits), dim3(kWgThreads), 0, s, a, lda, b, ldb, M,
                         P, Q, tiles_p, tiles_q, partial);
    }
  }
  hipLaunchKernelGGL(k_split_sum, dim3(dcl_grid_1d((long long)P * Q, 256)), dim3(256), 0, s, partial, splits, P, Q, dW, lddw);
  DCL_LAUNCH_CHECK();
  return 0;
}

DCL_API int dcl_relu_bwd(const float *h, int64_t ldh, const float *g, int64_t ldg, const float *roww, const float *gpool,
                         int64_t ldgp, int rows_per_crop, int M, int P, float *dz, int64_t lddz, float *partial, float *db,
                         dclStream_t stream) {
  DCL_CHECK_ARG(M >= 0 && P >= 1 && ldh >= P && lddz >= P && db && partial && aligned4(db) && aligned4(partial));
  DCL_CHECK_ARG(g ? ldg >= P : (ldgp >= P && rows_per_crop >= 1));
  DCL_CHECK_ARG(M == 0 || (h && dz && aligned4(h) && aligned4(dz) && aligned4(g)));
  DCL_CHECK_ARG(M == 0 || g || (roww && gpool && aligned4(roww) && aligned4(gpool)));
  hipStream_t s = (hipStream_t)stream;
  int splits = 0;
  if (M > 0) {
    (void)dcl_linear_wgrad_splits(M, &splits);
    DCL_CHECK_ARG(splits <= 65535);
    hipLaunchKernelGGL(k_relu_bwd, dim3(dcl_div_up(P, kRbCols), splits), dim3(kRbThreads), 0, s, h, ldh, g, ldg, roww, gpool, ldgp,
                       rows_per_crop, M, P, dz, lddz, partial);
  }
  hipLaunchKernelGGL(k_split_sum, dim3(dcl_grid_1d(P, 256)), dim3(256), 0, s, partial, splits, 1, P, db, (int64_t)P);
  DCL_LAUNCH_CHECK();
  return 0;
}
