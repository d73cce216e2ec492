// readout_grad.hip -- the gradient of the multi-scale voxel read-out (three_interpolate_grad of libs/pointnet_sp,
// interpolate_gpu.cu:124-148) as an ordered gather: dcl_three_interpolate_grad_sp_ordered.
//
// grad_points[j][ch] = sum over the flat positions q = 3p + k with idx[q] == j, in ASCENDING q, of
// fmul(grad_out[p][ch], weight[q]), one rounded product and one rounded add at a time, starting from +0 -- numpy.add.at on
// float32, and one of the orders the reference's atomic scatter could have produced.  grad_out is (n, c) with a row stride
// (a column block of the 480-channel concat's gradient is read where it lies), grad_points (m, c) is written whole.
//
// MI355X mapping.  The layout is row-major and flat over all crops, m reaches several hundred thousand voxel rows at the
// first level and a few hundred at the last.  At every level more than half of the rows are named by nobody and the named
// ones collect hundreds to thousands of positions (measured: profiles/readout_grad.txt).  Two parts:
//   inverse index (from idx alone, shared by all channels; workspace linear in 3n + m)
//     k_ro_count        cnt[j] += 1 per position (integer atomics)
//     k_ro_chunk_sums   the counts of each of <= 1024 chunks of rows
//     k_ro_starts       start[j] = exclusive prefix of cnt (a chunk adds the sums of the chunks in front of it itself: no
//                       workgroup waits for another); cursor[j] = start[j]
//     k_ro_place        tmp[cursor[j]++] = q (integer atomics: a row's entries arrive in any order)
//     k_ro_sort         every row's entries ascending -> rows[e] = q / 3, wl[e] = weight[q].  After the sort nothing depends
//                       on the order the atomics were served in.  Lists of up to 64 entries (nearly all rows of the fine
//                       levels) are ranked in one wave's registers; longer ones by the workgroup, bitonic in LDS up to
//                       8192 entries.  A workgroup owns 32 rows where lists are short on average and ONE row where they
//                       are long (3n / m > 64: the last level, where every row is long and rows are few), so that
//                       the long sorts spread over the chip.  Beyond 8192 entries a list is ranked by counting smaller
//                       entries straight from memory: len^2 / 256 reads per thread of ONE workgroup, 2.8 million
//                       at 27 000 entries, 39 million at 10^5, growing with the square and with no bound below
//                       3n < 2^31 -- a degenerate batch that piles its positions on one row (three_nn_sp names row 0
//                       for every missing neighbour) keeps one CU busy that long.  At 1024 points per crop the longest
//                       list is 1024 entries; at 12288 points per crop a whole crop's points name one last-level row
//                       and the 12288-entry lists take this form: 17 of that shape's 21 ms (profiles/readout_grad.txt)
//   gather
//     k_ro_gather       lanes over channels, 16 bytes per lane: a row of c floats takes c/4 lanes, so a wave holds
//                       256/c output rows (8 at c = 32, 1 at c = 256) and every load instruction covers whole 128-byte
//                       segments of the grad_out rows it names.  A lane walks its row's list four entries at a time: the
//                       four grad_out rows of a step are loaded together at its top, and the LIST entries (source row and
//                       weight) of the next step are requested under them, so a step's row loads wait for no index; the
//                       rows themselves are not requested a step ahead.  The adds stay in list order.  Odd widths,
//                       strides or bases: the same kernel with one float per lane.
// No float atomics, no workgroup waits for another, nothing is read back to the host.
#include "common.h"

namespace {

constexpr int kRoBlock = 256;
constexpr int kRoMaxChunks = 1024;             // chunks of rows of the prefix sum (their sums: 4 KiB of workspace)
constexpr int kRoSortRows = 32;                // rows per sorting workgroup where lists are short (one where they are long)
constexpr int kRoSortLds = 8192;               // longest list sorted in LDS
constexpr int kRoAhead = 4;                    // list entries per step of the gather

struct RoWs {
  int32_t *start, *cur, *bsum, *tmp, *rows;
  float *wl;
};

// start[m + 1], cursor[m], chunk sums[1024], then three arrays of 3n: placed positions, sorted source rows, their weights
long long ro_ws(int n, int m, void *ws, RoWs *out) {
  const long long nq = 3ll * n;
  const long long sz[6] = {(long long)m + 1, m, kRoMaxChunks, nq, nq, nq};
  long long off[6], total = 0;
  for (int i = 0; i < 6; ++i) {
    off[i] = total;
    total += sz[i] * 4;
  }
  if (ws && out) {
    char *p = static_cast<char *>(ws);
    out->start = reinterpret_cast<int32_t *>(p + off[0]);
    out->cur = reinterpret_cast<int32_t *>(p + off[1]);
    out->bsum = reinterpret_cast<int32_t *>(p + off[2]);
    out->tmp = reinterpret_cast<int32_t *>(p + off[3]);
    out->rows = reinterpret_cast<int32_t *>(p + off[4]);
    out->wl = reinterpret_cast<float *>(p + off[5]);
  }
  return total;
}

bool ro_shape_ok(int c, int n, int m) {
  return c >= 0 && n >= 0 && m >= 0 && 3ll * n < (1ll << 31) - 8192 && m < (1 << 30) && c <= 65535;
}

// rows per chunk of the prefix sum: a multiple of the workgroup size, at most kRoMaxChunks chunks
int ro_chunk(int m) { return kRoBlock * max(8, dcl_div_up(m, (long long)kRoMaxChunks * kRoBlock)); }

__global__ void k_ro_count(const int32_t *__restrict__ idx, int nq, int m, int32_t *__restrict__ cnt) {
  for (long long q = blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += gridDim.x * blockDim.x) {
    const int j = idx[q];
    if ((unsigned)j < (unsigned)m) atomicAdd(cnt + j, 1);
  }
}

// sum of the workgroup's 256 values, in every thread
__device__ __forceinline__ int ro_block_sum(int v, int32_t *part) {
  const int t = threadIdx.x;
  part[t] = v;
  __syncthreads();
  for (int d = kRoBlock / 2; d > 0; d >>= 1) {
    if (t < d) part[t] += part[t + d];
    __syncthreads();
  }
  const int s = part[0];
  __syncthreads();
  return s;
}

__global__ __launch_bounds__(kRoBlock) void k_ro_chunk_sums(const int32_t *__restrict__ cnt, int m, int chunk,
                                                            int32_t *__restrict__ bsum) {
  __shared__ int32_t part[kRoBlock];
  const int lo = blockIdx.x * chunk, hi = min(lo + chunk, m);
  int s = 0;
  for (int i = lo + threadIdx.x; i < hi; i += kRoBlock) s += cnt[i];
  s = ro_block_sum(s, part);
  if (threadIdx.x == 0) bsum[blockIdx.x] = s;
}

// cur holds the counts on entry and the start offsets (the cursors of k_ro_place) on exit
__global__ __launch_bounds__(kRoBlock) void k_ro_starts(int32_t *__restrict__ cur, int m, int chunk,
                                                        const int32_t *__restrict__ bsum, int32_t *__restrict__ start) {
  __shared__ int32_t part[kRoBlock];
  const int t = threadIdx.x, blk = blockIdx.x;
  int s = 0;
  for (int b = t; b < blk; b += kRoBlock) s += bsum[b];
  const int base = ro_block_sum(s, part);
  const int per = chunk / kRoBlock;                                  // consecutive rows per thread
  const int lo = min(blk * chunk + t * per, m), hi = min(lo + per, m);
  int own = 0;
  for (int i = lo; i < hi; ++i) own += cur[i];
  part[t] = own;
  __syncthreads();
  for (int d = 1; d < kRoBlock; d <<= 1) {
    const int v = t >= d ? part[t - d] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int run = base + part[t] - own;
  for (int i = lo; i < hi; ++i) {
    const int v = cur[i];
    cur[i] = run;
    start[i] = run;
    run += v;
  }
  if (blk == (int)gridDim.x - 1 && t == kRoBlock - 1) start[m] = base + part[kRoBlock - 1];
}

__global__ void k_ro_place(const int32_t *__restrict__ idx, int nq, int m, int32_t *__restrict__ cur,
                           int32_t *__restrict__ tmp) {
  for (long long q = blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += gridDim.x * blockDim.x) {
    const int j = idx[q];
    if ((unsigned)j < (unsigned)m) tmp[atomicAdd(cur + j, 1)] = (int32_t)q;
  }
}

// tmp[start[j] .. start[j+1]) in any order -> the same positions ascending, as source row and weight
__global__ __launch_bounds__(kRoBlock) void k_ro_sort(const int32_t *__restrict__ start, int m, int rows_per_group,
                                                      const int32_t *__restrict__ tmp, const float *__restrict__ weight,
                                                      int32_t *__restrict__ rows, float *__restrict__ wl) {
  __shared__ int32_t sh[kRoSortLds];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int j0 = blockIdx.x * rows_per_group, j1 = min(j0 + rows_per_group, m);
  // lists of one wave's width: a lane's entry goes where the number of smaller entries says (positions are distinct)
  for (int j = j0 + wave; j < j1; j += kRoBlock / 64) {
    const int s = start[j], len = start[j + 1] - s;
    if (len > 64) continue;
    const int x = lane < len ? tmp[s + lane] : INT_MAX;
    int r = 0;
    for (int i = 0; i < len; ++i) r += __shfl(x, i) < x;
    if (lane < len) {
      rows[s + r] = x / 3;
      wl[s + r] = weight[x];
    }
  }
  // longer lists: the whole workgroup, one list at a time (s and len are the same in every thread)
  for (int j = j0; j < j1; ++j) {
    const int s = start[j], len = start[j + 1] - s;
    if (len <= 64) continue;
    if (len <= kRoSortLds) {
      int p2 = 128;
      while (p2 < len) p2 <<= 1;
      for (int i = t; i < p2; i += kRoBlock) sh[i] = i < len ? tmp[s + i] : INT_MAX;
      __syncthreads();
      for (int k = 2; k <= p2; k <<= 1)
        for (int d = k >> 1; d > 0; d >>= 1) {
          for (int i = t; i < p2; i += kRoBlock) {
            const int o = i ^ d;
            if (o > i) {
              const int a = sh[i], b = sh[o];
              if ((a > b) == ((i & k) == 0)) {
                sh[i] = b;
                sh[o] = a;
              }
            }
          }
          __syncthreads();
        }
      for (int i = t; i < len; i += kRoBlock) {
        const int x = sh[i];
        rows[s + i] = x / 3;
        wl[s + i] = weight[x];
      }
      __syncthreads();
    } else {
      for (int i = t; i < len; i += kRoBlock) {
        const int x = tmp[s + i];
        int r = 0;
        for (int y = 0; y < len; ++y) r += tmp[s + y] < x;
        rows[s + r] = x / 3;
        wl[s + r] = weight[x];
      }
    }
  }
}

template <int W> struct RoVec;
template <> struct RoVec<4> {
  typedef float4 T;
  static __device__ __forceinline__ T zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
  static __device__ __forceinline__ T add_scaled(T a, T g, float w) {
    a.x = __fadd_rn(a.x, __fmul_rn(g.x, w));
    a.y = __fadd_rn(a.y, __fmul_rn(g.y, w));
    a.z = __fadd_rn(a.z, __fmul_rn(g.z, w));
    a.w = __fadd_rn(a.w, __fmul_rn(g.w, w));
    return a;
  }
};
template <> struct RoVec<1> {
  typedef float T;
  static __device__ __forceinline__ T zero() { return 0.f; }
  static __device__ __forceinline__ T add_scaled(T a, T g, float w) { return __fadd_rn(a, __fmul_rn(g, w)); }
};

// W floats per lane; 1 << lpr_log2 lanes per output row (a wave holds 64 >> lpr_log2 rows); rows wider than 64 lanes' worth
// are walked in several passes
template <int W>
__global__ __launch_bounds__(kRoBlock) void k_ro_gather(int c, int m, int lpr_log2, const float *__restrict__ grad_out,
                                                        long long stride, const int32_t *__restrict__ start,
                                                        const int32_t *__restrict__ rows, const float *__restrict__ wl,
                                                        float *__restrict__ grad_points) {
  typedef typename RoVec<W>::T V;
  const int lane = threadIdx.x & 63, wave = blockIdx.x * (kRoBlock / 64) + (threadIdx.x >> 6);
  const int lpr = 1 << lpr_log2, sub = lane & (lpr - 1);
  const long long jl = ((long long)wave << (6 - lpr_log2)) + (lane >> lpr_log2);
  if (jl >= m) return;
  const int j = (int)jl;
  const int s0 = start[j], s1 = start[j + 1];
  const int units = c / W;
  for (int u0 = sub; u0 < units; u0 += lpr) {
    const float *G = grad_out + (size_t)u0 * W;
    V acc = RoVec<W>::zero();
    int p[kRoAhead];
    float w[kRoAhead];
#pragma unroll
    for (int u = 0; u < kRoAhead; ++u) {
      const bool on = s0 + u < s1;
      p[u] = on ? rows[s0 + u] : 0;
      w[u] = on ? wl[s0 + u] : 0.f;
    }
    for (int e = s0; e < s1; e += kRoAhead) {
      V g[kRoAhead];
#pragma unroll
      for (int u = 0; u < kRoAhead; ++u)
        g[u] = e + u < s1 ? *reinterpret_cast<const V *>(G + (size_t)p[u] * stride) : RoVec<W>::zero();
      int pn[kRoAhead];
      float wn[kRoAhead];
#pragma unroll
      for (int u = 0; u < kRoAhead; ++u) {                           // the next entries, in flight under this step's rows
        const bool on = e + kRoAhead + u < s1;
        pn[u] = on ? rows[e + kRoAhead + u] : 0;
        wn[u] = on ? wl[e + kRoAhead + u] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < kRoAhead; ++u)
        if (e + u < s1) acc = RoVec<W>::add_scaled(acc, g[u], w[u]);
#pragma unroll
      for (int u = 0; u < kRoAhead; ++u) {
        p[u] = pn[u];
        w[u] = wn[u];
      }
    }
    *reinterpret_cast<V *>(grad_points + (size_t)j * c + (size_t)u0 * W) = acc;
  }
}

}  // namespace

DCL_API int dcl_three_interpolate_grad_sp_ws_bytes(int c, int n, int m, int64_t *bytes_host) {
  DCL_CHECK_ARG(ro_shape_ok(c, n, m) && bytes_host);
  *bytes_host = ro_ws(n, m, nullptr, nullptr);
  return 0;
}

DCL_API int dcl_three_interpolate_grad_sp_ordered(int c, int n, int m, const float *grad_out, int64_t grad_stride,
                                                  const int32_t *idx, const float *weight, float *grad_points, void *ws,
                                                  int64_t ws_bytes, dclStream_t stream) {
  DCL_CHECK_ARG(ro_shape_ok(c, n, m) && grad_stride >= c);
  if (c == 0 || m == 0) return 0;
  DCL_CHECK_ARG(grad_points);
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) {
    const hipError_t e = hipMemsetAsync(grad_points, 0, (size_t)m * c * 4, s);
    if (e != hipSuccess) {
      dcl_set_error("%s: memset failed: %s", __func__, hipGetErrorString(e));
      return (int)e;
    }
    return 0;
  }
  DCL_CHECK_ARG(grad_out && idx && weight && ws);
  RoWs w;
  if (ws_bytes < ro_ws(n, m, ws, &w)) {
    dcl_set_error("%s: invalid argument: ws_bytes %lld < %lld", __func__, (long long)ws_bytes,
                  ro_ws(n, m, nullptr, nullptr));
    return DCL_EINVAL;
  }
  const int nq = 3 * n;
  const hipError_t e = hipMemsetAsync(w.cur, 0, (size_t)m * 4, s);
  if (e != hipSuccess) {
    dcl_set_error("%s: memset failed: %s", __func__, hipGetErrorString(e));
    return (int)e;
  }
  const int chunk = ro_chunk(m), nchunks = dcl_div_up(m, chunk);
  hipLaunchKernelGGL(k_ro_count, dim3(dcl_grid_1d(nq, kRoBlock)), dim3(kRoBlock), 0, s, idx, nq, m, w.cur);
  hipLaunchKernelGGL(k_ro_chunk_sums, dim3(nchunks), dim3(kRoBlock), 0, s, w.cur, m, chunk, w.bsum);
  hipLaunchKernelGGL(k_ro_starts, dim3(nchunks), dim3(kRoBlock), 0, s, w.cur, m, chunk, w.bsum, w.start);
  hipLaunchKernelGGL(k_ro_place, dim3(dcl_grid_1d(nq, kRoBlock)), dim3(kRoBlock), 0, s, idx, nq, m, w.cur, w.tmp);
  const int sort_rows = nq / m > 64 ? 1 : kRoSortRows;
  hipLaunchKernelGGL(k_ro_sort, dim3(dcl_div_up(m, sort_rows)), dim3(kRoBlock), 0, s, w.start, m, sort_rows, w.tmp, weight,
                     w.rows, w.wl);
  // 16-byte loads and stores where every row of both arrays starts on a 16-byte boundary
  const bool vec = c % 4 == 0 && grad_stride % 4 == 0 && (reinterpret_cast<uintptr_t>(grad_out) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(grad_points) & 15) == 0;
  const int units = vec ? c / 4 : c;
  int lpr_log2 = 0;
  while (lpr_log2 < 6 && (1 << lpr_log2) < units) ++lpr_log2;
  const int rows_per_block = (kRoBlock / 64) * (64 >> lpr_log2);
  const dim3 grid(dcl_div_up(m, rows_per_block));
  if (vec)
    hipLaunchKernelGGL(k_ro_gather<4>, grid, dim3(kRoBlock), 0, s, c, m, lpr_log2, grad_out, (long long)grad_stride, w.start,
                       w.rows, w.wl, grad_points);
  else
    hipLaunchKernelGGL(k_ro_gather<1>, grid, dim3(kRoBlock), 0, s, c, m, lpr_log2, grad_out, (long long)grad_stride, w.start,
                       w.rows, w.wl, grad_points);
  DCL_LAUNCH_CHECK();
  return 0;
}
