// backward.hip -- training-side kernels of the ops on DCL-Net's path:
//
//   voxelize_bp            libs/pointgroup_ops/src/voxelize/voxelize.cu:35-50
//   indice_conv backward   libs/spconv/include/spconv/spconv_ops.h:351-438 (per offset: dW[k] = X_k^T dO_k, dX += dO_k W[k]^T)
//   indice_avgpool bwd     libs/spconv/src/spconv/avgpool.cu:178-206, pool_ops.h:211-246 (din[i] += dout[o] / rf[o])
//   three_interpolate grad libs/pointnet_sp/src/interpolate_gpu.cu:124-148
//   pointnet_lib grads     libs/pointnet_lib/src/group_points_gpu.cu:8-25, sampling_gpu.cu:46-63, interpolate_gpu.cu:192-215
//
// MI355X mapping.  The reference scatters (per-offset gather -> GEMM -> scatter-add, or atomics); here everything that
// can be a GATHER is one: the forward rulebook nbr[k][o] = i is transposed once into inv[k][i] = o (every (k, i) has at
// most one o), after which  dX = sparse_conv_fwd(dO, inv, W^T)  reuses the forward MFMA kernel unchanged and the pooling
// gradient is a 27-term gather in the reference's ascending-offset order (bit-exact).  dW is a rows-contracted MFMA GEMM per
// offset: both operands are read straight from global memory with the 32 lanes of a half-wave on 32 consecutive channels
// (coalesced 128-B segments), split over row ranges into partial sums that a second kernel adds in split order
// (deterministic; the reference's cuBLAS order is unspecified, so parity is by tolerance -- and bit for bit on exactly
// representable operands, whose partial sums are integers below 2^24 in any order: tests/test_gpu_conv_backward.py).
// pointnet_sp's interpolation
// gradient is an ordered gather of its own (readout_grad.hip: row-major (n, C) rows, flat over all crops, a workspace linear
// in the problem); the reference's atomic scatter stays below as dcl_three_interpolate_grad_sp, the unspecified-order form
// that tests and tools/bench_readout_grad.py compare it with, and nothing on the training path calls it.  pointnet_lib's three
// gradients are gathers too: an inverse index of idx (each point's positions in ascending order, built once per call and
// shared by all channels) drives an LDS-staged pass that adds each point's contributions in that order -- deterministic,
// and equal to a sequential scatter in position order bit for bit.
#include "common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

__global__ void k_fill_i32(int32_t *__restrict__ p, long long n, int32_t v) {
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (long long)gridDim.x * blockDim.x) p[t] = v;
}

__global__ void k_rulebook_transpose(const int32_t *__restrict__ nbr, int cap_out, const int32_t *__restrict__ n_out_dev,
                                     int n_out_host, int kvol, int32_t *__restrict__ inv, int cap_in) {
  int n = n_out_dev ? *n_out_dev : n_out_host;
  n = n < cap_out ? n : cap_out;
  const long long total = (long long)n * kvol;
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
    const int k = (int)(t / n), o = (int)(t - (long long)k * n);
    const int i = nbr[(size_t)k * cap_out + o];
    if (i >= 0 && i < cap_in) inv[(size_t)k * cap_in + i] = o;
  }
}

// din[i] = ((0 + dout[o_k0]/rf[o_k0]) + dout[o_k1]/rf[o_k1]) + ...  ascending offsets (avgpool.cu:204, pool_ops.h:222)
__global__ void k_sparse_avgpool_bwd(const float *__restrict__ dout, const int32_t *__restrict__ inv, int cap_in, int n_in,
                                     const int32_t *__restrict__ rf, int c, int kvol, float *__restrict__ din) {
  const int c4 = c >> 2;
  const long long total = (long long)n_in * c4;
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
    const int row = (int)(t / c4), q = (int)(t - (long long)row * c4);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k = 0; k < kvol; ++k) {
      const int o = inv[(size_t)k * cap_in + row];
      if (o < 0) continue;
      const float d = (float)rf[o];
      const float4 g = reinterpret_cast<const float4 *>(dout + (size_t)o * c)[q];
      acc.x = acc.x + g.x / d; acc.y = acc.y + g.y / d; acc.z = acc.z + g.z / d; acc.w = acc.w + g.w / d;
    }
    reinterpret_cast<float4 *>(din + (size_t)row * c)[q] = acc;
  }
}

__global__ void k_three_interp_grad_sp(int c, int n, const float *__restrict__ grad_out, const int32_t *__restrict__ idx,
                                       const float *__restrict__ weight, float *__restrict__ grad_points) {
  const long long total = (long long)n * c;
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
    const int p = (int)(t / c), ch = (int)(t - (long long)p * c);
    const float g = grad_out[t];
#pragma unroll
    for (int j = 0; j < 3; ++j) atomicAdd(grad_points + (size_t)idx[p * 3 + j] * c + ch, g * weight[p * 3 + j]);
  }
}

__global__ void k_voxelize_bp(int n_rows, int max_active, int c, const float *__restrict__ d_out,
                              const int32_t *__restrict__ rules, int average, float *__restrict__ d_feats) {
  const long long total = (long long)n_rows * c;
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
    const int row = (int)(t / c), plane = (int)(t - (long long)row * c);
    const int32_t *r = rules + (size_t)row * (max_active + 1);
    const int na = r[0];
    const float mult = (average && na > 0) ? 1.0f / (float)na : 1.0f;
    const float v = mult * d_out[t];
    for (int i = 1; i <= na; ++i) atomicAdd(d_feats + (size_t)r[i] * c + plane, v);
  }
}

// ---- dW[k] = sum_o X[nbr[k][o]]^T dO[o]: one wave = (32*TM) x (32*TN) block of dW[k] over a row range
template <int TM, int TN>
__global__ __launch_bounds__(64) void k_conv_wgrad_mfma(const float *__restrict__ feat, const int32_t *__restrict__ nbr,
                                                        int cap, int n_out, const float *__restrict__ dout, int cin,
                                                        int cout, int rows_per_split, float *__restrict__ partial) {
  const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
  const int tiles_n = cout / (32 * TN);
  const int tm = blockIdx.x / tiles_n, tn = blockIdx.x - tm * tiles_n;
  const int k = blockIdx.y;
  const int ci0 = tm * 32 * TM, co0 = tn * 32 * TN;
  const int row_lo = blockIdx.z * rows_per_split, row_hi = min(row_lo + rows_per_split, n_out);
  f32x16 acc[TM][TN];
#pragma unroll
  for (int a = 0; a < TM; ++a)
#pragma unroll
    for (int b = 0; b < TN; ++b)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.0f;
  for (int o0 = row_lo; o0 < row_hi; o0 += 8) {
    // 4 MFMA steps of 2 rows each; lane half h owns row o0 + 2s + h
    int v[4];
    float av[4][TM], bv[4][TN];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int o = o0 + 2 * s + h;
      v[s] = o < row_hi ? nbr[(size_t)k * cap + o] : -1;
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int o = o0 + 2 * s + h;
#pragma unroll
      for (int a = 0; a < TM; ++a) av[s][a] = v[s] >= 0 ? feat[(size_t)v[s] * cin + ci0 + 32 * a + r] : 0.0f;
#pragma unroll
      for (int b = 0; b < TN; ++b) bv[s][b] = v[s] >= 0 ? dout[(size_t)o * cout + co0 + 32 * b + r] : 0.0f;
    }
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < TN; ++b)
          acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s][a], bv[s][b], acc[a][b], 0, 0, 0);
  }
  asm volatile("s_nop 15\n\ts_nop 7" ::: "memory");
  float *P = partial + ((size_t)blockIdx.z * gridDim.y + k) * cin * cout;
#pragma unroll
  for (int a = 0; a < TM; ++a)
#pragma unroll
    for (int b = 0; b < TN; ++b)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int ci = ci0 + 32 * a + (e & 3) + 8 * (e >> 2) + 4 * h;       // C/D layout: row = (e&3)+8(e>>2)+4h, col = lane&31
        P[(size_t)ci * cout + co0 + 32 * b + r] = acc[a][b][e];
      }
}

// any channel counts: thread = one (ci, co) element of dW[k], running sum over the split's rows in row order
__global__ void k_conv_wgrad_valu(const float *__restrict__ feat, const int32_t *__restrict__ nbr, int cap, int n_out,
                                  const float *__restrict__ dout, int cin, int cout, int rows_per_split,
                                  float *__restrict__ partial) {
  const int k = blockIdx.y;
  const int row_lo = blockIdx.z * rows_per_split, row_hi = min(row_lo + rows_per_split, n_out);
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= cin * cout) return;
  const int ci = e / cout, co = e - ci * cout;
  float acc = 0.0f;
  for (int o = row_lo; o < row_hi; ++o) {
    const int v = nbr[(size_t)k * cap + o];
    if (v >= 0) acc = __fmaf_rn(feat[(size_t)v * cin + ci], dout[(size_t)o * cout + co], acc);
  }
  partial[((size_t)blockIdx.z * gridDim.y + k) * cin * cout + e] = acc;
}

__global__ void k_wgrad_reduce(const float *__restrict__ partial, int nsplit, long long n, float *__restrict__ dW) {
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (long long)gridDim.x * blockDim.x) {
    float a = partial[t];
    for (int z = 1; z < nsplit; ++z) a = a + partial[(size_t)z * n + t];
    dW[t] = a;
  }
}

// ---- pointnet_lib gradients: inverse index (CSR per batch entry) + ordered gather
// Positions q of a batch entry (q = p*nsample + s, q = p, q = i*3 + k) reference points j = idx[q].  The inverse index lists,
// for every point, its positions in ascending order: list[start[j] .. start[j+1]).  It is a stable counting sort of the
// positions by point, built in four launches from idx alone (shared by all C channels):
//   k_pn_inv_rank      one wave walks kInvTile positions in order, 64 at a time, with a per-point cursor in LDS; lanes holding
//                      the same point find each other by one ballot per key bit; rank[q] = earlier positions of the tile with
//                      the same point; the cursor ends as the tile's per-point counts -> cnt[b][tile][j]
//   k_pn_inv_colscan   cnt[b][tile][j] -> exclusive prefix over the tiles; tot[b][j] = all positions of point j
//   k_pn_inv_rowscan   start[b][0..n] = exclusive prefix of tot over the points
//   k_pn_inv_place     list[start[j] + cnt[tile][j] + rank[q]] = q; bit 31 marks a point's last entry
// Indices outside [0, n) take no part in any of it (never an address).
constexpr int kInvTile = 8192;                 // positions per walking wave
constexpr int kInvKeyWin = 16384;              // points per LDS cursor window (64 KiB); larger clouds take several windows
constexpr int kInvKeyBits = 14;                // log2(kInvKeyWin)
constexpr int32_t kInvLast = (int32_t)0x80000000;

__global__ __launch_bounds__(64) void k_pn_inv_rank(const int32_t *__restrict__ idx, int nq, int n, int ntiles,
                                                    int32_t *__restrict__ rank, int32_t *__restrict__ cnt) {
  extern __shared__ int32_t inv_cur[];         // [kInvKeyWin]
  const int lane = threadIdx.x, tile = blockIdx.x, bs = blockIdx.y;
  const int q0 = tile * kInvTile, q1 = min(q0 + kInvTile, nq);
  const int32_t *I = idx + (size_t)bs * nq;
  int32_t *R = rank + (size_t)bs * nq;
  int32_t *Cn = cnt + ((size_t)bs * ntiles + tile) * n;
  const unsigned long long lt = (1ull << lane) - 1ull;
  for (int w0 = 0; w0 < n; w0 += kInvKeyWin) {
    const int wn = min(kInvKeyWin, n - w0);
    for (int k = lane; k < wn; k += 64) inv_cur[k] = 0;
    // one wave: its LDS accesses complete in order, no barrier between the clear, the walk and the read-out
    int jn = q0 + lane < q1 ? I[q0 + lane] : -1;
    for (int base = q0; base < q1; base += 64) {
      const int j = jn;
      jn = base + 64 + lane < q1 ? I[base + 64 + lane] : -1;            // next 64 in flight
      const int key = j - w0;
      const bool act = j >= w0 && key < wn;                             // j in this window (and in [0, n))
      unsigned long long peers = __ballot(act);
#pragma unroll
      for (int bit = 0; bit < kInvKeyBits; ++bit) {
        const bool on = (key >> bit) & 1;
        const unsigned long long m = __ballot(act && on);
        peers &= on ? m : ~m;
      }
      if (act) {
        const int before = __popcll(peers & lt);
        const int c0 = inv_cur[key];
        R[base + lane] = c0 + before;
        if (before == 0) inv_cur[key] = c0 + __popcll(peers);          // the lowest lane of the group advances the cursor
      }
    }
    for (int k = lane; k < wn; k += 64) Cn[w0 + k] = inv_cur[k];
  }
}

__global__ void k_pn_inv_colscan(int32_t *__restrict__ cnt, int ntiles, int n, int32_t *__restrict__ tot) {
  const int bs = blockIdx.y;
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
    int32_t *Cn = cnt + (size_t)bs * ntiles * n + j;
    int run = 0;
    for (int t = 0; t < ntiles; ++t) {
      const int v = Cn[(size_t)t * n];
      Cn[(size_t)t * n] = run;
      run += v;
    }
    tot[(size_t)bs * n + j] = run;
  }
}

__global__ __launch_bounds__(1024) void k_pn_inv_rowscan(const int32_t *__restrict__ tot, int n, int32_t *__restrict__ start) {
  __shared__ int32_t part[1024];
  const int bs = blockIdx.x, t = threadIdx.x;
  const int per = (n + 1023) / 1024;
  const int j0 = min(t * per, n), j1 = min(j0 + per, n);
  const int32_t *T = tot + (size_t)bs * n;
  int s = 0;
  for (int j = j0; j < j1; ++j) s += T[j];
  part[t] = s;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {
    const int v = t >= d ? part[t - d] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int run = part[t] - s;
  int32_t *S = start + (size_t)bs * (n + 1);
  for (int j = j0; j < j1; ++j) { S[j] = run; run += T[j]; }
  if (t == 1023) S[n] = part[1023];
}

template <bool W>
__global__ void k_pn_inv_place(const int32_t *__restrict__ idx, int nq, int n, int ntiles, const int32_t *__restrict__ rank,
                               const int32_t *__restrict__ cnt, const int32_t *__restrict__ start,
                               const float *__restrict__ weight, int32_t *__restrict__ list, float *__restrict__ wl) {
  const int bs = blockIdx.y;
  const int32_t *S = start + (size_t)bs * (n + 1);
  for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += gridDim.x * blockDim.x) {
    const int j = idx[(size_t)bs * nq + q];
    if ((unsigned)j >= (unsigned)n) continue;
    const int e = S[j] + cnt[((size_t)bs * ntiles + q / kInvTile) * n + j] + rank[(size_t)bs * nq + q];
    list[(size_t)bs * nq + e] = q | (e == S[j + 1] - 1 ? kInvLast : 0);
    if (W) wl[(size_t)bs * nq + e] = weight[(size_t)bs * nq + q];
  }
}

// Ordered gather: a workgroup owns PT*kGradThreads points (lane-consecutive) of one batch entry and CC channel rows; it streams
// the grad_out rows through LDS in chunks (double-buffered, register-staged 16-B loads) and every thread keeps its points'
// running sums in registers, adding the staged entries its lists name while they fall inside the chunk -- each point's
// contributions in ascending position order, one fp32 add at a time (INTERP: the product g*w rounded first).  grad_out row
// offsets are 64-bit; list entries are positions inside the batch entry (< 2^31).
constexpr int kGradThreads = 1024;

// CHF: floats per LDS buffer (CC rows of CHF/CC positions); 16 (or 8) floats per thread in flight
template <int CC, int PT, int CHF, bool INTERP>
__global__ __launch_bounds__(kGradThreads) void k_pn_grad_gather(int c, int n, int rowlen, int nq,
                                                                 const float *__restrict__ grad_out,
                                                                 const int32_t *__restrict__ start,
                                                                 const int32_t *__restrict__ list,
                                                                 const float *__restrict__ wl, float *__restrict__ grad_points) {
  extern __shared__ __attribute__((aligned(16))) float gg_lds[];   // [2][CC][chunk]
  constexpr int chunk = CHF / CC;
  constexpr int kV = CHF / 4 / kGradThreads;                       // float4 per thread per chunk
  const int bs = blockIdx.z, c0 = blockIdx.y * CC, ncc = min(CC, c - c0);
  const int t = threadIdx.x;
  const int32_t *S = start + (size_t)bs * (n + 1);
  const int32_t *L = list + (size_t)bs * nq;
  const float *WL = INTERP ? wl + (size_t)bs * nq : nullptr;
  const float *G = grad_out + ((size_t)bs * c + c0) * rowlen;
  float *GP = grad_points + ((size_t)bs * c + c0) * n;
  float acc[PT][CC];
  int ptr[PT], cur[PT];                        // cur: the list entry at ptr (bit 31 = last of the point), INT_MAX = done
  float wv[PT];
#pragma unroll
  for (int p = 0; p < PT; ++p) {
    const int j = (blockIdx.x * PT + p) * kGradThreads + t;
    const bool live = j < n;
    const int s0 = live ? S[j] : 0, s1 = live ? S[j + 1] : 0;
    ptr[p] = s0;
    cur[p] = s0 < s1 ? L[s0] : INT_MAX;
    wv[p] = INTERP && s0 < s1 ? WL[s0] : 0.0f;
#pragma unroll
    for (int cc = 0; cc < CC; ++cc) acc[p][cc] = live && cc < ncc ? GP[(size_t)cc * n + j] : 0.0f;
  }
  const bool vec = (rowlen & 3) == 0 && (reinterpret_cast<uintptr_t>(grad_out) & 15) == 0;
  float4 pre[kV];
  auto load = [&](int r0) {
#pragma unroll
    for (int v = 0; v < kV; ++v) {
      const int e = 4 * (v * kGradThreads + t), cc = e / chunk, r = r0 + e - cc * chunk;
      const float *src = G + (size_t)cc * rowlen + r;
      float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
      if (cc < ncc) {
        if (vec && r + 4 <= rowlen) {
          x = *reinterpret_cast<const float4 *>(src);
        } else {
          if (r < rowlen) x.x = src[0];
          if (r + 1 < rowlen) x.y = src[1];
          if (r + 2 < rowlen) x.z = src[2];
          if (r + 3 < rowlen) x.w = src[3];
        }
      }
      pre[v] = x;
    }
  };
  auto stash = [&](int buf) {
#pragma unroll
    for (int v = 0; v < kV; ++v) reinterpret_cast<float4 *>(gg_lds + buf * CHF)[v * kGradThreads + t] = pre[v];
  };
  load(0);
  stash(0);
  __syncthreads();
  const int nchunks = (rowlen + chunk - 1) / chunk;
  for (int k = 0; k < nchunks; ++k) {
    const int r0 = k * chunk;
    if (k + 1 < nchunks) load(r0 + chunk);                         // next chunk in flight while this one is consumed
    const float *B = gg_lds + (k & 1) * CHF;
    const int qend = INTERP ? 3 * min(r0 + chunk, rowlen) : min(r0 + chunk, rowlen);
    for (;;) {
      bool more = false;
#pragma unroll
      for (int p = 0; p < PT; ++p) {
        const int q = cur[p] & 0x7fffffff;
        if (q < qend) {
          const int li = (INTERP ? q / 3 : q) - r0;
#pragma unroll
          for (int cc = 0; cc < CC; ++cc) {
            const float g = B[cc * chunk + li];
            acc[p][cc] = __fadd_rn(acc[p][cc], INTERP ? __fmul_rn(g, wv[p]) : g);
          }
          if (cur[p] < 0) {
            cur[p] = INT_MAX;
          } else {
            ++ptr[p];
            cur[p] = L[ptr[p]];
            if (INTERP) wv[p] = WL[ptr[p]];
          }
        }
      }
#pragma unroll
      for (int p = 0; p < PT; ++p) more |= (cur[p] & 0x7fffffff) < qend;
      if (__ballot(more) == 0ull) break;
    }
    if (k + 1 < nchunks) stash((k + 1) & 1);
    __syncthreads();
  }
#pragma unroll
  for (int p = 0; p < PT; ++p) {
    const int j = (blockIdx.x * PT + p) * kGradThreads + t;
    if (j < n)
#pragma unroll
      for (int cc = 0; cc < CC; ++cc)
        if (cc < ncc) GP[(size_t)cc * n + j] = acc[p][cc];
  }
}

}  // namespace

DCL_API int dcl_rulebook_transpose(const int32_t *nbr, int cap_out, const int32_t *n_out_dev, int n_out_host, int kvol,
                                   int32_t *inv, int cap_in, dclStream_t stream) {
  DCL_CHECK_ARG(nbr && inv && cap_out > 0 && cap_in > 0 && kvol > 0 && kvol <= 27 && (n_out_dev || n_out_host >= 0));
  hipStream_t s = (hipStream_t)stream;
  const long long ni = (long long)kvol * cap_in;
  hipLaunchKernelGGL(k_fill_i32, dim3(dcl_grid_1d(ni, 256)), dim3(256), 0, s, inv, ni, -1);
  const int rows = n_out_dev ? cap_out : n_out_host;
  if (rows > 0)
    hipLaunchKernelGGL(k_rulebook_transpose, dim3(dcl_grid_1d((long long)rows * kvol, 256)), dim3(256), 0, s, nbr, cap_out,
                       n_out_dev, n_out_host, kvol, inv, cap_in);
  DCL_LAUNCH_CHECK();
  return 0;
}

DCL_API int dcl_sparse_avgpool_bwd(const float *dout, const int32_t *inv, int cap_in, int n_in, const int32_t *rf, int c,
                                   int kvol, float *din, dclStream_t stream) {
  DCL_CHECK_ARG(n_in >= 0 && c > 0 && c % 4 == 0 && kvol > 0 && kvol <= 27 && cap_in >= n_in);
  if (n_in == 0) return 0;
  DCL_CHECK_ARG(dout && inv && rf && din);
  hipLaunchKernelGGL(k_sparse_avgpool_bwd, dim3(dcl_grid_1d((long long)n_in * (c / 4), 256)), dim3(256), 0,
                     (hipStream_t)stream, dout, inv, cap_in, n_in, rf, c, kvol, din);
  DCL_LAUNCH_CHECK();
  return 0;
}

DCL_API int dcl_three_interpolate_grad_sp(int c, int n, int m, const float *grad_out, const int32_t *idx, const float *weight,
                                          float *grad_points_zeroed, dclStream_t stream) {
  DCL_CHECK_ARG(c >= 0 && n >= 0 && m >= 0);
  if (c == 0 || n == 0) return 0;
  DCL_CHECK_ARG(grad_out && idx && weight && grad_points_zeroed && m > 0);
  hipLaunchKernelGGL(k_three_interp_grad_sp, dim3(dcl_grid_1d((long long)n * c, 256)), dim3(256), 0, (hipStream_t)stream, c,
                     n, grad_out, idx, weight, grad_points_zeroed);
  DCL_LAUNCH_CHECK();
  return 0;
}

DCL_API int dcl_voxelize_bp(const float *d_out, const int32_t *rules, float *d_feats_zeroed, int n_rows, int max_active, int c,
                            int average, dclStream_t stream) {
  DCL_CHECK_ARG(n_rows >= 0 && max_active >= 0 && c > 0);
  if (n_rows == 0) return 0;
  DCL_CHECK_ARG(d_out && rules && d_feats_zeroed);
  hipLaunchKernelGGL(k_voxelize_bp, dim3(dcl_grid_1d((long long)n_rows * c, 256)), dim3(256), 0, (hipStream_t)stream, n_rows,
                     max_active, c, d_out, rules, average, d_feats_zeroed);
  DCL_LAUNCH_CHECK();
  return 0;
}

DCL_API int dcl_sparse_conv_wgrad_splits(int n_out, int32_t *splits_host) {
  DCL_CHECK_ARG(n_out >= 0 && splits_host);
  int s = dcl_div_up(n_out > 0 ? n_out : 1, 2048);
  *splits_host = s > 64 ? 64 : s;
  return 0;
}

DCL_API int dcl_sparse_conv_wgrad(const float *feat, const int32_t *nbr, int cap, int n_out, const float *dout, int cin,
                                  int cout, int kvol, float *partial /* splits*kvol*cin*cout */, float *dW,
                                  dclStream_t stream) {
  DCL_CHECK_ARG(n_out >= 0 && cap >= n_out && cin > 0 && cout > 0 && kvol > 0 && kvol <= 27 && dW && partial);
  DCL_CHECK_ARG(n_out == 0 || (feat && nbr && dout));
  hipStream_t s = (hipStream_t)stream;
  int splits;
  (void)dcl_sparse_conv_wgrad_splits(n_out, &splits);
  const int rps = dcl_div_up(dcl_div_up(n_out > 0 ? n_out : 1, splits), 8) * 8;
  const long long n = (long long)kvol * cin * cout;
  if (cin % 64 == 0 && cout % 64 == 0)
    hipLaunchKernelGGL((k_conv_wgrad_mfma<2, 2>), dim3((cin / 64) * (cout / 64), kvol, splits), dim3(64), 0, s, feat, nbr, cap,
                       n_out, dout, cin, cout, rps, partial);
  else if (cin % 32 == 0 && cout % 32 == 0)
    hipLaunchKernelGGL((k_conv_wgrad_mfma<1, 1>), dim3((cin / 32) * (cout / 32), kvol, splits), dim3(64), 0, s, feat, nbr, cap,
                       n_out, dout, cin, cout, rps, partial);
  else
    hipLaunchKernelGGL(k_conv_wgrad_valu, dim3(dcl_div_up(cin * cout, 256), kvol, splits), dim3(256), 0, s, feat, nbr, cap,
                       n_out, dout, cin, cout, rps, partial);
  hipLaunchKernelGGL(k_wgrad_reduce, dim3(dcl_grid_1d(n, 256)), dim3(256), 0, s, partial, splits, n, dW);
  DCL_LAUNCH_CHECK();
  return 0;
}

// ---- pointnet_lib gradients (group_points_grad / gather_points_grad / three_interpolate_grad)
namespace {

struct PnInvWs {
  int32_t *cnt, *tot, *start, *rank, *list;
  float *wl;
};

// workspace of the inverse index of b batch entries x nq positions over n points (with_w: the weights in list order too);
// ws == nullptr: size only
long long pn_inv_ws(int b, int n, int nq, bool with_w, void *ws, PnInvWs *out) {
  const long long ntiles = (nq + kInvTile - 1) / kInvTile;
  const long long sz[6] = {(long long)b * ntiles * n, (long long)b * n, (long long)b * (n + 1), (long long)b * nq,
                           (long long)b * nq, with_w ? (long long)b * nq : 0};
  long long off[6], total = 0;
  for (int i = 0; i < 6; ++i) {
    off[i] = total;
    total += (sz[i] * 4 + 255) & ~255ll;
  }
  if (ws && out) {
    char *p = static_cast<char *>(ws);
    out->cnt = reinterpret_cast<int32_t *>(p + off[0]);
    out->tot = reinterpret_cast<int32_t *>(p + off[1]);
    out->start = reinterpret_cast<int32_t *>(p + off[2]);
    out->rank = reinterpret_cast<int32_t *>(p + off[3]);
    out->list = reinterpret_cast<int32_t *>(p + off[4]);
    out->wl = with_w ? reinterpret_cast<float *>(p + off[5]) : nullptr;
  }
  return total;
}

// shapes every entry point accepts: positions per batch entry < 2^31, grid dimensions inside HIP's limits
bool pn_grad_shape_ok(int b, int c, int n, long long nq) {
  return b >= 0 && c >= 0 && n >= 0 && nq >= 0 && nq < (1ll << 31) - kInvTile && n < (1 << 30) && b <= 65535 &&
         c <= 65535;
}

template <bool INTERP>
int pn_grad_launch(int b, int c, int n, int rowlen, int nq, const float *grad_out, const int32_t *idx, const float *weight,
                   float *grad_points, void *ws, int64_t ws_bytes, hipStream_t s) {
  PnInvWs w;
  if (ws_bytes < pn_inv_ws(b, n, nq, INTERP, ws, &w)) {
    dcl_set_error("pointnet grad: invalid argument: ws_bytes %lld < %lld", (long long)ws_bytes,
                  pn_inv_ws(b, n, nq, INTERP, nullptr, nullptr));
    return DCL_EINVAL;
  }
  const int ntiles = dcl_div_up(nq, kInvTile);
  const size_t lds_inv = (size_t)min(n, kInvKeyWin) * 4;
  if (lds_inv > 48 * 1024)
    (void)hipFuncSetAttribute((const void *)k_pn_inv_rank, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_inv);
  hipLaunchKernelGGL(k_pn_inv_rank, dim3(ntiles, b), dim3(64), lds_inv, s, idx, nq, n, ntiles, w.rank, w.cnt);
  hipLaunchKernelGGL(k_pn_inv_colscan, dim3(dcl_div_up(n, 256), b), dim3(256), 0, s, w.cnt, ntiles, n, w.tot);
  hipLaunchKernelGGL(k_pn_inv_rowscan, dim3(b), dim3(1024), 0, s, w.tot, n, w.start);
  hipLaunchKernelGGL((k_pn_inv_place<INTERP>), dim3(dcl_grid_1d(nq, 256, 1024), b), dim3(256), 0, s, idx, nq, n, ntiles,
                     w.rank, w.cnt, w.start, weight, w.list, w.wl);
  // points per thread: the fewest that cover the cloud in one workgroup (up to 12); CC channel rows per workgroup; the
  // 12-point form takes 2 rows and stages half the chunk so that its sums, list cursors and staging fit 128 VGPRs
  const int pt = n <= kGradThreads ? 1 : n <= 2 * kGradThreads ? 2 : n <= 4 * kGradThreads ? 4 : n <= 8 * kGradThreads ? 8 : 12;
  const int cc = pt == 12 ? 2 : pt == 8 ? 4 : 8;
  const int xb = dcl_div_up(n, (long long)pt * kGradThreads);
  const dim3 grid(xb, dcl_div_up(c, cc), b);
#define PNG(CC, PT, CHF)                                                                                                \
  do {                                                                                                                  \
    const size_t lds = 2 * (CHF) * 4;                                                                                   \
    (void)hipFuncSetAttribute((const void *)k_pn_grad_gather<CC, PT, CHF, INTERP>,                                     \
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);                                    \
    hipLaunchKernelGGL((k_pn_grad_gather<CC, PT, CHF, INTERP>), grid, dim3(kGradThreads), lds, s, c, n, rowlen, nq,      \
                       grad_out, w.start, w.list, w.wl, grad_points);                                                   \
  } while (0)
  if (pt == 1) PNG(8, 1, 16384); else if (pt == 2) PNG(8, 2, 16384); else if (pt == 4) PNG(8, 4, 16384);
  else if (pt == 8) PNG(4, 8, 16384); else PNG(2, 12, 8192);
#undef PNG
  DCL_LAUNCH_CHECK();
  return 0;
}

}  // namespace

DCL_API int dcl_group_points_grad_ws_bytes(int b, int c, int n, int npoints, int nsample, int64_t *bytes_host) {
  DCL_CHECK_ARG(npoints >= 0 && nsample >= 0 && pn_grad_shape_ok(b, c, n, (long long)npoints * nsample) && bytes_host);
  *bytes_host = pn_inv_ws(b, n, npoints * nsample, false, nullptr, nullptr);
  return 0;
}

DCL_API int dcl_group_points_grad(int b, int c, int n, int npoints, int nsample, const float *grad_out, const int32_t *idx,
                                  float *grad_points, void *ws, int64_t ws_bytes, dclStream_t stream) {
  DCL_CHECK_ARG(npoints >= 0 && nsample >= 0 && pn_grad_shape_ok(b, c, n, (long long)npoints * nsample));
  const int nq = npoints * nsample;
  if (b == 0 || c == 0 || n == 0 || nq == 0) return 0;
  DCL_CHECK_ARG(grad_out && idx && grad_points && ws);
  return pn_grad_launch<false>(b, c, n, nq, nq, grad_out, idx, nullptr, grad_points, ws, ws_bytes, (hipStream_t)stream);
}

DCL_API int dcl_gather_points_grad_ws_bytes(int b, int c, int n, int npoints, int64_t *bytes_host) {
  return dcl_group_points_grad_ws_bytes(b, c, n, npoints, 1, bytes_host);
}

DCL_API int dcl_gather_points_grad(int b, int c, int n, int npoints, const float *grad_out, const int32_t *idx,
                                   float *grad_points, void *ws, int64_t ws_bytes, dclStream_t stream) {
  // gather_points_grad is group_points_grad with nsample == 1 (sampling_gpu.cu:46-63 vs group_points_gpu.cu:8-25)
  return dcl_group_points_grad(b, c, n, npoints, 1, grad_out, idx, grad_points, ws, ws_bytes, stream);
}

DCL_API int dcl_three_interpolate_grad_ws_bytes(int b, int c, int n, int m, int64_t *bytes_host) {
  DCL_CHECK_ARG(m >= 0 && pn_grad_shape_ok(b, c, m, 3ll * (n < 0 ? -1 : n)) && bytes_host);
  *bytes_host = pn_inv_ws(b, m, 3 * n, true, nullptr, nullptr);
  return 0;
}

DCL_API int dcl_three_interpolate_grad(int b, int c, int n, int m, const float *grad_out, const int32_t *idx,
                                       const float *weight, float *grad_points, void *ws, int64_t ws_bytes,
                                       dclStream_t stream) {
  DCL_CHECK_ARG(m >= 0 && pn_grad_shape_ok(b, c, m, 3ll * (n < 0 ? -1 : n)));
  if (b == 0 || c == 0 || n == 0 || m == 0) return 0;
  DCL_CHECK_ARG(grad_out && idx && weight && grad_points && ws);
  return pn_grad_launch<true>(b, c, m, n, 3 * n, grad_out, idx, weight, grad_points, ws, ws_bytes, (hipStream_t)stream);
}
