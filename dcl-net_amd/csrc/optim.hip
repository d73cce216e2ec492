// optim.hip -- what follows loss.backward() in a training step: the global gradient norm (AutoClip's measurement) and the
// Adam update with the clip factor folded in, each over ALL parameter tensors in one launch.
//
// The reference (tools/train_YCBV_stage1.py:119-125, 212-231) takes one norm kernel and one blocking read-back per parameter
// tensor (156 in Network), computes every norm a second time in clip_grad_norm_, multiplies every gradient and then runs
// torch.optim.Adam.  Here two device tables drive everything (include/dclnet_hip.h at dclOptimTensor): a tensor table with
// the four addresses, the length and the two bias corrections of every tensor that has a gradient, and a chunk table that
// cuts the tensors into runs of DCL_OPTIM_CHUNK elements.  One 256-thread workgroup takes one chunk.
//
// Both passes are bound by memory (4 B per element the norm, 28 B the update), so a lane's whole share of a chunk -- four
// 16-byte vectors per array, 16 loads in the update -- is issued before the first use: 64 KiB in flight per workgroup.
// A chunk that is not full, or whose addresses are not 16-byte aligned (tails, tiny tensors, a parameter that is a view at an
// odd element offset), moves scalars under the same element-to-lane map, so the norm's summation order is one and the same.
//
// dcl_grad_sqnorm: launch 1 writes one float64 partial per chunk (exact products, fixed lane order, fixed tree), launch 2
// (one workgroup) adds a tensor's partials in chunk order, the tensors in table order, and takes the root.  No atomics.
// dcl_adam_step: the five documented fp32 lines per element, in that order (the library is built with -ffp-contract=off).
// dcl_adam_step_dev: the same body with the clip factor read from device memory.
// dcl_autoclip_observe: AutoClip's percentile over a history kept sorted on the device -- launch 1 inserts this step's norm
// (one lane per held entry, ping-pong buffers), launch 2 (one lane) evaluates np.percentile and the factor (optim_clip.h).
#include "common.h"
#include "optim_clip.h"
#include <math.h>

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = DCL_OPTIM_CHUNK;
constexpr int kVecs = kChunk / (4 * kThreads);            // 16-byte vectors per lane and array
static_assert(kVecs * 4 * kThreads == kChunk, "a chunk is a whole number of 16-byte vectors per lane");

// elements of chunk c's tensor from its begin on, at most kChunk (<= 0: a table that breaks the contract; nothing is touched)
__device__ __forceinline__ int chunk_count(const dclOptimTensor &T, int64_t begin) {
  const int64_t left = T.numel - begin;
  return left < (int64_t)kChunk ? (int)left : kChunk;
}
__device__ __forceinline__ bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
// A pointer read from the tensor table is a generic one to the compiler, and its accesses become flat_load / flat_store,
// which also count on lgkmcnt.  The arrays are global memory by contract: say so.
typedef float vec4_t __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) vec4_t global_vec4_t;
__device__ __forceinline__ float4 load4(const float *base, int at) {
  const vec4_t x = ((const global_vec4_t *)base)[at];
  return make_float4(x.x, x.y, x.z, x.w);
}
__device__ __forceinline__ void store4(float *base, int at, const float4 &x) {
  ((global_vec4_t *)base)[at] = vec4_t{x.x, x.y, x.z, x.w};
}

__global__ __launch_bounds__(kThreads) void k_grad_sqnorm_chunks(const dclOptimTensor *__restrict__ table,
                                                                 const int32_t *__restrict__ chunk_tensor,
                                                                 const int64_t *__restrict__ chunk_begin,
                                                                 double *__restrict__ partials) {
  __shared__ double wave_sum[kThreads / 64];
  const int c = blockIdx.x, tid = threadIdx.x;
  const dclOptimTensor T = table[chunk_tensor[c]];
  const int64_t begin = chunk_begin[c];
  const int count = chunk_count(T, begin);
  const float *g = T.grad + begin;
  double s = 0.0;
  if (count == kChunk && aligned16(g)) {
    float4 G[kVecs];
#pragma unroll
    for (int k = 0; k < kVecs; ++k) G[k] = load4(g, k * kThreads + tid);
    __builtin_amdgcn_sched_barrier(0);                   // every load is issued before the first product
#pragma unroll
    for (int k = 0; k < kVecs; ++k) {
      s += (double)G[k].x * (double)G[k].x;
      s += (double)G[k].y * (double)G[k].y;
      s += (double)G[k].z * (double)G[k].z;
      s += (double)G[k].w * (double)G[k].w;
    }
  } else {
#pragma unroll
    for (int k = 0; k < kVecs; ++k)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int e = (k * kThreads + tid) * 4 + j;
        if (e < count) s += (double)g[e] * (double)g[e];
      }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
  if ((tid & 63) == 0) wave_sum[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) partials[c] = (wave_sum[0] + wave_sum[1]) + (wave_sum[2] + wave_sum[3]);
}

// sum of x[0 .. n) in ascending order; the loads of 16 terms are issued together, the additions stay in order
__device__ __forceinline__ double ordered_sum(const double *x, int n) {
  double s = 0.0;
  int i = 0;
  for (; i + 16 <= n; i += 16) {
    double v[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = x[i + j];
#pragma unroll
    for (int j = 0; j < 16; ++j) s += v[j];
  }
  for (; i < n; ++i) s += x[i];
  return s;
}

// The ordered sums are chains of dependent additions whose terms other workgroups have just written: read one by one from
// memory a chain pays a memory latency per 16 terms (216 terms the longest of Network's, 156 the final one: ~30 us measured).
// So the workgroup first copies the partials into LDS with all its lanes, and keeps the tensors' sums there for the final
// chain; a table too large for that is summed from memory in the same order (same bits, slower).
constexpr int kStageChunks = 6144;                        // 48 KiB of partials: 25 M elements
constexpr int kStageTensors = 1024;                       // 8 KiB of per-tensor sums

__global__ __launch_bounds__(kThreads) void k_grad_sqnorm_finish(int n_tensors, const dclOptimTensor *__restrict__ table,
                                                                 int n_chunks, const int32_t *__restrict__ chunk_tensor,
                                                                 const int64_t *__restrict__ chunk_begin,
                                                                 const double *partials, double *sq_per_tensor,
                                                                 double *__restrict__ norm) {
  __shared__ double part_lds[kStageChunks];
  __shared__ double sq_lds[kStageTensors];
  const bool stage_chunks = n_chunks <= kStageChunks, stage_tensors = n_tensors <= kStageTensors;
  if (stage_chunks) {
    for (int c = threadIdx.x; c < n_chunks; c += kThreads) part_lds[c] = partials[c];
    __syncthreads();
  }
  const double *part = stage_chunks ? part_lds : partials;
  // the lane that meets a tensor's first chunk adds all of that tensor's partials (they follow it in the chunk table)
  for (int c = threadIdx.x; c < n_chunks; c += kThreads) {
    if (chunk_begin[c] != 0) continue;
    const int t = chunk_tensor[c];
    if ((unsigned)t >= (unsigned)n_tensors) continue;
    const int64_t want = (table[t].numel + kChunk - 1) / kChunk;
    const int n = want < (int64_t)(n_chunks - c) ? (int)want : n_chunks - c;
    const double s = ordered_sum(part + c, n);
    sq_per_tensor[t] = s;
    if (stage_tensors) sq_lds[t] = s;
  }
  __syncthreads();                                       // the sums above are visible to the whole workgroup
  if (threadIdx.x == 0) norm[0] = sqrt(ordered_sum(stage_tensors ? sq_lds : sq_per_tensor, n_tensors));
}

struct AdamConst {
  float grad_scale, beta1, omb1, beta2, omb2, eps;
};

// the contract of include/dclnet_hip.h at dcl_adam_step, line by line
__device__ __forceinline__ void adam_element(float &p, float g, float &m, float &v, float step_size, float bc2_sqrt,
                                             const AdamConst &k) {
  const float gs = g * k.grad_scale;
  m = m * k.beta1 + gs * k.omb1;
  v = v * k.beta2 + (gs * gs) * k.omb2;
  const float d = sqrtf(v) / bc2_sqrt + k.eps;
  p = p - step_size * (m / d);
}

// one chunk's update; kDevScale: the clip factor is read from device memory here instead of arriving in k
template <bool kDevScale>
__device__ __forceinline__ void adam_chunk(const dclOptimTensor *__restrict__ table, const int32_t *__restrict__ chunk_tensor,
                                           const int64_t *__restrict__ chunk_begin, AdamConst k,
                                           const float *__restrict__ grad_scale_dev) {
  if (kDevScale) k.grad_scale = grad_scale_dev[0];
  const int c = blockIdx.x, tid = threadIdx.x;
  const dclOptimTensor T = table[chunk_tensor[c]];
  const int64_t begin = chunk_begin[c];
  const int count = chunk_count(T, begin);
  float *p = T.param + begin, *m = T.exp_avg + begin, *v = T.exp_avg_sq + begin;
  const float *g = T.grad + begin;
  if (count == kChunk && aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v)) {
    float4 P[kVecs], G[kVecs], M[kVecs], V[kVecs];
#pragma unroll
    for (int i = 0; i < kVecs; ++i) {
      const int at = i * kThreads + tid;
      G[i] = load4(g, at);
      M[i] = load4(m, at);
      V[i] = load4(v, at);
      P[i] = load4(p, at);
    }
    __builtin_amdgcn_sched_barrier(0);                   // all 16 loads are issued before the first use: 64 KiB in flight
#pragma unroll
    for (int i = 0; i < kVecs; ++i) {
      adam_element(P[i].x, G[i].x, M[i].x, V[i].x, T.step_size, T.bc2_sqrt, k);
      adam_element(P[i].y, G[i].y, M[i].y, V[i].y, T.step_size, T.bc2_sqrt, k);
      adam_element(P[i].z, G[i].z, M[i].z, V[i].z, T.step_size, T.bc2_sqrt, k);
      adam_element(P[i].w, G[i].w, M[i].w, V[i].w, T.step_size, T.bc2_sqrt, k);
      const int at = i * kThreads + tid;
      store4(m, at, M[i]);
      store4(v, at, V[i]);
      store4(p, at, P[i]);
    }
  } else {
    for (int e = tid; e < count; e += kThreads) {
      float pe = p[e], me = m[e], ve = v[e];
      adam_element(pe, g[e], me, ve, T.step_size, T.bc2_sqrt, k);
      m[e] = me;
      v[e] = ve;
      p[e] = pe;
    }
  }
}

__global__ __launch_bounds__(kThreads) void k_adam_step(const dclOptimTensor *__restrict__ table,
                                                        const int32_t *__restrict__ chunk_tensor,
                                                        const int64_t *__restrict__ chunk_begin, AdamConst k) {
  adam_chunk<false>(table, chunk_tensor, chunk_begin, k, nullptr);
}

__global__ __launch_bounds__(kThreads) void k_adam_step_dev(const dclOptimTensor *__restrict__ table,
                                                            const int32_t *__restrict__ chunk_tensor,
                                                            const int64_t *__restrict__ chunk_begin, AdamConst k,
                                                            const float *__restrict__ grad_scale_dev) {
  adam_chunk<true>(table, chunk_tensor, chunk_begin, k, grad_scale_dev);
}

// AutoClip's insertion: one lane per held entry (optim_clip.h: dcl_clip_insert_lane); lane 0 exists for n == 0 as well
__global__ __launch_bounds__(kThreads) void k_autoclip_insert(int64_t n, const double *__restrict__ src, double *__restrict__ dst,
                                                              double *__restrict__ arrival, const double *__restrict__ norm) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n && i != 0) return;
  dcl_clip_insert_lane(n, src, dst, arrival, norm[0], i);
}

__global__ __launch_bounds__(64) void k_autoclip_finish(int64_t n, const double *__restrict__ sorted, const double *__restrict__ norm,
                                                        double percentile, double *__restrict__ out) {
  if (blockIdx.x == 0 && threadIdx.x == 0) dcl_clip_finish(n, sorted, norm[0], percentile, out);
}

}  // namespace

DCL_API int dcl_grad_sqnorm(int n_tensors, const dclOptimTensor *table, int n_chunks, const int32_t *chunk_tensor,
                            const int64_t *chunk_begin, double *partials, double *sq_per_tensor, double *norm,
                            dclStream_t stream) {
  DCL_CHECK_ARG(n_tensors >= 0 && n_chunks >= 0);
  if (n_tensors == 0) return 0;
  DCL_CHECK_ARG(n_chunks >= n_tensors);
  DCL_CHECK_ARG(table && chunk_tensor && chunk_begin && partials && sq_per_tensor && norm);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_grad_sqnorm_chunks, dim3(n_chunks), dim3(kThreads), 0, s, table, chunk_tensor, chunk_begin, partials);
  DCL_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_grad_sqnorm_finish, dim3(1), dim3(kThreads), 0, s, n_tensors, table, n_chunks, chunk_tensor,
                     chunk_begin, partials, sq_per_tensor, norm);
  DCL_LAUNCH_CHECK();
  return 0;
}

static AdamConst adam_const(float grad_scale, float beta1, float beta2, float eps) {
  AdamConst k;
  k.grad_scale = grad_scale;
  k.beta1 = beta1;
  k.omb1 = (float)(1.0 - (double)beta1);
  k.beta2 = beta2;
  k.omb2 = (float)(1.0 - (double)beta2);
  k.eps = eps;
  return k;
}

DCL_API int dcl_adam_step(int n_tensors, const dclOptimTensor *table, int n_chunks, const int32_t *chunk_tensor,
                          const int64_t *chunk_begin, float grad_scale, float beta1, float beta2, float eps,
                          dclStream_t stream) {
  DCL_CHECK_ARG(n_tensors >= 0 && n_chunks >= 0);
  DCL_CHECK_ARG(isfinite(grad_scale));
  DCL_CHECK_ARG(beta1 >= 0.0f && beta1 < 1.0f && beta2 >= 0.0f && beta2 < 1.0f);
  DCL_CHECK_ARG(eps > 0.0f);
  if (n_tensors == 0) return 0;
  DCL_CHECK_ARG(n_chunks >= n_tensors);
  DCL_CHECK_ARG(table && chunk_tensor && chunk_begin);
  const AdamConst k = adam_const(grad_scale, beta1, beta2, eps);
  hipLaunchKernelGGL(k_adam_step, dim3(n_chunks), dim3(kThreads), 0, (hipStream_t)stream, table, chunk_tensor, chunk_begin, k);
  DCL_LAUNCH_CHECK();
  return 0;
}

DCL_API int dcl_adam_step_dev(int n_tensors, const dclOptimTensor *table, int n_chunks, const int32_t *chunk_tensor,
                              const int64_t *chunk_begin, const float *grad_scale_dev, float beta1, float beta2, float eps,
                              dclStream_t stream) {
  DCL_CHECK_ARG(n_tensors >= 0 && n_chunks >= 0);
  DCL_CHECK_ARG(beta1 >= 0.0f && beta1 < 1.0f && beta2 >= 0.0f && beta2 < 1.0f);
  DCL_CHECK_ARG(eps > 0.0f);
  if (n_tensors == 0) return 0;
  DCL_CHECK_ARG(n_chunks >= n_tensors);
  DCL_CHECK_ARG(table && chunk_tensor && chunk_begin && grad_scale_dev);
  DCL_CHECK_ARG((reinterpret_cast<uintptr_t>(grad_scale_dev) & 3) == 0);
  const AdamConst k = adam_const(1.0f, beta1, beta2, eps);            // grad_scale: the kernel reads it
  hipLaunchKernelGGL(k_adam_step_dev, dim3(n_chunks), dim3(kThreads), 0, (hipStream_t)stream, table, chunk_tensor, chunk_begin,
                     k, grad_scale_dev);
  DCL_LAUNCH_CHECK();
  return 0;
}

DCL_API int dcl_autoclip_observe(int64_t n, const double *sorted_src, double *sorted_dst, double *arrival, const double *norm,
                                 double percentile, void *out, dclStream_t stream) {
  DCL_AUTOCLIP_CHECK_ARGS();
  hipStream_t s = (hipStream_t)stream;
  const int64_t lanes = n > 0 ? n : 1;
  hipLaunchKernelGGL(k_autoclip_insert, dim3((unsigned)((lanes + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, n, sorted_src,
                     sorted_dst, arrival, norm);
  DCL_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_autoclip_finish, dim3(1), dim3(64), 0, s, n, (const double *)sorted_dst, norm, percentile, (double *)out);
  DCL_LAUNCH_CHECK();
  return 0;
}
