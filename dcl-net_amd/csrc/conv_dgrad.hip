// conv_dgrad.hip -- the sparse convolution's input gradient on a kernel of its own (ops.sparse_conv_backward(dgrad="direct")),
// beside the route that re-enters the forward dispatcher with the transposed rulebook and a transposed copy of W ("conv", the
// default, untouched).
//
//   dX[i][ci] = sum_k sum_co dout[inv[k][i]][co] * W[k][ci][co]        inv: kvol x cap_in, from dcl_rulebook_transpose
//
// W is read AS REGISTERED (kvol x cin x cout): an element's reduction runs along W's contiguous axis, so a row of W[k] and a
// gathered row of dout are both the "k-major" operand of v_mfma_f32_32x32x2_f32 -- lane l holds A[row l & 31][step half l >> 5]
// and B[step half l >> 5][column l & 31] -- and no transposed copy is needed.  The summation order is conv_dgrad.h's: one
// accumulator per element, offsets ascending, channels ascending, nothing split.
//
// k_conv_dgrad: a workgroup of four waves owns BM input rows x BN input channels (WP x WQ waves of one 32 x 32 accumulator).
//   1. it reads its rows' 27 entries of inv once, keeps the neighbours (or -1) in LDS and ORs a bit per offset that any of its
//      rows has (one ballot per 64 entries): offsets none of its rows has are skipped altogether;
//   2. it walks the (offset, 32-channel chunk) segments that are left, ascending: global -> registers -> LDS, two LDS
//      buffers -- the next segment's dout rows and its BN x 32 piece of W[k] fly under this segment's 16 MFMA steps.  A whole
//      256 x 128 W[k] is 128 KiB, so the reduction channels are chunked;
//   3. LDS rows hold a chunk DE-INTERLEAVED (conv_slab.h, shared with conv_fwd_compact.hip): a lane's 16 values of a chunk are
//      four ds_read_b128 instead of sixteen ds_read_b32.
// Rows past n_in, columns past cin, channels past cout and rows without the offset are zero lanes of the same body: any cin,
// cout >= 1, no VALU fallback; 16-byte loads are only the fast path of aligned rows.  No atomics on floats, no counters, no
// scratch.
#include <vector>

#include "common.h"
#include "mfma_tile.h"
#include "conv_slab.h"
#include "conv_dgrad.h"

namespace {

template <int WP, int WQ, bool VEC>
__global__ __launch_bounds__(kDgThreads) void k_conv_dgrad(const float *__restrict__ dout, int n_out,
                                                           const int32_t *__restrict__ inv, int cap_in, int n_in,
                                                           const float *__restrict__ W, int cin, int cout, int kvol,
                                                           float *__restrict__ dx) {
  static_assert(WP * WQ * 64 == kDgThreads, "four waves");
  constexpr int BM = 32 * WP, BN = 32 * WQ;
  static_assert(BM % 64 == 0, "the 64 entries of a wave's ballot belong to one offset");
  __shared__ __attribute__((aligned(16))) float As[2][BM * kDgPitch];
  __shared__ __attribute__((aligned(16))) float Bs[2][BN * kDgPitch];
  __shared__ int s_idx[kDgradMaxKvol * BM];                  // [k][row of the tile]: the neighbour's dout row, or -1
  __shared__ unsigned s_mask;                                // bit k: a row of the tile has offset k
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5;
  const int wp = wave / WQ, wq = wave - wp * WQ;
  const long long row0 = (long long)blockIdx.x * BM;
  const int q0 = blockIdx.y * BN;

  if (t == 0) s_mask = 0u;
  __syncthreads();
  for (int e = t; e < kvol * BM; e += kDgThreads) {          // (kvol * BM % 64 == 0: the trip count is wave-uniform)
    const int k = e / BM, rr = e - k * BM;
    const long long row = row0 + rr;
    const int v = row < n_in ? inv[(size_t)k * cap_in + row] : -1;
    const bool ok = dgrad_is_nbr(v, n_out);
    s_idx[e] = ok ? v : -1;
    if (__ballot(ok) != 0ull && lane == 0) atomicOr(&s_mask, 1u << k);
  }
  __syncthreads();
  const unsigned mask = s_mask;
  const int nchunks = (cout + kDgKC - 1) / kDgKC;
  const int nseg = __popc(mask) * nchunks;

  f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.0f;

  DgSlab<BM> sa;
  DgSlab<BN> sb;
  // the segment to fetch next: offset fk (the lowest bit of `left` that is gone from it), chunk fc
  unsigned left = mask;
  int fk = 0, fc = 0;
  auto next_offset = [&]() {
    fk = left ? __ffs(left) - 1 : 0;
    left &= left - 1u;
  };
  auto fetch = [&]() {
    const int c0 = fc * kDgKC;
#pragma unroll
    for (int i = 0; i < DgSlab<BM>::kPer; ++i) {
      const int item = t + i * kDgThreads;
      const int o = s_idx[fk * BM + (item >> 3)];
      sa.r[i] = dg_load4<VEC>(dout + (size_t)(o >= 0 ? o : 0) * (size_t)cout, c0 + 4 * (item & 7), cout);
      sa.valid[i] = dg_valid(c0 + 4 * (item & 7), cout, o >= 0);
    }
#pragma unroll
    for (int i = 0; i < DgSlab<BN>::kPer; ++i) {
      const int item = t + i * kDgThreads;
      const int ci = q0 + (item >> 3);
      sb.r[i] = dg_load4<VEC>(W + ((size_t)fk * cin + (ci < cin ? ci : cin - 1)) * (size_t)cout, c0 + 4 * (item & 7), cout);
      sb.valid[i] = dg_valid(c0 + 4 * (item & 7), cout, ci < cin);
    }
    if (++fc == nchunks) {
      fc = 0;
      next_offset();
    }
  };

  if (nseg > 0) {
    next_offset();
    fetch();
    sa.put(As[0], t);
    sb.put(Bs[0], t);
  }
  __syncthreads();
  // The body is ONE basic block on purpose.  A fetch or a put under `if (s + 1 < nseg)` makes the loaded registers values of
  // a phi, whose copies the compiler places right behind the loads -- in front of the MFMAs, where they wait for the loads.
  // So the last iteration fetches once more (after the last segment fk = fc = 0: offset 0, chunk 0, clamped rows -- valid
  // addresses, since nseg > 0 means n_out > 0) and puts what it got into the buffer nobody reads again.
  for (int s = 0; s < nseg; ++s) {                           // (nseg is the same in every thread of the workgroup)
    const int cur = s & 1;
    fetch();                                                 // the next segment's loads fly during this segment's MFMAs:
    __builtin_amdgcn_sched_barrier(0);                       // they are issued here, not where register pressure would like them,
    float av[16], bv[16];
    dg_read16(As[cur] + (wp * 32 + r) * kDgPitch + h * (kDgKC / 2), av);
    dg_read16(Bs[cur] + (wq * 32 + r) * kDgPitch + h * (kDgKC / 2), bv);
#pragma unroll
    for (int st = 0; st < kDgKC / 2; ++st)                   // step st: channel 2 st (lanes 0..31), then 2 st + 1 (lanes 32..63)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[st], bv[st], acc, 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);                       // and nothing that touches a loaded value moves in front of the MFMAs
    sa.put(As[cur ^ 1], t);                                  // (the other buffer: last read before the previous barrier)
    sb.put(Bs[cur ^ 1], t);
    __syncthreads();
  }
  // accumulator register e of lane half h: tile row rowmap(e, h), column lane & 31.  Every element of the tile's live rows and
  // columns is written, +0 for a row without neighbours
  const int ci = q0 + wq * 32 + r;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const long long row = row0 + wp * 32 + rowmap(e, h);
    if (row < n_in && ci < cin) dx[(size_t)row * (size_t)cin + ci] = acc[e];
  }
}

template <int WP, int WQ>
void launch_dgrad(hipStream_t s, const float *dout, int n_out, const int32_t *inv, int cap_in, int n_in, const float *W, int cin,
                  int cout, int kvol, float *dx) {
  const dim3 grid(dcl_div_up(n_in, 32 * WP), dcl_div_up(cin, 32 * WQ));
  // 16-byte loads where every row of dout and of W starts on a 16-byte boundary
  if ((((size_t)dout | (size_t)W) & 15) == 0 && (cout & 3) == 0)
    hipLaunchKernelGGL((k_conv_dgrad<WP, WQ, true>), grid, dim3(kDgThreads), 0, s, dout, n_out, inv, cap_in, n_in, W, cin, cout, kvol,
                       dx);
  else
    hipLaunchKernelGGL((k_conv_dgrad<WP, WQ, false>), grid, dim3(kDgThreads), 0, s, dout, n_out, inv, cap_in, n_in, W, cin, cout,
                       kvol, dx);
}

bool dg_aligned4(const void *p) { return ((size_t)p & 3) == 0; }

#if !defined(__HIP_DEVICE_COMPILE__)
// The host twin's rows.  wt is W with each offset transposed to (cout, cin), made by the caller, so that the innermost loop runs
// over the cin INDEPENDENT chains of a row; each of them takes conv_dgrad.h's steps in conv_dgrad.h's order.
__attribute__((always_inline)) inline void dg_host_rows(const float *dout, int n_out, const int32_t *inv, int cap_in, int n_in,
                                                        const float *wt, int cin, int cout, int kvol, float *dx) {
  for (int i = 0; i < n_in; ++i) {
    float *a = dx + (size_t)i * cin;
    for (int ci = 0; ci < cin; ++ci) a[ci] = 0.0f;
    for (int k = 0; k < kvol; ++k) {
      const int o = inv[(size_t)k * cap_in + i];
      if (!dgrad_is_nbr(o, n_out)) continue;
      const float *g = dout + (size_t)o * cout, *wk = wt + (size_t)k * cin * cout;
      for (int co = 0; co < cout; ++co) {
        const float gv = g[co];
        const float *w = wk + (size_t)co * cin;
        for (int ci = 0; ci < cin; ++ci) a[ci] = dgrad_step(a[ci], gv, w[ci]);
      }
    }
  }
}
void dg_host_rows_plain(const float *dout, int n_out, const int32_t *inv, int cap_in, int n_in, const float *wt, int cin, int cout,
                        int kvol, float *dx) {
  dg_host_rows(dout, n_out, inv, cap_in, n_in, wt, cin, cout, kvol, dx);
}
#if defined(__x86_64__)
// the same steps where the processor has a fused multiply-add of its own: fmaf is one instruction instead of a library call
__attribute__((target("avx2,fma"))) void dg_host_rows_fma(const float *dout, int n_out, const int32_t *inv, int cap_in, int n_in,
                                                          const float *wt, int cin, int cout, int kvol, float *dx) {
  dg_host_rows(dout, n_out, inv, cap_in, n_in, wt, cin, cout, kvol, dx);
}
#endif
#endif

}  // namespace

#define DCL_CONV_DGRAD_CHECK()                                                                                              \
  DCL_CHECK_ARG(kvol >= 1 && kvol <= kDgradMaxKvol && n_in >= 0 && n_out >= 0 && cin >= 1 && cout >= 1 && cap_in >= n_in);  \
  DCL_CHECK_ARG(cap_in >= 1 && n_in < (1 << 30) && (long long)cin * cout < (1ll << 31) / 27);                               \
  DCL_CHECK_ARG(W && dg_aligned4(W) && (n_out == 0 || (dout && dg_aligned4(dout))));                                        \
  DCL_CHECK_ARG(n_in == 0 || (inv && dx && dg_aligned4(inv) && dg_aligned4(dx)))

DCL_API int dcl_sparse_conv_dgrad(const float *dout, int n_out, const int32_t *inv, int cap_in, int n_in, const float *W,
                                  int cin, int cout, int kvol, float *dx, dclStream_t stream) {
  DCL_CONV_DGRAD_CHECK();
  if (n_in == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  // one 32 x 32 accumulator per wave.  Narrow layers are the shallow ones with many rows: 128 rows x 32 channels; wider ones
  // take 64 x 64 tiles and as many tile columns as cin needs -- the deep layers have few rows (13 k at 128 -> 256), and smaller
  // tiles keep their workgroups well above the CU count (64 x 128 tiles measured slower on both 128-wide layers)
  if (cin <= 32) launch_dgrad<4, 1>(s, dout, n_out, inv, cap_in, n_in, W, cin, cout, kvol, dx);
  else launch_dgrad<2, 2>(s, dout, n_out, inv, cap_in, n_in, W, cin, cout, kvol, dx);
  DCL_LAUNCH_CHECK();
  return 0;
}

DCL_API int dcl_sparse_conv_dgrad_host(const float *dout, int n_out, const int32_t *inv, int cap_in, int n_in, const float *W,
                                       int cin, int cout, int kvol, float *dx) {
  DCL_CONV_DGRAD_CHECK();
#if !defined(__HIP_DEVICE_COMPILE__)
  if (n_in == 0) return 0;
  std::vector<float> wt((size_t)kvol * cin * cout);
  for (int k = 0; k < kvol; ++k)
    for (int ci = 0; ci < cin; ++ci)
      for (int co = 0; co < cout; ++co) wt[((size_t)k * cout + co) * cin + ci] = W[((size_t)k * cin + ci) * cout + co];
#if defined(__x86_64__)
  if (__builtin_cpu_supports("avx2") && __builtin_cpu_supports("fma")) {
    dg_host_rows_fma(dout, n_out, inv, cap_in, n_in, wt.data(), cin, cout, kvol, dx);
    return 0;
  }
#endif
  dg_host_rows_plain(dout, n_out, inv, cap_in, n_in, wt.data(), cin, cout, kvol, dx);
#endif
  return 0;
}
