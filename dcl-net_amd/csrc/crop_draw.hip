// crop_draw.hip -- the crop builders' sampling draws on the device (crops.py: CropBuilder(draws="device")).
//
// The loaders draw the N observed points of a crop with np.random.choice on the host's MT19937 stream, which needs every
// instance's point count on the host: the builder's one read-back per frame.  This is a different, fully specified sample of the
// same distribution from a counter-based generator (crop_draw.h; contract in include/dclnet_hip.h), made where the counts are:
//
//   dcl_crop_draw          m = counts[inst][2] > npoint: the npoint indices j < m with the smallest key(j), in ascending key
//                          order -- the head of a uniform random permutation; 0 < m <= npoint: idx[j] = floor(key(j) m / 2^64),
//                          with replacement; an instance that gives no crop: a row of zeros and valid = 0
//   dcl_crop_draw_keyed    the same kernel with a (frame, inst) key per row: a batch of several frames draws what the frames
//                          draw one by one (CropBuilder.build_frames)
//   dcl_crop_sample_valid  dcl_crop_sample's rows for the valid instances (crops_body.h: crop_sample_row), a lattice dummy crop
//                          (one point per voxel) for the others, so that nothing uninitialised is read and the capacity form's
//                          pitch flag stays down
//
// k_crop_draw is one workgroup per instance and reads nothing but its counts row.  Keys are a pure function of the index, so
// "the npoint smallest of m keys" is a selection over a stream that costs no memory traffic:
//   1. guess a threshold T near 2^64 (npoint + slack) / m and collect the (key, j) with key <= T into an LDS list (the order of
//      arrival is the order of an LDS counter: it does not matter, the list is sorted next);
//   2. fewer than npoint: double T and collect again (at 2^64 - 1 every index passes, and m > npoint);
//      more than the list holds: find T by a most-significant-digit-first radix select over the keys -- 8-bit digits, descending
//      into the bin that holds the npoint-th smallest key until everything up to that bin fits the list.  Keys of distinct
//      indices differ (crop_draw.h), so the last digit's bin holds one key: at most 8 passes;
//   3. bitonic sort of the list by (key, j) in LDS, the first npoint indices are the draw.
// The result is fixed by the definition, not by the route: every route selects the same set and sorts it.  No float arithmetic, no
// global atomic, no scratch, no workgroup waits for another.
#include "common.h"
#include "crops_body.h"
#include "crop_draw.h"

namespace {

constexpr int kDrawThreads = 1024;
constexpr int kDrawList = 2 * DCL_CROP_DRAW_MAX_POINTS;       // entries of the LDS candidate list: a power of two (the sort's size)
static_assert((kDrawList & (kDrawList - 1)) == 0, "the bitonic sort wants a power of two");

// route: 0 = as described above; diagnostic library only: 1 = radix select from the start, 2 = a first guess 256 times too small
// (the doubling loop), 3 = a first guess of 2^64 - 1 (the list overflows for m > kDrawList: the radix select behind a failed guess)
DCL_HOOK_INT(g_draw_route, 0);

__global__ __launch_bounds__(kDrawThreads) void k_crop_draw(int npoint, const int32_t *__restrict__ counts, int min_valid,
                                                            int keep_sparse, uint64_t seed, uint64_t frame,
                                                            const uint64_t *__restrict__ keys /* (n,2) frame, inst or null */,
                                                            int route, int64_t *__restrict__ sample_idx,
                                                            int32_t *__restrict__ valid) {
  __shared__ uint64_t s_key[kDrawList];
  __shared__ int32_t s_j[kDrawList];
  __shared__ int s_hist[256];
  __shared__ int s_cnt;
  const int t = threadIdx.x, lane = t & 63, inst = blockIdx.x;
  const int32_t *c = counts + (size_t)inst * 3;
  // dcl_crop_draw_keyed: the row's own (frame, inst) key; everything else -- counts row, output row -- stays the row's
  const int kinst = keys ? (int)keys[(size_t)inst * 2 + 1] : inst;
  if (keys) frame = keys[(size_t)inst * 2];
  const int ok = draw_valid(c, min_valid, keep_sparse);
  const uint32_t m = ok ? (uint32_t)c[2] : 0u;
  int64_t *out = sample_idx + (size_t)inst * npoint;
  if (t == 0) valid[inst] = ok;
  if (!ok) {
    for (int j = t; j < npoint; j += kDrawThreads) out[j] = 0;
    return;
  }
  if (m <= (uint32_t)npoint) {                                         // with replacement
    const uint64_t base = draw_base(seed, frame, kinst, kDrawWithReplacement);
    for (int j = t; j < npoint; j += kDrawThreads) out[j] = (int64_t)draw_mulhi(draw_key(base, (uint64_t)j), (uint64_t)m);
    return;
  }
  const uint64_t base = draw_base(seed, frame, kinst, kDrawWithoutReplacement);
  const uint64_t kAll = ~0ull;

  // every (key, j) with key <= T -> the list, as far as it holds them; returns how many there are
  auto collect = [&](uint64_t T) -> int {
    __syncthreads();
    if (t == 0) s_cnt = 0;
    __syncthreads();
    for (uint32_t j0 = 0; j0 < m; j0 += kDrawThreads) {                // a wave-uniform trip count: the ballot below
      const uint32_t j = j0 + t;
      const uint64_t k = draw_key(base, (uint64_t)j);
      const bool pass = j < m && k <= T;
      const unsigned long long bal = __ballot(pass);
      if (bal) {                                                       // one LDS add per wave, the lanes take consecutive slots
        const int leader = __ffsll((long long)bal) - 1;
        int first = 0;
        if (lane == leader) first = atomicAdd(&s_cnt, __popcll(bal));
        first = __shfl(first, leader, 64);
        const int pos = first + __popcll(bal & ((1ull << lane) - 1ull));
        if (pass && pos < kDrawList) { s_key[pos] = k; s_j[pos] = (int32_t)j; }
      }
    }
    __syncthreads();
    return s_cnt;
  };

  // the smallest T = (digits so far | all ones below) under which at least npoint and at most kDrawList keys lie
  auto radix_threshold = [&]() -> uint64_t {
    uint64_t prefix = 0;
    int below = 0;                                                     // keys in front of the prefix' range
    for (int shift = 56; shift >= 0; shift -= 8) {
      const uint64_t himask = shift == 56 ? 0ull : ~0ull << (shift + 8);
      __syncthreads();
      if (t < 256) s_hist[t] = 0;
      __syncthreads();
      for (uint32_t j = t; j < m; j += kDrawThreads) {
        const uint64_t k = draw_key(base, (uint64_t)j);
        if ((k & himask) == prefix) atomicAdd(&s_hist[(int)((k >> shift) & 255ull)], 1);
      }
      __syncthreads();
      int acc = below, bin = 255, binc = 0;
      for (int d = 0; d < 256; ++d) {                                  // every thread walks the same 256 counts
        const int h = s_hist[d];
        if (acc + h >= npoint) { bin = d; binc = h; break; }
        acc += h;
      }
      below = acc;
      prefix |= (uint64_t)bin << shift;
      if (below + binc <= kDrawList) return prefix | (shift ? (1ull << shift) - 1ull : 0ull);
    }
    return prefix;                                                     // not reached: the last digit's bin holds one key
  };

  bool radix = route == 1;
  int cnt = 0;
  if (!radix) {
    const uint32_t want = (uint32_t)npoint + 64u + (uint32_t)npoint / 8u;   // the expected size of the list: 5 sigma and more above npoint
    uint64_t T = (route == 3 || want >= m) ? kAll : (kAll / (uint64_t)m) * (uint64_t)want;
    if (route == 2) T >>= 8;
    for (;;) {
      cnt = collect(T);
      if (cnt > kDrawList) { radix = true; break; }
      if (cnt >= npoint) break;
      T = T > (kAll >> 1) ? kAll : 2ull * T + 1ull;                    // strictly wider; at kAll every index passes and m > npoint
    }
  }
  if (radix) cnt = collect(radix_threshold());
  cnt = min(cnt, kDrawList);                                           // (npoint <= cnt <= kDrawList by construction: the list's bound, restated)

  // pad to the next power of two behind every real entry, bitonic sort by (key, j)
  int n2 = 1;
  while (n2 < cnt) n2 <<= 1;
  for (int i = cnt + t; i < n2; i += kDrawThreads) { s_key[i] = kAll; s_j[i] = 0x7fffffff; }
  __syncthreads();
  for (int k = 2; k <= n2; k <<= 1) {
    for (int d = k >> 1; d > 0; d >>= 1) {
      for (int i = t; i < n2; i += kDrawThreads) {
        const int p = i ^ d;
        if (p > i) {
          const uint64_t ka = s_key[i], kb = s_key[p];
          const int32_t ja = s_j[i], jb = s_j[p];
          const bool up = (i & k) == 0;
          if (draw_less(kb, jb, ka, ja) == up) { s_key[i] = kb; s_key[p] = ka; s_j[i] = jb; s_j[p] = ja; }
        }
      }
      __syncthreads();
    }
  }
  for (int j = t; j < npoint; j += kDrawThreads) out[j] = (int64_t)s_j[j];
}

// dcl_crop_sample's rows for the instances with valid > 0, the lattice dummy crop for the others (valid == 0: no crop; valid < 0:
// a padding row of build_frames(pad_to=...), which has no xyz row at all -- it must not become an address)
__global__ void k_crop_sample_valid(int n_inst, int npoint, int cap, const float *__restrict__ xyz, const float *__restrict__ rgb,
                                    const int64_t *__restrict__ sample_idx, const int32_t *__restrict__ counts, int min_valid,
                                    const int32_t *__restrict__ valid, float half0, float ux, float uy, float uz, int S,
                                    float *__restrict__ feats, int64_t *__restrict__ coords) {
  const long long total = (long long)n_inst * npoint;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    const int inst = (int)(e / npoint);
    const long long j = e - (long long)inst * npoint;
    if (valid[inst] > 0) {
      const long long i = min(max(sample_idx[e], 0ll), (long long)cap - 1);     // a draw lies in [0, m), m <= cap: nothing outside is read
      crop_sample_row(xyz + ((size_t)inst * cap + i) * 3, rgb + ((size_t)inst * cap + i) * 3,
                      counts && counts[inst * 3 + 1] <= min_valid, inst, half0, ux, uy, uz, (float)S, feats + e * 7, coords + e * 4);
    } else {
      crop_lattice_row(j, S, inst, half0, ux, uy, uz, feats + e * 7, coords + e * 4);
    }
  }
}

}  // namespace

#ifdef DCL_DIAG
DCL_API void dcl_debug_crop_draw_route(int route) { g_draw_route = route; }
#endif

DCL_API int dcl_crop_draw(int n_inst, int npoint, const int32_t *counts, int min_valid, int keep_sparse, uint64_t seed,
                          uint64_t frame, int64_t *sample_idx, int32_t *valid, dclStream_t stream) {
  DCL_CHECK_ARG(n_inst >= 0 && npoint >= 1 && npoint <= DCL_CROP_DRAW_MAX_POINTS);
  if (n_inst == 0) return 0;
  DCL_CHECK_ARG(counts && sample_idx && valid);
  const int route = g_draw_route;
  hipLaunchKernelGGL(k_crop_draw, dim3(n_inst), dim3(kDrawThreads), 0, (hipStream_t)stream, npoint, counts, min_valid,
                     keep_sparse ? 1 : 0, seed, frame, (const uint64_t *)nullptr, route, sample_idx, valid);
  DCL_LAUNCH_CHECK();
  return 0;
}

DCL_API int dcl_crop_draw_keyed(int n_inst, int npoint, const int32_t *counts, int min_valid, int keep_sparse, uint64_t seed,
                                const uint64_t *keys, int64_t *sample_idx, int32_t *valid, dclStream_t stream) {
  DCL_CHECK_ARG(n_inst >= 0 && npoint >= 1 && npoint <= DCL_CROP_DRAW_MAX_POINTS);
  if (n_inst == 0) return 0;
  DCL_CHECK_ARG(counts && keys && sample_idx && valid);
  const int route = g_draw_route;
  hipLaunchKernelGGL(k_crop_draw, dim3(n_inst), dim3(kDrawThreads), 0, (hipStream_t)stream, npoint, counts, min_valid,
                     keep_sparse ? 1 : 0, seed, (uint64_t)0, keys, route, sample_idx, valid);
  DCL_LAUNCH_CHECK();
  return 0;
}

DCL_API int dcl_crop_sample_valid(int n_inst, int npoint, int cap, const float *xyz, const float *rgb, const int64_t *sample_idx,
                                  const int32_t *counts, int min_valid, const int32_t *valid, float half_extent0,
                                  const float *unit_host /*3*/, int voxel_limit, float *feats, int64_t *coords,
                                  dclStream_t stream) {
  DCL_CHECK_ARG(n_inst >= 0 && npoint >= 1 && npoint <= DCL_CROP_DRAW_MAX_POINTS && cap > 0 && voxel_limit > 0);
  DCL_CHECK_ARG(crop_lattice_fits(npoint, voxel_limit));
  if (n_inst == 0) return 0;
  DCL_CHECK_ARG(xyz && rgb && sample_idx && valid && unit_host && feats && coords);
  hipLaunchKernelGGL(k_crop_sample_valid, dim3(dcl_grid_1d((long long)n_inst * npoint, 256)), dim3(256), 0, (hipStream_t)stream,
                     n_inst, npoint, cap, xyz, rgb, sample_idx, counts, min_valid, valid, half_extent0, unit_host[0], unit_host[1],
                     unit_host[2], voxel_limit, feats, coords);
  DCL_LAUNCH_CHECK();
  return 0;
}
