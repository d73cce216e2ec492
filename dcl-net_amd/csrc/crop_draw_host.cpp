// crop_draw_host.cpp -- the host twins of crop_draw.hip in plain C++ (what the tests compare the kernels with; no GPU call): the
// same draw from the same definition (crop_draw.h) by another route -- every key of the instance, a partial sort -- and the same
// sample / lattice rows through the shared bodies (crops_body.h).
#include <algorithm>
#include <utility>
#include <vector>
#include "common.h"
#include "crops_body.h"
#include "crop_draw.h"

// base(seed, frame, inst, s) and its first n keys (tests pin them; include/dclnet_hip.h)
DCL_API int dcl_crop_draw_keys_host(uint64_t seed, uint64_t frame, int inst, int s, int n, uint64_t *base, uint64_t *keys) {
  DCL_CHECK_ARG(inst >= 0 && (s == 0 || s == 1) && n >= 0 && base && (keys || n == 0));
  *base = draw_base(seed, frame, inst, s);
  for (int j = 0; j < n; ++j) keys[j] = draw_key(*base, (uint64_t)j);
  return 0;
}

namespace {

// rows [0, n_inst) of the draw; row_keys (n_inst,2) {frame, inst} or null: (frame, row)
int crop_draw_rows(int n_inst, int npoint, const int32_t *counts, int min_valid, int keep_sparse, uint64_t seed, uint64_t frame0,
                   const uint64_t *row_keys, int64_t *sample_idx, int32_t *valid) {
  std::vector<std::pair<uint64_t, int32_t>> keys;
  for (int row = 0; row < n_inst; ++row) {
    const int32_t *c = counts + (size_t)row * 3;
    int64_t *out = sample_idx + (size_t)row * npoint;
    const uint64_t frame = row_keys ? row_keys[(size_t)row * 2] : frame0;
    const int inst = row_keys ? (int)row_keys[(size_t)row * 2 + 1] : row;
    const int ok = draw_valid(c, min_valid, keep_sparse ? 1 : 0);
    valid[row] = ok;
    if (!ok) {
      std::fill(out, out + npoint, (int64_t)0);
      continue;
    }
    const int32_t m = c[2];
    if (m <= npoint) {
      const uint64_t base = draw_base(seed, frame, inst, kDrawWithReplacement);
      for (int j = 0; j < npoint; ++j) out[j] = (int64_t)draw_mulhi(draw_key(base, (uint64_t)j), (uint64_t)m);
      continue;
    }
    const uint64_t base = draw_base(seed, frame, inst, kDrawWithoutReplacement);
    keys.resize((size_t)m);
    for (int32_t j = 0; j < m; ++j) keys[(size_t)j] = std::make_pair(draw_key(base, (uint64_t)j), j);
    std::partial_sort(keys.begin(), keys.begin() + npoint, keys.end());          // pairs compare as (key, j)
    for (int j = 0; j < npoint; ++j) out[j] = keys[(size_t)j].second;
  }
  return 0;
}

}  // namespace

DCL_API int dcl_crop_draw_host(int n_inst, int npoint, const int32_t *counts, int min_valid, int keep_sparse, uint64_t seed,
                               uint64_t frame, int64_t *sample_idx, int32_t *valid) {
  DCL_CHECK_ARG(n_inst >= 0 && npoint >= 1 && npoint <= DCL_CROP_DRAW_MAX_POINTS);
  if (n_inst == 0) return 0;
  DCL_CHECK_ARG(counts && sample_idx && valid);
  return crop_draw_rows(n_inst, npoint, counts, min_valid, keep_sparse, seed, frame, nullptr, sample_idx, valid);
}

DCL_API int dcl_crop_draw_keyed_host(int n_inst, int npoint, const int32_t *counts, int min_valid, int keep_sparse, uint64_t seed,
                                     const uint64_t *keys, int64_t *sample_idx, int32_t *valid) {
  DCL_CHECK_ARG(n_inst >= 0 && npoint >= 1 && npoint <= DCL_CROP_DRAW_MAX_POINTS);
  if (n_inst == 0) return 0;
  DCL_CHECK_ARG(counts && keys && sample_idx && valid);
  return crop_draw_rows(n_inst, npoint, counts, min_valid, keep_sparse, seed, 0, keys, sample_idx, valid);
}

DCL_API int dcl_crop_sample_valid_host(int n_inst, int npoint, int cap, const float *xyz, const float *rgb,
                                       const int64_t *sample_idx, const int32_t *counts, int min_valid, const int32_t *valid,
                                       float half_extent0, const float *unit_host /*3*/, int voxel_limit, float *feats,
                                       int64_t *coords) {
  DCL_CHECK_ARG(n_inst >= 0 && npoint >= 1 && npoint <= DCL_CROP_DRAW_MAX_POINTS && cap > 0 && voxel_limit > 0);
  DCL_CHECK_ARG(crop_lattice_fits(npoint, voxel_limit));
  if (n_inst == 0) return 0;
  DCL_CHECK_ARG(xyz && rgb && sample_idx && valid && unit_host && feats && coords);
  const float ux = unit_host[0], uy = unit_host[1], uz = unit_host[2];
  for (int inst = 0; inst < n_inst; ++inst)
    for (int j = 0; j < npoint; ++j) {
      const size_t e = (size_t)inst * npoint + j;
      if (valid[inst] > 0) {
        const long long i = std::min(std::max((long long)sample_idx[e], 0ll), (long long)cap - 1);
        crop_sample_row(xyz + ((size_t)inst * cap + i) * 3, rgb + ((size_t)inst * cap + i) * 3,
                        counts && counts[inst * 3 + 1] <= min_valid, inst, half_extent0, ux, uy, uz, (float)voxel_limit,
                        feats + e * 7, coords + e * 4);
      } else {
        crop_lattice_row(j, voxel_limit, inst, half_extent0, ux, uy, uz, feats + e * 7, coords + e * 4);
      }
    }
  return 0;
}
