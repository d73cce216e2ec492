// crop_draw_host_check.cpp -- a stand-alone program over the HOST twins of the device draw (csrc/crop_draw_host.cpp), for a CPU
// sanitizer build:  make -C dcl-net_amd/csrc hostcheck   compiles the twins' sources and this file with
// -fsanitize=address,undefined (host code only, no device pass) and runs it.  It calls no GPU function.
// Every buffer is allocated at its exact size, so that a write or read one element past any of them is reported.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../include/dclnet_hip.h"

#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      fprintf(stderr, "crop_draw_host_check: FAILED: %s (line %d): %s\n", #cond, __LINE__, dcl_last_error()); \
      return 1;                                                       \
    }                                                                 \
  } while (0)

int main() {
  uint64_t base = 0, keys[2];
  CHECK(dcl_crop_draw_keys_host(1, 0, 0, 0, 2, &base, keys) == 0);
  CHECK(base == 0x6df1421574b0d586ull && keys[0] == 0x96c9f513020798b9ull && keys[1] == 0xf7dd055ed9ec356full);
  CHECK(dcl_crop_draw_keys_host(2, 7, 3, 1, 2, &base, keys) == 0);
  CHECK(base == 0x9fb95fa8ca6188d9ull && keys[0] == 0xc1bed6510d07ff6cull && keys[1] == 0x3c33370239554870ull);

  const int npoints[] = {1, 16, 1000, 1024, 4096};
  for (int npoint : npoints) {
    const int ms[] = {0, 1, 5, npoint - 1, npoint, npoint + 1, 2 * npoint + 3, 4097, 70001, 300000};
    const int n = (int)(sizeof(ms) / sizeof(ms[0]));
    std::vector<int32_t> counts((size_t)n * 3), valid((size_t)n);
    std::vector<int64_t> idx((size_t)n * npoint);
    for (int i = 0; i < n; ++i) counts[3 * i] = counts[3 * i + 1] = counts[3 * i + 2] = ms[i];
    for (uint64_t frame : {0ull, 1ull << 40}) {
      CHECK(dcl_crop_draw_host(n, npoint, counts.data(), 32, 1, 0xFEDCBA9876543210ull, frame, idx.data(), valid.data()) == 0);
      for (int i = 0; i < n; ++i) {
        CHECK(valid[i] == (ms[i] > 0));
        for (int j = 0; j < npoint; ++j) CHECK(idx[(size_t)i * npoint + j] >= 0 && idx[(size_t)i * npoint + j] < (ms[i] > 0 ? ms[i] : 1));
      }
    }
    // the keyed twin on scrambled (frame, inst) keys: row i is row keys[i][1] of the plain draw with frame keys[i][0], made here
    // on a counts array that has the row's counts at that position
    {
      std::vector<uint64_t> rk((size_t)n * 2);
      std::vector<int32_t> kvalid((size_t)n), c2((size_t)n * 3), v2((size_t)n);
      std::vector<int64_t> kidx((size_t)n * npoint), idx2((size_t)n * npoint);
      for (int i = 0; i < n; ++i) { rk[2 * i] = (i % 3 == 0) ? (1ull << 40) + 5 : (uint64_t)(i % 3); rk[2 * i + 1] = (uint64_t)((i * 7 + 3) % n); }
      CHECK(dcl_crop_draw_keyed_host(n, npoint, counts.data(), 32, 1, 0xFEDCBA9876543210ull, rk.data(), kidx.data(), kvalid.data()) == 0);
      for (int i = 0; i < n; ++i) {
        const int r = (int)rk[2 * i + 1];
        for (int q = 0; q < n * 3; ++q) c2[q] = 0;
        c2[3 * r] = c2[3 * r + 1] = c2[3 * r + 2] = ms[i];
        CHECK(dcl_crop_draw_host(n, npoint, c2.data(), 32, 1, 0xFEDCBA9876543210ull, rk[2 * i], idx2.data(), v2.data()) == 0);
        CHECK(kvalid[i] == v2[r]);
        for (int j = 0; j < npoint; ++j) CHECK(kidx[(size_t)i * npoint + j] == idx2[(size_t)r * npoint + j]);
      }
    }
    // the sample rows over clouds of exactly the rows the draw may address, one instance without a crop among them
    const int inst = 3, cap = 700, S = 64;
    const int32_t c3[inst * 3] = {cap, cap, cap, 0, 0, 0, cap, 20, cap};
    std::vector<float> xyz((size_t)inst * cap * 3), rgb((size_t)inst * cap * 3), feats((size_t)inst * npoint * 7);
    for (size_t i = 0; i < xyz.size(); ++i) { xyz[i] = (float)((int)(i % 97) - 48) * 0.005f; rgb[i] = (float)(i % 13) * 0.05f; }
    std::vector<int64_t> pick((size_t)inst * npoint), coords((size_t)inst * npoint * 4);
    std::vector<int32_t> v3(inst);
    const float unit[3] = {0.006f, 0.006f, 0.006f};
    CHECK(dcl_crop_draw_host(inst, npoint, c3, 32, 1, 7, 11, pick.data(), v3.data()) == 0);
    CHECK(v3[0] == 1 && v3[1] == 0 && v3[2] == 1);
    CHECK(dcl_crop_sample_valid_host(inst, npoint, cap, xyz.data(), rgb.data(), pick.data(), c3, 32, v3.data(), 0.192f, unit, S,
                                     feats.data(), coords.data()) == 0);
    for (int j = 0; j < npoint; ++j) {
      const int64_t *o = &coords[((size_t)npoint + j) * 4];
      CHECK(o[0] == 1 && o[1] == j % S && o[2] == (j / S) % S && o[3] == j / (S * S));
    }
    for (size_t e = 0; e < (size_t)inst * npoint; ++e)
      for (int k = 1; k < 4; ++k) CHECK(e / npoint == 0 || (coords[e * 4 + k] >= 0 && coords[e * 4 + k] < S));
  }
  // refusals
  int32_t c1[3] = {5, 5, 5}, v1 = 0;
  int64_t i1[8];
  CHECK(dcl_crop_draw_host(1, 0, c1, 32, 1, 0, 0, i1, &v1) == DCL_EINVAL);
  CHECK(dcl_crop_draw_host(1, 4097, c1, 32, 1, 0, 0, i1, &v1) == DCL_EINVAL);
  CHECK(dcl_crop_draw_host(1, 8, nullptr, 32, 1, 0, 0, i1, &v1) == DCL_EINVAL);
  CHECK(dcl_crop_draw_host(0, 8, nullptr, 32, 1, 0, 0, nullptr, nullptr) == 0);
  CHECK(dcl_crop_draw_host(1, 8, c1, 32, 1, 2, 7, i1, &v1) == 0 && v1 == 1);
  const uint64_t k1[2] = {7, 0};
  CHECK(dcl_crop_draw_keyed_host(1, 0, c1, 32, 1, 0, k1, i1, &v1) == DCL_EINVAL);
  CHECK(dcl_crop_draw_keyed_host(1, 4097, c1, 32, 1, 0, k1, i1, &v1) == DCL_EINVAL);
  CHECK(dcl_crop_draw_keyed_host(1, 8, c1, 32, 1, 0, nullptr, i1, &v1) == DCL_EINVAL);
  CHECK(dcl_crop_draw_keyed_host(0, 8, nullptr, 32, 1, 0, nullptr, nullptr, nullptr) == 0);
  // the pinned constants through the keyed twin: base(2,7,3,1) with m = 5 <= npoint draws floor(key(j) * 5 / 2^64)
  const uint64_t k2[2] = {7, 3};
  CHECK(dcl_crop_draw_keyed_host(1, 8, c1, 32, 1, 2, k2, i1, &v1) == 0 && v1 == 1);
  CHECK(i1[0] == (int64_t)(((unsigned __int128)0xc1bed6510d07ff6cull * 5) >> 64));
  CHECK(i1[1] == (int64_t)(((unsigned __int128)0x3c33370239554870ull * 5) >> 64));
  printf("crop_draw_host_check: ok\n");
  return 0;
}
