// metric_table_host_check.cpp -- a stand-alone program over the HOST twin of the evaluation tables' update
// (csrc/metric_table_host.cpp), for a CPU sanitizer build:  make -C dcl-net_amd/csrc hostcheck  compiles the twin and this file
// with -fsanitize=address,undefined (host code only, no device pass) and runs it.  It calls no GPU function.
// Every buffer is allocated at its exact size, so that a write or read one element past any of them is reported; the expected
// tables come from a second, per-crop transcription of sharding.AddsTable.add / LmTable.add / LmoTable.add_lost below.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <limits>
#include <vector>
#include "../include/dclnet_hip.h"

#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      fprintf(stderr, "metric_table_host_check: FAILED: %s (line %d): %s\n", #cond, __LINE__, dcl_last_error()); \
      return 1;                                                       \
    }                                                                 \
  } while (0)

struct Table {
  int T, C;
  std::vector<double> sums, maxd, diameter;
  std::vector<int64_t> counts;
  int32_t bad;
  Table(int T_, int C_) : T(T_), C(C_), sums((size_t)T_ * C_ * 4), maxd((size_t)T_ * C_), diameter((size_t)C_),
                          counts((size_t)T_ * C_ * 2), bad(0) {}
  bool same(const Table &o) const {
    return sums.size() == o.sums.size() && !memcmp(sums.data(), o.sums.data(), sums.size() * 8) &&
           !memcmp(maxd.data(), o.maxd.data(), maxd.size() * 8) && counts == o.counts && bad == o.bad;
  }
};

// the host classes, one crop at a time
static void expect(int mode, Table &w, int t, int c, float df, bool valid) {
  if (c < 0 || c >= w.C) { w.bad = 1; return; }
  const size_t e = (size_t)t * w.C + c;
  const double d = valid ? (double)df : std::numeric_limits<double>::infinity();
  if (mode == DCL_TABLE_ADDS) {
    w.sums[e * 4] += 1;
    if (d <= 0.1) { w.sums[e * 4 + 1] += 1; w.sums[e * 4 + 2] += d; w.maxd[e] = d > w.maxd[e] ? d : w.maxd[e]; }
    if (d < 0.02) w.sums[e * 4 + 3] += 1;
    return;
  }
  if (!valid) { if (mode == DCL_TABLE_LMO) w.counts[e * 2] += 1; return; }
  w.counts[e * 2] += 1;
  if (d < w.diameter[(size_t)c]) w.counts[e * 2 + 1] += 1;
}

static int run(int mode, Table &g, int b, const float *dis, const int32_t *cls, const int32_t *valid) {
  return dcl_metric_tabulate_host(mode, g.T, b, g.C, dis, cls, valid, g.diameter.data(), g.sums.data(), g.maxd.data(),
                                  g.counts.data(), &g.bad);
}

int main() {
  const float inf = std::numeric_limits<float>::infinity();
  const float edge[] = {nextafterf(0.1f, 0.0f), 0.1f, nextafterf(0.02f, 0.0f), 0.02f, 0.0f, 1e-42f, nanf(""), inf, 0.05f, 0.3f};
  const int n_edge = (int)(sizeof(edge) / sizeof(edge[0]));
  CHECK((double)0.1f > 0.1 && (double)0.02f < 0.02);                  // the reason the comparisons are pinned in double
  const int modes[] = {DCL_TABLE_ADDS, DCL_TABLE_LM, DCL_TABLE_LMO};
  const int Cs[] = {1, 21, 64, 65, 130}, bs[] = {0, 1, 7, 33}, Ts[] = {1, 3};
  for (int mode : modes)
    for (int C : Cs)
      for (int T : Ts) {
        Table got(T, C), want(T, C);
        for (int c = 0; c < C; ++c) {
          // a diameter equal to a distance, one ulp above it, and an ordinary one
          const double dd = (double)edge[c % 5];
          got.diameter[(size_t)c] = want.diameter[(size_t)c] = c % 3 == 0 ? dd : c % 3 == 1 ? nextafter(dd, 1.0) : 0.015;
        }
        int frame = 0;
        for (int b : bs)
          for (int all_invalid = 0; all_invalid < 2; ++all_invalid, ++frame) {
            std::vector<float> dis((size_t)T * b);
            std::vector<int32_t> cls((size_t)b), valid((size_t)b);
            for (int i = 0; i < b; ++i) {
              cls[(size_t)i] = (i * 5 + frame) % C;
              valid[(size_t)i] = all_invalid ? 0 : (i % 4 != 3);
              for (int t = 0; t < T; ++t) dis[(size_t)t * b + i] = edge[(i + 3 * t + frame) % n_edge];
            }
            const int32_t *vp = (frame % 3 == 2 && !all_invalid) ? nullptr : valid.data();
            CHECK(run(mode, got, b, dis.data(), cls.data(), vp) == 0);
            for (int t = 0; t < T; ++t)
              for (int i = 0; i < b; ++i) expect(mode, want, t, cls[(size_t)i], dis[(size_t)t * b + i], !vp || vp[i] != 0);
            CHECK(got.same(want));
          }
        CHECK(got.bad == 0);
        // class ids -1 and C raise `bad` and change nothing else
        const Table before = got;
        const int32_t out_of_range[2] = {-1, C};
        const float d2[6] = {0.01f, 0.01f, 0.01f, 0.01f, 0.01f, 0.01f};
        CHECK(run(mode, got, 2, d2, out_of_range, nullptr) == 0);
        CHECK(got.bad == 1);
        got.bad = 0;
        CHECK(got.same(before));
        // rows of valid < 0 are not crops: nothing changes and `bad` stays down, whatever their class id and distance
        const int32_t pad_cls[4] = {0, -1, C, 1 << 30}, pad_valid[4] = {-1, -7, -1, INT32_MIN};
        const float d4[12] = {0.01f, NAN, INFINITY, 0.0f, 0.01f, NAN, INFINITY, 0.0f, 0.01f, NAN, INFINITY, 0.0f};
        CHECK(run(mode, got, 4, d4, pad_cls, pad_valid) == 0);
        CHECK(got.bad == 0 && got.same(before));
      }
  // refusals
  Table t1(1, 2);
  const float d1[1] = {0.01f};
  const int32_t c1[1] = {0};
  CHECK(run(3, t1, 1, d1, c1, nullptr) == DCL_EINVAL);
  CHECK(run(-1, t1, 1, d1, c1, nullptr) == DCL_EINVAL);
  CHECK(run(DCL_TABLE_ADDS, t1, -1, d1, c1, nullptr) == DCL_EINVAL);
  CHECK(run(DCL_TABLE_ADDS, t1, 1, nullptr, c1, nullptr) == DCL_EINVAL);
  CHECK(run(DCL_TABLE_ADDS, t1, 1, d1, nullptr, nullptr) == DCL_EINVAL);
  CHECK(dcl_metric_tabulate_host(DCL_TABLE_ADDS, 0, 1, 2, d1, c1, nullptr, nullptr, t1.sums.data(), t1.maxd.data(), nullptr, &t1.bad) == DCL_EINVAL);
  CHECK(dcl_metric_tabulate_host(DCL_TABLE_ADDS, 1, 1, 0, d1, c1, nullptr, nullptr, t1.sums.data(), t1.maxd.data(), nullptr, &t1.bad) == DCL_EINVAL);
  CHECK(dcl_metric_tabulate_host(DCL_TABLE_ADDS, 1, 1, 2, d1, c1, nullptr, nullptr, nullptr, t1.maxd.data(), nullptr, &t1.bad) == DCL_EINVAL);
  CHECK(dcl_metric_tabulate_host(DCL_TABLE_ADDS, 1, 1, 2, d1, c1, nullptr, nullptr, t1.sums.data(), t1.maxd.data(), nullptr, nullptr) == DCL_EINVAL);
  CHECK(dcl_metric_tabulate_host(DCL_TABLE_LM, 1, 1, 2, d1, c1, nullptr, nullptr, nullptr, nullptr, t1.counts.data(), &t1.bad) == DCL_EINVAL);
  CHECK(dcl_metric_tabulate_host(DCL_TABLE_LMO, 1, 1, 2, d1, c1, nullptr, t1.diameter.data(), nullptr, nullptr, nullptr, &t1.bad) == DCL_EINVAL);
  // the arrays a mode does not use may be NULL; an empty batch touches nothing
  CHECK(dcl_metric_tabulate_host(DCL_TABLE_ADDS, 1, 1, 2, d1, c1, nullptr, nullptr, t1.sums.data(), t1.maxd.data(), nullptr, &t1.bad) == 0);
  CHECK(dcl_metric_tabulate_host(DCL_TABLE_LM, 1, 1, 2, d1, c1, nullptr, t1.diameter.data(), nullptr, nullptr, t1.counts.data(), &t1.bad) == 0);
  CHECK(dcl_metric_tabulate_host(DCL_TABLE_LM, 1, 0, 2, nullptr, nullptr, nullptr, t1.diameter.data(), nullptr, nullptr, t1.counts.data(), &t1.bad) == 0);
  CHECK(t1.sums[0] == 1 && t1.sums[1] == 1 && t1.sums[3] == 1 && t1.counts[0] == 1 && t1.counts[1] == 0 && t1.bad == 0);
  printf("metric_table_host_check: ok\n");
  return 0;
}
