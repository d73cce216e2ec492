// autoclip_host_check.cpp -- a stand-alone program over the HOST twin of AutoClip's device form (csrc/optim_clip_host.cpp), for
// a CPU sanitizer build:  make -C dcl-net_amd/csrc hostcheck  compiles the twin and this file with -fsanitize=address,undefined
// (host code only, no device pass) and runs it.  It calls no GPU function.
// Every buffer is allocated at its exact size (n entries the source, n + 1 the destination and the arrivals), so that a write
// or read one element past any of them is reported; the expected values come from a second transcription below: a stable
// insertion into a std::vector and the percentile written out from numpy's `linear` method.
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <limits>
#include <vector>
#include "../include/dclnet_hip.h"

#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      fprintf(stderr, "autoclip_host_check: FAILED: %s (line %d): %s\n", #cond, __LINE__, dcl_last_error()); \
      return 1;                                                       \
    }                                                                 \
  } while (0)

static bool same_bits(double a, double b) { return !memcmp(&a, &b, 8); }
static bool key_less(double a, double b) { return (a < b) || (a == a && b != b); }      // NaN last, all NaN equal

struct Out {
  double norm, clip, scale;
  float scale32;
  uint32_t pad;
};
static_assert(sizeof(Out) == DCL_AUTOCLIP_OUT_BYTES && offsetof(Out, scale32) == DCL_AUTOCLIP_SCALE_F32_OFFSET, "out layout");

// np.percentile(sorted, q), method `linear`, and min(1.0, clip / (norm + 1e-6))
static Out expect(const std::vector<double> &s, double x, double q) {
  const int64_t m = (int64_t)s.size();
  const double vi = (double)(m - 1) * (q / 100.0), fl = floor(vi), t = vi - fl;
  const int64_t lo = std::min<int64_t>((int64_t)fl, m - 1), hi = std::min<int64_t>(lo + 1, m - 1);
  const double a = s[(size_t)lo], b = s[(size_t)hi], d = b - a;
  double clip;
  if (t >= 0.5) { const double w = 1.0 - t; const double dw = d * w; clip = b - dw; }
  else { const double dt = d * t; clip = a + dt; }
  if (s.back() != s.back()) clip = s.back();
  const double qq = clip / (x + 1e-6);
  Out o;
  o.norm = x; o.clip = clip; o.scale = qq < 1.0 ? qq : 1.0; o.scale32 = (float)o.scale; o.pad = 0;
  return o;
}

static int feed(const std::vector<double> &seq, double q, bool *took_upper, bool *took_lower) {
  std::vector<double> want, arrival_want, src;                       // src: exactly n entries
  for (size_t step = 0; step < seq.size(); ++step) {
    const int64_t n = (int64_t)step;
    const double x = seq[step];
    std::vector<double> dst((size_t)n + 1, -1.0), arrival((size_t)n + 1, -1.0);
    std::copy(arrival_want.begin(), arrival_want.end(), arrival.begin());
    Out got;
    memset(&got, 0xAB, sizeof(got));
    CHECK(dcl_autoclip_observe_host(n, n ? src.data() : nullptr, dst.data(), arrival.data(), &x, q, &got) == 0);
    want.insert(std::upper_bound(want.begin(), want.end(), x, key_less), x);
    arrival_want.push_back(x);
    CHECK(!memcmp(dst.data(), want.data(), want.size() * 8));
    CHECK(!memcmp(arrival.data(), arrival_want.data(), arrival_want.size() * 8));
    const Out e = expect(want, x, q);
    CHECK(same_bits(got.norm, e.norm) && same_bits(got.scale, e.scale) && !memcmp(&got.scale32, &e.scale32, 4));
    CHECK(same_bits(got.clip, e.clip) || (got.clip != got.clip && e.clip != e.clip && want.back() == want.back()));
    CHECK(got.scale >= 0.0 && got.scale <= 1.0);
    const double vi = (double)n * (q / 100.0);
    (vi - floor(vi) >= 0.5 ? *took_upper : *took_lower) = true;
    src = dst;
  }
  return 0;
}

int main() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  std::vector<std::vector<double>> seqs;
  std::vector<double> up, down, same, mixed;
  uint64_t r = 0x9E3779B97F4A7C15ull;
  for (int i = 0; i < 70; ++i) {
    up.push_back(0.25 * i);
    down.push_back(200.0 - 1.5 * i);                                  // norms: never below +0
    same.push_back(3.0);
    r = r * 6364136223846793005ull + 1442695040888963407ull;
    mixed.push_back((double)(r >> 40) / 1024.0 * (i % 7 == 0 ? 0.0 : 1.0));     // ties at +0 among random values
  }
  seqs.push_back(up); seqs.push_back(down); seqs.push_back(same); seqs.push_back(mixed);
  seqs.push_back({1.0, inf});
  seqs.push_back({2.0, inf, 1.0, inf, 0.5, 3.0});
  seqs.push_back({1.0, 2.0, 0.5, 4.0, nan, 3.0, 0.25, inf, 5.0, nan, 1.0, 0.0});
  seqs.push_back({7.0});
  seqs.push_back({0.0, 0.0});
  const double qs[] = {0.0, 10.0, 25.0, 37.5, 50.0, 90.0, 99.9, 100.0};
  bool upper = false, lower = false;
  for (const auto &seq : seqs)
    for (double q : qs)
      if (feed(seq, q, &upper, &lower)) return 1;
  CHECK(upper && lower);                                              // both branches of t >= 0.5
  // refusals: before any work, so the poisoned destination stays as it is
  double src[2] = {1.0, 2.0}, dst[3] = {-1.0, -1.0, -1.0}, arr[3] = {-1.0, -1.0, -1.0}, x = 1.5;
  Out o;
  CHECK(dcl_autoclip_observe_host(-1, src, dst, arr, &x, 50.0, &o) == DCL_EINVAL);
  CHECK(dcl_autoclip_observe_host(2, nullptr, dst, arr, &x, 50.0, &o) == DCL_EINVAL);
  CHECK(dcl_autoclip_observe_host(2, src, nullptr, arr, &x, 50.0, &o) == DCL_EINVAL);
  CHECK(dcl_autoclip_observe_host(2, src, dst, nullptr, &x, 50.0, &o) == DCL_EINVAL);
  CHECK(dcl_autoclip_observe_host(2, src, dst, arr, nullptr, 50.0, &o) == DCL_EINVAL);
  CHECK(dcl_autoclip_observe_host(2, src, dst, arr, &x, 50.0, nullptr) == DCL_EINVAL);
  CHECK(dcl_autoclip_observe_host(2, src, src, arr, &x, 50.0, &o) == DCL_EINVAL);
  CHECK(dcl_autoclip_observe_host(2, src, dst, arr, &x, -1.0, &o) == DCL_EINVAL);
  CHECK(dcl_autoclip_observe_host(2, src, dst, arr, &x, 100.5, &o) == DCL_EINVAL);
  CHECK(dcl_autoclip_observe_host(2, src, dst, arr, &x, nan, &o) == DCL_EINVAL);
  CHECK(dst[0] == -1.0 && dst[1] == -1.0 && dst[2] == -1.0 && arr[2] == -1.0);
  CHECK(dcl_autoclip_observe_host(2, src, dst, arr, &x, 50.0, &o) == 0);
  CHECK(dst[0] == 1.0 && dst[1] == 1.5 && dst[2] == 2.0 && arr[2] == 1.5 && o.clip == 1.5 && o.scale < 1.0);
  printf("autoclip_host_check: ok\n");
  return 0;
}
