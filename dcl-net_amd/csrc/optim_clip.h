// optim_clip.h -- what AutoClip's device form (optim.hip: dcl_autoclip_observe) and its host twin (optim_clip_host.cpp) share:
// the order of the norm history, one lane's part of the insertion, and the percentile / clip-factor arithmetic of
// include/dclnet_hip.h line by line -- so the kernels have the twin's bits, and the twin np.percentile's.
#pragma once
#include "common.h"
#include <math.h>

// The key of the sorted history: ascending numeric, a NaN of either sign behind everything else and all NaN equal.  Entries
// are norms (>= +0, +inf or NaN), so -0 never meets +0.  true: the held entry e stays BEHIND the new x; an entry equal to x
// stays in front of it.
__host__ __device__ inline bool dcl_clip_after(double e, double x) { return e > x || (e != e && x == x); }

// Lane i of the insertion of x into src[0 .. n) (ascending by the key above) -> dst[0 .. n]: the lane moves src[i] to i or
// i + 1, and the lane at the boundary also stores x -- behind the last entry that is not after x, or lane 0 at the head when
// every entry is.  Lane 0 runs for n == 0 too (it stores x alone) and records the arrival.  Exactly one lane stores x, every
// slot of dst[0 .. n] is written once, nothing else is touched.
__host__ __device__ inline void dcl_clip_insert_lane(int64_t n, const double *src, double *dst, double *arrival, double x,
                                                     int64_t i) {
  if (i == 0) {
    arrival[n] = x;
    if (n == 0 || dcl_clip_after(src[0], x)) dst[0] = x;
  }
  if (i >= n) return;
  const double e = src[i];
  if (dcl_clip_after(e, x)) {
    dst[i + 1] = e;
    return;
  }
  dst[i] = e;
  if (i == n - 1 || dcl_clip_after(src[i + 1], x)) dst[i + 1] = x;
}

// out[0] = norm, out[1] = clip_value, out[2] = scale as doubles; the float at byte DCL_AUTOCLIP_SCALE_F32_OFFSET = scale
// rounded once.  s = the m = n + 1 sorted norms, this step's included.  numpy's `linear` percentile (lerp with its t >= 0.5
// form, NaN when the history holds one) and Python's min(1.0, clip / (norm + 1e-6)), every operation rounded on its own.
__host__ __device__ inline void dcl_clip_finish(int64_t n, const double *s, double norm, double percentile, double *out) {
#pragma clang fp contract(off)
  const int64_t m = n + 1;
  const double vi = (double)(m - 1) * (percentile / 100.0);
  const double fl = floor(vi);
  const double t = vi - fl;
  int64_t lo = (int64_t)fl;
  lo = lo < 0 ? 0 : (lo > m - 1 ? m - 1 : lo);
  const int64_t hi = lo + 1 < m - 1 ? lo + 1 : m - 1;
  const double a = s[lo], b = s[hi];
  const double d = b - a;
  double clip;
  if (t >= 0.5) {
    const double w = 1.0 - t;
    const double dw = d * w;
    clip = b - dw;
  } else {
    const double dt = d * t;
    clip = a + dt;
  }
  // A NaN the interpolation makes itself (inf - inf) has no operand to take its bits from, and processors differ in the sign
  // they give it: it is written as the quiet NaN with the sign set, which is what numpy's own subtraction leaves on x86-64.
  if (clip != clip) clip = __builtin_bit_cast(double, (uint64_t)0xFFF8000000000000ull);
  const double last = s[m - 1];
  if (last != last) clip = last;                                       // np.percentile with a NaN anywhere: the last entry itself
  const double q = clip / (norm + 1e-6);
  const double scale = q < 1.0 ? q : 1.0;
  out[0] = norm;
  out[1] = clip;
  out[2] = scale;
  reinterpret_cast<float *>(out)[DCL_AUTOCLIP_SCALE_F32_OFFSET / 4] = (float)scale;
}

// the refusals both entries make before any work
#define DCL_AUTOCLIP_CHECK_ARGS()                                                                                       \
  do {                                                                                                                  \
    DCL_CHECK_ARG(n >= 0 && n <= DCL_AUTOCLIP_MAX_N);                                                                   \
    DCL_CHECK_ARG(percentile >= 0.0 && percentile <= 100.0);                                                            \
    DCL_CHECK_ARG(sorted_dst && arrival && norm && out && (sorted_src || n == 0));                                      \
    DCL_CHECK_ARG(sorted_src != sorted_dst);                                                                            \
  } while (0)
