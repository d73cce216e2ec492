// optim_clip_host.cpp -- the host twin of optim.hip's dcl_autoclip_observe in plain C++ (what the tests compare the kernels
// with; no GPU call): the same lane function over i = 0 .. n-1 and the same finish (optim_clip.h).
#include "common.h"
#include "optim_clip.h"

DCL_API int dcl_autoclip_observe_host(int64_t n, const double *sorted_src, double *sorted_dst, double *arrival,
                                      const double *norm, double percentile, void *out) {
  DCL_AUTOCLIP_CHECK_ARGS();
  const double x = norm[0];
  const int64_t lanes = n > 0 ? n : 1;
  for (int64_t i = 0; i < lanes; ++i) dcl_clip_insert_lane(n, sorted_src, sorted_dst, arrival, x, i);
  dcl_clip_finish(n, sorted_dst, x, percentile, (double *)out);
  return 0;
}
