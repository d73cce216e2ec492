// metric_table_host.cpp -- the host twin of metric_table.hip's tabulation in plain C++ (what the tests compare the kernel with,
// and what tables on CPU tensors update through; no GPU call): the same step (metric_table.h: dcl_table_step) in the same
// order -- per step t the crops i = 0 .. b-1 ascending, each into the entry of its own class.
#include "common.h"
#include "metric_table.h"

DCL_API int dcl_metric_tabulate_host(int mode, int T, int b, int C, const float *dis, const int32_t *cls, const int32_t *valid,
                                     const double *diameter, double *sums, double *maxd, int64_t *counts, int32_t *bad) {
  DCL_TABLE_CHECK_ARGS();
  if (b == 0) return 0;
  DCL_CHECK_ARG(dis && cls && T <= (1 << 20));
  for (int t = 0; t < T; ++t)
    for (int i = 0; i < b; ++i) {
      if (valid && valid[i] < 0) continue;                               // not a crop: nothing is updated, bad included
      const int c = cls[i];
      if ((unsigned)c >= (unsigned)C) {
        bad[0] = 1;
        continue;
      }
      const size_t e = (size_t)t * C + c;
      DclTableAcc a;
      dcl_table_load(mode, e, sums, maxd, counts, a);
      dcl_table_step(mode, !(valid && valid[i] == 0), dis[(size_t)t * b + i], mode == DCL_TABLE_ADDS ? 0.0 : diameter[c], a);
      dcl_table_store(mode, e, a, sums, maxd, counts);
    }
  return 0;
}
