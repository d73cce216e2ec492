// template_rows.hip -- deal cached per-class template rows into a call's activation buffers (models/DCL_Net.py: TemplateCache).
//
// In eval mode the template half of a forward -- geometry, backbone_tmp, read-out, the four disengage_Yo stacks -- is a pure
// function of (weights, class).  Network.cache_templates keeps its result per class as rows [p1 256 | m1 64 | p2 256 | m2 64 |
// xyz 3]; a call that carries class ids instead of template clouds gets its Yo activations by ONE launch of this kernel: for
// crop i, row r and column block j, dst_j[(i n_tmp + r) pitch_j + c] = cache[lut[cls[i]]][r][src_col_j + c].  The class ids
// stay on the device: nothing is read back.  A pure stream -- no atomics, no scratch, no LDS; contract in include/dclnet_hip.h.
#include "common.h"

namespace {
struct TemplateBlocks {
  DclTemplateBlock blk[DCL_TEMPLATE_MAX_BLOCKS];
  int32_t unit0[DCL_TEMPLATE_MAX_BLOCKS + 1];      // prefix of the blocks' units per row (a unit = 16 bytes or one float)
  uint32_t vec_mask;                               // bit j: block j moves 16 bytes per lane
  int32_t nblocks;
};

// the cache slot of crop i, -1 for a miss (an id outside the table or a class that is not cached): the table is only read
// inside its bounds
__host__ __device__ inline int template_slot(const int32_t *lut, int lut_len, int id) {
  if ((unsigned)id >= (unsigned)lut_len) return -1;
  const int s = lut[id];
  return s < 0 ? -1 : s;
}

__global__ void __launch_bounds__(256)
k_template_rows(const float *__restrict__ cache, long long class_floats, int row_floats, int n_tmp, const int32_t *__restrict__ lut,
                int lut_len, const int32_t *__restrict__ cls, long long rows, const TemplateBlocks tb, int32_t *miss) {
  const int units = tb.unit0[tb.nblocks];
  const long long total = rows * units;
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
    const long long row = t / units;                                 // crop i, template row r
    const int u = (int)(t - row * units);
    const int i = (int)(row / n_tmp), r = (int)(row - (long long)i * n_tmp);
    int j = 0;
    while (j + 1 < tb.nblocks && u >= tb.unit0[j + 1]) ++j;
    const DclTemplateBlock q = tb.blk[j];
    const int c = u - tb.unit0[j];
    const int slot = template_slot(lut, lut_len, cls[i]);
    const float *src = cache + (slot < 0 ? 0 : (size_t)slot * class_floats + (size_t)r * row_floats + q.src_col);
    float *dst = q.dst + (size_t)row * q.dst_pitch;
    if ((tb.vec_mask >> j) & 1u) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (slot >= 0) v = reinterpret_cast<const float4 *>(src)[c];
      reinterpret_cast<float4 *>(dst)[c] = v;
    } else {
      dst[c] = slot >= 0 ? src[c] : 0.f;
    }
    if (slot < 0 && u == 0) *miss = 1;                               // a plain vector store: every writer stores the same value
  }
}

int check_blocks(const char *func, const DclTemplateBlock *blocks, int nblocks, int row_floats) {
  for (int j = 0; j < nblocks; ++j) {
    const DclTemplateBlock &q = blocks[j];
    if (!(q.dst && ((uintptr_t)q.dst & 3) == 0 && q.src_col >= 0 && q.width >= 1 && q.dst_pitch >= q.width &&
          (long long)q.src_col + q.width <= row_floats)) {
      dcl_set_error("%s: invalid argument: block %d (dst, 0 <= src_col, 1 <= width <= dst_pitch, src_col + width <= row_floats)",
                    func, j);
      return DCL_EINVAL;
    }
  }
  return 0;
}
}  // namespace

#define DCL_TEMPLATE_CHECK_ARGS()                                                                                            \
  DCL_CHECK_ARG(cache && lut && cls && blocks && miss);                                                                      \
  DCL_CHECK_ARG((((uintptr_t)cache | (uintptr_t)lut | (uintptr_t)cls | (uintptr_t)miss) & 3) == 0);                          \
  DCL_CHECK_ARG(b >= 1 && n_tmp >= 1 && nblocks >= 1 && nblocks <= DCL_TEMPLATE_MAX_BLOCKS && lut_len >= 0);                 \
  DCL_CHECK_ARG(row_floats >= 1 && class_floats >= (int64_t)n_tmp * row_floats);                                             \
  if (check_blocks(__func__, blocks, nblocks, row_floats)) return DCL_EINVAL

DCL_API int dcl_template_rows(const float *cache, int64_t class_floats, int row_floats, int n_tmp, const int32_t *lut, int lut_len,
                              const int32_t *cls, int b, const DclTemplateBlock *blocks, int nblocks, int32_t *miss,
                              dclStream_t stream) {
  DCL_TEMPLATE_CHECK_ARGS();
  TemplateBlocks tb;
  tb.nblocks = nblocks;
  tb.vec_mask = 0;
  tb.unit0[0] = 0;
  const bool src_vec = ((uintptr_t)cache & 15) == 0 && (class_floats & 3) == 0 && (row_floats & 3) == 0;
  for (int j = 0; j < nblocks; ++j) {
    const DclTemplateBlock &q = blocks[j];
    const bool vec = src_vec && ((uintptr_t)q.dst & 15) == 0 && ((q.src_col | q.width) & 3) == 0 && (q.dst_pitch & 3) == 0;
    if (vec) tb.vec_mask |= 1u << j;
    tb.blk[j] = q;
    tb.unit0[j + 1] = tb.unit0[j] + (vec ? q.width >> 2 : q.width);
  }
  for (int j = nblocks; j < DCL_TEMPLATE_MAX_BLOCKS; ++j) {
    tb.blk[j] = blocks[nblocks - 1];
    tb.unit0[j + 1] = tb.unit0[nblocks];
  }
  // the grid follows the work -- b n_tmp rows of sum(width) floats, one unit a lane -- never the device
  const long long rows = (long long)b * n_tmp, total = rows * tb.unit0[nblocks];
  hipLaunchKernelGGL(k_template_rows, dim3(dcl_grid_1d(total, 256, 1 << 20)), dim3(256), 0, (hipStream_t)stream, cache,
                     (long long)class_floats, row_floats, n_tmp, lut, lut_len, cls, rows, tb, miss);
  DCL_LAUNCH_CHECK();
  return 0;
}

// the same contract in plain C++ on host pointers (what the tests compare the kernel with; no GPU call)
DCL_API int dcl_template_rows_host(const float *cache, int64_t class_floats, int row_floats, int n_tmp, const int32_t *lut,
                                   int lut_len, const int32_t *cls, int b, const DclTemplateBlock *blocks, int nblocks,
                                   int32_t *miss) {
  DCL_TEMPLATE_CHECK_ARGS();
  for (int i = 0; i < b; ++i) {
    const int slot = template_slot(lut, lut_len, cls[i]);
    if (slot < 0) *miss = 1;
    for (int r = 0; r < n_tmp; ++r)
      for (int j = 0; j < nblocks; ++j) {
        const DclTemplateBlock &q = blocks[j];
        float *dst = q.dst + ((size_t)i * n_tmp + r) * q.dst_pitch;
        const float *src = cache + (slot < 0 ? 0 : (size_t)slot * class_floats + (size_t)r * row_floats + q.src_col);
        for (int c = 0; c < q.width; ++c) dst[c] = slot >= 0 ? src[c] : 0.f;
      }
  }
  return 0;
}
