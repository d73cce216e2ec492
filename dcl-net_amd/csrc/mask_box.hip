// mask_box.hip -- the loaders' `get_bbox(mask_to_bbox(mask_label, padding))` on the device: from a label image to the crop
// rows dcl_crop_points takes, without the mask leaving HBM (semantics, the tie rule and the box arithmetic: mask_box.h).
//
// The mask is labelled by RUNS of set pixels per row, not by pixels: a segmentation mask of 480 x 640 has a few hundred
// runs, the worst case (every other pixel of every row) H * ceil(W / 2) = 153 600, which is what the workspace is sized for.
// Six launches, integer arithmetic and integer atomics only, no workgroup waits for another, nothing is read back:
//   k_mb_bits     label == value -> one bit per pixel, rows padded to whole 32-bit words (a wave's ballot is two words)
//   k_mb_rows     one workgroup per image: runs per row (a run starts where `word & ~(word << 1 | carry)` has a bit; the
//                 carry is bit 31 of the word before it in the row), then the rows' exclusive offsets (workgroup scan,
//                 the total carried from one block of rows to the next)
//   k_mb_place    one lane per word: the runs that START in it get consecutive slots behind the row's offset and the starts
//                 of the words in front of it; a run's end is the first clear bit behind its start, in this word or a later
//                 one.  Slot order = raster order of the runs' first pixels.  Every run starts as its own component
//   k_mb_union    one lane per run: the runs of the row above that touch it (a.start <= b.end + 1 && b.start <= a.end + 1:
//                 8-connectivity) are found by bisection and united with it -- lock-free union-find whose links always
//                 point to the LOWER slot, so a component's root is the run holding its first pixel in raster order,
//                 whatever order the lanes were served in
//   k_mb_stats    one lane per run: min / max column, max row and pixel count into its root (atomicMin / Max / Add)
//   k_mb_select   one workgroup per image: the winner among the roots (mb_better), the component count, the ten integers
// After k_mb_union the partition is a function of the mask alone, and min / max / integer sums do not depend on their order:
// the same bits on every call.
#include "common.h"
#include "mask_box.h"

#include <vector>

namespace {

constexpr int kMbBlock = 256;
constexpr int kMbMaxBlocks = 4096;

// per image: bit words, H + 1 row offsets, then per run slot: first column, last column, row, parent, and at a root the
// component's min column, max column, max row and pixel count
struct MbWs {
  uint32_t *bits;
  int32_t *rowoff, *rs, *re, *rrow, *parent, *xmin, *xmax, *ymax, *npix;
};

__host__ __device__ inline long long mb_ws_ints(int H, int W) {
  return (long long)H * mb_words_per_row(W) + (H + 1) + 8 * mb_run_cap(H, W);
}

__host__ __device__ inline MbWs mb_ws_of(int32_t *ws, int img, int H, int W) {
  int32_t *p = ws + (size_t)img * mb_ws_ints(H, W);
  const long long cap = mb_run_cap(H, W);
  MbWs w;
  w.bits = reinterpret_cast<uint32_t *>(p); p += (size_t)H * mb_words_per_row(W);
  w.rowoff = p; p += H + 1;
  w.rs = p; p += cap;
  w.re = p; p += cap;
  w.rrow = p; p += cap;
  w.parent = p; p += cap;
  w.xmin = p; p += cap;
  w.xmax = p; p += cap;
  w.ymax = p; p += cap;
  w.npix = p;
  return w;
}

bool mb_shape_ok(int n, int H, int W) {
  // pixel and run indices are int32; the words of all images are counted in 64 bits
  return n >= 0 && H >= 1 && W >= 1 && (long long)H * W < (1ll << 31) - 64 &&
         (n == 0 || mb_ws_ints(H, W) < (1ll << 62) / (4ll * n));
}

// ---- 1. bits: lane l of a wave looks at column 64 * k + l of its (image, row); the ballot is the row's words 2k and 2k + 1
__global__ __launch_bounds__(kMbBlock) void k_mb_bits(const int32_t *__restrict__ label, int n, int H, int W, int32_t value,
                                                      int32_t *__restrict__ ws) {
  const int lane = threadIdx.x & 63;
  const int wpr = mb_words_per_row(W), cpr = (W + 63) / 64;                // words / 64-column chunks per row
  const long long items = (long long)n * H * cpr;
  const long long wave0 = ((long long)blockIdx.x * kMbBlock + threadIdx.x) >> 6, nwaves = ((long long)gridDim.x * kMbBlock) >> 6;
  // bound: ceil(n * H * ceil(W / 64) / waves in the grid)
  for (long long it = wave0; it < items; it += nwaves) {
    const int k = (int)(it % cpr);
    const long long ir = it / cpr;
    const int row = (int)(ir % H), img = (int)(ir / H);
    const int col = 64 * k + lane;
    const bool set = col < W && label[((size_t)img * H + row) * W + col] == value;
    const unsigned long long b = __ballot(set);
    uint32_t *bits = mb_ws_of(ws, img, H, W).bits + (size_t)row * wpr;
    if (lane == 0) bits[2 * k] = (uint32_t)b;
    if (lane == 1 && 2 * k + 1 < wpr) bits[2 * k + 1] = (uint32_t)(b >> 32);
  }
}

__device__ __forceinline__ uint32_t mb_starts(uint32_t m, uint32_t prev) { return m & ~((m << 1) | (prev >> 31)); }

// ---- 2. runs per row and the rows' exclusive offsets; rowoff[H] = the image's run count
__global__ __launch_bounds__(kMbBlock) void k_mb_rows(int H, int W, int32_t *__restrict__ ws) {
  __shared__ int s_wave[kMbBlock / 64];
  __shared__ int s_carry;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const MbWs w = mb_ws_of(ws, blockIdx.x, H, W);
  const int wpr = mb_words_per_row(W);
  if (t == 0) s_carry = 0;
  __syncthreads();
  // bound: ceil(H / 256) blocks of rows
  for (int r0 = 0; r0 < H; r0 += kMbBlock) {
    const int row = r0 + t;
    int cnt = 0;
    if (row < H) {
      uint32_t prev = 0;
      for (int k = 0; k < wpr; ++k) {                                      // bound: ceil(W / 32)
        const uint32_t m = w.bits[(size_t)row * wpr + k];
        cnt += __popc(mb_starts(m, prev));
        prev = m;
      }
    }
    int incl = cnt;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int up = __shfl_up(incl, d, 64);
      if (lane >= d) incl += up;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    int base = s_carry, total = 0;
#pragma unroll
    for (int v = 0; v < kMbBlock / 64; ++v) {
      if (v < wave) base += s_wave[v];
      total += s_wave[v];
    }
    if (row < H) w.rowoff[row] = base + incl - cnt;
    __syncthreads();                                                       // everybody has read s_carry and s_wave
    if (t == 0) s_carry += total;
    __syncthreads();
  }
  if (t == 0) w.rowoff[H] = s_carry;
}

// ---- 3. the runs that start in a word, in raster order
__global__ __launch_bounds__(kMbBlock) void k_mb_place(int n, int H, int W, int32_t *__restrict__ ws) {
  const int wpr = mb_words_per_row(W);
  const long long items = (long long)n * H * wpr, step = (long long)gridDim.x * kMbBlock;
  // bound: ceil(n * H * ceil(W / 32) / threads in the grid)
  for (long long it = (long long)blockIdx.x * kMbBlock + threadIdx.x; it < items; it += step) {
    const int k = (int)(it % wpr);
    const long long ir = it / wpr;
    const int row = (int)(ir % H), img = (int)(ir / H);
    const MbWs w = mb_ws_of(ws, img, H, W);
    const uint32_t *bits = w.bits + (size_t)row * wpr;
    const uint32_t m = bits[k];
    uint32_t s = mb_starts(m, k > 0 ? bits[k - 1] : 0u);
    if (!s) continue;
    int slot = w.rowoff[row];
    uint32_t prev = 0;
    for (int j = 0; j < k; ++j) {                                          // bound: ceil(W / 32)
      const uint32_t mj = bits[j];
      slot += __popc(mb_starts(mj, prev));
      prev = mj;
    }
    while (s) {                                                            // bound: 16 starts in a word
      const int b = __builtin_ctz(s);
      s &= s - 1;
      const uint32_t clear = ~(m >> b);                                    // bit i: pixel b + i is clear (or beyond the word)
      int len = clear ? __builtin_ctz(clear) : 32;
      if (b + len == 32) {                                                 // runs on into the next words
        for (int j = k + 1; j < wpr; ++j) {                                // bound: ceil(W / 32)
          const uint32_t mj = bits[j];
          if (mj != 0xffffffffu) { len += __builtin_ctz(~mj); break; }
          len += 32;
        }
      }
      const int x0 = 32 * k + b, x1 = x0 + len - 1;
      w.rs[slot] = x0; w.re[slot] = x1; w.rrow[slot] = row; w.parent[slot] = slot;
      w.xmin[slot] = x0; w.xmax[slot] = x1; w.ymax[slot] = row; w.npix[slot] = len;
      ++slot;
    }
  }
}

// root of x.  Links always point to a lower slot, so the walk is strictly descending: at most `x` steps (< run count).  On
// the way every visited slot is pointed at its grandparent (path halving): a slot that has a parent never becomes a root
// again, and any ancestor is a valid parent, so these plain stores cannot undo a link made by the compare-and-swap below.
__device__ __forceinline__ int mb_find(int32_t *parent, int x) {
  int p = __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  while (p != x) {
    const int g = __hip_atomic_load(parent + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (g != p) __hip_atomic_store(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    x = p;
    p = g;
  }
  return x;
}

// lock-free union: link the higher root under the lower one.  The compare-and-swap fails only when another lane has just
// linked that root (that lane made progress); the roots then found are lower, so there are fewer retries than runs.
__device__ __forceinline__ void mb_union(int32_t *parent, int a, int b) {
  for (;;) {
    a = mb_find(parent, a);
    b = mb_find(parent, b);
    if (a == b) return;
    const int hi = a > b ? a : b, lo = a > b ? b : a;
    int expect = hi;
    if (__hip_atomic_compare_exchange_strong(parent + hi, &expect, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
      return;
    a = hi; b = lo;
  }
}

// image and slot of a flat item over n * cap run slots; false where the slot holds no run
__device__ __forceinline__ bool mb_slot(long long it, long long cap, int H, int W, int32_t *ws, MbWs &w, int &slot) {
  const int img = (int)(it / cap);
  slot = (int)(it - (long long)img * cap);
  w = mb_ws_of(ws, img, H, W);
  return slot < w.rowoff[H];
}

// ---- 4. unite every run with the runs of the row above that touch it
__global__ __launch_bounds__(kMbBlock) void k_mb_union(int n, int H, int W, int32_t *__restrict__ ws) {
  const long long cap = mb_run_cap(H, W), items = (long long)n * cap, step = (long long)gridDim.x * kMbBlock;
  // bound: ceil(n * H * ceil(W / 2) / threads in the grid)
  for (long long it = (long long)blockIdx.x * kMbBlock + threadIdx.x; it < items; it += step) {
    MbWs w;
    int i;
    if (!mb_slot(it, cap, H, W, ws, w, i)) continue;
    const int row = w.rrow[i];
    if (row == 0) continue;
    const int a0 = w.rs[i], a1 = w.re[i];
    int lo = w.rowoff[row - 1];
    const int end = w.rowoff[row];
    int hi = end;
    while (lo < hi) {                                                      // first run above with end >= a0 - 1; bound: 32 halvings
      const int mid = lo + ((hi - lo) >> 1);
      if (w.re[mid] < a0 - 1) lo = mid + 1; else hi = mid;
    }
    for (int j = lo; j < end && w.rs[j] <= a1 + 1; ++j) mb_union(w.parent, i, j);   // bound: runs of the row above
  }
}

// ---- 5. every run that is not a root adds itself to its root
__global__ __launch_bounds__(kMbBlock) void k_mb_stats(int n, int H, int W, int32_t *__restrict__ ws) {
  const long long cap = mb_run_cap(H, W), items = (long long)n * cap, step = (long long)gridDim.x * kMbBlock;
  // bound: ceil(n * H * ceil(W / 2) / threads in the grid)
  for (long long it = (long long)blockIdx.x * kMbBlock + threadIdx.x; it < items; it += step) {
    MbWs w;
    int i;
    if (!mb_slot(it, cap, H, W, ws, w, i)) continue;
    int r = i;
    for (int p = w.parent[r]; p != r; p = w.parent[r]) r = p;               // bound: strictly descending, < run count
    if (r == i) continue;
    atomicMin(w.xmin + r, w.rs[i]);
    atomicMax(w.xmax + r, w.re[i]);
    atomicMax(w.ymax + r, w.rrow[i]);
    atomicAdd(w.npix + r, w.re[i] - w.rs[i] + 1);
  }
}

// ---- 6. the winner among the roots
__global__ __launch_bounds__(kMbBlock) void k_mb_select(int H, int W, int padding, int32_t *__restrict__ ws,
                                                        int32_t *__restrict__ out) {
  __shared__ MbComp s_best[kMbBlock];
  __shared__ int s_cnt[kMbBlock];
  const int t = threadIdx.x;
  const MbWs w = mb_ws_of(ws, blockIdx.x, H, W);
  const int runs = w.rowoff[H];
  MbComp best = mb_none();
  int cnt = 0;
  for (int i = t; i < runs; i += kMbBlock) {                               // bound: ceil(run count / 256)
    if (w.parent[i] != i) continue;
    const MbComp c = mb_comp(w.xmin[i], w.xmax[i], w.rrow[i], w.ymax[i], w.npix[i], w.rs[i], W);
    if (mb_better(c, best)) best = c;
    ++cnt;
  }
  s_best[t] = best;
  s_cnt[t] = cnt;
  __syncthreads();
  for (int d = kMbBlock / 2; d >= 1; d >>= 1) {                            // bound: 8 halvings
    if (t < d) {
      if (mb_better(s_best[t + d], s_best[t])) s_best[t] = s_best[t + d];
      s_cnt[t] += s_cnt[t + d];
    }
    __syncthreads();
  }
  if (t == 0) mb_finish(s_best[0], s_cnt[0], padding, H, W, out + (size_t)blockIdx.x * 10);
}

}  // namespace

DCL_API int dcl_mask_box_ws_bytes(int n, int H, int W, int64_t *bytes_host) {
  DCL_CHECK_ARG(mb_shape_ok(n, H, W) && bytes_host);
  *bytes_host = 4ll * n * mb_ws_ints(H, W);
  return 0;
}

DCL_API int dcl_mask_box(const int32_t *label, int n, int H, int W, int32_t value, int padding, int32_t *out, void *ws,
                         int64_t ws_bytes, dclStream_t stream) {
  DCL_CHECK_ARG(mb_shape_ok(n, H, W) && padding >= 0 && padding < (1 << 30));
  if (n == 0) return 0;
  DCL_CHECK_ARG(label && out && ws);
  if (ws_bytes < 4ll * n * mb_ws_ints(H, W)) {
    dcl_set_error("%s: invalid argument: ws_bytes %lld < %lld", __func__, (long long)ws_bytes, 4ll * n * mb_ws_ints(H, W));
    return DCL_EINVAL;
  }
  hipStream_t s = (hipStream_t)stream;
  int32_t *w = static_cast<int32_t *>(ws);
  const long long cap = mb_run_cap(H, W);
  const int g_bits = dcl_grid_1d((long long)n * H * ((W + 63) / 64) * 64, kMbBlock, kMbMaxBlocks);
  const int g_words = dcl_grid_1d((long long)n * H * mb_words_per_row(W), kMbBlock, kMbMaxBlocks);
  const int g_runs = dcl_grid_1d((long long)n * cap, kMbBlock, kMbMaxBlocks);
  hipLaunchKernelGGL(k_mb_bits, dim3(g_bits), dim3(kMbBlock), 0, s, label, n, H, W, value, w);
  hipLaunchKernelGGL(k_mb_rows, dim3(n), dim3(kMbBlock), 0, s, H, W, w);
  hipLaunchKernelGGL(k_mb_place, dim3(g_words), dim3(kMbBlock), 0, s, n, H, W, w);
  hipLaunchKernelGGL(k_mb_union, dim3(g_runs), dim3(kMbBlock), 0, s, n, H, W, w);
  hipLaunchKernelGGL(k_mb_stats, dim3(g_runs), dim3(kMbBlock), 0, s, n, H, W, w);
  hipLaunchKernelGGL(k_mb_select, dim3(n), dim3(kMbBlock), 0, s, H, W, padding, w, out);
  DCL_LAUNCH_CHECK();
  return 0;
}

// The host twin: the same semantics by the plainest route -- runs from a pixel scan, a sequential union-find with the same
// "lower slot is the root" rule, then mb_better / mb_finish.  Host memory only; no GPU call.
DCL_API int dcl_mask_box_host(const int32_t *label, int n, int H, int W, int32_t value, int padding, int32_t *out) {
  DCL_CHECK_ARG(mb_shape_ok(n, H, W) && padding >= 0 && padding < (1 << 30));
  if (n == 0) return 0;
  DCL_CHECK_ARG(label && out);
  std::vector<int> rs, re, rrow, parent, rowoff(H + 1);
  for (int img = 0; img < n; ++img) {
    const int32_t *L = label + (size_t)img * H * W;
    rs.clear(); re.clear(); rrow.clear();
    for (int r = 0; r < H; ++r) {
      rowoff[r] = (int)rs.size();
      for (int c = 0; c < W;) {
        if (L[(size_t)r * W + c] != value) { ++c; continue; }
        int e = c;
        while (e + 1 < W && L[(size_t)r * W + e + 1] == value) ++e;
        rs.push_back(c); re.push_back(e); rrow.push_back(r);
        c = e + 1;
      }
    }
    const int runs = (int)rs.size();
    rowoff[H] = runs;
    parent.resize(runs);
    for (int i = 0; i < runs; ++i) parent[i] = i;
    auto find = [&](int x) {
      while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; }
      return x;
    };
    for (int r = 1; r < H; ++r) {
      int j0 = rowoff[r - 1];                                              // both rows are sorted: the first candidate only moves right
      for (int i = rowoff[r]; i < rowoff[r + 1]; ++i) {
        while (j0 < rowoff[r] && re[j0] + 1 < rs[i]) ++j0;
        for (int j = j0; j < rowoff[r] && rs[j] <= re[i] + 1; ++j) {
          const int a = find(i), b = find(j);
          if (a != b) parent[a > b ? a : b] = a > b ? b : a;
        }
      }
    }
    std::vector<MbComp> comp(runs);
    for (int i = 0; i < runs; ++i) comp[i] = mb_comp(rs[i], re[i], rrow[i], rrow[i], re[i] - rs[i] + 1, rs[i], W);
    for (int i = 0; i < runs; ++i) {
      const int r = find(i);
      if (r == i) continue;
      MbComp &c = comp[r];
      c = mb_comp(std::min(c.x0, rs[i]), std::max(c.x1, re[i]), c.y0, std::max(c.y1, rrow[i]), c.npix + re[i] - rs[i] + 1, rs[r], W);
    }
    MbComp best = mb_none();
    int ncomp = 0;
    for (int i = 0; i < runs; ++i) {
      if (parent[i] != i) continue;
      ++ncomp;
      if (mb_better(comp[i], best)) best = comp[i];
    }
    mb_finish(best, ncomp, padding, H, W, out + (size_t)img * 10);
  }
  return 0;
}
