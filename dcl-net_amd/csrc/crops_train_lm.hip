// crops_train_lm.hip -- the front end of the LineMOD TRAINING loader (LM/dataloader_train_LM.py:125-222,293-348) on the device.
//
// What this loader adds to the YCB-V one (crops_train.hip):
//
//   dcl_mask_extent          what `occlude_with_another_object` reduces of an object mask (n,H,W,3) u8: the row / column extent
//                            of channel 0 (:301-306) and the sum of all bytes (:343).  k_mask_extent_fill writes the identities,
//                            k_mask_extent makes one pass: a thread walks 4 consecutive pixels at a time, the workgroup
//                            reduces through shuffles and LDS, one lane merges into the frame's row with integer atomics.
//   dcl_occlude_paste        the compositing (:335-342) into working copies, and the loader's `if mask.sum() >= 20` (:343-346)
//                            WITHOUT the host: k_occlude_paste copies every pixel, composites the target rectangle and adds what
//                            it removed from the mask to the frame's accumulator (64-bit integer atomics, one per workgroup);
//                            k_occlude_finish -- a second launch, so the accumulator is complete -- restores the rectangle from
//                            the originals where original - removed < 20, writes {committed, remaining} and counts the pixels
//                            of the crop box with label' == 255 && depth' != 0 (`len(choose)`, :157).  The slicing (:311-334,
//                            with the loader's x-limit and row trims) is integer work on two extents: crops.py::lm_paste_plan
//                            does it on the host and hands over one 16-integer row per frame (PastePlan below).
//   dcl_crop_points_posed64  dcl_crop_points_posed with the re-pose in FLOAT64 (crops_body.h: kPoseF64) and LineMOD's camera
//                            rows {cx, cy, fx, fy, scale, post_div}.  The pose row of a crop:
//
//       struct CropPoseRow64 (192 bytes, little endian)      who writes it: crops.py::CropBuilder.build_train_lm, once per batch
//         double t_gt[3]   cam_t_m2c / 1000.0                 (:154)
//         double R0[9]     cam_R_m2c, row major               (:153)
//         double j[3]      the three random.uniform(-0.03, 0.03) draws (:186)
//         double A[9]      aug_r = euler2mat(a1, a2, a3)      (:183)
//
//   dcl_mask_extent_host, dcl_occlude_paste_host, dcl_crop_repose64_host: the twins in plain C++ (no GPU call); the float64
//   re-pose compiles the same __host__ __device__ routines as the kernels.
#include "common.h"
#include "crops_body.h"

#include <climits>
#include <cstring>

namespace {

constexpr int kLmThreads = 256;
constexpr int kLmPerThread = 4;                 // consecutive pixels of a thread
constexpr int kLmMaxBlocksPerFrame = 1024;
constexpr long long kLmCommitSum = 20;          // `if mask.sum() >= 20` (:343)

bool lm_shape_ok(int n, int H, int W) {
  return n >= 0 && H >= 1 && W >= 1 && (long long)H * W < (1ll << 31) - 64 && (long long)n * kLmMaxBlocksPerFrame < (1ll << 31);
}

__host__ __device__ inline int lm_blocks_per_frame(int H, int W) {
  const long long per = (long long)kLmThreads * kLmPerThread;
  const long long b = ((long long)H * W + per - 1) / per;
  return (int)(b < kLmMaxBlocksPerFrame ? b : kLmMaxBlocksPerFrame);
}

__host__ __device__ inline int lm_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the int64 behind columns 4:6 of an extent row (a row is 24 bytes, the pair starts at byte 16: 8-byte aligned)
__host__ __device__ inline long long *extent_sum(int32_t *row) { return reinterpret_cast<long long *>(row + 4); }
__host__ __device__ inline const long long *extent_sum(const int32_t *row) { return reinterpret_cast<const long long *>(row + 4); }

// ---- sum over the workgroup of one unsigned count per thread (kLmThreads threads); the total is returned to thread 0
__device__ __forceinline__ unsigned long long lm_block_sum(unsigned long long v, unsigned long long *s_part /* [4] */) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  __syncthreads();                              // s_part may still be read from the previous call
  if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = v;
  __syncthreads();
  unsigned long long total = 0;
#pragma unroll
  for (int w = 0; w < kLmThreads / 64; ++w) total += s_part[w];
  return total;
}

// ------------------------------------------------------------------------------------------------------------ mask extent
__global__ void k_mask_extent_fill(int n, int32_t *__restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int32_t *o = out + (size_t)i * 6;
  o[0] = INT_MAX; o[1] = -1; o[2] = INT_MAX; o[3] = -1; o[4] = 0; o[5] = 0;
}

__global__ __launch_bounds__(kLmThreads) void k_mask_extent(const uint8_t *__restrict__ mask, int H, int W, int bpf,
                                                            int32_t *__restrict__ out) {
  __shared__ unsigned long long s_part[kLmThreads / 64];
  __shared__ int s_ext[4];
  const int t = threadIdx.x;
  const int frame = blockIdx.x / bpf, blk = blockIdx.x - frame * bpf;
  if (t == 0) { s_ext[0] = INT_MAX; s_ext[1] = -1; s_ext[2] = INT_MAX; s_ext[3] = -1; }
  __syncthreads();
  const int npix = H * W;
  const uint8_t *M = mask + (size_t)frame * npix * 3;
  int r0 = INT_MAX, r1 = -1, c0 = INT_MAX, c1 = -1;
  unsigned sum = 0;                             // at most ceil(npix / (bpf * 1024)) * 4 * 765 < 2^32 (npix < 2^31)
  // bound: ceil(H * W / (1024 * workgroups of the frame)) rounds
  for (long long first = ((long long)blk * kLmThreads + t) * kLmPerThread; first < npix; first += (long long)bpf * kLmThreads * kLmPerThread) {
    int r = (int)(first / W), c = (int)(first - (long long)r * W);
#pragma unroll
    for (int u = 0; u < kLmPerThread; ++u) {
      const long long p = first + u;
      if (p < npix) {
        const uint8_t *px = M + (size_t)p * 3;
        const unsigned m0 = px[0];
        sum += m0 + px[1] + px[2];
        if (m0) { r0 = min(r0, r); r1 = max(r1, r); c0 = min(c0, c); c1 = max(c1, c); }
      }
      if (++c == W) { c = 0; ++r; }
    }
  }
  if (r1 >= 0) { atomicMin(&s_ext[0], r0); atomicMax(&s_ext[1], r1); atomicMin(&s_ext[2], c0); atomicMax(&s_ext[3], c1); }
  const unsigned long long total = lm_block_sum(sum, s_part);   // its barriers also order s_ext
  if (t == 0) {
    int32_t *o = out + (size_t)frame * 6;
    if (s_ext[1] >= 0) { atomicMin(o, s_ext[0]); atomicMax(o + 1, s_ext[1]); atomicMin(o + 2, s_ext[2]); atomicMax(o + 3, s_ext[3]); }
    if (total) atomicAdd(reinterpret_cast<unsigned long long *>(o + 4), total);
  }
}

// ------------------------------------------------------------------------------------------------------------ occlusion paste
// a plan row as the kernels use it: every field clamped so that no pixel outside either frame can be named
struct PastePlan { int enabled, other, py0, px0, ty0, tx0, th, tw, rep_y, rep_x, rmin, rmax, cmin, cmax; };

__host__ __device__ inline PastePlan paste_plan_load(const int32_t *row, int H, int W, int n_other) {
  PastePlan p;
  p.enabled = row[0] != 0 && n_other > 0;
  p.other = lm_clamp(row[1], 0, n_other > 0 ? n_other - 1 : 0);
  p.py0 = lm_clamp(row[2], 0, H - 1); p.px0 = lm_clamp(row[3], 0, W - 1);
  p.ty0 = lm_clamp(row[6], 0, H); p.tx0 = lm_clamp(row[7], 0, W);
  p.th = p.enabled ? lm_clamp(row[8], 0, H - p.ty0) : 0;
  p.tw = p.enabled ? lm_clamp(row[9], 0, W - p.tx0) : 0;
  p.rep_y = row[10] != 0; p.rep_x = row[11] != 0;
  p.rmin = lm_clamp(row[12], 0, H); p.rmax = lm_clamp(row[13], p.rmin, H);
  p.cmin = lm_clamp(row[14], 0, W); p.cmax = lm_clamp(row[15], p.cmin, W);
  return p;
}

// the host's check of the host copy of a row: what the clamps above would otherwise hide
bool paste_plan_ok(const int32_t *row, int H, int W, int n_other) {
  if (row[12] < 0 || row[12] > H || row[13] < 0 || row[13] > H || row[14] < 0 || row[14] > W || row[15] < 0 || row[15] > W) return false;
  if (row[0] == 0) return true;
  const long long other = row[1], py0 = row[2], px0 = row[3], ph = row[4], pw = row[5], ty0 = row[6], tx0 = row[7], th = row[8], tw = row[9];
  if (other < 0 || other >= n_other) return false;
  if (ph < 0 || pw < 0 || th < 0 || tw < 0) return false;
  if (py0 < 0 || px0 < 0 || py0 + ph > H || px0 + pw > W) return false;
  if (ty0 < 0 || tx0 < 0 || ty0 + th > H || tx0 + tw > W) return false;
  if (!(row[10] ? ph == 1 : ph == th) || !(row[11] ? pw == 1 : pw == tw)) return false;   // numpy's broadcast of the patch
  return true;
}

// is pixel (r, c) inside the target rectangle, and which occluder pixel lands on it (flat index inside a frame)
__host__ __device__ inline bool paste_source(const PastePlan &p, int r, int c, int H, int W, size_t &q) {
  const int dy = r - p.ty0, dx = c - p.tx0;
  if (dy < 0 || dy >= p.th || dx < 0 || dx >= p.tw) return false;
  const int sy = lm_clamp(p.py0 + (p.rep_y ? 0 : dy), 0, H - 1), sx = lm_clamp(p.px0 + (p.rep_x ? 0 : dx), 0, W - 1);
  q = (size_t)sy * W + sx;
  return true;
}

struct PastePixel { uint8_t rgb[3]; uint16_t depth; int32_t label; unsigned removed; };

// :335-342 for one pixel of the rectangle: `x *= (om == 0); other[om == 0] = 0; x += other` is a select per channel
__host__ __device__ inline void paste_pixel(const uint8_t *own_rgb, uint16_t own_depth, const uint8_t *own_mask,
                                            const uint8_t *o_rgb, uint16_t o_depth, const uint8_t *o_mask, PastePixel &out) {
  out.removed = 0;
  for (int k = 0; k < 3; ++k) {
    out.rgb[k] = o_mask[k] == 0 ? own_rgb[k] : o_rgb[k];
    out.removed += o_mask[k] == 0 ? 0u : (unsigned)own_mask[k];
  }
  out.depth = o_mask[0] == 0 ? own_depth : o_depth;
  out.label = o_mask[0] == 0 ? (int32_t)own_mask[0] : 0;
}

__global__ __launch_bounds__(kLmThreads) void k_occlude_paste(
    const uint8_t *__restrict__ rgb, const uint16_t *__restrict__ depth, const uint8_t *__restrict__ mask, int H, int W, int C,
    const uint8_t *__restrict__ other_rgb, const uint16_t *__restrict__ other_depth, const uint8_t *__restrict__ other_mask,
    int n_other, const int32_t *__restrict__ plan, int bpf, uint8_t *__restrict__ out_rgb, uint16_t *__restrict__ out_depth,
    int32_t *__restrict__ out_label, long long *__restrict__ info) {
  __shared__ unsigned long long s_part[kLmThreads / 64];
  const int t = threadIdx.x;
  const int frame = blockIdx.x / bpf, blk = blockIdx.x - frame * bpf;
  const PastePlan P = paste_plan_load(plan + (size_t)frame * DCL_PASTE_PLAN_INTS, H, W, n_other);
  const int npix = H * W;
  const size_t fbase = (size_t)frame * npix, obase = (size_t)P.other * npix;
  unsigned removed = 0;                         // at most rounds * 4 * 765 < 2^32, as in k_mask_extent
  for (long long first = ((long long)blk * kLmThreads + t) * kLmPerThread; first < npix; first += (long long)bpf * kLmThreads * kLmPerThread) {
    int r = (int)(first / W), c = (int)(first - (long long)r * W);
#pragma unroll
    for (int u = 0; u < kLmPerThread; ++u) {
      const long long p = first + u;
      if (p < npix) {
        const size_t pix = fbase + (size_t)p;
        const uint8_t *px = rgb + pix * C;
        PastePixel o;
        o.rgb[0] = px[0]; o.rgb[1] = px[1]; o.rgb[2] = px[2];
        o.depth = depth[pix];
        o.label = mask[pix * 3];
        size_t q;
        if (paste_source(P, r, c, H, W, q)) {
          q += obase;
          paste_pixel(px, o.depth, mask + pix * 3, other_rgb + q * 3, other_depth[q], other_mask + q * 3, o);
          removed += o.removed;
        }
        uint8_t *dst = out_rgb + pix * C;
        dst[0] = o.rgb[0]; dst[1] = o.rgb[1]; dst[2] = o.rgb[2];
        for (int k = 3; k < C; ++k) dst[k] = px[k];
        out_depth[pix] = o.depth;
        out_label[pix] = o.label;
      }
      if (++c == W) { c = 0; ++r; }
    }
  }
  const unsigned long long total = lm_block_sum(removed, s_part);
  if (t == 0 && total) atomicAdd(reinterpret_cast<unsigned long long *>(info + (size_t)frame * 4 + 3), total);
}

// second launch: info[frame][3] is complete.  Restores the rectangle where the composite is not kept, counts the box
__global__ __launch_bounds__(kLmThreads) void k_occlude_finish(
    const uint8_t *__restrict__ rgb, const uint16_t *__restrict__ depth, const uint8_t *__restrict__ mask, int H, int W, int C,
    int n_other, const int32_t *__restrict__ plan, const int32_t *__restrict__ extent, int bpf, uint8_t *__restrict__ out_rgb,
    uint16_t *__restrict__ out_depth, int32_t *__restrict__ out_label, long long *__restrict__ info) {
  __shared__ unsigned long long s_part[kLmThreads / 64];
  const int t = threadIdx.x;
  const int frame = blockIdx.x / bpf, blk = blockIdx.x - frame * bpf;
  const PastePlan P = paste_plan_load(plan + (size_t)frame * DCL_PASTE_PLAN_INTS, H, W, n_other);
  long long *inf = info + (size_t)frame * 4;
  const long long remaining = *extent_sum(extent + (size_t)frame * 6) - inf[3];
  const bool commit = P.enabled && remaining >= kLmCommitSum, restore = P.enabled && !commit;
  if (blk == 0 && t == 0) { inf[0] = commit ? 1 : 0; inf[1] = remaining; }
  const int npix = H * W;
  const size_t fbase = (size_t)frame * npix;
  unsigned valid = 0;
  for (long long first = ((long long)blk * kLmThreads + t) * kLmPerThread; first < npix; first += (long long)bpf * kLmThreads * kLmPerThread) {
    int r = (int)(first / W), c = (int)(first - (long long)r * W);
#pragma unroll
    for (int u = 0; u < kLmPerThread; ++u) {
      const long long p = first + u;
      if (p < npix) {
        const size_t pix = fbase + (size_t)p;
        size_t q;
        const bool undo = restore && paste_source(P, r, c, H, W, q);
        const bool in_box = r >= P.rmin && r < P.rmax && c >= P.cmin && c < P.cmax;
        if (undo) {
          const uint8_t *px = rgb + pix * C;
          uint8_t *dst = out_rgb + pix * C;
          dst[0] = px[0]; dst[1] = px[1]; dst[2] = px[2];
          out_depth[pix] = depth[pix];
          out_label[pix] = mask[pix * 3];
        }
        if (in_box) {
          const int32_t l = undo ? (int32_t)mask[pix * 3] : out_label[pix];
          const uint16_t d = undo ? depth[pix] : out_depth[pix];
          valid += l == 255 && d != 0;
        }
      }
      if (++c == W) { c = 0; ++r; }
    }
  }
  const unsigned long long total = lm_block_sum(valid, s_part);
  if (t == 0 && total) atomicAdd(reinterpret_cast<unsigned long long *>(inf + 2), total);
}

bool paste_args_ok(int n, int H, int W, int C, int n_other) {
  return lm_shape_ok(n, H, W) && C >= 3 && n_other >= 0 && (long long)n_other * H * W < (1ll << 40) && (long long)n * H * W < (1ll << 40);
}

// ---- the three crop kernels with a per-crop source, LineMOD's camera rows and the float64 re-pose
__global__ __launch_bounds__(kCropThreads) void k_crop_mask_posed64(
    const uint16_t *__restrict__ depth, const int32_t *__restrict__ label, const uint8_t *__restrict__ rgb, int n_frames, int H,
    int W, int rgb_channels, const int32_t *__restrict__ src /* (n,6) rmin,rmax,cmin,cmax,class,frame */,
    const float *__restrict__ cams /* (n,6) cx,cy,fx,fy,scale,post_div */, double mean_r, double mean_g, double mean_b, int cap,
    int nch, float *__restrict__ raw_xyz, float *__restrict__ raw_rgb, int32_t *__restrict__ ws) {
  const int inst = blockIdx.x / nch, chunk = blockIdx.x - inst * nch;
  const int32_t *s = src + (size_t)inst * 6;
  CropBox box = {s[0], s[1], s[2], s[3], s[4]};
  int frame = s[5];
  if (frame < 0 || frame >= n_frames) {           // no such frame: an empty crop (the host copy was checked by the call)
    frame = 0;
    box.rmax = box.rmin;
  }
  const float *cm = cams + (size_t)inst * 6;
  const CropCam cam = {cm[0], cm[1], cm[2], cm[3], cm[4], cm[5]};
  const size_t npix = (size_t)H * W;
  crop_mask_body(depth + frame * npix, label + frame * npix, rgb + frame * npix * rgb_channels, H, W, rgb_channels, box, cam,
                 mean_r, mean_g, mean_b, cap, chunk, raw_xyz + (size_t)inst * cap * 3, raw_rgb + (size_t)inst * cap * 3,
                 ws + (size_t)inst * crop_ws_ints(cap) + 4);
}

__global__ __launch_bounds__(kCropThreads) void k_crop_centroid_posed64(int cap, int nch, double hx, double hy, double hz,
                                                                        int min_valid, const float *__restrict__ raw_xyz,
                                                                        float *__restrict__ centroid, int32_t *__restrict__ counts,
                                                                        int32_t *__restrict__ ws,
                                                                        const CropPoseRow64 *__restrict__ pose,
                                                                        float *__restrict__ rot_gt, float *__restrict__ trans_gt) {
  crop_centroid_body<kPoseF64>(blockIdx.x, cap, nch, hx, hy, hz, min_valid, 1, raw_xyz, centroid, counts, ws, pose, rot_gt, trans_gt);
}

__global__ __launch_bounds__(kCropThreads) void k_crop_keep_posed64(int cap, int nch, double hx, double hy, double hz,
                                                                    const float *__restrict__ raw_xyz,
                                                                    const float *__restrict__ raw_rgb,
                                                                    const float *__restrict__ centroid, float *__restrict__ out_xyz,
                                                                    float *__restrict__ out_rgb, const int32_t *__restrict__ ws,
                                                                    const CropPoseRow64 *__restrict__ pose) {
  const int inst = blockIdx.x / nch, chunk = blockIdx.x - inst * nch;
  crop_keep_body<kPoseF64>(inst, chunk, cap, nch, hx, hy, hz, raw_xyz, raw_rgb, centroid, out_xyz, out_rgb, ws, pose);
}

}  // namespace

DCL_API int dcl_mask_extent(const uint8_t *mask, int n, int H, int W, int32_t *out, dclStream_t stream) {
  DCL_CHECK_ARG(lm_shape_ok(n, H, W));
  if (n == 0) return 0;
  DCL_CHECK_ARG(mask && out);
  hipStream_t s = (hipStream_t)stream;
  const int bpf = lm_blocks_per_frame(H, W);
  hipLaunchKernelGGL(k_mask_extent_fill, dim3(dcl_div_up(n, 256)), dim3(256), 0, s, n, out);
  hipLaunchKernelGGL(k_mask_extent, dim3(n * bpf), dim3(kLmThreads), 0, s, mask, H, W, bpf, out);
  DCL_LAUNCH_CHECK();
  return 0;
}

DCL_API int dcl_mask_extent_host(const uint8_t *mask, int n, int H, int W, int32_t *out) {
  DCL_CHECK_ARG(lm_shape_ok(n, H, W));
  if (n == 0) return 0;
  DCL_CHECK_ARG(mask && out);
  for (int f = 0; f < n; ++f) {
    int32_t *o = out + (size_t)f * 6;
    o[0] = INT_MAX; o[1] = -1; o[2] = INT_MAX; o[3] = -1;
    long long sum = 0;
    const uint8_t *M = mask + (size_t)f * H * W * 3;
    for (int r = 0; r < H; ++r)
      for (int c = 0; c < W; ++c) {
        const uint8_t *px = M + ((size_t)r * W + c) * 3;
        sum += (long long)px[0] + px[1] + px[2];
        if (px[0]) {
          if (r < o[0]) o[0] = r;
          if (r > o[1]) o[1] = r;
          if (c < o[2]) o[2] = c;
          if (c > o[3]) o[3] = c;
        }
      }
    memcpy(o + 4, &sum, sizeof(sum));
  }
  return 0;
}

DCL_API int dcl_occlude_paste(const uint8_t *rgb, const uint16_t *depth, const uint8_t *mask, int n, int H, int W,
                              int rgb_channels, const uint8_t *other_rgb, const uint16_t *other_depth, const uint8_t *other_mask,
                              int n_other, const int32_t *plan_host, const int32_t *plan, const int32_t *extent, uint8_t *out_rgb,
                              uint16_t *out_depth, int32_t *out_label, int64_t *info, dclStream_t stream) {
  DCL_CHECK_ARG(paste_args_ok(n, H, W, rgb_channels, n_other));
  if (n == 0) return 0;
  DCL_CHECK_ARG(rgb && depth && mask && plan_host && plan && extent && out_rgb && out_depth && out_label && info);
  DCL_CHECK_ARG(n_other == 0 || (other_rgb && other_depth && other_mask));
  for (int f = 0; f < n; ++f) DCL_CHECK_ARG(paste_plan_ok(plan_host + (size_t)f * DCL_PASTE_PLAN_INTS, H, W, n_other));
  hipStream_t s = (hipStream_t)stream;
  const int bpf = lm_blocks_per_frame(H, W);
  long long *inf = reinterpret_cast<long long *>(info);
  dcl_internal_zero_words(info, (long long)n * 8, s);          // n_box_valid and the removed sums: accumulated by atomics
  hipLaunchKernelGGL(k_occlude_paste, dim3(n * bpf), dim3(kLmThreads), 0, s, rgb, depth, mask, H, W, rgb_channels, other_rgb,
                     other_depth, other_mask, n_other, plan, bpf, out_rgb, out_depth, out_label, inf);
  hipLaunchKernelGGL(k_occlude_finish, dim3(n * bpf), dim3(kLmThreads), 0, s, rgb, depth, mask, H, W, rgb_channels, n_other, plan,
                     extent, bpf, out_rgb, out_depth, out_label, inf);
  DCL_LAUNCH_CHECK();
  return 0;
}

DCL_API int dcl_occlude_paste_host(const uint8_t *rgb, const uint16_t *depth, const uint8_t *mask, int n, int H, int W,
                                   int rgb_channels, const uint8_t *other_rgb, const uint16_t *other_depth,
                                   const uint8_t *other_mask, int n_other, const int32_t *plan, const int32_t *extent,
                                   uint8_t *out_rgb, uint16_t *out_depth, int32_t *out_label, int64_t *info) {
  DCL_CHECK_ARG(paste_args_ok(n, H, W, rgb_channels, n_other));
  if (n == 0) return 0;
  DCL_CHECK_ARG(rgb && depth && mask && plan && extent && out_rgb && out_depth && out_label && info);
  DCL_CHECK_ARG(n_other == 0 || (other_rgb && other_depth && other_mask));
  for (int f = 0; f < n; ++f) DCL_CHECK_ARG(paste_plan_ok(plan + (size_t)f * DCL_PASTE_PLAN_INTS, H, W, n_other));
  const int C = rgb_channels;
  const size_t npix = (size_t)H * W;
  for (int f = 0; f < n; ++f) {
    const PastePlan P = paste_plan_load(plan + (size_t)f * DCL_PASTE_PLAN_INTS, H, W, n_other);
    const size_t fbase = (size_t)f * npix, obase = (size_t)P.other * npix;
    long long removed = 0;
    for (int r = 0; r < H; ++r)
      for (int c = 0; c < W; ++c) {
        const size_t pix = fbase + (size_t)r * W + c;
        const uint8_t *px = rgb + pix * C;
        PastePixel o;
        o.rgb[0] = px[0]; o.rgb[1] = px[1]; o.rgb[2] = px[2];
        o.depth = depth[pix];
        o.label = mask[pix * 3];
        size_t q;
        if (paste_source(P, r, c, H, W, q)) {
          q += obase;
          paste_pixel(px, o.depth, mask + pix * 3, other_rgb + q * 3, other_depth[q], other_mask + q * 3, o);
          removed += o.removed;
        }
        uint8_t *dst = out_rgb + pix * C;
        for (int k = 0; k < C; ++k) dst[k] = k < 3 ? o.rgb[k] : px[k];
        out_depth[pix] = o.depth;
        out_label[pix] = o.label;
      }
    long long orig;
    memcpy(&orig, extent + (size_t)f * 6 + 4, sizeof(orig));
    const long long remaining = orig - removed;
    const bool commit = P.enabled && remaining >= kLmCommitSum;
    if (P.enabled && !commit)
      for (int r = P.ty0; r < P.ty0 + P.th; ++r)
        for (int c = P.tx0; c < P.tx0 + P.tw; ++c) {
          const size_t pix = fbase + (size_t)r * W + c;
          for (int k = 0; k < 3; ++k) out_rgb[pix * C + k] = rgb[pix * C + k];
          out_depth[pix] = depth[pix];
          out_label[pix] = mask[pix * 3];
        }
    long long valid = 0;
    for (int r = P.rmin; r < P.rmax; ++r)
      for (int c = P.cmin; c < P.cmax; ++c) {
        const size_t pix = fbase + (size_t)r * W + c;
        valid += out_label[pix] == 255 && out_depth[pix] != 0;
      }
    info[(size_t)f * 4] = commit ? 1 : 0; info[(size_t)f * 4 + 1] = remaining; info[(size_t)f * 4 + 2] = valid;
    info[(size_t)f * 4 + 3] = removed;
  }
  return 0;
}

DCL_API int dcl_crop_points_posed64(const uint16_t *depth, const int32_t *label, const uint8_t *rgb, int n_frames, int H, int W,
                                    int rgb_channels, int n_inst, const int32_t *frame_idx_host, const int32_t *src,
                                    const float *cams, const void *pose, const double *rgb_mean_host,
                                    const double *half_extent_host, int min_valid, int cap, float *raw_xyz, float *raw_rgb,
                                    float *out_xyz, float *out_rgb, float *centroid, int32_t *counts, float *rot_gt,
                                    float *trans_gt, int32_t *ws, dclStream_t stream) {
  DCL_CHECK_ARG(n_inst >= 0 && n_frames >= 0 && H > 0 && W > 0 && (long long)H * W < (1ll << 31) - 64 && rgb_channels >= 3 &&
                cap > 0 && cap <= 1024 * kCropChunk && min_valid >= 0);
  if (n_inst == 0) return 0;
  DCL_CHECK_ARG(depth && label && rgb && frame_idx_host && src && cams && pose && rgb_mean_host && half_extent_host && raw_xyz &&
                raw_rgb && out_xyz && out_rgb && centroid && counts && rot_gt && trans_gt && ws);
  DCL_CHECK_ARG(((uintptr_t)pose & 7) == 0);                    // rows of doubles
  for (int i = 0; i < n_inst; ++i) DCL_CHECK_ARG(frame_idx_host[i] >= 0 && frame_idx_host[i] < n_frames);
  const int nch = dcl_div_up(cap, kCropChunk);
  DCL_CHECK_ARG((long long)n_inst * nch < (1ll << 31));
  hipStream_t s = (hipStream_t)stream;
  const CropPoseRow64 *rows = static_cast<const CropPoseRow64 *>(pose);
  dcl_internal_zero_words(ws, (long long)n_inst * crop_ws_ints(cap), s);       // chunk statuses: 0 = not yet published
  hipLaunchKernelGGL(k_crop_mask_posed64, dim3(n_inst * nch), dim3(kCropThreads), 0, s, depth, label, rgb, n_frames, H, W,
                     rgb_channels, src, cams, rgb_mean_host[0], rgb_mean_host[1], rgb_mean_host[2], cap, nch, raw_xyz, raw_rgb, ws);
  hipLaunchKernelGGL(k_crop_centroid_posed64, dim3(n_inst), dim3(kCropThreads), 0, s, cap, nch, half_extent_host[0],
                     half_extent_host[1], half_extent_host[2], min_valid, raw_xyz, centroid, counts, ws, rows, rot_gt, trans_gt);
  hipLaunchKernelGGL(k_crop_keep_posed64, dim3(n_inst * nch), dim3(kCropThreads), 0, s, cap, nch, half_extent_host[0],
                     half_extent_host[1], half_extent_host[2], raw_xyz, raw_rgb, centroid, out_xyz, out_rgb, ws, rows);
  DCL_LAUNCH_CHECK();
  return 0;
}

DCL_API int dcl_crop_repose64_host(const float *points, const void *pose_row, const float *centroid, int n,
                                   const double *half_extent, float *out_xyz, uint8_t *inside, float *out_R1, float *out_t1) {
  DCL_CHECK_ARG(n >= 0 && pose_row && centroid && out_R1 && out_t1 && (n == 0 || (points && out_xyz)));
  DCL_CHECK_ARG((half_extent != nullptr) == (inside != nullptr) || n == 0);
  CropPoseRow64 row;
  memcpy(&row, pose_row, sizeof(row));            // the caller's bytes need not be 8-byte aligned
  CropPose64 P;
  crop_pose_form(row, centroid, P);
  for (int k = 0; k < 9; ++k) out_R1[k] = (float)P.R1[k];
  for (int k = 0; k < 3; ++k) out_t1[k] = (float)P.t1[k];
  for (int i = 0; i < n; ++i) {
    double x = points[(size_t)i * 3], y = points[(size_t)i * 3 + 1], z = points[(size_t)i * 3 + 2];
    crop_repose(P, x, y, z);
    out_xyz[(size_t)i * 3] = (float)x; out_xyz[(size_t)i * 3 + 1] = (float)y; out_xyz[(size_t)i * 3 + 2] = (float)z;
    if (inside) inside[i] = fabs(x) < half_extent[0] && fabs(y) < half_extent[1] && fabs(z) < half_extent[2];
  }
  return 0;
}
