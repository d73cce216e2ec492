// crops_train.hip -- the front end of the TRAINING loader (YCBV/dataloader_train_YCBV.py:105-210) on the device.
//
// The training loader differs from the test loader in every data-dependent step: the box comes from the mask's own extent,
// one object per frame is drawn until one with enough valid pixels comes up, the centred cloud is re-posed with a jittered
// ground-truth pose BEFORE the grid filter, the filter is unconditional, and the labels are the jittered pose.
//
//   dcl_label_table         what the pick loop and get_bbox(mask_label) need of a frame, for every class at once: the number
//                           of pixels with label == c && depth != 0 (:128-131) and the row / column extent of label == c
//                           (:134,280-285).  k_label_table_fill writes the identities, k_label_table makes ONE pass over the
//                           pixels: a thread walks 8 consecutive pixels and keeps the current class's five integers in
//                           registers (a label image is long runs of one value), flushes them into its workgroup's table
//                           in LDS when the class changes, and the workgroup merges the classes it has seen into the
//                           frame's table with integer atomics.  Integer min / max / sum: the order does not matter
//   dcl_crop_points_posed   dcl_crop_points (the bodies of crops_body.h) with a per-crop source frame and camera, and the
//                           loader's re-pose between the centroid and the grid filter.  The pose row of a crop:
//
//       struct CropPoseRow (112 bytes, little endian)        who writes it: crops.py::CropBuilder.build_train, once per batch
//         double t_gt[3]   meta['poses'][:, 3, idx]           float64 until the centroid is subtracted (:136,159)
//         float  R0[9]     meta['poses'][:, 0:3, idx]         row major, rounded to float32 as torch.FloatTensor does (:169)
//         float  j[3]      the three random.uniform(-0.03, 0.03) draws, rounded to float32 (:172)
//         float  A[9]      aug_r = euler2mat(a1, a2, a3), rounded to float32 (:165-166)
//         float  pad
//
//                           after the centroid one lane forms t0 = f32(t_gt - f64(centroid)), t1 = t0 + j, R1 = R0 A
//                           (crop_pose_form) and writes the labels rot_gt = R1, trans_gt = t1; every centred point goes
//                           through crop_repose.  k_crop_keep_posed forms the same pose again from the same row and the
//                           stored centroid (the same function: the same bits) instead of reading 24 floats back.
//   dcl_crop_repose_host    crop_pose_form + crop_repose on the host: the twin the tests compare the kernels with.
#include "common.h"
#include "crops_body.h"

#include <climits>
#include <cstring>

namespace {

constexpr int kLtThreads = 256;
constexpr int kLtPerThread = 8;                 // consecutive pixels of a thread
constexpr int kLtMaxClasses = 256;
constexpr int kLtMaxBlocksPerFrame = 256;

bool lt_shape_ok(int n, int H, int W, int n_classes) {
  return n >= 0 && H >= 1 && W >= 1 && (long long)H * W < (1ll << 31) - 64 && n_classes >= 1 && n_classes <= kLtMaxClasses &&
         (long long)n * kLtMaxBlocksPerFrame < (1ll << 31) && (long long)n * n_classes * 5 < (1ll << 31);
}

__host__ __device__ inline int lt_blocks_per_frame(int H, int W) {
  const long long per = (long long)kLtThreads * kLtPerThread;
  const long long b = ((long long)H * W + per - 1) / per;
  return (int)(b < kLtMaxBlocksPerFrame ? b : kLtMaxBlocksPerFrame);
}

// {count, min row, max row, min col, max col} of an absent class
__global__ void k_label_table_fill(int rows, int32_t *__restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows) return;
  int32_t *o = out + (size_t)i * 5;
  o[0] = 0; o[1] = INT_MAX; o[2] = -1; o[3] = INT_MAX; o[4] = -1;
}

__global__ __launch_bounds__(kLtThreads) void k_label_table(const int32_t *__restrict__ label, const uint16_t *__restrict__ depth,
                                                            int H, int W, int n_classes, int bpf, int32_t *__restrict__ out) {
  __shared__ int s_tab[kLtMaxClasses * 5];
  const int t = threadIdx.x;
  const int frame = blockIdx.x / bpf, blk = blockIdx.x - frame * bpf;
  for (int i = t; i < n_classes; i += kLtThreads) {   // bound: n_classes <= 256: one round
    s_tab[i * 5] = 0; s_tab[i * 5 + 1] = INT_MAX; s_tab[i * 5 + 2] = -1; s_tab[i * 5 + 3] = INT_MAX; s_tab[i * 5 + 4] = -1;
  }
  __syncthreads();
  const int npix = H * W;
  const int32_t *L = label + (size_t)frame * npix;
  const uint16_t *D = depth + (size_t)frame * npix;
  int cur = -1, cnt = 0, r0 = INT_MAX, r1 = -1, c0 = INT_MAX, c1 = -1;
  auto flush = [&]() {
    if (cur >= 0) {                               // cur is -1 or a class id inside [0, n_classes): the only LDS address
      if (cnt) atomicAdd(&s_tab[cur * 5], cnt);
      atomicMin(&s_tab[cur * 5 + 1], r0); atomicMax(&s_tab[cur * 5 + 2], r1);
      atomicMin(&s_tab[cur * 5 + 3], c0); atomicMax(&s_tab[cur * 5 + 4], c1);
    }
  };
  // bound: ceil(H * W / (2048 * workgroups of the frame)) rounds
  for (long long first = ((long long)blk * kLtThreads + t) * kLtPerThread; first < npix; first += (long long)bpf * kLtThreads * kLtPerThread) {
    int r = (int)(first / W), c = (int)(first - (long long)r * W);
#pragma unroll
    for (int u = 0; u < kLtPerThread; ++u) {
      const long long p = first + u;
      if (p < npix) {
        const int32_t v = L[p];
        if ((uint32_t)v < (uint32_t)n_classes) {
          if (v != cur) {
            flush();
            cur = v; cnt = 0; r0 = INT_MAX; r1 = -1; c0 = INT_MAX; c1 = -1;
          }
          cnt += D[p] != 0;
          r0 = min(r0, r); r1 = max(r1, r); c0 = min(c0, c); c1 = max(c1, c);
        }
      }
      if (++c == W) { c = 0; ++r; }
    }
  }
  flush();
  __syncthreads();
  int32_t *o = out + (size_t)frame * n_classes * 5;
  for (int i = t; i < n_classes; i += kLtThreads) {
    if (s_tab[i * 5 + 2] < 0) continue;           // this workgroup has not seen the class
    if (s_tab[i * 5]) atomicAdd(o + i * 5, s_tab[i * 5]);
    atomicMin(o + i * 5 + 1, s_tab[i * 5 + 1]); atomicMax(o + i * 5 + 2, s_tab[i * 5 + 2]);
    atomicMin(o + i * 5 + 3, s_tab[i * 5 + 3]); atomicMax(o + i * 5 + 4, s_tab[i * 5 + 4]);
  }
}

// ---- the three crop kernels with a per-crop source and the re-pose
__global__ __launch_bounds__(kCropThreads) void k_crop_mask_posed(
    const uint16_t *__restrict__ depth, const int32_t *__restrict__ label, const uint8_t *__restrict__ rgb, int n_frames, int H,
    int W, int rgb_channels, const int32_t *__restrict__ src /* (n,6) rmin,rmax,cmin,cmax,class,frame */,
    const float *__restrict__ cams /* (n,5) cx,cy,fx,fy,scale */, double mean_r, double mean_g, double mean_b, int cap, int nch,
    float *__restrict__ raw_xyz, float *__restrict__ raw_rgb, int32_t *__restrict__ ws) {
  const int inst = blockIdx.x / nch, chunk = blockIdx.x - inst * nch;
  const int32_t *s = src + (size_t)inst * 6;
  CropBox box = {s[0], s[1], s[2], s[3], s[4]};
  int frame = s[5];
  if (frame < 0 || frame >= n_frames) {           // no such frame: an empty crop (the host copy was checked by the call)
    frame = 0;
    box.rmax = box.rmin;
  }
  const float *cm = cams + (size_t)inst * 5;
  const CropCam cam = {cm[0], cm[1], cm[2], cm[3], cm[4], 1.0f};
  const size_t npix = (size_t)H * W;
  crop_mask_body(depth + frame * npix, label + frame * npix, rgb + frame * npix * rgb_channels, H, W, rgb_channels, box, cam,
                 mean_r, mean_g, mean_b, cap, chunk, raw_xyz + (size_t)inst * cap * 3, raw_rgb + (size_t)inst * cap * 3,
                 ws + (size_t)inst * crop_ws_ints(cap) + 4);
}

__global__ __launch_bounds__(kCropThreads) void k_crop_centroid_posed(int cap, int nch, float hx, float hy, float hz, int min_valid,
                                                                      const float *__restrict__ raw_xyz,
                                                                      float *__restrict__ centroid, int32_t *__restrict__ counts,
                                                                      int32_t *__restrict__ ws, const CropPoseRow *__restrict__ pose,
                                                                      float *__restrict__ rot_gt, float *__restrict__ trans_gt) {
  crop_centroid_body<kPoseF32>(blockIdx.x, cap, nch, hx, hy, hz, min_valid, 1, raw_xyz, centroid, counts, ws, pose, rot_gt, trans_gt);
}

__global__ __launch_bounds__(kCropThreads) void k_crop_keep_posed(int cap, int nch, float hx, float hy, float hz,
                                                                  const float *__restrict__ raw_xyz, const float *__restrict__ raw_rgb,
                                                                  const float *__restrict__ centroid, float *__restrict__ out_xyz,
                                                                  float *__restrict__ out_rgb, const int32_t *__restrict__ ws,
                                                                  const CropPoseRow *__restrict__ pose) {
  const int inst = blockIdx.x / nch, chunk = blockIdx.x - inst * nch;
  crop_keep_body<kPoseF32>(inst, chunk, cap, nch, hx, hy, hz, raw_xyz, raw_rgb, centroid, out_xyz, out_rgb, ws, pose);
}

}  // namespace

DCL_API int dcl_label_table(const int32_t *label, const uint16_t *depth, int n, int H, int W, int n_classes, int32_t *out,
                            dclStream_t stream) {
  DCL_CHECK_ARG(lt_shape_ok(n, H, W, n_classes));
  if (n == 0) return 0;
  DCL_CHECK_ARG(label && depth && out);
  hipStream_t s = (hipStream_t)stream;
  const int rows = n * n_classes, bpf = lt_blocks_per_frame(H, W);
  hipLaunchKernelGGL(k_label_table_fill, dim3(dcl_div_up(rows, 256)), dim3(256), 0, s, rows, out);
  hipLaunchKernelGGL(k_label_table, dim3(n * bpf), dim3(kLtThreads), 0, s, label, depth, H, W, n_classes, bpf, out);
  DCL_LAUNCH_CHECK();
  return 0;
}

DCL_API int dcl_label_table_host(const int32_t *label, const uint16_t *depth, int n, int H, int W, int n_classes, int32_t *out) {
  DCL_CHECK_ARG(lt_shape_ok(n, H, W, n_classes));
  if (n == 0) return 0;
  DCL_CHECK_ARG(label && depth && out);
  for (int f = 0; f < n; ++f) {
    int32_t *o = out + (size_t)f * n_classes * 5;
    for (int c = 0; c < n_classes; ++c) { o[c * 5] = 0; o[c * 5 + 1] = INT_MAX; o[c * 5 + 2] = -1; o[c * 5 + 3] = INT_MAX; o[c * 5 + 4] = -1; }
    const int32_t *L = label + (size_t)f * H * W;
    const uint16_t *D = depth + (size_t)f * H * W;
    for (int r = 0; r < H; ++r)
      for (int c = 0; c < W; ++c) {
        const int32_t v = L[(size_t)r * W + c];
        if (v < 0 || v >= n_classes) continue;
        int32_t *e = o + (size_t)v * 5;
        e[0] += D[(size_t)r * W + c] != 0;
        if (r < e[1]) e[1] = r;
        if (r > e[2]) e[2] = r;
        if (c < e[3]) e[3] = c;
        if (c > e[4]) e[4] = c;
      }
  }
  return 0;
}

DCL_API int dcl_crop_points_posed(const uint16_t *depth, const int32_t *label, const uint8_t *rgb, int n_frames, int H, int W,
                                  int rgb_channels, int n_inst, const int32_t *frame_idx_host, const int32_t *src,
                                  const float *cams, const void *pose, const double *rgb_mean_host,
                                  const float *half_extent_host, int min_valid, int cap, float *raw_xyz, float *raw_rgb,
                                  float *out_xyz, float *out_rgb, float *centroid, int32_t *counts, float *rot_gt,
                                  float *trans_gt, int32_t *ws, dclStream_t stream) {
  DCL_CHECK_ARG(n_inst >= 0 && n_frames >= 0 && H > 0 && W > 0 && (long long)H * W < (1ll << 31) - 64 && rgb_channels >= 3 &&
                cap > 0 && cap <= 1024 * kCropChunk && min_valid >= 0);
  if (n_inst == 0) return 0;
  DCL_CHECK_ARG(depth && label && rgb && frame_idx_host && src && cams && pose && rgb_mean_host && half_extent_host && raw_xyz &&
                raw_rgb && out_xyz && out_rgb && centroid && counts && rot_gt && trans_gt && ws);
  for (int i = 0; i < n_inst; ++i) DCL_CHECK_ARG(frame_idx_host[i] >= 0 && frame_idx_host[i] < n_frames);
  const int nch = dcl_div_up(cap, kCropChunk);
  DCL_CHECK_ARG((long long)n_inst * nch < (1ll << 31));
  hipStream_t s = (hipStream_t)stream;
  const CropPoseRow *rows = static_cast<const CropPoseRow *>(pose);
  dcl_internal_zero_words(ws, (long long)n_inst * crop_ws_ints(cap), s);       // chunk statuses: 0 = not yet published
  hipLaunchKernelGGL(k_crop_mask_posed, dim3(n_inst * nch), dim3(kCropThreads), 0, s, depth, label, rgb, n_frames, H, W,
                     rgb_channels, src, cams, rgb_mean_host[0], rgb_mean_host[1], rgb_mean_host[2], cap, nch, raw_xyz, raw_rgb, ws);
  hipLaunchKernelGGL(k_crop_centroid_posed, dim3(n_inst), dim3(kCropThreads), 0, s, cap, nch, half_extent_host[0],
                     half_extent_host[1], half_extent_host[2], min_valid, raw_xyz, centroid, counts, ws, rows, rot_gt, trans_gt);
  hipLaunchKernelGGL(k_crop_keep_posed, dim3(n_inst * nch), dim3(kCropThreads), 0, s, cap, nch, half_extent_host[0],
                     half_extent_host[1], half_extent_host[2], raw_xyz, raw_rgb, centroid, out_xyz, out_rgb, ws, rows);
  DCL_LAUNCH_CHECK();
  return 0;
}

DCL_API int dcl_crop_repose_host(const float *points, const void *pose_row, const float *centroid, int n, float *out_xyz,
                                 float *out_R1, float *out_t1) {
  DCL_CHECK_ARG(n >= 0 && pose_row && centroid && out_R1 && out_t1 && (n == 0 || (points && out_xyz)));
  CropPoseRow row;
  memcpy(&row, pose_row, sizeof(row));            // the caller's bytes need not be 8-byte aligned
  CropPose P;
  crop_pose_form(row, centroid, P);
  for (int k = 0; k < 9; ++k) out_R1[k] = P.R1[k];
  for (int k = 0; k < 3; ++k) out_t1[k] = P.t1[k];
  for (int i = 0; i < n; ++i) {
    float x = points[(size_t)i * 3], y = points[(size_t)i * 3 + 1], z = points[(size_t)i * 3 + 2];
    crop_repose(P, x, y, z);
    out_xyz[(size_t)i * 3] = x; out_xyz[(size_t)i * 3 + 1] = y; out_xyz[(size_t)i * 3 + 2] = z;
  }
  return 0;
}
