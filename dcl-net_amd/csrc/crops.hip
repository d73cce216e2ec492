// crops.hip -- the crop builder that runs in front of DCL_Net.forward, on the device.
//
// The reference builds every object crop of an image on the CPU inside the DataLoader workers
// (YCBV/dataloader_test_YCBV.py:124-183; LineMOD's loader has the same arithmetic): mask the detection box, back-project
// the depth pixels, subtract the centroid, drop points outside the voxel grid, sample N of them, emit the (N,7) feature
// rows and the integer voxel coordinates that voxelize_idx consumes.  Here the data-dependent part runs on the device in
// the reference's ORDER (ascending flat pixel index inside the box) and with the reference's float32 / float64 arithmetic
// step by step, so that the results are bit-identical:
//
//   dcl_crop_points   box mask -> ordered compaction -> back-projection -> sequential float32 centroid (numpy's
//                     mean(axis=0) is a row-order running sum, verified in tests) -> box filter -> ordered compaction
//   [host: np.random.choice(count, N) -- the sampling indices stay the caller's, it owns the RNG stream]
//   dcl_crop_sample   gather the sampled points, write feats rows [1,r,g,b,x,y,z] and (batch,x,y,z) voxel coordinates
//
// dcl_crop_points is three launches (round 5; until then ONE workgroup per instance walked its box chunk by chunk, 159 us for
// the six instances of a frame on a 256-CU chip):
//   k_crop_mask      one workgroup per 4096-pixel chunk of a box: mask, count, ordered compaction through a decoupled
//                    look-back over the instance's earlier chunks (lower workgroup ids: running or done), back-projection
//   k_crop_centroid  one workgroup per instance: the only part that is sequential by contract -- the row-order float32 sum
//                    (three lanes, one coordinate each, LDS-fed) -- then, all threads, the in-grid count per 4096-row chunk and
//                    the chunks' exclusive output offsets
//   k_crop_keep      one workgroup per 4096-row chunk: filter, ordered compaction at the chunk's offset, centring
// dcl_crop_points_frames is the same three launches over stacked frames: k_crop_mask_frames takes the crop's frame from its
// src row, the other two kernels are the ones above (the multi-frame eval builders, crops.py: CropBuilder.build_frames).
#include "common.h"
#include "crops_body.h"

// The bodies of the three kernels live in crops_body.h: the training loader's entry (crops_train.hip) runs the same code with
// a per-crop source and the loader's re-pose in front of the grid filter.

namespace {

// ---- 1. masked pixels of the box in flat order (dataloader_test_YCBV.py:128-133), back-projection (:147-154)
__global__ __launch_bounds__(kCropThreads) void k_crop_mask(
    const uint16_t *__restrict__ depth, const int32_t *__restrict__ label, const uint8_t *__restrict__ rgb, int H, int W,
    int rgb_channels, const int32_t *__restrict__ boxes /* (n,4) rmin,rmax,cmin,cmax */, const int32_t *__restrict__ obj_ids,
    CropCam cam, double mean_r, double mean_g, double mean_b, int cap, int nch, float *__restrict__ raw_xyz,
    float *__restrict__ raw_rgb, int32_t *__restrict__ ws) {
  const int inst = blockIdx.x / nch, chunk = blockIdx.x - inst * nch;
  const CropBox box = {boxes[inst * 4], boxes[inst * 4 + 1], boxes[inst * 4 + 2], boxes[inst * 4 + 3], obj_ids[inst]};
  crop_mask_body(depth, label, rgb, H, W, rgb_channels, box, cam, mean_r, mean_g, mean_b, cap, chunk,
                 raw_xyz + (size_t)inst * cap * 3, raw_rgb + (size_t)inst * cap * 3, ws + (size_t)inst * crop_ws_ints(cap) + 4);
}

// k_crop_mask over stacked frames (dcl_crop_points_frames): the crop's box, class AND frame come from its src row; the
// centroid and keep kernels below never see a frame (they read the crop's own scratch), so they serve both entries
__global__ __launch_bounds__(kCropThreads) void k_crop_mask_frames(
    const uint16_t *__restrict__ depth, const int32_t *__restrict__ label, const uint8_t *__restrict__ rgb, int n_frames, int H,
    int W, int rgb_channels, const int32_t *__restrict__ src /* (n,6) rmin,rmax,cmin,cmax,class,frame */, CropCam cam,
    double mean_r, double mean_g, double mean_b, int cap, int nch, float *__restrict__ raw_xyz, float *__restrict__ raw_rgb,
    int32_t *__restrict__ ws) {
  const int inst = blockIdx.x / nch, chunk = blockIdx.x - inst * nch;
  const int32_t *s = src + (size_t)inst * 6;
  CropBox box = {s[0], s[1], s[2], s[3], s[4]};
  int frame = s[5];
  if (frame < 0 || frame >= n_frames) {           // no such frame: an empty crop (the host copy was checked by the call)
    frame = 0;
    box.rmax = box.rmin;
  }
  const size_t npix = (size_t)H * W;
  crop_mask_body(depth + frame * npix, label + frame * npix, rgb + frame * npix * rgb_channels, H, W, rgb_channels, box, cam,
                 mean_r, mean_g, mean_b, cap, chunk, raw_xyz + (size_t)inst * cap * 3, raw_rgb + (size_t)inst * cap * 3,
                 ws + (size_t)inst * crop_ws_ints(cap) + 4);
}

// ---- 2. centroid = np.mean(cloud, axis=0): running float32 sum in row order, one division (:156); in-grid counts (:160-163)
__global__ __launch_bounds__(kCropThreads) void k_crop_centroid(int cap, int nch, float hx, float hy, float hz, int min_valid,
                                                                int always_filter, const float *__restrict__ raw_xyz,
                                                                float *__restrict__ centroid, int32_t *__restrict__ counts,
                                                                int32_t *__restrict__ ws) {
  crop_centroid_body<kPoseNone>(blockIdx.x, cap, nch, hx, hy, hz, min_valid, always_filter, raw_xyz, centroid, counts, ws, nullptr,
                            nullptr, nullptr);
}

// ---- 3. keep the points inside the grid (in order), centred (:160-165)
__global__ __launch_bounds__(kCropThreads) void k_crop_keep(int cap, int nch, float hx, float hy, float hz,
                                                            const float *__restrict__ raw_xyz, const float *__restrict__ raw_rgb,
                                                            const float *__restrict__ centroid, float *__restrict__ out_xyz,
                                                            float *__restrict__ out_rgb, const int32_t *__restrict__ ws) {
  const int inst = blockIdx.x / nch, chunk = blockIdx.x - inst * nch;
  crop_keep_body<kPoseNone>(inst, chunk, cap, nch, hx, hy, hz, raw_xyz, raw_rgb, centroid, out_xyz, out_rgb, ws, nullptr);
}

// feats row [1, r, g, b, x, y, z] and voxel coordinate row [batch, ix, iy, iz] of every sampled point (:170-176,186-190):
//   voxel = trunc((xyz + half_extent0) / unit) in float32, clamped to [0, limit-1] first when the crop had <= 32 points
//   inside the grid.  sample_idx == nullptr: identity (template clouds, :179-182).
__global__ void k_crop_sample(int n_inst, int npoint, int cap, const float *__restrict__ xyz, const float *__restrict__ rgb,
                              const int64_t *__restrict__ sample_idx, const int32_t *__restrict__ counts, int min_valid,
                              float half0, float ux, float uy, float uz, float limit, float *__restrict__ feats,
                              int64_t *__restrict__ coords) {
  const long long total = (long long)n_inst * npoint;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    const int inst = (int)(e / npoint);
    const long long i = sample_idx ? sample_idx[e] : (e - (long long)inst * npoint);
    const float *p = xyz + ((size_t)inst * cap + i) * 3, *c = rgb + ((size_t)inst * cap + i) * 3;
    crop_sample_row(p, c, counts && counts[inst * 3 + 1] <= min_valid, inst, half0, ux, uy, uz, limit, feats + e * 7,
                    coords + e * 4);
  }
}

}  // namespace

DCL_API int dcl_crop_points_ws_ints(int n_inst, int cap, int64_t *ints_host) {
  DCL_CHECK_ARG(n_inst >= 0 && cap > 0 && ints_host);
  *ints_host = (int64_t)n_inst * crop_ws_ints(cap);
  return 0;
}

DCL_API int dcl_crop_points(const uint16_t *depth, const int32_t *label, const uint8_t *rgb, int H, int W, int rgb_channels,
                            int n_inst, const int32_t *boxes, const int32_t *obj_ids, const float *cam_host /*6*/,
                            const double *rgb_mean_host /*3*/, const float *half_extent_host /*3*/, int min_valid,
                            int always_filter, int cap,
                            float *raw_xyz, float *raw_rgb, float *out_xyz, float *out_rgb, float *centroid,
                            int32_t *counts, int32_t *ws, dclStream_t stream) {
  DCL_CHECK_ARG(n_inst >= 0 && H > 0 && W > 0 && rgb_channels >= 3 && cap > 0 && cap <= 1024 * kCropChunk);
  if (n_inst == 0) return 0;
  DCL_CHECK_ARG(depth && label && rgb && boxes && obj_ids && cam_host && rgb_mean_host && half_extent_host && raw_xyz &&
                raw_rgb && out_xyz && out_rgb && centroid && counts && ws);
  const CropCam cam = {cam_host[0], cam_host[1], cam_host[2], cam_host[3], cam_host[4], cam_host[5]};
  DCL_CHECK_ARG(cam.scale != 0.0f && cam.post_div != 0.0f);
  const int nch = dcl_div_up(cap, kCropChunk);
  DCL_CHECK_ARG((long long)n_inst * nch < (1ll << 31));
  hipStream_t s = (hipStream_t)stream;
  dcl_internal_zero_words(ws, (long long)n_inst * crop_ws_ints(cap), s);       // chunk statuses: 0 = not yet published
  hipLaunchKernelGGL(k_crop_mask, dim3(n_inst * nch), dim3(kCropThreads), 0, s, depth, label, rgb, H, W, rgb_channels, boxes,
                     obj_ids, cam, rgb_mean_host[0], rgb_mean_host[1], rgb_mean_host[2], cap, nch, raw_xyz, raw_rgb, ws);
  hipLaunchKernelGGL(k_crop_centroid, dim3(n_inst), dim3(kCropThreads), 0, s, cap, nch, half_extent_host[0], half_extent_host[1],
                     half_extent_host[2], min_valid, always_filter, raw_xyz, centroid, counts, ws);
  hipLaunchKernelGGL(k_crop_keep, dim3(n_inst * nch), dim3(kCropThreads), 0, s, cap, nch, half_extent_host[0], half_extent_host[1],
                     half_extent_host[2], raw_xyz, raw_rgb, centroid, out_xyz, out_rgb, ws);
  DCL_LAUNCH_CHECK();
  return 0;
}

DCL_API int dcl_crop_points_frames(const uint16_t *depth, const int32_t *label, const uint8_t *rgb, int n_frames, int H, int W,
                                   int rgb_channels, int n_inst, const int32_t *frame_idx_host, const int32_t *src,
                                   const float *cam_host /*6*/, const double *rgb_mean_host /*3*/,
                                   const float *half_extent_host /*3*/, int min_valid, int always_filter, int cap,
                                   float *raw_xyz, float *raw_rgb, float *out_xyz, float *out_rgb, float *centroid,
                                   int32_t *counts, int32_t *ws, dclStream_t stream) {
  DCL_CHECK_ARG(n_inst >= 0 && n_frames >= 0 && H > 0 && W > 0 && (long long)H * W < (1ll << 31) - 64 && rgb_channels >= 3 &&
                cap > 0 && cap <= 1024 * kCropChunk);
  if (n_inst == 0) return 0;
  DCL_CHECK_ARG(depth && label && rgb && frame_idx_host && src && cam_host && rgb_mean_host && half_extent_host && raw_xyz &&
                raw_rgb && out_xyz && out_rgb && centroid && counts && ws);
  for (int i = 0; i < n_inst; ++i) DCL_CHECK_ARG(frame_idx_host[i] >= 0 && frame_idx_host[i] < n_frames);
  const CropCam cam = {cam_host[0], cam_host[1], cam_host[2], cam_host[3], cam_host[4], cam_host[5]};
  DCL_CHECK_ARG(cam.scale != 0.0f && cam.post_div != 0.0f);
  const int nch = dcl_div_up(cap, kCropChunk);
  DCL_CHECK_ARG((long long)n_inst * nch < (1ll << 31));
  hipStream_t s = (hipStream_t)stream;
  dcl_internal_zero_words(ws, (long long)n_inst * crop_ws_ints(cap), s);       // chunk statuses: 0 = not yet published
  hipLaunchKernelGGL(k_crop_mask_frames, dim3(n_inst * nch), dim3(kCropThreads), 0, s, depth, label, rgb, n_frames, H, W,
                     rgb_channels, src, cam, rgb_mean_host[0], rgb_mean_host[1], rgb_mean_host[2], cap, nch, raw_xyz, raw_rgb, ws);
  hipLaunchKernelGGL(k_crop_centroid, dim3(n_inst), dim3(kCropThreads), 0, s, cap, nch, half_extent_host[0], half_extent_host[1],
                     half_extent_host[2], min_valid, always_filter, raw_xyz, centroid, counts, ws);
  hipLaunchKernelGGL(k_crop_keep, dim3(n_inst * nch), dim3(kCropThreads), 0, s, cap, nch, half_extent_host[0], half_extent_host[1],
                     half_extent_host[2], raw_xyz, raw_rgb, centroid, out_xyz, out_rgb, ws);
  DCL_LAUNCH_CHECK();
  return 0;
}

DCL_API int dcl_crop_sample(int n_inst, int npoint, int cap, const float *xyz, const float *rgb, const int64_t *sample_idx,
                            const int32_t *counts, int min_valid, float half_extent0, const float *unit_host /*3*/,
                            int voxel_limit, float *feats, int64_t *coords, dclStream_t stream) {
  DCL_CHECK_ARG(n_inst >= 0 && npoint >= 0 && cap > 0 && voxel_limit > 0);
  if (n_inst == 0 || npoint == 0) return 0;
  DCL_CHECK_ARG(xyz && rgb && unit_host && feats && coords);
  hipLaunchKernelGGL(k_crop_sample, dim3(dcl_grid_1d((long long)n_inst * npoint, 256)), dim3(256), 0, (hipStream_t)stream,
                     n_inst, npoint, cap, xyz, rgb, sample_idx, counts, min_valid, half_extent0, unit_host[0],
                     unit_host[1], unit_host[2], (float)voxel_limit, feats, coords);
  DCL_LAUNCH_CHECK();
  return 0;
}
