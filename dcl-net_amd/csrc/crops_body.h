// crops_body.h -- the bodies of the three crop kernels, shared by the evaluation entry (crops.hip: dcl_crop_points) and the
// training entry (crops_train.hip: dcl_crop_points_posed).  Each kernel of either file is a thin wrapper that fetches its
// crop's box, source frame and camera and calls the body; the training wrappers pass a kPose other than kPoseNone, which adds the loader's
// re-pose (dataloader_train_YCBV.py:159-174) between the centroid and the grid filter.  With kPoseNone a body is, statement
// for statement, what k_crop_mask / k_crop_centroid / k_crop_keep were before the split: the same float operations in the
// same order (the library is built with -ffp-contract=off), so the same bits.
// The posed path has two precisions (the template argument kPose): kPoseF32, the YCB-V training loader's float32 re-pose, and
// kPoseF64, the LineMOD training loader's (LM/dataloader_train_LM.py:177-188,200-209), which holds the cloud in float64 from the
// moment the float64 translation is subtracted until the FloatTensor of the sampled rows is made (crops_train_lm.hip).
#pragma once
#include "common.h"

namespace {

constexpr int kCropThreads = 1024;
constexpr int kCropChunk = 4096;                // pixels / rows per workgroup step: 4 consecutive per thread

// exclusive prefix of one small count per thread over the workgroup (order = thread id); returns the block total
__device__ __forceinline__ int block_excl_scan(int v, int *s_wave /* [16] */, int &total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int up = __shfl_up(incl, d, 64);
    if (lane >= d) incl += up;
  }
  __syncthreads();                             // s_wave may still be read from the previous call
  if (lane == 63) s_wave[wave] = incl;
  __syncthreads();
  int base = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < kCropThreads / 64; ++w) {
    const int t = s_wave[w];
    if (w < wave) base += t;
    total += t;
  }
  return base + incl - v;
}

struct CropCam { float cx, cy, fx, fy, scale, post_div; };
struct CropBox { int rmin, rmax, cmin, cmax, obj; };

// scratch of an instance (ints): [0] n (masked pixels), [1] rows kept, [2] filter applied, [3] reserved,
// [4 .. 4 + nch): status of the mask chunks (count + 1; 0 = not yet published), [4 + nch .. 4 + 2 nch): output offset of the row chunks
__host__ __device__ inline int crop_ws_ints(int cap) { return 4 + 2 * ((cap + kCropChunk - 1) / kCropChunk); }

// ---- the pose row of a training crop (include/dclnet_hip.h: DCL_CROP_POSE_ROW_BYTES) and what one lane makes of it
struct CropPoseRow {
  double t_gt[3];      // meta['poses'][:, 3, idx], float64 as the loader holds it until the centroid is subtracted (:136,159)
  float R0[9];         // meta['poses'][:, 0:3, idx] as torch.FloatTensor, row major (:135,169)
  float j[3];          // [random.uniform(-0.03, 0.03)] * 3 as torch.FloatTensor (:172)
  float A[9];          // aug_r = euler2mat(a1, a2, a3) as torch.FloatTensor (:162-166)
  float pad;
};
static_assert(sizeof(CropPoseRow) == DCL_CROP_POSE_ROW_BYTES, "pose row layout");

struct CropPose { float R0[9], R1[9], t0[3], t1[3]; };

// t0 = f32(t_gt - f64(centroid)): ONE rounding (:159 float64 difference, :168 FloatTensor); t1 = t0 + j (:172); R1 = R0 A (:173),
// each element the left-to-right three-term sum
__host__ __device__ inline void crop_pose_form(const CropPoseRow &row, const float *cen, CropPose &P) {
  for (int k = 0; k < 3; ++k) {
    P.t0[k] = (float)(row.t_gt[k] - (double)cen[k]);
    P.t1[k] = P.t0[k] + row.j[k];
  }
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)
      P.R1[i * 3 + j] = (row.R0[i * 3] * row.A[j] + row.R0[i * 3 + 1] * row.A[3 + j]) + row.R0[i * 3 + 2] * row.A[6 + j];
  for (int k = 0; k < 9; ++k) P.R0[k] = row.R0[k];
}

// the loader's re-pose of one CENTRED point (:171-174): cloud = (cloud - t0) @ R0; cloud = cloud @ R1.T + t1
__host__ __device__ inline void crop_repose(const CropPose &P, float &x, float &y, float &z) {
  const float d0 = x - P.t0[0], d1 = y - P.t0[1], d2 = z - P.t0[2];
  const float q0 = (d0 * P.R0[0] + d1 * P.R0[3]) + d2 * P.R0[6];
  const float q1 = (d0 * P.R0[1] + d1 * P.R0[4]) + d2 * P.R0[7];
  const float q2 = (d0 * P.R0[2] + d1 * P.R0[5]) + d2 * P.R0[8];
  const float r0 = (q0 * P.R1[0] + q1 * P.R1[1]) + q2 * P.R1[2];
  const float r1 = (q0 * P.R1[3] + q1 * P.R1[4]) + q2 * P.R1[5];
  const float r2 = (q0 * P.R1[6] + q1 * P.R1[7]) + q2 * P.R1[8];
  x = r0 + P.t1[0]; y = r1 + P.t1[1]; z = r2 + P.t1[2];
}

// ---- the float64 pose row of a LineMOD training crop (include/dclnet_hip.h: DCL_CROP_POSE_ROW64_BYTES): everything float64, as
// the loader holds it (LM/dataloader_train_LM.py:153-154,183,186)
struct CropPoseRow64 {
  double t_gt[3];      // np.array(meta['cam_t_m2c']) / 1000.0 (:154)
  double R0[9];        // np.resize(np.array(meta['cam_R_m2c']), (3, 3)), row major (:153)
  double j[3];         // [random.uniform(-0.03, 0.03)] * 3 (:186)
  double A[9];         // aug_r = euler2mat(a1, a2, a3) (:183)
};
static_assert(sizeof(CropPoseRow64) == DCL_CROP_POSE_ROW64_BYTES, "float64 pose row layout");

struct CropPose64 { double R0[9], R1[9], t0[3], t1[3]; };

// t0 = t_gt - f64(centroid) (:177), t1 = t0 + j (:186), R1 = R0 A (:187): crop_pose_form's order, nothing rounded
__host__ __device__ inline void crop_pose_form(const CropPoseRow64 &row, const float *cen, CropPose64 &P) {
  for (int k = 0; k < 3; ++k) {
    P.t0[k] = row.t_gt[k] - (double)cen[k];
    P.t1[k] = P.t0[k] + row.j[k];
  }
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)
      P.R1[i * 3 + j] = (row.R0[i * 3] * row.A[j] + row.R0[i * 3 + 1] * row.A[3 + j]) + row.R0[i * 3 + 2] * row.A[6 + j];
  for (int k = 0; k < 9; ++k) P.R0[k] = row.R0[k];
}

// the re-pose of one CENTRED float32 point in float64 (:185,188): crop_repose's order on widened operands
__host__ __device__ inline void crop_repose(const CropPose64 &P, double &x, double &y, double &z) {
  const double d0 = x - P.t0[0], d1 = y - P.t0[1], d2 = z - P.t0[2];
  const double q0 = (d0 * P.R0[0] + d1 * P.R0[3]) + d2 * P.R0[6];
  const double q1 = (d0 * P.R0[1] + d1 * P.R0[4]) + d2 * P.R0[7];
  const double q2 = (d0 * P.R0[2] + d1 * P.R0[5]) + d2 * P.R0[8];
  const double r0 = (q0 * P.R1[0] + q1 * P.R1[1]) + q2 * P.R1[2];
  const double r1 = (q0 * P.R1[3] + q1 * P.R1[4]) + q2 * P.R1[5];
  const double r2 = (q0 * P.R1[6] + q1 * P.R1[7]) + q2 * P.R1[8];
  x = r0 + P.t1[0]; y = r1 + P.t1[1]; z = r2 + P.t1[2];
}

// what the precision of the posed path decides: the pose row, the formed pose, the type the re-posed point and the grid's
// half extent are held in (kPoseNone: the evaluation kernels, nothing is re-posed)
constexpr int kPoseNone = 0, kPoseF32 = 1, kPoseF64 = 2;
template <int kPose> struct CropPrec { using real = float; using row_t = CropPoseRow; using pose_t = CropPose; };
template <> struct CropPrec<kPoseF64> { using real = double; using row_t = CropPoseRow64; using pose_t = CropPose64; };
__device__ __forceinline__ float crop_abs(float v) { return fabsf(v); }
__device__ __forceinline__ double crop_abs(double v) { return fabs(v); }

// ---- 1. masked pixels of the box in flat order (dataloader_test_YCBV.py:128-133), back-projection (:147-154)
// depth / label / rgb: the crop's FRAME; status / rx / rc: the crop's own scratch
__device__ __forceinline__ void crop_mask_body(const uint16_t *__restrict__ depth, const int32_t *__restrict__ label,
                                               const uint8_t *__restrict__ rgb, int H, int W, int rgb_channels, const CropBox box,
                                               const CropCam cam, double mean_r, double mean_g, double mean_b, int cap, int chunk,
                                               float *__restrict__ rx, float *__restrict__ rc, int32_t *__restrict__ status) {
  __shared__ int s_wave[kCropThreads / 64];
  __shared__ int s_base;
  const int t = threadIdx.x;
  const int rmin = box.rmin, rmax = box.rmax, cmin = box.cmin, cmax = box.cmax;
  const int bh = max(rmax - rmin, 0), bw = max(cmax - cmin, 0);
  const int area = min(bh * bw, cap);
  const int obj = box.obj;
  const int base = chunk * kCropChunk;
  bool keep[4];
  int cnt = 0;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int f = base + 4 * t + u;
    keep[u] = false;
    if (f < area) {
      const int r = rmin + f / bw, c = cmin + f % bw;
      if (r >= 0 && r < H && c >= 0 && c < W)
        keep[u] = label[(size_t)r * W + c] == obj && depth[(size_t)r * W + c] != 0;
    }
    cnt += keep[u];
  }
  int total;
  const int mine = block_excl_scan(cnt, s_wave, total);
  // publish this chunk's count, then add up the earlier chunks' (decoupled look-back: they belong to lower workgroup ids)
  if (t == 0) __hip_atomic_store(status + chunk, total + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
  if (t < 64) {
    int sum = 0;
    for (int c0 = 0; c0 < chunk; c0 += 64) {
      const int c = c0 + t;
      int v = 1;
      if (c < chunk)
        while ((v = __hip_atomic_load(status + c, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT)) == 0) __builtin_amdgcn_s_sleep(1);
      sum += v - 1;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, 64);
    if (t == 0) s_base = sum;
  }
  __syncthreads();
  int o = s_base + mine;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    if (!keep[u]) continue;
    const int f = base + 4 * t + u;
    const int r = rmin + f / bw, c = cmin + f % bw;
    const size_t pix = (size_t)r * W + c;
    const float pt2 = (float)depth[pix] / cam.scale;
    const float pt0 = ((float)c - cam.cx) * pt2 / cam.fx;
    const float pt1 = ((float)r - cam.cy) * pt2 / cam.fy;
    // LineMOD's loader converts millimetres afterwards, `cloud = cloud / 1000.0` (LM/dataloader_test_LM.py:160); x / 1.0f
    // is the identity for the YCB-V loaders
    rx[(size_t)o * 3] = pt0 / cam.post_div; rx[(size_t)o * 3 + 1] = pt1 / cam.post_div; rx[(size_t)o * 3 + 2] = pt2 / cam.post_div;
    // img/255.0 in float32, minus the float64 mean, rounded to float32 when the FloatTensor is made (:143-145,168)
    const uint8_t *px = rgb + pix * rgb_channels;
    rc[(size_t)o * 3] = (float)((double)((float)px[0] / 255.0f) - mean_r);
    rc[(size_t)o * 3 + 1] = (float)((double)((float)px[1] / 255.0f) - mean_g);
    rc[(size_t)o * 3 + 2] = (float)((double)((float)px[2] / 255.0f) - mean_b);
    ++o;
  }
}

// ---- 2. centroid = np.mean(cloud, axis=0): running float32 sum in row order, one division (:156); in-grid counts (:160-163)
// kPosed: one lane forms the crop's pose from its row and the centroid (rot_gt / trans_gt are written here), and the in-grid
// test is made on the RE-POSED point; the filter is unconditional and a crop with at most min_valid points inside the grid
// writes no row at all (dataloader_train_YCBV.py:189-191,208-210)
// kPoseF64: the pose and the re-posed point are float64, the grid test is made on the float64 point against a float64 half
// extent, and the labels are rounded to float32 once (LM/dataloader_train_LM.py:200,218)
template <int kPose>
__device__ __forceinline__ void crop_centroid_body(int inst, int cap, int nch, typename CropPrec<kPose>::real hx,
                                                   typename CropPrec<kPose>::real hy, typename CropPrec<kPose>::real hz,
                                                   int min_valid, int always_filter, const float *__restrict__ raw_xyz,
                                                   float *__restrict__ centroid, int32_t *__restrict__ counts,
                                                   int32_t *__restrict__ ws,
                                                   const typename CropPrec<kPose>::row_t *__restrict__ pose,
                                                   float *__restrict__ rot_gt, float *__restrict__ trans_gt) {
  constexpr bool kPosed = kPose != kPoseNone;
  using real = typename CropPrec<kPose>::real;
  __shared__ int s_wave[kCropThreads / 64];
  __shared__ float s_stage[2][kCropChunk * 3];
  __shared__ float s_cen[3];
  __shared__ int s_cnt[1024];                    // in-grid rows of every 4096-row chunk (cap <= 4 Mi pixels)
  __shared__ typename CropPrec<kPose>::pose_t s_pose;
  const int t = threadIdx.x;
  int32_t *w = ws + (size_t)inst * crop_ws_ints(cap);
  const float *rx = raw_xyz + (size_t)inst * cap * 3;
  int n = 0;
  for (int c = t; c < nch; c += kCropThreads) n += w[4 + c] - 1;
  {
    int total;
    (void)block_excl_scan(n, s_wave, total);
    n = total;
  }
  if (n == 0) {                                 // empty mask: the reference skips the instance (:135-143)
    if (t < 3) { counts[inst * 3 + t] = 0; centroid[inst * 3 + t] = 0.0f; }
    if (t == 0) { w[0] = 0; w[1] = 0; w[2] = 0; }
    if constexpr (kPosed) {
      if (t < 9) rot_gt[inst * 9 + t] = 0.0f;
      if (t < 3) trans_gt[inst * 3 + t] = 0.0f;
    }
    return;
  }
  // the sum is sequential by contract (row order, one rounding per row): a chain of n dependent adds per coordinate.  Everything
  // else is taken off the chain: the rest of the workgroup stages chunk j + 1 into LDS (one array per coordinate) while three
  // lanes add chunk j -- 16-byte LDS reads, the next 64 rows in registers before the current 64 are added
  float acc = 0.0f;
  const int nchunk = (n + kCropChunk - 1) / kCropChunk;
  auto stage = [&](int buf, int first_row, int rows, int j0, int step) {
    float *dst = &s_stage[buf][0];
    for (int j = j0; j < rows * 3; j += step) {
      const int row = j / 3, c = j - 3 * row;
      dst[c * kCropChunk + row] = rx[(size_t)first_row * 3 + j];
    }
  };
  stage(0, 0, min(kCropChunk, n), t, kCropThreads);
  __syncthreads();
  for (int ch = 0; ch < nchunk; ++ch) {
    const int base = ch * kCropChunk, rows = min(kCropChunk, n - base);
    if (t >= 64) {                              // the other waves: next chunk -> the other buffer
      const int nb = base + kCropChunk;
      if (nb < n) stage((ch + 1) & 1, nb, min(kCropChunk, n - nb), t - 64, kCropThreads - 64);
    } else if (t < 3) {
      const float *col = &s_stage[ch & 1][t * kCropChunk];
      const float4 *col4 = reinterpret_cast<const float4 *>(col);
      const int nb64 = rows >> 5;                          // blocks of 32 rows
      // two register sets in turn (A: even blocks, B: odd ones; 2 x 32 registers -- the 1024-thread workgroup has 128): the loads of one set fly under the adds of the other
      float4 va[8], vb[8];
      auto load16 = [&](float4 (&v)[8], int blk) {
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = col4[blk * 8 + q];
      };
      auto add16 = [&](const float4 (&v)[8]) {
#pragma unroll
        for (int q = 0; q < 8; ++q) { acc = acc + v[q].x; acc = acc + v[q].y; acc = acc + v[q].z; acc = acc + v[q].w; }
      };
      if (nb64 > 0) load16(va, 0);
      int b64 = 0;
      for (; b64 + 2 <= nb64; b64 += 2) {
        load16(vb, b64 + 1);
        add16(va);
        if (b64 + 2 < nb64) load16(va, b64 + 2);
        add16(vb);
      }
      if (b64 < nb64) add16(va);
      for (int i = nb64 << 5; i < rows; ++i) acc = acc + col[i];
    }
    __syncthreads();
  }
  if (t < 3) { const float cen = acc / (float)n; s_cen[t] = cen; centroid[inst * 3 + t] = cen; }
  __syncthreads();
  const float cx = s_cen[0], cy = s_cen[1], cz = s_cen[2];
  typename CropPrec<kPose>::pose_t P;
  if constexpr (kPosed) {
    if (t == 0) {                               // the pose: one lane, read by every thread through LDS
      crop_pose_form(pose[inst], s_cen, s_pose);
#pragma unroll
      for (int k = 0; k < 9; ++k) rot_gt[inst * 9 + k] = (float)s_pose.R1[k];
#pragma unroll
      for (int k = 0; k < 3; ++k) trans_gt[inst * 3 + k] = (float)s_pose.t1[k];
    }
    __syncthreads();
    P = s_pose;
  }
  // points inside the voxel grid, per 4096-row chunk
  int valid = 0;
  for (int ch = 0; ch < nchunk; ++ch) {
    int v = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = ch * kCropChunk + 4 * t + u;
      if (i < n) {
        real x = rx[(size_t)i * 3] - cx, y = rx[(size_t)i * 3 + 1] - cy, z = rx[(size_t)i * 3 + 2] - cz;   // centred in float32
        if constexpr (kPosed) crop_repose(P, x, y, z);
        v += crop_abs(x) < hx && crop_abs(y) < hy && crop_abs(z) < hz;
      }
    }
    int total;
    (void)block_excl_scan(v, s_wave, total);
    if (t == 0) s_cnt[ch] = total;
    valid += total;
  }
  __syncthreads();
  const bool filter = kPosed || valid > min_valid || always_filter;   // `if valid_num > 32` (:163); LM eval mode filters always (:197)
  if (t == 0) {
    int off = 0;
    for (int ch = 0; ch < nchunk; ++ch) {
      w[4 + nch + ch] = off;
      off += filter ? s_cnt[ch] : min(kCropChunk, n - ch * kCropChunk);
    }
    if (kPosed && valid <= min_valid) {         // the training loader's dummy (:191,208-210): no row is written
      w[0] = 0; w[1] = 0; w[2] = 1;
      counts[inst * 3] = n; counts[inst * 3 + 1] = valid; counts[inst * 3 + 2] = 0;
    } else {
      w[0] = n; w[1] = off; w[2] = filter ? 1 : 0;
      counts[inst * 3] = n; counts[inst * 3 + 1] = valid; counts[inst * 3 + 2] = off;
    }
  }
}

// ---- 3. keep the points inside the grid (in order), centred (:160-165); kPosed: centred, re-posed, then the grid test
// kPoseF64: the grid test on the float64 point, the point rounded to float32 once when it is written
template <int kPose>
__device__ __forceinline__ void crop_keep_body(int inst, int chunk, int cap, int nch, typename CropPrec<kPose>::real hx,
                                               typename CropPrec<kPose>::real hy, typename CropPrec<kPose>::real hz,
                                               const float *__restrict__ raw_xyz, const float *__restrict__ raw_rgb,
                                               const float *__restrict__ centroid, float *__restrict__ out_xyz,
                                               float *__restrict__ out_rgb, const int32_t *__restrict__ ws,
                                               const typename CropPrec<kPose>::row_t *__restrict__ pose) {
  constexpr bool kPosed = kPose != kPoseNone;
  using real = typename CropPrec<kPose>::real;
  __shared__ int s_wave[kCropThreads / 64];
  const int t = threadIdx.x;
  const int32_t *w = ws + (size_t)inst * crop_ws_ints(cap);
  const int n = w[0];
  if (chunk * kCropChunk >= n) return;
  const bool filter = w[2] != 0;
  const float cx = centroid[inst * 3], cy = centroid[inst * 3 + 1], cz = centroid[inst * 3 + 2];
  typename CropPrec<kPose>::pose_t P;
  if constexpr (kPosed) {                       // the same function of the same row and centroid as in the centroid kernel
    const float cen[3] = {cx, cy, cz};
    crop_pose_form(pose[inst], cen, P);
  }
  const float *rx = raw_xyz + (size_t)inst * cap * 3, *rc = raw_rgb + (size_t)inst * cap * 3;
  float *ox = out_xyz + (size_t)inst * cap * 3, *oc = out_rgb + (size_t)inst * cap * 3;
  bool keep[4];
  float p[4][3];
  int cnt = 0;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int i = chunk * kCropChunk + 4 * t + u;
    keep[u] = false;
    if (i < n) {
      real x = rx[(size_t)i * 3] - cx, y = rx[(size_t)i * 3 + 1] - cy, z = rx[(size_t)i * 3 + 2] - cz;
      if constexpr (kPosed) crop_repose(P, x, y, z);
      keep[u] = !filter || (crop_abs(x) < hx && crop_abs(y) < hy && crop_abs(z) < hz);
      p[u][0] = (float)x; p[u][1] = (float)y; p[u][2] = (float)z;
    }
    cnt += keep[u];
  }
  int total;
  int o = w[4 + nch + chunk] + block_excl_scan(cnt, s_wave, total);
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    if (!keep[u]) continue;
    const int i = chunk * kCropChunk + 4 * t + u;
#pragma unroll
    for (int j = 0; j < 3; ++j) { ox[(size_t)o * 3 + j] = p[u][j]; oc[(size_t)o * 3 + j] = rc[(size_t)i * 3 + j]; }
    ++o;
  }
}

// ---- 4. one sampled point -> its feats row [1, r, g, b, x, y, z] and voxel coordinate row [inst, ix, iy, iz] (:170-176,186-190):
//   voxel = trunc((xyz + half_extent0) / unit) in float32, clamped to [0, limit - 1] first where `clamp` (the crop had at most
//   min_valid points inside the grid).  p / c: the point's xyz and colour.  The body of k_crop_sample and k_crop_sample_valid
//   and of the host twin.
__host__ __device__ inline void crop_sample_row(const float *p, const float *c, bool clamp, int64_t inst, float half0, float ux,
                                                float uy, float uz, float limit, float *f, int64_t *o) {
  const float x = p[0], y = p[1], z = p[2];
  f[0] = 1.0f; f[1] = c[0]; f[2] = c[1]; f[3] = c[2]; f[4] = x; f[5] = y; f[6] = z;
  float vx = (x + half0) / ux, vy = (y + half0) / uy, vz = (z + half0) / uz;
  if (clamp) {
    vx = fminf(fmaxf(vx, 0.0f), limit - 1.0f); vy = fminf(fmaxf(vy, 0.0f), limit - 1.0f);
    vz = fminf(fmaxf(vz, 0.0f), limit - 1.0f);
  }
  o[0] = inst; o[1] = (int64_t)vx; o[2] = (int64_t)vy; o[3] = (int64_t)vz;
}

// point j of the LATTICE DUMMY crop of an instance that gives no crop (dcl_crop_sample_valid): the centre of voxel
// (j mod S, (j div S) mod S, j div S^2), colour 0 -- one point per voxel, npoint <= S^3
inline bool crop_lattice_fits(int npoint, int S) { return S >= 2048 || (long long)npoint <= (long long)S * S * S; }
__host__ __device__ inline void crop_lattice_row(int64_t j, int S, int64_t inst, float half0, float ux, float uy, float uz,
                                                 float *f, int64_t *o) {
  const int ix = (int)(j % S), iy = (int)((j / S) % S), iz = (int)(j / ((int64_t)S * S));
  f[0] = 1.0f; f[1] = 0.0f; f[2] = 0.0f; f[3] = 0.0f;
  f[4] = ((float)ix + 0.5f) * ux - half0; f[5] = ((float)iy + 0.5f) * uy - half0; f[6] = ((float)iz + 0.5f) * uz - half0;
  o[0] = inst; o[1] = ix; o[2] = iy; o[3] = iz;
}

}  // namespace
