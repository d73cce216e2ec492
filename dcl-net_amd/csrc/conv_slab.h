// conv_slab.h -- the operand slabs of the sparse convolution's staged fp32-MFMA kernels (conv_dgrad.hip, conv_fwd_compact.hip):
// rows of 32 reduction channels on their way global -> registers -> LDS, and a lane's 16 values of a 32-row operand tile.
// LDS rows hold a chunk DE-INTERLEAVED, even channels in floats 0 .. 15 and odd ones in 16 .. 31 (pitch 36): MFMA step s of
// v_mfma_f32_32x32x2_f32 takes channel 2 s from the lanes 0 .. 31 and 2 s + 1 from the lanes 32 .. 63, so a lane's 16 values of
// a chunk are four ds_read_b128 instead of sixteen ds_read_b32.  Device-only; include after common.h.
#pragma once

namespace {

constexpr int kDgThreads = 256;
constexpr int kDgKC = 32;                    // reduction channels of one LDS slab: 16 MFMA steps
constexpr int kDgPitch = 36;                 // floats between LDS rows: 16-byte aligned, and not a multiple of 32 banks

// 4 consecutive floats, columns c .. c + 3, of a row of `cols` floats, AS LOADED: an address that would be out of the row is
// clamped into it, and dg_valid says how many of the four count.  Branch-free, and nothing here looks at the loaded value, so
// that the loads of a slab are issued back to back and waited for only when the slab goes to LDS (DgSlab::put).
// VEC: rows are 16-byte aligned and cols % 4 == 0 -- one 16-byte load
template <bool VEC>
__device__ __forceinline__ float4 dg_load4(const float *row, int c, int cols) {
  if constexpr (VEC) {
    return *reinterpret_cast<const float4 *>(row + (c < cols ? c : 0));
  } else {
    const int last = cols - 1;
    return make_float4(row[c < last ? c : last], row[c + 1 < last ? c + 1 : last], row[c + 2 < last ? c + 2 : last],
                       row[c + 3 < last ? c + 3 : last]);
  }
}
// how many of the four columns c .. c + 3 exist; none in a row that is not `live`
__device__ __forceinline__ int dg_valid(int c, int cols, bool live) {
  const int n = cols - c;
  return live ? (n > 4 ? 4 : n) : 0;
}

// ROWS x kDgKC floats on their way from global memory to LDS: thread t holds the float4 items t, t + 256, ...; item = row * 8 + q
template <int ROWS>
struct DgSlab {
  static_assert(ROWS % 32 == 0, "whole items per thread");
  static constexpr int kPer = ROWS * (kDgKC / 4) / kDgThreads;
  float4 r[kPer];
  int valid[kPer];                                                               // the leading elements of r[i] that count: the rest is 0
  __device__ __forceinline__ void put(float *lds, int t) const {
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
      const int item = t + i * kDgThreads;
      float *p = lds + (item >> 3) * kDgPitch + 2 * (item & 7);
      const float x = valid[i] > 0 ? r[i].x : 0.f, y = valid[i] > 1 ? r[i].y : 0.f, z = valid[i] > 2 ? r[i].z : 0.f,
                  w = valid[i] > 3 ? r[i].w : 0.f;
      *reinterpret_cast<float2 *>(p) = make_float2(x, z);                        // channels 4 q, 4 q + 2
      *reinterpret_cast<float2 *>(p + kDgKC / 2) = make_float2(y, w);            // channels 4 q + 1, 4 q + 3
    }
  }
};

// a lane's 16 values of one 32-row operand tile: channels 2 s + h, s = 0 .. 15
__device__ __forceinline__ void dg_read16(const float *row_h, float (&v)[16]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float4 q = *reinterpret_cast<const float4 *>(row_h + 4 * j);
    v[4 * j] = q.x; v[4 * j + 1] = q.y; v[4 * j + 2] = q.z; v[4 * j + 3] = q.w;
  }
}

}  // namespace
