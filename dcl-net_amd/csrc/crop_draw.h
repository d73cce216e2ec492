// crop_draw.h -- the counter-based sampling draw of the crop builders' device form (include/dclnet_hip.h: dcl_crop_draw), shared
// by the kernel (crop_draw.hip) and its host twin (crop_draw_host.cpp).  Integer arithmetic only, all of it uint64 mod 2^64:
//   mix(z)                      the splitmix64 finaliser, a bijection of uint64
//   base(seed, frame, inst, s)  = mix(mix(mix(seed + G) ^ (frame + G)) ^ (2 inst + s + G))
//   key(j)                      = mix(base + (j + 1) G)          G is odd: distinct j < 2^64 give distinct keys
// A key is a pure function of its index, so a pass over an instance's m indices reads no memory.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DCL_DRAW_HD __host__ __device__
#else
#define DCL_DRAW_HD
#endif

namespace {

constexpr uint64_t kDrawG = 0x9E3779B97F4A7C15ull;
constexpr int kDrawWithoutReplacement = 0, kDrawWithReplacement = 1;     // the stream s of an instance's base

DCL_DRAW_HD inline uint64_t draw_mix(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

DCL_DRAW_HD inline uint64_t draw_base(uint64_t seed, uint64_t frame, int inst, int s) {
  return draw_mix(draw_mix(draw_mix(seed + kDrawG) ^ (frame + kDrawG)) ^ (2ull * (uint64_t)inst + (uint64_t)s + kDrawG));
}

DCL_DRAW_HD inline uint64_t draw_key(uint64_t base, uint64_t j) { return draw_mix(base + (j + 1) * kDrawG); }

// floor(a * b / 2^64): the high half of the 128-bit product, from 32-bit pieces (the same code on both sides)
DCL_DRAW_HD inline uint64_t draw_mulhi(uint64_t a, uint64_t b) {
  const uint64_t a0 = a & 0xffffffffull, a1 = a >> 32, b0 = b & 0xffffffffull, b1 = b >> 32;
  const uint64_t p00 = a0 * b0, p01 = a0 * b1, p10 = a1 * b0, p11 = a1 * b1;
  const uint64_t mid = (p00 >> 32) + (p01 & 0xffffffffull) + (p10 & 0xffffffffull);
  return p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32);
}

// the loaders' rule for "this instance gives a crop" on a row {masked pixels, points inside the grid, rows written} of
// dcl_crop_points' counts; a row without a written point draws nothing whatever the rule says
DCL_DRAW_HD inline int draw_valid(const int32_t *c, int min_valid, int keep_sparse) {
  return c[0] > 0 && (keep_sparse || c[1] > min_valid) && c[2] > 0;
}

// (key, j) order: keys of distinct indices differ, the index only places the sort's padding behind every real entry
DCL_DRAW_HD inline bool draw_less(uint64_t ka, int32_t ja, uint64_t kb, int32_t jb) { return ka < kb || (ka == kb && ja < jb); }

}  // namespace
