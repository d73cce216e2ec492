// linear_wgrad_split.hip -- the weight gradient of a per-point linear layer on the bf16 matrix pipe with fp32 results:
// dcl_linear_wgrad_split, dW[p][q] = sum_j a[j][p] b[j][q] (a = dZ (M x P), b = the layer input (M x Q), both row-major), the
// contract of dcl_linear_wgrad (linear_bwd.hip) with the arithmetic of linear_split.hip.
//
//   * every fp32 operand is the exact sum of three bf16 pieces (bf16_split2 of mfma_tile.h, the one split everyone shares) and a
//     product is accumulated as its six piece products al bh + ah bl + am bm + am bh + ah bm + ah bh, in that order, in the fp32
//     accumulators of v_mfma_f32_32x32x16_bf16.  BOTH operands are activations: nothing can be split once per layer, so the
//     split happens in the kernel, on the global -> register -> LDS path (a pre-pass writing piece planes would move 10 bytes
//     per element through HBM for a GEMM this shallow).
//   * both operands have the reduction index j on their ROWS, and a lane of the MFMA wants 8 consecutive j of one column: the
//     stage's pieces lie in LDS as row-major bf16 images [piece][16 rows][tile columns] and both MFMA operands are read with the
//     transposing ds_read_b64_tr_b16 (per 16 lanes a block of 4 rows x 16 columns, delivered column-major).  The instruction
//     needs EXEC all ones and 8-byte aligned lane addresses: the images are whole padded tiles (columns past P / Q and rows past
//     the split's end hold zero pieces), every lane of every wave reads, and no read sits in divergent code.  Row pitch of an
//     image = 64 bytes mod 256: the four rows of a 32-lane half's blocks fall on the four quarters of the 64 banks -- no
//     conflicts (checked with SQ_LDS_BANK_CONFLICT, profiles/linear_wgrad_split.txt).
//   * the order is dcl_linear_wgrad's: the M rows in splits of DCL_WGRAD_ROWS rows, a workgroup owns one (P, Q) tile of one split
//     -- its 4 waves tile (P, Q), never the rows --, an output element is ONE accumulator from +0 fed the split's 16-row chunks
//     ascending and the six products per chunk in the order above; linear_bwd.hip's k_split_sum adds the splits ascending.  No
//     float atomics, no workgroup waits on another, and the order never depends on pitch or alignment (the 16-byte load is only
//     a fast path).  A zero piece adds an exact zero, so padding changes no bit.
#include "common.h"
#include "mfma_tile.h"

namespace {

constexpr int kWsKC = 16;            // rows per LDS stage: one MFMA k step
constexpr int kWsThreads = 256;

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) s16x4 lds_s16x4_t;

// 4 consecutive floats of row `row`, columns c .. c + 3 of a (rows x cols) row-major matrix with pitch ld; 0 outside
// (linear_bwd.hip's loader: the two weight-gradient kernels guard and zero-fill alike)
__device__ __forceinline__ float4 ws_load4(const float *m, int64_t ld, int64_t row, int64_t row_hi, int c, int cols, bool vec_ok) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (row >= row_hi || c >= cols) return v;
  const float *p = m + (size_t)row * (size_t)ld + c;
  if (vec_ok && c + 3 < cols) return *reinterpret_cast<const float4 *>(p);
  v.x = p[0];
  if (c + 1 < cols) v.y = p[1];
  if (c + 2 < cols) v.z = p[2];
  if (c + 3 < cols) v.w = p[3];
  return v;
}

// One operand's stage of kWsKC rows x W columns: global -> registers (the prefetch, fp32 as it lies) and registers -> split ->
// LDS, three row-major bf16 images [piece][row][kPitch bytes]
template <int W>
struct WsStage {
  static constexpr int kItems = kWsKC * W / 4;                                 // float4 items
  static constexpr int kPer = (kItems + kWsThreads - 1) / kWsThreads;
  static constexpr int kPitch = (W * 2 + 191) / 256 * 256 + 64;                // bytes: >= a row's 2 W, = 64 (mod 256)
  static constexpr int kPiece = kWsKC * kPitch;                                // bytes of one piece image
  static constexpr int kBytes = 3 * kPiece;
  static_assert(kPitch >= 2 * W && kPitch % 256 == 64, "image pitch");
  float4 r[kPer];
  __device__ __forceinline__ void fetch(const float *m, int64_t ld, int64_t j0, int64_t row_hi, int c0, int cols, bool vec_ok) {
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
      const int item = threadIdx.x + i * kWsThreads;
      const int row = item / (W / 4), c4 = (item - row * (W / 4)) * 4;
      r[i] = item < kItems ? ws_load4(m, ld, j0 + row, row_hi, c0 + c4, cols, vec_ok) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  __device__ __forceinline__ void put(unsigned char *lds) const {
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
      const int item = threadIdx.x + i * kWsThreads;
      const int row = item / (W / 4), c4 = (item - row * (W / 4)) * 4;
      if (item < kItems) {
        uint2 h, m, l;
        bf16_split2(r[i].x, r[i].y, h.x, m.x, l.x);
        bf16_split2(r[i].z, r[i].w, h.y, m.y, l.y);
        unsigned char *at = lds + row * kPitch + c4 * 2;                       // 8-byte aligned: c4 % 4 == 0, kPitch % 8 == 0
        *reinterpret_cast<uint2 *>(at) = h;
        *reinterpret_cast<uint2 *>(at + kPiece) = m;
        *reinterpret_cast<uint2 *>(at + 2 * kPiece) = l;
      }
    }
  }
};

// The MFMA operand of a 32-column block of a piece image: lane l gets column (l & 31), rows 8 (l >> 5) .. + 7 -- two transposed
// reads of 4 rows each.  `at` is the lane's address in the block: row 8 (l >> 5) + ((l & 15) >> 2), column 16 ((l >> 4) & 1) +
// 4 (l & 3) (lane 4q + p of a 16-lane group supplies row q, columns 4p .. 4p + 3 of the group's 4 x 16 block).
__device__ __forceinline__ bf16x8 ws_operand(const unsigned char *at, int pitch) {
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t *)at);
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t *)(at + 4 * pitch));
  const uint2 a = __builtin_bit_cast(uint2, lo), b = __builtin_bit_cast(uint2, hi);
  const u32x4 v = {a.x, a.y, b.x, b.y};
  return as_bf16x8(v);
}

// WP x WQ waves (= 4), each TP x TQ accumulator tiles of 32 x 32: the workgroup's tile is (32 WP TP) x (32 WQ TQ)
template <int WP, int WQ, int TP, int TQ>
__global__ __launch_bounds__(kWsThreads) void k_linear_wgrad_split(const float *__restrict__ a, int64_t lda,
                                                                   const float *__restrict__ b, int64_t ldb, int M, int P, int Q,
                                                                   int tiles_p, int tiles_q, float *__restrict__ partial) {
  static_assert(WP * WQ * 64 == kWsThreads, "four waves");
  constexpr int BP = 32 * WP * TP, BQ = 32 * WQ * TQ;
  typedef WsStage<BP> StA;
  typedef WsStage<BQ> StB;
  __shared__ __attribute__((aligned(16))) unsigned char As[2][StA::kBytes];
  __shared__ __attribute__((aligned(16))) unsigned char Bs[2][StB::kBytes];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
  const int wp = wave / WQ, wq = wave - wp * WQ;
  // workgroup -> (split, tile): the tiles of one split are neighbours, so they read the same rows of a and b together
  const int tiles = tiles_p * tiles_q;
  const int split = blockIdx.x / tiles, tile = blockIdx.x - split * tiles;
  const int tp = tile / tiles_q, tq = tile - tp * tiles_q;
  const int p0 = tp * BP, q0 = tq * BQ;
  const int64_t row_lo = (int64_t)split * DCL_WGRAD_ROWS;
  const int64_t row_hi = row_lo + DCL_WGRAD_ROWS < (int64_t)M ? row_lo + DCL_WGRAD_ROWS : (int64_t)M;
  const bool vec_a = (((size_t)a & 15) == 0) && (lda & 3) == 0, vec_b = (((size_t)b & 15) == 0) && (ldb & 3) == 0;

  f32x16 acc[TP][TQ];
#pragma unroll
  for (int i = 0; i < TP; ++i)
#pragma unroll
    for (int j = 0; j < TQ; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;

  // the lane's place in a 32-column block of an image (ws_operand)
  const int blk_row = 8 * h + ((lane & 15) >> 2), blk_col = 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
  const int off_a = blk_row * StA::kPitch + (wp * (32 * TP) + blk_col) * 2;
  const int off_b = blk_row * StB::kPitch + (wq * (32 * TQ) + blk_col) * 2;

  StA sa;
  StB sb;
  const int nchunks = (int)((row_hi - row_lo + kWsKC - 1) / kWsKC);
  sa.fetch(a, lda, row_lo, row_hi, p0, P, vec_a);
  sb.fetch(b, ldb, row_lo, row_hi, q0, Q, vec_b);
  sa.put(As[0]);
  sb.put(Bs[0]);
  __syncthreads();
  for (int c = 0; c < nchunks; ++c) {                        // the split's 16-row chunks, ascending
    const int cur = c & 1;
    if (c + 1 < nchunks) {                                   // the next stage's loads fly during this stage's MFMAs
      const int64_t j0 = row_lo + (int64_t)(c + 1) * kWsKC;
      sa.fetch(a, lda, j0, row_hi, p0, P, vec_a);
      sb.fetch(b, ldb, j0, row_hi, q0, Q, vec_b);
    }
    // (every lane of all four waves reads, outside any lane-dependent branch: the transposed read needs EXEC all ones)
    bf16x8 ap[TP][3], bp[TQ][3];
#pragma unroll
    for (int i = 0; i < TP; ++i)
#pragma unroll
      for (int s = 0; s < 3; ++s) ap[i][s] = ws_operand(As[cur] + s * StA::kPiece + off_a + 64 * i, StA::kPitch);
#pragma unroll
    for (int j = 0; j < TQ; ++j)
#pragma unroll
      for (int s = 0; s < 3; ++s) bp[j][s] = ws_operand(Bs[cur] + s * StB::kPiece + off_b + 64 * j, StB::kPitch);
#pragma unroll
    for (int i = 0; i < TP; ++i)
#pragma unroll
      for (int j = 0; j < TQ; ++j) {                         // small terms first (linear_split.hip): l.h, h.l, m.m, m.h, h.m, h.h
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ap[i][2], bp[j][0], acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ap[i][0], bp[j][2], acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ap[i][1], bp[j][1], acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ap[i][1], bp[j][0], acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ap[i][0], bp[j][1], acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ap[i][0], bp[j][0], acc[i][j], 0, 0, 0);
      }
    if (c + 1 < nchunks) {                                   // (the other buffer: last read before the previous barrier)
      sa.put(As[cur ^ 1]);
      sb.put(Bs[cur ^ 1]);
    }
    __syncthreads();
  }
  // accumulator register e of lane half h: output row rowmap(e, h), column lane & 31
  float *out = partial + (size_t)split * (size_t)P * (size_t)Q;
#pragma unroll
  for (int i = 0; i < TP; ++i)
#pragma unroll
    for (int j = 0; j < TQ; ++j) {
      const int q = q0 + wq * (32 * TQ) + 32 * j + r;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int p = p0 + wp * (32 * TP) + 32 * i + rowmap(e, h);
        if (p < P && q < Q) out[(size_t)p * Q + q] = acc[i][j][e];
      }
    }
}

bool aligned4(const void *p) { return ((size_t)p & 3) == 0; }

}  // namespace

DCL_API int dcl_linear_wgrad_split(const float *a, int64_t lda, const float *b, int64_t ldb, int M, int P, int Q, float *partial,
                                   float *dW, int64_t lddw, dclStream_t stream) {
  DCL_CHECK_ARG(M >= 0 && P >= 1 && Q >= 1 && lda >= P && ldb >= Q && lddw >= Q);
  DCL_CHECK_ARG(dW && partial && aligned4(dW) && aligned4(partial));
  DCL_CHECK_ARG(M == 0 || (a && b && aligned4(a) && aligned4(b)));
  hipStream_t s = (hipStream_t)stream;
  int splits = 0;
  if (M > 0) {
    (void)dcl_linear_wgrad_splits(M, &splits);
    if (Q <= 32) {
      const int tiles_p = dcl_div_up(P, 128), tiles_q = 1;
      DCL_CHECK_ARG((long long)tiles_p * tiles_q * splits < (1ll << 31));
      hipLaunchKernelGGL((k_linear_wgrad_split<4, 1, 1, 1>), dim3(tiles_p * tiles_q * splits), dim3(kWsThreads), 0, s, a, lda, b,
                         ldb, M, P, Q, tiles_p, tiles_q, partial);
    } else {
      const int tiles_p = dcl_div_up(P, 128), tiles_q = dcl_div_up(Q, 128);
      DCL_CHECK_ARG((long long)tiles_p * tiles_q * splits < (1ll << 31));
      hipLaunchKernelGGL((k_linear_wgrad_split<2, 2, 2, 2>), dim3(tiles_p * tiles_q * splits), dim3(kWsThreads), 0, s, a, lda, b,
                         ldb, M, P, Q, tiles_p, tiles_q, partial);
    }
  }
  return dcl_internal_split_sum(partial, splits, P, Q, dW, lddw, s);
}
