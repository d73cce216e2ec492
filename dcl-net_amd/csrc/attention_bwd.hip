// attention_bwd.hip -- gradients of the correspondence attention (dcl_cross_attention) without the attention map.
//
// Notation of include/dclnet_hip.h: S[j,i] = <K[j,:], Q[i,:]> (64 ch), P = softmax over the KEY axis j,
// O = [O1|O2] = P^T [V1|V2] (320 ch).  With delta_i = <dO[i,:], O[i,:]>, dP[j,i] = <dO[i,:], V[j,:]> and
// dS = P (dP - delta):   dV[j,:] = sum_i P[j,i] dO[i,:],   dK[j,:] = sum_i dS[j,i] Q[i,:],   dQ[i,:] = sum_j dS[j,i] K[j,:].
//
// Nothing of size nq*nk is stored: P is recomputed tile by tile from the per-query log-sum-exp.  Three launches, every one
// owning the rows it writes -- no float atomics, no workgroup waits on another, so the result is bit-reproducible:
//   k_attn_bwd_stats        lse_i = max_j S + ln sum_j exp(S - max) and delta_i, per query row   (workspace: 2 floats / query)
//   k_attn_bwd_sweep<true>  a workgroup owns 64 KEYS, sweeps all 32-query slices, keeps dK and dV in accumulators
//   k_attn_bwd_sweep<false> a workgroup owns 64 QUERIES, sweeps all 32-key slices, keeps dQ in accumulators
// The price of the two sweeps is that S and dP are formed twice.
//
// One sweep body serves both: the FIXED side's rows sit on the MFMA lane (their 64 + 320 operand channels in registers for the
// whole sweep), the STREAMED side's 32-row slices pass through LDS as one [32][64 | 320] image that is read by rows for
// S and dP and by columns for the gradient products.  S and dP come out with the streamed row in the 16 accumulator
// registers and the fixed row on the lane, which is the B-operand layout of the products that sum over the streamed row
// (dK, dV resp. dQ): no shuffle, no LDS round trip for P or dS.
// 32 fixed rows are shared by a PAIR of waves that split the CHANNELS: wave p contracts channels [32p, 32p+32) of S and
// [160p, 160p+160) of dP -- half the operand registers each -- the two exchange their partial tiles through LDS once per
// slice, and wave p then accumulates the output channels [32p, 32p+32) (dK/dQ) and [160p, 160p+160) (dV): 96 accumulator
// registers instead of 192.  k_attn_bwd_stats adds the two 32-channel chains of S in the same order, so the exponent
// S - lse is formed from the same bits in all three kernels.
#include "common.h"
#include "mfma_tile.h"
#include <math.h>

namespace {

constexpr int kDK = 64, kDV1 = 256, kDV2 = 64, kDV = kDV1 + kDV2;
constexpr int kRowF4 = (kDK + kDV) / 4;                 // float4 per streamed row: 96
constexpr int kPitch = kDK + kDV + 4;                   // floats per row of the LDS image (4 pad: b128 row reads conflict-free)
constexpr int kTileFloats = 32 * kPitch;
constexpr int kXchFloats = 4 * 8 * 64 * 4;              // per wave: 8 float4 (partial S, partial dP) per lane
constexpr size_t kSweepLds = (size_t)(2 * kTileFloats + kXchFloats) * sizeof(float);

__device__ __forceinline__ float f4at(const float4 &v, int j) { return j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w; }

#define DCL_MFMA4(acc, a, breg, i)                                                    \
  do {                                                                                \
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32((a).x, breg[4 * (i) + 0], acc, 0, 0, 0); \
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32((a).y, breg[4 * (i) + 1], acc, 0, 0, 0); \
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32((a).z, breg[4 * (i) + 2], acc, 0, 0, 0); \
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32((a).w, breg[4 * (i) + 3], acc, 0, 0, 0); \
  } while (0)

// lse (log-sum-exp of a query's scores over the keys) and delta, rows [b][nq_pad] (nq_pad = nq rounded up to 32; the pad
// entries are written as 0).  Workgroup = 4 waves = 128 queries of one crop; query on the lane, 32 keys per step straight
// from global memory (this pass is 1/10 of the sweeps' matrix work).
__global__ __launch_bounds__(256) void k_attn_bwd_stats(int nq, int nk, int nq_pad, const float *__restrict__ Q, int ldq,
                                                        const float *__restrict__ K, int ldk, const float *__restrict__ O1, int ldo1,
                                                        const float *__restrict__ O2, int ldo2, const float *__restrict__ dO1,
                                                        int lddo1, const float *__restrict__ dO2, int lddo2,
                                                        float *__restrict__ lse, float *__restrict__ delta) {
  const int b = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int q = blockIdx.x * 128 + wave * 32 + r;
  const bool qlive = q < nq;
  const size_t qrow = (size_t)b * nq + (qlive ? q : nq - 1);

  // chain p contracts channels [32p, 32p+32): MFMA step s takes {32p+s, 32p+16+s}; lane half h holds 32p+16h+s
  float Qr[2][16];
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float4 v = *reinterpret_cast<const float4 *>(Q + qrow * ldq + 32 * p + 16 * h + 4 * i);
      Qr[p][4 * i] = v.x; Qr[p][4 * i + 1] = v.y; Qr[p][4 * i + 2] = v.z; Qr[p][4 * i + 3] = v.w;
    }

  float m_run = -INFINITY, l_run = 0.0f;
  for (int kb = 0; kb < nk; kb += 32) {
    const float *krow = K + ((size_t)b * nk + min(kb + r, nk - 1)) * ldk + 16 * h;     // rows past nk: masked below
    float4 kv[2][4];
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int i = 0; i < 4; ++i) kv[p][i] = *reinterpret_cast<const float4 *>(krow + 32 * p + 4 * i);
    f32x16 S0, S1;
#pragma unroll
    for (int e = 0; e < 16; ++e) { S0[e] = 0.0f; S1[e] = 0.0f; }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      DCL_MFMA4(S0, kv[0][i], Qr[0], i);
      DCL_MFMA4(S1, kv[1][i], Qr[1], i);
    }
    float s[16], m_tile = -INFINITY;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      s[e] = S0[e] + S1[e];
      if (kb + rowmap(e, h) >= nk) s[e] = -INFINITY;
      m_tile = fmaxf(m_tile, s[e]);
    }
    const float m_new = fmaxf(m_run, m_tile);
    const float m_safe = m_new == -INFINITY ? 0.0f : m_new;      // (a lane half whose keys so far are all past nk)
    float l_tile = 0.0f;
#pragma unroll
    for (int e = 0; e < 16; ++e) l_tile += expf(s[e] - m_safe);
    l_run = l_run * expf(m_run - m_safe) + l_tile;
    m_run = m_new;
  }
  // the two lane halves saw disjoint keys (key 0 is in half 0, so the joint maximum is finite)
  const float m_oth = __shfl_xor(m_run, 32, 64), l_oth = __shfl_xor(l_run, 32, 64);
  const float m = fmaxf(m_run, m_oth);
  const float l = l_run * expf(m_run - m) + l_oth * expf(m_oth - m);

  // delta: lane half h sums channels [160h, 160h+160) of dO . O in a fixed order
  float d = 0.0f;
#pragma unroll 8
  for (int i = 0; i < 40; ++i) {
    const int c = 160 * h + 4 * i;
    float4 g = make_float4(0.f, 0.f, 0.f, 0.f), o = g;
    if (c < kDV1) {
      g = *reinterpret_cast<const float4 *>(dO1 + qrow * lddo1 + c);
      o = *reinterpret_cast<const float4 *>(O1 + qrow * ldo1 + c);
    } else if (dO2) {
      g = *reinterpret_cast<const float4 *>(dO2 + qrow * lddo2 + (c - kDV1));
      o = *reinterpret_cast<const float4 *>(O2 + qrow * ldo2 + (c - kDV1));
    }
    d += g.x * o.x; d += g.y * o.y; d += g.z * o.z; d += g.w * o.w;
  }
  const float d_oth = __shfl_xor(d, 32, 64);
  if (h == 0 && q < nq_pad) {
    lse[(size_t)b * nq_pad + q] = qlive ? m + logf(l) : 0.0f;
    delta[(size_t)b * nq_pad + q] = qlive ? d + d_oth : 0.0f;
  }
}

// The sweep (see the head of the file).  Fixed side: rows [nf] per crop with operands F64 (64 ch) and [F1 | F2] (256 | 64 ch);
// streamed side: rows [ns] with T64 and [T1 | T2].  KEYS_FIXED: F = (K, V1, V2), T = (Q, dO1, dO2), G64 = dK, [G1 | G2] = dV;
// else F = (Q, dO1, dO2), T = (K, V1, V2), G64 = dQ.  F2 / T2 = nullptr (a missing dO2) read as zeros.
// Workgroup = 4 waves = 2 row groups x 2 channel halves = 64 fixed rows; grid (ceil(nf / 64), b).
template <bool KEYS_FIXED>
__global__ __launch_bounds__(256, 1) void k_attn_bwd_sweep(int nf, int ns, int nq_pad, const float *__restrict__ F64, int ldf64,
                                                           const float *__restrict__ F1, int ldf1, const float *__restrict__ F2, int ldf2,
                                                           const float *__restrict__ T64, int ldt64, const float *__restrict__ T1,
                                                           int ldt1, const float *__restrict__ T2, int ldt2,
                                                           const float *__restrict__ lse, const float *__restrict__ delta,
                                                           float *__restrict__ G64, int ldg64, float *__restrict__ G1, int ldg1,
                                                           float *__restrict__ G2, int ldg2) {
  extern __shared__ __attribute__((aligned(16))) float attn_bwd_lds[];      // [2][32][kPitch] slices, [4 waves][8][64 lanes] float4
  float *xch = attn_bwd_lds + 2 * kTileFloats;
  const int b = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int grp = wave >> 1, p = wave & 1;
  const int f = blockIdx.x * 64 + 32 * grp + r;
  const bool flive = f < nf;
  const size_t frow = (size_t)b * nf + (flive ? f : nf - 1);          // dead lanes compute on a live row and are masked

  // B operands of the partial S and dP chains: step s contracts channels {base + s, base + half + s}, lane half h holds the second
  float F64r[16], F320r[80];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float4 v = *reinterpret_cast<const float4 *>(F64 + frow * ldf64 + 32 * p + 16 * h + 4 * i);
    F64r[4 * i] = v.x; F64r[4 * i + 1] = v.y; F64r[4 * i + 2] = v.z; F64r[4 * i + 3] = v.w;
  }
#pragma unroll
  for (int i = 0; i < 20; ++i) {
    const int c = 160 * p + 80 * h + 4 * i;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c < kDV1) v = *reinterpret_cast<const float4 *>(F1 + frow * ldf1 + c);
    else if (F2) v = *reinterpret_cast<const float4 *>(F2 + frow * ldf2 + (c - kDV1));
    F320r[4 * i] = v.x; F320r[4 * i + 1] = v.y; F320r[4 * i + 2] = v.z; F320r[4 * i + 3] = v.w;
  }
  float lse_f = 0.0f, delta_f = 0.0f;                                  // the row constants belong to the query side
  if (!KEYS_FIXED && flive) {
    lse_f = lse[(size_t)b * nq_pad + f];
    delta_f = delta[(size_t)b * nq_pad + f];
  }

  // one streamed slice = 32 rows x 96 float4 = 12 float4 per thread; rows past ns are zero-filled
  float4 st[12];
  auto stage_load = [&](int s0) {
#pragma unroll
    for (int i = 0; i < 12; ++i) {
      const int idx = tid + 256 * i, row = idx / kRowF4, c = (idx - row * kRowF4) * 4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (s0 + row < ns) {
        const size_t gr = (size_t)b * ns + s0 + row;
        if (c < kDK) v = *reinterpret_cast<const float4 *>(T64 + gr * ldt64 + c);
        else if (c < kDK + kDV1) v = *reinterpret_cast<const float4 *>(T1 + gr * ldt1 + (c - kDK));
        else if (T2) v = *reinterpret_cast<const float4 *>(T2 + gr * ldt2 + (c - kDK - kDV1));
      }
      st[i] = v;
    }
  };
  auto stage_write = [&](float *buf) {
#pragma unroll
    for (int i = 0; i < 12; ++i) {
      const int idx = tid + 256 * i, row = idx / kRowF4, c = (idx - row * kRowF4) * 4;
      *reinterpret_cast<float4 *>(buf + row * kPitch + c) = st[i];
    }
  };

  f32x16 acc64, acc320[5];
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    acc64[e] = 0.0f;
#pragma unroll
    for (int t = 0; t < 5; ++t) acc320[t][e] = 0.0f;
  }

  const int nt = (ns + 31) / 32;
  stage_load(0);
  stage_write(attn_bwd_lds);
  __syncthreads();
  for (int t = 0; t < nt; ++t) {
    const float *cur = attn_bwd_lds + (t & 1) * kTileFloats;
    const int s0 = t * 32;
    const bool more = t + 1 < nt;
    if (more) stage_load(s0 + 32);                       // in flight during this slice's products

    float4 cl[4], cd[4];                                 // lse / delta of the streamed rows rowmap(4g .. 4g+3, h) = 8g + 4h ..
    if (KEYS_FIXED) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        cl[g] = *reinterpret_cast<const float4 *>(lse + (size_t)b * nq_pad + s0 + 8 * g + 4 * h);
        cd[g] = *reinterpret_cast<const float4 *>(delta + (size_t)b * nq_pad + s0 + 8 * g + 4 * h);
      }
    }

    // ---- partial S and dP over this wave's channels: A = streamed row r (LDS row read), B = fixed row (registers) ----
    f32x16 S, D;
#pragma unroll
    for (int e = 0; e < 16; ++e) { S[e] = 0.0f; D[e] = 0.0f; }
    {
      const float *trow = cur + r * kPitch;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float4 a = *reinterpret_cast<const float4 *>(trow + 32 * p + 16 * h + 4 * i);
        DCL_MFMA4(S, a, F64r, i);
      }
#pragma unroll
      for (int i = 0; i < 20; ++i) {
        const float4 a = *reinterpret_cast<const float4 *>(trow + kDK + 160 * p + 80 * h + 4 * i);
        DCL_MFMA4(D, a, F320r, i);
      }
    }

    // ---- the pair exchanges its partial tiles (a + b is the same float either way round) ----
    {
      float *mine = xch + wave * 2048 + lane * 4;
      const float *theirs = xch + (wave ^ 1) * 2048 + lane * 4;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        *reinterpret_cast<float4 *>(mine + g * 256) = make_float4(S[4 * g], S[4 * g + 1], S[4 * g + 2], S[4 * g + 3]);
        *reinterpret_cast<float4 *>(mine + (4 + g) * 256) = make_float4(D[4 * g], D[4 * g + 1], D[4 * g + 2], D[4 * g + 3]);
      }
      __syncthreads();
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 os = *reinterpret_cast<const float4 *>(theirs + g * 256);
        const float4 od = *reinterpret_cast<const float4 *>(theirs + (4 + g) * 256);
        S[4 * g] += os.x; S[4 * g + 1] += os.y; S[4 * g + 2] += os.z; S[4 * g + 3] += os.w;
        D[4 * g] += od.x; D[4 * g + 1] += od.y; D[4 * g + 2] += od.z; D[4 * g + 3] += od.w;
      }
    }

    // ---- P = exp(S - lse) (never above 1: lse >= the row maximum), dS = P (dP - delta); rows / lanes out of range give 0 ----
    float P[16], dS[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const bool live = flive && s0 + rowmap(e, h) < ns;
      const float l = KEYS_FIXED ? f4at(cl[e >> 2], e & 3) : lse_f;
      const float dl = KEYS_FIXED ? f4at(cd[e >> 2], e & 3) : delta_f;
      const float pe = live ? expf(S[e] - l) : 0.0f;
      P[e] = pe;
      dS[e] = live ? pe * (D[e] - dl) : 0.0f;
    }

    // ---- G^T[c][fixed] += sum over streamed rows: A = column c of the image (row rowmap(e, h)), B = register e ----
    {
      const float *tcol = cur + 4 * h * kPitch + r;
#pragma unroll
      for (int e = 0; e < 16; ++e)
        acc64 = __builtin_amdgcn_mfma_f32_32x32x2f32(tcol[rowmap(e, 0) * kPitch + 32 * p], dS[e], acc64, 0, 0, 0);
      if (KEYS_FIXED) {
#pragma unroll
        for (int tt = 0; tt < 5; ++tt) {
#pragma unroll
          for (int e = 0; e < 16; ++e)
            acc320[tt] = __builtin_amdgcn_mfma_f32_32x32x2f32(tcol[rowmap(e, 0) * kPitch + kDK + 160 * p + 32 * tt],
                                                              P[e], acc320[tt], 0, 0, 0);
        }
      }
    }
    if (more) stage_write(attn_bwd_lds + ((t + 1) & 1) * kTileFloats);
    __syncthreads();
  }

  if (flive) {
    const size_t row = (size_t)b * nf + f;
#pragma unroll
    for (int g = 0; g < 4; ++g) {                           // registers 4g .. 4g+3 = 4 consecutive channels
      const int c = 32 * p + 8 * g + 4 * h;
      *reinterpret_cast<float4 *>(G64 + row * ldg64 + c) = make_float4(acc64[4 * g], acc64[4 * g + 1], acc64[4 * g + 2], acc64[4 * g + 3]);
    }
    if (KEYS_FIXED) {
#pragma unroll
      for (int tt = 0; tt < 5; ++tt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int c = 160 * p + 32 * tt + 8 * g + 4 * h;
          const float4 v = make_float4(acc320[tt][4 * g], acc320[tt][4 * g + 1], acc320[tt][4 * g + 2], acc320[tt][4 * g + 3]);
          if (c < kDV1) *reinterpret_cast<float4 *>(G1 + row * ldg1 + c) = v;
          else *reinterpret_cast<float4 *>(G2 + row * ldg2 + (c - kDV1)) = v;
        }
    }
  }
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// rows of lse / delta per crop: nq rounded up to a whole 32-query slice (float4 reads of a slice's constants stay aligned)
long long bwd_nq_pad(int nq) { return ((long long)nq + 31) / 32 * 32; }

int bwd_sizes_ok(int b, int nq, int nk) {
  return b >= 0 && nq >= 0 && nk >= 0 && b <= 65535 && (long long)b * bwd_nq_pad(nq) <= 0x7fffffffLL - 8192 &&
         (long long)b * nk <= 0x7fffffffLL - 8192;
}

}  // namespace

DCL_API int dcl_cross_attention_bwd_ws_bytes(int b, int nq, int nk, int64_t *bytes_host) {
  DCL_CHECK_ARG(bytes_host != nullptr);
  DCL_CHECK_ARG(bwd_sizes_ok(b, nq, nk));
  *bytes_host = 256 + 2 * (int64_t)b * bwd_nq_pad(nq) * (int64_t)sizeof(float);     // lse, delta (+ a floor so that it is never 0)
  return 0;
}

DCL_API int dcl_cross_attention_bwd(int b, int nq, int nk, const float *Q, int ldq, const float *K, int ldk, const float *V1,
                                    int dv1, int ldv1, const float *V2, int dv2, int ldv2, const float *O1, int ldo1,
                                    const float *O2, int ldo2, const float *dO1, int lddo1, const float *dO2, int lddo2,
                                    float *dQ, int lddq, float *dK, int lddk, float *dV1, int lddv1, float *dV2, int lddv2,
                                    void *ws, int64_t ws_bytes, dclStream_t stream) {
  DCL_CHECK_ARG(b >= 1 && nq >= 1 && nk >= 1 && bwd_sizes_ok(b, nq, nk));
  if (dv1 != kDV1 || dv2 != kDV2) {
    dcl_set_error("dcl_cross_attention_bwd: invalid argument: only dv1 = 256, dv2 = 64 is built (got %d, %d)", dv1, dv2);
    return DCL_EINVAL;
  }
  int64_t need = 0;
  if (dcl_cross_attention_bwd_ws_bytes(b, nq, nk, &need) != 0) return DCL_EINVAL;
  DCL_CHECK_ARG(ws != nullptr && aligned16(ws) && ws_bytes >= need);
  DCL_CHECK_ARG(Q && K && V1 && V2 && O1 && O2 && dO1 && dQ && dK && dV1 && dV2);
  DCL_CHECK_ARG(ldq >= kDK && ldk >= kDK && lddq >= kDK && lddk >= kDK);
  DCL_CHECK_ARG(ldv1 >= kDV1 && ldo1 >= kDV1 && lddo1 >= kDV1 && lddv1 >= kDV1);
  DCL_CHECK_ARG(ldv2 >= kDV2 && ldo2 >= kDV2 && lddv2 >= kDV2 && (dO2 == nullptr || lddo2 >= kDV2));
  DCL_CHECK_ARG(((ldq | ldk | ldv1 | ldv2 | ldo1 | ldo2 | lddo1 | lddq | lddk | lddv1 | lddv2) & 3) == 0);
  DCL_CHECK_ARG(dO2 == nullptr || (lddo2 & 3) == 0);
  DCL_CHECK_ARG(aligned16(Q) && aligned16(K) && aligned16(V1) && aligned16(V2) && aligned16(O1) && aligned16(O2) &&
                aligned16(dO1) && aligned16(dO2) && aligned16(dQ) && aligned16(dK) && aligned16(dV1) && aligned16(dV2));
  hipStream_t s = (hipStream_t)stream;
  const int nq_pad = (int)bwd_nq_pad(nq);
  float *lse = (float *)ws, *delta = lse + (size_t)b * nq_pad;

  hipLaunchKernelGGL(k_attn_bwd_stats, dim3(dcl_div_up(nq, 128), b), dim3(256), 0, s, nq, nk, nq_pad, Q, ldq, K, ldk, O1, ldo1,
                     O2, ldo2, dO1, lddo1, dO2, lddo2, lse, delta);
  DCL_LAUNCH_CHECK();
  (void)hipFuncSetAttribute((const void *)k_attn_bwd_sweep<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSweepLds);
  hipLaunchKernelGGL((k_attn_bwd_sweep<true>), dim3(dcl_div_up(nk, 64), b), dim3(256), kSweepLds, s, nk, nq, nq_pad, K, ldk, V1,
                     ldv1, V2, ldv2, Q, ldq, dO1, lddo1, dO2, lddo2, (const float *)lse, (const float *)delta, dK, lddk, dV1,
                     lddv1, dV2, lddv2);
  DCL_LAUNCH_CHECK();
  (void)hipFuncSetAttribute((const void *)k_attn_bwd_sweep<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSweepLds);
  hipLaunchKernelGGL((k_attn_bwd_sweep<false>), dim3(dcl_div_up(nq, 64), b), dim3(256), kSweepLds, s, nq, nk, nq_pad, Q, ldq, dO1,
                     lddo1, dO2, lddo2, K, ldk, V1, ldv1, V2, ldv2, (const float *)lse, (const float *)delta, dQ, lddq,
                     (float *)nullptr, 0, (float *)nullptr, 0);
  DCL_LAUNCH_CHECK();
  return 0;
}
