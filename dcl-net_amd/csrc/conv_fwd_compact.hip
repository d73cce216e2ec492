// conv_fwd_compact.hip -- the sparse convolution's forward over the PRESENT (row, offset) pairs (ops.sparse_conv(form="compact")),
// beside the tile forward of sparse_conv.hip / conv_body.h ("tiles", the default, untouched), whose 128-row tiles run every
// offset that any of their rows has with all 128 rows on the matrix pipe.  No BatchNorm / ReLU epilogue: the module path, the
// only caller, applies those itself.
//
//   out[o][co] = sum_k sum_ci X[nbr[k][o]][ci] * W[k][ci][co]              nbr: kvol x cap, X: n_in x cin, W: kvol x cin x cout
//
// in the order of conv_fwd_compact.h: per present offset a chain of its own over ci ascending, added to the element with one
// fp32 add, offsets in the forward's visiting order.
//
// k_conv_fwd_compact: a workgroup of four waves owns BM consecutive output rows x BN = 32 WQ output columns (grid.y: further
// column passes of wider layers).
//   1. every wave reads the nbr entries of its offsets (k = wave, wave + 4, ...) for the BM rows and COMPACTS the present ones
//      with one ballot and a popcount prefix per 64 entries: per offset a list of (tile row, input row) in ascending tile row
//      and a count, in LDS.  Offsets with count 0 cost nothing; the raw table is never stored;
//   2. it walks the segments (offset in visiting order, block of PB = 32 WP pairs, 32-channel chunk of cin) through two LDS
//      buffers, global -> registers -> LDS: the gathered X rows and the 32 x BN piece of W[k] of the next two segments fly under
//      this segment's 16 MFMA steps (conv_slab.h: the X rows de-interleaved, as in conv_dgrad.hip; W rows as they are, pitch BN | 32
//      so that the two lane halves of a step, one W row apart, read different banks).  Wave (wp, wq) multiplies the block's
//      pairs 32 wp .. 32 wp + 31 with the columns 32 wq .. 32 wq + 31; its accumulators start at zero for a block and run
//      through all chunks of cin: one chain per element.  A wave whose 32 pairs are all padding skips the MFMAs;
//   3. behind a block's last chunk the 32 x 32 result is ADDED, one fp32 add per element, into the output tile that lives in
//      LDS, at the tile rows the block's list names; padding pairs are dropped.  Inside an offset a tile row occurs at most
//      once, so the waves of a segment never meet in an element; the barrier that ends every segment orders the segments;
//   4. the tile is written to `out` once, as whole rows (+0 for a row without neighbours).
// Rows past n_out, channels past cin and columns past cout are zero lanes of the same body: any cin, cout >= 1, no VALU
// fallback; 16-byte loads and stores are only the fast path of aligned rows.  No atomics on floats, no counters, no scratch, no
// stream-K: one launch, capturable.
#include <vector>

#include "common.h"
#include "mfma_tile.h"
#include "conv_slab.h"
#include "conv_fwd_compact.h"

namespace {

template <int BM, int WQ>
struct CfcShape {
  static_assert(BM % 64 == 0 && BM <= 128, "a wave's ballot covers 64 rows of one offset; a tile row fits a byte");
  static_assert(WQ == 1 || WQ == 2 || WQ == 4, "four waves");
  static constexpr int WP = 4 / WQ, BN = 32 * WQ, PB = 32 * WP;
  static constexpr int BP = BN | 32;                               // floats between W rows in LDS: 32, 96, 160
  static constexpr int OP = BN + 4;                                // floats between rows of the output tile
  static constexpr int kA = PB * kDgPitch, kB = kDgKC * BP, kO = BM * OP;
  // [A 0][A 1][B 0][B 1][output tile][input row of pair j of offset k: 27 x BM][count of offset k: 32][tile row of the pair: bytes]
  static constexpr size_t kLdsBytes = (size_t)(2 * kA + 2 * kB + kO + kCfcMaxKvol * BM + 32) * 4 + (size_t)kCfcMaxKvol * BM;
};

// where the walk stands: visiting step, its offset k and pair count, block of PB pairs, chunk of cin
struct CfcWalk {
  int step, k, cnt, b, c;
};

template <int BM, int WQ, bool VEC>
__global__ __launch_bounds__(kDgThreads) void k_conv_fwd_compact(const float *__restrict__ feat, int n_in,
                                                                 const int32_t *__restrict__ nbr, int cap, int n_out,
                                                                 const float *__restrict__ W, int cin, int cout, int kvol, int subm,
                                                                 float *__restrict__ out) {
  using S = CfcShape<BM, WQ>;
  constexpr int BN = S::BN, PB = S::PB, BP = S::BP, OP = S::OP;
  extern __shared__ __attribute__((aligned(16))) float cfc_lds[];
  float *As = cfc_lds, *Bs = As + 2 * S::kA, *Os = Bs + 2 * S::kB;
  int32_t *s_in = reinterpret_cast<int32_t *>(Os + S::kO);
  int32_t *s_cnt = s_in + kCfcMaxKvol * BM;
  unsigned char *s_tr = reinterpret_cast<unsigned char *>(s_cnt + 32);
  const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6), r = lane & 31, h = lane >> 5;
  const int wp = wave / WQ, wq = wave - wp * WQ;
  const long long row0 = (long long)blockIdx.x * BM;
  const int q0 = blockIdx.y * BN;

  // ---- 1. the output tile starts at +0; the present pairs of every offset, compacted in ascending tile row
  for (int i = t; i < S::kO; i += kDgThreads) Os[i] = 0.0f;
  {
    constexpr int KPW = (kCfcMaxKvol + 3) / 4, HALVES = BM / 64;
    int v[KPW][HALVES];
#pragma unroll
    for (int i = 0; i < KPW; ++i)                              // (all of a wave's entries are in flight together)
#pragma unroll
      for (int hf = 0; hf < HALVES; ++hf) {
        const int k = wave + 4 * i;
        const long long row = row0 + hf * 64 + lane;
        v[i][hf] = (k < kvol && row < n_out) ? nbr[(size_t)k * cap + row] : -1;
      }
#pragma unroll
    for (int i = 0; i < KPW; ++i) {
      const int k = wave + 4 * i;
      if (k < kvol) {                                          // (wave-uniform)
        int base = 0;
#pragma unroll
        for (int hf = 0; hf < HALVES; ++hf) {
          const bool ok = cfc_is_nbr(v[i][hf], n_in);
          const unsigned long long bal = __ballot(ok);
          const int pos = base + __builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u));
          if (ok) {                                            // (pos < BM: at most BM rows are present)
            s_in[k * BM + pos] = v[i][hf];
            s_tr[k * BM + pos] = (unsigned char)(hf * 64 + lane);
          }
          base += __popcll(bal);
        }
        if (lane == 0) s_cnt[k] = base;
      }
    }
  }
  __syncthreads();
  const int nchunks = (cin + kDgKC - 1) / kDgKC;
  unsigned smask = 0u;                                         // bit s: the offset visited at step s has a pair in this tile
  int nseg = 0;
  for (int st = 0; st < kvol; ++st) {
    const int c = s_cnt[cfc_offset_at(st, kvol, subm)];
    if (c > 0) {
      smask |= 1u << st;
      nseg += (c + PB - 1) / PB;
    }
  }
  nseg *= nchunks;                                             // (the same in every thread of the workgroup)

  // ---- 2. the walk.  seek: the first step at or behind w.step that has pairs; none left: offset 0 with no pair
  auto seek = [&](CfcWalk &w) {
    const unsigned rest = w.step < 32 ? (smask >> w.step) << w.step : 0u;
    w.step = rest ? __ffs(rest) - 1 : kvol;
    w.k = rest ? cfc_offset_at(w.step, kvol, subm) : 0;
    w.cnt = rest ? s_cnt[w.k] : 0;
  };
  auto advance = [&](CfcWalk &w) {
    if (++w.c == nchunks) {
      w.c = 0;
      if (++w.b * PB >= w.cnt) {
        w.b = 0;
        ++w.step;
        seek(w);
      }
    }
  };
  // a segment's operands on their way from global memory to LDS: the gathered X rows and the 32 x BN piece of W[k] (item = W
  // row * (BN / 4) + q).  TWO of them: a segment is fetched two segments ahead of its MFMAs and put into LDS one ahead, so a
  // load has a whole segment and a half to land (one wave per SIMD: nothing else hides the latency, and registers are plenty)
  struct Stage {
    DgSlab<PB> a;
    float4 br[WQ];
    int bvalid[WQ];
  };
  auto fetch = [&](const CfcWalk &w, Stage &sg) {
    const int c0 = w.c * kDgKC;
#pragma unroll
    for (int i = 0; i < DgSlab<PB>::kPer; ++i) {
      const int item = t + i * kDgThreads;
      const int j = w.b * PB + (item >> 3);                    // the pair; past the count: a zero row, whatever the list holds there
      const bool live = j < w.cnt;
      const int o = s_in[w.k * BM + (j < BM - 1 ? j : BM - 1)];
      sg.a.r[i] = dg_load4<VEC>(feat + (size_t)(live ? o : 0) * (size_t)cin, c0 + 4 * (item & 7), cin);
      sg.a.valid[i] = dg_valid(c0 + 4 * (item & 7), cin, live);
    }
#pragma unroll
    for (int i = 0; i < WQ; ++i) {
      const int item = t + i * kDgThreads;
      const int ci = c0 + item / (BN / 4), col = q0 + 4 * (item % (BN / 4));
      sg.br[i] = dg_load4<VEC>(W + ((size_t)w.k * cin + (ci < cin ? ci : cin - 1)) * (size_t)cout, col, cout);
      sg.bvalid[i] = dg_valid(col, cout, ci < cin);
    }
  };
  auto put = [&](const Stage &sg, int buf) {
    sg.a.put(As + buf * S::kA, t);
    float *lds = Bs + buf * S::kB;
#pragma unroll
    for (int i = 0; i < WQ; ++i) {
      const int item = t + i * kDgThreads;
      const float x = sg.bvalid[i] > 0 ? sg.br[i].x : 0.f, y = sg.bvalid[i] > 1 ? sg.br[i].y : 0.f,
                  z = sg.bvalid[i] > 2 ? sg.br[i].z : 0.f, w = sg.bvalid[i] > 3 ? sg.br[i].w : 0.f;
      *reinterpret_cast<float4 *>(lds + (item / (BN / 4)) * BP + 4 * (item % (BN / 4))) = make_float4(x, y, z, w);
    }
  };

  f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
  CfcWalk fw = {0, 0, 0, 0, 0};                                // the segment to fetch next
  seek(fw);
  CfcWalk cw = fw;                                             // the segment on the matrix pipe
  Stage sg0, sg1;
  if (nseg > 0) {                                              // (nseg > 0: a present pair exists, so n_in > 0 and row 0 of feat is an address)
    fetch(fw, sg0);
    advance(fw);
    put(sg0, 0);
    fetch(fw, sg1);
    advance(fw);
  }
  __syncthreads();
  // As in k_conv_dgrad the fetch and the put are unconditional: the last iterations fetch past the end (the walk has run out:
  // offset 0, no live pair -- row 0 of feat and clamped rows of W[0], valid addresses) and put into the buffer nobody reads again.
  // segment s: fetch segment s + 2 into `next` (whose last content is in LDS already), MFMAs on buffer s & 1, `prev` (segment
  // s + 1) into the other buffer
  auto segment = [&](int s, Stage &next, const Stage &prev) {
    const int cur = s & 1;
    fetch(fw, next);
    advance(fw);
    __builtin_amdgcn_sched_barrier(0);
    const bool mine = cw.b * PB + wp * 32 < cw.cnt;            // (wave-uniform) some of this wave's 32 pairs exist
    if (mine) {
      float av[16], bv[16];
      dg_read16(As + cur * S::kA + (wp * 32 + r) * kDgPitch + h * (kDgKC / 2), av);
      const float *bcol = Bs + cur * S::kB + h * BP + wq * 32 + r;
#pragma unroll
      for (int st = 0; st < kDgKC / 2; ++st) bv[st] = bcol[2 * st * BP];
#pragma unroll
      for (int st = 0; st < kDgKC / 2; ++st)                   // step st: channel 2 st (lanes 0..31), then 2 st + 1 (lanes 32..63)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[st], bv[st], acc, 0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
    put(prev, cur ^ 1);                                        // (the other buffers: last read before the previous barrier)
    if (cw.c == nchunks - 1 && mine) {
      // ---- 3. the block is complete: accumulator register e of lane half h is pair rowmap(e, h) of the wave's 32, column r
      asm volatile("s_nop 15\n\ts_nop 7" ::: "memory");       // MFMA -> VALU read of the accumulator
      // The tile rows of the wave's pairs first (pairs rowmap(4 g .. 4 g + 3, h) are four consecutive bytes of the list), then
      // all sixteen elements of the tile, then the adds and the stores: written as load-after-store per element, every element
      // would wait for the one before it, because the byte list may alias the tile as far as the compiler can tell.  The sixteen
      // tile rows differ, so the order among them is free.  (j0 + 31 < BM: j0 is a multiple of 32 below the count.)
      const unsigned *trow4 = reinterpret_cast<const unsigned *>(s_tr + cw.k * BM);
      const int j0 = cw.b * PB + wp * 32;
      unsigned pk[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) pk[g] = trow4[(j0 + 8 * g + 4 * h) >> 2];
      float *p[16];
      float v[16];
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const bool live = j0 + rowmap(e, h) < cw.cnt;          // a padding pair: row 0 is read and nothing is stored
        p[e] = Os + (live ? (int)((pk[e >> 2] >> (8 * (e & 3))) & 0xffu) : 0) * OP + wq * 32 + r;
      }
#pragma unroll
      for (int e = 0; e < 16; ++e) v[e] = *p[e];
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        if (j0 + rowmap(e, h) < cw.cnt) *p[e] = cfc_add(v[e], acc[e]);
        acc[e] = 0.0f;
      }
    }
    advance(cw);
    __syncthreads();
  };
  // Segments go in PAIRS, the second one unconditionally: under `if (s + 1 < nseg)` the compiler folds the pair back into one
  // segment per iteration whose two stages swap through register copies, and the copies wait for every load in flight.  An odd
  // nseg ends with one empty segment: the walk has run out (no live pair: no MFMAs, nothing added), one barrier more.
  for (int s = 0; s < nseg; s += 2) {                          // (nseg is the same in every thread of the workgroup)
    segment(s, sg0, sg1);
    segment(s + 1, sg1, sg0);
  }

  // ---- 4. whole rows of the tile, once
  for (int item = t; item < BM * (BN / 4); item += kDgThreads) {
    const int rr = item / (BN / 4), c4 = 4 * (item % (BN / 4));
    const long long row = row0 + rr;
    const int col = q0 + c4;
    if (row < n_out && col < cout) {
      const float4 v = *reinterpret_cast<const float4 *>(Os + rr * OP + c4);
      float *dst = out + (size_t)row * (size_t)cout + col;
      if constexpr (VEC) {
        *reinterpret_cast<float4 *>(dst) = v;
      } else {
        dst[0] = v.x;
        if (col + 1 < cout) dst[1] = v.y;
        if (col + 2 < cout) dst[2] = v.z;
        if (col + 3 < cout) dst[3] = v.w;
      }
    }
  }
}

template <int BM, int WQ>
void launch_cfc(hipStream_t s, const float *feat, int n_in, const int32_t *nbr, int cap, int n_out, const float *W, int cin,
                int cout, int kvol, int subm, float *out) {
  using S = CfcShape<BM, WQ>;
  const dim3 grid(dcl_div_up(n_out, BM), dcl_div_up(cout, S::BN));
  // 16-byte loads and stores where every row of feat, of W and of out starts on a 16-byte boundary
  const bool vec = (((size_t)feat | (size_t)W | (size_t)out) & 15) == 0 && (cin & 3) == 0 && (cout & 3) == 0;
  if (vec) {
    (void)hipFuncSetAttribute((const void *)k_conv_fwd_compact<BM, WQ, true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)S::kLdsBytes);
    hipLaunchKernelGGL((k_conv_fwd_compact<BM, WQ, true>), grid, dim3(kDgThreads), S::kLdsBytes, s, feat, n_in, nbr, cap, n_out, W,
                       cin, cout, kvol, subm, out);
  } else {
    (void)hipFuncSetAttribute((const void *)k_conv_fwd_compact<BM, WQ, false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)S::kLdsBytes);
    hipLaunchKernelGGL((k_conv_fwd_compact<BM, WQ, false>), grid, dim3(kDgThreads), S::kLdsBytes, s, feat, n_in, nbr, cap, n_out, W,
                       cin, cout, kvol, subm, out);
  }
}

bool cfc_aligned4(const void *p) { return ((size_t)p & 3) == 0; }

#if !defined(__HIP_DEVICE_COMPILE__)
// The host twin's rows: conv_fwd_compact.h's steps in conv_fwd_compact.h's order.  The innermost loop runs over the cout
// INDEPENDENT chains of an offset (W's contiguous axis); each of them takes its channels ascending.
__attribute__((always_inline)) inline void cfc_host_rows(const float *feat, int n_in, const int32_t *nbr, int cap, int n_out,
                                                         const float *W, int cin, int cout, int kvol, int subm, float *part,
                                                         float *out) {
  for (int o = 0; o < n_out; ++o) {
    float *a = out + (size_t)o * cout;
    for (int co = 0; co < cout; ++co) a[co] = 0.0f;
    for (int st = 0; st < kvol; ++st) {
      const int k = cfc_offset_at(st, kvol, subm);
      const int v = nbr[(size_t)k * cap + o];
      if (!cfc_is_nbr(v, n_in)) continue;
      const float *x = feat + (size_t)v * cin, *wk = W + (size_t)k * cin * cout;
      for (int co = 0; co < cout; ++co) part[co] = 0.0f;
      for (int ci = 0; ci < cin; ++ci) {
        const float xv = x[ci];
        const float *w = wk + (size_t)ci * cout;
        for (int co = 0; co < cout; ++co) part[co] = cfc_step(part[co], xv, w[co]);
      }
      for (int co = 0; co < cout; ++co) a[co] = cfc_add(a[co], part[co]);
    }
  }
}
void cfc_host_rows_plain(const float *feat, int n_in, const int32_t *nbr, int cap, int n_out, const float *W, int cin, int cout,
                         int kvol, int subm, float *part, float *out) {
  cfc_host_rows(feat, n_in, nbr, cap, n_out, W, cin, cout, kvol, subm, part, out);
}
#if defined(__x86_64__)
// the same steps where the processor has a fused multiply-add of its own: fmaf is one instruction instead of a library call
__attribute__((target("avx2,fma"))) void cfc_host_rows_fma(const float *feat, int n_in, const int32_t *nbr, int cap, int n_out,
                                                           const float *W, int cin, int cout, int kvol, int subm, float *part,
                                                           float *out) {
  cfc_host_rows(feat, n_in, nbr, cap, n_out, W, cin, cout, kvol, subm, part, out);
}
#endif
#endif

// rows per tile: 0 = by the layer's width (below), 64 or 128 = forced (diagnostic library: tools/bench_conv_fwd.py)
DCL_HOOK_INT(g_cfc_bm, 0);

}  // namespace

#ifdef DCL_DIAG
DCL_API void dcl_debug_conv_fwd_compact_bm(int bm) { g_cfc_bm = bm; }
#endif

#define DCL_CONV_FWD_COMPACT_CHECK()                                                                                        \
  DCL_CHECK_ARG(kvol >= 1 && kvol <= kCfcMaxKvol && n_in >= 0 && n_out >= 0 && cin >= 1 && cout >= 1 && cap >= n_out);      \
  DCL_CHECK_ARG(n_in < (1 << 30) && n_out < (1 << 30) && (long long)cin * cout < (1ll << 31) / 27);                         \
  DCL_CHECK_ARG(W && cfc_aligned4(W) && (n_in == 0 || (feat && cfc_aligned4(feat))));                                       \
  DCL_CHECK_ARG(n_out == 0 || (nbr && out && cfc_aligned4(nbr) && cfc_aligned4(out)))

DCL_API int dcl_sparse_conv_fwd_compact(const float *feat, int n_in, const int32_t *nbr, int cap, int n_out, const float *W,
                                        int cin, int cout, int kvol, int subm, float *out, dclStream_t stream) {
  DCL_CONV_FWD_COMPACT_CHECK();
  if (n_out == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  subm = subm ? 1 : 0;
  // the four waves tile (pairs, columns): up to 32 columns 128 pairs x 32, up to 64 columns 64 x 64, wider layers 32 pairs x
  // 128 columns per pass.  Rows per tile: profiles/conv_fwd_compact.txt
  const int bm = (int)g_cfc_bm == 64 || (int)g_cfc_bm == 128 ? (int)g_cfc_bm : (cout <= 32 ? 128 : 64);
#define CFC_LAUNCH(BM_)                                                                                                     \
  do {                                                                                                                      \
    if (cout <= 32) launch_cfc<BM_, 1>(s, feat, n_in, nbr, cap, n_out, W, cin, cout, kvol, subm, out);                      \
    else if (cout <= 64) launch_cfc<BM_, 2>(s, feat, n_in, nbr, cap, n_out, W, cin, cout, kvol, subm, out);                 \
    else launch_cfc<BM_, 4>(s, feat, n_in, nbr, cap, n_out, W, cin, cout, kvol, subm, out);                                 \
  } while (0)
  if (bm == 128) CFC_LAUNCH(128);
  else CFC_LAUNCH(64);
#undef CFC_LAUNCH
  DCL_LAUNCH_CHECK();
  return 0;
}

DCL_API int dcl_sparse_conv_fwd_compact_host(const float *feat, int n_in, const int32_t *nbr, int cap, int n_out, const float *W,
                                             int cin, int cout, int kvol, int subm, float *out) {
  DCL_CONV_FWD_COMPACT_CHECK();
#if !defined(__HIP_DEVICE_COMPILE__)
  if (n_out == 0) return 0;
  std::vector<float> part((size_t)cout);
#if defined(__x86_64__)
  if (__builtin_cpu_supports("avx2") && __builtin_cpu_supports("fma")) {
    cfc_host_rows_fma(feat, n_in, nbr, cap, n_out, W, cin, cout, kvol, subm ? 1 : 0, part.data(), out);
    return 0;
  }
#endif
  cfc_host_rows_plain(feat, n_in, nbr, cap, n_out, W, cin, cout, kvol, subm ? 1 : 0, part.data(), out);
#endif
  return 0;
}
