// conv_wgrad_pairs.hip -- the sparse-conv weight gradient over the rulebook's PAIRS (ops.sparse_conv_backward(wgrad="pairs")),
// beside the row-walking form of backward.hip, which stays the default.
//
// dcl_conv_pairs: the ordered pair list of a gather table.  (k, o) is a pair iff o < n_out and 0 <= nbr[k][o] < n_in.  Three
//   launches, all prefix sums -- no atomic, no workgroup waits on another:
//     k_pairs_count   one workgroup per (chunk of kPairChunk rows, offset): how many pairs the chunk holds
//     k_pairs_scan    one workgroup per offset: the chunk counts -> their exclusive prefix (in place) and count[k]
//     k_pairs_place   one workgroup per (chunk, offset): start[k] from count[0 .. k), then the chunk's pairs to
//                     start[k] + prefix[chunk] + (rank inside the chunk, by ballots): ascending o.  The chunk-0 workgroup of an
//                     offset also writes start[k] and the offset's rows of the split table.
//   A pair at position >= max_pairs is not stored (head[61] says how many); the split table covers the stored pairs only.
// dcl_sparse_conv_wgrad_pairs: dW[k] = sum over the pairs of X[pair_in]^T dO[pair_out] on v_mfma_f32_32x32x2_f32 in the
//   transposed-A form of k_linear_wgrad (linear_bwd.hip): lane l of BOTH operands holds element [pair 2s + (l >> 5)][col l & 31],
//   so the gathered rows go to LDS as they lie.  A workgroup owns WS splits and one (cin, cout) tile; the WP x WQ waves of a split
//   tile (cin, cout), never the pairs -- an output element is ONE accumulator fed by its split's pairs ascending.  16-pair slabs,
//   global -> registers -> LDS, two LDS buffers: the next slab's rows fly under this slab's MFMAs, and its pair indices were
//   fetched one slab earlier.  LDS rows have the tile's width as their pitch: a ds_read_b32 serves its two 32-lane halves in
//   turn (pair 2s and pair 2s + 1: 32 consecutive floats each, 32 banks), and the float4 writes of a slab are contiguous.
//   k_pairs_split_sum then adds each offset's splits ascending and writes every element of dW (+0 for an offset without pairs).
#include "common.h"
#include "mfma_tile.h"

namespace {

constexpr int kPairChunk = 1024;       // rows of one (chunk, offset) workgroup: 4 rounds of 256
constexpr int kPairThreads = 256;
constexpr int kHeadStart = 32, kHeadNsplit = 60, kHeadOverflow = 61, kHeadFirstSplit = 64;

__device__ __forceinline__ bool pair_ok(int v, int n_in) { return (unsigned)v < (unsigned)n_in; }

// exclusive prefix of `v` over the workgroup's kPairThreads threads; *total = the sum.  tmp: kPairThreads / 64 + 1 ints of LDS
__device__ __forceinline__ int block_excl_scan(int v, int *tmp, int *total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int u = __shfl_up(inc, d, 64);
    if (lane >= d) inc += u;
  }
  __syncthreads();                                           // (tmp may still be read by the previous call)
  if (lane == 63) tmp[wave] = inc;
  __syncthreads();
  int off = 0, all = 0;
#pragma unroll
  for (int w = 0; w < kPairThreads / 64; ++w) {
    const int t = tmp[w];
    off += w < wave ? t : 0;
    all += t;
  }
  *total = all;
  return off + inc - v;
}

__global__ __launch_bounds__(kPairThreads) void k_pairs_count(const int32_t *__restrict__ nbr, int cap, int n_out, int n_in,
                                                              int nchunks, int32_t *__restrict__ cnt) {
  __shared__ int tmp[kPairThreads / 64 + 1];
  const int chunk = blockIdx.x, k = blockIdx.y;
  int mine = 0;
#pragma unroll
  for (int r = 0; r < kPairChunk / kPairThreads; ++r) {
    const int o = chunk * kPairChunk + r * kPairThreads + threadIdx.x;
    if (o < n_out) mine += pair_ok(nbr[(size_t)k * cap + o], n_in) ? 1 : 0;
  }
  int total;
  (void)block_excl_scan(mine, tmp, &total);
  if (threadIdx.x == 0) cnt[(size_t)k * nchunks + chunk] = total;
}

__global__ __launch_bounds__(kPairThreads) void k_pairs_scan(int nchunks, int32_t *__restrict__ cnt, int32_t *__restrict__ head) {
  __shared__ int tmp[kPairThreads / 64 + 1];
  const int k = blockIdx.x;
  int32_t *c = cnt + (size_t)k * nchunks;
  const int per = (nchunks + kPairThreads - 1) / kPairThreads;           // a thread owns `per` consecutive chunks
  const int lo = threadIdx.x * per, hi = lo + per < nchunks ? lo + per : nchunks;
  int mine = 0;
  for (int i = lo; i < hi; ++i) mine += c[i];
  int total;
  int run = block_excl_scan(mine, tmp, &total);
  for (int i = lo; i < hi; ++i) {
    const int v = c[i];
    c[i] = run;
    run += v;
  }
  if (threadIdx.x == 0) head[k] = total;
}

__global__ __launch_bounds__(kPairThreads) void k_pairs_place(const int32_t *__restrict__ nbr, int cap, int kvol, int n_out,
                                                              int n_in, int max_pairs, int nchunks,
                                                              const int32_t *__restrict__ cnt, int32_t *__restrict__ head,
                                                              int32_t *__restrict__ pair_in, int32_t *__restrict__ pair_out,
                                                              int32_t *__restrict__ split_tab) {
  __shared__ int tmp[kPairThreads / 64 + 1];
  constexpr int S = DCL_CONV_PAIRS_SPLIT;
  const int chunk = blockIdx.x, k = blockIdx.y;
  // start[k] and the first split of offset k from the counts in front of it (27 at the most; the same in every thread)
  long long start = 0;
  int first_split = 0;
  for (int j = 0; j < k; ++j) {
    const int c = head[j];
    const long long room = (long long)max_pairs - start;
    const int stored = room <= 0 ? 0 : (room < c ? (int)room : c);
    first_split += (stored + S - 1) / S;
    start += c;
  }
  if (chunk == 0) {
    const int c = head[k];
    const long long room = (long long)max_pairs - start;
    const int stored = room <= 0 ? 0 : (room < c ? (int)room : c);
    const int ns = (stored + S - 1) / S;
    for (int s = threadIdx.x; s < ns; s += kPairThreads) {
      const int len = stored - s * S < S ? stored - s * S : S;
      reinterpret_cast<int4 *>(split_tab)[first_split + s] = make_int4(k, (int)start + s * S, len, 0);
    }
    if (threadIdx.x == 0) {
      head[kHeadStart + k] = (int)start;
      head[kHeadFirstSplit + k] = first_split;
      if (k == kvol - 1) {
        const long long all = start + c;
        head[kHeadStart + kvol] = (int)all;
        head[kHeadFirstSplit + kvol] = first_split + ns;
        head[kHeadNsplit] = first_split + ns;
        head[kHeadOverflow] = all > max_pairs ? (int)(all - max_pairs) : 0;
      }
    }
  }
  long long pos = start + cnt[(size_t)k * nchunks + chunk];
#pragma unroll 1
  for (int r = 0; r < kPairChunk / kPairThreads; ++r) {
    const int o = chunk * kPairChunk + r * kPairThreads + threadIdx.x;
    const int v = o < n_out ? nbr[(size_t)k * cap + o] : -1;
    const bool ok = pair_ok(v, n_in);
    int total;
    const long long p = pos + block_excl_scan(ok ? 1 : 0, tmp, &total);
    if (ok && p < max_pairs) {
      pair_in[p] = v;
      pair_out[p] = o;
    }
    pos += total;
  }
}

// ---- the weight gradient -----------------------------------------------------------------------------------------------------
constexpr int kCpKC = 16;            // pairs per LDS slab (8 MFMA k-steps)
constexpr int kCpThreads = 256;

// 4 consecutive floats, columns c .. c + 3, of a row of `cols` floats; 0 past the row's end
__device__ __forceinline__ float4 cp_load4(const float *row, int c, int cols, bool vec_ok) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (c >= cols) return v;
  if (vec_ok && c + 3 < cols) return *reinterpret_cast<const float4 *>(row + c);
  v.x = row[c];
  if (c + 1 < cols) v.y = row[c + 1];
  if (c + 2 < cols) v.z = row[c + 2];
  if (c + 3 < cols) v.w = row[c + 3];
  return v;
}

// one operand's slab of kCpKC gathered rows x W columns, staged by the TG threads of a split's group
template <int W, int TG>
struct CpSlab {
  static constexpr int kItems = kCpKC * W / 4;                                 // float4 items
  static constexpr int kPer = (kItems + TG - 1) / TG;
  int idx[kPer];                                                               // the row of each item, of the slab to fetch next
  float4 r[kPer];
  // the rows of the slab whose first pair is p0 (pairs at or past p_hi: none)
  __device__ __forceinline__ void load_idx(const int32_t *__restrict__ list, int p0, int p_hi, int tg) {
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
      const int item = tg + i * TG;
      const int p = p0 + item / (W / 4);
      idx[i] = (item < kItems && p < p_hi) ? list[p] : -1;
    }
  }
  __device__ __forceinline__ void fetch(const float *__restrict__ m, int nrows, int c0, int cols, bool vec_ok, int tg) {
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
      const int item = tg + i * TG;
      const int c4 = (item % (W / 4)) * 4;
      r[i] = (unsigned)idx[i] < (unsigned)nrows ? cp_load4(m + (size_t)idx[i] * (size_t)cols, c0 + c4, cols, vec_ok)
                                               : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  __device__ __forceinline__ void put(float *lds, int tg) const {
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
      const int item = tg + i * TG;
      if (item < kItems) *reinterpret_cast<float4 *>(lds + item * 4) = r[i];   // (pitch W: item * 4 = row * W + c4)
    }
  }
};

// WS splits per workgroup, each with WP x WQ waves of TP x TQ accumulator tiles of 32 x 32: the tile is (32 WP TP) x (32 WQ TQ)
template <int WS, int WP, int WQ, int TP, int TQ>
__global__ __launch_bounds__(kCpThreads) void k_conv_wgrad_pairs(const float *__restrict__ feat, int n_in,
                                                                 const float *__restrict__ dout, int n_out, int cin, int cout,
                                                                 const int32_t *__restrict__ head,
                                                                 const int32_t *__restrict__ pair_in,
                                                                 const int32_t *__restrict__ pair_out,
                                                                 const int32_t *__restrict__ split_tab, int max_splits, int tiles_p,
                                                                 int tiles_q, float *__restrict__ partial) {
  static_assert(WS * WP * WQ * 64 == kCpThreads, "four waves");
  constexpr int BP = 32 * WP * TP, BQ = 32 * WQ * TQ, TG = kCpThreads / WS;
  __shared__ __attribute__((aligned(16))) float As[WS][2][kCpKC * BP];
  __shared__ __attribute__((aligned(16))) float Bs[WS][2][kCpKC * BQ];
  const int tiles = tiles_p * tiles_q;
  const int sblock = blockIdx.x / tiles, tile = blockIdx.x - sblock * tiles;
  const int nsplit = head[kHeadNsplit] < max_splits ? head[kHeadNsplit] : max_splits;
  if (sblock * WS >= nsplit) return;                                           // workgroup-uniform
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
  const int grp = wave / (WP * WQ), wl = wave - grp * (WP * WQ), tg = threadIdx.x - grp * TG;
  const int wp = wl / WQ, wq = wl - wp * WQ;
  const int tp = tile / tiles_q, tq = tile - tp * tiles_q;
  const int p0 = tp * BP, q0 = tq * BQ;
  // this group's split, and the longest of the workgroup's (the barriers run that many times)
  const int g = sblock * WS + grp;
  int first = 0, len = 0, max_len = 0;
#pragma unroll
  for (int i = 0; i < WS; ++i) {
    const int gi = sblock * WS + i;
    const int4 row = gi < nsplit ? reinterpret_cast<const int4 *>(split_tab)[gi] : make_int4(0, 0, 0, 0);
    if (i == grp) { first = row.y; len = row.z; }
    max_len = row.z > max_len ? row.z : max_len;
  }
  const int p_hi = first + len;
  const int my_chunks = (len + kCpKC - 1) / kCpKC, nchunks = (max_len + kCpKC - 1) / kCpKC;
  const bool vec_a = (((size_t)feat & 15) == 0) && (cin & 3) == 0, vec_b = (((size_t)dout & 15) == 0) && (cout & 3) == 0;

  f32x16 acc[TP][TQ];
#pragma unroll
  for (int i = 0; i < TP; ++i)
#pragma unroll
    for (int j = 0; j < TQ; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;

  CpSlab<BP, TG> sa;
  CpSlab<BQ, TG> sb;
  sa.load_idx(pair_in, first, p_hi, tg);
  sb.load_idx(pair_out, first, p_hi, tg);
  sa.fetch(feat, n_in, p0, cin, vec_a, tg);
  sb.fetch(dout, n_out, q0, cout, vec_b, tg);
  sa.load_idx(pair_in, first + kCpKC, p_hi, tg);
  sb.load_idx(pair_out, first + kCpKC, p_hi, tg);
  sa.put(As[grp][0], tg);
  sb.put(Bs[grp][0], tg);
  __syncthreads();
  for (int c = 0; c < nchunks; ++c) {
    const int cur = c & 1;
    if (c + 1 < nchunks) {                                   // the next slab's rows fly during this slab's MFMAs ...
      sa.fetch(feat, n_in, p0, cin, vec_a, tg);
      sb.fetch(dout, n_out, q0, cout, vec_b, tg);
      sa.load_idx(pair_in, first + (c + 2) * kCpKC, p_hi, tg);                 // ... and the indices of the one after it
      sb.load_idx(pair_out, first + (c + 2) * kCpKC, p_hi, tg);
    }
    if (c < my_chunks) {                                     // (wave-uniform: a shorter split of the workgroup is done)
      const float *A = As[grp][cur] + h * BP + wp * (32 * TP) + r;
      const float *B = Bs[grp][cur] + h * BQ + wq * (32 * TQ) + r;
#pragma unroll
      for (int s = 0; s < kCpKC / 2; ++s) {                  // k-step s: pairs 2s (lanes 0..31) and 2s + 1 (lanes 32..63), ascending
        float av[TP], bv[TQ];
#pragma unroll
        for (int i = 0; i < TP; ++i) av[i] = A[2 * s * BP + 32 * i];
#pragma unroll
        for (int j = 0; j < TQ; ++j) bv[j] = B[2 * s * BQ + 32 * j];
#pragma unroll
        for (int i = 0; i < TP; ++i)
#pragma unroll
          for (int j = 0; j < TQ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[j], acc[i][j], 0, 0, 0);
      }
    }
    if (c + 1 < nchunks) {                                   // (the other buffer: last read before the previous barrier)
      sa.put(As[grp][cur ^ 1], tg);
      sb.put(Bs[grp][cur ^ 1], tg);
    }
    __syncthreads();
  }
  if (g >= nsplit) return;
  // accumulator register e of lane half h: output row rowmap(e, h), column lane & 31
  float *out = partial + (size_t)g * (size_t)cin * (size_t)cout;
#pragma unroll
  for (int i = 0; i < TP; ++i)
#pragma unroll
    for (int j = 0; j < TQ; ++j) {
      const int q = q0 + wq * (32 * TQ) + 32 * j + r;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int p = p0 + wp * (32 * TP) + 32 * i + rowmap(e, h);
        if (p < cin && q < cout) out[(size_t)p * cout + q] = acc[i][j][e];
      }
    }
}

// dW[k][e] = the splits of offset k, ascending, from the first one's value (no split: +0)
__global__ __launch_bounds__(256) void k_pairs_split_sum(const float *__restrict__ partial, const int32_t *__restrict__ head,
                                                         int max_splits, int kvol, int n /* cin * cout */,
                                                         float *__restrict__ dW) {
  const long long all = (long long)kvol * n;
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < all; t += (long long)gridDim.x * blockDim.x) {
    const int k = (int)(t / n), e = (int)(t - (long long)k * n);
    const int s0 = head[kHeadFirstSplit + k];
    const int s1 = head[kHeadFirstSplit + k + 1] < max_splits ? head[kHeadFirstSplit + k + 1] : max_splits;
    float a = s0 < s1 ? partial[(size_t)s0 * n + e] : 0.0f;
    for (int z = s0 + 1; z < s1; ++z) a = a + partial[(size_t)z * n + e];
    dW[t] = a;
  }
}

bool aligned4(const void *p) { return ((size_t)p & 3) == 0; }
int pair_chunks(int n_out) { return n_out > 0 ? dcl_div_up(n_out, kPairChunk) : 1; }

template <int WS, int WP, int WQ, int TP, int TQ>
int launch_wgrad_pairs(hipStream_t s, const float *feat, int n_in, const float *dout, int n_out, int cin, int cout,
                       const int32_t *head, const int32_t *pair_in, const int32_t *pair_out, const int32_t *split_tab,
                       int max_splits, float *partial) {
  const int tiles_p = dcl_div_up(cin, 32 * WP * TP), tiles_q = dcl_div_up(cout, 32 * WQ * TQ);
  const long long grid = (long long)tiles_p * tiles_q * dcl_div_up(max_splits, WS);
  if (grid >= (1ll << 31)) return -1;
  hipLaunchKernelGGL((k_conv_wgrad_pairs<WS, WP, WQ, TP, TQ>), dim3((unsigned)grid), dim3(kCpThreads), 0, s, feat, n_in, dout,
                     n_out, cin, cout, head, pair_in, pair_out, split_tab, max_splits, tiles_p, tiles_q, partial);
  return 0;
}

}  // namespace

DCL_API int dcl_conv_pairs_ws_bytes(int kvol, int n_out, int64_t *bytes_host) {
  DCL_CHECK_ARG(kvol >= 1 && kvol <= 27 && n_out >= 0 && bytes_host);
  *bytes_host = (int64_t)4 * kvol * pair_chunks(n_out);
  return 0;
}

DCL_API int dcl_conv_pairs_max_splits(int max_pairs, int kvol, int32_t *splits_host) {
  DCL_CHECK_ARG(max_pairs >= 0 && max_pairs < (1 << 30) && kvol >= 1 && kvol <= 27 && splits_host);
  *splits_host = max_pairs / DCL_CONV_PAIRS_SPLIT + kvol;
  return 0;
}

#define DCL_CONV_PAIRS_CHECK()                                                                                              \
  DCL_CHECK_ARG(kvol >= 1 && kvol <= 27 && n_out >= 0 && n_in >= 0 && cap >= n_out && cap >= 1);                            \
  DCL_CHECK_ARG(max_pairs >= 0 && max_pairs < (1 << 30) && (long long)kvol * n_out < (1ll << 31));                          \
  DCL_CHECK_ARG(nbr && head && split_tab && aligned4(nbr) && aligned4(head) && ((size_t)split_tab & 15) == 0);              \
  DCL_CHECK_ARG(max_pairs == 0 || (pair_in && pair_out && aligned4(pair_in) && aligned4(pair_out)))

DCL_API int dcl_conv_pairs(const int32_t *nbr, int cap, int kvol, int n_out, int n_in, int max_pairs, int32_t *head,
                           int32_t *pair_in, int32_t *pair_out, int32_t *split_tab, void *ws, int64_t ws_bytes,
                           dclStream_t stream) {
  DCL_CONV_PAIRS_CHECK();
  const int nchunks = pair_chunks(n_out);
  DCL_CHECK_ARG(ws && aligned4(ws) && ws_bytes >= (int64_t)4 * kvol * nchunks);
  hipStream_t s = (hipStream_t)stream;
  int32_t *cnt = (int32_t *)ws;
  hipLaunchKernelGGL(k_pairs_count, dim3(nchunks, kvol), dim3(kPairThreads), 0, s, nbr, cap, n_out, n_in, nchunks, cnt);
  hipLaunchKernelGGL(k_pairs_scan, dim3(kvol), dim3(kPairThreads), 0, s, nchunks, cnt, head);
  hipLaunchKernelGGL(k_pairs_place, dim3(nchunks, kvol), dim3(kPairThreads), 0, s, nbr, cap, kvol, n_out, n_in, max_pairs,
                     nchunks, cnt, head, pair_in, pair_out, split_tab);
  DCL_LAUNCH_CHECK();
  return 0;
}

DCL_API int dcl_conv_pairs_host(const int32_t *nbr, int cap, int kvol, int n_out, int n_in, int max_pairs, int32_t *head,
                                int32_t *pair_in, int32_t *pair_out, int32_t *split_tab) {
  DCL_CONV_PAIRS_CHECK();
  constexpr int S = DCL_CONV_PAIRS_SPLIT;
  long long pos = 0;
  int nsplit = 0;
  for (int k = 0; k < kvol; ++k) {
    const long long start = pos;
    for (int o = 0; o < n_out; ++o) {
      const int v = nbr[(size_t)k * cap + o];
      if (v < 0 || v >= n_in) continue;
      if (pos < max_pairs) {
        pair_in[pos] = v;
        pair_out[pos] = o;
      }
      ++pos;
    }
    const int count = (int)(pos - start);
    const long long room = (long long)max_pairs - start;
    const int stored = room <= 0 ? 0 : (room < count ? (int)room : count);
    head[k] = count;
    head[kHeadStart + k] = (int)start;
    head[kHeadFirstSplit + k] = nsplit;
    for (int f = 0; f < stored; f += S, ++nsplit) {
      int32_t *row = split_tab + (size_t)4 * nsplit;
      row[0] = k;
      row[1] = (int)start + f;
      row[2] = stored - f < S ? stored - f : S;
      row[3] = 0;
    }
  }
  head[kHeadStart + kvol] = (int)pos;
  head[kHeadFirstSplit + kvol] = nsplit;
  head[kHeadNsplit] = nsplit;
  head[kHeadOverflow] = pos > max_pairs ? (int)(pos - max_pairs) : 0;
  return 0;
}

DCL_API int dcl_sparse_conv_wgrad_pairs(const float *feat, int n_in, const float *dout, int n_out, int cin, int cout, int kvol,
                                        const int32_t *head, const int32_t *pair_in, const int32_t *pair_out,
                                        const int32_t *split_tab, int max_splits, float *partial, float *dW,
                                        dclStream_t stream) {
  DCL_CHECK_ARG(kvol >= 1 && kvol <= 27 && n_in >= 0 && n_out >= 0 && cin >= 1 && cout >= 1 && max_splits >= 1);
  DCL_CHECK_ARG((long long)cin * cout < (1ll << 31) / 27);
  DCL_CHECK_ARG(head && split_tab && partial && dW && aligned4(head) && ((size_t)split_tab & 15) == 0 && aligned4(partial) &&
                aligned4(dW));
  DCL_CHECK_ARG(pair_in && pair_out && aligned4(pair_in) && aligned4(pair_out));
  DCL_CHECK_ARG((n_in == 0 || (feat && aligned4(feat))) && (n_out == 0 || (dout && aligned4(dout))));
  hipStream_t s = (hipStream_t)stream;
  int rc;
#define DCL_WP_LAUNCH(WS, WP, WQ, TP, TQ)                                                                                   \
  rc = launch_wgrad_pairs<WS, WP, WQ, TP, TQ>(s, feat, n_in, dout, n_out, cin, cout, head, pair_in, pair_out, split_tab,    \
                                              max_splits, partial)
  if (cin <= 32 && cout <= 32) DCL_WP_LAUNCH(4, 1, 1, 1, 1);                   // 32 x 32: a wave's work -- four splits per workgroup
  else if (cin <= 32 && cout <= 64) DCL_WP_LAUNCH(2, 1, 2, 1, 1);              // 32 x 64: two splits of two waves
  else if (cin <= 64 && cout <= 64) DCL_WP_LAUNCH(1, 2, 2, 1, 1);              // 64 x 64
  else if (cin <= 64) DCL_WP_LAUNCH(1, 2, 2, 1, 2);                            // 64 x 128
  else DCL_WP_LAUNCH(1, 2, 2, 2, 2);                                           // 128 x 128
#undef DCL_WP_LAUNCH
  DCL_CHECK_ARG(rc == 0 && "grid");
  hipLaunchKernelGGL(k_pairs_split_sum, dim3(dcl_grid_1d((long long)kvol * cin * cout, 256)), dim3(256), 0, s, partial, head,
                     max_splits, kvol, cin * cout, dW);
  DCL_LAUNCH_CHECK();
  return 0;
}
