/*
 * dclnet_hip.h -- C ABI of libdclnet_hip.so: the MI355X (gfx950) kernels of
 * DCL-Net's per-crop RGB-D -> 6-DoF pose forward.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless its name ends in _host;
 *   - `stream` is a hipStream_t passed as void* (0 = the null stream); every
 *     call only enqueues work on it -- no allocation, no synchronisation, no
 *     host read-back (graph-capture safe) unless stated;
 *   - return value: 0 on success, otherwise a hipError_t (>0) or
 *     DCL_EINVAL (-1) for bad arguments; dcl_last_error() gives the text.
 *     (The reference's launchers print to stderr and exit(-1), e.g.
 *     libs/pointnet_lib/src/ball_query_gpu.cu:62-66; a library must not.)
 *   - layouts are the reference's: row-major fp32 / int32.
 *
 * Each entry point cites the reference interface it replaces (paths relative
 * to the upstream repository).  INTEGRATION.md shows the binding a maintainer
 * would add on the reference side.
 */
#ifndef DCLNET_HIP_H_
#define DCLNET_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DCL_EINVAL (-1)
typedef void *dclStream_t;

const char *dcl_last_error(void);
/* Version of THIS header's C ABI; a caller built against another version must not call in (dcl-net_amd/_native.py refuses to).
 *   1  rounds 1-4
 *   2  round 5-6: dcl_crop_points gained `int32_t *ws` in front of `stream`; dcl_backbone_features_stage,
 *      dcl_backbone_stage_ws_bytes and DCL_ESTAGE_UNSUPPORTED are gone; dcl_linear_fwd ignores its workspace arguments;
 *      new: dcl_linear_dma_fwd, dcl_linear_pool_fwd, dcl_linear_rowdot_fwd, dcl_conf_softmax, dcl_pool_finish2,
 *      dcl_linear_split_weight(_bytes), dcl_linear_split_fwd / _pool_fwd / _rowdot_fwd / _vpieces_fwd, dcl_cross_attention_ws3
 *      (+ _planes_bytes, _split_crops); later additions (no change to existing entries): dcl_conv_split_weight(_bytes),
 *      dcl_sparse_conv_fwd_sides, dcl_backbone_features_split / _cap_split / _pair_split, dcl_point_features_fold,
 *      dcl_linear_split_gather_fwd, dcl_linear_wgrad_split */
#define DCL_ABI_VERSION 2
int dcl_abi_version(void);

/* ------------------------------------------------------------------ PG_OP ---
 * voxelize_idx: libs/pointgroup_ops/src/pointgroup_ops_api.cpp:6 ->
 * src/voxelize/voxelize.cpp:10-152.  HOST function (the reference runs it in
 * DataLoader workers, YCBV/dataloader_test_YCBV.py:217,223).  Two calls, like
 * the reference's resize-in-place protocol split in two: _count fills
 * input_map and returns sizes, _fill writes the caller-allocated (zeroed)
 * outputs.  All five modes of voxelize.cpp:111-149: 0 = guaranteed unique (an
 * error here, an assert there, if not), 1 = the voxel's first point, 2 = its last
 * point (max_active == 1, rows [1, point]), 3 (sum) / 4 (mean) = every point.
 * dcl_voxelize_idx_fill is _fill_mode with mode 4.                              */
int dcl_voxelize_idx_count(const int64_t *coords_host, int n, int ncol, int batch_size, int mode,
                           int32_t *input_map_host, int32_t *n_active_host, int32_t *max_active_host);
int dcl_voxelize_idx_fill(const int64_t *coords_host, int n, int ncol, const int32_t *input_map_host,
                          int n_active, int max_active, int64_t *output_coords_host,
                          int32_t *output_map_host);
int dcl_voxelize_idx_fill_mode(const int64_t *coords_host, int n, int ncol, const int32_t *input_map_host,
                               int n_active, int max_active, int mode, int64_t *output_coords_host,
                               int32_t *output_map_host);

/* DEVICE voxelize_idx (same results as the host one, coords on the GPU inside a batch x S^3 grid).
 * _count: input_map (n) and info_dev = {n_active, max_active, error flag (coordinate out of range)}; the caller reads
 * info back (one sync) to allocate output_coords (V,4) i64 / output_map (V, max_active+1) i32, then calls _fill.     */
int dcl_voxelize_idx_gpu_ws_bytes(int n, int batch, int S, int64_t *bytes_host);
int dcl_voxelize_idx_gpu_count(const int64_t *coords, int n, int batch, int S, int mode, void *ws, int64_t ws_bytes,
                               int32_t *input_map, int32_t *info_dev, dclStream_t stream);
int dcl_voxelize_idx_gpu_fill(const int64_t *coords, int n, int batch, int S, void *ws, const int32_t *input_map,
                              int n_active, int max_active, int64_t *output_coords, int32_t *output_map,
                              dclStream_t stream);
/* The crop builder's case of the above in ONE launch and without a host read-back (the loader voxelises the
 * b x n sampled points of an image's crops, YCBV/dataloader_test_YCBV.py:213-223): b <= 64 crops of n_per <= 1024 points each
 * (rows c*n_per .. belong to crop c) on 64^3 grids, one workgroup per crop.  Outputs are CAPACITY-pitched: output_map rows of
 * `pitch` ints (1 + the most points a voxel can hold), output_coords (rows,4) int64 (occ32 = 0) or int32 (occ32 = 1), both
 * b*n_per rows of which the ones behind the V live rows are zeroed; info_dev = {V, maxActive, error}, error = a point outside its crop's grid or a voxel with more than
 * pitch-1 points.  Ids in first-encounter order, rows ascending, zero padded -- bit for bit voxelize.cpp:58-152 on the live
 * part.  comm: 2*b ints that persist between calls (zero before the first); gen != 0 must differ from the previous call's. */
int dcl_voxelize_idx_crops(const int64_t *coords, int batch, int n_per, int S, int mode, int pitch, int32_t *comm, int gen,
                           int32_t *input_map, void *output_coords, int occ32, int32_t *output_map, int32_t *info_dev,
                           dclStream_t stream);

/* voxelize_fp: pointgroup_ops_api.cpp:8 -> src/voxelize/voxelize.cu:9-31.
 * feats (N,C), rules (V,1+maxActive) -> out (V,C); out need not be zeroed.     */
int dcl_voxelize_fp(const float *feats, const int32_t *rules, float *out, int n_rows, int max_active,
                    int n_planes, int average, dclStream_t stream);

/* --------------------------------------------------------------- spconv ----
 * Replaces torch.ops.spconv.get_indice_pairs_3d / indice_conv_fp32 /
 * indiceSummaryRF / indice_avgpool_fp32 (libs/spconv/src/spconv/all.cc:19-42;
 * include/spconv/spconv_ops.h:27-137,253-349; pool_ops.h:141-208).
 *
 * An active set on a batch x S^3 grid is described on the device by
 *   mask    u32[batch*S^3/32]   occupancy bits, linear index ((b*S+x)*S+y)*S+z
 *   wprefix i32[batch*S^3/32+1] exclusive popcount prefix (last = #active)
 *   perm    i32[V] or NULL      rank (ascending linear index) -> feature row;
 *                               NULL = rows already in ascending order
 * Output voxels of conv/pool are numbered in ascending linear index, the
 * order the reference's GPU path produces (torch::_unique, spconv_ops.h:126).
 * The rulebook is kept in gather form: nbr[k*cap + o] = input row feeding
 * output row o through kernel offset k (or -1); k = kz + 3*ky + 9*kx as in
 * geometry.h:61-70.  All counts stay on the device.                            */

/* scratch: i32[(nwords+1023)/1024 + 1].  Builds mask/wprefix/perm from an explicit voxel list
 * (rows in any order, e.g. voxelize_idx's first-encounter order).              */
int dcl_grid_from_indices(const int32_t *indices, int n_rows, int batch, int S, uint32_t *mask,
                          int32_t *wprefix, int32_t *perm, int32_t *scratch, dclStream_t stream);

/* Step 1 of a non-submanifold conv / pool rulebook: the OUTPUT active set only
 * (prepareIndicePairsKernel + torch::_unique + assignGridAndIndiceOutKernel, indice.cu.h:24-65,
 * 112-128): out mask/wprefix on the S_out grid, out_indices (cap_out,4) in ascending linear
 * index, n_out_dev[0].  n_in is *n_in_dev if non-NULL (n_in_host then only bounds the launch).
 * scratch as above, sized for the S_out grid.                                   */
int dcl_conv_out_grid(const int32_t *in_indices, const int32_t *n_in_dev, int n_in_host,
                      const uint32_t *in_mask /* optional: enables the bit-parallel path */, int batch,
                      int S_in, int ksize, int stride, int padding, uint32_t *out_mask,
                      int32_t *out_wprefix, int32_t *out_indices, int32_t *n_out_dev, int cap_out,
                      int32_t *scratch, dclStream_t stream);

/* Step 2: the gather-form rulebook nbr i32[kvol*cap] of output rows `out_indices` against the
 * input set (in_mask, in_wprefix, in_perm) on the S_in grid: the input feeding output o through
 * offset k sits at o*stride - padding + k.  Submanifold conv = out set == in set, stride 1,
 * padding ksize/2.                                                              */
int dcl_rulebook_gather(const int32_t *out_indices, const int32_t *n_out_dev, int n_out_host,
                        const uint32_t *in_mask, const int32_t *in_wprefix, const int32_t *in_perm,
                        int batch, int S_in, int ksize, int stride, int padding, int32_t *nbr, int cap,
                        dclStream_t stream);

/* Non-submanifold conv / pool rulebook (ksize^3 offsets, stride, padding, dilation 1):
 * in_indices (n_in rows; n_in read from n_in_dev if non-NULL else n_in_host) ->
 * out mask/wprefix on the S_out grid, out_indices (cap_out,4), n_out_dev[0],
 * nbr i32[27*cap_out].  Rows beyond n_out are untouched.                      */
int dcl_rulebook_conv(const int32_t *in_indices, const int32_t *n_in_dev, int n_in_host,
                      const uint32_t *in_mask, const int32_t *in_wprefix, const int32_t *in_perm,
                      int batch, int S_in, int ksize, int stride, int padding,
                      uint32_t *out_mask, int32_t *out_wprefix, int32_t *out_indices,
                      int32_t *n_out_dev, int32_t *nbr, int cap_out, int32_t *scratch,
                      dclStream_t stream);

/* Submanifold rulebook: out set = in set (same rows).  nbr i32[27*cap].        */
int dcl_rulebook_subm(const int32_t *indices, const int32_t *n_dev, int n_host,
                      const uint32_t *mask, const int32_t *wprefix, const int32_t *perm,
                      int batch, int S, int ksize, int32_t *nbr, int cap, dclStream_t stream);

/* Export a gather-form rulebook in the reference's format: indice_pairs
 * i32[27][2][n_in_cap] (-1 padded) + indice_num i32[27] (spconv_ops.h:55-60).
 * Pair order inside an offset is unspecified, as in the reference.             */
int dcl_rulebook_to_pairs(const int32_t *nbr, int cap, const int32_t *n_out_dev, int n_out_host,
                          int kvol, int32_t *indice_pairs, int n_in_cap, int32_t *indice_num,
                          dclStream_t stream);

/* Importer for callers that hold the REFERENCE's rulebook format (the arguments of torch.ops.spconv.indice_conv_fp32 /
 * indice_avgpool_fp32 / indiceSummaryRF, libs/spconv/src/spconv/all.cc:19-42, as spconv/conv.py:149-166 and
 * pool.py:237-242 pass them): indice_pairs i32 (kvol, 2, pair_stride) [k][0][j] = input row, [k][1][j] = output row, -1
 * padded; indice_num i32 (kvol) ON THE DEVICE (no host read-back -- the reference copies it to the CPU,
 * spconv_ops.h:264).  Fills the gather table nbr (kvol, cap) (cap >= n_out) that dcl_sparse_conv_fwd* /
 * dcl_sparse_avgpool_fwd* consume; pairs that point outside [0,n_in) x [0,n_out) are dropped and counted in
 * *bad_pairs_dev (may be NULL).                                                                                          */
int dcl_rulebook_from_pairs(const int32_t *indice_pairs, int pair_stride, const int32_t *indice_num_dev, int kvol,
                            int n_in, int n_out, int32_t *nbr, int cap, int32_t *bad_pairs_dev, dclStream_t stream);
/* torch.ops.spconv.indiceSummaryRF (all.cc:33; summaryRF.cu:26-68) on the pair format: rf[o] = number of pairs whose
 * output row is o, i32 (n_out).                                                                                          */
int dcl_indice_summary_rf(const int32_t *indice_pairs, int pair_stride, const int32_t *indice_num_dev, int kvol,
                          int n_out, int32_t *rf, dclStream_t stream);

/* indice_conv_fp32 (+ the BatchNorm1d(eval)+ReLU that SparseSequential applies next,
 * models/Modules.py:36-40): out[o] = act( (sum_k feat[nbr[k][o]] * W[k]) * scale + shift ).
 * W (27,Cin,Cout); scale/shift (Cout) or NULL; subm != 0 accumulates the centre offset
 * first (spconv_ops.h:289-299).                                                */
int dcl_sparse_conv_fwd(const float *feat, const int32_t *nbr, int cap, const int32_t *n_out_dev,
                        int n_out_host, const float *W, int cin, int cout, int kvol, int subm,
                        const float *scale, const float *shift, int relu, float *out,
                        dclStream_t stream);

/* Same, with caller scratch (partial-tile slots + tile tickets): the launch's chunk units -- tile-major, 27*Cin/32 chunks
 * per 128 x {32,64,128} output tile -- are dealt evenly to the 2 x 256 resident workgroup slots ("stream-K"), or the tiles
 * are split into aligned K segments, or kept whole, whichever a small cost model prefers; partial tiles are combined
 * INSIDE the launch by the workgroup that draws a tile's last ticket, in ascending chunk order (deterministic), then the
 * epilogue.  Launches of a few rows (cap <= 4096, or <= 65536 capacity rows with n_out_dev: one-image calls are
 * latency-bound on the contraction loop) take 4 chunks per workgroup and combine in a second small launch.
 * The first 8192 int32 of `scratch` are the tickets: the call zeroes them (they are left zero).
 * scratch_floats >= dcl_sparse_conv_scratch_floats(cap, cout) enables every decomposition; NULL = whole tiles only.   */
int dcl_sparse_conv_fwd_ws(const float *feat, const int32_t *nbr, int cap, const int32_t *n_out_dev,
                           int n_out_host, const float *W, int cin, int cout, int kvol, int subm,
                           const float *scale, const float *shift, int relu, float *out, float *scratch,
                           int64_t scratch_floats, dclStream_t stream);

/* Row ordering of a conv layer's output rows + the launch that uses it (csrc/row_order.hip; replaces nothing in the
 * reference -- it re-orders the work of indiceConv, spconv_ops.h:284-344, not its results).  dcl_order_rows: for the output
 * set `out_indices` (rows, 4) [b,x,y,z] of a k3 / s1 / p1 layer whose INPUT set has the occupancy bits `in_mask` on a
 * batch x S_in^3 grid (S_in in {8,16,32,64}), writes
 *   order[i]  = the output row tile slot i computes (rows sorted, stably, by a 9-bit key of their neighbourhood shape),
 *   bal[t]    = number of used kernel-offset steps of the 128-row tiles in front of tile t (bal[ntiles] = their total),
 *   smask[t]  = tile t's step mask (bit s = step s of the visiting order has a neighbour among the tile's rows).
 * order: cap ints; bal: cap/128 + 2 ints; smask: cap/128 + 1 words; ws: dcl_order_rows_ws_bytes(cap).  Live row count from
 * n_out_dev (device-visible) or n_out_host.  dcl_sparse_conv_fwd_ordered = dcl_sparse_conv_fwd_ws with that order: same
 * output rows, same values up to the fp32 summation split points of the decomposition (bal / smask may be NULL: the order
 * alone).                                                                                                             */
int dcl_order_rows_ws_bytes(int cap, int64_t *bytes_host);
int dcl_order_rows(const int32_t *out_indices, const int32_t *n_out_dev, int n_out_host, int cap, const uint32_t *in_mask,
                   int S_in, int subm, void *ws, int64_t ws_bytes, int32_t *order, int32_t *bal, uint32_t *smask,
                   dclStream_t stream);
int dcl_sparse_conv_fwd_ordered(const float *feat, const int32_t *nbr, int cap, const int32_t *n_out_dev, int n_out_host,
                                const float *W, int cin, int cout, int kvol, int subm, const float *scale,
                                const float *shift, int relu, float *out, float *scratch, int64_t scratch_floats,
                                const int32_t *order, const int32_t *bal, const uint32_t *smask, dclStream_t stream);
int dcl_sparse_conv_scratch_floats(int rows_cap, int cout, int64_t *floats_host);

/* Split-bf16 form of the LDS-DMA conv kernel (csrc/conv_body.h): the product of a 32-channel chunk as six exact bf16 piece
 * products on the bf16 matrix pipe (the scheme of dcl_linear_split_fwd), for kvol = 27, cin in {32, 64, 128}, cout % 64 == 0.
 * dcl_conv_split_weight writes W (27, cin, cout) as three bf16 planes h + m + l == W (exactly) in the kernel's chunk / tile
 * order -- [k][cin / 32][cout / 64][plane][k step][lane half][64 columns][8 channels] -- into `planes` (16-byte aligned,
 * dcl_conv_split_weight_bytes = 6 * 27 * cin * cout bytes; 0 for widths the kernel does not take): once per layer.
 * dcl_sparse_conv_fwd_sides: one layer of one or two problems (per-side HOST arrays) in ONE launch, from explicit gather
 * tables; pieces != NULL: every side's prepared planes, the launch takes the split form; NULL: the fp32 form of the same
 * launch.  order / bal / smask: NULL or per-side arrays as in dcl_sparse_conv_fwd_ordered.  Same rows, same epilogue; the
 * two forms differ by fp32-sized rounding only and agree bit for bit where all piece products and partial sums are exact. */
int64_t dcl_conv_split_weight_bytes(int kvol, int cin, int cout);
int dcl_conv_split_weight(const float *W, int kvol, int cin, int cout, void *planes, dclStream_t stream);
int dcl_sparse_conv_fwd_sides(int nsides, const float *const *feat, const int32_t *const *nbr, const int32_t *cap,
                              const int32_t *n_out_host, const float *const *W, const void *const *pieces, int cin, int cout,
                              int kvol, int subm, const float *const *scale, const float *const *shift, int relu,
                              float *const *out, float *scratch, int64_t scratch_floats, const int32_t *const *order,
                              const int32_t *const *bal, const uint32_t *const *smask, dclStream_t stream);

/* indiceSummaryRF + indice_avgpool_fp32 (use_gs=False): rf[o] = #valid offsets,
 * out[o] = sum_k asc feat[nbr[k][o]] / (float)rf[o].  rf may be NULL.          */
int dcl_sparse_avgpool_fwd(const float *feat, const int32_t *nbr, int cap, const int32_t *n_out_dev,
                           int n_out_host, int c, int kvol, float *out, int32_t *rf,
                           dclStream_t stream);

/* torch.ops.spconv.indice_avgpool_fp32 (all.cc:34; pool_ops.h:170-208) with the caller's `summaryrf` (i32 (n_out): the
 * receptive-field counts of indiceSummaryRF when use_gs=False, the kernel volume when use_gs=True, functional.py:146-155)
 * as the divisor: out[o] = sum_k asc feat[nbr[k][o]] / (float)summaryrf[o].                                              */
int dcl_sparse_avgpool_fwd_rf(const float *feat, const int32_t *nbr, int cap, const int32_t *n_out_dev,
                              int n_out_host, int c, int kvol, const int32_t *summaryrf, float *out,
                              dclStream_t stream);

/* Several zero-padded 2-D copies of 4-byte elements in ONE launch (input staging / result hand-over of the whole-forward
 * hipGraph): job: dst (rows_dst x cols_dst; dense, or a column block with row pitch dst_pitch elements) <- src (rows_src x
 * cols_src, row pitch src_pitch elements; int64 elements narrowed to int32 when src_is_i64), zero outside src;
 * src == NULL fills dst with fill_value.                                                                                */
#define DCL_PAD_COPY_MAX_JOBS 12
typedef struct {
  void *dst;
  const void *src;
  int32_t rows_dst, cols_dst, rows_src, cols_src, src_pitch, src_is_i64, fill_value, dst_pitch /* 0 = dense */;
} DclPadCopyJob;
int dcl_pad_copy_many(const DclPadCopyJob *jobs_host, int njobs, dclStream_t stream);

/* ---------------------------------------------------- native backbone runner ---
 * One sparse backbone of DCL-Net (Backbone_SPCONV.forward, models/Modules.py:153-159: 4 x [SparseConv3d k3 s1 p1
 * + BN + ReLU, SubMConv3d k3 + BN + ReLU, SparseAvgPool3d k3 s2 p1]) and its point read-out
 * (Ops_GetPointFeat_spconv.forward, :236-251) as three enqueue-only calls with ONE host read-back of the 8 level
 * sizes in between (the reference: ~2.5k launches, 32 blocking copies).  Workspaces are caller-allocated;
 * `channels_host` = the 9 backbone dims [7,16,32,32,64,64,128,128,256]; counts = [n_conv1, n_pool1, ..., n_pool4].
 * `counts_dev` of the geometry calls is written by kernels: device memory, or device-visible pinned host memory
 * (hipHostMalloc) -- the caller then only waits for the stream and reads the 8 sizes, no copy is enqueued.              */
int dcl_backbone_ws_bytes(int batch, int S, int V0, int64_t *bytes_host);
int dcl_backbone_geometry(const int32_t *occ, int V0, int batch, int S, void *ws, int64_t ws_bytes,
                          int32_t *counts_dev /* i32[8] */, dclStream_t stream);
/* Same over a batch window: only the voxels of crops batch_lo .. batch_lo+batch-1 of `occ` (all V0 rows are scanned)
 * enter the pass, re-based to crop 0.  Sub-batch passes can then share one occupied-voxel / voxel-feature array, which is
 * how Network.forward pipelines the sparse half of chunk c+1 under the dense half of chunk c.  ws sized for (batch, S, V0). */
int dcl_backbone_geometry_window(const int32_t *occ, int V0, int batch_lo, int batch, int S, void *ws, int64_t ws_bytes,
                                 int32_t *counts_dev, dclStream_t stream);
int dcl_backbone_ws2_bytes(const int32_t *counts_host, const int32_t *channels_host, int64_t *bytes_host);
/* weights_host[8]/scales_host[8]/shifts_host[8]: HOST arrays of device pointers ((27,Cin,Cout) / (Cout));
 * level_out_host[4]: HOST array of device pointers, level m = (counts[2m+1], channels[2m+2]) floats.            */
int dcl_backbone_features(const int32_t *occ, int V0, int batch, int S, void *ws, const int32_t *counts_host,
                          const int32_t *channels_host, const float *vox_feats,
                          const float *const *weights_host, const float *const *scales_host,
                          const float *const *shifts_host, void *ws2, int64_t ws2_bytes,
                          float *const *level_out_host, dclStream_t stream);
/* Capacity mode of the three calls (whole-forward hipGraph capture): nothing on the host depends on the data.
 * occ holds V0_cap rows, the first *V0_dev live; buffers (level_out, ws2) are sized by dcl_backbone_caps' row
 * capacities (pass them as counts to dcl_backbone_ws2_bytes); kernels read the live counts from counts_dev.        */
int dcl_backbone_caps(int batch, int S, int V0_cap, int32_t *caps_host /* i32[8] */);
int dcl_backbone_geometry_cap(const int32_t *occ, const int32_t *V0_dev, int V0_cap, int batch, int S, void *ws,
                              int64_t ws_bytes, int32_t *counts_dev, dclStream_t stream);
/* dcl_backbone_geometry_cap + dcl_voxelize_fp(feats, rules, vox_out, rows, max_active, planes, average) of the pass's points:
 * a pass of up to 16 crops carries the voxelisation in its one geometry launch (it depends on the input only). */
int dcl_backbone_geometry_cap_vox(const int32_t *occ, const int32_t *V0_dev, int V0_cap, int batch, int S, void *ws,
                                  int64_t ws_bytes, int32_t *counts_dev, const float *feats, const int32_t *rules,
                                  float *vox_out, int rows, int max_active, int planes, int average, dclStream_t stream);
int dcl_backbone_features_cap(const int32_t *occ, int V0_cap, int batch, int S, void *ws, const int32_t *counts_dev,
                              const int32_t *channels_host, const float *vox_feats, const float *const *weights_host,
                              const float *const *scales_host, const float *const *shifts_host, void *ws2,
                              int64_t ws2_bytes, float *const *level_out_host, dclStream_t stream);
/* BOTH backbones of a forward in one feature stage (DCL-Net runs two of the same shape: observed crops and template clouds,
 * models/DCL_Net.py:93-94,173-186): per-side arrays of 2.  Every layer becomes ONE launch over both sides' tiles -- 8 conv
 * + 4 pool launches per forward instead of 16 + 8 -- with results identical to two dcl_backbone_features calls up to the
 * fp32 summation split points of the stream-K decomposition.  counts_dev != NULL selects capacity mode for both sides
 * (V0 are then capacities and counts_host is ignored); otherwise counts_host[i] are the sides' 8 level sizes.  The sides
 * share batch, S and the channel list; each has its own geometry workspace, parameters, ws2 and level outputs.         */
int dcl_backbone_features_pair(int batch, int S, const int32_t *channels_host, const int32_t *V0, void *const *ws,
                               const int32_t *const *counts_host, const int32_t *const *counts_dev,
                               const float *const *vox_feats, const float *const *const *weights,
                               const float *const *const *scales, const float *const *const *shifts, void *const *ws2,
                               const int64_t *ws2_bytes, float *const *const *level_out, dclStream_t stream);
/* The three feature calls with prepared filter pieces (dcl_conv_split_weight): wpieces_host[8] per side, entry i = conv layer
 * i's planes -- that layer runs the split-bf16 conv form -- or NULL -- it keeps the fp32 kernel; wpieces == NULL: none.  The
 * caller chooses by shape (layer widths, number of crops), never by data.                                                  */
int dcl_backbone_features_split(const int32_t *occ, int V0, int batch, int S, void *ws, const int32_t *counts_host,
                                const int32_t *channels_host, const float *vox_feats, const float *const *weights_host,
                                const void *const *wpieces_host, const float *const *scales_host,
                                const float *const *shifts_host, void *ws2, int64_t ws2_bytes, float *const *level_out_host,
                                dclStream_t stream);
int dcl_backbone_features_cap_split(const int32_t *occ, int V0_cap, int batch, int S, void *ws, const int32_t *counts_dev,
                                    const int32_t *channels_host, const float *vox_feats, const float *const *weights_host,
                                    const void *const *wpieces_host, const float *const *scales_host,
                                    const float *const *shifts_host, void *ws2, int64_t ws2_bytes,
                                    float *const *level_out_host, dclStream_t stream);
int dcl_backbone_features_pair_split(int batch, int S, const int32_t *channels_host, const int32_t *V0, void *const *ws,
                                     const int32_t *const *counts_host, const int32_t *const *counts_dev,
                                     const float *const *vox_feats, const float *const *const *weights,
                                     const void *const *const *wpieces, const float *const *const *scales,
                                     const float *const *const *shifts, void *const *ws2, const int64_t *ws2_bytes,
                                     float *const *const *level_out, dclStream_t stream);
int dcl_point_features_cap(int n, const float *points_b4, int batch, int S, int V0_cap, void *ws,
                           const int32_t *counts_dev, const int32_t *channels_host,
                           const float *const *level_feats_host, const float *voxel_extent_host, float offset,
                           float *out, int ld, void *tmp, int64_t tmp_bytes, dclStream_t stream);

/* byte offsets (inside ws) of pooled level `level`'s (b,x,y,z) rows and mask-word prefix, and its grid size */
int dcl_backbone_level_info(int batch, int S, int V0, int level, int64_t *indices_off_host,
                            int64_t *wprefix_off_host, int32_t *S_level_host);
/* points_b4 (n,4) [b,x,y,z] -> out (n, ld): levels' channels side by side.  voxel_extent_host[4] = unit*scale per
 * level (fp32), offset = -0.5*unit*64.  tmp >= 2*align256(48n) bytes: then the read-out is two launches (all
 * searches, all interpolations); with only 2*align256(12n) it goes level by level.                                */
int dcl_point_features(int n, const float *points_b4, int batch, int S, int V0, void *ws,
                       const int32_t *counts_host, const int32_t *channels_host,
                       const float *const *level_feats_host, const float *voxel_extent_host, float offset,
                       float *out, int ld, void *tmp, int64_t tmp_bytes, dclStream_t stream);
/* dcl_point_features with its nfold (1 or 2) deepest levels left to the GEMM that consumes the read-out
 * (dcl_linear_split_gather_fwd): out (n, ld) gets the columns of the first 4 - nfold levels only -- bit for bit the first
 * columns of dcl_point_features -- and for folded level l = 0 .. nfold - 1 (level 4 - nfold + l) the call returns
 * fw[l][n][3], the normalised inverse-distance weights the interpolation would have used (the same expressions, the same
 * bits), and fi[l][n][3], the rows of that level's features they weigh.  Always two launches (all searches, then the
 * interpolation); tmp >= 2*align256(48n) bytes.                                                                      */
int dcl_point_features_fold(int n, const float *points_b4, int batch, int S, int V0, void *ws, const int32_t *counts_host,
                            const int32_t *channels_host, const float *const *level_feats_host,
                            const float *voxel_extent_host, float offset, int nfold, float *out, int ld, float *fw,
                            int32_t *fi, void *tmp, int64_t tmp_bytes, dclStream_t stream);
/* The same read-out in two halves, so that a caller can overlap the searches with the convolutions: the 3-NN searches
 * need the level geometry only (dcl_backbone_geometry), the interpolation needs the level features.
 * dist2 / idx: 4 level blocks of n*3 entries each (level-major).  Results are identical to dcl_point_features.
 * The _cap forms take dcl_backbone_caps' V0_cap (whole-forward hipGraph capture).                                   */
int dcl_point_neighbours(int n, const float *points_b4, int batch, int S, int V0, void *ws, const int32_t *counts_host,
                         const float *voxel_extent_host, float offset, float *dist2, int32_t *idx, dclStream_t stream);
int dcl_point_neighbours_cap(int n, const float *points_b4, int batch, int S, int V0_cap, void *ws,
                             const float *voxel_extent_host, float offset, float *dist2, int32_t *idx,
                             dclStream_t stream);
int dcl_point_interpolate(int n, const int32_t *counts_host, const int32_t *channels_host,
                          const float *const *level_feats_host, const float *dist2, const int32_t *idx, float *out,
                          int ld, dclStream_t stream);

/* ----------------------------------------------------------- pointnet_sp ---
 * three_nn_wrapper(n, m, unknown(N,4), known(M,4), dist2(N,3), idx(N,3)):
 * libs/pointnet_sp/src/pointnet2_api.cpp:7 -> interpolate_gpu.cu:9-77.
 * known_seg (i32[nbatch+1], optional): known rows of batch b are exactly
 * [known_seg[b], known_seg[b+1]) -- lets a query scan only its own crop; NULL
 * scans all m rows comparing the batch column like the reference.              */
int dcl_three_nn_sp(int n, int m, const float *unknown, const float *known, float *dist2,
                    int32_t *idx, const int32_t *known_seg, int nbatch, dclStream_t stream);

/* three_interpolate_wrapper(c, m, n, points(M,C), idx, weight, out(N,C)):
 * pointnet2_api.cpp:8 -> interpolate_gpu.cu:80-122.  out_stride (>= c, in floats) lets the
 * caller write straight into a column block of the 480-channel concat.         */
int dcl_three_interpolate_sp(int c, int m, int n, const float *points, const int32_t *idx,
                             const float *weight, float *out, int out_stride, dclStream_t stream);

/* three_interpolate with the weights of Ops_nearest_neighbor_interpolate computed in-kernel
 * (models/Modules.py:221-224: dist = sqrt(dist2); w = (1/(dist+1e-8)) / sum) -- takes the dist2
 * that dcl_three_nn_sp returns.                                                */
int dcl_three_interpolate_dist2_sp(int c, int m, int n, const float *points, const int32_t *idx,
                                   const float *dist2, float *out, int out_stride,
                                   dclStream_t stream);

/* Ops_tensor2points (models/Modules.py:204-211): voxel rows (V,4) i32 [b,x,y,z] -> centres (V,4)
 * f32 [b, x*ve+off+0.5*ve, ...] (fp32, left to right).  n from n_dev if non-NULL (n_host = bound). */
int dcl_voxel_centres(const int32_t *indices, const int32_t *n_dev, int n_host, float ve, float off,
                      float *centres, dclStream_t stream);

/* ---------------------------------------------------------- pointnet_lib ---
 * libs/pointnet_lib/src/pointnet2_api.cpp:10-25, all ten wrappers (the three
 * *_grad ones below the forward ops).  Same argument order.                    */
int dcl_ball_query(int b, int n, int m, float radius, int nsample, const float *new_xyz,
                   const float *xyz, int32_t *idx, dclStream_t stream);       /* idx fully written */
int dcl_group_points(int b, int c, int n, int npoints, int nsample, const float *points,
                     const int32_t *idx, float *out, dclStream_t stream);
/* Same, writing channel block [0,c) of an output whose batch entries hold out_batch_channels >= c channels (pass `out`
 * already offset to the first channel to fill): lets QueryAndGroup fill its (B, C+3, npoint, nsample) result in place. */
int dcl_group_points_into(int b, int c, int n, int npoints, int nsample, const float *points, const int32_t *idx,
                          float *out, int out_batch_channels, dclStream_t stream);
int dcl_gather_points(int b, int c, int n, int npoints, const float *points, const int32_t *idx,
                      float *out, dclStream_t stream);
/* temp (B,N) must be pre-filled with 1e10 (pointnet2_utils.py:27); updated in place. */
int dcl_furthest_point_sampling(int b, int n, int m, const float *dataset, float *temp,
                                int32_t *idxs, dclStream_t stream);
int dcl_knn(int b, int n, int m, int k, const float *unknown, const float *known, float *dist2,
            int32_t *idx, dclStream_t stream);                                 /* k <= 200 */
int dcl_three_nn(int b, int n, int m, const float *unknown, const float *known, float *dist2,
                 int32_t *idx, dclStream_t stream);
int dcl_three_interpolate(int b, int c, int m, int n, const float *points, const int32_t *idx,
                          const float *weight, float *out, dclStream_t stream);

/* The three gradient wrappers of the same file (pointnet2_api.cpp:14,17,24), the reference's arguments in its order, then
 * a workspace: ws (16-byte aligned) of at least the *_ws_bytes of the same sizes.  Like the reference they ADD INTO
 * grad_points, which the caller has zero-filled:
 *   group_points_grad   grad_out (B,C,npoints,nsample), idx (B,npoints,nsample) -> grad_points (B,C,n)
 *   gather_points_grad  grad_out (B,C,npoints),         idx (B,npoints)         -> grad_points (B,C,n)
 *   three_interpolate_grad  grad_out (B,C,n), idx / weight (B,n,3)              -> grad_points (B,C,m)
 * Deterministic (csrc/backward.hip: an inverse index of idx per call, then a gather): every element of grad_points gets
 * the contributions that name it added one at a time, in ascending flat position order (p*nsample + s, p, i*3 + k;
 * interpolation: the product grad_out*weight rounded to fp32 before the add) -- numpy.add.at on float32, bit for bit.
 * Indices outside [0, n) (resp. [0, m)) contribute nothing and are never used as addresses.  Bad sizes (negative, more
 * than 2^31 - 8192 positions per batch entry, b > 65535) and a short workspace return DCL_EINVAL before any GPU work;
 * the size queries need no GPU.                                                                                         */
int dcl_group_points_grad_ws_bytes(int b, int c, int n, int npoints, int nsample, int64_t *bytes_host);
int dcl_group_points_grad(int b, int c, int n, int npoints, int nsample, const float *grad_out, const int32_t *idx,
                          float *grad_points, void *ws, int64_t ws_bytes, dclStream_t stream);
int dcl_gather_points_grad_ws_bytes(int b, int c, int n, int npoints, int64_t *bytes_host);
int dcl_gather_points_grad(int b, int c, int n, int npoints, const float *grad_out, const int32_t *idx,
                           float *grad_points, void *ws, int64_t ws_bytes, dclStream_t stream);
int dcl_three_interpolate_grad_ws_bytes(int b, int c, int n, int m, int64_t *bytes_host);
int dcl_three_interpolate_grad(int b, int c, int n, int m, const float *grad_out, const int32_t *idx,
                               const float *weight, float *grad_points, void *ws, int64_t ws_bytes,
                               dclStream_t stream);

/* ------------------------------------------------------------ dense path ---
 * All dense operands are POINT-major: X[(b*n + p)*ld + c] (row = point, ld = row stride in
 * floats).  That is the layout the 3-NN interpolation emits and 2-D GEMMs consume; the
 * reference's (b,C,n) tensors are transposed views of it.
 *
 * Cross-attention of Aligner.forward + the extra bmm (models/Modules.py:162-169;
 * models/DCL_Net.py:206-215), one direction per call, without materialising A:
 *   S[j,i] = <K[j,:], Q[i,:]> over 64 channels, A = softmax over the KEY axis j,
 *   O1[i,:] = sum_j A[j,i] V1[j,:]  (dv1 ch),  O2 likewise from V2 (dv2 ch; may be NULL/0)
 * Q (b*nq rows), K, V1, V2 (b*nk rows), O1, O2 (b*nq rows).  fp32 MFMA, online softmax.
 * The product library is built for DCL-Net's own channel split, dv1 = 256 and dv2 = 64 (DCL_EINVAL otherwise); the
 * diagnostic library (-DDCL_DIAG) also carries the general-shape predecessors: dv1, dv2 multiples of 32 with
 * (dv1+dv2)/32 in {1,2,4,8,10}.  All ld % 4 == 0, 16-B aligned.   */
int dcl_cross_attention(int b, int nq, int nk, const float *Q, int ldq, const float *K, int ldk,
                        const float *V1, int dv1, int ldv1, float *O1, int ldo1, const float *V2,
                        int dv2, int ldv2, float *O2, int ldo2, dclStream_t stream);
/* Same with caller scratch: launches with few workgroups (small batches) split the keys over up to 8 workgroups per query
 * block; the partial (unnormalised sums, running max, weight sum) records in `scratch` are merged by a second kernel.
 * scratch_floats >= dcl_cross_attention_scratch_floats(b, nq) enables every split; NULL = dcl_cross_attention.         */
int dcl_cross_attention_ws(int b, int nq, int nk, const float *Q, int ldq, const float *K, int ldk,
                           const float *V1, int dv1, int ldv1, float *O1, int ldo1,
                           const float *V2, int dv2, int ldv2, float *O2, int ldo2,
                           float *scratch, int64_t scratch_floats, dclStream_t stream);
/* Same; concurrent_launches = 2 tells the launcher that ANOTHER attention launch of the same size runs side by side on a second
 * stream / graph branch (the two directions of a forward): the workgroup shape is then chosen for the pair (1 = a lone launch =
 * dcl_cross_attention_ws).  A hint for speed only: results do not depend on it beyond the summation order of a key split. */
int dcl_cross_attention_ws2(int b, int nq, int nk, const float *Q, int ldq, const float *K, int ldk,
                            const float *V1, int dv1, int ldv1, float *O1, int ldo1,
                            const float *V2, int dv2, int ldv2, float *O2, int ldo2,
                            float *scratch, int64_t scratch_floats, int concurrent_launches, dclStream_t stream);
/* dcl_cross_attention_ws2 with both products of large calls (S = K Q^T and P.V) on the bf16 matrix pipe at fp32-sized errors
 * (csrc/dense.hip: k_cross_attn_split; the scheme of dcl_linear_split_fwd): `planes` is scratch for the three bf16 pieces of K and
 * V in tile order, dcl_cross_attention_planes_bytes(b, nq, nk, concurrent_launches) bytes (0 = a call of this size keeps the
 * fp32-MFMA kernel; planes = NULL or fewer bytes: likewise), 16-byte aligned.  V must be [256 | 64] channels. */
int64_t dcl_cross_attention_planes_bytes(int b, int nq, int nk, int concurrent_launches);
/* How many of the b crops of such a call take the split kernel: 0, b, or the whole rounds of a pair call.  When it is b, V1 may be
 * NULL in dcl_cross_attention_ws3: its pieces are then expected in `planes` already, written by the GEMM that computes V1
 * (dcl_linear_split_vpieces_fwd) -- the fp32 V1 is never stored and the piece pass skips its 256 channels. */
int dcl_cross_attention_split_crops(int b, int nq, int nk, int concurrent_launches);
int dcl_cross_attention_ws3(int b, int nq, int nk, const float *Q, int ldq, const float *K, int ldk,
                            const float *V1, int dv1, int ldv1, float *O1, int ldo1, const float *V2, int dv2,
                            int ldv2, float *O2, int ldo2, float *scratch, int64_t scratch_floats,
                            int concurrent_launches, void *planes, int64_t planes_bytes, dclStream_t stream);
int dcl_cross_attention_scratch_floats(int b, int nq, int64_t *floats_host);
/* Gradients of that contraction without the attention map (csrc/attention_bwd.hip), one direction per call.  With
 * V = [V1|V2], O = [O1|O2], dO = [dO1|dO2] (320 ch) and, per query row i, delta_i = <dO[i,:], O[i,:]>:
 *   dP[j,i] = <dO[i,:], V[j,:]>,  dS[j,i] = A[j,i] (dP[j,i] - delta_i),
 *   dV[j,:] = sum_i A[j,i] dO[i,:],  dK[j,:] = sum_i dS[j,i] Q[i,:],  dQ[i,:] = sum_j dS[j,i] K[j,:].
 * Q, K, V1, V2 as dcl_cross_attention took them, O1, O2 as it returned them; dO2 = NULL is a zero gradient for O2.  A is
 * recomputed tile by tile from the per-query log-sum-exp of the scores (exact-fp32 MFMA products, like the fp32 forward):
 * nothing of size nq*nk is stored.  ws: dcl_cross_attention_bwd_ws_bytes(b, nq, nk) bytes (two floats per query, so it does not
 * depend on nk), 16-byte aligned.  dQ (b*nq rows, 64 ch), dK (b*nk, 64), dV1 (b*nk, 256), dV2 (b*nk, 64) are OVERWRITTEN;
 * dK and dV2 are separate outputs even where the caller passed one tensor as K and V2 (it adds them).  Three launches, each
 * owning the rows it writes: no float atomics, no workgroup waits on another, bit-identical results call after call.
 * b, nq, nk >= 1 (any counts: ragged last tiles are masked); dv1 = 256 and dv2 = 64 only; all ld % 4 == 0, 16-B aligned.  Bad
 * sizes, unsupported dv1 / dv2 and a NULL, misaligned or short workspace return DCL_EINVAL before any GPU work; the size
 * query needs no GPU.                                                                                                    */
int dcl_cross_attention_bwd_ws_bytes(int b, int nq, int nk, int64_t *bytes_host);
int dcl_cross_attention_bwd(int b, int nq, int nk,
        const float *Q, int ldq, const float *K, int ldk,
        const float *V1, int dv1, int ldv1, const float *V2, int dv2, int ldv2,
        const float *O1, int ldo1, const float *O2, int ldo2,
        const float *dO1, int lddo1, const float *dO2, int lddo2,
        float *dQ, int lddq, float *dK, int lddk, float *dV1, int lddv1, float *dV2, int lddv2,
        void *ws, int64_t ws_bytes, dclStream_t stream);

/* Confidence pooling (models/DCL_Net.py:217-228): conf = sigmoid(cat[logit1 (b,n1), logit2
 * (b,n2)]) -> conf (b,n1+n2); w = softmax(conf) -> w_scratch (b,n1+n2);
 * part1 (b,nslices,C): slice partials of sum_{j<n1} w[j] F1[b,j,:]; part2 likewise over F2 with
 * w[n1+j]; wsum (b,2) = the two partial sums of w.  The caller adds the slices in index order
 * (deterministic).  pooled of the reference = sum(part1)+sum(part2) when F1/F2 already carry their
 * trailing BatchNorm, else s1*P1 + t1*wsum1 + s2*P2 + t2*wsum2.  C % 4 == 0.                    */
int dcl_conf_pool(int b, int c, int n1, int n2, const float *logit1, const float *logit2,
                  const float *F1, int ld1, const float *F2, int ld2, float *conf, float *w_scratch,
                  int nslices, float *part1, float *part2, float *wsum, dclStream_t stream);
/* The second form of that sum in one launch: out (b,C) = ((s1*P1 + t1*wsum1) + s2*P2) + t2*wsum2 with
 * P = the slice partials of dcl_conf_pool added in a fixed order (s, t: the fusers' trailing BatchNorm1d in eval form). */
int dcl_pool_finish(int b, int c, int nslices, const float *part1, const float *part2, const float *wsum,
                    const float *scale1, const float *shift1, const float *scale2, const float *shift2, float *out,
                    dclStream_t stream);

/* out (rows, c) = relu(term + xyz (rows,3) @ W3 (3,c)): the xyz part of the first MLP_share layer of the stage-2 refiner
 * (models/refiner.py:78-80: Conv1d(259 -> 512) over cat[xyz, F_Xo_p]; `term` = F_Xo_p's part + bias, constant over the
 * refine iterations) in ONE pass over the tensor.  c % 4 == 0, 16-B aligned rows.                                       */
int dcl_affine3_relu(int64_t rows, int c, const float *xyz, const float *W3, const float *term, float *out,
                     dclStream_t stream);
/* regressor_rot + regressor_trans (models/DCL_Net.py:139-151,231-235; Head_MultiLayerPerceptron 1024 -> 512 -> 128 -> 9 | 3,
 * ReLU after the first two layers) on the pooled feature (b,1024), both heads in two launches -- meant for a handful of
 * crops (one-image calls); large batches use library GEMMs.  rot_layers / trans_layers: {W1t (1024,512), b1, W2t (512,128),
 * b2, W3t (128,9|3), b3}, matrices stored (in, out) row-major.  h1_scratch: 2*b*512 floats.  R (b,3,3), may be NULL: the
 * rotation matrices ortho9d2matrix (dcl_ortho9d_to_matrix) makes of o9, formed by the second launch itself.              */
/* The confidence regressor (models/DCL_Net.py:115-126, 217-218: Head_MultiLayerPerceptron [128, 128, 128, 1], ReLU, ReLU, none)
 * on point rows, one launch: out[m] = w3 . relu(W2t^T relu(W1t^T x[m] + b1) + b2) + b3.  x (M rows, pitch ldx >= 128, 16-B
 * aligned), W1t / W2t (128 x 128, row = input channel, dense), w3 element k at w3[k * ldw3], b3 one float, out (M).  fp32 MFMA. */
int dcl_mlp128_to1(const float *x, int64_t ldx, int M, const float *W1t, const float *b1, const float *W2t,
                   const float *b2, const float *w3, int64_t ldw3, const float *b3, float *out, dclStream_t stream);
int dcl_pose_heads(int b, const float *pooled, const float *const *rot_layers, const float *const *trans_layers,
                   float *h1_scratch, float *o9, float *trans, float *R, dclStream_t stream);
/* The same heads fed with the confidence pooling's slice partials instead of the finished pooled feature (dcl_conf_pool's part1 /
 * part2 / wsum + the fusers' trailing BatchNorm affines, as dcl_pool_finish takes them): the finish is folded into the first
 * launch -- every workgroup of a crop forms the 1024 inputs itself, same operations, same bits.  For a handful of crops. */
int dcl_pose_heads_parts(int b, int nslices, const float *part1, const float *part2, const float *wsum,
                         const float *scale1, const float *shift1, const float *scale2, const float *shift2,
                         const float *const *rot_layers, const float *const *trans_layers, float *h1_scratch, float *o9,
                         float *trans, float *R, dclStream_t stream);

/* ---- the eval refine loop with the pose on the device (models/refiner.py: refine_loop(compose="device"); the loop of
 * tools/test_YCBV_stage2.py:204-225).  One pass of the loop is dcl_refine_first, two GEMMs of the own core (the second with the
 * pooling epilogue, dcl_linear_pool_fwd) and dcl_refine_heads: five launches, the pose read from and written to device arrays.
 * These entries join the ABI; the version stays.  Every order below is part of the contract (csrc/refine_pose.h holds the
 * routines, host + device, built with -ffp-contract=off).
 *
 * dcl_refine_first: out (b*n, c) = relu(term (b*n, c) + cur @ W3 (3, c)), cur = R^T (p - t) of the row's crop (crop = row / n),
 * never stored.  pts (b,n,3), R (b,3,3) row-major, t (b,3).  PINNED: q = p - t (three subtractions);
 * cur_j = fmaf(R_2j, q_2, fmaf(R_1j, q_1, R_0j * q_0)) (dcl_rigid_points with inverse = 1);
 * out = fmaxf(fmaf(cur_2, W_2k, fmaf(cur_1, W_1k, cur_0 * W_0k)) + term, 0) (dcl_affine3_relu).  One launch, one streaming pass.
 * c % 4 == 0, any b, n >= 1 with b * n * 3 <= INT32_MAX, term / out / W3 16-B aligned.  dcl_refine_first_host: the same routine on
 * HOST pointers (no GPU call).
 *
 * dcl_pose_compose_host (HOST pointers; the epilogue of dcl_refine_heads on its own), per crop, row-major:
 *   R_out[i][j] = fmaf(R_in[i][2], dR[2][j], fmaf(R_in[i][1], dR[1][j], R_in[i][0] * dR[0][j]))
 *   t_out[i]    = fmaf(R_in[i][2], dt[2],    fmaf(R_in[i][1], dt[1],    R_in[i][0] * dt[0])) + t_in[i]
 *
 * dcl_refine_heads: dcl_pose_heads (same weights, same h1_scratch of 2*b*512 floats, same bits of o9 / dt / dR) fed with the
 * pooled feature still as dcl_linear_pool_fwd's tile partials part (b*T, 1024), and with the pose composition as its epilogue;
 * two launches.  PINNED: x[crop][ch] = ((part[crop*T+0][ch] + part[crop*T+1][ch]) + ...) + part[crop*T+T-1][ch], one ascending
 * fp32 chain from tile 0, formed by every workgroup of the crop's first launch.  The second launch's rotation workgroup writes
 * R_out (b,3,3), its translation workgroup t_out (b,3), by the formulas above from R_in, t_in and the dR / dt just formed; o9
 * (b,9), dt (b,3), dR (b,3,3) are written as dcl_pose_heads writes them.  R_out / t_out must not overlap R_in / t_in (a crop's
 * two workgroups both read the inputs).  T >= 1, b <= 65535.                                                              */
int dcl_refine_first(int b, int n, int c, const float *pts, const float *R, const float *t, const float *W3,
                     const float *term, float *out, dclStream_t stream);
int dcl_refine_first_host(int b, int n, int c, const float *pts, const float *R, const float *t, const float *W3,
                          const float *term, float *out);
int dcl_pose_compose_host(int b, const float *R_in, const float *t_in, const float *dR, const float *dt, float *R_out,
                          float *t_out);
int dcl_refine_heads(int b, int T, const float *part, const float *const *rot_layers, const float *const *trans_layers,
                     float *h1_scratch, const float *R_in, const float *t_in, float *R_out, float *t_out, float *o9, float *dt,
                     float *dR, dclStream_t stream);

/* One per-point linear layer -- Conv1d(k=1) / 1x1x1 Conv3d with its BatchNorm folded in (models/Modules.py:58-97, 173-201;
 * the reference runs them as cuDNN pointwise convolutions): y[M x N] = act(x[M x K] Wt[K x N] + bias[N]), row-major, every
 * matrix with its own row pitch (ldx >= K, ldw >= N, ldy >= N floats) so that x, Wt and y can be column blocks of wider
 * buffers.  A library GEMM (hipBLASLt, fp32, bias / ReLU epilogue); bias may be NULL, relu 0/1.  workspace: device scratch
 * the caller may pass (kept for ABI stability) -- NEVER used: only algorithms that ask for no workspace are taken, and the call
 * fails with DCL_EINVAL when the library has none for the shape (two workspace-exchanging stream-K kernels side by side on
 * two streams hang the GPU; csrc/linear.cpp).                                                                            */
int dcl_linear_fwd(const float *x, int64_t ldx, const float *Wt, int64_t ldw, const float *bias, float *y, int64_t ldy,
                   int M, int N, int K, int relu, void *workspace, int64_t workspace_bytes, dclStream_t stream);

/* The same layer on the library's OWN fp32 MFMA GEMM core (csrc/linear_dma.hip: 128 x 128 / 128 x 64 / 64 x 64 tiles, LDS-DMA
 * operand rings, v_mfma_f32_32x32x2_f32; no vendor library, no workspace).  Same argument meaning as dcl_linear_fwd; needs
 * K % 32 == 0, 16-byte aligned x / Wt and ldx % 4 == ldw % 4 == 0, a row of Wt holding N rounded up to 4 floats (DCL_EINVAL
 * otherwise: such layers stay on dcl_linear_fwd).  Per output element the sum is ONE fmaf chain over k.                  */
int dcl_linear_dma_fwd(const float *x, int64_t ldx, const float *Wt, int64_t ldw, const float *bias, float *y, int64_t ldy,
                       int M, int N, int K, int relu, dclStream_t stream);
/* The last fuser layer WITH the confidence-weighted pooling of models/DCL_Net.py:223-228 as its epilogue: instead of storing
 * F = act(x Wt + bias) (M x N) it leaves  part[t][c] = sum over the rows j of row tile t (128 rows) of w_j * F[j][c]  for
 * t = 0 .. ceil(M / 128) - 1 (row pitch ldp >= N), with w_j = roww[(j / rows_per_crop) * w_stride + j % rows_per_crop] (the
 * softmax weights as dcl_conf_softmax leaves them: one row of n1 + n2 weights per crop, a direction's block addressed through
 * the base pointer).  With every crop a whole number of tiles, dcl_pool_finish2 adds a crop's partials in tile order.
 * Same shape constraints as dcl_linear_dma_fwd. */
int dcl_linear_pool_fwd(const float *x, int64_t ldx, const float *Wt, int64_t ldw, const float *bias, const float *roww,
                        int rows_per_crop, int64_t w_stride, float *part, int64_t ldp, int M, int N, int K, int relu,
                        dclStream_t stream);
/* The last TWO layers of a head whose last layer has one output (the confidence regressor, models/DCL_Net.py:115-126: 128 ->
 * 128 -> 1) on the own GEMM core: out[m] = w3 . relu(x[m] Wt + bias) + b3 with the N <= 128 hidden columns never stored (the
 * row dot is the GEMM's epilogue).  w3: N floats with stride ldw3 (a (N, 1) weight with padded rows); b3: one float. */
int dcl_linear_rowdot_fwd(const float *x, int64_t ldx, const float *Wt, int64_t ldw, const float *bias, const float *w3,
                          int64_t ldw3, const float *b3, float *out, int M, int N, int K, dclStream_t stream);
/* The same layers on the bf16 matrix pipe with fp32 results (csrc/linear_split.hip): every fp32 operand is the exact sum of
 * three bf16 pieces and a product is accumulated as its six piece products of weight >= 2^-16, in fp32 accumulators (what is dropped
 * is below the rounding of an fp32 FMA chain).  A layer's weight is prepared ONCE: dcl_linear_split_weight writes its pieces, in the
 * kernel's tile order, into `planes` (dcl_linear_split_weight_bytes(K, N) bytes, 16-byte aligned; 0 = K is no multiple of 16).
 * dcl_linear_split_fwd / _pool_fwd / _rowdot_fwd then mirror dcl_linear_dma_fwd / dcl_linear_pool_fwd / dcl_linear_rowdot_fwd with
 * `planes` in the place of (Wt, ldw); x 16-byte aligned, ldx % 4 == 0, K % 16 == 0; workgroup tiles of 256 rows x 128 columns: for
 * launches of at least a few hundred tiles (the fp32-MFMA core keeps the rest).
 * Error: against exact arithmetic an output is off by at most 1.5 x what a k-ordered fp32 FMA chain is off by on the same
 * operands, both in units of 2^-24 (sum_k |x_k| |w_k| + |bias|) (a row with s non-zeros: at most 6 s + 2 units); the pooling and
 * row-dot epilogues add 66 and 10 units of their own sums' magnitudes (tests/test_gpu_split_arithmetic.py).
 * Range: operands of magnitude < 2^-110 lose up to 2^-126 |w| (|x|) per product (third pieces below the bf16 range).  NOT
 * supported: |v| >= 3.3962e38 (bits 0x7F7F8000: finite in fp32, inf as a bf16 first piece), +-inf and NaN -- every output of such a
 * row of x (column of Wt) is NaN, also where the fp32 core gives +-inf, and 0 behind a ReLU epilogue; every other row and column
 * of the launch has exactly the bits it has without that value. */
int64_t dcl_linear_split_weight_bytes(int K, int N);
int dcl_linear_split_weight(const float *Wt, int64_t ldw, int K, int N, void *planes, dclStream_t stream);
int dcl_linear_split_fwd(const float *x, int64_t ldx, const void *planes, const float *bias, float *y, int64_t ldy, int M, int N,
                         int K, int relu, dclStream_t stream);
int dcl_linear_split_pool_fwd(const float *x, int64_t ldx, const void *planes, const float *bias, const float *roww,
                              int rows_per_crop, int64_t w_stride, float *part, int64_t ldp, int M, int N, int K, int relu,
                              dclStream_t stream);
/* dcl_linear_split_fwd with gathered rows added in its epilogue (a read-out whose deepest levels are folded through the layer:
 * dcl_point_features_fold):
 *     y[m][c] = act(fma(fw[l][m][2], G_l[fi[l][m][2]][c], fma(fw[l][m][1], G_l[fi[l][m][1]][c], fma(fw[l][m][0], G_l[fi[l][m][0]][c], ...
 *               (x Wt)[m][c] + bias[c]))))            levels l = 0 .. nfold - 1 in ascending order, nfold = 1 or 2
 * -- one fused-multiply-add chain per output in that fixed order, no atomics: the same bits on every run.  fw / fi: level l's
 * three weights / rows of row m at element l * level_stride + 3 m (level_stride >= 3 M); G_host[l]: (R_l, N) fp32 with row pitch
 * ldg_host[l] >= N (both arrays are host memory).  THE CALLER'S CONTRACT: every fi[l][m][i], m < M, is a row of G_l, 0 <= fi < R_l
 * -- the kernel cannot check it and reads wherever it points.  Error: dcl_linear_split_fwd's for the product, one rounding per
 * added term.  A non-finite value in a row of G_l reaches exactly the outputs of the rows m that name it (0 behind a ReLU for NaN). */
int dcl_linear_split_gather_fwd(const float *x, int64_t ldx, const void *planes, const float *bias, int nfold, const float *fw,
                                const int32_t *fi, int64_t level_stride, const float *const *G_host, const int64_t *ldg_host,
                                float *y, int64_t ldy, int M, int N, int K, int relu, dclStream_t stream);
/* y = act(x Wt + bias) written AS the attention's V pieces (N <= 320 channels from channel 0, rows = keys of crop row /
 * rows_per_crop, rows_per_crop % 256 == 0 = M / crops): `vplanes` = the `planes` scratch of the dcl_cross_attention_ws3 call that
 * consumes it with V1 = NULL. */
int dcl_linear_split_vpieces_fwd(const float *x, int64_t ldx, const void *planes, const float *bias, void *vplanes,
                                 int rows_per_crop, int M, int N, int K, int relu, dclStream_t stream);
int dcl_linear_split_rowdot_fwd(const float *x, int64_t ldx, const void *planes, const float *bias, const float *w3, int64_t ldw3,
                                const float *b3, float *out, int M, int N, int K, dclStream_t stream);
/* The softmax half of dcl_conf_pool alone: conf (b, n1 + n2) = sigmoid(cat[logit1, logit2]), w (b, n1 + n2) = softmax(conf) per
 * crop, wsum (b, 2) = the weight sums of the two directions (models/DCL_Net.py:217-222). */
int dcl_conf_softmax(int b, int n1, int n2, const float *logit1, const float *logit2, float *conf, float *w, float *wsum,
                     dclStream_t stream);
/* dcl_pool_finish with a slice count per direction: part1 (b, nslices1, c), part2 (b, nslices2, c). */
int dcl_pool_finish2(int b, int c, int nslices1, int nslices2, const float *part1, const float *part2, const float *wsum,
                     const float *scale1, const float *shift1, const float *scale2, const float *shift2, float *out,
                     dclStream_t stream);

/* Several INDEPENDENT per-point linear layers in one launch (csrc/linear_group.hip), for calls of a handful of crops: the
 * reference issues every Conv1d(k=1) / 1x1x1 Conv3d of its MLP stacks as its own launch (models/Modules.py:58-97,173-201; the
 * four disengage second layers of a side, models/DCL_Net.py:188-200, and a regressor_conf layer beside the neck_fuser layer
 * of the same depth, :207-216, do not depend on each other).  Each job is dcl_linear_fwd's problem: y[M x N] = act(x[M x K]
 * Wt[K x N] + bias[N]), row-major with free row pitches; K % 32 == 0, ldx % 4 == 0, ldw % 4 == 0 and ldw >= N rounded up to 4
 * (a layer with N % 4 != 0 passes a zero-padded Wt), x and Wt 16-byte aligned.  Own fp32 MFMA kernel (64 x 64 tiles), the sum
 * of an element runs over k ascending.  jobs: HOST array of njobs <= DCL_LINEAR_MAX_JOBS descriptors holding DEVICE pointers. */
#define DCL_LINEAR_MAX_JOBS 8
typedef struct DclLinearJob {
  const float *x; int64_t ldx;
  const float *Wt; int64_t ldw;
  const float *bias;          /* may be NULL */
  float *y; int64_t ldy;
  int M, N, K, relu;
} DclLinearJob;
int dcl_linear_group_fwd(const DclLinearJob *jobs, int njobs, dclStream_t stream);

/* ortho9d2matrix (models/DCL_Net.py:15-36): o9 (b,9) -> R (b,3,3).             */
int dcl_ortho9d_to_matrix(int b, const float *o9, float *R, dclStream_t stream);

/* Its gradient (csrc/rotation_grad.hip): grad_R (b,3,3) = dL/dR -> grad_o9 (b,9) = dL/do9, one launch, nothing saved by
 * the forward but o9, no workspace and no atomics: two calls give the same bits.  With M = the normalised axes as columns
 * and the projection's own factors U' = [u1, u2, u1 x u2], V' = [v1, v2, det(V) v3], M = U' diag(s') V'^T (s'_3 signed),
 *     B = U'^T grad_R V',   Y_ij = (B_ij - B_ji) / (s'_i + s'_j)  (i != j, Y_ii = 0),   dL/dM = U' Y V'^T,
 * evaluated in fp64, then through the normalisation of every raw axis r (mag = |r| + 1e-8, g = its column of dL/dM):
 *     dL/dr = g / mag - r (r . g) / (|r| mag^2),   the second term 0 where |r| = 0.
 * Guards: a term of Y whose denominator has |s'_i + s'_j| <= 1e-12 s'_1 contributes 0 (left-handed axes whose second and
 * third singular values agree, rank <= 1: the projection is not differentiable there); at most 30 Jacobi sweeps; finite
 * inputs give finite outputs (unless a value itself exceeds fp32), parallel axes, zero axes and all zeros included; a crop
 * with a non-finite value in its o9 or grad_R gets NaN in its own nine outputs and no other crop is touched.
 * b == 0 is not an error.  dcl_ortho9d_bwd_host runs the same routine on HOST pointers and makes no GPU call.          */
int dcl_ortho9d_bwd(int b, const float *o9, const float *grad_R, float *grad_o9, dclStream_t stream);
int dcl_ortho9d_bwd_host(int b, const float *o9, const float *grad_R, float *grad_o9);

/* ------------------------------------------------------------ training-side kernels (csrc/backward.hip) ---
 * Transposed rulebook: inv[k][i] = o for every nbr[k][o] = i >= 0, -1 elsewhere (inv: i32[kvol][cap_in]).  With it the
 * input gradient of indice_conv (spconv_ops.h:351-438) is either dcl_sparse_conv_fwd(dOut, inv, W^T per offset), the default
 * route, or dcl_sparse_conv_dgrad(dOut, inv, W) below, which reads W as registered.                                   */
int dcl_rulebook_transpose(const int32_t *nbr, int cap_out, const int32_t *n_out_dev, int n_out_host, int kvol,
                           int32_t *inv, int cap_in, dclStream_t stream);
/* Filter gradient of indice_conv: dW[k] = sum_o feat[nbr[k][o]]^T dout[o] (spconv_ops.h:413-417).  partial: scratch of
 * splits*kvol*cin*cout floats with splits = dcl_sparse_conv_wgrad_splits(n_out); partial sums are added in split order. */
int dcl_sparse_conv_wgrad_splits(int n_out, int32_t *splits_host);
int dcl_sparse_conv_wgrad(const float *feat, const int32_t *nbr, int cap, int n_out, const float *dout, int cin, int cout,
                          int kvol, float *partial, float *dW, dclStream_t stream);
/* ---- the same filter gradient over the rulebook's PAIRS, in a pinned order (csrc/conv_wgrad_pairs.hip).
 *
 * Ordered pair list of a gather table nbr (kvol x cap, i32): (k, o) is a pair iff o < n_out and 0 <= nbr[k][o] < n_in.  Any
 * other entry takes no part and is never an address; rows o >= n_out are never read.  head (DCL_CONV_PAIRS_HEAD i32):
 *   head[k]                        count[k], the pairs of offset k                                   (k < kvol)
 *   head[32 + k]                   start[k], the exclusive prefix of count                           (k <= kvol)
 *   head[60]                       nsplit, the rows of the split table in use
 *   head[61]                       overflow = max(0, start[kvol] - max_pairs), the pairs that were not stored
 *   head[64 + k]                   the first split of offset k (head[64 + kvol] = nsplit)            (k <= kvol)
 * pair_in / pair_out [start[k] + p] (max_pairs i32 each) = the p-th pair of offset k in ASCENDING o: its input row nbr[k][o]
 * and its output row o -- a stable compaction from prefix sums; no atomic takes part and no workgroup waits on another.  A
 * pair whose position is max_pairs or more is not stored; count and start stay the true figures and overflow says how many
 * pairs are missing (a caller that sized max_pairs as kvol * min(n_in, n_out) sees 0 whenever an input row meets an offset at
 * most once -- the precondition of dcl_rulebook_transpose).  split_tab (dcl_conv_pairs_max_splits(max_pairs, kvol) rows of 4
 * i32: offset, first pair, length, 0): the STORED pairs of offset k cut into splits of DCL_CONV_PAIRS_SPLIT consecutive pairs
 * (the last one shorter), offsets ascending; nsplit <= max_pairs / DCL_CONV_PAIRS_SPLIT + kvol.  ws: scratch of at least
 * dcl_conv_pairs_ws_bytes bytes.  Three launches, no read-back: capturable.  The two queries and dcl_conv_pairs_host (the same
 * contract in plain C++ on host pointers) make no GPU call.  DCL_EINVAL before any GPU work for kvol outside 1..27, a
 * negative size, cap < n_out, max_pairs >= 2^30, a NULL buffer or a short workspace. */
#define DCL_CONV_PAIRS_SPLIT 512
#define DCL_CONV_PAIRS_HEAD 96
int dcl_conv_pairs_ws_bytes(int kvol, int n_out, int64_t *bytes_host);
int dcl_conv_pairs_max_splits(int max_pairs, int kvol, int32_t *splits_host);
int dcl_conv_pairs(const int32_t *nbr, int cap, int kvol, int n_out, int n_in, int max_pairs, int32_t *head,
                   int32_t *pair_in, int32_t *pair_out, int32_t *split_tab, void *ws, int64_t ws_bytes, dclStream_t stream);
int dcl_conv_pairs_host(const int32_t *nbr, int cap, int kvol, int n_out, int n_in, int max_pairs, int32_t *head,
                        int32_t *pair_in, int32_t *pair_out, int32_t *split_tab);
/* dW[k][ci][co] = sum over the pairs of offset k of feat[pair_in][ci] * dout[pair_out][co] (feat n_in x cin, dout n_out x
 * cout, dW kvol x cin x cout, all dense row-major) on v_mfma_f32_32x32x2_f32: exact products, one rounding per step.
 * PINNED ORDER: an element of a split's result is ONE accumulator, started at +0 and fed by the split's pairs ascending (the
 * waves of a workgroup tile (cin, cout) or take different splits, never the pairs of one split); a second launch adds each
 * offset's splits ascending from the first one's value, and writes +0 for an offset without pairs: every element of dW is
 * written.  The result is a function of the ordered pair list and the rows it names alone -- not of cap, of rows that hold no
 * pair, or of the launch.  No float atomics, no waiting on counters.  Against exact arithmetic an element is off by at most
 * (DCL_CONV_PAIRS_SPLIT + splits_k + 2) * 2^-24 * sum |x| |g|.  Any cin, cout >= 1 (zero-filled lanes; 16-byte loads are only
 * the fast path of aligned rows).  Listed rows outside [0, n_in) / [0, n_out) read as zero rows and are never addresses.
 * max_splits: the rows of split_tab; partial: scratch of max_splits * cin * cout floats.  DCL_EINVAL as above.          */
int dcl_sparse_conv_wgrad_pairs(const float *feat, int n_in, const float *dout, int n_out, int cin, int cout, int kvol,
                                const int32_t *head, const int32_t *pair_in, const int32_t *pair_out,
                                const int32_t *split_tab, int max_splits, float *partial, float *dW, dclStream_t stream);
/* ---- the input gradient of indice_conv on a kernel of its own, in a pinned order (csrc/conv_dgrad.hip, conv_dgrad.h).
 *
 *   dx[i][ci] = sum_k sum_co dout[inv[k][i]][co] * W[k][ci][co]          i < n_in, ci < cin
 *
 * dout n_out x cout, dx n_in x cin, W kvol x cin x cout AS REGISTERED (no transposed copy), all dense row-major; inv kvol x
 * cap_in from dcl_rulebook_transpose.  An entry is a neighbour iff 0 <= inv[k][i] < n_out; any other entry takes no part and
 * is never an address, so rows of dout at or past n_out are never read.  fp32 MFMA (v_mfma_f32_32x32x2_f32): exact products,
 * one rounding per step.  PINNED ORDER: an element of dx is ONE accumulator, started at +0; offsets k ascending, an offset
 * that is no neighbour skipped, the channels co ascending inside an offset -- one fmaf chain, never split, which the host
 * twin runs literally.  The element is a function of its row's neighbours, of the dout rows they name and of W alone: not of
 * n_in, cap_in, other rows or the launch.  Every element of the n_in rows of dx is written, +0 for a row without neighbours;
 * nothing at or past row n_in is.  Any cin, cout >= 1 and kvol <= 27 through one body (zero-filled lanes; 16-byte loads are
 * only the fast path of aligned rows); W and the named rows of dout are taken to be finite.  No float atomics, no waiting on
 * counters, no scratch; one launch, capturable.  dcl_sparse_conv_dgrad_host is the same routine in plain C++ on HOST pointers
 * and makes no GPU call.  DCL_EINVAL before any GPU work for kvol outside 1..27, a negative size, cin or cout < 1, cap_in <
 * n_in, a NULL or misaligned buffer that a non-empty side needs; n_in == 0 or n_out == 0 is not an error.               */
int dcl_sparse_conv_dgrad(const float *dout, int n_out, const int32_t *inv, int cap_in, int n_in, const float *W, int cin,
                          int cout, int kvol, float *dx, dclStream_t stream);
int dcl_sparse_conv_dgrad_host(const float *dout, int n_out, const int32_t *inv, int cap_in, int n_in, const float *W, int cin,
                               int cout, int kvol, float *dx);
/* ---- the forward of indice_conv over the PRESENT (row, offset) pairs, in a pinned order (csrc/conv_fwd_compact.hip,
 * conv_fwd_compact.h): the second forward form, ops.sparse_conv(form="compact"), beside dcl_sparse_conv_fwd ("tiles").
 *
 *   out[o][co] = sum_k sum_ci feat[nbr[k][o]][ci] * W[k][ci][co]         o < n_out, co < cout
 *
 * feat n_in x cin, out n_out x cout, W kvol x cin x cout, all dense row-major; nbr kvol x cap (i32).  An entry is a neighbour
 * iff 0 <= nbr[k][o] < n_in; any other entry takes no part and is never an address, so rows of feat at or past n_in and rows
 * of nbr at or past n_out are never read.  fp32 MFMA (v_mfma_f32_32x32x2_f32): exact products, one rounding per step.
 * PINNED ORDER: an element of out is acc, started at +0; the offsets are visited in the forward's visiting order (k
 * ascending, the centre kvol / 2 first if subm != 0), an offset that is no neighbour skipped; a visited offset forms
 *   part = +0;  for ci = 0 .. cin - 1 ascending: part = fmaf(feat[nbr[k][o]][ci], W[k][ci][co], part)
 * and joins with ONE fp32 add, acc = acc + part -- the reference's own association (a GEMM per offset, then a scatter-add),
 * which the host twin runs literally.  The element is a function of its row's neighbours, of the feat rows they name and of W
 * alone: not of n_out, cap, other rows or the launch.  Every element of the n_out rows of out is written, +0 for a row
 * without neighbours; nothing at or past row n_out is.  Any cin, cout >= 1 and kvol <= 27, subm or not, through one body
 * (zero-filled lanes; 16-byte loads and stores are only the fast path of aligned rows); W and the named rows of feat are
 * taken to be finite.  No BatchNorm / ReLU epilogue.  No float atomics, no waiting on counters, no scratch, no stream-K; one
 * launch, capturable.  dcl_sparse_conv_fwd_compact_host is the same routine in plain C++ on HOST pointers and makes no GPU
 * call.  DCL_EINVAL before any GPU work for kvol outside 1..27, a negative size, cin or cout < 1, cap < n_out, a NULL or
 * misaligned buffer that a non-empty side needs; n_out == 0 returns 0 and touches nothing, n_in == 0 writes +0.          */
int dcl_sparse_conv_fwd_compact(const float *feat, int n_in, const int32_t *nbr, int cap, int n_out, const float *W, int cin,
                                int cout, int kvol, int subm, float *out, dclStream_t stream);
int dcl_sparse_conv_fwd_compact_host(const float *feat, int n_in, const int32_t *nbr, int cap, int n_out, const float *W, int cin,
                                     int cout, int kvol, int subm, float *out);
/* indice_avgpool backward (avgpool.cu:178-206): din[i] = sum_k asc dout[inv[k][i]] / (float)rf[inv[k][i]].  C % 4 == 0. */
int dcl_sparse_avgpool_bwd(const float *dout, const int32_t *inv, int cap_in, int n_in, const int32_t *rf, int c, int kvol,
                           float *din, dclStream_t stream);
/* three_interpolate_grad of libs/pointnet_sp (interpolate_gpu.cu:124-148): atomic scatter into a ZEROED (m,c) buffer.  */
int dcl_three_interpolate_grad_sp(int c, int n, int m, const float *grad_out, const int32_t *idx, const float *weight,
                                  float *grad_points_zeroed, dclStream_t stream);
/* The same gradient as an ordered gather (csrc/readout_grad.hip), what autograd.ThreeInterpolateFn uses: grad_points (m,c)
 * is WRITTEN WHOLE (rows nobody names get +0; the caller does not zero it); element [j][ch] is the sum, from +0, over the
 * flat positions q = 3p + k with idx[q] == j in ascending q of fmul(grad_out[p*grad_stride + ch], weight[q]), one rounded add
 * at a time -- numpy.add.at on float32 bit for bit, the same bits on every call, and one of the orders the atomic form can
 * take.  grad_out has row stride grad_stride >= c (floats): a column block of a wider tensor is read in place.  Indices
 * outside [0, m) contribute nothing and are never used as addresses; a query may name a row more than once.  ws: at least
 * the _ws_bytes of the same sizes (linear: 12 bytes per position, 8 per row, 4 KiB), 4-byte aligned.  No float atomics, no
 * read-back: capturable.  DCL_EINVAL before any device work for negative sizes, 3n >= 2^31 - 8192, m >= 2^30, c > 65535,
 * grad_stride < c, a null buffer of a non-empty problem or a short workspace; c == 0 or m == 0 does nothing; n == 0
 * zero-fills grad_points.  The size query needs no GPU.                                                                 */
int dcl_three_interpolate_grad_sp_ws_bytes(int c, int n, int m, int64_t *bytes_host);
int dcl_three_interpolate_grad_sp_ordered(int c, int n, int m, const float *grad_out, int64_t grad_stride,
                                          const int32_t *idx, const float *weight, float *grad_points,
                                          void *ws, int64_t ws_bytes, dclStream_t stream);
/* voxelize_bp (voxelize.cu:35-50): d_feats[rules[v][1+i]] += (average ? 1/n_v : 1) * d_out[v]; d_feats ZEROED (N,C).
 * The adds are atomic, as in the reference: a point that several voxels list receives them in an unspecified order (its sum
 * may differ in the last bit from call to call).  A voxelisation's rules list every point once: one add, the same bits.  */
int dcl_voxelize_bp(const float *d_out, const int32_t *rules, float *d_feats_zeroed, int n_rows, int max_active, int c,
                    int average, dclStream_t stream);

/* ---- a per-point Linear + ReLU stack's training side (the stage-2 refiner's MLP_share; csrc/linear_bwd.hip).  The input
 * gradient of such a layer is dcl_linear_dma_fwd with the registered (out, in) weight as its (K x N) matrix; these are the rest.
 *
 * Weight gradient: dW[p][q] = sum_{j < M} a[j][p] * b[j][q].  a = dZ (M x P, pitch lda >= P), b = the layer input (M x Q,
 * pitch ldb >= Q), dW (P x Q, pitch lddw >= Q: the Conv1d weight's own (out, in) layout; a column block of a wider gradient
 * is written in place and nothing beside it is touched).  fp32 MFMA (v_mfma_f32_32x32x2_f32), exact products.
 * PINNED ORDER: the M rows are cut into splits of DCL_WGRAD_ROWS rows, splits = dcl_linear_wgrad_splits(M) =
 * max(1, ceil(M / DCL_WGRAD_ROWS)) -- a function of M alone, never of P, Q, the device or its CU count.  Inside a split an
 * output element is ONE accumulator, started at +0 and fed by the split's rows in ascending order (the waves of a workgroup
 * tile (P, Q), never the rows); a second kernel adds the splits' results in ascending split order, one rounded add each.  No
 * float atomics and no workgroup waits on another: the same values give the same bits on every call, whatever the pitches and
 * the alignment.  Against exact arithmetic an element is therefore off by at most (DCL_WGRAD_ROWS + splits + 2) * 2^-24 *
 * sum_j |a_jp| |b_jq|.  partial: caller scratch of splits * P * Q floats.  Any P, Q >= 1, any M >= 0 (M == 0 zero-fills dW),
 * any pitches, any 4-byte aligned bases (16-byte aligned bases with pitches that are multiples of 4 floats load faster).
 * DCL_EINVAL before any GPU work for a NULL or misaligned pointer, a negative size, P or Q < 1, or a pitch below the width. */
#define DCL_WGRAD_ROWS 512
int dcl_linear_wgrad_splits(int M, int32_t *splits_host);
int dcl_linear_wgrad(const float *a, int64_t lda, const float *b, int64_t ldb, int M, int P, int Q, float *partial,
                     float *dW, int64_t lddw, dclStream_t stream);
/* The same weight gradient on the bf16 matrix pipe with fp32 results (csrc/linear_wgrad_split.hip): the arguments, shapes,
 * pitches, alignments, `partial` (dcl_linear_wgrad_splits(M) * P * Q floats, no other scratch) and DCL_EINVAL cases of
 * dcl_linear_wgrad; M == 0 zero-fills dW; a column block of a wider gradient is written in place and nothing beside it is
 * touched.  Every fp32 operand is the exact sum of three bf16 pieces h, m, l (the split of dcl_linear_split_fwd; both operands are
 * split inside the kernel, nothing is prepared) and a product a b is accumulated as its six piece products of weight >= 2^-16 in
 * the fp32 accumulators of v_mfma_f32_32x32x16_bf16.
 * PINNED ORDER: the M rows are cut into the splits of dcl_linear_wgrad (DCL_WGRAD_ROWS rows, dcl_linear_wgrad_splits(M) of them).
 * Inside a split an output element is ONE accumulator, started at +0; it is fed the split's 16-row chunks in ascending order and,
 * per chunk, the six products in the order al bh, ah bl, am bm, am bh, ah bm, ah bh (each one MFMA over the chunk's 16 rows).  The
 * waves of a workgroup tile (P, Q), never the rows; the kernel of dcl_linear_wgrad that adds the splits adds them here, ascending,
 * one rounded add each.  No float atomics and no workgroup waits on another; the order never depends on pitch or alignment: the
 * same values give the same bits on every call.  Rows past M and columns past P / Q are zero pieces, which add exact zeros.
 * Error: the piece products are exact; what is dropped (am bl + al bm + al bl) is below 1.5 * 2^-24 |a b| per product; counting
 * one rounding per piece product that enters an accumulator (6 per row, at most 6 * DCL_WGRAD_ROWS per split; the pieces'
 * magnitudes sum to at most 1.004 |v|) and one per added split, an element is off by at most
 *   (6 * DCL_WGRAD_ROWS + splits + 32) * 2^-24 * sum_j |a_jp| |b_jq|
 * against exact arithmetic -- the a-priori bound.  What it measures is the size of dcl_linear_wgrad's error: at most 1.5 x what
 * an fp32 FMA chain in the same order is off by (tests/test_gpu_linear_wgrad_split.py, on the operands of tests/split_cases.py).
 * Range (the split core's): operands of magnitude < 2^-110 lose up to 2^-126 |.| per product (third pieces below the bf16
 * range).  NOT supported: |v| >= 3.3962e38 (bits 0x7F7F8000: finite in fp32, inf as a bf16 first piece), +-inf and NaN -- such a
 * value in column p of a makes every dW[p][:] NaN, in column q of b every dW[:][q], also where dcl_linear_wgrad gives +-inf;
 * every other element has exactly the bits it has without that value. */
int dcl_linear_wgrad_split(const float *a, int64_t lda, const float *b, int64_t ldb, int M, int P, int Q, float *partial,
                           float *dW, int64_t lddw, dclStream_t stream);
/* ReLU mask + bias gradient of such a layer: h (M x P) is the layer's OUTPUT (after the ReLU),
 *   g != NULL:  dz[j][p] = h[j][p] > 0 ? g[j][p] : 0                       (g (M x P): the gradient that arrives; dz may be g),
 *   g == NULL:  dz[j][p] = h[j][p] > 0 ? roww[j] * gpool[j / rows_per_crop][p] : 0   (the pooled last layer: its output went
 *               into out[crop] = sum_j roww[j] h[j]; roww (M), gpool (crops x P, pitch ldgp) = the pooled gradient; the product
 *               is one rounded multiply; dz may be h),
 * and db[p] = sum_j dz[j][p] in the order of dcl_linear_wgrad: rows ascending inside a split of DCL_WGRAD_ROWS rows from +0 in
 * ONE FLOAT64 accumulator that is rounded to fp32 once per split, then the splits ascending, one rounded fp32 add each (off by
 * at most (splits + 1) * 2^-24 * sum_j |dz_jp|, far inside the (DCL_WGRAD_ROWS + splits) * 2^-24 * sum_j |dz_jp| of an fp32
 * chain); bit-identical call after call and in place or not.  h == 0 and NaN give 0.  partial: scratch of dcl_linear_wgrad_splits(M) * P floats; db (P).  Lanes run
 * over columns.  M == 0 zero-fills db.  DCL_EINVAL as above (the unused form's arguments are ignored). */
int dcl_relu_bwd(const float *h, int64_t ldh, const float *g, int64_t ldg, const float *roww, const float *gpool,
                 int64_t ldgp, int rows_per_crop, int M, int P, float *dz, int64_t lddz, float *partial, float *db,
                 dclStream_t stream);

/* ------------------------------------------------------------ crop builder ---
 * The per-object crop construction of the data loaders (YCBV/dataloader_test_YCBV.py:124-183), on the device, in the
 * reference's pixel order and float32/float64 arithmetic (results bit-identical to the numpy/torch code).
 *
 * dcl_crop_points (three launches: one workgroup per 4096-pixel chunk of a box -- one workgroup per instance for the
 * sequential centroid sum -- one workgroup per 4096-row chunk): pixels of box [rmin,rmax) x [cmin,cmax) with label == obj_ids[i] and
 * depth != 0, in ascending flat order (:128-133); back-projection pt2 = d/scale, pt0 = (col-cx)*pt2/fx,
 * pt1 = (row-cy)*pt2/fy (:147-154); rgb = float(double(float(v)/255) - mean) (:143-145); centroid = row-order running
 * float32 sum / n (np.mean(axis=0), :156); points centred; those with |x|,|y|,|z| < half_extent kept when more than
 * min_valid (32) of them exist, else all (:160-165).
 *   depth (H,W) u16, label (H,W) i32, rgb (H,W,rgb_channels) u8 -- device; boxes (n,4) i32 rmin,rmax,cmin,cmax (clipped
 *   to the image) and obj_ids (n) i32 -- device; cam_host = {cx, cy, fx, fy, scale, post_div}: the cloud is divided by
 *   post_div after back-projection (1000 for LineMOD, LM/dataloader_test_LM.py:156-160; 1 for YCB-V); always_filter: apply
 *   the grid filter whatever the count (LM eval mode, :197); cap >= every box area.
 *   raw_xyz/raw_rgb: scratch (n,cap,3); out_xyz/out_rgb (n,cap,3); centroid (n,3);
 *   counts (n,3) = {masked pixels, points inside the grid, rows written} (all zero: the reference skips the instance);
 *   ws: dcl_crop_points_ws_ints(n, cap) int32 of device scratch (chunk counts and offsets; zeroed by the call). */
int dcl_crop_points_ws_ints(int n_inst, int cap, int64_t *ints_host);
int dcl_crop_points(const uint16_t *depth, const int32_t *label, const uint8_t *rgb, int H, int W, int rgb_channels,
                    int n_inst, const int32_t *boxes, const int32_t *obj_ids, const float *cam_host,
                    const double *rgb_mean_host, const float *half_extent_host, int min_valid, int always_filter, int cap,
                    float *raw_xyz, float *raw_rgb, float *out_xyz, float *out_rgb, float *centroid,
                    int32_t *counts, int32_t *ws, dclStream_t stream);
/* dcl_crop_points over STACKED frames (the multi-frame eval builders, crops.py: CropBuilder.build_frames): depth / label
 * (n_frames,H,W), rgb (n_frames,H,W,rgb_channels); crop i reads frame src[i][5] of them, src (n_inst,6) i32 DEVICE rows
 * {rmin, rmax, cmin, cmax, class id, frame} (the row layout of dcl_crop_points_posed).  frame_idx_host (n_inst) is the HOST
 * copy of column 5: the call checks it against n_frames before any device work (DCL_EINVAL); a device row that disagrees and
 * names no frame gives an empty crop (counts row 0), never an address.  One camera (cam_host) for all frames; every other
 * argument, the scratch and ws as dcl_crop_points.  The same three kernel bodies (csrc/crops_body.h) without a pose:
 * out_xyz, out_rgb, centroid and counts of instance i are BIT FOR BIT what dcl_crop_points writes for that frame alone.   */
int dcl_crop_points_frames(const uint16_t *depth, const int32_t *label, const uint8_t *rgb, int n_frames, int H, int W,
                           int rgb_channels, int n_inst, const int32_t *frame_idx_host, const int32_t *src,
                           const float *cam_host, const double *rgb_mean_host, const float *half_extent_host,
                           int min_valid, int always_filter, int cap, float *raw_xyz, float *raw_rgb, float *out_xyz,
                           float *out_rgb, float *centroid, int32_t *counts, int32_t *ws, dclStream_t stream);
/* Sampled points -> feats rows [1,r,g,b,x,y,z] (n*npoint,7) and voxelize_idx input rows [instance,ix,iy,iz] (n*npoint,4)
 * i64 (:166-176,186-190): voxel = trunc((xyz + half_extent0)/unit) in float32, clamped to [0,voxel_limit-1] first for
 * instances with counts[i][1] <= min_valid.  sample_idx (n,npoint) i64 = the caller's np.random.choice draws (NULL:
 * identity, for the template clouds :179-182; then counts may be NULL).  xyz/rgb (n,cap,3).                          */
int dcl_crop_sample(int n_inst, int npoint, int cap, const float *xyz, const float *rgb, const int64_t *sample_idx,
                    const int32_t *counts, int min_valid, float half_extent0, const float *unit_host, int voxel_limit,
                    float *feats, int64_t *coords, dclStream_t stream);
/* ---- the sampling draws ON THE DEVICE (csrc/crop_draw.hip, csrc/crop_draw.h; crops.py: CropBuilder(draws="device"))
 * The loaders draw a crop's npoint points with np.random.choice on the host's MT19937 stream, which needs every instance's
 * point count on the host.  dcl_crop_draw is a DIFFERENT, fully specified sample of the same distribution, a pure function of
 * (seed, frame, instance row, counts row), made where the counts are.  All arithmetic is uint64, mod 2^64:
 *     G = 0x9E3779B97F4A7C15
 *     mix(z):  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  return z ^ (z >> 31)
 *     base(seed, frame, inst, s) = mix( mix( mix(seed + G) ^ (frame + G) ) ^ (2*inst + s + G) )
 *     key(j) = mix(base + (j + 1) * G)
 * inst = the row of counts (n_inst,3) i32 as dcl_crop_points writes it, m = counts[inst][2] the rows written.
 *   valid[inst] = counts[inst][0] > 0 && (keep_sparse || counts[inst][1] > min_valid) && m > 0      (the loaders' rule for "this
 *       instance gives a crop"; dcl_crop_points writes m = 0 under that rule only for LineMOD's eval mode with no point inside
 *       the grid, where the loader's own draw raises).  An instance that is not valid gets a row of zeros in sample_idx.
 *   m > npoint, stream s = 0, WITHOUT replacement: the npoint indices j in [0, m) with the smallest (key(j), j), in ascending
 *       (key, j) order -- the head of a uniform random permutation, np.argsort(keys, kind="stable")[:npoint].
 *   0 < m <= npoint, stream s = 1, WITH replacement: idx[j] = floor(key(j) * m / 2^64), the high half of the 128-bit product,
 *       for j in [0, npoint).
 * Pinned: base(1,0,0,0) = 0x6df1421574b0d586 with key(0), key(1) = 0x96c9f513020798b9, 0xf7dd055ed9ec356f; base(2,7,3,1) =
 * 0x9fb95fa8ca6188d9 with keys 0xc1bed6510d07ff6c, 0x3c33370239554870.
 * sample_idx (n_inst, npoint) i64 and valid (n_inst) i32 are written; counts, sample_idx, valid are DEVICE pointers.  One
 * workgroup per instance; keys are a function of the index, so the selection reads no memory: a guessed threshold, widened
 * while fewer than npoint keys lie under it, a most-significant-digit-first radix select where more lie under it than the LDS
 * list holds, a bitonic sort of the list.  The result is fixed by the definition above, not by the route; the kernel
 * terminates for every m < 2^31.  No float arithmetic, no global atomic, no scratch, no workgroup waits for another, nothing is
 * read back, no allocation: capturable.  DCL_EINVAL before any device work for npoint < 1 or > DCL_CROP_DRAW_MAX_POINTS,
 * n_inst < 0, or a null pointer of a non-empty call; n_inst == 0 returns 0 and launches nothing.
 *
 * dcl_crop_draw_keyed: dcl_crop_draw with a key PER ROW instead of (frame, row): keys (n_inst,2) u64 DEVICE rows
 * {frame, inst}, and row i draws with base(seed, keys[i][0], keys[i][1], s) on counts row i -- so row i equals row keys[i][1]
 * of dcl_crop_draw(..., frame = keys[i][0]) on the same counts row (one kernel body; the pinned constants above hold through
 * it).  A batch that stacks several frames draws what the frames draw one by one.  keys[i][1] < 2^31.  Same selection routes,
 * limits, DCL_EINVAL rules (keys is a required pointer of a non-empty call) and capturability.
 *
 * dcl_crop_sample_valid: dcl_crop_sample's rows (the same body, csrc/crops_body.h: the same bits) for every instance with
 * valid[inst] > 0 (0: no crop; < 0: not a crop at all, the padding rows of CropBuilder.build_frames(pad_to=...), which have
 * no xyz row and are never used as an address) (sample_idx required; an index is clamped to [0, cap - 1] before it addresses anything), and for the
 * others a LATTICE DUMMY CROP, S = voxel_limit: point j lies at the centre of voxel (ix, iy, iz) = (j mod S, (j div S) mod S,
 * j div S^2) -- feats row [1, 0, 0, 0, x, y, z] with x = (float(ix) + 0.5f) * unit[0] - half_extent0 (uncontracted; y, z alike),
 * coords row [inst, ix, iy, iz].  Requires npoint <= S^3 (and <= DCL_CROP_DRAW_MAX_POINTS).  Why not zeros: an instance
 * without a crop has no written xyz row to gather from, and npoint points in ONE voxel would raise the capacity form's pitch
 * flag (dcl_voxelize_idx_crops: info[2]) for the whole frame; the lattice has one point per voxel.
 *
 * dcl_crop_draw_host / dcl_crop_sample_valid_host: the same contracts in plain C++ on HOST pointers (csrc/crop_draw_host.cpp:
 * all m keys and a partial sort; the twins the tests compare the kernels with; no GPU call).  dcl_crop_draw_keys_host:
 * *base = base(seed, frame, inst, s) and keys[0..n) = key(0..n-1). */
#define DCL_CROP_DRAW_MAX_POINTS 4096
int dcl_crop_draw(int n_inst, int npoint, const int32_t *counts, int min_valid, int keep_sparse, uint64_t seed, uint64_t frame,
                  int64_t *sample_idx, int32_t *valid, dclStream_t stream);
int dcl_crop_draw_host(int n_inst, int npoint, const int32_t *counts, int min_valid, int keep_sparse, uint64_t seed,
                       uint64_t frame, int64_t *sample_idx, int32_t *valid);
int dcl_crop_draw_keys_host(uint64_t seed, uint64_t frame, int inst, int s, int n, uint64_t *base, uint64_t *keys);
int dcl_crop_draw_keyed(int n_inst, int npoint, const int32_t *counts, int min_valid, int keep_sparse, uint64_t seed,
                        const uint64_t *keys, int64_t *sample_idx, int32_t *valid, dclStream_t stream);
int dcl_crop_draw_keyed_host(int n_inst, int npoint, const int32_t *counts, int min_valid, int keep_sparse, uint64_t seed,
                             const uint64_t *keys, int64_t *sample_idx, int32_t *valid);
int dcl_crop_sample_valid(int n_inst, int npoint, int cap, const float *xyz, const float *rgb, const int64_t *sample_idx,
                          const int32_t *counts, int min_valid, const int32_t *valid, float half_extent0,
                          const float *unit_host, int voxel_limit, float *feats, int64_t *coords, dclStream_t stream);
int dcl_crop_sample_valid_host(int n_inst, int npoint, int cap, const float *xyz, const float *rgb, const int64_t *sample_idx,
                               const int32_t *counts, int min_valid, const int32_t *valid, float half_extent0,
                               const float *unit_host, int voxel_limit, float *feats, int64_t *coords);
/* The loaders' `get_bbox(mask_to_bbox(mask_label, padding))` (LM/dataloader_test_LMO.py:26-42,215,360-402; the LineMOD loader's
 * eval mode, LM/dataloader_test_LM.py:144) for n label images (n,H,W) i32 (csrc/mask_box.hip; semantics: csrc/mask_box.h).
 * A pixel is set where label == value; components are 8-connected; the winner is the component whose bounding rectangle
 * has the largest w*h, among equal ones the one whose first pixel in raster order comes last.  out (n,10) i32:
 *   [0:4]  box = [x - padding/2, y - padding/2, w + padding, h + padding] ([0,0,0,0] when no pixel is set)
 *   [4:8]  the box row dcl_crop_points takes: crops.lm_box(box, H, W), then max(r0,0), min(r1,H), max(c0,0), min(c1,W)
 *   [8]    number of components          [9]  pixel count of the winner
 * The tie rule and "a pixel on the image border is a pixel" are ASSUMPTIONS about cv2.findContours that are not pinned
 * against cv2 (absent where this project is built); neither matters for a mask with a unique largest rectangle away from
 * the border.  Six launches over runs of set pixels, integer atomics only, the same bits on every call; no workgroup waits
 * for another, nothing is read back, no allocation: capturable.  ws: dcl_mask_box_ws_bytes(n, H, W) bytes of device
 * scratch, 4-byte aligned, sized for the worst mask (H * ceil(W/2) runs per image; 4.9 MB per 480 x 640 image), not
 * zeroed by the caller.  dcl_mask_box_host: the same ten integers from host memory by a sequential route (the twin the
 * tests compare the kernels with; no GPU call).  DCL_EINVAL before any device work for a null pointer of a non-empty call,
 * H or W < 1, H*W >= 2^31 - 64, padding < 0 or a short workspace; n == 0 returns 0 and launches nothing.                  */
int dcl_mask_box_ws_bytes(int n, int H, int W, int64_t *bytes_host);
int dcl_mask_box(const int32_t *label, int n, int H, int W, int32_t value, int padding, int32_t *out, void *ws,
                 int64_t ws_bytes, dclStream_t stream);
int dcl_mask_box_host(const int32_t *label, int n, int H, int W, int32_t value, int padding, int32_t *out);

/* ---- the TRAINING loader's front end (YCBV/dataloader_train_YCBV.py:105-210; csrc/crops_train.hip)
 * Per-frame class table: for every frame of label (n,H,W) i32 / depth (n,H,W) u16 and every class id c in [0, n_classes),
 * out[frame][c] = { pixels with label == c && depth != 0 (`len(mask.nonzero()[0])`, :128-131),
 *                   min row, max row, min col, max col of label == c -- the LABEL alone, what get_bbox(mask_label) reduces
 *                   (:134,280-285) }.
 * An absent class: count 0, min = INT32_MAX, max = -1 (empty extent, min > max).  Labels outside [0, n_classes) take no
 * part and are never an address.  Two launches (identity fill; one pass over the pixels with per-workgroup tables in LDS
 * merged by integer atomics), integers only, no workgroup waits for another, nothing is read back: capturable, the same
 * bits on every call.  DCL_EINVAL before any device work: n < 0, H or W < 1, H*W >= 2^31 - 64, n_classes outside
 * [1, 256], a null pointer of a non-empty call; n == 0 returns 0.  dcl_label_table_host: the same integers from host
 * memory in plain C++ (no GPU call).                                                                                     */
int dcl_label_table(const int32_t *label, const uint16_t *depth, int n, int H, int W, int n_classes, int32_t *out,
                    dclStream_t stream);
int dcl_label_table_host(const int32_t *label, const uint16_t *depth, int n, int H, int W, int n_classes, int32_t *out);
/* dcl_crop_points for the training loader: the same masked back-projection, row-order centroid and ordered compaction, with
 *   per-crop source   crop i reads frame src[i][5] of the stacked depth / label (n_frames,H,W) and rgb (n_frames,H,W,C)
 *                     tensors; src (n_inst,6) i32 DEVICE rows {rmin, rmax, cmin, cmax, class id, frame}.  frame_idx_host
 *                     (n_inst) is the HOST copy of column 5: the call checks it against n_frames before any device work;
 *                     a device row that disagrees and names no frame gives an empty crop, never an address.
 *   per-crop camera   cams (n_inst,5) f32 DEVICE rows {cx, cy, fx, fy, depth scale} (:113-122,150)
 *   per-crop pose row pose (n_inst) DEVICE rows of DCL_CROP_POSE_ROW_BYTES = 112 bytes, little endian:
 *                       [  0: 24)  t_gt  3 x f64   meta['poses'][:, 3, idx]             (:136)
 *                       [ 24: 60)  R0    9 x f32   meta['poses'][:, 0:3, idx], row major (:135,169)
 *                       [ 60: 72)  j     3 x f32   the translation jitter                (:172)
 *                       [ 72:108)  A     9 x f32   aug_r = euler2mat(a1, a2, a3)         (:162-166)
 *                       [108:112)  padding
 * After the centroid one lane per crop forms t0 = f32(t_gt - f64(centroid)) (:159,168), t1 = t0 + j (:172) and
 * R1 = R0 A (:173); every centred point p goes through the loader's re-pose (:171-174) in float32, uncontracted, in this
 * order:  d = p - t0;  q_j = (d0 R0[0][j] + d1 R0[1][j]) + d2 R0[2][j];  r_i = (q0 R1[i][0] + q1 R1[i][1]) + q2 R1[i][2];
 * p' = r + t1  (R1[i][j] = (R0[i][0] A[0][j] + R0[i][1] A[1][j]) + R0[i][2] A[2][j]).  The grid filter |p'| < half_extent
 * (strict, :189) is ALWAYS applied, in order.  counts (n_inst,3) = {masked pixels of the box, points inside the grid, rows
 * written}; rows written = points inside the grid when there are more than min_valid (50, :191) of them, else 0 (the
 * loader's dummy sample).  rot_gt (n_inst,3,3) = R1, trans_gt (n_inst,3) = t1 (zeros for an empty mask).  out_xyz holds p'.
 * Other arguments, scratch and ws as dcl_crop_points (dcl_crop_points_ws_ints).  The pose never visits the host.
 * dcl_crop_repose_host: the arithmetic above in plain C++ for n CENTRED points (n,3) of one crop: out_xyz (n,3) = p' of
 * every point (unfiltered), out_R1 (9), out_t1 (3).                                                                      */
#define DCL_CROP_POSE_ROW_BYTES 112
int dcl_crop_points_posed(const uint16_t *depth, const int32_t *label, const uint8_t *rgb, int n_frames, int H, int W,
                          int rgb_channels, int n_inst, const int32_t *frame_idx_host, const int32_t *src,
                          const float *cams, const void *pose, const double *rgb_mean_host,
                          const float *half_extent_host, int min_valid, int cap, float *raw_xyz, float *raw_rgb,
                          float *out_xyz, float *out_rgb, float *centroid, int32_t *counts, float *rot_gt,
                          float *trans_gt, int32_t *ws, dclStream_t stream);
int dcl_crop_repose_host(const float *points, const void *pose_row, const float *centroid, int n, float *out_xyz,
                         float *out_R1, float *out_t1);

/* ---- the LineMOD TRAINING loader's front end (LM/dataloader_train_LM.py:125-222,293-348; csrc/crops_train_lm.hip)
 * dcl_mask_extent: what `occlude_with_another_object` needs of an object mask (:301-306,343), for n masks (n,H,W,3) u8.
 * out (n,6) i32, a row = { min row, max row, min col, max col of mask[:, :, 0] != 0 (`np.nonzero(mask[:, :, 0])`; an empty
 * mask: min = INT32_MAX, max = -1),  [4:6] = ONE int64 (little endian, 8-byte aligned: a row is 24 bytes): the sum of ALL
 * bytes of the mask, `mask.sum()` }.  Two launches (identity fill; one pass, per-workgroup reduction, integer atomics),
 * integers only, no workgroup waits for another, nothing is read back.  DCL_EINVAL: n < 0, H or W < 1,
 * H*W >= 2^31 - 64, a null pointer of a non-empty call; n == 0 returns 0.  dcl_mask_extent_host: the same in plain C++.
 *
 * dcl_occlude_paste: the compositing of :335-346 for n frames, into WORKING COPIES (the inputs are not modified):
 *   rgb (n,H,W,C) u8 with C >= 3, depth (n,H,W) u16, mask (n,H,W,3) u8            this frame
 *   other_rgb (n_other,H,W,3) u8, other_depth (n_other,H,W) u16, other_mask (n_other,H,W,3) u8   the occluder frames
 *   plan (n, DCL_PASTE_PLAN_INTS) i32 DEVICE rows, plan_host their HOST copy (crops.py::lm_paste_plan makes them):
 *       [0] enabled   0: the frame is copied through and only counted
 *       [1] other     the occluder frame of this frame, an index into other_*
 *       [2] py0 [3] px0   origin of the patch inside the occluder frame: the occluder mask's first row / column plus the
 *                         rows the loader's trims removed in front (the patch row window starts here)
 *       [4] ph  [5] pw    shape of the patch (rows of the window, columns)
 *       [6] ty0 [7] tx0   origin of the target rectangle inside this frame
 *       [8] th  [9] tw    shape of the target rectangle (numpy's clipped slice)
 *       [10] rep_y [11] rep_x   1: the patch has ONE row / column on this axis and numpy's broadcast repeats it
 *       [12..15] rmin, rmax, cmin, cmax   the crop box, clipped to the frame (counted for every frame)
 *   extent (n,6) i32    dcl_mask_extent's rows of `mask` (the original sums), DEVICE
 *   out_rgb (n,H,W,C), out_depth (n,H,W) u16, out_label (n,H,W) i32 = channel 0 of the mask afterwards (what
 *   dcl_crop_points_posed64 tests: label == 255 && depth != 0 is `mask_label * mask_depth`, :143-148)
 *   info (n,4) i64 = { committed, remaining mask sum = original - removed (what the decision is taken on; it stays so after
 *                      a roll-back), n_box_valid, what the paste removed }
 * Inside the target rectangle, per channel, with om the occluder mask's value at the patch pixel:
 *   rgb' = om == 0 ? rgb : other rgb;  mask' = om == 0 ? mask : 0;  depth' = om[channel 0] == 0 ? depth : other depth
 * (the loader's multiply-then-add: the two terms never overlap), outside it the copy equals the original.  The first launch
 * composites and adds what it removed from the mask to info[3] with integer atomics; the second one restores the rectangle
 * from the originals where the remaining sum (original - removed) is below 20 (:343-346), writes committed / remaining, and
 * counts n_box_valid = pixels of the box with label' == 255 && depth' != 0 (`len(choose)`, :157) -- no host decision, no
 * read-back, no float atomics, no workgroup waits for another.  DCL_EINVAL before any device work: the shape limits of
 * dcl_mask_extent, C < 3, null pointers, and a row of plan_host that names a pixel outside either frame, an occluder frame
 * that is not there, a patch that does not broadcast to its target (an axis must be equal, or 1 with its repeat flag) or a
 * box outside the frame.  A DEVICE row that disagrees is clamped: never an address.  dcl_occlude_paste_host: the same from
 * host memory in plain C++ (plan = host rows).
 *
 * dcl_crop_points_posed64: dcl_crop_points_posed in the precision of the LineMOD training loader, which applies the
 * jittered pose in FLOAT64 (`cloud - target_t` promotes the float32 cloud, :185; nothing is rounded until the FloatTensor
 * of the sampled rows, :209).  Same arguments, except:
 *   cams (n_inst,6) f32 rows {cx, cy, fx, fy, depth scale, post_div}: LineMOD's are (.., 1, 1000) -- the back-projection is
 *        made in millimetres and divided by 1000 afterwards (:168-173), float32 as in dcl_crop_points
 *   pose (n_inst) DEVICE rows of DCL_CROP_POSE_ROW64_BYTES = 192 bytes, little endian, all float64:
 *                       [  0: 24)  t_gt  3 x f64   cam_t_m2c / 1000.0                    (:154)
 *                       [ 24: 96)  R0    9 x f64   cam_R_m2c, row major                  (:153)
 *                       [ 96:120)  j     3 x f64   the translation jitter                (:186)
 *                       [120:192)  A     9 x f64   aug_r = euler2mat(a1, a2, a3)         (:183)
 *        (the 112-byte row of dcl_crop_points_posed holds t_gt as f64 and R0, j, A as f32: see above)
 *   half_extent_host: 3 DOUBLES, total_voxel_extent * 0.5 (:200)
 * One lane forms t0 = t_gt - (double)centroid, t1 = t0 + j, R1 = R0 A; every centred float32 point is widened and goes
 * through the re-pose of dcl_crop_points_posed, same order, double operands, uncontracted; |p'| < half_extent is tested on
 * the doubles (strict, always); out_xyz, rot_gt = f32(R1), trans_gt = f32(t1) are rounded to float32 once.  min_valid:
 * LineMOD's is 128 (:201).  dcl_crop_repose64_host: the arithmetic in plain C++ for n CENTRED points: out_xyz (n,3) = f32(p')
 * of every point, inside (n) u8 = the grid test on the doubles (NULL with half_extent NULL: not wanted), out_R1, out_t1. */
#define DCL_CROP_POSE_ROW64_BYTES 192
#define DCL_PASTE_PLAN_INTS 16
int dcl_mask_extent(const uint8_t *mask, int n, int H, int W, int32_t *out, dclStream_t stream);
int dcl_mask_extent_host(const uint8_t *mask, int n, int H, int W, int32_t *out);
int dcl_occlude_paste(const uint8_t *rgb, const uint16_t *depth, const uint8_t *mask, int n, int H, int W,
                      int rgb_channels, const uint8_t *other_rgb, const uint16_t *other_depth, const uint8_t *other_mask,
                      int n_other, const int32_t *plan_host, const int32_t *plan, const int32_t *extent, uint8_t *out_rgb,
                      uint16_t *out_depth, int32_t *out_label, int64_t *info, dclStream_t stream);
int dcl_occlude_paste_host(const uint8_t *rgb, const uint16_t *depth, const uint8_t *mask, int n, int H, int W,
                           int rgb_channels, const uint8_t *other_rgb, const uint16_t *other_depth,
                           const uint8_t *other_mask, int n_other, const int32_t *plan, const int32_t *extent,
                           uint8_t *out_rgb, uint16_t *out_depth, int32_t *out_label, int64_t *info);
int dcl_crop_points_posed64(const uint16_t *depth, const int32_t *label, const uint8_t *rgb, int n_frames, int H, int W,
                            int rgb_channels, int n_inst, const int32_t *frame_idx_host, const int32_t *src,
                            const float *cams, const void *pose, const double *rgb_mean_host,
                            const double *half_extent_host, int min_valid, int cap, float *raw_xyz, float *raw_rgb,
                            float *out_xyz, float *out_rgb, float *centroid, int32_t *counts, float *rot_gt,
                            float *trans_gt, int32_t *ws, dclStream_t stream);
int dcl_crop_repose64_host(const float *points, const void *pose_row, const float *centroid, int n,
                           const double *half_extent, float *out_xyz, uint8_t *inside, float *out_R1, float *out_t1);

/* ------------------------------------------------------------ eval metric ---
 * ADD-S per object (tools/test_YCBV_stage1.py:186-189): out[o] = mean_i min_j |R_pred x_i + t_pred - (R_gt x_j + t_gt)|
 * over the P points of the object's class cloud.  cld (n_clouds, P, 3); cls i32[b] selects the cloud of object o
 * (NULL: cloud o).  partial_scratch: b * ceil(P/256) floats.  No (b,P,P,3) intermediate.                           */
int dcl_add_s(int b, int P, const float *cld, const int32_t *cls, const float *R_pred, const float *t_pred,
              const float *R_gt, const float *t_gt, float *partial_scratch, float *out, dclStream_t stream);

/* LineMOD metric (tools/test_LM.py:123-135).  dcl_add: ADD = mean_i |R_pred x_i + t_pred - (R_gt x_i + t_gt)| (the
 * reference's `l2_dis`, non-symmetric objects).  dcl_add_by_symmetry: per object, sym_flag[o] == 0 -> ADD, != 0 -> ADD-S
 * (`cd_dis`), one launch.  Same buffers as dcl_add_s.                                                                    */
int dcl_add(int b, int P, const float *cld, const int32_t *cls, const float *R_pred, const float *t_pred,
            const float *R_gt, const float *t_gt, float *partial_scratch, float *out, dclStream_t stream);
int dcl_add_by_symmetry(int b, int P, const float *cld, const int32_t *cls, const int32_t *sym_flag,
                        const float *R_pred, const float *t_pred, const float *R_gt, const float *t_gt,
                        float *partial_scratch, float *out, dclStream_t stream);

/* ------------------------------------------------- device-resident eval tables ---
 * The sufficient statistics of the three benchmarks' tables (dcl-net_amd/sharding.py: AddsTable, LmTable, LmoTable) as plain
 * device arrays, updated from device-side distances, class ids and the crop builder's `valid` -- nothing is read back
 * (csrc/metric_table.hip; the shared arithmetic: csrc/metric_table.h).
 *
 * dcl_add_traj: the distances of T poses per crop against ONE ground truth.  R_pred (T,b,3,3), t_pred (T,b,3), R_gt (b,3,3),
 * t_gt (b,3); cld (n_clouds,P,3); cls i32[b] picks crop i's cloud (NULL: cloud i, then n_clouds >= b); sym i32[b] / all_mode
 * as dcl_add_by_symmetry / dcl_add_s / dcl_add: sym given -> ADD where sym[i] == 0, ADD-S elsewhere; sym NULL -> all_mode 1 =
 * ADD-S, 0 = ADD.  partial_scratch: T * b * ceil(P/256) floats.  -> dis (T,b) fp32.  One workgroup per (crop, 256-point
 * slice) stages the ground-truth-posed cloud once and walks the T poses (three per scan of the staged cloud, as independent
 * minimum chains); per (pose, crop) the arithmetic is dcl_add_s's own (one shared device function, the one-pose order whatever
 * the grouping) and the slices are added in ascending order, so dis[t] has the bits of dcl_add_s / dcl_add /
 * dcl_add_by_symmetry called with pose t.  valid i32[b] or NULL: a crop with valid[i] == 0 does no work, its poses are not
 * read, dis[t,i] = +inf.  A cls[i] outside [0, n_clouds) reads no cloud and gives +inf as well.  Two launches.
 * P * 12 <= 150 KiB, b <= 65535, T >= 1; b == 0 returns 0 without a launch; anything else, a NULL required pointer or
 * all_mode outside 0 / 1 returns DCL_EINVAL before any GPU work.
 *
 * The table of one benchmark, T steps (poses per crop), C classes -- the arrays a mode does not use may be NULL:
 *     sums   f64 (T,C,4)  [n, m, sum D, #(D < 0.02)]      DCL_TABLE_ADDS
 *     maxd   f64 (T,C)    max D over the valid D           DCL_TABLE_ADDS
 *     counts i64 (T,C,2)  [num, success]                   DCL_TABLE_LM, DCL_TABLE_LMO   (+ diameter f64 (C), device)
 *     bad    i32 (1)      raised (set to 1) by a class id outside [0, C); never cleared, never read by an update
 * dcl_metric_tabulate adds the crops of dis (T,b) fp32, cls i32[b], valid i32[b] or NULL to it.  PINNED: one launch, the grid
 * spans T, lane c owns class c and walks the crops i = 0 .. b-1 in ASCENDING order, updating its own entries only -- no
 * atomics, the same bits on every run.  Every comparison is made in DOUBLE on the exactly converted fp32 distance:
 * (double)d <= 0.1, (double)d < 0.02, (double)d < diameter[c]  (0.1f > 0.1 but 0.02f < 0.02 in double).  Per crop of class c:
 *     DCL_TABLE_ADDS  AddsTable.add:  n += 1;  if d <= 0.1: m += 1, sum D += d (float64), maxd = max(maxd, d);
 *                     if d < 0.02: that count += 1.  valid[i] == 0 is add(c, inf): n += 1 only.
 *     DCL_TABLE_LM    LmTable.add:    num += 1, success += d < diameter[c].  valid[i] == 0: dropped (a lost detection).
 *     DCL_TABLE_LMO   LmoTable:       as LM, but valid[i] == 0 is add_lost: num += 1.
 * NaN and +-inf take the branches these comparisons take (misses); they are never skipped and never reach sum D.  A class id
 * outside [0, C) updates nothing and raises bad[0].
 * THE THIRD STATE OF valid: valid[i] < 0 is "not a crop" (a padding row of a batch padded to a fixed size).  dcl_add_traj does
 * no work for it, does not read its poses and writes dis[t,i] = +inf; dcl_metric_tabulate, dcl_add_tabulate and the host twin
 * update NOTHING for it in any mode -- no entry, and not bad either, whatever its class id or cloud index.  valid[i] == 0 and
 * valid[i] > 0 mean what they mean above.  b == 0 returns 0 without a launch; T < 1, C < 1, b < 0, an unknown mode
 * or a NULL required pointer (dis, cls, bad, the mode's arrays) returns DCL_EINVAL before any GPU work.
 * dcl_metric_tabulate_host: the same contract in plain C++ on HOST pointers (csrc/metric_table_host.cpp; no GPU call).
 *
 * dcl_add_tabulate: one frame from poses to table in TWO launches -- dcl_add_traj's slice launch, then one launch that
 * finishes the distances and tabulates them (the same bits as dcl_add_traj followed by dcl_metric_tabulate).  cloud i32[b] or
 * NULL picks the clouds as dcl_add_traj's cls does; cls i32[b] is the table's class id; dis (T,b) or NULL also receives the
 * distances.  A cloud index outside [0, n_clouds) is tabulated as d = +inf and raises bad[0].                              */
#define DCL_TABLE_ADDS 0
#define DCL_TABLE_LM 1
#define DCL_TABLE_LMO 2
int dcl_add_traj(int T, int b, int P, int n_clouds, const float *cld, const int32_t *cls, const int32_t *sym, int all_mode,
                 const float *R_pred, const float *t_pred, const float *R_gt, const float *t_gt, const int32_t *valid,
                 float *partial_scratch, float *dis, dclStream_t stream);
int dcl_metric_tabulate(int mode, int T, int b, int C, const float *dis, const int32_t *cls, const int32_t *valid,
                        const double *diameter, double *sums, double *maxd, int64_t *counts, int32_t *bad,
                        dclStream_t stream);
int dcl_metric_tabulate_host(int mode, int T, int b, int C, const float *dis, const int32_t *cls, const int32_t *valid,
                             const double *diameter, double *sums, double *maxd, int64_t *counts, int32_t *bad);
int dcl_add_tabulate(int mode, int T, int b, int P, int n_clouds, int C, const float *cld, const int32_t *cloud,
                     const int32_t *cls, const int32_t *sym, int all_mode, const float *R_pred, const float *t_pred,
                     const float *R_gt, const float *t_gt, const int32_t *valid, const double *diameter,
                     float *partial_scratch, float *dis, double *sums, double *maxd, int64_t *counts, int32_t *bad,
                     dclStream_t stream);

/* ------------------------------------------------------ training objective ---
 * Both-direction nearest-neighbour (Chamfer) distances of the point-set losses (models/DCL_Net.py:306-312 `CD_Dis`) without
 * the pairwise matrix (csrc/chamfer.hip).  pred (b,n,3), target (b,m,3) fp32 contiguous, any n, m >= 1.  One launch writes
 *   dist_pt (b,n) = min_j |pred_i - target_j|, idx_pt (b,n) i32 = that j;  dist_tp (b,m), idx_tp (b,m): the other way round.
 * Squared distance = fma(dz,dz, fma(dy,dy, dx*dx)) of fp32 differences (dcl_add_s's form); the minimum is taken on squared
 * distances by an ascending scan with strict '<' (the lowest index wins a tie, as in dcl_three_nn / dcl_knn); sqrt is
 * applied once, to the minimum.  active i32[b] (NULL: every crop): a crop whose flag is 0 does no distance work, its
 * distances are written as 0 and its indices as -1.  No workspace.                                                       */
int dcl_chamfer_fwd(int b, int n, int m, const float *pred, const float *target, const int32_t *active,
                    float *dist_pt, int32_t *idx_pt, float *dist_tp, int32_t *idx_tp, dclStream_t stream);
/* Gradients of that call with respect to both clouds.  idx_pt, idx_tp as dcl_chamfer_fwd returned them, g_pt (b,n) and
 * g_tp (b,m) the upstream gradients of dist_pt and dist_tp.  With u(p,t) = (p - t)/|p - t|, 0 where |p - t| = 0 (torch's
 * subgradient of norm at 0):
 *   grad_pred[i]   =  g_pt[i] u(p_i, t_idx_pt[i]) + sum_{j ascending, idx_tp[j] = i} g_tp[j] u(p_i, t_j)
 *   grad_target[j] = -g_tp[j] u(p_idx_tp[j], t_j) - sum_{i ascending, idx_pt[i] = j} g_pt[i] u(p_i, t_j)
 * (each term evaluated as (g / |p - t|) (p - t)).  grad_pred (b,n,3) and grad_target (b,m,3) are OVERWRITTEN; either may be
 * NULL and is then skipped (not both).  Crops whose flag is 0 get zero gradients; an index outside its cloud contributes
 * nothing.  One launch, one lane per output point, which adds its own term and then the incoming ones in ascending index
 * order: no float atomics, no workspace, no workgroup waits on another, bit-identical results call after call.
 * Both calls: n < 1, m < 1, b < 0, a NULL required pointer with b > 0 (or both gradient outputs NULL) return DCL_EINVAL
 * before any GPU call; b == 0 returns 0.                                                                                 */
int dcl_chamfer_bwd(int b, int n, int m, const float *pred, const float *target, const int32_t *active,
                    const int32_t *idx_pt, const int32_t *idx_tp, const float *g_pt, const float *g_tp,
                    float *grad_pred, float *grad_target, dclStream_t stream);

/* The rest of the objective (models/DCL_Net.py:264-304, models/refiner.py:101-125; csrc/objective.hip, csrc/objective.h).
 * All arrays fp32 contiguous.  fma(a,b,c) is one rounding; everything else is rounded operation by operation as written.
 *
 * PINNED ORDER of every per-crop sum below: one workgroup of 256 lanes per crop; lane l adds the terms of points l, l+256,
 * l+512, ... ascending into its own accumulator (from 0); the 256 accumulators are folded by a tree with strides 128, 64,
 * ..., 1 (slot l += slot l+stride for l < stride).  Crops are added afterwards in ascending order (from 0).  No float atomics:
 * the same inputs give the same bits.  The *_host entry points run the same routines on HOST pointers and make no GPU call.
 *
 * dcl_rigid_points: pts (b,n,3), R (b,3,3), t (b,3) -> out (b,n,3), one launch.
 *   inverse == 0: out_i = R p_i + t   (bmm(p, R^T) + t), row r = fma(R_r2,p_2, fma(R_r1,p_1, R_r0*p_0)) + t_r
 *   inverse == 1: out_i = R^T (p_i - t)   (bmm(p - t, R)), q = p_i - t, column c = fma(R_2c,q_2, fma(R_1c,q_1, R_0c*q_0))
 * dcl_rigid_points_bwd: g_out (b,n,3) -> g_R (b,3,3), g_t (b,3), g_pts (b,n,3; may be NULL: skipped), all OVERWRITTEN, one
 * launch.  Per point, accumulated in the pinned order:
 *   inverse == 0: g_R[r][c] = fma(g_r, p_c, g_R[r][c]); g_t[r] += g_r;        g_pts_i = R^T g_i
 *   inverse == 1: g_R[r][c] = fma(q_r, g_c, g_R[r][c]); g_t[r] -= (R g_i)_r;  g_pts_i = R g_i
 * b < 0, n < 1, inverse not 0 / 1, a NULL required pointer with b > 0 return DCL_EINVAL before any GPU call; b == 0 returns 0. */
int dcl_rigid_points(int b, int n, const float *pts, const float *R, const float *t, int inverse, float *out,
                     dclStream_t stream);
int dcl_rigid_points_bwd(int b, int n, const float *pts, const float *R, const float *t, int inverse, const float *g_out,
                         float *g_R, float *g_t, float *g_pts, dclStream_t stream);
int dcl_rigid_points_host(int b, int n, const float *pts, const float *R, const float *t, int inverse, float *out);
int dcl_rigid_points_bwd_host(int b, int n, const float *pts, const float *R, const float *t, int inverse,
                              const float *g_out, float *g_R, float *g_t, float *g_pts);
/* dcl_pose_objective_fwd: the per-point terms and their sums.  posed, posed_gt, Yc, cano_pred, cano_gt, Xo (b,n,3); conf
 * (b,2n); sym (b,) the float multiplier of the formula; cd_*_pt / cd_*_tp (b,n) the two halves dcl_chamfer_fwd returned for
 * (posed, posed_gt), (Xo, template) and (Yc, posed_gt).  With s = sym[crop], |a - b| = sqrt(fma(dz,dz, fma(dy,dy, dx*dx))):
 *   pose_i = (1-s) * |posed_i - posed_gt_i| + s * (0.5 * (cd_pose_pt_i + cd_pose_tp_i))
 *   LXo_i  = (1-s) * |Xo_i - cano_gt_i|  + (0.5*s) * (0.5 * (cd_Xo_pt_i + cd_Xo_tp_i) + |Xo_i - cano_pred_i|)
 *   LYc_i  = (1-s) * |Yc_i - posed_gt_i| + (0.5*s) * (0.5 * (cd_Yc_pt_i + cd_Yc_tp_i) + |Yc_i - posed_i|)
 *   conf terms  LXo_i * conf[i] - 0.01 * log(conf[i])  and  LYc_i * conf[n+i] - 0.01 * log(conf[n+i])
 * Outputs: L (b,2n) = [LXo | LYc] per crop (kept for the backward); crop_sums (b,5) = per crop, in the pinned order, the sums
 * of pose, LXo, LYc, the conf terms of the Xo half and those of the Yc half; packed (5,) = [loss_pose, loss_Xo, loss_Yc,
 * loss_conf, loss_all] with T_k = column k of crop_sums added over the crops ascending:
 *   loss_pose = T_0 / (b n), loss_Xo = T_1 / (b n), loss_Yc = T_2 / (b n), loss_conf = (T_3 + T_4) / (2 b n),
 *   loss_all = ((loss_pose + 5 * loss_Xo) + loss_Yc) + loss_conf.
 * Two launches (per-crop sums; one wave adds the crops).  conf <= 0 is not guarded: it gives what log gives.
 * Pose-only form (the refiner's loss): Yc, cano_pred, cano_gt, Xo, conf, cd_Xo_*, cd_Yc_* and L all NULL -> packed =
 * [loss_pose, 0, 0, 0, loss_pose]; only column 0 of crop_sums is meaningful.
 *
 * dcl_pose_objective_bwd: one launch, no reduction.  It takes the forward's clouds, conf, sym and L, not the Chamfer halves
 * (their gradients depend on sym alone).  g_packed (5,) is the DEVICE upstream gradient of packed; the weights
 *   W_pose = (g0 + g4) / (b n), W_Xo = fma(5, g4, g1) / (b n), W_Yc = (g2 + g4) / (b n), W_conf = (g3 + g4) / (2 b n)
 * are formed on the device.  With u_k(a, b) = (k / |a - b|) (a - b), 0 where |a - b| == 0 (torch.norm's subgradient):
 *   g_posed_i = u_{W_pose (1-s)}(posed_i, posed_gt_i)                   (posed is detached inside LYc)
 *   g_Xo_i    = u_{W_Xo (1-s)}(Xo_i, cano_gt_i)  + u_{W_Xo 0.5 s}(Xo_i, cano_pred_i)
 *   g_Yc_i    = u_{W_Yc (1-s)}(Yc_i, posed_gt_i) + u_{W_Yc 0.5 s}(Yc_i, posed_i)
 *   g_conf_j  = W_conf * (L_j - 0.01 / conf_j)                          (L is detached inside loss_conf)
 *   g_cd_pose_{pt,tp}_i = (W_pose s) * 0.5,  g_cd_Xo_{pt,tp}_i = (W_Xo 0.5 s) * 0.5,  g_cd_Yc_{pt,tp}_i = (W_Yc 0.5 s) * 0.5
 * All outputs OVERWRITTEN.  Pose-only form: the optional inputs, L and g_Xo, g_Yc, g_conf, g_cd_Xo_*, g_cd_Yc_* all NULL.
 * Both calls: b < 0, n < 1, a NULL required pointer or a PARTIAL set of the optional ones (with b > 0) return DCL_EINVAL
 * before any GPU call; b == 0 returns 0.                                                                                 */
int dcl_pose_objective_fwd(int b, int n, const float *posed, const float *posed_gt, const float *Yc, const float *cano_pred,
                           const float *cano_gt, const float *Xo, const float *conf, const float *sym,
                           const float *cd_pose_pt, const float *cd_pose_tp, const float *cd_Xo_pt, const float *cd_Xo_tp,
                           const float *cd_Yc_pt, const float *cd_Yc_tp, float *L, float *crop_sums, float *packed,
                           dclStream_t stream);
int dcl_pose_objective_bwd(int b, int n, const float *posed, const float *posed_gt, const float *Yc, const float *cano_pred,
                           const float *cano_gt, const float *Xo, const float *conf, const float *sym, const float *L,
                           const float *g_packed,
                           float *g_posed, float *g_Xo, float *g_Yc, float *g_conf, float *g_cd_pose_pt, float *g_cd_pose_tp,
                           float *g_cd_Xo_pt, float *g_cd_Xo_tp, float *g_cd_Yc_pt, float *g_cd_Yc_tp, dclStream_t stream);
int dcl_pose_objective_fwd_host(int b, int n, const float *posed, const float *posed_gt, const float *Yc,
                                const float *cano_pred, const float *cano_gt, const float *Xo, const float *conf,
                                const float *sym, const float *cd_pose_pt, const float *cd_pose_tp, const float *cd_Xo_pt,
                                const float *cd_Xo_tp, const float *cd_Yc_pt, const float *cd_Yc_tp, float *L,
                                float *crop_sums, float *packed);
int dcl_pose_objective_bwd_host(int b, int n, const float *posed, const float *posed_gt, const float *Yc,
                                const float *cano_pred, const float *cano_gt, const float *Xo, const float *conf,
                                const float *sym, const float *L, const float *g_packed, float *g_posed, float *g_Xo, float *g_Yc, float *g_conf,
                                float *g_cd_pose_pt, float *g_cd_pose_tp, float *g_cd_Xo_pt, float *g_cd_Xo_tp,
                                float *g_cd_Yc_pt, float *g_cd_Yc_tp);

/* ------------------------------------------------------ confidence pooling, channel-major, with its gradient ---
 * The pooling that ends stage 1's dense half on the differentiable module path (models/DCL_Net.py: conf_1 ... F_p_wei;
 * csrc/conf_pool_grad.hip, csrc/conf_pool_grad.h).  All arrays fp32 contiguous: F1 (b,c,n1), F2 (b,c,n2) channel-major, conf
 * and w (b, n1+n2) as dcl_conf_softmax leaves them (direction 1 first), L = n1 + n2.  Any c, n1, n2 >= 1; element offsets are
 * 64-bit.  fma(a,b,c) is one rounding; everything else is rounded operation by operation as written.  Per crop:
 *   pooled[c] = sum_{j<n1} w[j] F1[c][j] + sum_{j<n2} w[n1+j] F2[c][j]
 *   d[j]      = sum_c g_pooled[c] F[c][j]                  (F = F1 | F2 along j)
 *   dot       = sum_j w[j] d[j]
 *   ds[j]     = fma(w[j], d[j] - dot, g_conf[j])           (g_conf NULL: w[j] * (d[j] - dot))
 *   dlogit[j] = (ds[j] * s) * (1 - s),  s = conf[j]        (j < n1 -> dlogit1 (b,n1), else dlogit2 (b,n2))
 *   dF[c][j]  = g_pooled[c] * w[j]
 * PINNED ORDER of every sum, a function of c, n1, n2 alone (not of b, of the grid or of a row's alignment); no atomics:
 *   pooled: a row has 256 slots; slot k runs one fma chain from +0 over F1's columns k, k+256, ... ascending, then over F2's
 *     columns k, k+256, ... ascending (a missing column adds nothing); slots 4l .. 4l+3 fold as (s0 + s1) + (s2 + s3) into lane
 *     value l, and the 64 lane values by a butterfly with strides 32, 16, ..., 1 (v[l] = v[l] + v[l ^ stride]).
 *   d: channels in chunks of 256 (the last may be short); a chunk of a column is one fma chain from +0, channels ascending;
 *     the chunks are added ascending from chunk 0's value.
 *   dot: 256 lanes; lane l runs fma(w[j], d[j], acc) from +0 over j = l, l+256, ... ascending; the accumulators are folded by a
 *     tree with strides 128, 64, ..., 1 (slot l += slot l+stride for l < stride).
 * The same inputs give the same bits, and a crop gives the same bits alone as inside a batch.
 *
 * dcl_conf_pool_cm_fwd: w, F1, F2 -> pooled (b,c), one launch.
 * dcl_conf_pool_cm_bwd: g_pooled (b,c) and g_conf (b,L; may be NULL = zero) are the upstream gradients of pooled and conf.
 *   dlogit1 / dlogit2 are both given or both NULL, dF1 (b,c,n1) / dF2 (b,c,n2) likewise, not all four NULL; what is given is
 *   OVERWRITTEN.  The logits' gradient takes two launches (partials of d: F read once; the per-crop rest), dF one streaming
 *   write.  ws: scratch of at least dcl_conf_pool_cm_bwd_ws_bytes(b, c, n1, n2) bytes (the chunks' partials and d); read only
 *   when dlogit1 / dlogit2 are given, otherwise it may be NULL.
 * The *_host entry points run the same routines on HOST pointers, take no scratch and make no GPU call.
 * All: b < 0, c < 1, n1 < 1, n2 < 1, a NULL required pointer (with b > 0), an incomplete pair of outputs or too small a
 * ws_bytes return DCL_EINVAL before any GPU call; b == 0 returns 0.                                                      */
int dcl_conf_pool_cm_fwd(int b, int c, int n1, int n2, const float *w, const float *F1, const float *F2,
                         float *pooled, dclStream_t stream);
int dcl_conf_pool_cm_bwd_ws_bytes(int b, int c, int n1, int n2, int64_t *bytes_host);
int dcl_conf_pool_cm_bwd(int b, int c, int n1, int n2, const float *conf, const float *w, const float *F1,
                         const float *F2, const float *g_pooled, const float *g_conf,
                         float *dlogit1, float *dlogit2, float *dF1, float *dF2, void *ws, int64_t ws_bytes,
                         dclStream_t stream);
int dcl_conf_pool_cm_fwd_host(int b, int c, int n1, int n2, const float *w, const float *F1, const float *F2,
                              float *pooled);
int dcl_conf_pool_cm_bwd_host(int b, int c, int n1, int n2, const float *conf, const float *w, const float *F1,
                              const float *F2, const float *g_pooled, const float *g_conf,
                              float *dlogit1, float *dlogit2, float *dF1, float *dF2);

/* ------------------------------------------------------ confidence pooling, point-major, with its gradient ---
 * The same pooling on POINT-major activations (models/DCL_Net.py: train_dense = "point_major"; csrc/conf_pool_pm.hip,
 * csrc/conf_pool_pm.h).  All arrays fp32 contiguous: F1 (b n1, c), F2 (b n2, c) row-major, a point's channels contiguous, crop i
 * owning rows i n1 .. i n1 + n1 - 1 of F1 and likewise of F2; conf and w (b, n1+n2) as dcl_conf_softmax leaves them (direction 1
 * first), L = n1 + n2.  Any c, n1, n2 >= 1; element offsets are 64-bit.  Per crop, with F = F1 | F2 along j:
 *   pooled[c] = sum_{j<n1} w[j] F1[j][c] + sum_{j<n2} w[n1+j] F2[j][c]
 *   d[j]      = sum_c g_pooled[c] F[j][c]
 *   dot, ds[j], dlogit[j]   as for dcl_conf_pool_cm_bwd above (the same per-crop kernel and host routine)
 *   dF[j][c]  = g_pooled[c] * w[j]
 * PINNED ORDER of every sum, a function of c, n1, n2 alone (not of b, of the grid or of a row's alignment); no atomics:
 *   pooled: each direction's rows are cut into chunks of DCL_POOL_PM_ROWS rows (a direction's last chunk may be short, no chunk
 *     spans both directions); a chunk of a channel is one fma chain from +0, fma(w[j], F[j][c], p), rows ascending; the chunks
 *     are added ascending, all of F1's before F2's, from the first chunk's value: ((p_0 + p_1) + p_2) + ...
 *   d: a row has 256 slots; slot k runs one fma chain from +0, fma(g_pooled[c], F[j][c], s), over channels k, k+256, ...
 *     ascending (a missing channel adds nothing); slots 4l .. 4l+3 fold as (s0 + s1) + (s2 + s3) into lane value l, and the 64
 *     lane values by a butterfly with strides 32, 16, ..., 1 (v[l] = v[l] + v[l ^ stride]).
 *   dot: as above (256 lanes, tree with strides 128, ..., 1).
 * 16-byte and float-by-float accesses give the same bits (every channel of pooled and every slot of d has its own chain); the
 * same inputs give the same bits, and a crop gives the same bits alone as inside a batch.
 *
 * dcl_conf_pool_pm_fwd: w, F1, F2 -> pooled (b,c), one launch, F read once; no scratch (the chunks meet in LDS).
 * dcl_conf_pool_pm_bwd: arguments and rules of dcl_conf_pool_cm_bwd.  The logits' gradient takes three launches (d of each
 *   direction: F read once; the per-crop rest), dF one streaming write per direction.  ws: scratch of at least
 *   dcl_conf_pool_pm_bwd_ws_bytes(b, c, n1, n2) bytes (d: b L floats); read only when dlogit1 / dlogit2 are given, otherwise
 *   it may be NULL.
 * The *_host entry points run the same routines on HOST pointers, take no scratch and make no GPU call.
 * All: b < 0, c < 1, n1 < 1, n2 < 1, a NULL required pointer (with b > 0), an incomplete pair of outputs or too small a
 * ws_bytes return DCL_EINVAL before any GPU call; b == 0 returns 0.                                                      */
#ifndef DCL_POOL_PM_ROWS
#define DCL_POOL_PM_ROWS 64        /* rows per chunk of pooled; measured against 16, 32 and 128 (profiles/dense_pm.txt) */
#endif
int dcl_conf_pool_pm_fwd(int b, int c, int n1, int n2, const float *w, const float *F1, const float *F2,
                         float *pooled, dclStream_t stream);
int dcl_conf_pool_pm_bwd_ws_bytes(int b, int c, int n1, int n2, int64_t *bytes_host);
int dcl_conf_pool_pm_bwd(int b, int c, int n1, int n2, const float *conf, const float *w, const float *F1,
                         const float *F2, const float *g_pooled, const float *g_conf,
                         float *dlogit1, float *dlogit2, float *dF1, float *dF2, void *ws, int64_t ws_bytes,
                         dclStream_t stream);
int dcl_conf_pool_pm_fwd_host(int b, int c, int n1, int n2, const float *w, const float *F1, const float *F2,
                              float *pooled);
int dcl_conf_pool_pm_bwd_host(int b, int c, int n1, int n2, const float *conf, const float *w, const float *F1,
                              const float *F2, const float *g_pooled, const float *g_conf,
                              float *dlogit1, float *dlogit2, float *dF1, float *dF2);

/* ------------------------------------------------------ sparse-conv BatchNorm + ReLU, train mode, with its gradient ---
 * nn.BatchNorm1d -> nn.ReLU on the (rows, c) row-major feature matrix of a sparse tensor, in train mode (models/Modules.py:
 * BasicBlock_SPCONV.norm_form = "fused"; csrc/bn_relu.hip, csrc/bn_relu.h).  x, g, z, dx fp32 contiguous (V = rows, C = c);
 * gamma, beta, mean, invstd, the running statistics and dgamma / dbeta hold c floats.  Any c >= 1, rows >= 2; element offsets
 * are 64-bit.  Every operation is rounded as written (no contraction).  Per channel:
 *   float64:  mean = S1 / V,  var = max(S2 / V - mean^2, 0),  invstd = 1 / sqrt(var + (double)eps),  S1 = sum x, S2 = sum x^2;
 *             mean and invstd are rounded to fp32 once and are what the apply and the backward use
 *   fp32:     running_mean = (1 - m) running_mean + m mean;  running_var = (1 - m) running_var + m (float)(var V / (V - 1))
 *   fp32:     xhat = (x - mean) invstd;  y = xhat gamma + beta;  z = y > 0 ? y : 0          (relu = 0: z = y)
 *   backward: dy = (relu == 0 || y > 0) ? g : 0, y recomputed from x by the same expression, hence the same bits;
 *             T1 = sum dy, T2 = sum dy xhat in float64;  dbeta = (float)T1;  dgamma = (float)T2;
 *             mb = (float)(T1 / V);  mg = (float)(T2 / V);  a = gamma invstd;  dx = a ((dy - mb) - xhat mg)
 * PINNED ORDER of S1, S2, T1, T2, a function of (V, C) alone (not of the grid, of a pointer's alignment or of the load path);
 * float64 throughout, no atomics:
 *   the rows are cut into chunks of DCL_BN_ROWS rows (the last may be short), the channels into groups of 4 adjacent ones,
 *   G = ceil(C / 4).  Inside a chunk a channel has S slots, S = floor(256 / min(G, 16)); slot s adds the
 *   chunk's rows s, s + S, s + 2S, ... ascending from +0.0 (acc = acc + (double)v; acc2 = acc2 + (double)v * (double)w with an
 *   exact product); the S slot values are added ascending from +0.0 into the chunk's partial; the chunks' partials are added
 *   ascending from +0.0.  16-byte and float-by-float accesses feed the same accumulators in the same order.
 * The same inputs give the same bits.  Non-finite inputs propagate as they fall; nothing is promised for them.
 *
 * dcl_bn_relu_fwd: three launches (chunk sums, finish, apply).  running_mean / running_var are both given or both NULL; when
 *   given they are updated by the finish launch (no host read-back).  mean, invstd (c floats) and z (rows, c) are OVERWRITTEN.
 * dcl_bn_relu_bwd: g (rows, c) is the upstream gradient of z.  dx (rows, c) may be NULL and may be g itself; dgamma / dbeta are
 *   both given or both NULL; not all three NULL.  Two launches (chunk sums, finish) and one more for dx.
 * ws: scratch of at least dcl_bn_relu_ws_bytes(rows, c) bytes (the chunks' float64 partials, then mb and mg), 8-byte aligned.
 * The *_host entry points run the same routines on HOST pointers, take no scratch and make no GPU call.
 * All: rows < 0, rows == 1 (no variance, as torch refuses it), c < 1, a NULL required pointer, half a pair, relu other than
 * 0 / 1, eps < 0, momentum outside [0, 1] or too small a ws_bytes return DCL_EINVAL before any GPU call; rows == 0 returns 0. */
#ifndef DCL_BN_ROWS
#define DCL_BN_ROWS 256
#endif
int dcl_bn_relu_ws_bytes(int64_t rows, int c, int64_t *bytes_host);
int dcl_bn_relu_fwd(int64_t rows, int c, const float *x, const float *gamma, const float *beta, float eps, float momentum,
                    float *running_mean, float *running_var, float *mean, float *invstd, float *z, int relu,
                    void *ws, int64_t ws_bytes, dclStream_t stream);
int dcl_bn_relu_bwd(int64_t rows, int c, const float *x, const float *gamma, const float *beta, const float *mean,
                    const float *invstd, const float *g, int relu, float *dx, float *dgamma, float *dbeta,
                    void *ws, int64_t ws_bytes, dclStream_t stream);
int dcl_bn_relu_fwd_host(int64_t rows, int c, const float *x, const float *gamma, const float *beta, float eps,
                         float momentum, float *running_mean, float *running_var, float *mean, float *invstd, float *z,
                         int relu);
int dcl_bn_relu_bwd_host(int64_t rows, int c, const float *x, const float *gamma, const float *beta, const float *mean,
                         const float *invstd, const float *g, int relu, float *dx, float *dgamma, float *dbeta);

/* ------------------------------------------------------ narrow per-point layer, with its gradients ---
 * A per-point linear layer with very few output columns -- the last layers (1 or 3 columns) of stage 1's per-point heads -- for
 * the training path (models/DCL_Net.py: train_heads = "kernels"; csrc/linear_narrow.hip, csrc/linear_narrow.h).  fp32:
 *   y[m][j]  = sum_k x[m][k] W[j][k] + bias[j]          x (M, K) with a row pitch of x_pitch floats (>= K: a column block of a
 *   dx[m][k] = sum_j g[m][j] W[j][k]                    wider matrix is served as it lies), W (N, K) as the convolution registers
 *   dW[j][k] = sum_m g[m][j] x[m][k]                    it (no transposed copy), bias (N) or NULL, y, g (M, N) and dx (M, K)
 *   db[j]    = sum_m g[m][j]                            dense.  1 <= N <= DCL_NARROW_MAX_N, any K >= 1, any M >= 0.
 * Nothing needs an alignment; element offsets are 64-bit.  Bandwidth-bound: the forward reads x once, the backward reads x and g
 * once and writes dx once as a stream, the dW / db partials formed in the same pass.
 * PINNED ORDER of every sum, a function of (M, K, N) alone (not of the grid, of the pitch or of a pointer's alignment); no atomics:
 *   y: a row has 64 slots; slot k = 4 l + e of lane l < 16 runs one fma chain from +0, fma(x[m][c], W[j][c], s), over the columns
 *     k, k+64, k+128, ... ascending (a missing column adds nothing); slots 4l .. 4l+3 fold as (s0 + s1) + (s2 + s3) into lane value
 *     l, and the 16 lane values by a butterfly with strides 8, 4, 2, 1 (v[l] = v[l] + v[l ^ stride]); then + bias[j].
 *   dx: one fma chain from +0 over the outputs, fma(g[m][j], W[j][k], d), j ascending.
 *   dW, db: the rows are cut into chunks of DCL_NARROW_ROWS rows (the last may be short); a chunk of an element is one chain from
 *     +0, rows ascending -- fma(g[m][j], x[m][k], p) for dW, p + g[m][j] for db; a finish launch adds the chunks ascending from the
 *     first chunk's value: ((p_0 + p_1) + p_2) + ...
 * 16-byte and float-by-float accesses give the same bits (every element has its own chain), any pitch and any alignment give the
 * same bits, and the same inputs give the same bits.
 *
 * dcl_linear_narrow_fwd: one launch.
 * dcl_linear_narrow_bwd: any subset of dx, dW (N, K), db (N) is given, the others NULL; not all NULL.  One launch for dx and
 *   the partials, one more (the finish) when dW or db is given.  ws: scratch of at least dcl_linear_narrow_bwd_ws_bytes(M, K, N)
 *   bytes (the chunks' partials), read only when dW or db is given, otherwise it may be NULL.
 * The *_host entry points run the same routines on HOST pointers, take no scratch and make no GPU call.
 * All: M < 0, K < 1, N < 1, N > DCL_NARROW_MAX_N, x_pitch < K (with M > 1), a NULL required pointer (with M > 0), no output at
 * all or too small a ws_bytes return DCL_EINVAL before any GPU call; M == 0 returns 0 and writes nothing.                    */
#define DCL_NARROW_MAX_N 16        /* widest layer served: the accumulators of all outputs live in registers */
#ifndef DCL_NARROW_ROWS
#define DCL_NARROW_ROWS 64         /* rows per chunk of dW / db */
#endif
int dcl_linear_narrow_fwd(int64_t M, int K, int N, const float *x, int64_t x_pitch, const float *W, const float *bias,
                          float *y, dclStream_t stream);
int dcl_linear_narrow_bwd_ws_bytes(int64_t M, int K, int N, int64_t *bytes_host);
int dcl_linear_narrow_bwd(int64_t M, int K, int N, const float *x, int64_t x_pitch, const float *W, const float *g,
                          float *dx, float *dW, float *db, void *ws, int64_t ws_bytes, dclStream_t stream);
int dcl_linear_narrow_fwd_host(int64_t M, int K, int N, const float *x, int64_t x_pitch, const float *W, const float *bias,
                               float *y);
int dcl_linear_narrow_bwd_host(int64_t M, int K, int N, const float *x, int64_t x_pitch, const float *W, const float *g,
                               float *dx, float *dW, float *db);

/* ------------------------------------------------------ the two pose heads in training, with their gradients ---
 * The rotation and the translation head on the b pooled rows of a training step (models/DCL_Net.py, models/refiner.py:
 * train_heads = "kernels"; csrc/pose_heads_grad.hip, csrc/pose_heads_grad.h).  Each head is three layers on x (b, d0):
 *   h1 = relu(x W0^T + b0) (b, d1),  h2 = relu(h1 W1^T + b1) (b, d2),  out = h2 W2^T + b2 (b, n_rot | n_trans)
 * with the weights as the convolutions register them -- W0 (d1, d0), W1 (d2, d1), W2 (n, d2), read in that layout, nothing folded
 * or transposed.  The r.. arguments are the rotation head's, the t.. ones the translation head's.  All arrays fp32 contiguous;
 * h1 (2, b, d1) and h2 (2, b, d2) hold the rotation head's activations first.  Both heads share every launch, and a weight matrix
 * is read once per launch for all b rows.  The values are NOT the eval kernels' bits (dcl_pose_heads: folded, transposed weights
 * and other slice orders).
 * Accepted: any b >= 0; d0, d1, d2 multiples of 4 in [4, DCL_POSE_TRAIN_MAX_WIDTH] (the model's 1024, 512, 128); 1 <= n_rot,
 * n_trans <= DCL_POSE_TRAIN_MAX_OUT (the model's 9 and 3); x, the weight matrices, h1, h2, dx, the weight gradients and ws 16-byte
 * aligned.  Anything else returns DCL_EINVAL.
 * PINNED ORDER of every sum, a function of the widths alone (not of b, of the grid or of the outputs asked for); no atomics:
 *   z[r][o]: 256 slots; slot k = 4 l + e of lane l < 64 runs one fma chain from +0, fma(in[r][c], W[o][c], s), over the columns
 *     k, k+256, ... ascending; slots fold as (s0 + s1) + (s2 + s3), the 64 lane values by a butterfly with strides 32, ..., 1;
 *     then + bias[o]; relu is z > 0 ? z : 0.
 *   dW[o][k], db[o]: one chain from +0, rows ascending: fma(dz[r][o], in[r][k], p) and p + dz[r][o].
 *   input gradients: a layer's outputs are cut into chunks of DCL_POSE_TRAIN_CHUNK (the last may be short); a chunk is one fma
 *     chain from +0, fma(dz[r][o], W[o][k], p), outputs ascending; the chunks are added ascending from the first chunk's value.
 *     dz of the layer below = h > 0 ? that sum : 0, the mask recomputed from the stored activation.  dx = R + T: the rotation
 *     head's sum, then the translation head's.
 * The same inputs give the same bits, and a crop gives the same o9, t3 and dx bits alone as inside a batch.
 *
 * dcl_pose_heads_train_fwd: three launches (one per layer); h1, h2, o9 (b, n_rot) and t3 (b, n_trans) are overwritten.
 * dcl_pose_heads_train_bwd: g_o9 (b, n_rot) and / or g_t3 (b, n_trans), the upstream gradients; a NULL one is a zero gradient.
 *   dx (b, d0) and the twelve parameter gradients (shaped as their parameters) may each be NULL, not all of them.  At most six
 *   launches: per layer one for dW, db and the chunk partials of the input gradient, one that adds the chunks and masks.
 *   ws: scratch of at least dcl_pose_heads_train_bwd_ws_bytes(...) bytes, always required.
 * The *_host entry points run the same orders on HOST pointers, take no scratch, need no alignment and make no GPU call.
 * b == 0 returns 0 and writes nothing; a NULL required pointer, no gradient or no output at all, too small a ws_bytes return
 * DCL_EINVAL before any GPU call.                                                                                          */
#define DCL_POSE_TRAIN_MAX_WIDTH 1024   /* a weight row of an output lives in one wave's registers */
#define DCL_POSE_TRAIN_MAX_OUT 16
#define DCL_POSE_TRAIN_CHUNK 32         /* outputs per chain of an input gradient: the weight tile of a chunk fills 32 KB of LDS */
int dcl_pose_heads_train_fwd(int b, int d0, int d1, int d2, int n_rot, int n_trans, const float *x, const float *rW0,
                             const float *rb0, const float *rW1, const float *rb1, const float *rW2, const float *rb2,
                             const float *tW0, const float *tb0, const float *tW1, const float *tb1, const float *tW2,
                             const float *tb2, float *h1, float *h2, float *o9, float *t3, dclStream_t stream);
int dcl_pose_heads_train_bwd_ws_bytes(int b, int d0, int d1, int d2, int n_rot, int n_trans, int64_t *bytes_host);
int dcl_pose_heads_train_bwd(int b, int d0, int d1, int d2, int n_rot, int n_trans, const float *x, const float *rW0,
                             const float *rW1, const float *rW2, const float *tW0, const float *tW1, const float *tW2,
                             const float *h1, const float *h2, const float *g_o9, const float *g_t3, float *dx, float *d_rW0,
                             float *d_rb0, float *d_rW1, float *d_rb1, float *d_rW2, float *d_rb2, float *d_tW0, float *d_tb0,
                             float *d_tW1, float *d_tb1, float *d_tW2, float *d_tb2, void *ws, int64_t ws_bytes,
                             dclStream_t stream);
int dcl_pose_heads_train_fwd_host(int b, int d0, int d1, int d2, int n_rot, int n_trans, const float *x, const float *rW0,
                                  const float *rb0, const float *rW1, const float *rb1, const float *rW2, const float *rb2,
                                  const float *tW0, const float *tb0, const float *tW1, const float *tb1, const float *tW2,
                                  const float *tb2, float *h1, float *h2, float *o9, float *t3);
int dcl_pose_heads_train_bwd_host(int b, int d0, int d1, int d2, int n_rot, int n_trans, const float *x, const float *rW0,
                                  const float *rW1, const float *rW2, const float *tW0, const float *tW1, const float *tW2,
                                  const float *h1, const float *h2, const float *g_o9, const float *g_t3, float *dx,
                                  float *d_rW0, float *d_rb0, float *d_rW1, float *d_rb1, float *d_rW2, float *d_rb2,
                                  float *d_tW0, float *d_tb0, float *d_tW1, float *d_tb1, float *d_tW2, float *d_tb2);

/* ------------------------------------------------------ optimizer step ---
 * What follows loss.backward() in the reference's training scripts (tools/train_YCBV_stage1.py:119-125, 212-231): the global
 * gradient norm that AutoClip measures, and the Adam update with the clip factor folded in (csrc/optim.hip).  Both calls walk
 * ALL parameter tensors in one launch, driven by two device tables.
 *   Tensor table, dclOptimTensor[n_tensors]: only the tensors that have a gradient this step.  The four arrays hold `numel`
 *     (>= 1) contiguous fp32 each; they need no alignment.  step_size = lr / (1 - beta1^t) and bc2_sqrt = sqrt(1 - beta2^t),
 *     evaluated by the host in double from THIS tensor's step count t (1 at its first update) and rounded once to fp32, so a
 *     tensor that had no gradient in some earlier step still gets its own corrections.  dcl_grad_sqnorm reads grad and numel only.
 *   Chunk table, chunk_tensor[n_chunks] / chunk_begin[n_chunks]: chunk c covers the elements [chunk_begin[c],
 *     min(chunk_begin[c] + DCL_OPTIM_CHUNK, numel)) of tensor chunk_tensor[c]; every element of every tensor lies in exactly
 *     one chunk, the chunks of a tensor are consecutive and ascending and the first begins at 0.  One 256-thread workgroup
 *     takes one chunk.  Where the chunk is full and its addresses are 16-byte aligned the lanes move 16-byte vectors (lane l
 *     holds the vectors l, l + 256, l + 512, l + 768 of the chunk, all loads issued before the first use), elsewhere scalars
 *     with the same element-to-lane map.                                                                                   */
#define DCL_OPTIM_CHUNK 4096
typedef struct dclOptimTensor {
  float *param;
  const float *grad;
  float *exp_avg;
  float *exp_avg_sq;
  int64_t numel;
  float step_size;
  float bc2_sqrt;
} dclOptimTensor;
/* sq_per_tensor[t] = sum of grad_t[i]^2 in float64, norm[0] = sqrt of their sum: the 2-norm of all gradients together.
 * Launch 1: workgroup c writes partials[c] = the sum of (double)g * (double)g (exact products) over its chunk: lane l adds its
 * elements 4 (l + 256 k) + j in the order k, j ascending, the 64 lanes of a wave combine by an xor butterfly (distances 32, 16,
 * .. 1) and the four wave sums are added as (w0 + w1) + (w2 + w3).  Launch 2, one workgroup: sq_per_tensor[t] = that tensor's
 * partials added in ascending chunk order, total = sq_per_tensor added in ascending tensor order, norm[0] = sqrt(total).
 * No atomics, no workgroup waits on another: the same inputs give the same bits in every call, and the result does not depend
 * on the grid.  partials: n_chunks doubles, sq_per_tensor: n_tensors, norm: one; the caller owns all three.                */
int dcl_grad_sqnorm(int n_tensors, const dclOptimTensor *table, int n_chunks, const int32_t *chunk_tensor,
                    const int64_t *chunk_begin, double *partials, double *sq_per_tensor, double *norm, dclStream_t stream);
/* torch.optim.Adam's update (no weight decay, no amsgrad) of every listed tensor in one launch, the gradient scaled by
 * grad_scale (the clip factor) on the way in.  Per element, in fp32, every line one correctly rounded operation after the
 * other in exactly this order (no contraction into fma; division and sqrtf are the correctly rounded ones):
 *     g' = g * grad_scale                       (grad_scale == 1.0f leaves g's bits alone)
 *     m  = m*beta1 + g'*omb1                    omb1 = (float)(1.0 - (double)beta1)
 *     v  = v*beta2 + (g'*g')*omb2               omb2 = (float)(1.0 - (double)beta2)
 *     d  = sqrtf(v)/bc2_sqrt + eps
 *     p  = p - step_size*(m/d)
 * This order is part of the contract (tests/test_gpu_optim.py compares bit for bit against it).  param, exp_avg and
 * exp_avg_sq are updated in place; grad is read only.
 * Both calls: a negative count, n_chunks < n_tensors, a NULL required pointer with n_tensors > 0, a non-finite grad_scale,
 * beta1 or beta2 outside [0, 1) and eps <= 0 return DCL_EINVAL before any GPU call; n_tensors == 0 returns 0 without a
 * launch.                                                                                                                  */
int dcl_adam_step(int n_tensors, const dclOptimTensor *table, int n_chunks, const int32_t *chunk_tensor,
                  const int64_t *chunk_begin, float grad_scale, float beta1, float beta2, float eps, dclStream_t stream);
/* dcl_adam_step with the clip factor read from DEVICE memory when the kernel runs (grad_scale_dev: one fp32, 4-byte aligned;
 * what dcl_autoclip_observe leaves at DCL_AUTOCLIP_SCALE_F32_OFFSET): the same kernel body and the same five lines, so a
 * factor of equal bits gives dcl_adam_step's bits.  The host cannot look at the factor: it is the producer's contract that it
 * lies in [0, 1].  A NULL grad_scale_dev (with n_tensors > 0) and everything dcl_adam_step refuses return DCL_EINVAL before
 * any GPU call.                                                                                                            */
int dcl_adam_step_dev(int n_tensors, const dclOptimTensor *table, int n_chunks, const int32_t *chunk_tensor,
                      const int64_t *chunk_begin, const float *grad_scale_dev, float beta1, float beta2, float eps,
                      dclStream_t stream);

/* AutoClip's arithmetic on the device (csrc/optim.hip; the shared functions: csrc/optim_clip.h): the history of gradient norms
 * is kept SORTED in device memory, one call inserts this step's norm and evaluates the reference's
 *     clip_value = np.percentile(history, percentile);  scale = min(1.0, clip_value / (norm + 1e-6))
 * (tools/train_YCBV_stage1.py:212-231) without a read-back.  n = the norms already held -- a HOST integer, the caller counts
 * its own calls; sorted_src = those n float64 ascending; norm = the device double dcl_grad_sqnorm wrote (x below).
 *   Key of the order: ascending numeric, a NaN of either sign behind everything else, all NaN equal.  Entries are norms:
 *     >= +0, +inf or NaN (an entry with the sign bit set is the caller's to refuse).  The new entry goes BEHIND equal ones.
 *   Launch 1, one lane per held entry (256-lane workgroups, at least one): lane i stores sorted_src[i] at sorted_dst[i], or
 *     at [i + 1] when it is behind x by the key; the lane whose entry is the last not behind x also stores x at [i + 1], lane 0
 *     stores it at [0] when every entry is behind x (or n == 0) and writes arrival[n] = x.  sorted_dst[0 .. n] and arrival[n]
 *     are written, each slot once, nothing beyond them; sorted_src and sorted_dst must not overlap (ping-pong buffers).
 *   Launch 2, one lane, with s = sorted_dst and every operation rounded on its own (no contraction into fma):
 *     m = n + 1;  vi = (m - 1) * (percentile / 100.0);  lo = floor(vi);  t = vi - lo;  hi = min(lo + 1, m - 1)
 *     a = s[lo];  b = s[hi];  d = b - a
 *     clip = (t >= 0.5) ? b - d * (1 - t) : a + d * t          numpy's `linear` method, its lerp included
 *     if clip is NaN: clip = the quiet NaN 0xFFF8000000000000  (only inf - inf makes one here; x86-64's bits for it)
 *     if s[m - 1] is NaN: clip = s[m - 1]                       np.percentile with a NaN anywhere returns that entry
 *     q = clip / (x + 1e-6);  scale = (q < 1.0) ? q : 1.0       Python's min(1.0, q): a NaN quotient gives 1.0
 *   out (DCL_AUTOCLIP_OUT_BYTES, 8-byte aligned): doubles {x, clip, scale} at bytes 0, 8, 16 and (float)scale, rounded once,
 *     at byte DCL_AUTOCLIP_SCALE_F32_OFFSET -- the pointer dcl_adam_step_dev takes.  scale is always in [0, 1].
 * Stream-ordered, plain 8-byte loads and stores (16 n bytes of traffic), no atomics, no workgroup waits on another, the result
 * does not depend on the grid, nothing is read back or allocated.  n < 0, n > DCL_AUTOCLIP_MAX_N, a percentile outside
 * [0, 100] (NaN included), a NULL pointer (sorted_src may be NULL with n == 0) and sorted_src == sorted_dst return DCL_EINVAL
 * before any work.
 * dcl_autoclip_observe_host: the same contract in plain C++ on HOST pointers (csrc/optim_clip_host.cpp; no GPU call).      */
#define DCL_AUTOCLIP_OUT_BYTES 32
#define DCL_AUTOCLIP_SCALE_F32_OFFSET 24
#define DCL_AUTOCLIP_MAX_N ((int64_t)1 << 31)
int dcl_autoclip_observe(int64_t n, const double *sorted_src, double *sorted_dst, double *arrival, const double *norm,
                         double percentile, void *out, dclStream_t stream);
int dcl_autoclip_observe_host(int64_t n, const double *sorted_src, double *sorted_dst, double *arrival, const double *norm,
                              double percentile, void *out);

/* The loaders' point-sampling draws, bit for bit (host code, no GPU call): for each of k objects out[o*n .. o*n+n) =
 * np.random.permutation(m[o])[:n] = what np.random.choice(m[o], n, replace=False) returns (YCBV/dataloader_test_YCBV.py:166-169,
 * LM/dataloader_test_LM.py:176-181) -- numpy's legacy Fisher-Yates walk (mtrand.pyx: _shuffle_raw, random_interval: MT19937
 * words masked and rejected) on the CALLER's generator state: key624 = np.random.get_state()[1] (updated in place), *pos_io =
 * [2] (in / out); put them back with np.random.set_state() and the global stream has advanced exactly as under numpy.
 * Requires n <= m[o] < 2^31; scratch = max(m) int32.  ~3x numpy's speed (a tight 32-bit loop instead of 3 memcpy per swap). */
int dcl_legacy_permutation_heads(uint32_t *key624, int32_t *pos_io, const int32_t *m, int k, int n, int64_t *out,
                                 int32_t *scratch);

/* ---------------------------------------------------- per-class template cache ---
 * Deals cached class rows into a call's activation buffers in ONE launch (csrc/template_rows.hip; models/DCL_Net.py:
 * Network.cache_templates keeps, per object class, what the template half of an eval-mode forward leaves behind).
 *   cache   device fp32, C classes of n_tmp rows: element (s, r, k) at cache[s * class_floats + r * row_floats + k].
 *           row_floats is the row PITCH in floats (the network keeps 643 columns [p1 256 | m1 64 | p2 256 | m2 64 | xyz 3] in
 *           rows of 644, so that rows stay 16-byte aligned); class_floats >= n_tmp * row_floats.
 *   lut     device int32 (lut_len): class id -> cache slot, -1 where the class is absent.  A slot must be < C.
 *   cls     device int32 (b): the crops' class ids.  They are read by the kernel only: no read-back on this path.
 *   blocks  host array of nblocks <= DCL_TEMPLATE_MAX_BLOCKS column blocks: for crop i < b, row r < n_tmp and c < width
 *               dst[(i * n_tmp + r) * dst_pitch + c] = cache[lut[cls[i]]][r][src_col + c].
 *           A destination is a column block of a wider row-major buffer (dst_pitch floats per row); columns outside a block
 *           are not touched.  Blocks must not overlap each other.
 *   miss    device int32: a class id outside [0, lut_len) or with lut[id] < 0 is a MISS -- that crop's rows are written as +0
 *           and *miss is set to 1 by an ordinary store (every writer stores the same value); nothing is read out of range.
 *           A call without a miss does not write *miss (the caller zeroes it once).
 * A block whose dst, src_col, width and dst_pitch -- and the cache's base, row_floats and class_floats -- are multiples of 16
 * bytes moves 16 bytes per lane; any other block goes float by float, with the same result.  No atomics, no scratch, no LDS;
 * the grid is sized from b * n_tmp * sum(width); capturable.  DCL_EINVAL before any GPU work for a NULL or misaligned (4-byte)
 * pointer, b, n_tmp or nblocks < 1, nblocks > DCL_TEMPLATE_MAX_BLOCKS, lut_len < 0, row_floats < 1, class_floats < n_tmp *
 * row_floats, and per block src_col < 0, width < 1, dst_pitch < width or src_col + width > row_floats.
 * dcl_template_rows_host is the same contract in plain C++ on HOST pointers (what the tests compare with; no GPU call).      */
#define DCL_TEMPLATE_MAX_BLOCKS 8
typedef struct {
  int32_t src_col, width;
  float *dst;
  int64_t dst_pitch;
} DclTemplateBlock;
int dcl_template_rows(const float *cache, int64_t class_floats, int row_floats, int n_tmp, const int32_t *lut, int lut_len,
                      const int32_t *cls, int b, const DclTemplateBlock *blocks, int nblocks, int32_t *miss, dclStream_t stream);
int dcl_template_rows_host(const float *cache, int64_t class_floats, int row_floats, int n_tmp, const int32_t *lut, int lut_len,
                           const int32_t *cls, int b, const DclTemplateBlock *blocks, int nblocks, int32_t *miss);

/* The ONE measurement facility of the product library (it selects nothing and changes no result; every tuning / A-B switch
 * lives in the diagnostic library below): between _begin and _end every sparse-conv call (runner or op API) is bracketed by
 * HIP events on its launch stream; _end waits for them and returns the summed device milliseconds and the number of calls.
 * bench.py's `roofline_sparse_conv` is measured with it on the product library itself.  Thread-safe (a mutex around the
 * event list); do not use under stream capture.                                                                          */
int dcl_profile_conv_begin(void);
int dcl_profile_conv_end(double *ms_total_host, int32_t *calls_host);
/* The same, plus the calls one by one in call order: ms_per_call_host[i] = device milliseconds of call i and
 * what_per_call_host[4 i ..] = its (Cin, Cout, subm, problems in the launch), for the first `cap` calls (either array may be NULL).
 * bench.py's `roofline_sparse_conv.layers[]` is taken with it. */
int dcl_profile_conv_end_calls(double *ms_total_host, int32_t *calls_host, float *ms_per_call_host, int32_t *what_per_call_host,
                               int32_t cap);

/* ---- DIAGNOSTIC library only (csrc/Makefile `make diag` -> tools/_bin/libdclnet_hip_diag.so, built with -DDCL_DIAG) ----
 * The dcl_debug_* entry points are TEST / TUNING hooks, not part of the operator API and NOT exported by the product library
 * libdclnet_hip.so (where every switch is a compile-time constant and the superseded kernel variants are not compiled):
 * each sets one process-wide atomic switch that later calls from any thread read (A/B kernel variants in tests, tuning
 * sweeps in tools/).  They never change results beyond the tolerance of the op.                                          */
#ifdef DCL_DIAG
/* Test hook, sparse-conv kernel variant: 0 = automatic (LDS-DMA implicit GEMM where Cout % 64 == 0), 1 = plain VALU
 * kernel for every layer (A/B check of the MFMA ones), 2 = MFMA without LDS staging (the general fallback),
 * 4 = register-staged tile kernel instead of the LDS-DMA one, 5 = 4-wave 128x64 tiles for Cout = 64 (the default has 8 waves). */
void dcl_debug_force_valu_conv(int on);
/* Test hook, attention kernel: 0 = automatic, 1 = shared-tile 8-wave variant, 2 = double-buffered 4-wave register
 * staging, 3 / 4 = LDS-DMA pipeline with 8 / 4 waves. */
void dcl_debug_attention_variant(int v);
/* Tuning hook: 0 = automatic key split of small attention launches (dcl_cross_attention_ws), n = force n splits. */
void dcl_debug_attention_split(int n);
/* Tuning hook: 1 (default) = the LDS-DMA attention kernel renumbers its workgroups so that the query blocks of one crop share
 * an XCD (one L2 fetch of the crop's K/V per XCD group), 0 = plain blockIdx order (traffic A/B). */
void dcl_debug_attention_xcd_remap(int on);
/* Test hook, geometry stage: 1 (default) = the 8 occupancy masks of a pass come from one launch (one workgroup per crop walks
 * the conv/pool chain in LDS; 64^3 grids), 0 = 8 chained launches.  Both produce identical masks.  Process-wide atomic. */
int dcl_debug_geometry_chain(int mode);
/* Tuning hook: smallest batch whose deep conv layers get a row order (default 12); a huge value switches the ordering off. */
void dcl_debug_order_min_batch(int n);
/* Tuning hook: first backbone level (0..3) whose conv layers get a row order (default 2: the two deep levels). */
void dcl_debug_order_min_level(int m);
/* Test hook, 3-NN of the point read-out: 1 (default) = grid-pruned search on the 32^3 / 16^3 levels, 0 = per-crop scan on
 * every level, 2 = grid kernel with its scan fallback forced for every query, 3 / 4 / 5 = grid kernel with one / four /
 * eight lanes per query whatever the number of points (automatic: eight up to 40960 points, four up to 131072, else
 * one).  All give identical results. */
void dcl_debug_three_nn_grid(int mode);
/* Test hook, batched three_nn / knn (k = 1): 0 (default) = bucketed exact search, 1 = the plain scan (A/B). */
void dcl_debug_nn_batched_mode(int mode);
/* Tuning hook: queries per thread of the bucketed batched search (1..4; 0 = automatic). */
void dcl_debug_nn_qpt(int q);
/* Diagnostic: (query, point) distance evaluations the bucketed three_nn / knn searches have executed since the last reset
 * (synchronises the device; reset != 0 zeroes the counter) -- what bench.py prices those kernels against. */
unsigned long long dcl_debug_nn_tests_executed(int reset);
/* Tuning hook: 0 = automatic split-K choice in dcl_sparse_conv_fwd_ws, n = force n splits (when the scratch allows),
 * -1 = at most 8 splits even for few-row launches, -2 = never split. */
void dcl_debug_conv_split(int n);
/* Tuning hook: least number of chunks a workgroup of a few-row conv launch walks (default 4). */
void dcl_debug_conv_few_chunks(int n);
/* Tuning hook: 1 (default) = few-row conv launches use 64-row tiles, 0 = 128-row tiles for every launch. */
void dcl_debug_conv_few_tiles(int on);
/* Tuning hook: 1 (default) = the Cin 16 / 32 -> 32 conv layers of many rows run the filter-resident kernel, 0 = LDS-DMA kernel. */
void dcl_debug_conv_wlds(int on);
/* Tuning hooks of the own GEMM core: tile shape (0 = automatic, 1 = 128x128, 2 = 128x64, 3 = 64x64, 4 / 5 = 64x64 with
 * the two halves / four quarters of K on two / four wave groups), XCD-aware
 * workgroup renumbering (default 1). */
void dcl_debug_linear_tile(int t);
void dcl_debug_linear_xcd_remap(int on);
void dcl_debug_linear_persist(int rounds);   /* rounds of resident workgroups from which a GEMM launch is persistent (default: never) */
/* Diagnostic: times the GEMM library's first ncand heuristic candidates (32 MiB of workspace on offer) for an (M, N, K)
 * linear layer, each alone on the GPU; ms_out[i] = mean ms, ws_out[i] (may be NULL) = the workspace candidate i asks for.
 * dcl_linear_fwd itself only ever takes an algorithm that asks for none (it queries with a maximum of 0 bytes and refuses
 * the call when nothing is left), so candidates with ws_out[i] > 0 are the ones it can never run. */
int dcl_debug_linear_candidates(int M, int N, int K, int ncand, float *ms_out, long long *ws_out, int *found_out);
/* Diagnostic: bytes of workspace the algorithm dcl_linear_fwd takes for (M, N, K) asks for: 0, or -1 = the library has no
 * zero-workspace algorithm for the shape (dcl_linear_fwd returns DCL_EINVAL then -- never a workspace-exchanging kernel). */
long long dcl_debug_linear_plan_workspace(int M, int N, int K);
/* Tuning hook: 1 (default) = a pair of attention launches (dcl_cross_attention_ws2, concurrent = 2) that makes whole rounds of
 * 8-wave workgroups plus a rest is issued as two launches (rounds, rest); 0 = one launch. */
void dcl_debug_attention_pair_split(int on);
/* Tuning hook: 0 = large attention calls keep the fp32-MFMA kernel even when `planes` are handed in (dcl_cross_attention_ws3);
 * dcl_cross_attention_planes_bytes then returns 0.  1 (default) = P.V on the bf16 matrix pipe (k_cross_attn_split). */
void dcl_debug_attention_bf16(int on);
/* Diagnostic: 0 = plain tile numbering in k_linear_split (1 = XCD-aware, default); what-if runs of k_linear_split (WRONG results;
 * timing only) -- bit 0: no LDS-DMA after a tile's first chunk, bit 1: no operand split, bit 2: no store epilogue. */
void dcl_debug_linear_split_xcd_remap(int on);
void dcl_debug_linear_split_whatif(int bits);
/* Diagnostic: what-if runs of k_cross_attn_split (WRONG results; timing only) -- bit 0: no P.V phase, bit 1: no S / softmax phase,
 * bit 2: no LDS-DMA after the first tile. */
void dcl_debug_attention_whatif(int bits);
/* Tuning hook: most crops of a pass whose geometry stage runs as one launch (k_geometry_small; default 16, at most 64;
 * passes of more than 8 crops also need at most 32768 voxel rows). */
void dcl_debug_geometry_small_batch(int n);
int dcl_debug_geometry_small_stamps(unsigned long long *host32);   /* s_memrealtime (100 MHz) at the phase boundaries of workgroup 0 of the last k_geometry_small (0..9), after each mask-chain stage (16..23) */
/* Diagnostic: a one-thread launch that writes the 100 MHz wall clock into *slot_dev (a time stamp inside a stream or a
 * captured graph: tools/graph_timeline.py). */
int dcl_debug_stamp(unsigned long long *slot_dev, dclStream_t stream);
/* Tuning hook: row CAPACITY up to which a capacity-mode conv launch (whole-forward graph) counts as a few-row launch. */
void dcl_debug_conv_few_cap(int rows);
/* Tuning hook: EXPECTED rows (the backbone runner's hint) up to which a capacity-mode conv launch counts as few-row. */
void dcl_debug_conv_few_hint(int rows);
/* Tuning hook: number of workgroups the stream-K / split-K decompositions of a sparse-conv launch are dealt over (default
 * 512 = the 2 x 256 resident slots; 256 leaves one slot per CU to a concurrent launch of the other backbone).  64..512. */
void dcl_debug_conv_slots(int n);
/* Test hook, row order of the LDS-DMA conv launches (dcl_sparse_conv_fwd_ordered, the backbone runner): 0 = as given,
 * 1 = ignore the order (natural rows, nominal units), 2 = keep the order but deal nominal chunk units. */
void dcl_debug_conv_order_mode(int mode);
/* Diagnostic: s_memrealtime stamps (100 MHz) of the phases of the last row-order launch's first workgroup. */
int dcl_debug_order_stamps(unsigned long long *host16);
/* Tuning hook: 1 (default) = the LDS-DMA conv kernel renumbers its workgroups XCD-aware (column tiles of a row tile and
 * neighbouring row tiles share an L2), 0 = plain blockIdx order. */
void dcl_debug_conv_xcd_remap(int on);
/* Tuning hook: output rows per tile of dcl_sparse_conv_fwd_compact, 64 or 128; 0 (default) = by the layer's width. */
void dcl_debug_conv_fwd_compact_bm(int bm);
/* Test hook, dcl_crop_draw's route to its (route-independent) result: 0 (default) = guessed threshold, widened or replaced by
 * the radix select as needed; 1 = radix select from the start; 2 = a first guess 256 times too small (the widening loop);
 * 3 = a first guess of 2^64 - 1 (the list overflows where m > 8192: the radix select behind a failed guess). */
void dcl_debug_crop_draw_route(int route);
/* Tuning hook for dcl_group_points' LDS-staged kernel: channel rows per workgroup, x-blocks, threads per workgroup,
 * store kind (2 = plain instead of nontemporal); 0 = built-in choice for each. */
void dcl_debug_group_points_cfg(int cc, int xb, int threads, int nontemporal);
/* Launch census: every kernel launch of the diagnostic library is counted by kernel (demangled name incl. template arguments).
 * _census writes "name<TAB>launches<NEWLINE>" lines into buf (NUL-terminated, cut at cap) and returns the bytes the whole text
 * needs; _reset empties the table.  tests/test_kernel_census.py: every kernel a committed profile names must have been
 * launched by a test that compares with the oracle. */
void dcl_debug_launch_census_reset(void);
long long dcl_debug_launch_census(char *buf, long long cap);
#endif /* DCL_DIAG */

#ifdef __cplusplus
}
#endif
#endif /* DCLNET_HIP_H_ */
