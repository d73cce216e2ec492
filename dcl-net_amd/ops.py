"""Thin torch-tensor front end of the C ABI (include/dclnet_hip.h).

Every function takes/returns CUDA tensors (PyTorch is the allocator and stream provider), checks
arguments the way the reference's Python wrappers do (contiguity, dtypes) and calls the HIP
library on torch's current stream.  No function here has a CPU fallback.

One calling convention: scalars go in as plain Python ints / floats (_native declares every entry point's signature from the
header, so nothing is wrapped by hand here), pointers as N.ptr(tensor) / ctypes arrays / None; a size asked through an
out-parameter is N.query(...), and a kernel with a host twin is N.twin(...) on one argument list.
"""
import ctypes as C
import threading

import weakref

import torch

from . import _native as N

# bench.py sets this to a list to collect (name, start_event, end_event) around selected launches on torch's
# current stream (the stream the kernels are launched on); None = off.
PROFILE_EVENTS = None


def _i32_ptr_or_null(t):
    return N.ptr(t) if t is not None else N.vp(0)


# ------------------------------------------------------------------------------------ PG_OP
def voxelize_idx(coords, batch_size, mode=4):
    """PG_OP.voxelize_idx (libs/pointgroup_ops/functions/pointgroup_ops.py:11-39): HOST op.
    coords long (N, 3|4) CPU -> (output_coords long (M,ncol), input_map int (N), output_map int (M,1+maxActive))."""
    if coords.is_cuda:
        raise RuntimeError("voxelize_idx is a host (DataLoader-side) op: pass a CPU tensor")
    assert coords.is_contiguous() and coords.dtype == torch.int64 and coords.dim() == 2
    n, ncol = coords.shape
    input_map = torch.zeros(n, dtype=torch.int32)
    na, ma = N.query("dcl_voxelize_idx_count", N.ptr(coords), n, ncol, int(batch_size), int(mode), N.ptr(input_map),
                     ctype=(C.c_int32, C.c_int32))
    out_coords = torch.zeros((na, ncol), dtype=torch.int64)
    out_map = torch.zeros((na, ma + 1), dtype=torch.int32)
    N.check(N.lib().dcl_voxelize_idx_fill_mode(N.ptr(coords), n, ncol, N.ptr(input_map), na, ma, int(mode),
                                               N.ptr(out_coords), N.ptr(out_map)), "voxelize_idx_fill")
    return out_coords, input_map, out_map


def voxelize_idx_gpu(coords, batch_size, S=64, mode=4):
    """Device version of voxelize_idx for coords (N,4) int64 CUDA inside a batch x S^3 grid: identical outputs
    (first-encounter voxel ids, ascending point lists), one host read-back of {V, maxActive}."""
    N.need_cuda(coords)
    assert coords.is_contiguous() and coords.dtype == torch.int64 and coords.shape[1] == 4
    n, dev = coords.shape[0], coords.device
    nbytes = N.query("dcl_voxelize_idx_gpu_ws_bytes", n, int(batch_size), int(S))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    input_map = torch.empty(max(n, 1), dtype=torch.int32, device=dev)[:n]
    info = torch.empty(3, dtype=torch.int32, device=dev)
    N.check(N.lib().dcl_voxelize_idx_gpu_count(N.ptr(coords), n, int(batch_size), int(S), int(mode), N.ptr(ws), nbytes,
                                               N.ptr(input_map), N.ptr(info), N.stream()), "voxelize_idx_gpu_count")
    V, ma, err = info.cpu().tolist()
    if err:
        raise RuntimeError("voxelize_idx_gpu: a coordinate lies outside the batch x S^3 grid")
    ma = max(ma, 1)
    out_coords = torch.empty((V, 4), dtype=torch.int64, device=dev)
    out_map = torch.empty((V, ma + 1), dtype=torch.int32, device=dev)
    N.check(N.lib().dcl_voxelize_idx_gpu_fill(N.ptr(coords), n, int(batch_size), int(S), N.ptr(ws), N.ptr(input_map), V, ma,
                                              N.ptr(out_coords), N.ptr(out_map), N.stream()), "voxelize_idx_gpu_fill")
    return out_coords, input_map, out_map


VI_CROPS_MAX_BATCH, VI_CROPS_MAX_POINTS, VI_CROPS_S = 64, 1024, 64
_VI_COMM = {}
_VI_LOCK = threading.Lock()


def voxelize_idx_crops(coords, batch_size, n_per, S=64, mode=4, pitch=33, occ_dtype=torch.int64):
    """voxelize_idx for the crop builder's layout -- batch_size crops of exactly n_per <= 1024 points each (rows c*n_per .. of
    `coords` (b*n_per, 4) int64 belong to crop c), 64^3 grids, at most 64 crops -- in ONE launch and WITHOUT a host read-back
    (csrc/voxelize_idx.hip: k_vi_crops).  Returns CAPACITY-shaped tensors: occ (b*n_per, 4) of occ_dtype, input_map (b*n_per),
    v2p (b*n_per, pitch) and info = device int32 {V, maxActive, error}: the first V rows of occ / v2p are live and equal
    voxelize_idx_gpu's rows bit for bit (v2p[:V, :maxActive+1]); error = a point outside its grid or a voxel with more than
    pitch-1 points."""
    N.need_cuda(coords)
    b, n_per = int(batch_size), int(n_per)
    assert coords.is_contiguous() and coords.dtype == torch.int64 and tuple(coords.shape) == (b * n_per, 4)
    assert 1 <= b <= VI_CROPS_MAX_BATCH and 1 <= n_per <= VI_CROPS_MAX_POINTS and int(S) == VI_CROPS_S
    dev = coords.device
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    with _VI_LOCK:         # (the builder thread of a CropPrefetcher and the caller's thread may both arrive here first)
        ent = _VI_COMM.get(key)
        if ent is None:    # a ring of 64 regions of 2 ints per crop that persist between calls + the call counter: consecutive calls
            ent = _VI_COMM[key] = [torch.zeros(64 * 2 * VI_CROPS_MAX_BATCH, dtype=torch.int32, device=dev), 0]   # (also on other streams / threads) use different words
        ent[1] = ent[1] % 0x3fffffff + 1
        gen = ent[1]
    comm = ent[0][(gen % 64) * 2 * VI_CROPS_MAX_BATCH:]
    occ = torch.empty((b * n_per, 4), dtype=occ_dtype, device=dev)
    input_map = torch.empty(b * n_per, dtype=torch.int32, device=dev)
    v2p = torch.empty((b * n_per, int(pitch)), dtype=torch.int32, device=dev)
    info = torch.empty(3, dtype=torch.int32, device=dev)
    assert occ_dtype in (torch.int64, torch.int32)
    N.check(N.lib().dcl_voxelize_idx_crops(N.ptr(coords), b, n_per, int(S), int(mode), int(pitch), N.ptr(comm), gen,
                                           N.ptr(input_map), N.ptr(occ), int(occ_dtype == torch.int32), N.ptr(v2p), N.ptr(info),
                                           N.stream()), "voxelize_idx_crops")
    return occ, input_map, v2p, info


def voxelize_fp(feats, map_rule, mode=4):
    """PG_OP.voxelize_fp (pointgroup_ops.py:42-62): feats (N,C) f32, map_rule (M,1+maxActive) i32 -> (M,C)."""
    N.need_cuda(feats, map_rule)
    assert feats.is_contiguous() and map_rule.is_contiguous()
    assert feats.dtype == torch.float32 and map_rule.dtype == torch.int32
    M, ma = map_rule.shape[0], map_rule.shape[1] - 1
    out = torch.empty((M, feats.shape[1]), dtype=torch.float32, device=feats.device)
    N.check(N.lib().dcl_voxelize_fp(N.ptr(feats), N.ptr(map_rule), N.ptr(out), M, ma, feats.shape[1],
                                    int(mode == 4), N.stream()), "voxelize_fp")
    return out


class _PadCopyJob(C.Structure):
    _fields_ = [("dst", C.c_void_p), ("src", C.c_void_p), ("rows_dst", C.c_int32), ("cols_dst", C.c_int32),
                ("rows_src", C.c_int32), ("cols_src", C.c_int32), ("src_pitch", C.c_int32), ("src_is_i64", C.c_int32),
                ("fill_value", C.c_int32), ("dst_pitch", C.c_int32)]


def pad_copy_many(jobs):
    """jobs: list of (dst, src) 2-D CUDA tensor pairs of 4-byte elements (src may be int64 -> narrowed; may be smaller than
    dst -> zero padded; may be a column block of a wider row-major tensor) or (dst, int) fills -- ONE launch for all."""
    arr = (_PadCopyJob * len(jobs))()
    for j, (dst, src) in enumerate(jobs):
        assert dst.is_cuda and dst.element_size() == 4
        pitch = 0
        if dst.dim() == 2 and not dst.is_contiguous():                 # a column block of a wider row-major buffer
            assert dst.stride(1) == 1 and dst.stride(0) >= dst.shape[1]
            d2, pitch = dst, dst.stride(0)
        elif dst.dim() == 2:
            d2 = dst
        elif torch.is_tensor(src):
            d2 = dst.reshape(-1, src.shape[1])         # same logical rows as the source
        else:
            d2 = dst.reshape(1, -1)
        q = arr[j]
        assert pitch or dst.is_contiguous()
        q.dst, q.rows_dst, q.cols_dst, q.dst_pitch = dst.data_ptr(), d2.shape[0], d2.shape[1], pitch
        if torch.is_tensor(src):
            # (a one-column source has no column stride of its own: torch keeps whatever stride the view it came from had --
            # the class id of a ONE-crop frame is such a view)
            assert src.is_cuda and src.dim() == 2 and (src.stride(1) == 1 or src.shape[1] == 1) and src.element_size() in (4, 8)
            assert src.element_size() == 4 or src.dtype == torch.int64
            q.src, q.rows_src, q.cols_src = src.data_ptr(), src.shape[0], src.shape[1]
            q.src_pitch = _pitch(src)
            q.src_is_i64 = int(src.dtype == torch.int64)
        else:
            q.src, q.fill_value = None, int(src)
    N.check(N.lib().dcl_pad_copy_many(arr, len(jobs), N.stream()), "pad_copy_many")


# ------------------------------------------------------------------------------------ per-class template cache
TEMPLATE_MAX_BLOCKS = N.define("DCL_TEMPLATE_MAX_BLOCKS")


class _TemplateBlock(C.Structure):
    _fields_ = [("src_col", C.c_int32), ("width", C.c_int32), ("dst", C.c_void_p), ("dst_pitch", C.c_int64)]


def _template_rows(cache, lut, cls, blocks, miss, host):
    what = "template_rows_host" if host else "template_rows"
    dev = cache.device
    if host:
        if cache.is_cuda:
            raise RuntimeError("%s is the host twin: pass CPU tensors" % what)
    else:
        N.need_cuda(cache)
    if not (cache.dim() == 3 and cache.dtype == torch.float32 and cache.stride(2) == 1 and cache.shape[0] >= 1):
        raise ValueError("%s: cache must be float32 (C, n_tmp, columns) with unit column stride" % what)
    n_tmp, cols = int(cache.shape[1]), int(cache.shape[2])
    row_floats = int(cache.stride(1)) if n_tmp > 1 else cols
    class_floats = int(cache.stride(0)) if cache.shape[0] > 1 else n_tmp * row_floats
    if not (lut.dim() == 1 and lut.dtype == torch.int32 and lut.is_contiguous() and lut.device == dev):
        raise ValueError("%s: lut must be a contiguous int32 vector on the cache's device" % what)
    if not torch.is_tensor(cls):
        cls = torch.as_tensor(cls, dtype=torch.int64)
    if cls.dim() != 1 or cls.dtype not in (torch.int32, torch.int64) or cls.numel() < 1:
        raise ValueError("%s: cls must be a non-empty (b,) vector of int32 or int64 class ids" % what)
    # (ids the caller keeps on the host, or as int64, are narrowed and uploaded here; device int32 ids are taken as they are)
    cls = cls.to(device=dev, dtype=torch.int32).contiguous()
    b = int(cls.numel())
    if miss is None:
        miss = torch.zeros(1, dtype=torch.int32, device=dev)
    if not (miss.dtype == torch.int32 and miss.numel() == 1 and miss.device == dev):
        raise ValueError("%s: miss must be a 1-element int32 tensor on the cache's device" % what)
    if not 1 <= len(blocks) <= TEMPLATE_MAX_BLOCKS:
        raise ValueError("%s: 1 .. %d column blocks" % (what, TEMPLATE_MAX_BLOCKS))
    arr = (_TemplateBlock * len(blocks))()
    for j, (src_col, dst) in enumerate(blocks):
        if not (torch.is_tensor(dst) and dst.dim() == 2 and dst.dtype == torch.float32 and dst.device == dev and
                dst.shape[0] == b * n_tmp and (dst.stride(1) == 1 or dst.shape[1] == 1)):
            raise ValueError("%s: block %d: dst must be float32 (b * n_tmp, width) rows with unit column stride on the cache's "
                             "device" % (what, j))
        width = int(dst.shape[1])
        if int(src_col) < 0 or int(src_col) + width > cols:
            raise ValueError("%s: block %d: columns %d .. %d lie outside the cache's %d" % (what, j, src_col, src_col + width, cols))
        q = arr[j]
        q.src_col, q.width, q.dst = int(src_col), width, dst.data_ptr()
        q.dst_pitch = int(dst.stride(0)) if dst.shape[0] > 1 else width
    N.twin("dcl_template_rows", host, what, N.ptr(cache), class_floats, row_floats, n_tmp, N.ptr(lut), int(lut.numel()), N.ptr(cls),
           b, arr, len(blocks), N.ptr(miss))
    return miss


def template_rows(cache, lut, cls, blocks, miss=None):
    """Deal cached class rows into a call's activation buffers, ONE launch (csrc/template_rows.hip; contract in
    include/dclnet_hip.h at dcl_template_rows).  cache (C, n_tmp, columns) float32 CUDA, possibly a view with padded row / class
    pitches; lut (lut_len,) int32 CUDA, class id -> cache slot or -1; cls (b,) class ids -- an int32 CUDA tensor is taken as it
    is (nothing is read back), an int64 or host tensor or a list is narrowed and uploaded; blocks = [(src_col, dst), ...] with
    dst a (b * n_tmp, width) float32 CUDA tensor, possibly a column block of a wider row-major buffer: dst[i * n_tmp + r, c] =
    cache[lut[cls[i]], r, src_col + c].  Blocks must not overlap.  miss: a 1-element int32 CUDA tensor that is set to 1 when an
    id is outside the table or not cached (that crop's rows are zeros); None makes a zeroed one.  Returns miss."""
    return _template_rows(cache, lut, cls, blocks, miss, False)


def template_rows_host(cache, lut, cls, blocks, miss=None):
    """template_rows on CPU tensors: the same contract in plain C++ (dcl_template_rows_host; what the tests compare with)"""
    return _template_rows(cache, lut, cls, blocks, miss, True)


# ------------------------------------------------------------------------------------ rulebooks
def grid_words(batch, S):
    return (batch * S * S * S + 31) // 32


def scan_scratch(nwords, device):
    return torch.empty(((nwords + 1023) // 1024) + 1, dtype=torch.int32, device=device)


class ActiveSet(object):
    """Device-side description of an active voxel set (see include/dclnet_hip.h, spconv section)."""
    __slots__ = ("indices", "n", "n_dev", "cap", "mask", "wprefix", "perm", "S", "batch")

    def __init__(self, indices, n, n_dev, cap, mask, wprefix, perm, S, batch):
        self.indices, self.n, self.n_dev, self.cap = indices, n, n_dev, cap
        self.mask, self.wprefix, self.perm, self.S, self.batch = mask, wprefix, perm, S, batch

    def segments(self):
        """i32[batch+1]: rows of crop b are [seg[b], seg[b+1]) (rows are in ascending linear index
        unless perm is set)."""
        wpc = (self.S ** 3) // 32
        assert wpc * 32 == self.S ** 3 and self.perm is None
        return self.wprefix[::wpc].contiguous()


def grid_from_indices(indices, batch, S):
    """ActiveSet of an explicit voxel list (rows in any order)."""
    N.need_cuda(indices)
    assert indices.dtype == torch.int32 and indices.is_contiguous() and indices.shape[1] == 4
    V = indices.shape[0]
    dev = indices.device
    nw = grid_words(batch, S)
    mask = torch.empty(nw, dtype=torch.int32, device=dev)
    wprefix = torch.empty(nw + 1, dtype=torch.int32, device=dev)
    perm = torch.empty(max(V, 1), dtype=torch.int32, device=dev)
    N.check(N.lib().dcl_grid_from_indices(N.ptr(indices), V, batch, S, N.ptr(mask), N.ptr(wprefix), N.ptr(perm),
                                          N.ptr(scan_scratch(nw, dev)), N.stream()), "grid_from_indices")
    return ActiveSet(indices, V, None, V, mask, wprefix, perm, S, batch)


def conv_out_size(S, k, s, p):
    return (S + 2 * p - (k - 1) - 1) // s + 1


def conv_out_grid(inp, ksize, stride, padding, cap=None):
    """Output active set of a non-submanifold conv/pool over `inp` (count stays on the device)."""
    S_out = conv_out_size(inp.S, ksize, stride, padding)
    dev = inp.indices.device
    bound = inp.batch * S_out ** 3
    if cap is None:
        cap = min(inp.cap * ksize ** 3, bound)
    cap = max(int(cap), 1)
    nw = grid_words(inp.batch, S_out)
    mask = torch.empty(nw, dtype=torch.int32, device=dev)
    wprefix = torch.empty(nw + 1, dtype=torch.int32, device=dev)
    out_idx = torch.empty((cap, 4), dtype=torch.int32, device=dev)
    n_in_dev = inp.n_dev if inp.n is None else None
    n_in_host = inp.cap if inp.n is None else inp.n
    N.check(N.lib().dcl_conv_out_grid(N.ptr(inp.indices), _i32_ptr_or_null(n_in_dev), int(n_in_host),
                                      N.ptr(inp.mask), inp.batch, inp.S, ksize, stride, padding, N.ptr(mask), N.ptr(wprefix), N.ptr(out_idx),
                                      N.ptr(wprefix[nw:]), cap, N.ptr(scan_scratch(nw, dev)), N.stream()),
            "conv_out_grid")
    return ActiveSet(out_idx, None, wprefix[nw:], cap, mask, wprefix, None, S_out, inp.batch)


def rulebook_gather(out, inp, ksize, stride, padding):
    """Gather-form rulebook nbr i32 (kvol, rows(out)) of `out` rows against the `inp` set."""
    dev = out.indices.device
    rows = out.cap if out.n is None else out.n
    rows_alloc = max(rows, 1)
    nbr = torch.empty((ksize ** 3, rows_alloc), dtype=torch.int32, device=dev)
    n_dev = out.n_dev if out.n is None else None
    N.check(N.lib().dcl_rulebook_gather(N.ptr(out.indices), _i32_ptr_or_null(n_dev), int(rows if out.n is not None else 0),
                                        N.ptr(inp.mask), N.ptr(inp.wprefix), _i32_ptr_or_null(inp.perm), inp.batch,
                                        inp.S, ksize, stride, padding, N.ptr(nbr), rows_alloc, N.stream()),
            "rulebook_gather")
    return nbr


def rulebook_to_pairs(nbr, n_out, n_in):
    """Reference-format rulebook: indice_pairs i32 (kvol,2,n_in) (-1 padded), indice_num i32 (kvol)."""
    kvol, cap = nbr.shape
    pairs = torch.empty((kvol, 2, max(n_in, 1)), dtype=torch.int32, device=nbr.device)
    num = torch.empty(kvol, dtype=torch.int32, device=nbr.device)
    N.check(N.lib().dcl_rulebook_to_pairs(N.ptr(nbr), cap, N.vp(0), int(n_out), kvol, N.ptr(pairs), int(n_in),
                                          N.ptr(num), N.stream()), "rulebook_to_pairs")
    return pairs[:, :, :n_in], num


def rulebook_from_pairs(indice_pairs, indice_num, n_in, n_out, check=False):
    """Reference-format rulebook (indice_pairs i32 (kvol,2,V) -1 padded, indice_num i32 (kvol)) -> gather table
    nbr i32 (kvol, max(n_out,1)).  indice_num may live on the host (it does in the reference after spconv_ops.h:264) or
    on the device; it is used from the device, without a read-back.  check=True reads back the count of pairs that
    pointed outside the row ranges and raises if there were any."""
    N.need_cuda(indice_pairs)
    assert indice_pairs.dtype == torch.int32 and indice_pairs.dim() == 3 and indice_pairs.shape[1] == 2
    pairs = indice_pairs.contiguous()
    kvol, _, stride = pairs.shape
    num = indice_num.to(device=pairs.device, dtype=torch.int32, non_blocking=True).contiguous()
    assert num.numel() == kvol
    cap = max(int(n_out), 1)
    nbr = torch.empty((kvol, cap), dtype=torch.int32, device=pairs.device)
    bad = torch.empty(1, dtype=torch.int32, device=pairs.device) if check else None
    N.check(N.lib().dcl_rulebook_from_pairs(N.ptr(pairs), int(stride), N.ptr(num), kvol, int(n_in), int(n_out), N.ptr(nbr),
                                            cap, N.ptr(bad), N.stream()), "rulebook_from_pairs")
    if check and int(bad.item()):
        raise ValueError("rulebook_from_pairs: %d pairs point outside the feature / output rows" % int(bad.item()))
    return nbr


def indice_summary_rf(indice_pairs, indice_num, n_out):
    """torch.ops.spconv.indiceSummaryRF: receptive-field count i32 (n_out) from the pair format."""
    N.need_cuda(indice_pairs)
    pairs = indice_pairs.contiguous()
    kvol, _, stride = pairs.shape
    num = indice_num.to(device=pairs.device, dtype=torch.int32, non_blocking=True).contiguous()
    rf = torch.empty(int(n_out), dtype=torch.int32, device=pairs.device)
    N.check(N.lib().dcl_indice_summary_rf(N.ptr(pairs), int(stride), N.ptr(num), kvol, int(n_out), N.ptr(rf), N.stream()),
            "indice_summary_rf")
    return rf


def sparse_avgpool_rf(feat, nbr, n_out, summaryrf):
    """indice_avgpool_fp32 with the caller's divisor tensor (use_gs=True passes the kernel volume)."""
    N.need_cuda(feat, nbr, summaryrf)
    kvol, cap = nbr.shape
    c = feat.shape[1]
    out = torch.empty((n_out, c), dtype=torch.float32, device=feat.device)
    if n_out:
        rf = N.i32c(summaryrf)
        assert rf.numel() >= n_out
        N.check(N.lib().dcl_sparse_avgpool_fwd_rf(N.ptr(feat.contiguous()), N.ptr(nbr), cap, N.vp(0), int(n_out), c, kvol,
                                                  N.ptr(rf), N.ptr(out), N.stream()), "sparse_avgpool_fwd_rf")
    return out


def order_rows(out_set, in_mask, subm):
    """Row order of a k3 / s1 / p1 conv layer with output set `out_set` (ActiveSet) and the INPUT set's occupancy bits
    `in_mask` on the same batch x S^3 grid (csrc/row_order.hip) -> (order (n,) i32, bal (ntiles+1,) i32, smask (ntiles,) i32)
    for sparse_conv(..., order=...): tile slot i of the launch computes output row order[i]."""
    N.need_cuda(out_set.indices, in_mask)
    n, dev = int(out_set.n), out_set.indices.device
    cap = max(n, 1)
    tiles = (cap + 127) // 128
    nbytes = N.query("dcl_order_rows_ws_bytes", cap)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    order = torch.empty(cap, dtype=torch.int32, device=dev)
    bal = torch.zeros(tiles + 2, dtype=torch.int32, device=dev)
    smask = torch.zeros(tiles + 1, dtype=torch.int32, device=dev)
    N.check(N.lib().dcl_order_rows(N.ptr(out_set.indices), N.vp(0), n, cap, N.ptr(in_mask), int(out_set.S), int(bool(subm)),
                                   N.ptr(ws), nbytes, N.ptr(order), N.ptr(bal), N.ptr(smask), N.stream()), "order_rows")
    nt = (n + 127) // 128
    return order[:n], bal[:nt + 1], smask[:nt]


def sparse_conv(feat, nbr, n_out, W, subm, scale=None, shift=None, relu=False, order=None, form="tiles"):
    """indice_conv_fp32 (+ folded BatchNorm1d(eval) + ReLU).  feat (V_in,Cin); W (kvol,Cin,Cout).  order: the triple of
    order_rows -- the launch then computes its rows in that order and deals its work in used chunks (same output).  form: "tiles"
    (default: the dispatcher of csrc/sparse_conv.hip, whose tiles run every offset any of their rows has) or "compact"
    (sparse_conv_compact: csrc/conv_fwd_compact.hip, the present (row, offset) pairs only, in a pinned order; it has no
    epilogue and no row order -- ValueError if scale, shift, relu or order is given)."""
    if check_conv_fwd(form, "form") == "compact":
        if scale is not None or shift is not None or relu or order is not None:
            raise ValueError('sparse_conv(form="compact") has no scale / shift / relu epilogue and takes no row order')
        return sparse_conv_compact(feat, nbr, n_out, W, subm)
    N.need_cuda(feat, nbr, W)
    kvol, cap = nbr.shape
    cin, cout = W.shape[-2], W.shape[-1]
    assert feat.is_contiguous() and W.is_contiguous() and feat.shape[1] == cin
    out = torch.empty((n_out, cout), dtype=torch.float32, device=feat.device)
    if n_out == 0:
        return out
    # stream-K scratch (partial-tile slots + tile tickets, csrc/sparse_conv.hip::launch_conv_dma)
    scratch = None
    if cout % 32 == 0:
        scratch = torch.empty(N.query("dcl_sparse_conv_scratch_floats", int(cap), int(cout)), dtype=torch.float32, device=feat.device)
    if order is not None:
        o, bal, smask = order
        assert o.numel() >= n_out and o.dtype == torch.int32 and o.is_cuda
        N.check(N.lib().dcl_sparse_conv_fwd_ordered(N.ptr(feat), N.ptr(nbr), cap, N.vp(0), int(n_out), N.ptr(W), cin, cout, kvol,
                                                    int(bool(subm)), N.ptr(scale), N.ptr(shift), int(bool(relu)), N.ptr(out),
                                                    N.ptr(scratch), 0 if scratch is None else scratch.numel(),
                                                    N.ptr(o), N.ptr(bal), N.ptr(smask), N.stream()), "sparse_conv_fwd_ordered")
        return out
    N.check(N.lib().dcl_sparse_conv_fwd_ws(N.ptr(feat), N.ptr(nbr), cap, N.vp(0), int(n_out), N.ptr(W), cin, cout, kvol,
                                           int(bool(subm)), N.ptr(scale), N.ptr(shift), int(bool(relu)), N.ptr(out),
                                           N.ptr(scratch), 0 if scratch is None else scratch.numel(),
                                           N.stream()), "sparse_conv_fwd")
    return out


def sparse_avgpool(feat, nbr, n_out, want_rf=False):
    """indiceSummaryRF + indice_avgpool_fp32 (use_gs=False)."""
    N.need_cuda(feat, nbr)
    kvol, cap = nbr.shape
    c = feat.shape[1]
    out = torch.empty((n_out, c), dtype=torch.float32, device=feat.device)
    rf = torch.empty(max(n_out, 1), dtype=torch.int32, device=feat.device) if want_rf else None
    if n_out:
        N.check(N.lib().dcl_sparse_avgpool_fwd(N.ptr(feat), N.ptr(nbr), cap, N.vp(0), int(n_out), c, kvol, N.ptr(out),
                                               N.ptr(rf), N.stream()), "sparse_avgpool_fwd")
    return (out, rf[:n_out]) if want_rf else out


# ------------------------------------------------------------------------------------ native backbone runner
BACKBONE_CHANNELS = (7, 16, 32, 32, 64, 64, 128, 128, 256)


def _ptr_array(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


# ---- split-bf16 form of the LDS-DMA conv kernel (csrc/conv_body.h, SPLIT): the chunk's product as six exact bf16 piece products on
# the bf16 matrix pipe, the filter as three bf16 planes prepared once per layer.  Which launches take it is decided HERE, by shape
# and never by data: a layer (cin, cout, subm) of the table, from its minimum EXPECTED row count on -- crops x the per-crop mean
# of the layer's level (the runner's own expect_rows), the same number launch by launch and under graph capture, so both run the
# same form.  Filled from profiles/conv_split.txt: a width is listed only where every split timing was below every fp32 timing.
CONV_SPLIT = True                                      # False: the fp32-MFMA kernels everywhere (same-job A/B, like GEMM_SPLIT)
# (cin, cout, subm) -> minimum expected rows of the launch.  Measured at 32 crops (both shapes, every split timing below every fp32
# timing: 200 -> 150, 127 -> 110, 260 -> 203, 163 -> 132, 376 -> 278 us); smaller batches were not measured and keep the fp32 kernels,
# so each threshold is the layer's expected rows at 32 crops.
CONV_SPLIT_WIDTHS = {(32, 64, True): 57600, (64, 64, False): 28800, (64, 128, True): 28800,
                     (128, 128, False): 14400, (128, 256, True): 14400}
CONV_SPLIT_ROWS_PER_CROP = (3600, 1800, 900, 450)      # csrc/backbone.hip: expect_rows


def conv_split_ok(kvol, cin, cout):
    """the widths the split kernel is built for (one 128 x 64 tile shape on 32-channel chunks)"""
    return int(kvol) == 27 and int(cin) in (32, 64, 128) and int(cout) % 64 == 0


def conv_split_weight(W):
    """W (27, cin, cout) fp32 -> uint8 tensor of three bf16 planes h + m + l == W exactly, in the split kernel's chunk / tile order:
    [k][cin / 32][cout / 64][plane][k step][lane half][64 columns][8 channels] (csrc/sparse_conv.hip: dcl_conv_split_weight)"""
    N.need_cuda(W)
    kvol, cin, cout = W.shape
    assert W.is_contiguous() and W.dtype == torch.float32 and conv_split_ok(kvol, cin, cout)
    lib = N.lib()
    nbytes = int(lib.dcl_conv_split_weight_bytes(int(kvol), int(cin), int(cout)))
    planes = torch.empty(nbytes, dtype=torch.uint8, device=W.device)
    N.check(lib.dcl_conv_split_weight(N.ptr(W), int(kvol), int(cin), int(cout), N.ptr(planes), N.stream()), "conv_split_weight")
    return planes


def conv_split_planes(planes, cin, cout):
    """the three planes of conv_split_weight back in filter order: (3, 27, cin, cout) float32 (tests)"""
    v = planes.view(torch.bfloat16).view(27, cin // 32, cout // 64, 3, 2, 2, 64, 8).float()
    # [k][chunk][by][plane][s][h][col][j] -> [plane][k][chunk][s][h][j][by][col]
    return v.permute(3, 0, 1, 4, 5, 7, 2, 6).reshape(3, 27, cin, cout)


class ConvSplitPieces(object):
    """The prepared filter pieces of a backbone's conv layers (runner order: conv, subm conv per level) and, per batch size,
    the pointer array the runner's _split entry points take: a layer's entry is its pieces where the table takes the split
    form for that many crops, NULL where the fp32 kernel stays.  Built beside the folded weights (Network._fold) and dropped
    with them."""

    def __init__(self, layers):
        self.meta = [(tuple(int(d) for d in W.shape), bool(subm)) for W, _, _, subm in layers]
        # (weights still on the host -- a Network before .cuda(), which cannot run and folds again once it has moved: no pieces)
        self.planes = [conv_split_weight(W) if W.is_cuda and conv_split_ok(*W.shape) else None for W, _, _, _ in layers]
        self._arrs = {}

    def ptrs(self, batch):
        if not CONV_SPLIT or not CONV_SPLIT_WIDTHS:
            return None
        key = (int(batch), tuple(sorted(CONV_SPLIT_WIDTHS.items())))
        if key not in self._arrs:
            take = []
            for i, ((kvol, cin, cout), subm) in enumerate(self.meta):
                min_rows = CONV_SPLIT_WIDTHS.get((cin, cout, subm))
                rows = int(batch) * CONV_SPLIT_ROWS_PER_CROP[i // 2]
                take.append(self.planes[i] if min_rows is not None and rows >= min_rows else None)
            self._arrs[key] = None if all(t is None for t in take) else \
                (C.c_void_p * len(take))(*[None if t is None else t.data_ptr() for t in take])
        return self._arrs[key]


def sparse_conv_sides(feats, nbrs, n_outs, Ws, subm, pieces=None, scales=None, shifts=None, relu=False, orders=None):
    """One conv layer of one or two problems in ONE launch (what the backbone runner issues for the two backbones of a level),
    from explicit gather tables.  pieces: per side conv_split_weight(W) -- the launch takes the split-bf16 form -- or None: the
    fp32 form of the same launch.  orders: per side the triple of order_rows.  -> list of outputs."""
    ns = len(feats)
    assert ns in (1, 2) and len(nbrs) == ns and len(Ws) == ns
    N.need_cuda(*feats)
    kvol, cin, cout = Ws[0].shape
    outs = [torch.empty((int(n), cout), dtype=torch.float32, device=feats[0].device) for n in n_outs]
    cap_sum = sum(int(nb.shape[1]) for nb in nbrs)
    scratch = torch.empty(N.query("dcl_sparse_conv_scratch_floats", int(cap_sum), int(cout)), dtype=torch.float32,
                          device=feats[0].device)
    arr = lambda ts: None if ts is None else _ptr_array(ts)                                   # noqa: E731
    N.check(N.lib().dcl_sparse_conv_fwd_sides(
        ns, _ptr_array(feats), _ptr_array(nbrs), (C.c_int32 * ns)(*[int(nb.shape[1]) for nb in nbrs]),
        (C.c_int32 * ns)(*[int(n) for n in n_outs]), _ptr_array(Ws), arr(pieces), int(cin), int(cout), int(kvol), int(bool(subm)),
        arr(scales), arr(shifts), int(bool(relu)), _ptr_array(outs), N.ptr(scratch), scratch.numel(),
        arr(None if orders is None else [o[0] for o in orders]), arr(None if orders is None else [o[1] for o in orders]),
        arr(None if orders is None else [o[2] for o in orders]), N.stream()), "sparse_conv_fwd_sides")
    return outs


class BackboneRun(object):
    """State of one backbone pass driven by the native runner (csrc/backbone.hip)."""

    def __init__(self, occ, batch, S, batch_lo=0, counts_dev=None):
        """occ (V0,4) i32 [b,x,y,z]; batch_lo > 0 (or batch < number of crops in occ): pass over the crop window
        batch_lo .. batch_lo+batch-1 only (its crops are re-based to 0).  counts_dev: optional i32[8] slice of a caller's
        tensor that receives the level sizes -- a device tensor (several passes can then be read back with one copy) or
        PINNED host memory, which the geometry kernels write directly (the caller waits for the stream and reads it)."""
        N.need_cuda(occ)
        assert occ.dtype == torch.int32 and occ.is_contiguous()
        self.occ, self.batch, self.S, self.V0 = occ, int(batch), int(S), occ.shape[0]
        nbytes = N.query("dcl_backbone_ws_bytes", self.batch, self.S, self.V0)
        self.ws = torch.empty(nbytes, dtype=torch.uint8, device=occ.device)
        if counts_dev is not None and not counts_dev.is_cuda and not counts_dev.is_pinned():
            raise RuntimeError("BackboneRun: a host counts buffer must be pinned (the geometry kernels write into it)")
        self.counts_dev = torch.empty(8, dtype=torch.int32, device=occ.device) if counts_dev is None else counts_dev
        self.chan = (C.c_int32 * 9)(*BACKBONE_CHANNELS)
        N.check(N.lib().dcl_backbone_geometry_window(N.ptr(occ), self.V0, int(batch_lo), self.batch, self.S, N.ptr(self.ws),
                                                     nbytes, N.ptr(self.counts_dev), N.stream()),
                "backbone_geometry")
        self.counts = None
        self.levels = None

    def set_counts(self, counts):
        self.counts = [int(c) for c in counts]
        self.ccounts = (C.c_int32 * 8)(*self.counts)

    def features(self, vox_feats, weights_arr, scales_arr, shifts_arr, split=None):
        """-> list of 4 level feature tensors (n_pool_m, C_m).  split: the backbone's ConvSplitPieces (the layers CONV_SPLIT_WIDTHS
        lists for this many crops then run the split-bf16 conv form) or None."""
        dev = vox_feats.device
        nbytes = N.query("dcl_backbone_ws2_bytes", self.ccounts, self.chan)
        ws2 = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self.levels = [torch.empty((self.counts[2 * m + 1], BACKBONE_CHANNELS[2 * m + 2]), dtype=torch.float32,
                                   device=dev) for m in range(4)]
        N.check(N.lib().dcl_backbone_features_split(N.ptr(self.occ), self.V0, self.batch, self.S, N.ptr(self.ws), self.ccounts,
                                                    self.chan, N.ptr(vox_feats), weights_arr,
                                                    None if split is None else split.ptrs(self.batch), scales_arr, shifts_arr,
                                                    N.ptr(ws2), nbytes, _ptr_array(self.levels), N.stream()),
                "backbone_features")
        return self.levels

    def level_indices(self, m):
        """(n_pool_m, 4) int32 view of pooled level m's voxel rows inside the workspace."""
        off, _, _ = N.query("dcl_backbone_level_info", self.batch, self.S, self.V0, m, ctype=(C.c_int64, C.c_int64, C.c_int32))
        n = self.counts[2 * m + 1]
        return self.ws[off:off + 16 * n].view(torch.int32).view(n, 4)

    def point_features(self, points_b4, voxel_extents, offset, out=None):
        """points_b4 (n,4) -> (n,480) interpolated multi-scale features."""
        n = points_b4.shape[0]
        dev = points_b4.device
        if out is None:
            out = torch.empty((n, 480), dtype=torch.float32, device=dev)
        tmp_bytes = 2 * (((n * 48) + 255) // 256 * 256)                       # dist2 + idx of the 4 levels
        tmp = torch.empty(tmp_bytes, dtype=torch.uint8, device=dev)
        ve = (C.c_float * 4)(*[float(v) for v in voxel_extents])
        N.check(N.lib().dcl_point_features(n, N.ptr(points_b4), self.batch, self.S, self.V0, N.ptr(self.ws), self.ccounts,
                                           self.chan, _ptr_array(self.levels), ve, offset, N.ptr(out),
                                           out.stride(0), N.ptr(tmp), tmp_bytes, N.stream()), "point_features")
        return out

    def point_features_fold(self, points_b4, voxel_extents, offset, nfold, out=None):
        """point_features with its nfold (1 or 2) deepest levels left to the GEMM that consumes the read-out (linear_split_gather):
        -> (out (n, 224 or 96): exactly the first columns of point_features; fw (nfold, n, 3) float32: the folded levels'
        normalised interpolation weights; fi (nfold, n, 3) int32: their neighbour rows), folded levels ascending.  Always the
        two-launch read-out (csrc/backbone.hip: dcl_point_features_fold)."""
        assert nfold in (1, 2)
        n = points_b4.shape[0]
        dev = points_b4.device
        K0 = sum(BACKBONE_CHANNELS[2 * m + 2] for m in range(4 - nfold))
        if out is None:
            out = torch.empty((n, K0), dtype=torch.float32, device=dev)
        assert out.shape == (n, K0) and out.dtype == torch.float32 and out.stride(1) == 1
        fw = torch.empty((nfold, n, 3), dtype=torch.float32, device=dev)
        fi = torch.empty((nfold, n, 3), dtype=torch.int32, device=dev)
        tmp_bytes = 2 * (((n * 48) + 255) // 256 * 256)                       # dist2 + idx of the 4 levels
        tmp = torch.empty(tmp_bytes, dtype=torch.uint8, device=dev)
        ve = (C.c_float * 4)(*[float(v) for v in voxel_extents])
        N.check(N.lib().dcl_point_features_fold(n, N.ptr(points_b4), self.batch, self.S, self.V0, N.ptr(self.ws), self.ccounts,
                                                self.chan, _ptr_array(self.levels), ve, offset, int(nfold), N.ptr(out),
                                                out.stride(0), N.ptr(fw), N.ptr(fi), N.ptr(tmp), tmp_bytes, N.stream()),
                "point_features_fold")
        return out, fw, fi

    def point_neighbours(self, points_b4, voxel_extents, offset):
        """first half of point_features: the four 3-NN searches (need geometry + counts only, not the level features).
        Returns (dist2, idx), each (4, n, 3)."""
        n = points_b4.shape[0]
        dev = points_b4.device
        dist2 = torch.empty((4, n, 3), dtype=torch.float32, device=dev)
        idx = torch.empty((4, n, 3), dtype=torch.int32, device=dev)
        ve = (C.c_float * 4)(*[float(v) for v in voxel_extents])
        N.check(N.lib().dcl_point_neighbours(n, N.ptr(points_b4), self.batch, self.S, self.V0, N.ptr(self.ws), self.ccounts,
                                             ve, offset, N.ptr(dist2), N.ptr(idx), N.stream()),
                "point_neighbours")
        return dist2, idx

    def point_interpolate(self, dist2, idx, out=None):
        """second half of point_features: inverse-distance interpolation of the four levels' features -> (n, 480)."""
        n = idx.shape[1]
        if out is None:
            out = torch.empty((n, 480), dtype=torch.float32, device=idx.device)
        N.check(N.lib().dcl_point_interpolate(n, self.ccounts, self.chan, _ptr_array(self.levels), N.ptr(dist2),
                                              N.ptr(idx), N.ptr(out), out.stride(0), N.stream()), "point_interpolate")
        return out


def backbone_features_pair(run_a, vox_a, ptrs_a, run_b, vox_b, ptrs_b):
    """The feature stage of BOTH backbones of a forward (observed / template side; two BackboneRun or two BackboneRunCap of
    the same batch and grid): every layer is one launch over both sides' tiles (dcl_backbone_features_pair), so the fixed
    part of a launch is paid once per layer, not once per layer and side.  ptrs_*: (weights, scales, shifts) pointer
    arrays of a side, optionally followed by the side's ConvSplitPieces.  Fills run_*.levels like run.features()."""
    cap_mode = isinstance(run_a, BackboneRunCap)
    assert isinstance(run_b, type(run_a)) and run_a.batch == run_b.batch and run_a.S == run_b.S
    dev = vox_a.device
    runs, voxs, ptrs = (run_a, run_b), (vox_a, vox_b), (ptrs_a, ptrs_b)
    if cap_mode:
        ws2 = [r.ws2 for r in runs]
        ws2_bytes = [r.ws2_bytes for r in runs]
        counts_host, counts_dev = None, (C.c_void_p * 2)(*[r.counts_dev.data_ptr() for r in runs])
    else:
        ws2, ws2_bytes = [], []
        for r in runs:
            ws2_bytes.append(N.query("dcl_backbone_ws2_bytes", r.ccounts, r.chan))
            ws2.append(torch.empty(ws2_bytes[-1], dtype=torch.uint8, device=dev))
            r.levels = [torch.empty((r.counts[2 * m + 1], BACKBONE_CHANNELS[2 * m + 2]), dtype=torch.float32, device=dev)
                        for m in range(4)]
        counts_host = (C.POINTER(C.c_int32) * 2)(*[C.cast(r.ccounts, C.POINTER(C.c_int32)) for r in runs])
        counts_dev = None
    level_ptrs = [r.level_ptrs if cap_mode else _ptr_array(r.levels) for r in runs]
    pp = lambda arrs: (C.c_void_p * 2)(*[C.cast(a, C.c_void_p) for a in arrs])                # noqa: E731
    pieces = [p[3].ptrs(run_a.batch) if len(p) > 3 and p[3] is not None else None for p in ptrs]
    N.check(N.lib().dcl_backbone_features_pair_split(
        run_a.batch, run_a.S, run_a.chan, (C.c_int32 * 2)(run_a.V0, run_b.V0),
        (C.c_void_p * 2)(*[r.ws.data_ptr() for r in runs]), counts_host, counts_dev,
        (C.c_void_p * 2)(*[v.data_ptr() for v in voxs]), pp([p[0] for p in ptrs]),
        None if all(q is None for q in pieces) else pp(pieces), pp([p[1] for p in ptrs]),
        pp([p[2] for p in ptrs]), (C.c_void_p * 2)(*[w.data_ptr() for w in ws2]), (C.c_int64 * 2)(*ws2_bytes),
        pp(level_ptrs), N.stream()), "backbone_features_pair")
    if not cap_mode:
        for r, w in zip(runs, ws2):
            r._ws2_keep = w                                # the levels are separate tensors; the scratch may go when the run goes
    return run_a.levels, run_b.levels


class BackboneRunCap(object):
    """Capacity-mode backbone pass (whole-forward hipGraph capture): every buffer is sized from (batch, S, V0_cap) alone,
    live row counts stay on the device, no host read-back.  `occ` is a STATIC (V0_cap,4) buffer whose first *v0_dev rows
    are live.  All methods only enqueue work, so they can run under torch.cuda.graph()."""

    def __init__(self, occ, v0_dev, batch, S):
        N.need_cuda(occ, v0_dev)
        assert occ.dtype == torch.int32 and occ.is_contiguous() and v0_dev.dtype == torch.int32
        self.occ, self.v0_dev, self.batch, self.S, self.V0 = occ, v0_dev, int(batch), int(S), occ.shape[0]
        dev = occ.device
        self.ws_bytes = N.query("dcl_backbone_ws_bytes", self.batch, self.S, self.V0)
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=dev)
        self.counts_dev = torch.zeros(8, dtype=torch.int32, device=dev)
        self.chan = (C.c_int32 * 9)(*BACKBONE_CHANNELS)
        self.caps = (C.c_int32 * 8)()
        N.check(N.lib().dcl_backbone_caps(self.batch, self.S, self.V0, self.caps), "backbone_caps")
        self.ws2_bytes = N.query("dcl_backbone_ws2_bytes", self.caps, self.chan)
        self.ws2 = torch.empty(self.ws2_bytes, dtype=torch.uint8, device=dev)
        self.levels = [torch.empty((self.caps[2 * m + 1], BACKBONE_CHANNELS[2 * m + 2]), dtype=torch.float32, device=dev)
                       for m in range(4)]
        self.level_ptrs = _ptr_array(self.levels)

    def geometry(self, voxelize=None):
        """voxelize = (feats (N,C) f32, map_rule (M, 1 + maxActive) i32, mode): also returns voxelize_fp(feats, map_rule, mode),
        carried by the geometry stage's own launch where that is one launch (up to 16 crops)"""
        if voxelize is None:
            N.check(N.lib().dcl_backbone_geometry_cap(N.ptr(self.occ), N.ptr(self.v0_dev), self.V0, self.batch, self.S,
                                                      N.ptr(self.ws), self.ws_bytes, N.ptr(self.counts_dev), N.stream()),
                    "backbone_geometry_cap")
            return None
        feats, rule, mode = voxelize
        N.need_cuda(feats, rule)
        assert feats.is_contiguous() and rule.is_contiguous() and feats.dtype == torch.float32 and rule.dtype == torch.int32
        out = torch.empty((rule.shape[0], feats.shape[1]), dtype=torch.float32, device=feats.device)
        N.check(N.lib().dcl_backbone_geometry_cap_vox(N.ptr(self.occ), N.ptr(self.v0_dev), self.V0, self.batch, self.S,
                                                      N.ptr(self.ws), self.ws_bytes, N.ptr(self.counts_dev), N.ptr(feats),
                                                      N.ptr(rule), N.ptr(out), rule.shape[0], rule.shape[1] - 1, feats.shape[1],
                                                      int(mode == 4), N.stream()), "backbone_geometry_cap_vox")
        return out

    def features(self, vox_feats, weights_arr, scales_arr, shifts_arr, split=None):
        N.check(N.lib().dcl_backbone_features_cap_split(N.ptr(self.occ), self.V0, self.batch, self.S, N.ptr(self.ws),
                                                        N.ptr(self.counts_dev), self.chan, N.ptr(vox_feats), weights_arr,
                                                        None if split is None else split.ptrs(self.batch), scales_arr,
                                                        shifts_arr, N.ptr(self.ws2), self.ws2_bytes, self.level_ptrs,
                                                        N.stream()), "backbone_features_cap")
        return self.levels

    def point_features(self, points_b4, voxel_extents, offset, out, tmp):
        n = points_b4.shape[0]
        ve = (C.c_float * 4)(*[float(v) for v in voxel_extents])
        N.check(N.lib().dcl_point_features_cap(n, N.ptr(points_b4), self.batch, self.S, self.V0, N.ptr(self.ws),
                                               N.ptr(self.counts_dev), self.chan, self.level_ptrs, ve, offset,
                                               N.ptr(out), out.stride(0), N.ptr(tmp), tmp.numel(), N.stream()),
                "point_features_cap")
        return out

    def tmp_bytes(self, n):
        return 2 * (((n * 48) + 255) // 256 * 256)

    def point_neighbours(self, points_b4, voxel_extents, offset, dist2, idx):
        """dist2 / idx: static (4, n, 3) buffers (see BackboneRun.point_neighbours)"""
        n = points_b4.shape[0]
        ve = (C.c_float * 4)(*[float(v) for v in voxel_extents])
        N.check(N.lib().dcl_point_neighbours_cap(n, N.ptr(points_b4), self.batch, self.S, self.V0, N.ptr(self.ws), ve,
                                                 offset, N.ptr(dist2), N.ptr(idx), N.stream()),
                "point_neighbours_cap")

    def point_interpolate(self, dist2, idx, out):
        n = idx.shape[1]
        N.check(N.lib().dcl_point_interpolate(n, self.caps, self.chan, self.level_ptrs, N.ptr(dist2), N.ptr(idx),
                                              N.ptr(out), out.stride(0), N.stream()), "point_interpolate")
        return out


# ------------------------------------------------------------------------------------ pointnet_sp
def three_nn_sp(unknown, known, known_seg=None):
    """pointnet2_cuda.three_nn_wrapper of libs/pointnet_sp: returns (dist2 (N,3), idx (N,3) i32)."""
    N.need_cuda(unknown, known)
    assert unknown.is_contiguous() and known.is_contiguous()
    assert unknown.shape[1] == 4 and known.shape[1] == 4
    n, m = unknown.shape[0], known.shape[0]
    dist2 = torch.empty((n, 3), dtype=torch.float32, device=unknown.device)
    idx = torch.empty((n, 3), dtype=torch.int32, device=unknown.device)
    nb = 0 if known_seg is None else known_seg.numel() - 1
    N.check(N.lib().dcl_three_nn_sp(n, m, N.ptr(unknown), N.ptr(known), N.ptr(dist2), N.ptr(idx),
                                    _i32_ptr_or_null(known_seg), nb, N.stream()), "three_nn_sp")
    return dist2, idx


def three_interpolate_sp(features, idx, weight, out=None, from_dist2=False):
    """three_interpolate_wrapper of libs/pointnet_sp: features (M,C), idx (n,3), weight (n,3) -> (n,C).
    `out` may be a column block of a wider row-major buffer (its row stride is honoured);
    from_dist2=True treats `weight` as three_nn's dist2 and forms the weights in-kernel."""
    N.need_cuda(features, idx, weight)
    assert features.is_contiguous() and idx.is_contiguous() and weight.is_contiguous()
    m, c = features.shape
    n = idx.shape[0]
    if out is None:
        out = torch.empty((n, c), dtype=torch.float32, device=features.device)
    assert out.shape == (n, c) and out.stride(1) == 1
    fn = N.lib().dcl_three_interpolate_dist2_sp if from_dist2 else N.lib().dcl_three_interpolate_sp
    N.check(fn(c, m, n, N.ptr(features), N.ptr(idx), N.ptr(weight), N.ptr(out), out.stride(0) if n > 1 else c,
               N.stream()), "three_interpolate_sp")
    return out


def voxel_centres(aset_or_indices, ve, off, n=None):
    """Ops_tensor2points (models/Modules.py:204-211) on device."""
    ind = aset_or_indices
    n = ind.shape[0] if n is None else n
    out = torch.empty((max(n, 1), 4), dtype=torch.float32, device=ind.device)
    N.check(N.lib().dcl_voxel_centres(N.ptr(ind), N.vp(0), int(n), ve, off, N.ptr(out), N.stream()),
            "voxel_centres")
    return out[:n]


# ------------------------------------------------------------------------------------ pointnet_lib
def ball_query(radius, nsample, xyz, new_xyz):
    N.need_cuda(xyz, new_xyz)
    assert xyz.is_contiguous() and new_xyz.is_contiguous()
    B, n, _ = xyz.shape
    m = new_xyz.shape[1]
    idx = torch.empty((B, m, nsample), dtype=torch.int32, device=xyz.device)
    N.check(N.lib().dcl_ball_query(B, n, m, radius, int(nsample), N.ptr(new_xyz), N.ptr(xyz), N.ptr(idx),
                                   N.stream()), "ball_query")
    return idx


def group_points(features, idx, out=None):
    """out (optional): a channel block out_full[:, c0:c0+c] of a contiguous (B, C_total, npoint, nsample) tensor, filled
    in place (no concatenation copy afterwards)."""
    N.need_cuda(features, idx, out)
    assert features.is_contiguous() and idx.is_contiguous() and idx.dtype == torch.int32
    B, c, n = features.shape
    _, npoint, ns = idx.shape
    if out is None:
        out = torch.empty((B, c, npoint, ns), dtype=torch.float32, device=features.device)
    assert out.shape == (B, c, npoint, ns) and out.stride(3) == 1 and out.stride(2) == ns and out.stride(1) == npoint * ns
    oc = out.stride(0) // (npoint * ns) if B > 1 else c
    assert B == 1 or out.stride(0) == oc * npoint * ns
    N.check(N.lib().dcl_group_points_into(B, c, n, npoint, ns, N.ptr(features), N.ptr(idx), N.ptr(out), int(oc),
                                          N.stream()), "group_points")
    return out


def gather_points(features, idx):
    N.need_cuda(features, idx)
    assert features.is_contiguous() and idx.is_contiguous() and idx.dtype == torch.int32
    B, c, n = features.shape
    m = idx.shape[1]
    out = torch.empty((B, c, m), dtype=torch.float32, device=features.device)
    N.check(N.lib().dcl_gather_points(B, c, n, m, N.ptr(features), N.ptr(idx), N.ptr(out), N.stream()), "gather_points")
    return out


def furthest_point_sampling(xyz, npoint):
    N.need_cuda(xyz)
    assert xyz.is_contiguous()
    B, n, _ = xyz.shape
    temp = torch.full((B, n), 1e10, dtype=torch.float32, device=xyz.device)
    idx = torch.empty((B, npoint), dtype=torch.int32, device=xyz.device)
    N.check(N.lib().dcl_furthest_point_sampling(B, n, int(npoint), N.ptr(xyz), N.ptr(temp), N.ptr(idx), N.stream()),
            "furthest_point_sampling")
    return idx


def knn(k, unknown, known):
    N.need_cuda(unknown, known)
    assert unknown.is_contiguous() and known.is_contiguous()
    B, n, _ = unknown.shape
    m = known.shape[1]
    if k <= 3:
        # the sorted strict-'<' list of length k is the first k entries of the 3-NN cascade (same tie rule, same
        # defaults for missing neighbours): use the tiled three_nn kernel (DCL-Net only calls knn with k = 1)
        d2, idx = three_nn(unknown, known)
        return d2[:, :, :k].contiguous(), idx[:, :, :k].contiguous()
    dist2 = torch.empty((B, n, k), dtype=torch.float32, device=unknown.device)
    idx = torch.empty((B, n, k), dtype=torch.int32, device=unknown.device)
    N.check(N.lib().dcl_knn(B, n, m, int(k), N.ptr(unknown), N.ptr(known), N.ptr(dist2), N.ptr(idx), N.stream()), "knn")
    return dist2, idx


def three_nn(unknown, known):
    N.need_cuda(unknown, known)
    assert unknown.is_contiguous() and known.is_contiguous()
    B, n, _ = unknown.shape
    m = known.shape[1]
    dist2 = torch.empty((B, n, 3), dtype=torch.float32, device=unknown.device)
    idx = torch.empty((B, n, 3), dtype=torch.int32, device=unknown.device)
    N.check(N.lib().dcl_three_nn(B, n, m, N.ptr(unknown), N.ptr(known), N.ptr(dist2), N.ptr(idx), N.stream()),
            "three_nn")
    return dist2, idx


def _chamfer_args(pred, target, active):
    N.need_cuda(pred, target, active)
    assert pred.dim() == 3 and target.dim() == 3 and pred.shape[2] == 3 and target.shape[2] == 3
    assert pred.shape[0] == target.shape[0] and pred.dtype == torch.float32 and target.dtype == torch.float32
    assert pred.is_contiguous() and target.is_contiguous()
    assert active is None or (active.dtype == torch.int32 and active.shape == (pred.shape[0],) and active.is_contiguous())
    return pred.shape[0], pred.shape[1], target.shape[1]


def chamfer(pred, target, active=None):
    """Nearest-neighbour distances in both directions without the pairwise matrix (csrc/chamfer.hip; include/dclnet_hip.h at
    dcl_chamfer_fwd): pred (b,n,3), target (b,m,3) fp32 contiguous -> (dist_pt (b,n), idx_pt (b,n) i32, dist_tp (b,m),
    idx_tp (b,m) i32).  active (b,) i32 or None: crops whose flag is 0 are not computed (distance 0, index -1)."""
    b, n, m = _chamfer_args(pred, target, active)
    dev = pred.device
    dist_pt, idx_pt = torch.empty((b, n), dtype=torch.float32, device=dev), torch.empty((b, n), dtype=torch.int32, device=dev)
    dist_tp, idx_tp = torch.empty((b, m), dtype=torch.float32, device=dev), torch.empty((b, m), dtype=torch.int32, device=dev)
    N.check(N.lib().dcl_chamfer_fwd(b, n, m, N.ptr(pred), N.ptr(target), N.ptr(active), N.ptr(dist_pt), N.ptr(idx_pt),
                                    N.ptr(dist_tp), N.ptr(idx_tp), N.stream()), "chamfer_fwd")
    return dist_pt, idx_pt, dist_tp, idx_tp


def chamfer_backward(pred, target, idx_pt, idx_tp, g_pt, g_tp, active=None, need_pred=True, need_target=True):
    """Gradients of one chamfer call (dcl_chamfer_bwd): idx_pt, idx_tp as chamfer returned them, g_pt (b,n), g_tp (b,m) the
    upstream gradients of the two distance outputs -> (grad_pred (b,n,3), grad_target (b,m,3)); a gradient that is not
    needed is None and is not computed.  Deterministic: the same inputs give the same bits."""
    b, n, m = _chamfer_args(pred, target, active)
    N.need_cuda(idx_pt, idx_tp, g_pt, g_tp)
    assert need_pred or need_target
    assert idx_pt.shape == (b, n) and idx_tp.shape == (b, m) and idx_pt.dtype == torch.int32 and idx_tp.dtype == torch.int32
    assert g_pt.shape == (b, n) and g_tp.shape == (b, m) and g_pt.dtype == torch.float32 and g_tp.dtype == torch.float32
    assert idx_pt.is_contiguous() and idx_tp.is_contiguous() and g_pt.is_contiguous() and g_tp.is_contiguous()
    grad_pred = torch.empty((b, n, 3), dtype=torch.float32, device=pred.device) if need_pred else None
    grad_target = torch.empty((b, m, 3), dtype=torch.float32, device=pred.device) if need_target else None
    N.check(N.lib().dcl_chamfer_bwd(b, n, m, N.ptr(pred), N.ptr(target), N.ptr(active), N.ptr(idx_pt), N.ptr(idx_tp),
                                    N.ptr(g_pt), N.ptr(g_tp), N.ptr(grad_pred), N.ptr(grad_target), N.stream()),
            "chamfer_bwd")
    return grad_pred, grad_target


def _f32_like(t, shape, what):
    assert t.dtype == torch.float32 and tuple(t.shape) == tuple(shape) and t.is_contiguous(), \
        "%s: fp32 contiguous %s wanted, got %s %s" % (what, tuple(shape), t.dtype, tuple(t.shape))


def _same_side(host, what, *ts):
    """host twins take CPU tensors, the kernels the GPU's"""
    for t in ts:
        if t is not None and t.is_cuda == host:
            raise RuntimeError("%s takes %s tensors (got a %s one)%s" % (
                what, "CPU" if host else "GPU", t.device, "" if host else "; no CPU fallback"))


def _rigid_args(pts, R, t, inverse, host, what):
    _same_side(host, what, pts, R, t)
    assert pts.dim() == 3 and pts.shape[2] == 3, tuple(pts.shape)
    b, n = pts.shape[0], pts.shape[1]
    _f32_like(pts, (b, n, 3), "pts")
    _f32_like(R, (b, 3, 3), "R")
    _f32_like(t, (b, 3), "t")
    return b, n, int(bool(inverse))


def _rigid_points(pts, R, t, inverse, host):
    what = "rigid_points_host" if host else "rigid_points"
    b, n, inv = _rigid_args(pts, R, t, inverse, host, what)
    out = torch.empty_like(pts)
    N.twin("dcl_rigid_points", host, what, b, n, N.ptr(pts), N.ptr(R), N.ptr(t), inv, N.ptr(out))
    return out


def _rigid_points_backward(pts, R, t, inverse, g_out, need_pts, host):
    what = "rigid_points_backward_host" if host else "rigid_points_backward"
    b, n, inv = _rigid_args(pts, R, t, inverse, host, what)
    _same_side(host, what, g_out)
    _f32_like(g_out, (b, n, 3), "g_out")
    g_R, g_t = torch.empty_like(R), torch.empty_like(t)
    g_pts = torch.empty_like(pts) if need_pts else None
    N.twin("dcl_rigid_points_bwd", host, what, b, n, N.ptr(pts), N.ptr(R), N.ptr(t), inv, N.ptr(g_out), N.ptr(g_R), N.ptr(g_t),
           N.ptr(g_pts))
    return g_R, g_t, g_pts


def rigid_points(pts, R, t, inverse=False):
    """Rigid transform of b clouds in one launch (dcl_rigid_points): pts (b,n,3), R (b,3,3), t (b,3), fp32 contiguous ->
    (b,n,3).  inverse=False: R p + t (= bmm(p, R^T) + t); inverse=True: R^T (p - t) (= bmm(p - t, R)).  No vendor GEMM."""
    return _rigid_points(pts, R, t, inverse, False)


def rigid_points_backward(pts, R, t, inverse, g_out, need_pts=False):
    """Gradients of rigid_points (dcl_rigid_points_bwd): g_out (b,n,3) -> (g_R (b,3,3), g_t (b,3), g_pts (b,n,3) or None).
    The sums over a crop's points run in the order include/dclnet_hip.h pins: the same inputs give the same bits."""
    return _rigid_points_backward(pts, R, t, inverse, g_out, need_pts, False)


def rigid_points_host(pts, R, t, inverse=False):
    """rigid_points on CPU tensors (the kernel's routine compiled for the host).  For checking the arithmetic where there is
    no GPU; no model path calls it."""
    return _rigid_points(pts, R, t, inverse, True)


def rigid_points_backward_host(pts, R, t, inverse, g_out, need_pts=False):
    """rigid_points_backward on CPU tensors, in the kernel's summation order; no model path calls it."""
    return _rigid_points_backward(pts, R, t, inverse, g_out, need_pts, True)


_OBJ_OPTIONAL = ("Yc", "cano_pred", "cano_gt", "Xo", "conf", "cd_Xo", "cd_Yc")


def _objective_args(posed, posed_gt, sym, cd_pose, Yc, cano_pred, cano_gt, Xo, conf, cd_Xo, cd_Yc, host, what, cd=True):
    """-> (b, n, full, the pointers of the C argument list after b, n: 8 inputs and, with cd, the 6 Chamfer halves)"""
    opt = (Yc, cano_pred, cano_gt, Xo, conf) + ((cd_Xo, cd_Yc) if cd else ())
    full = opt[0] is not None
    if any((o is not None) != full for o in opt):
        raise ValueError("%s: %s go together: all of them, or none for the pose-only form" % (what, ", ".join(_OBJ_OPTIONAL)))
    assert posed.dim() == 3 and posed.shape[2] == 3, tuple(posed.shape)
    b, n = posed.shape[0], posed.shape[1]
    clouds = (posed, posed_gt) + ((Yc, cano_pred, cano_gt, Xo) if full else ())
    halves = (tuple(cd_pose) + ((tuple(cd_Xo) + tuple(cd_Yc)) if full else ())) if cd else ()
    assert len(halves) == ((6 if full else 2) if cd else 0), "every cd_* is the pair (dist_pt, dist_tp) of one chamfer call"
    _same_side(host, what, sym, *(clouds + halves + ((conf,) if full else ())))
    for c in clouds:
        _f32_like(c, (b, n, 3), "cloud")
    for h in halves:
        _f32_like(h, (b, n), "chamfer half")
    _f32_like(sym, (b,), "sym")
    if full:
        _f32_like(conf, (b, 2 * n), "conf")
    p = N.ptr
    ptrs = (p(posed), p(posed_gt), p(Yc), p(cano_pred), p(cano_gt), p(Xo), p(conf), p(sym))
    if cd:
        cdx, cdy = (cd_Xo, cd_Yc) if full else ((None, None), (None, None))
        ptrs += (p(cd_pose[0]), p(cd_pose[1]), p(cdx[0]), p(cdx[1]), p(cdy[0]), p(cdy[1]))
    return b, n, full, ptrs


def _pose_objective(posed, posed_gt, sym, cd_pose, Yc, cano_pred, cano_gt, Xo, conf, cd_Xo, cd_Yc, host):
    what = "pose_objective_host" if host else "pose_objective"
    b, n, full, ptrs = _objective_args(posed, posed_gt, sym, cd_pose, Yc, cano_pred, cano_gt, Xo, conf, cd_Xo, cd_Yc, host, what)
    dev = posed.device
    L = torch.empty((b, 2 * n), dtype=torch.float32, device=dev) if full else None
    crop_sums = torch.empty((max(b, 1), 5), dtype=torch.float32, device=dev)
    packed = torch.zeros((5,), dtype=torch.float32, device=dev) if b == 0 else torch.empty((5,), dtype=torch.float32, device=dev)
    N.twin("dcl_pose_objective_fwd", host, what, b, n, *ptrs, N.ptr(L), N.ptr(crop_sums), N.ptr(packed))
    return packed, L


def _pose_objective_backward(g_packed, posed, posed_gt, sym, Yc, cano_pred, cano_gt, Xo, conf, L, host):
    what = "pose_objective_backward_host" if host else "pose_objective_backward"
    b, n, full, ptrs = _objective_args(posed, posed_gt, sym, None, Yc, cano_pred, cano_gt, Xo, conf, None, None, host, what,
                                       cd=False)
    _same_side(host, what, g_packed, L)
    _f32_like(g_packed, (5,), "g_packed")
    assert (L is not None) == full, "L goes with the full form"
    if full:
        _f32_like(L, (b, 2 * n), "L")
    dev = posed.device
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)                  # noqa: E731
    g_posed = new(b, n, 3)
    g_cd = [new(b, n) for _ in range(6 if full else 2)] + ([] if full else [None] * 4)
    g_Xo, g_Yc, g_conf = (new(b, n, 3), new(b, n, 3), new(b, 2 * n)) if full else (None, None, None)
    outs = (N.ptr(g_packed), N.ptr(g_posed), N.ptr(g_Xo), N.ptr(g_Yc), N.ptr(g_conf)) + tuple(N.ptr(g) for g in g_cd)
    N.twin("dcl_pose_objective_bwd", host, what, b, n, *ptrs, N.ptr(L), *outs)
    return g_posed, g_Xo, g_Yc, g_conf, (g_cd[0], g_cd[1]), (g_cd[2], g_cd[3]), (g_cd[4], g_cd[5])


def pose_objective(posed, posed_gt, sym, cd_pose, Yc=None, cano_pred=None, cano_gt=None, Xo=None, conf=None, cd_Xo=None,
                   cd_Yc=None):
    """The per-point terms of `losses.forward` and their ordered sums (dcl_pose_objective_fwd; include/dclnet_hip.h has the
    formulas and the pinned summation order).  posed, posed_gt, Yc, cano_pred, cano_gt, Xo (b,n,3); conf (b,2n); sym (b,)
    float; cd_pose, cd_Xo, cd_Yc: the (dist_pt, dist_tp) pairs `chamfer` returned for (posed, posed_gt), (Xo, template),
    (Yc, posed_gt), each (b,n).  -> (packed (5,) = [loss_pose, loss_Xo, loss_Yc, loss_conf, loss_all], L (b,2n) = the
    per-point [loss_Xo | loss_Yc] rows the backward reads).  With the optional arguments all None only the pose term is
    formed (`losses_refiner`): packed = [loss_pose, 0, 0, 0, loss_pose], L = None.  No host synchronisation."""
    return _pose_objective(posed, posed_gt, sym, cd_pose, Yc, cano_pred, cano_gt, Xo, conf, cd_Xo, cd_Yc, False)


def pose_objective_backward(g_packed, posed, posed_gt, sym, Yc=None, cano_pred=None, cano_gt=None, Xo=None, conf=None, L=None):
    """Every gradient of pose_objective in one launch (dcl_pose_objective_bwd): g_packed (5,) the upstream gradient of
    packed, on the device; the clouds, conf, sym as the forward took them and the L it returned (the Chamfer halves are not
    read: their gradients depend on sym alone) -> (g_posed, g_Xo, g_Yc, g_conf, g_cd_pose, g_cd_Xo, g_cd_Yc), the last
    three (pt, tp) pairs; the pose-only form returns None for what it does not have.  Deterministic."""
    return _pose_objective_backward(g_packed, posed, posed_gt, sym, Yc, cano_pred, cano_gt, Xo, conf, L, False)


def pose_objective_host(posed, posed_gt, sym, cd_pose, Yc=None, cano_pred=None, cano_gt=None, Xo=None, conf=None,
                        cd_Xo=None, cd_Yc=None):
    """pose_objective on CPU tensors: the kernels' routines compiled for the host, in their summation order.  For checking the
    arithmetic where there is no GPU; no model path calls it."""
    return _pose_objective(posed, posed_gt, sym, cd_pose, Yc, cano_pred, cano_gt, Xo, conf, cd_Xo, cd_Yc, True)


def pose_objective_backward_host(g_packed, posed, posed_gt, sym, Yc=None, cano_pred=None, cano_gt=None, Xo=None, conf=None,
                                 L=None):
    """pose_objective_backward on CPU tensors; no model path calls it."""
    return _pose_objective_backward(g_packed, posed, posed_gt, sym, Yc, cano_pred, cano_gt, Xo, conf, L, True)


def _conf_pool_cm_args(w, F1, F2, host, what):
    _same_side(host, what, w, F1, F2)
    assert F1.dim() == 3 and F2.dim() == 3 and F1.shape[:2] == F2.shape[:2], (tuple(F1.shape), tuple(F2.shape))
    b, c, n1, n2 = F1.shape[0], F1.shape[1], F1.shape[2], F2.shape[2]
    assert tuple(w.shape) == (b, n1 + n2), "w: (b, n1 + n2) = %s wanted, got %s" % ((b, n1 + n2), tuple(w.shape))
    return b, c, n1, n2, N.f32c(w), N.f32c(F1), N.f32c(F2)


def _conf_pool_pm_args(w, F1, F2, host, what):
    _same_side(host, what, w, F1, F2)
    assert F1.dim() == 2 and F2.dim() == 2 and F1.shape[1] == F2.shape[1], (tuple(F1.shape), tuple(F2.shape))
    assert w.dim() == 2, tuple(w.shape)
    b, c = w.shape[0], F1.shape[1]
    assert b >= 1 and F1.shape[0] % b == 0 and F2.shape[0] % b == 0, (b, tuple(F1.shape), tuple(F2.shape))
    n1, n2 = F1.shape[0] // b, F2.shape[0] // b
    assert tuple(w.shape) == (b, n1 + n2), "w: (b, n1 + n2) = %s wanted, got %s" % ((b, n1 + n2), tuple(w.shape))
    return b, c, n1, n2, N.f32c(w), N.f32c(F1), N.f32c(F2)


_CONF_POOL_ARGS = {"cm": _conf_pool_cm_args, "pm": _conf_pool_pm_args}


def _conf_pool_layout(layout, w, F1, F2, host):
    """conf_pool_cm / conf_pool_pm and their host twins: one implementation, the layout picks the shape check and the symbols"""
    what = "conf_pool_%s%s" % (layout, "_host" if host else "")
    b, c, n1, n2, w, F1, F2 = _CONF_POOL_ARGS[layout](w, F1, F2, host, what)
    pooled = torch.empty((b, c), dtype=torch.float32, device=F1.device)
    N.twin("dcl_conf_pool_%s_fwd" % layout, host, what, b, c, n1, n2, N.ptr(w), N.ptr(F1), N.ptr(F2), N.ptr(pooled))
    return pooled


def _conf_pool_layout_backward(layout, conf, w, F1, F2, g_pooled, g_conf, need_logits, need_F, host):
    what = "conf_pool_%s_backward%s" % (layout, "_host" if host else "")
    b, c, n1, n2, w, F1, F2 = _CONF_POOL_ARGS[layout](w, F1, F2, host, what)
    _same_side(host, what, conf, g_pooled, g_conf)
    assert need_logits or need_F
    assert tuple(conf.shape) == (b, n1 + n2) and tuple(g_pooled.shape) == (b, c), (tuple(conf.shape), tuple(g_pooled.shape))
    assert g_conf is None or tuple(g_conf.shape) == (b, n1 + n2), tuple(g_conf.shape)
    conf, g_pooled = N.f32c(conf), N.f32c(g_pooled)
    g_conf = None if g_conf is None else N.f32c(g_conf)
    dev = F1.device
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)                  # noqa: E731
    dl1, dl2 = (new(b, n1), new(b, n2)) if need_logits else (None, None)
    dF1, dF2 = (torch.empty_like(F1), torch.empty_like(F2)) if need_F else (None, None)
    scratch = ()
    if not host:
        ws, nbytes = None, 0
        if need_logits:
            nbytes = N.query("dcl_conf_pool_%s_bwd_ws_bytes" % layout, b, c, n1, n2)
            ws = torch.empty((max(nbytes, 4) // 4,), dtype=torch.float32, device=dev)
        scratch = (N.ptr(ws), nbytes)
    N.twin("dcl_conf_pool_%s_bwd" % layout, host, what, b, c, n1, n2, N.ptr(conf), N.ptr(w), N.ptr(F1), N.ptr(F2), N.ptr(g_pooled),
           N.ptr(g_conf), N.ptr(dl1), N.ptr(dl2), N.ptr(dF1), N.ptr(dF2), *scratch)
    return dl1, dl2, dF1, dF2


def conf_pool_cm(w, F1, F2):
    """The confidence-weighted pooling on channel-major activations (dcl_conf_pool_cm_fwd; csrc/conf_pool_grad.hip): w (b, n1+n2)
    the softmax weights as conf_softmax leaves them, F1 (b,C,n1), F2 (b,C,n2) -> pooled (b,C) = sum_j w[j] F[c][j] over both
    directions, in the summation order include/dclnet_hip.h pins.  One launch; F is read once and nothing of its size is made
    (a non-contiguous F is copied first)."""
    return _conf_pool_layout("cm", w, F1, F2, False)


def conf_pool_cm_backward(conf, w, F1, F2, g_pooled, g_conf=None, need_logits=True, need_F=True):
    """Gradients of sigmoid -> softmax -> conf_pool_cm (dcl_conf_pool_cm_bwd): conf, w (b, n1+n2) as conf_softmax returned them,
    g_pooled (b,C) and g_conf (b, n1+n2) or None (zero) the upstream gradients of pooled and conf -> (dlogit1 (b,n1), dlogit2
    (b,n2), dF1 (b,C,n1), dF2 (b,C,n2)); a pair that is not needed is None and is not computed.  F is read once (for the
    logits), dF is a pure write; no atomics, every sum in a pinned order: the same inputs give the same bits."""
    return _conf_pool_layout_backward("cm", conf, w, F1, F2, g_pooled, g_conf, need_logits, need_F, False)


def conf_pool_cm_host(w, F1, F2):
    """conf_pool_cm on CPU tensors: the kernel's routines compiled for the host, in their summation order.  For checking the
    arithmetic where there is no GPU; no model path calls it."""
    return _conf_pool_layout("cm", w, F1, F2, True)


def conf_pool_cm_backward_host(conf, w, F1, F2, g_pooled, g_conf=None, need_logits=True, need_F=True):
    """conf_pool_cm_backward on CPU tensors; no model path calls it."""
    return _conf_pool_layout_backward("cm", conf, w, F1, F2, g_pooled, g_conf, need_logits, need_F, True)


POOL_PM_ROWS = N.define("DCL_POOL_PM_ROWS")         # the rows per chunk of the point-major pooling's sums


def conf_pool_pm(w, F1, F2):
    """The confidence-weighted pooling on point-major activations (dcl_conf_pool_pm_fwd; csrc/conf_pool_pm.hip): w (b, n1+n2)
    the softmax weights as conf_softmax leaves them, F1 (b n1, C), F2 (b n2, C) row-major, crop i owning rows i n .. i n + n - 1
    -> pooled (b,C) = sum_j w[j] F[j][c] over both directions, in the summation order include/dclnet_hip.h pins (chunks of
    POOL_PM_ROWS rows).  One launch; F is read once and nothing of its size is made (a non-contiguous F is copied first)."""
    return _conf_pool_layout("pm", w, F1, F2, False)


def conf_pool_pm_backward(conf, w, F1, F2, g_pooled, g_conf=None, need_logits=True, need_F=True):
    """Gradients of sigmoid -> softmax -> conf_pool_pm (dcl_conf_pool_pm_bwd): conf, w (b, n1+n2) as conf_softmax returned them,
    g_pooled (b,C) and g_conf (b, n1+n2) or None (zero) the upstream gradients of pooled and conf -> (dlogit1 (b,n1), dlogit2
    (b,n2), dF1 (b n1, C), dF2 (b n2, C)); a pair that is not needed is None and is not computed.  F is read once (for the
    logits), dF is a pure write; no atomics, every sum in a pinned order: the same inputs give the same bits."""
    return _conf_pool_layout_backward("pm", conf, w, F1, F2, g_pooled, g_conf, need_logits, need_F, False)


def conf_pool_pm_host(w, F1, F2):
    """conf_pool_pm on CPU tensors: the kernel's routines compiled for the host, in their summation order.  For checking the
    arithmetic where there is no GPU; no model path calls it."""
    return _conf_pool_layout("pm", w, F1, F2, True)


def conf_pool_pm_backward_host(conf, w, F1, F2, g_pooled, g_conf=None, need_logits=True, need_F=True):
    """conf_pool_pm_backward on CPU tensors; no model path calls it."""
    return _conf_pool_layout_backward("pm", conf, w, F1, F2, g_pooled, g_conf, need_logits, need_F, True)


N_ = N                         # (below, N is a layer's width)
NARROW_MAX_N = N.define("DCL_NARROW_MAX_N")         # the widest layer linear_narrow serves
NARROW_ROWS = N.define("DCL_NARROW_ROWS")           # the rows per chunk of its dW / db sums
TRAIN_HEADS_MODES = ("modules", "kernels")


def check_train_heads(value, what="train_heads"):
    if value not in TRAIN_HEADS_MODES:
        raise ValueError('%s must be "modules" or "kernels", got %r' % (what, value))
    return value


def _narrow_args(x, W, host, what):
    """x (M,K) fp32 with dense rows (a column block of a wider matrix stays a view), W (N,K) or (N,K,1...) -> M, K, N, x, pitch, W2d"""
    _same_side(host, what, x, W)
    assert x.dim() == 2 and W.dim() >= 2 and W.numel() == W.shape[0] * W.shape[1] and W.shape[1] == x.shape[1], \
        (tuple(x.shape), tuple(W.shape))
    x = x if x.dtype == torch.float32 else x.float()
    if x.shape[1] > 1 and x.stride(1) != 1 or (x.shape[0] > 1 and x.stride(0) < x.shape[1]):
        x = x.contiguous()
    M, K = x.shape
    N = W.shape[0]
    if not 1 <= N <= NARROW_MAX_N:
        raise ValueError("%s serves 1 <= N <= %d output columns, got N = %d" % (what, NARROW_MAX_N, N))
    return M, K, N, x, (x.stride(0) if M > 1 else K), N_.f32c(W).view(N, K)


def _linear_narrow(x, W, bias, host):
    what = "linear_narrow_host" if host else "linear_narrow"
    M, K, N, x, pitch, W = _narrow_args(x, W, host, what)
    _same_side(host, what, bias)
    bias = None if bias is None else N_.f32c(bias)
    assert bias is None or tuple(bias.shape) == (N,), tuple(bias.shape)
    y = torch.empty((M, N), dtype=torch.float32, device=x.device)
    N_.twin("dcl_linear_narrow_fwd", host, what, M, K, N, N_.ptr(x), pitch, N_.ptr(W), N_.ptr(bias), N_.ptr(y))
    return y


def _linear_narrow_backward(x, W, g, need_x, need_w, need_b, host):
    what = "linear_narrow_backward_host" if host else "linear_narrow_backward"
    M, K, N, x, pitch, W = _narrow_args(x, W, host, what)
    _same_side(host, what, g)
    assert need_x or need_w or need_b
    assert tuple(g.shape) == (M, N), "g: (M, N) = %s wanted, got %s" % ((M, N), tuple(g.shape))
    g = N_.f32c(g)
    dev = x.device
    # (an empty batch launches nothing: the sums are zero)
    new = (lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)) if M == 0 else \
        (lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev))
    dx, dW, db = new(M, K) if need_x else None, new(N, K) if need_w else None, new(N) if need_b else None
    scratch = ()
    if not host:
        ws, nbytes = None, 0
        if need_w or need_b:
            nbytes = N_.query("dcl_linear_narrow_bwd_ws_bytes", M, K, N)
            ws = torch.empty((max(nbytes, 4) // 4,), dtype=torch.float32, device=dev)
        scratch = (N_.ptr(ws), nbytes)
    N_.twin("dcl_linear_narrow_bwd", host, what, M, K, N, N_.ptr(x), pitch, N_.ptr(W), N_.ptr(g), N_.ptr(dx), N_.ptr(dW), N_.ptr(db),
            *scratch)
    return dx, dW, db


def linear_narrow(x, W, bias=None):
    """A per-point linear layer with 1 <= N <= NARROW_MAX_N output columns (dcl_linear_narrow_fwd; csrc/linear_narrow.hip):
    x (M,K) -- dense, or a column block of a wider matrix, served as it lies -- W (N,K) or (N,K,1...) as the convolution registers
    it, bias (N,) or None -> y (M,N) = x W^T + bias.  One launch, x read once, no transposed copy of W; the summation order
    include/dclnet_hip.h pins: any pitch and alignment give the same bits."""
    return _linear_narrow(x, W, bias, False)


def linear_narrow_backward(x, W, g, need_x=True, need_w=True, need_b=True):
    """Gradients of linear_narrow (dcl_linear_narrow_bwd): g (M,N) the upstream gradient -> (dx (M,K), dW (N,K), db (N,)); one that
    is not needed is None and is not computed.  x and g are read once, dx is a pure streaming write, the dW / db partials of
    NARROW_ROWS-row chunks are formed in the same pass and added in ascending order by a finish launch; no atomics: the same
    inputs give the same bits."""
    return _linear_narrow_backward(x, W, g, need_x, need_w, need_b, False)


def linear_narrow_host(x, W, bias=None):
    """linear_narrow on CPU tensors: the kernel's routines compiled for the host, in their summation order.  For checking the
    arithmetic where there is no GPU; no model path calls it."""
    return _linear_narrow(x, W, bias, True)


def linear_narrow_backward_host(x, W, g, need_x=True, need_w=True, need_b=True):
    """linear_narrow_backward on CPU tensors; no model path calls it."""
    return _linear_narrow_backward(x, W, g, need_x, need_w, need_b, True)


POSE_TRAIN_GRADS = ("rW0", "rb0", "rW1", "rb1", "rW2", "rb2", "tW0", "tb0", "tW1", "tb1", "tW2", "tb2")


def _pose_train_args(x, params, host, what):
    """x (b,d0), params = (rW0, rb0, rW1, rb1, rW2, rb2, tW0, ..., tb2) as the convolutions register them -> dims, fp32 contiguous
    tensors (a contiguous fp32 parameter is used where it lies)"""
    assert len(params) == 12, len(params)
    _same_side(host, what, x, *params)
    x = N_.f32c(x)
    params = [N_.f32c(p) for p in params]
    assert x.dim() == 2, tuple(x.shape)
    b, d0 = x.shape
    Ws = params[0::2]
    for Wm, bias in zip(Ws, params[1::2]):
        assert Wm.dim() >= 2 and Wm.numel() == Wm.shape[0] * Wm.shape[1] and tuple(bias.shape) == (Wm.shape[0],), \
            (tuple(Wm.shape), tuple(bias.shape))
    d1, d2, n_rot, n_trans = Ws[0].shape[0], Ws[1].shape[0], Ws[2].shape[0], Ws[5].shape[0]
    want = [(d1, d0), (d2, d1), (n_rot, d2), (d1, d0), (d2, d1), (n_trans, d2)]
    assert [tuple(Wm.shape[:2]) for Wm in Ws] == want, ([tuple(Wm.shape) for Wm in Ws], want)
    return (b, d0, d1, d2, n_rot, n_trans), x, params


def _pose_heads_train(x, params, host):
    what = "pose_heads_train_host" if host else "pose_heads_train"
    dims, x, params = _pose_train_args(x, params, host, what)
    b, d0, d1, d2, n_rot, n_trans = dims
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=x.device)            # noqa: E731
    h1, h2, o9, t3 = new(2, b, d1), new(2, b, d2), new(b, n_rot), new(b, n_trans)
    ptrs = [N_.ptr(t) for t in [x] + params + [h1, h2, o9, t3]]
    N_.twin("dcl_pose_heads_train_fwd", host, what, *dims, *ptrs)
    return o9, t3, h1, h2


def _pose_heads_train_backward(x, params, h1, h2, g_o9, g_t3, need_x, need_params, host):
    what = "pose_heads_train_backward_host" if host else "pose_heads_train_backward"
    dims, x, params = _pose_train_args(x, params, host, what)
    b, d0, d1, d2, n_rot, n_trans = dims
    _same_side(host, what, h1, h2, g_o9, g_t3)
    assert g_o9 is not None or g_t3 is not None
    assert tuple(h1.shape) == (2, b, d1) and tuple(h2.shape) == (2, b, d2), (tuple(h1.shape), tuple(h2.shape))
    assert g_o9 is None or tuple(g_o9.shape) == (b, n_rot), tuple(g_o9.shape)
    assert g_t3 is None or tuple(g_t3.shape) == (b, n_trans), tuple(g_t3.shape)
    if need_params is True or need_params is False:
        need_params = (bool(need_params),) * 12
    assert len(need_params) == 12 and (need_x or any(need_params))
    h1, h2 = N_.f32c(h1), N_.f32c(h2)
    g_o9, g_t3 = None if g_o9 is None else N_.f32c(g_o9), None if g_t3 is None else N_.f32c(g_t3)
    new = torch.zeros_like if b == 0 else torch.empty_like                                   # an empty batch launches nothing
    dx = new(x) if need_x else None
    grads = [new(p) if need else None for p, need in zip(params, need_params)]
    ins = [N_.ptr(t) for t in [x] + params[0:6:2] + params[6:12:2] + [h1, h2, g_o9, g_t3]]
    outs = [N_.ptr(dx)] + [N_.ptr(t) for t in grads]
    scratch = ()
    if not host:
        nbytes = N_.query("dcl_pose_heads_train_bwd_ws_bytes", *dims)
        ws = torch.empty((max(nbytes, 4) // 4,), dtype=torch.float32, device=x.device)
        scratch = (N_.ptr(ws), nbytes)
    N_.twin("dcl_pose_heads_train_bwd", host, what, *dims, *ins, *outs, *scratch)
    return dx, grads


def pose_heads_train(x, params):
    """Both pose heads on the pooled rows of a training step (dcl_pose_heads_train_fwd; csrc/pose_heads_grad.hip): x (b,d0),
    params = (rW0, rb0, rW1, rb1, rW2, rb2, tW0, tb0, tW1, tb1, tW2, tb2), the rotation then the translation head's weights
    (out, in[, 1]) and biases as registered -> (o9 (b,n_rot), t3 (b,n_trans), h1 (2,b,d1), h2 (2,b,d2)), the hidden activations
    for the backward.  Three launches shared by both heads, each weight matrix read once for all b rows; NOT the eval kernels'
    bits (ops.pose_heads: folded weights, other slice orders)."""
    return _pose_heads_train(x, params, False)


def pose_heads_train_backward(x, params, h1, h2, g_o9, g_t3, need_x=True, need_params=True):
    """Gradients of pose_heads_train (dcl_pose_heads_train_bwd): g_o9 (b,n_rot) / g_t3 (b,n_trans) the upstream gradients (None =
    zero, not both) -> (dx (b,d0) or None, [the twelve parameter gradients in POSE_TRAIN_GRADS order, shaped as their parameters,
    None where need_params -- a bool or twelve of them -- says so]).  At most six launches, the ReLU masks recomputed from h1 / h2,
    every sum in a pinned order: the same inputs give the same bits."""
    return _pose_heads_train_backward(x, params, h1, h2, g_o9, g_t3, need_x, need_params, False)


def pose_heads_train_host(x, params):
    """pose_heads_train on CPU tensors, in the kernels' summation orders; no model path calls it."""
    return _pose_heads_train(x, params, True)


def pose_heads_train_backward_host(x, params, h1, h2, g_o9, g_t3, need_x=True, need_params=True):
    """pose_heads_train_backward on CPU tensors; no model path calls it."""
    return _pose_heads_train_backward(x, params, h1, h2, g_o9, g_t3, need_x, need_params, True)


BN_ROWS = N.define("DCL_BN_ROWS")                   # the rows per chunk of the BatchNorm sums
TRAIN_NORM_MODES = ("modules", "fused")


def check_train_norm(value, what="train_norm"):
    if value not in TRAIN_NORM_MODES:
        raise ValueError('%s must be "modules" or "fused", got %r' % (what, value))
    return value


def _bn_relu_args(x, host, what, *vectors):
    _same_side(host, what, x, *vectors)
    assert x.dim() == 2, "%s: x must be (rows, C), got %s" % (what, tuple(x.shape))
    rows, c = int(x.shape[0]), int(x.shape[1])
    if rows == 1:
        raise ValueError("%s: expected more than 1 row per channel when training, got input size %s" % (what, tuple(x.shape)))
    for v in vectors:
        assert v is None or tuple(v.shape) == (c,), "%s: per-channel vectors hold C = %d floats, got %s" % (what, c, tuple(v.shape))
    return rows, c


def _bn_relu_ws(rows, c, dev):
    nbytes = N.query("dcl_bn_relu_ws_bytes", rows, c)
    return torch.empty(((nbytes + 7) // 8,), dtype=torch.float64, device=dev), nbytes


def _running_inplace(t, what):
    if t is not None and not (t.dtype == torch.float32 and t.is_contiguous()):
        raise ValueError("%s is updated in place: it must be a contiguous fp32 tensor" % what)


def _bn_relu(x, gamma, beta, running_mean, running_var, momentum, eps, relu, host):
    what = "bn_relu_host" if host else "bn_relu"
    rows, c = _bn_relu_args(x, host, what, gamma, beta, running_mean, running_var)
    assert (running_mean is None) == (running_var is None), "running_mean and running_var come as a pair"
    _running_inplace(running_mean, "running_mean"), _running_inplace(running_var, "running_var")
    x, gamma, beta = N.f32c(x), N.f32c(gamma), N.f32c(beta)
    z = torch.empty_like(x)
    mean = torch.empty((c,), dtype=torch.float32, device=x.device)
    invstd = torch.empty_like(mean)
    if rows == 0:
        return z, mean.zero_(), invstd.zero_()
    scratch = ()
    if not host:
        ws, nbytes = _bn_relu_ws(rows, c, x.device)
        scratch = (N.ptr(ws), nbytes)
    N.twin("dcl_bn_relu_fwd", host, what, rows, c, N.ptr(x), N.ptr(gamma), N.ptr(beta), float(eps), float(momentum),
           N.ptr(running_mean), N.ptr(running_var), N.ptr(mean), N.ptr(invstd), N.ptr(z), int(bool(relu)), *scratch)
    return z, mean, invstd


def _bn_relu_backward(x, gamma, beta, mean, invstd, g, relu, need_x, need_affine, out, host):
    what = "bn_relu_backward_host" if host else "bn_relu_backward"
    rows, c = _bn_relu_args(x, host, what, gamma, beta, mean, invstd)
    _same_side(host, what, g, out)
    assert need_x or need_affine
    assert tuple(g.shape) == (rows, c), "g: %s wanted, got %s" % ((rows, c), tuple(g.shape))
    x, gamma, beta, mean, invstd, g = (N.f32c(t) for t in (x, gamma, beta, mean, invstd, g))
    dx = None
    if need_x:
        if out is not None:
            assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (rows, c), "out: contiguous fp32 (rows, C)"
            dx = out
        else:
            dx = torch.empty_like(x)
    dgamma, dbeta = (torch.empty_like(gamma), torch.empty_like(gamma)) if need_affine else (None, None)
    if rows == 0:
        return dx, None if dgamma is None else dgamma.zero_(), None if dbeta is None else dbeta.zero_()
    scratch = ()
    if not host:
        ws, nbytes = _bn_relu_ws(rows, c, x.device)
        scratch = (N.ptr(ws), nbytes)
    N.twin("dcl_bn_relu_bwd", host, what, rows, c, N.ptr(x), N.ptr(gamma), N.ptr(beta), N.ptr(mean), N.ptr(invstd), N.ptr(g),
           int(bool(relu)), N.ptr(dx), N.ptr(dgamma), N.ptr(dbeta), *scratch)
    return dx, dgamma, dbeta


def bn_relu(x, gamma, beta, running_mean=None, running_var=None, momentum=0.1, eps=1e-5, relu=True):
    """Train-mode BatchNorm1d + ReLU on a (rows, C) row-major matrix (dcl_bn_relu_fwd; csrc/bn_relu.hip): batch statistics in
    float64 in the summation order include/dclnet_hip.h pins, mean and invstd rounded to fp32 once, z = relu((x - mean) invstd
    gamma + beta) (relu=False: without the ReLU) -> (z, mean (C,), invstd (C,)).  running_mean / running_var, when given, are
    updated IN PLACE by the same launches with the unbiased variance, as nn.BatchNorm1d does; nothing is read back.  rows >= 2
    (0 rows: nothing is launched); a non-contiguous x is copied first."""
    return _bn_relu(x, gamma, beta, running_mean, running_var, momentum, eps, relu, False)


def bn_relu_backward(x, gamma, beta, mean, invstd, g, relu=True, need_x=True, need_affine=True, out=None):
    """Gradients of bn_relu (dcl_bn_relu_bwd): mean, invstd as bn_relu returned them, g (rows, C) the upstream gradient of z ->
    (dx, dgamma, dbeta); what is not needed is None and is not computed.  The ReLU mask is recomputed from x by the forward's
    expression (y and z are not kept); the two per-channel sums are float64 in the forward's order.  out: where dx goes -- a
    contiguous fp32 (rows, C) tensor, which may be g itself."""
    return _bn_relu_backward(x, gamma, beta, mean, invstd, g, relu, need_x, need_affine, out, False)


def bn_relu_host(x, gamma, beta, running_mean=None, running_var=None, momentum=0.1, eps=1e-5, relu=True):
    """bn_relu on CPU tensors: the kernels' routines compiled for the host, in their summation order.  For checking the
    arithmetic where there is no GPU; no model path calls it."""
    return _bn_relu(x, gamma, beta, running_mean, running_var, momentum, eps, relu, True)


def bn_relu_backward_host(x, gamma, beta, mean, invstd, g, relu=True, need_x=True, need_affine=True, out=None):
    """bn_relu_backward on CPU tensors; no model path calls it."""
    return _bn_relu_backward(x, gamma, beta, mean, invstd, g, relu, need_x, need_affine, out, True)


OPTIM_CHUNK = N.define("DCL_OPTIM_CHUNK")
OPTIM_TENSOR_BYTES = 48        # sizeof(dclOptimTensor): four pointers, int64 numel, float step_size, float bc2_sqrt


def _optim_tables(table, chunk_tensor, chunk_begin):
    N.need_cuda(table, chunk_tensor, chunk_begin)
    assert table.dtype == torch.uint8 and table.dim() == 1 and table.is_contiguous() and table.numel() % OPTIM_TENSOR_BYTES == 0
    assert chunk_tensor.dtype == torch.int32 and chunk_begin.dtype == torch.int64
    assert chunk_tensor.dim() == 1 and chunk_tensor.shape == chunk_begin.shape
    assert chunk_tensor.is_contiguous() and chunk_begin.is_contiguous()
    assert table.data_ptr() % 8 == 0
    return table.numel() // OPTIM_TENSOR_BYTES, chunk_tensor.numel()


def grad_sqnorm(table, chunk_tensor, chunk_begin):
    """The 2-norm of all listed gradients together, in float64 (csrc/optim.hip; include/dclnet_hip.h at dcl_grad_sqnorm):
    table = the packed dclOptimTensor rows (uint8, OPTIM_TENSOR_BYTES each), chunk_tensor i32 / chunk_begin i64 = the chunk
    table -> (sq_per_tensor (n_tensors,) f64, norm (1,) f64), both on the device.  Deterministic, no host read-back."""
    n_tensors, n_chunks = _optim_tables(table, chunk_tensor, chunk_begin)
    dev = table.device
    sq = torch.zeros(n_tensors, dtype=torch.float64, device=dev)
    norm = torch.zeros(1, dtype=torch.float64, device=dev)
    partials = torch.empty(n_chunks, dtype=torch.float64, device=dev)
    N.check(N.lib().dcl_grad_sqnorm(n_tensors, N.ptr(table), n_chunks, N.ptr(chunk_tensor), N.ptr(chunk_begin),
                                    N.ptr(partials), N.ptr(sq), N.ptr(norm), N.stream()), "grad_sqnorm")
    return sq, norm


def adam_step(table, chunk_tensor, chunk_begin, grad_scale, beta1, beta2, eps):
    """torch.optim.Adam's update of every listed tensor in one launch, the gradients multiplied by grad_scale on the way in
    (dcl_adam_step; the header states the order of operations).  Updates param, exp_avg and exp_avg_sq in place THROUGH RAW
    POINTERS: the caller moves the tensors' version counters (dcl.optim.Adam does)."""
    n_tensors, n_chunks = _optim_tables(table, chunk_tensor, chunk_begin)
    N.check(N.lib().dcl_adam_step(n_tensors, N.ptr(table), n_chunks, N.ptr(chunk_tensor), N.ptr(chunk_begin),
                                  grad_scale, beta1, beta2, eps, N.stream()),
            "adam_step")


def adam_step_dev(table, chunk_tensor, chunk_begin, grad_scale, beta1, beta2, eps):
    """adam_step with the clip factor read from device memory when the kernel runs (dcl_adam_step_dev): grad_scale = a
    one-element fp32 CUDA tensor, in [0, 1] by its producer's contract (ops.autoclip_observe's fp32 slot).  Nothing is read
    back; equal factor bits give adam_step's bits."""
    n_tensors, n_chunks = _optim_tables(table, chunk_tensor, chunk_begin)
    N.need_cuda(grad_scale)
    assert grad_scale.dtype == torch.float32 and grad_scale.numel() == 1 and grad_scale.device == table.device
    N.check(N.lib().dcl_adam_step_dev(n_tensors, N.ptr(table), n_chunks, N.ptr(chunk_tensor), N.ptr(chunk_begin),
                                      N.ptr(grad_scale), beta1, beta2, eps, N.stream()),
            "adam_step_dev")


AUTOCLIP_OUT_DOUBLES = N.define("DCL_AUTOCLIP_OUT_BYTES") // 8                # {norm, clip_value, scale} and the fp32 slot
AUTOCLIP_SCALE_F32_INDEX = N.define("DCL_AUTOCLIP_SCALE_F32_OFFSET") // 4     # where (float)scale lies in out.view(torch.float32)


def _autoclip_observe(n, sorted_src, sorted_dst, arrival, norm, percentile, out, host):
    n = int(n)
    ts = (sorted_src, sorted_dst, arrival, norm, out)
    if host:
        assert not any(t.is_cuda for t in ts)
    else:
        N.need_cuda(*ts)
        assert all(t.device == out.device for t in ts)
    assert all(t.dtype == torch.float64 and t.dim() == 1 and t.is_contiguous() for t in ts)
    assert n >= 0 and sorted_src.numel() >= n and sorted_dst.numel() >= n + 1 and arrival.numel() >= n + 1
    assert norm.numel() == 1 and out.numel() == AUTOCLIP_OUT_DOUBLES
    N.twin("dcl_autoclip_observe", host, "autoclip_observe_host" if host else "autoclip_observe", n, N.ptr(sorted_src),
           N.ptr(sorted_dst), N.ptr(arrival), N.ptr(norm), float(percentile), N.ptr(out))
    return out


def autoclip_observe(n, sorted_src, sorted_dst, arrival, norm, percentile, out):
    """AutoClip's host arithmetic on the device (dcl_autoclip_observe, two launches, no read-back): inserts norm (1,) f64 into
    the n ascending norms of sorted_src -> sorted_dst[:n + 1] (NaN last, the new one behind equal ones), writes arrival[n],
    and out (AUTOCLIP_OUT_DOUBLES,) f64 = {norm, np.percentile(history, percentile), min(1.0, clip / (norm + 1e-6))} with the
    factor rounded once to fp32 at out.view(torch.float32)[AUTOCLIP_SCALE_F32_INDEX].  n is the HOST's count of held norms."""
    return _autoclip_observe(n, sorted_src, sorted_dst, arrival, norm, percentile, out, False)


def autoclip_observe_host(n, sorted_src, sorted_dst, arrival, norm, percentile, out):
    """the host twin of autoclip_observe (dcl_autoclip_observe_host, plain C++, no GPU call) on CPU tensors"""
    return _autoclip_observe(n, sorted_src, sorted_dst, arrival, norm, percentile, out, True)


def three_interpolate(features, idx, weight):
    N.need_cuda(features, idx, weight)
    assert features.is_contiguous() and idx.is_contiguous() and weight.is_contiguous()
    B, c, m = features.shape
    n = idx.shape[1]
    out = torch.empty((B, c, n), dtype=torch.float32, device=features.device)
    N.check(N.lib().dcl_three_interpolate(B, c, m, n, N.ptr(features), N.ptr(idx), N.ptr(weight), N.ptr(out),
                                          N.stream()), "three_interpolate")
    return out


# ------------------------------------------------------------------------------------ dense path
def _ld(t):
    assert t.dim() == 2 and t.stride(1) == 1
    return t.stride(0) if t.shape[0] > 1 else t.shape[1]


ATTENTION_SPLIT = True        # large attention calls: P.V on the bf16 matrix pipe at fp32-sized errors (False: fp32 MFMA everywhere)


def attention_planes(b, nq, nk, concurrent=1, device=None):
    """scratch for the K / V pieces of a cross_attention call of this size that takes the split-bf16 kernel: (planes, whole) --
    planes None = the call keeps the fp32 kernel; whole = ALL b crops take the split kernel, i.e. the caller may have V1 written
    as pieces straight into `planes` by the GEMM that makes it (linear_split_vpieces) and pass V1 = None."""
    if not ATTENTION_SPLIT:
        return None, False
    lib = N.lib()
    pb = int(lib.dcl_cross_attention_planes_bytes(int(b), int(nq), int(nk), int(concurrent)))
    if not pb:
        return None, False
    whole = int(lib.dcl_cross_attention_split_crops(int(b), int(nq), int(nk), int(concurrent))) == int(b)
    return torch.empty(pb, dtype=torch.uint8, device=device if device is not None else torch.device("cuda")), whole


def cross_attention(b, Q, K, V1, O1, V2=None, O2=None, concurrent=1, planes=None):
    """One direction of the correspondence attention on POINT-major 2-D operands (row = point):
    Q (b*nq, 64), K (b*nk, 64), V1 (b*nk, dv1) -> O1 (b*nq, dv1) [, V2 -> O2].  Operands may be
    column blocks of wider buffers (row stride honoured).  The PRODUCT library carries DCL-Net's own channel split only,
    dv1 = 256 with dv2 = 64 (anything else: DCL_EINVAL at run time -- include/dclnet_hip.h says so at dcl_cross_attention);
    the general-shape kernels (dv1, dv2 multiples of 32) live in the diagnostic library.
    concurrent = 2: another launch of the same size runs side by side on a second stream (the other direction of a forward) --
    a hint for the launcher's choice of workgroup shape (dcl_cross_attention_ws2)."""
    N.need_cuda(Q, K, V1, O1, V2, O2)
    nq, nk = Q.shape[0] // b, K.shape[0] // b
    assert Q.shape[1] == 64 and K.shape[1] == 64 and O1.shape[0] == Q.shape[0]
    assert V1 is not None or planes is not None, "V1 = None: its pieces are expected in `planes` (attention_planes, linear_split_vpieces)"
    assert V1 is None or V1.shape[0] == K.shape[0]
    dv1 = 256 if V1 is None else V1.shape[1]
    dv2 = 0 if V2 is None else V2.shape[1]
    ev = None
    if PROFILE_EVENTS is not None:
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
    scratch = None
    if dv1 == 256 and dv2 == 64:          # key-split partial records (small launches, badly quantised large ones)
        need = N.query("dcl_cross_attention_scratch_floats", b, nq)
        if need:
            scratch = torch.empty(need, dtype=torch.float32, device=Q.device)
    if planes is None and dv1 == 256 and dv2 == 64:    # large calls: scratch for the K / V pieces of the split-bf16 kernel (csrc/dense.hip)
        planes, _ = attention_planes(b, nq, nk, concurrent, Q.device)
    N.check(N.lib().dcl_cross_attention_ws3(b, nq, nk, N.ptr(Q), _ld(Q), N.ptr(K), _ld(K), N.ptr(V1), dv1, 256 if V1 is None else _ld(V1),
                                            N.ptr(O1), _ld(O1), N.ptr(V2), dv2, 0 if V2 is None else _ld(V2), N.ptr(O2),
                                            0 if O2 is None else _ld(O2), N.ptr(scratch),
                                            0 if scratch is None else scratch.numel(), int(concurrent), N.ptr(planes),
                                            0 if planes is None else planes.numel(), N.stream()),
            "cross_attention")
    if ev is not None:
        ev[1].record()
        PROFILE_EVENTS.append(("cross_attention", ev[0], ev[1]))
    return O1, O2


def cross_attention_backward(b, Q, K, V1, V2, O1, O2, dO1, dO2=None):
    """Gradients of one cross_attention call without the attention map (csrc/attention_bwd.hip; include/dclnet_hip.h at
    dcl_cross_attention_bwd): the 2-D point-major operands cross_attention took and returned plus dO1 (b*nq, 256), dO2 (b*nq, 64)
    or None (= zeros) -> (dQ, dK, dV1, dV2), new contiguous tensors.  Row strides are honoured.  dK and dV2 are separate
    even where K and V2 are one tensor (the caller adds them).  Deterministic: the same inputs give the same bits."""
    N.need_cuda(Q, K, V1, V2, O1, O2, dO1, dO2)
    nq, nk = Q.shape[0] // b, K.shape[0] // b
    assert Q.shape == (b * nq, 64) and K.shape == (b * nk, 64)
    assert V1.shape[0] == b * nk and V2.shape[0] == b * nk and O1.shape == (b * nq, V1.shape[1]) and O2.shape == (b * nq, V2.shape[1])
    assert dO1.shape == O1.shape and (dO2 is None or dO2.shape == O2.shape)
    assert all(t is None or t.dtype == torch.float32 for t in (Q, K, V1, V2, O1, O2, dO1, dO2))
    dev = Q.device
    dQ, dK = torch.empty((b * nq, 64), dtype=torch.float32, device=dev), torch.empty((b * nk, 64), dtype=torch.float32, device=dev)
    dV1, dV2 = torch.empty(V1.shape, dtype=torch.float32, device=dev), torch.empty(V2.shape, dtype=torch.float32, device=dev)
    return cross_attention_backward_into(b, Q, K, V1, V2, O1, O2, dO1, dO2, dQ, dK, dV1, dV2)


def cross_attention_backward_into(b, Q, K, V1, V2, O1, O2, dO1, dO2, dQ, dK, dV1, dV2):
    """cross_attention_backward writing into the caller's dQ, dK, dV1, dV2 (which may be column blocks of wider buffers)."""
    N.need_cuda(Q, K, V1, V2, O1, O2, dO1, dO2, dQ, dK, dV1, dV2)
    nq, nk = Q.shape[0] // b, K.shape[0] // b
    nbytes = N.query("dcl_cross_attention_bwd_ws_bytes", int(b), nq, nk)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=Q.device)
    N.check(N.lib().dcl_cross_attention_bwd(int(b), nq, nk, N.ptr(Q), _ld(Q), N.ptr(K), _ld(K), N.ptr(V1), V1.shape[1], _ld(V1),
                                            N.ptr(V2), V2.shape[1], _ld(V2), N.ptr(O1), _ld(O1), N.ptr(O2), _ld(O2),
                                            N.ptr(dO1), _ld(dO1), N.ptr(dO2), 0 if dO2 is None else _ld(dO2),
                                            N.ptr(dQ), _ld(dQ), N.ptr(dK), _ld(dK), N.ptr(dV1), _ld(dV1), N.ptr(dV2), _ld(dV2),
                                            N.ptr(ws), nbytes, N.stream()), "cross_attention_bwd")
    return dQ, dK, dV1, dV2


def conf_pool(b, logit1, logit2, F1, F2, affine=None, finish=True):
    """Confidence pooling: logits (b*n1,)/(b*n2,), F1 (b*n1,C), F2 (b*n2,C) point-major ->
    conf (b,n1+n2), pooled1 (b,C), pooled2 (b,C), wsum (b,2).
    affine = (s1, t1, s2, t2), each (C,): returns (conf, ((s1*P1 + t1*wsum1) + s2*P2) + t2*wsum2) instead -- the pooled
    feature behind trailing BatchNorms that were not applied to F1 / F2 -- finished in one launch; finish=False: (conf, parts)
    with the slice partials for pose_heads_parts, which finishes them inside its first launch."""
    N.need_cuda(logit1, logit2, F1, F2)
    n1, n2 = F1.shape[0] // b, F2.shape[0] // b
    c = F1.shape[1]
    assert logit1.is_contiguous() and logit2.is_contiguous() and logit1.numel() == b * n1 and logit2.numel() == b * n2
    dev = F1.device
    # enough (crop, channel-chunk, slice) blocks to fill 256 CUs several times over
    nslices = max(1, min(64, 2048 // max(1, b * ((c + 255) // 256))))
    conf = torch.empty((b, n1 + n2), dtype=torch.float32, device=dev)
    w = torch.empty((b, n1 + n2), dtype=torch.float32, device=dev)
    part1 = torch.empty((b, nslices, c), dtype=torch.float32, device=dev)
    part2 = torch.empty((b, nslices, c), dtype=torch.float32, device=dev)
    ws = torch.empty((b, 2), dtype=torch.float32, device=dev)
    N.check(N.lib().dcl_conf_pool(b, c, n1, n2, N.ptr(logit1), N.ptr(logit2), N.ptr(F1), _ld(F1), N.ptr(F2), _ld(F2),
                                  N.ptr(conf), N.ptr(w), nslices, N.ptr(part1), N.ptr(part2), N.ptr(ws), N.stream()),
            "conf_pool")
    if affine is not None:
        s1, t1, s2, t2 = affine
        N.need_cuda(s1, t1, s2, t2)
        assert all(t.is_contiguous() and t.numel() == c and t.dtype == torch.float32 for t in affine)
        if not finish:                                 # the caller folds the finish into its next launch (pose_heads_parts)
            return conf, (nslices, part1, part2, ws)
        out = torch.empty((b, c), dtype=torch.float32, device=dev)
        N.check(N.lib().dcl_pool_finish(b, c, nslices, N.ptr(part1), N.ptr(part2), N.ptr(ws), N.ptr(s1), N.ptr(t1),
                                        N.ptr(s2), N.ptr(t2), N.ptr(out), N.stream()), "pool_finish")
        return conf, out
    return conf, part1.sum(dim=1), part2.sum(dim=1), ws


def affine3_relu(xyz, W3, term):
    """relu(term + xyz @ W3): xyz (rows,3), W3 (3,c), term (rows,c) -> (rows,c), one pass (csrc/dense.hip: k_affine3_relu) -- the
    xyz part of the refiner's first shared layer (models/refiner.py:78-80)."""
    N.need_cuda(xyz, W3, term)
    assert xyz.is_contiguous() and W3.is_contiguous() and term.is_contiguous() and xyz.shape[1] == 3
    rows, c = term.shape
    assert tuple(W3.shape) == (3, c) and xyz.shape[0] == rows
    out = torch.empty_like(term)
    N.check(N.lib().dcl_affine3_relu(rows, int(c), N.ptr(xyz), N.ptr(W3), N.ptr(term), N.ptr(out), N.stream()),
            "affine3_relu")
    return out


def pose_heads(pooled, rot_layers, trans_layers, with_rotation=False):
    """regressor_rot / regressor_trans on the pooled (b,1024) feature for a handful of crops: both 3-layer heads in two
    launches.  *_layers: [(W1t, b1), (W2t, b2), (W3t, b3)] with (in, out) matrices -> (o9 (b,9), trans (b,3)); with_rotation:
    also R (b,3,3) = ortho9d_to_matrix(o9), formed by the second launch."""
    N.need_cuda(pooled)
    pooled = pooled.contiguous()
    b, dev = pooled.shape[0], pooled.device
    assert pooled.shape[1] == 1024 and tuple(rot_layers[0][0].shape) == (1024, 512) and tuple(rot_layers[2][0].shape) == (128, 9)
    assert tuple(trans_layers[1][0].shape) == (512, 128) and tuple(trans_layers[2][0].shape) == (128, 3)
    flat = lambda layers: _ptr_array([t for pair in layers for t in pair])                    # noqa: E731
    assert all(t.is_contiguous() and t.dtype == torch.float32 for layers in (rot_layers, trans_layers) for p in layers for t in p)
    h1 = torch.empty((2, b, 512), dtype=torch.float32, device=dev)
    o9 = torch.empty((b, 9), dtype=torch.float32, device=dev)
    trans = torch.empty((b, 3), dtype=torch.float32, device=dev)
    R = torch.empty((b, 3, 3), dtype=torch.float32, device=dev) if with_rotation else None
    N.check(N.lib().dcl_pose_heads(b, N.ptr(pooled), flat(rot_layers), flat(trans_layers), N.ptr(h1), N.ptr(o9), N.ptr(trans),
                                   N.ptr(R), N.stream()), "pose_heads")
    return (o9, trans, R) if with_rotation else (o9, trans)


def pose_heads_parts(parts, affine, rot_layers, trans_layers, with_rotation=False):
    """pose_heads on the pooled feature still in parts (conf_pool(..., affine, finish=False)): the pooling's finish runs inside
    the heads' first launch -- a launch less for a handful of crops, bit-identical to conf_pool(finish=True) + pose_heads."""
    nslices, part1, part2, ws = parts
    s1, t1, s2, t2 = affine
    b, dev = part1.shape[0], part1.device
    assert part1.shape[2] == 1024 and tuple(rot_layers[0][0].shape) == (1024, 512) and tuple(rot_layers[2][0].shape) == (128, 9)
    assert tuple(trans_layers[1][0].shape) == (512, 128) and tuple(trans_layers[2][0].shape) == (128, 3)
    flat = lambda layers: _ptr_array([t for pair in layers for t in pair])                    # noqa: E731
    assert all(t.is_contiguous() and t.dtype == torch.float32 for layers in (rot_layers, trans_layers) for p in layers for t in p)
    h1 = torch.empty((2, b, 512), dtype=torch.float32, device=dev)
    o9 = torch.empty((b, 9), dtype=torch.float32, device=dev)
    trans = torch.empty((b, 3), dtype=torch.float32, device=dev)
    R = torch.empty((b, 3, 3), dtype=torch.float32, device=dev) if with_rotation else None
    N.check(N.lib().dcl_pose_heads_parts(b, int(nslices), N.ptr(part1), N.ptr(part2), N.ptr(ws), N.ptr(s1), N.ptr(t1), N.ptr(s2),
                                         N.ptr(t2), flat(rot_layers), flat(trans_layers), N.ptr(h1), N.ptr(o9), N.ptr(trans),
                                         N.ptr(R), N.stream()), "pose_heads_parts")
    return (o9, trans, R) if with_rotation else (o9, trans)


def _refine_first(pts, R, t, W3, term, host):
    what = "refine_first_host" if host else "refine_first"
    b, n, _ = _rigid_args(pts, R, t, True, host, what)
    _same_side(host, what, W3, term)
    assert term.dim() == 2 and term.shape[0] == b * n, tuple(term.shape)
    c = term.shape[1]
    if c % 4:
        raise ValueError("%s needs c %% 4 == 0 (16-byte groups of channels), got c = %d" % (what, c))
    _f32_like(term, (b * n, c), "term")
    _f32_like(W3, (3, c), "W3")
    out = torch.empty_like(term)
    N.twin("dcl_refine_first", host, what, b, n, c, N.ptr(pts), N.ptr(R), N.ptr(t), N.ptr(W3), N.ptr(term), N.ptr(out))
    return out


def refine_first(pts, R, t, W3, term):
    """relu(term + cur @ W3) with cur = R^T (p - t) formed on the way and never stored (csrc/dense.hip: k_refine_first): pts
    (b,n,3) observed points, R (b,3,3) / t (b,3) the crops' current pose ON THE DEVICE, W3 (3,c), term (b*n,c) -> (b*n,c), one
    launch.  Bit for bit affine3_relu(rigid_points(pts, R, t, inverse=True).view(b*n, 3), W3, term): the first shared layer of
    the refine loop's device form (models/refiner.py: refine_loop(compose="device")).  c % 4 == 0 (ValueError otherwise)."""
    return _refine_first(pts, R, t, W3, term, False)


def refine_first_host(pts, R, t, W3, term):
    """refine_first on CPU tensors (the kernel's routines compiled for the host).  For checking the arithmetic where there is
    no GPU; no model path calls it."""
    return _refine_first(pts, R, t, W3, term, True)


def pose_compose_host(R, t, dR, dt):
    """The pose composition refine_heads carries as its epilogue, on CPU tensors (the kernel's routine compiled for the host):
    R (b,3,3), t (b,3), dR (b,3,3), dt (b,3) -> (R dR, R dt + t), every dot product as fmaf(R_i2, d_2, fmaf(R_i1, d_1, R_i0 * d_0))
    (include/dclnet_hip.h).  No model path calls it."""
    _same_side(True, "pose_compose_host", R, t, dR, dt)
    assert R.dim() == 3, tuple(R.shape)
    b = R.shape[0]
    _f32_like(R, (b, 3, 3), "R")
    _f32_like(t, (b, 3), "t")
    _f32_like(dR, (b, 3, 3), "dR")
    _f32_like(dt, (b, 3), "dt")
    R_out, t_out = torch.empty_like(R), torch.empty_like(t)
    N.check(N.lib().dcl_pose_compose_host(b, N.ptr(R), N.ptr(t), N.ptr(dR), N.ptr(dt), N.ptr(R_out), N.ptr(t_out)),
            "pose_compose_host")
    return R_out, t_out


def refine_heads(part, T, rot_layers, trans_layers, R_in, t_in, R_out, t_out):
    """pose_heads on the pooled feature still as linear_pool's tile partials, with the pose composition as its epilogue
    (dcl_refine_heads, two launches): part (b*T, 1024), crop i's pooled feature = its T partials added in one ascending chain
    from tile 0 by the first launch; the second launch WRITES R_out (b,3,3) = R_in dR and t_out (b,3) = R_in dt + t_in (views of
    the loop's pose arrays; they must not overlap R_in / t_in, which are left as they are).  -> (o9 (b,9), dt (b,3), dR (b,3,3)),
    the bits pose_heads(x, ..., with_rotation=True) gives.  b <= 65535 (ValueError otherwise)."""
    N.need_cuda(part, R_in, t_in, R_out, t_out)
    T = int(T)
    if T < 1 or part.dim() != 2 or part.shape[0] % T:
        raise ValueError("refine_heads needs part (b*T, 1024) with T >= 1, got %s for T = %d" % (tuple(part.shape), T))
    b, dev = part.shape[0] // T, part.device
    if b > 65535:
        raise ValueError("refine_heads needs b <= 65535 crops (one grid row per crop), got b = %d" % b)
    _f32_like(part, (b * T, 1024), "part")
    assert tuple(rot_layers[0][0].shape) == (1024, 512) and tuple(rot_layers[2][0].shape) == (128, 9)
    assert tuple(trans_layers[1][0].shape) == (512, 128) and tuple(trans_layers[2][0].shape) == (128, 3)
    flat = lambda layers: _ptr_array([t for pair in layers for t in pair])                    # noqa: E731
    assert all(t.is_contiguous() and t.dtype == torch.float32 for layers in (rot_layers, trans_layers) for p in layers for t in p)
    for t, shape, what in ((R_in, (b, 3, 3), "R_in"), (t_in, (b, 3), "t_in"), (R_out, (b, 3, 3), "R_out"), (t_out, (b, 3), "t_out")):
        _f32_like(t, shape, what)
    h1 = torch.empty((2, b, 512), dtype=torch.float32, device=dev)
    o9 = torch.empty((b, 9), dtype=torch.float32, device=dev)
    dt = torch.empty((b, 3), dtype=torch.float32, device=dev)
    dR = torch.empty((b, 3, 3), dtype=torch.float32, device=dev)
    N.check(N.lib().dcl_refine_heads(b, T, N.ptr(part), flat(rot_layers), flat(trans_layers), N.ptr(h1), N.ptr(R_in), N.ptr(t_in),
                                     N.ptr(R_out), N.ptr(t_out), N.ptr(o9), N.ptr(dt), N.ptr(dR), N.stream()), "refine_heads")
    return o9, dt, dR


VENDOR_GEMM = False           # tools / tests only: True sends linear() to the vendor library whatever the shape (A/B runs)


def linear(x, Wt, bias=None, relu=False, out=None):
    """One per-point linear layer (Conv1d k=1 / 1x1x1 Conv3d + folded BN of the reference's MLP stacks): act(x @ Wt + bias).
    x (M,K), Wt (K,N), out (M,N) are row-major 2-D tensors whose rows may be strided (column blocks of wider buffers):
    `out=buf[:, 256:512]` is written in place, no copy.  Runs on the library's OWN fp32 MFMA GEMM core (linear_dma,
    csrc/linear_dma.hip) -- every layer shape of the forward does; a shape that core does not take (K no multiple of 32,
    operands not 16-byte aligned) goes to the vendor library (linear_lt).  A layer whose weight has been PREPARED
    (prepare_linear: the Network's and the Refiner's folded weights are) runs its big launches on the split-bf16 core
    (linear_split, csrc/linear_split.hip: fp32-sized errors at 1.5x the fp32 MFMA's rate)."""
    if not VENDOR_GEMM and x.is_cuda and Wt.is_cuda and x.dim() == 2 and Wt.dim() == 2:
        sw = prepared_linear(Wt, x)
        if sw is not None:
            return linear_split(x, sw, bias, relu, out)
        if linear_dma_ok(x, Wt):
            return linear_dma(x, Wt, bias, relu, out)
    return linear_lt(x, Wt, bias, relu, out)


def _pitch(t):
    """row pitch of a 2-D tensor in elements (a single row has none of its own: at least its width)"""
    return int(t.stride(0)) if t.shape[0] > 1 else max(int(t.stride(0)), int(t.shape[1]))


def _layer_io(x, K, n, bias, out, dense=()):
    """The operand checks of a (M, K) -> (M, n) layer with linear()'s conventions (dense: further 2-D operands whose rows must be
    dense).  Returns out, allocated if None."""
    assert x.dim() == 2 and x.shape[1] == K and x.dtype == torch.float32
    M = x.shape[0]
    if out is None:
        out = torch.empty((M, n), dtype=torch.float32, device=x.device)
    assert out.shape == (M, n) and out.dtype == torch.float32 and out.is_cuda
    for t in (x,) + dense + (out,):
        assert t.stride(1) == 1 or t.shape[1] == 1, "rows must be dense"
    if bias is not None:
        assert bias.is_cuda and bias.dtype == torch.float32 and bias.numel() == n and bias.is_contiguous()
    return out


def _linear_fp32(x, Wt, bias, relu, out, vendor):
    """linear_lt / linear_dma: the same operands, one entry point each"""
    N.need_cuda(x, Wt)
    assert Wt.dim() == 2 and Wt.dtype == torch.float32
    K, n = Wt.shape
    out = _layer_io(x, K, n, bias, out, dense=(Wt,))
    M = x.shape[0]
    args = (N.ptr(x), _pitch(x), N.ptr(Wt), _pitch(Wt), N.ptr(bias), N.ptr(out), _pitch(out),
            int(M), int(n), int(K), int(bool(relu)))
    if vendor:
        N.check(N.lib().dcl_linear_fwd(*args, None, 0, N.stream()), "linear_fwd")
    else:
        N.check(N.lib().dcl_linear_dma_fwd(*args, N.stream()), "linear_dma_fwd")
    return out


def linear_lt(x, Wt, bias=None, relu=False, out=None):
    """linear() as a vendor-library GEMM (hipBLASLt, bias / ReLU epilogue) called through the C-ABI (dcl_linear_fwd): only
    algorithms that ask for NO workspace are ever taken (csrc/linear.cpp: two workspace-exchanging stream-K kernels side by
    side hang the GPU); the call fails when the library has none for the shape."""
    return _linear_fp32(x, Wt, bias, relu, out, vendor=True)


def linear_dma_ok(x, Wt):
    """can linear_dma take this layer?  (K in whole 32-chunks, 16-byte aligned operands and pitches: csrc/linear_dma.hip)"""
    K, n = Wt.shape
    pw = int(Wt.stride(0)) if K > 1 else n
    px = int(x.stride(0)) if x.shape[0] > 1 else K
    return (K >= 32 and K % 32 == 0 and px % 4 == 0 and pw % 4 == 0 and x.data_ptr() % 16 == 0 and Wt.data_ptr() % 16 == 0 and
            pw >= (n + 3) // 4 * 4)


def linear_dma(x, Wt, bias=None, relu=False, out=None):
    """linear() on the library's OWN fp32 MFMA GEMM core (csrc/linear_dma.hip; no vendor library): act(x @ Wt + bias), same
    conventions -- x (M,K), Wt (K,N), out (M,N) row-major with free row pitches."""
    return _linear_fp32(x, Wt, bias, relu, out, vendor=False)


GEMM_SPLIT = True              # big launches of prepared layers run on the split-bf16 core (False: the fp32-MFMA core everywhere)
SPLIT_MIN_TILES = 192          # ... from this many 256 x 128 tiles on (fewer cannot fill the chip: the fp32 core's smaller tiles win)
_PREPARED = {}                 # id(Wt) -> (weakref to Wt, SplitWeight)


def prepare_linear(Wt):
    """Prepare a layer's (K, N) weight for the split-bf16 GEMM core: its three bf16 pieces in tile order, kept beside the weight
    for as long as the weight tensor lives.  The weight must not be modified in place afterwards (the models' folded weights are
    rebuilt, never modified).  Layers of at most 64 output columns or with K no multiple of 16 stay on the fp32 core."""
    K, n = Wt.shape
    if not Wt.is_cuda or n <= 64 or K % 16 or K < 16:
        return None
    ent = _PREPARED.get(id(Wt))
    if ent is not None and ent[0]() is Wt:
        return ent[1]
    sw = SplitWeight(Wt)
    sw.Wt = None                                            # (the registry must not keep the weight alive)
    key = id(Wt)
    _PREPARED[key] = (weakref.ref(Wt, lambda _r, key=key: _PREPARED.pop(key, None)), sw)
    return sw


def prepared_linear(Wt, x):
    """the SplitWeight of a prepared layer if this launch should run on the split-bf16 core, else None"""
    if not GEMM_SPLIT:
        return None
    ent = _PREPARED.get(id(Wt))
    if ent is None or ent[0]() is not Wt:
        return None
    sw = ent[1]
    M = x.shape[0]
    if ((M + 255) // 256) * ((sw.n + 127) // 128) < SPLIT_MIN_TILES or not linear_split_ok(x, sw.K):
        return None
    return sw


LINEAR_POOL_TILE = 128         # rows per partial of linear_pool (the GEMM's row tile)


def _linear_pool(fn, what, x, wargs, K, n, bias, roww, relu, part, rows_per_crop, w_stride):
    """linear_pool on either core: fn = the entry point (`what` names it in an error), wargs = its weight arguments"""
    M = x.shape[0]
    if rows_per_crop is None:
        rows_per_crop, w_stride = M, 0
        assert roww.is_contiguous() and roww.numel() == M
    assert roww.dtype == torch.float32 and M % rows_per_crop == 0
    tiles = (M + LINEAR_POOL_TILE - 1) // LINEAR_POOL_TILE
    if part is None:
        part = torch.empty((tiles, n), dtype=torch.float32, device=x.device)
    assert part.shape == (tiles, n) and part.stride(1) == 1
    N.check(fn(N.ptr(x), _pitch(x), *wargs, N.ptr(bias), N.ptr(roww), int(rows_per_crop),
                                          int(w_stride), N.ptr(part), _pitch(part), int(M), int(n), int(K),
                                          int(bool(relu)), N.stream()), what)
    return part


def linear_pool(x, Wt, bias, roww, relu=True, part=None, rows_per_crop=None, w_stride=0):
    """The last fuser layer with the confidence-weighted pooling as its epilogue (csrc/linear_dma.hip, EPI = 1):
    part[t] = sum over rows j of row tile t (128 rows) of w_j * act(x[j] @ Wt + bias) -- (ceil(M/128), N); the (M, N)
    activation is never stored.  w_j = roww[j] by default; with rows_per_crop / w_stride, row j = (crop, point) weighs
    roww[crop * w_stride + point] (a direction's block of conf_softmax's (b, n1 + n2) weights).  With every crop a whole
    number of tiles, a crop's pooled feature is the sum of its tiles' partials (pool_finish2 adds them in tile order)."""
    N.need_cuda(x, Wt, roww)
    sw = prepared_linear(Wt, x)
    if sw is not None:
        return linear_split_pool(x, sw, bias, roww, relu, part, rows_per_crop, w_stride)
    M, K = x.shape
    return _linear_pool(N.lib().dcl_linear_pool_fwd, "linear_pool_fwd", x, (N.ptr(Wt), _pitch(Wt)), K, Wt.shape[1], bias, roww, relu, part,
                        rows_per_crop, w_stride)


def _linear_rowdot(fn, what, x, wargs, K, n, bias, w3, b3, out):
    """linear_rowdot on either core: fn = the entry point (`what` names it in an error), wargs = its weight arguments"""
    M = x.shape[0]
    assert n <= 128 and w3.shape == (n, 1) and b3.numel() == 1 and bias.numel() == n
    if out is None:
        out = torch.empty((M, 1), dtype=torch.float32, device=x.device)
    assert out.is_contiguous() and out.numel() == M
    if M == 0:                                              # (an empty tensor has no address to pass)
        return out
    N.check(fn(N.ptr(x), _pitch(x), *wargs, N.ptr(bias), N.ptr(w3), int(w3.stride(0)),
                                          N.ptr(b3), N.ptr(out), int(M), int(n), int(K), N.stream()), what)
    return out


def linear_rowdot(x, Wt, bias, w3, b3, out=None):
    """out[m] = w3 . relu(x[m] @ Wt + bias) + b3: the last two layers of a one-output head (regressor_conf: 128 -> 128 -> 1) as ONE
    GEMM of the own core with the row dot as its epilogue (csrc/linear_dma.hip, EPI = 2) -- the hidden columns are never stored.
    x (M,K), Wt (K,N <= 128), bias (N,), w3 (N,1) (rows may be padded: pad_linear_weight), b3 (1,) -> (M,1)."""
    N.need_cuda(x, Wt, w3, b3)
    sw = prepared_linear(Wt, x)
    if sw is not None:
        return linear_split_rowdot(x, sw, bias, w3, b3, out)
    M, K = x.shape
    return _linear_rowdot(N.lib().dcl_linear_rowdot_fwd, "linear_rowdot_fwd", x, (N.ptr(Wt), _pitch(Wt)), K, Wt.shape[1],
                          bias, w3, b3, out)


class SplitWeight:
    """A layer's weight prepared for the split-bf16 GEMM core (csrc/linear_split.hip): its three bf16 pieces in the kernel's
    tile order (`planes`), beside the (K, N) fp32 weight they were made from."""
    __slots__ = ("Wt", "planes", "K", "n")

    def __init__(self, Wt):
        N.need_cuda(Wt)
        assert Wt.dim() == 2 and Wt.dtype == torch.float32 and (Wt.stride(1) == 1 or Wt.shape[1] == 1)
        self.Wt, (self.K, self.n) = Wt, Wt.shape
        lib = N.lib()
        nbytes = int(lib.dcl_linear_split_weight_bytes(int(self.K), int(self.n)))
        assert nbytes > 0, "split-bf16 GEMM core: K must be a multiple of 16"
        self.planes = torch.empty(nbytes, dtype=torch.uint8, device=Wt.device)
        N.check(lib.dcl_linear_split_weight(N.ptr(Wt), _pitch(Wt), int(self.K), int(self.n), N.ptr(self.planes), N.stream()),
                "linear_split_weight")


def linear_split_ok(x, K):
    """can the split-bf16 core take this operand?  (K in whole 16-chunks, 16-byte aligned rows)"""
    px = int(x.stride(0)) if x.shape[0] > 1 else K
    return K >= 16 and K % 16 == 0 and px % 4 == 0 and x.data_ptr() % 16 == 0


def linear_split(x, sw, bias=None, relu=False, out=None):
    """linear() on the split-bf16 GEMM core (csrc/linear_split.hip): act(x @ sw.Wt + bias) with fp32-sized errors at the bf16
    matrix pipe's rate (three bf16 pieces per operand, six piece products per product, fp32 accumulation).  sw: SplitWeight."""
    N.need_cuda(x)
    M, K, n = x.shape[0], sw.K, sw.n
    out = _layer_io(x, K, n, bias, out)
    N.check(N.lib().dcl_linear_split_fwd(N.ptr(x), _pitch(x), N.ptr(sw.planes), N.ptr(bias), N.ptr(out), _pitch(out),
                                         int(M), int(n), int(K), int(bool(relu)), N.stream()), "linear_split_fwd")
    return out


READOUT_FOLD = 2               # deepest read-out levels folded through the first disengage GEMM: 0 = none (read-out of 480 columns, K = 480
                               # GEMM), 1 = the 256-channel level, 2 = the 128- and 256-channel levels (same-job A/B, tools/ab_readout_fold.py,
                               # profiles/readout_fold.txt: stress step 14.63 / 13.77 / 13.40 ms for 0 / 1 / 2)
READOUT_FOLD_MIN_POINTS = 40961   # ... for sides of at least this many points (below: the one-launch read-out, which is not folded)
READOUT_FOLD_K0 = {1: 224, 2: 96}                      # columns the read-out still writes = K of the first layer's GEMM


def linear_split_gather(x, sw, bias, fw, fi, G, relu=False, out=None):
    """act(x @ sw.Wt + bias + sum_l sum_i fw[l, m, i] * G[l][fi[l, m, i]]) per row m, on the split-bf16 core with the sums over
    the folded levels as its epilogue (csrc/linear_split.hip, EPI 4): per output ONE fmaf chain, levels ascending, i = 0, 1, 2.
    fw (L, M, 3) float32, fi (L, M, 3) int32, G: L = 1 or 2 matrices (R_l, N) with dense rows of any pitch.  Every fi[l] must
    index inside G[l] (not checked)."""
    N.need_cuda(x, fw, fi, *G)
    M, K, n = x.shape[0], sw.K, sw.n
    out = _layer_io(x, K, n, bias, out)
    L = len(G)
    assert L in (1, 2) and fw.shape == (L, M, 3) and fi.shape == (L, M, 3) and fw.is_contiguous() and fi.is_contiguous()
    assert fw.dtype == torch.float32 and fi.dtype == torch.int32
    for g in G:
        assert g.dim() == 2 and g.shape[1] == n and g.dtype == torch.float32 and (g.stride(1) == 1 or n == 1) and g.shape[0] > 0
    N.check(N.lib().dcl_linear_split_gather_fwd(N.ptr(x), _pitch(x), N.ptr(sw.planes), N.ptr(bias), L, N.ptr(fw), N.ptr(fi),
                                                3 * int(M), _ptr_array(list(G)), (C.c_int64 * L)(*[_pitch(g) for g in G]),
                                                N.ptr(out), _pitch(out), int(M), int(n), int(K), int(bool(relu)), N.stream()),
            "linear_split_gather_fwd")
    return out


def linear_split_pool(x, sw, bias, roww, relu=True, part=None, rows_per_crop=None, w_stride=0):
    """linear_pool() on the split-bf16 core: same partials layout (one row of `part` per 128 rows of x)"""
    N.need_cuda(x, roww)
    assert x.shape[1] == sw.K
    return _linear_pool(N.lib().dcl_linear_split_pool_fwd, "linear_split_pool_fwd", x, (N.ptr(sw.planes),), sw.K, sw.n, bias, roww,
                        relu, part, rows_per_crop, w_stride)


def linear_split_vpieces(x, sw, bias, vplanes, rows_per_crop, relu=True):
    """act(x @ sw.Wt + bias) written AS the attention's V pieces into `vplanes` (attention_planes' scratch of the call that consumes
    them with V1 = None): csrc/linear_split.hip, EPI = 3 -- the fp32 activation is never stored.  Rows = keys; every crop
    rows_per_crop rows (a multiple of 256)."""
    N.need_cuda(x, vplanes)
    M, K, n = x.shape[0], sw.K, sw.n
    assert x.shape[1] == K and n <= 320 and n % 32 == 0 and rows_per_crop % 256 == 0 and M % rows_per_crop == 0
    N.check(N.lib().dcl_linear_split_vpieces_fwd(N.ptr(x), _pitch(x), N.ptr(sw.planes), N.ptr(bias), N.ptr(vplanes),
                                                 int(rows_per_crop), int(M), int(n), int(K), int(bool(relu)), N.stream()),
            "linear_split_vpieces_fwd")
    return vplanes


def linear_split_rowdot(x, sw, bias, w3, b3, out=None):
    """linear_rowdot() on the split-bf16 core"""
    N.need_cuda(x, w3, b3)
    assert x.shape[1] == sw.K
    return _linear_rowdot(N.lib().dcl_linear_split_rowdot_fwd, "linear_split_rowdot_fwd", x, (N.ptr(sw.planes),), sw.K, sw.n, bias, w3, b3, out)


def conf_softmax(b, logit1, logit2):
    """the softmax half of conf_pool alone: logits (b*n1,), (b*n2,) -> conf (b, n1+n2) = sigmoid, w (b, n1+n2) = softmax(conf)
    per crop, wsum (b, 2) (models/DCL_Net.py:217-222)"""
    N.need_cuda(logit1, logit2)
    assert logit1.is_contiguous() and logit2.is_contiguous() and logit1.numel() % b == 0 and logit2.numel() % b == 0
    n1, n2 = logit1.numel() // b, logit2.numel() // b
    dev = logit1.device
    conf = torch.empty((b, n1 + n2), dtype=torch.float32, device=dev)
    w = torch.empty((b, n1 + n2), dtype=torch.float32, device=dev)
    ws = torch.empty((b, 2), dtype=torch.float32, device=dev)
    N.check(N.lib().dcl_conf_softmax(b, n1, n2, N.ptr(logit1), N.ptr(logit2), N.ptr(conf), N.ptr(w), N.ptr(ws), N.stream()),
            "conf_softmax")
    return conf, w, ws


def pool_finish2(part1, part2, ws, affine):
    """pooled (b, c) = ((s1*P1 + t1*wsum1) + s2*P2) + t2*wsum2 with P = a crop's tile partials added in tile order: part1
    (b*ns1, c), part2 (b*ns2, c) as linear_pool leaves them"""
    b, c = ws.shape[0], part1.shape[1]
    s1, t1, s2, t2 = affine
    assert part1.is_contiguous() and part2.is_contiguous() and part1.shape[0] % b == 0 and part2.shape[0] % b == 0
    out = torch.empty((b, c), dtype=torch.float32, device=part1.device)
    N.check(N.lib().dcl_pool_finish2(b, c, part1.shape[0] // b, part2.shape[0] // b, N.ptr(part1), N.ptr(part2), N.ptr(ws),
                                     N.ptr(s1), N.ptr(t1), N.ptr(s2), N.ptr(t2), N.ptr(out), N.stream()), "pool_finish2")
    return out


class _LinearJob(C.Structure):
    _fields_ = [("x", C.c_void_p), ("ldx", C.c_int64), ("Wt", C.c_void_p), ("ldw", C.c_int64), ("bias", C.c_void_p),
                ("y", C.c_void_p), ("ldy", C.c_int64), ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("relu", C.c_int32)]


LINEAR_GROUP_MAX = N.define("DCL_LINEAR_MAX_JOBS")


def linear_group(jobs):
    """Independent per-point linear layers in ONE launch (csrc/linear_group.hip; calls of a handful of crops, where a forward
    costs its number of dependent launches).  jobs: list of (x, Wt, bias, relu, out) with linear()'s conventions -- x (M,K),
    Wt (K,N), out (M,N) row-major with free row pitches, out=None allocates; K % 32 == 0; a Wt whose N is not a multiple of 4
    must be a column block of a buffer with rows padded to 4 floats (pad_linear_weight).  Returns the outputs."""
    assert 1 <= len(jobs) <= LINEAR_GROUP_MAX
    arr = (_LinearJob * len(jobs))()
    outs, keep = [], []
    for q, (x, Wt, bias, relu, out) in zip(arr, jobs):
        N.need_cuda(x, Wt)
        assert Wt.dim() == 2 and Wt.dtype == torch.float32
        K, n = Wt.shape
        out = _layer_io(x, K, n, bias, out, dense=(Wt,))
        M = x.shape[0]
        q.x, q.ldx, q.Wt, q.ldw, q.bias = x.data_ptr(), _pitch(x), Wt.data_ptr(), _pitch(Wt), (None if bias is None else bias.data_ptr())
        q.y, q.ldy, q.M, q.N, q.K, q.relu = out.data_ptr(), _pitch(out), int(M), int(n), int(K), int(bool(relu))
        outs.append(out)
        keep.append((x, Wt, bias))
    N.check(N.lib().dcl_linear_group_fwd(arr, len(jobs), N.stream()), "linear_group_fwd")
    return outs


def pad_linear_weight(Wt):
    """(K,N) weight as a column block of a (K, N rounded up to 4) zero-padded buffer: what linear_group wants for N % 4 != 0"""
    K, n = Wt.shape
    if n % 4 == 0:
        return Wt.contiguous()
    buf = torch.zeros((K, (n + 3) // 4 * 4), dtype=Wt.dtype, device=Wt.device)
    buf[:, :n] = Wt
    return buf[:, :n]


def mlp128_to1(x, layers, out=None):
    """The confidence regressor (models/DCL_Net.py:115-126: Head_MultiLayerPerceptron [128, 128, 128, 1], ReLU, ReLU, none) on
    point rows in ONE launch (csrc/dense.hip: k_mlp128_to1): x (M, 128) rows of pitch >= 128 (a column block of a wider buffer
    is fine), layers = [(W1t (128,128), b1), (W2t (128,128), b2), (W3t (128,1), b3)] as Network._fold() keeps them.
    Returns (M, 1) logits."""
    (W1t, b1), (W2t, b2), (W3t, b3) = layers
    N.need_cuda(x, W1t, W2t, W3t)
    M = x.shape[0]
    assert x.dim() == 2 and x.shape[1] == 128 and x.dtype == torch.float32 and (x.stride(1) == 1) and x.stride(0) % 4 == 0
    for W in (W1t, W2t):
        assert W.shape == (128, 128) and W.is_contiguous() and W.dtype == torch.float32
    assert W3t.shape == (128, 1) and b1.numel() == 128 and b2.numel() == 128 and b3.numel() == 1
    if out is None:
        out = torch.empty((M, 1), dtype=torch.float32, device=x.device)
    assert out.is_contiguous() and out.numel() == M
    N.check(N.lib().dcl_mlp128_to1(N.ptr(x), _pitch(x), int(M), N.ptr(W1t), N.ptr(b1), N.ptr(W2t),
                                   N.ptr(b2), N.ptr(W3t), int(W3t.stride(0)), N.ptr(b3), N.ptr(out), N.stream()), "mlp128_to1")
    return out


def ortho9d_to_matrix(o9):
    """ortho9d2matrix (models/DCL_Net.py:15-36): (b,9) -> (b,3,3)."""
    N.need_cuda(o9)
    o9 = o9.contiguous()
    b = o9.shape[0]
    R = torch.empty((b, 3, 3), dtype=torch.float32, device=o9.device)
    N.check(N.lib().dcl_ortho9d_to_matrix(b, N.ptr(o9), N.ptr(R), N.stream()), "ortho9d_to_matrix")
    return R


def _ortho9d_bwd_args(o9, grad_R):
    b = o9.shape[0]
    assert o9.shape == (b, 9) and grad_R.shape == (b, 3, 3), (tuple(o9.shape), tuple(grad_R.shape))
    assert o9.dtype == torch.float32 and grad_R.dtype == torch.float32
    assert o9.is_contiguous() and grad_R.is_contiguous()
    return b


def ortho9d_backward(o9, grad_R):
    """Gradient of ortho9d_to_matrix (dcl_ortho9d_bwd): o9 (b,9), grad_R (b,3,3) = dL/dR, both contiguous fp32 -> dL/do9 (b,9).
    One launch, no host synchronisation, no workspace; the same inputs give the same bits.  A crop with a non-finite o9 or
    grad_R gets NaN in its nine outputs and touches no other crop (include/dclnet_hip.h has the formula and the guards)."""
    N.need_cuda(o9, grad_R)
    b = _ortho9d_bwd_args(o9, grad_R)
    out = torch.empty((b, 9), dtype=torch.float32, device=o9.device)
    N.check(N.lib().dcl_ortho9d_bwd(b, N.ptr(o9), N.ptr(grad_R), N.ptr(out), N.stream()), "ortho9d_bwd")
    return out


def ortho9d_backward_host(o9, grad_R):
    """ortho9d_backward on CPU tensors (dcl_ortho9d_bwd_host: the kernel's routine compiled for the host).  For checking the
    mathematics where there is no GPU; no model path calls it."""
    if o9.is_cuda or grad_R.is_cuda:
        raise RuntimeError("ortho9d_backward_host is the host twin: pass CPU tensors (ortho9d_backward takes the GPU's)")
    b = _ortho9d_bwd_args(o9, grad_R)
    out = torch.empty((b, 9), dtype=torch.float32)
    N.check(N.lib().dcl_ortho9d_bwd_host(b, N.ptr(o9), N.ptr(grad_R), N.ptr(out)), "ortho9d_bwd_host")
    return out


def add_s(cld, R_pred, t_pred, R_gt, t_gt, cls=None, sym_flag=None, mode="adds"):
    """ADD-S per object (tools/test_YCBV_stage1.py:186-189) without the (b,P,P,3) intermediate.
    cld (n_clouds,P,3) f32; cls (b,) int32 picks each object's cloud (None: cloud o for object o) -> (b,) f32.
    mode="add": ADD (corresponding points, tools/test_LM.py:123); sym_flag (b,) given: ADD where it is 0, ADD-S elsewhere
    (the LineMOD rule, tools/test_LM.py:130-135)."""
    N.need_cuda(cld, R_pred, t_pred, R_gt, t_gt, cls, sym_flag)
    cld, R_pred, t_pred = N.f32c(cld), N.f32c(R_pred), N.f32c(t_pred)
    R_gt, t_gt = N.f32c(R_gt), N.f32c(t_gt)
    b, P = R_pred.shape[0], cld.shape[1]
    if cls is not None:
        cls = N.i32c(cls)
    else:
        assert cld.shape[0] == b
    part = torch.empty((b, (P + 255) // 256), dtype=torch.float32, device=cld.device)
    out = torch.empty(b, dtype=torch.float32, device=cld.device)
    if sym_flag is not None:
        sym = N.i32c(sym_flag)
        assert sym.numel() == b
        N.check(N.lib().dcl_add_by_symmetry(b, P, N.ptr(cld), N.ptr(cls), N.ptr(sym), N.ptr(R_pred), N.ptr(t_pred),
                                            N.ptr(R_gt), N.ptr(t_gt), N.ptr(part), N.ptr(out), N.stream()), "add_by_symmetry")
        return out
    fn = {"adds": N.lib().dcl_add_s, "add": N.lib().dcl_add}[mode]
    N.check(fn(b, P, N.ptr(cld), N.ptr(cls), N.ptr(R_pred), N.ptr(t_pred), N.ptr(R_gt), N.ptr(t_gt),
               N.ptr(part), N.ptr(out), N.stream()), "add_s")
    return out


def add(cld, R_pred, t_pred, R_gt, t_gt, cls=None):
    """ADD per object: mean_i |pred_i - gt_i| (tools/test_LM.py:123 `l2_dis`)."""
    return add_s(cld, R_pred, t_pred, R_gt, t_gt, cls, mode="add")


# ------------------------------------------------------------------------------------ device-resident evaluation tables
TABLE_MODES = {"adds": N.define("DCL_TABLE_ADDS"), "lm": N.define("DCL_TABLE_LM"), "lmo": N.define("DCL_TABLE_LMO")}


def metric_table_arrays(mode, steps=1, n_classes=21, device="cpu"):
    """the zeroed arrays of one table (include/dclnet_hip.h, "device-resident eval tables"): sums (T,C,4) f64 and maxd (T,C) f64
    for "adds", counts (T,C,2) i64 for "lm" / "lmo", bad (1) i32 -- a dict; the arrays the mode does not use are None."""
    T, C = int(steps), int(n_classes)
    if mode not in TABLE_MODES or T < 1 or C < 1:
        raise ValueError("metric table: mode must be one of %s, steps and n_classes >= 1" % sorted(TABLE_MODES))
    adds = mode == "adds"
    return {"sums": torch.zeros((T, C, 4), dtype=torch.float64, device=device) if adds else None,
            "maxd": torch.zeros((T, C), dtype=torch.float64, device=device) if adds else None,
            "counts": None if adds else torch.zeros((T, C, 2), dtype=torch.int64, device=device),
            "bad": torch.zeros(1, dtype=torch.int32, device=device)}


def _table_shape(table, mode, diameter, cuda):
    """(T, C) of a table dict after checking dtypes, contiguity and the side (CUDA for the kernels, CPU for the twin)"""
    if mode not in TABLE_MODES:
        raise ValueError("metric table: mode must be one of %s" % sorted(TABLE_MODES))
    lead = table["sums"] if mode == "adds" else table["counts"]
    used = [("bad", table["bad"], torch.int32)]
    used += [("sums", table["sums"], torch.float64), ("maxd", table["maxd"], torch.float64)] if mode == "adds" else \
        [("counts", table["counts"], torch.int64), ("diameter", diameter, torch.float64)]
    for name, t, dt in used:
        if t is None or t.dtype != dt or not t.is_contiguous() or t.is_cuda != cuda:
            raise RuntimeError("metric table: %s must be a contiguous %s %s tensor" % (name, "CUDA" if cuda else "CPU", dt))
    T, C = int(lead.shape[0]), int(lead.shape[1])
    assert tuple(lead.shape) == ((T, C, 4) if mode == "adds" else (T, C, 2)) and table["bad"].numel() == 1
    assert mode != "adds" or tuple(table["maxd"].shape) == (T, C)
    assert mode == "adds" or diameter.numel() == C
    return T, C


def _steps_of(R_pred, t_pred):
    """R_pred (b,3,3) / (T,b,3,3) and t_pred (b,3) / (T,b,3), float32 contiguous -> (R, t, T, b, squeeze)"""
    R_pred, t_pred = N.f32c(R_pred), N.f32c(t_pred)
    squeeze = R_pred.dim() == 3
    if squeeze:
        R_pred, t_pred = R_pred.unsqueeze(0), t_pred.unsqueeze(0)
    T, b = int(R_pred.shape[0]), int(R_pred.shape[1])
    assert tuple(R_pred.shape) == (T, b, 3, 3) and tuple(t_pred.shape) == (T, b, 3)
    return R_pred, t_pred, T, b, squeeze


def _traj_buffers(T, b, P, dev, out, scratch):
    ns = (P + 255) // 256
    if scratch is None:
        scratch = torch.empty((T, b, ns), dtype=torch.float32, device=dev)
    assert scratch.dtype == torch.float32 and scratch.is_contiguous() and scratch.numel() >= T * b * ns and scratch.is_cuda
    if out is not None:
        assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (T, b) and out.is_cuda
    return out, scratch


def add_traj(cld, R_pred, t_pred, R_gt, t_gt, cls=None, sym_flag=None, mode="adds", valid=None, out=None, scratch=None):
    """add_s for the T poses of a trajectory against one ground truth (dcl_add_traj): R_pred (T,b,3,3), t_pred (T,b,3) ->
    dis (T,b) f32 with dis[t] == add_s(cld, R_pred[t], t_pred[t], ...) bit for bit, the ground-truth cloud posed once.
    valid (b,) i32 or None: a crop with valid == 0 does no work and gets +inf.  out (T,b) / scratch (T,b,ceil(P/256)) f32:
    buffers to reuse.  A (b,3,3) R_pred is one step and returns (b,)."""
    N.need_cuda(cld, R_pred, t_pred, R_gt, t_gt, cls, sym_flag, valid)
    cld, R_gt, t_gt = N.f32c(cld), N.f32c(R_gt), N.f32c(t_gt)
    R_pred, t_pred, T, b, squeeze = _steps_of(R_pred, t_pred)
    P = cld.shape[1]
    cls = None if cls is None else N.i32c(cls)
    sym = None if sym_flag is None else N.i32c(sym_flag)
    valid = None if valid is None else N.i32c(valid)
    assert all(t is None or t.numel() == b for t in (cls, sym, valid)) and R_gt.shape[0] == b
    out, scratch = _traj_buffers(T, b, P, cld.device, out, scratch)
    if out is None:
        out = torch.empty((T, b), dtype=torch.float32, device=cld.device)
    N.check(N.lib().dcl_add_traj(T, b, P, cld.shape[0], N.ptr(cld), N.ptr(cls), N.ptr(sym), {"adds": 1, "add": 0}[mode],
                                 N.ptr(R_pred), N.ptr(t_pred), N.ptr(R_gt), N.ptr(t_gt), N.ptr(valid), N.ptr(scratch),
                                 N.ptr(out), N.stream()), "add_traj")
    return out[0] if squeeze else out


def _tabulate(table, dis, cls, valid, mode, diameter, host):
    T, C = _table_shape(table, mode, diameter, not host)
    if host and any(t is not None and t.is_cuda for t in (dis, cls, valid)):
        raise RuntimeError("metric_tabulate_host is the host twin: pass CPU tensors (metric_tabulate takes the GPU's)")
    if not host:
        N.need_cuda(dis, cls, valid)
    dis, cls = N.f32c(dis), N.i32c(cls)
    if dis.dim() == 1:
        dis = dis.unsqueeze(0)
    b = int(cls.numel())
    assert tuple(dis.shape) == (T, b), "dis must be (steps, b) = %s, got %s" % ((T, b), tuple(dis.shape))
    valid = None if valid is None else N.i32c(valid)
    assert valid is None or valid.numel() == b
    N.twin("dcl_metric_tabulate", host, "metric_tabulate_host" if host else "metric_tabulate", TABLE_MODES[mode], T, b, C,
           N.ptr(dis), N.ptr(cls), N.ptr(valid), N.ptr(diameter), N.ptr(table["sums"]), N.ptr(table["maxd"]),
           N.ptr(table["counts"]), N.ptr(table["bad"]))
    return table


def metric_tabulate(table, dis, cls, valid=None, mode="adds", diameter=None):
    """adds the crops (dis (T,b) f32, cls (b,) i32, valid (b,) i32 or None) to a device-resident table IN PLACE
    (dcl_metric_tabulate: one launch, lane c owns class c and walks the crops in ascending order; no atomics, no read-back).
    table: metric_table_arrays(...)'s dict; diameter (C,) f64 CUDA for "lm" / "lmo".  The semantics are the host classes'
    (sharding.AddsTable / LmTable / LmoTable), comparisons in double on the fp32 distance."""
    return _tabulate(table, dis, cls, valid, mode, diameter, False)


def metric_tabulate_host(table, dis, cls, valid=None, mode="adds", diameter=None):
    """the host twin of metric_tabulate (dcl_metric_tabulate_host, plain C++, no GPU call) on CPU tensors"""
    return _tabulate(table, dis, cls, valid, mode, diameter, True)


def add_tabulate(table, cld, cls, R_pred, t_pred, R_gt, t_gt, valid=None, cloud=None, sym_flag=None, metric="adds", mode="adds",
                 diameter=None, out=None, scratch=None):
    """one frame from poses to table in TWO launches (dcl_add_tabulate): add_traj's slice launch, then one launch that finishes
    the distances and tabulates them -- the bits of add_traj followed by metric_tabulate.  cls (b,) i32: the table's class
    ids; cloud (b,) i32 picks each crop's cloud of cld (n_clouds,P,3) (None: cloud i for crop i).  metric / sym_flag as
    add_traj's mode / sym_flag.  out (T,b) f32, if given, also receives the distances."""
    N.need_cuda(cld, cls, R_pred, t_pred, R_gt, t_gt, valid, cloud, sym_flag)
    Tt, C = _table_shape(table, mode, diameter, True)
    cld, R_gt, t_gt = N.f32c(cld), N.f32c(R_gt), N.f32c(t_gt)
    R_pred, t_pred, T, b, _ = _steps_of(R_pred, t_pred)
    assert T == Tt, "the table holds %d steps, the poses %d" % (Tt, T)
    P = cld.shape[1]
    cls = N.i32c(cls)
    cloud = None if cloud is None else N.i32c(cloud)
    sym = None if sym_flag is None else N.i32c(sym_flag)
    valid = None if valid is None else N.i32c(valid)
    assert all(t is None or t.numel() == b for t in (cls, cloud, sym, valid)) and R_gt.shape[0] == b
    out, scratch = _traj_buffers(T, b, P, cld.device, out, scratch)
    N.check(N.lib().dcl_add_tabulate(TABLE_MODES[mode], T, b, P, cld.shape[0], C, N.ptr(cld), N.ptr(cloud), N.ptr(cls),
                                     N.ptr(sym), {"adds": 1, "add": 0}[metric], N.ptr(R_pred), N.ptr(t_pred), N.ptr(R_gt),
                                     N.ptr(t_gt), N.ptr(valid), N.ptr(diameter), N.ptr(scratch), N.ptr(out),
                                     N.ptr(table["sums"]), N.ptr(table["maxd"]), N.ptr(table["counts"]), N.ptr(table["bad"]),
                                     N.stream()), "add_tabulate")
    return table


# ------------------------------------------------------------------------------------ crop builder
def legacy_choice_heads(ms, n):
    """[np.random.choice(m, n, replace=False) for m in ms] on the GLOBAL legacy generator, bit for bit and with the same
    advance of its state, ~3x faster (csrc/legacy_rng.cpp: numpy's Fisher-Yates walk as a tight branch-free loop).  Host
    code; every m must be >= n.  -> int64 array (len(ms), n).  (The loaders' sampling draws: YCBV/dataloader_test_YCBV.py:166-169.)"""
    import numpy as np
    k = len(ms)
    out = np.empty((k, int(n)), np.int64)
    if k == 0:
        return out
    st = np.random.get_state()
    assert st[0] == "MT19937"
    key = np.ascontiguousarray(st[1], dtype=np.uint32).copy()
    pos = C.c_int32(int(st[2]))
    m = np.ascontiguousarray(np.asarray(ms, np.int32))
    scratch = np.empty(int(m.max()), np.int32)
    N.check(N.lib().dcl_legacy_permutation_heads(key.ctypes.data_as(C.c_void_p), C.byref(pos), m.ctypes.data_as(C.c_void_p), k, int(n),
                                                 out.ctypes.data_as(C.c_void_p), scratch.ctypes.data_as(C.c_void_p)),
            "legacy_permutation_heads")
    np.random.set_state((st[0], key, int(pos.value), st[3], st[4]))
    return out


def crop_points(depth, label, rgb, boxes, obj_ids, cam, rgb_mean, half_extent, min_valid=32, always_filter=False, cap=None):
    """Masked back-projection + centring + grid filter of every object instance of one image
    (YCBV/dataloader_test_YCBV.py:124-165).  depth (H,W) u16 viewed as int16 storage, label (H,W) i32, rgb (H,W,C) u8,
    boxes (n,4) i32 [rmin,rmax,cmin,cmax], obj_ids (n) i32 -- all CUDA.  cam = (cx,cy,fx,fy,scale[,post_div]).
    -> xyz (n,cap,3), rgb (n,cap,3), centroid (n,3), counts (n,3) i32 [masked, inside grid, rows]."""
    N.need_cuda(depth, label, rgb, boxes, obj_ids)
    assert depth.dtype in (torch.int16, torch.uint16) and label.dtype == torch.int32 and rgb.dtype == torch.uint8
    assert depth.is_contiguous() and label.is_contiguous() and rgb.is_contiguous()
    assert boxes.dtype == torch.int32 and obj_ids.dtype == torch.int32 and boxes.is_contiguous()
    H, W = depth.shape
    n = boxes.shape[0]
    dev = depth.device
    if cap is None:                                            # (a caller that made the boxes on the host passes the largest area)
        bx = boxes.cpu()
        cap = int(max(1, ((bx[:, 1] - bx[:, 0]).clamp(min=0) * (bx[:, 3] - bx[:, 2]).clamp(min=0)).max().item())) if n else 1
    raw_xyz = torch.empty((n, cap, 3), dtype=torch.float32, device=dev)
    raw_rgb = torch.empty((n, cap, 3), dtype=torch.float32, device=dev)
    xyz = torch.empty((n, cap, 3), dtype=torch.float32, device=dev)
    col = torch.empty((n, cap, 3), dtype=torch.float32, device=dev)
    centroid = torch.empty((n, 3), dtype=torch.float32, device=dev)
    counts = torch.zeros((n, 3), dtype=torch.int32, device=dev)
    ws = torch.empty(max(N.query("dcl_crop_points_ws_ints", n, int(cap)), 1), dtype=torch.int32, device=dev)
    cam_a = (C.c_float * 6)(*([float(v) for v in cam] + [1.0])[:6])
    mean_a = (C.c_double * 3)(*[float(v) for v in rgb_mean])
    he_a = (C.c_float * 3)(*[float(v) for v in half_extent])
    N.check(N.lib().dcl_crop_points(N.ptr(depth), N.ptr(label), N.ptr(rgb), H, W, rgb.shape[2], n, N.ptr(boxes),
                                    N.ptr(obj_ids), cam_a, mean_a, he_a, int(min_valid), int(bool(always_filter)), cap,
                                    N.ptr(raw_xyz),
                                    N.ptr(raw_rgb), N.ptr(xyz), N.ptr(col), N.ptr(centroid), N.ptr(counts), N.ptr(ws), N.stream()),
            "crop_points")
    return xyz, col, centroid, counts


def crop_points_frames(depth, label, rgb, frame_idx, src, cam, rgb_mean, half_extent, min_valid=32, always_filter=False, cap=None,
                       rows=None):
    """crop_points over STACKED frames (csrc/crops.hip: dcl_crop_points_frames): depth / label (f,H,W), rgb (f,H,W,C);
    frame_idx: the crops' frames as a HOST sequence (checked against f by the call, before any device work); src (n,6) i32
    [rmin,rmax,cmin,cmax,class,frame] CUDA -- a device row that names no frame gives an empty crop.  One camera
    cam = (cx,cy,fx,fy,scale[,post_div]) for all frames.  -> xyz (n,cap,3), rgb (n,cap,3), centroid (n,3), counts (n,3) i32, for
    every instance bit for bit what crop_points returns for its frame alone.  No host synchronisation when cap is given.
    rows >= n: centroid and counts have that many rows, the ones behind n are zero (the padding rows of a padded batch)."""
    import numpy as np
    N.need_cuda(depth, label, rgb, src)
    assert depth.dtype in (torch.int16, torch.uint16) and label.dtype == torch.int32 and rgb.dtype == torch.uint8
    assert depth.dim() == 3 and label.shape == depth.shape and rgb.dim() == 4 and rgb.shape[:3] == depth.shape
    assert depth.is_contiguous() and label.is_contiguous() and rgb.is_contiguous()
    n = src.shape[0]
    assert src.dtype == torch.int32 and src.is_contiguous() and tuple(src.shape) == (n, 6)
    fidx = np.ascontiguousarray(np.asarray(frame_idx, np.int32).reshape(-1))
    assert fidx.shape[0] == n
    f, H, W = depth.shape
    dev = depth.device
    if cap is None:
        bx = src.cpu()
        cap = int(max(1, ((bx[:, 1] - bx[:, 0]).clamp(min=0) * (bx[:, 3] - bx[:, 2]).clamp(min=0)).max().item())) if n else 1
    raw_xyz = torch.empty((n, cap, 3), dtype=torch.float32, device=dev)
    raw_rgb = torch.empty((n, cap, 3), dtype=torch.float32, device=dev)
    xyz = torch.empty((n, cap, 3), dtype=torch.float32, device=dev)
    col = torch.empty((n, cap, 3), dtype=torch.float32, device=dev)
    rows = n if rows is None else int(rows)
    assert rows >= n
    centroid = (torch.empty if rows == n else torch.zeros)((rows, 3), dtype=torch.float32, device=dev)
    counts = torch.zeros((rows, 3), dtype=torch.int32, device=dev)
    ws = torch.empty(max(N.query("dcl_crop_points_ws_ints", n, int(cap)), 1), dtype=torch.int32, device=dev)
    cam_a = (C.c_float * 6)(*([float(v) for v in cam] + [1.0])[:6])
    mean_a = (C.c_double * 3)(*[float(v) for v in rgb_mean])
    he_a = (C.c_float * 3)(*[float(v) for v in half_extent])
    N.check(N.lib().dcl_crop_points_frames(N.ptr(depth), N.ptr(label), N.ptr(rgb), f, H, W, rgb.shape[3], n,
                                           fidx.ctypes.data_as(C.c_void_p), N.ptr(src), cam_a, mean_a, he_a, int(min_valid),
                                           int(bool(always_filter)), int(cap), N.ptr(raw_xyz), N.ptr(raw_rgb), N.ptr(xyz),
                                           N.ptr(col), N.ptr(centroid), N.ptr(counts), N.ptr(ws), N.stream()),
            "crop_points_frames")
    return xyz, col, centroid, counts


def crop_sample(xyz, rgb, sample_idx, counts, half_extent0, unit, voxel_limit, npoint=None, min_valid=32):
    """Sampled points -> feats (n*npoint,7) [1,rgb,xyz] and voxelize_idx input rows (n*npoint,4) i64 [instance,ix,iy,iz]
    (dataloader_test_YCBV.py:166-177,186-190).  sample_idx (n,npoint) i64 CUDA or None (identity, template clouds)."""
    N.need_cuda(xyz, rgb, sample_idx, counts)
    assert xyz.is_contiguous() and rgb.is_contiguous() and xyz.dtype == torch.float32 and rgb.dtype == torch.float32
    n, cap = xyz.shape[0], xyz.shape[1]
    if sample_idx is not None:
        assert sample_idx.dtype == torch.int64 and sample_idx.is_contiguous() and sample_idx.shape[0] == n
        npoint = sample_idx.shape[1]
    else:
        npoint = cap if npoint is None else npoint
    dev = xyz.device
    feats = torch.empty((n * npoint, 7), dtype=torch.float32, device=dev)
    coords = torch.empty((n * npoint, 4), dtype=torch.int64, device=dev)
    unit_a = (C.c_float * 3)(*[float(v) for v in unit])
    N.check(N.lib().dcl_crop_sample(n, npoint, cap, N.ptr(xyz), N.ptr(rgb), N.ptr(sample_idx), N.ptr(counts),
                                    int(min_valid), half_extent0, unit_a, int(voxel_limit), N.ptr(feats),
                                    N.ptr(coords), N.stream()), "crop_sample")
    return feats, coords


CROP_DRAW_MAX_POINTS = N.define("DCL_CROP_DRAW_MAX_POINTS")
_U64 = (1 << 64) - 1


def crop_draw(counts, npoint, seed, frame, min_valid=32, keep_sparse=True):
    """The sampling draws of every instance ON THE DEVICE (csrc/crop_draw.hip; the definition: include/dclnet_hip.h,
    dcl_crop_draw): counts (n,3) i32 CUDA as crop_points returns it -> sample_idx (n,npoint) i64, valid (n) i32, both CUDA.
    A pure function of (seed, frame, row, counts row) -- NOT the loader's np.random stream; no host synchronisation."""
    N.need_cuda(counts)
    assert counts.dtype == torch.int32 and counts.is_contiguous() and counts.dim() == 2 and counts.shape[1] == 3
    n = counts.shape[0]
    idx = torch.empty((n, max(int(npoint), 0)), dtype=torch.int64, device=counts.device)
    valid = torch.empty((n,), dtype=torch.int32, device=counts.device)
    N.check(N.lib().dcl_crop_draw(n, int(npoint), N.ptr(counts), int(min_valid), int(bool(keep_sparse)),
                                  int(seed) & _U64, int(frame) & _U64, N.ptr(idx), N.ptr(valid),
                                  N.stream()), "crop_draw")
    return idx, valid


def crop_draw_host(counts, npoint, seed, frame, min_valid=32, keep_sparse=True):
    """the host twin of crop_draw (dcl_crop_draw_host, plain C++, no GPU call): counts (n,3) integer numpy array ->
    (sample_idx (n,npoint) int64, valid (n) int32) numpy arrays."""
    import numpy as np
    cnt = np.ascontiguousarray(np.asarray(counts).astype(np.int32)).reshape(-1, 3)
    n = cnt.shape[0]
    idx = np.zeros((n, max(int(npoint), 0)), np.int64)
    valid = np.zeros(n, np.int32)
    N.check(N.lib().dcl_crop_draw_host(n, int(npoint), cnt.ctypes.data_as(C.c_void_p), int(min_valid), int(bool(keep_sparse)),
                                       int(seed) & _U64, int(frame) & _U64,
                                       idx.ctypes.data_as(C.c_void_p), valid.ctypes.data_as(C.c_void_p)), "crop_draw_host")
    return idx, valid


def crop_draw_keyed(counts, npoint, seed, keys, min_valid=32, keep_sparse=True, rows=None):
    """crop_draw with a key per row (dcl_crop_draw_keyed): keys (n,2) CUDA int64 storage of the uint64 rows {frame, inst}; row i
    draws what row keys[i][1] of crop_draw(..., frame=keys[i][0]) draws on the same counts row -- a batch of several frames
    draws what the frames draw one by one.  -> sample_idx (n,npoint) i64, valid (n) i32, both CUDA; no host synchronisation.
    counts may hold more than n rows (the zero rows of a padded batch): the first n are drawn.  rows >= n: the outputs have that many rows, the ones behind n are PADDING (sample_idx 0, valid -1: "not a crop")."""
    N.need_cuda(counts, keys)
    assert counts.dtype == torch.int32 and counts.is_contiguous() and counts.dim() == 2 and counts.shape[1] == 3
    n = keys.shape[0]
    assert keys.dtype == torch.int64 and keys.is_contiguous() and tuple(keys.shape) == (n, 2) and counts.shape[0] >= n
    rows = n if rows is None else int(rows)
    assert rows >= n
    if rows > n:
        idx = torch.zeros((rows, max(int(npoint), 0)), dtype=torch.int64, device=counts.device)
        valid = torch.full((rows,), -1, dtype=torch.int32, device=counts.device)
    else:
        idx = torch.empty((n, max(int(npoint), 0)), dtype=torch.int64, device=counts.device)
        valid = torch.empty((n,), dtype=torch.int32, device=counts.device)
    N.check(N.lib().dcl_crop_draw_keyed(n, int(npoint), N.ptr(counts), int(min_valid), int(bool(keep_sparse)),
                                        int(seed) & _U64, N.ptr(keys), N.ptr(idx), N.ptr(valid), N.stream()),
            "crop_draw_keyed")
    return idx, valid


def crop_draw_keyed_host(counts, npoint, seed, keys, min_valid=32, keep_sparse=True):
    """the host twin of crop_draw_keyed (dcl_crop_draw_keyed_host, plain C++, no GPU call): counts (n,3) and keys (n,2)
    {frame, inst} integer numpy arrays -> (sample_idx (n,npoint) int64, valid (n) int32) numpy arrays."""
    import numpy as np
    cnt = np.ascontiguousarray(np.asarray(counts).astype(np.int32)).reshape(-1, 3)
    n = cnt.shape[0]
    ks = None if keys is None else np.ascontiguousarray(np.asarray(keys).astype(np.uint64)).reshape(-1, 2)
    assert ks is None or ks.shape[0] == n
    idx = np.zeros((n, max(int(npoint), 0)), np.int64)
    valid = np.zeros(n, np.int32)
    N.check(N.lib().dcl_crop_draw_keyed_host(n, int(npoint), cnt.ctypes.data_as(C.c_void_p), int(min_valid), int(bool(keep_sparse)),
                                             int(seed) & _U64,
                                             C.c_void_p(0) if ks is None else ks.ctypes.data_as(C.c_void_p),
                                             idx.ctypes.data_as(C.c_void_p), valid.ctypes.data_as(C.c_void_p)),
            "crop_draw_keyed_host")
    return idx, valid


def crop_draw_keys_host(seed, frame, inst, s, n):
    """base(seed, frame, inst, s) and key(0..n-1) of the draw's generator (dcl_crop_draw_keys_host) -> (int, uint64 array)"""
    import numpy as np
    base = np.zeros(1, np.uint64)
    keys = np.zeros(int(n), np.uint64)
    N.check(N.lib().dcl_crop_draw_keys_host(int(seed) & _U64, int(frame) & _U64, int(inst), int(s), int(n),
                                            base.ctypes.data_as(C.c_void_p), keys.ctypes.data_as(C.c_void_p)), "crop_draw_keys_host")
    return int(base[0]), keys


def crop_sample_valid(xyz, rgb, sample_idx, counts, valid, half_extent0, unit, voxel_limit, min_valid=32):
    """crop_sample for the instances with valid > 0 (the same rows, bit for bit), a lattice dummy crop -- point j at the centre
    of voxel (j mod S, (j div S) mod S, j div S^2), colour 0 -- for the others (csrc/crop_draw.hip).  sample_idx (n,npoint) i64,
    valid (n) i32, counts (n,3) i32 or None, all CUDA.  -> feats (n*npoint,7), coords (n*npoint,4) i64.
    sample_idx / valid may have MORE rows than xyz (crop_draw_keyed(rows=...)): the rows behind xyz's are padding, their valid
    must be <= 0 (the kernel addresses xyz, rgb and counts only through rows with valid > 0) and they get lattice rows too."""
    N.need_cuda(xyz, rgb, sample_idx, counts, valid)
    assert xyz.is_contiguous() and rgb.is_contiguous() and xyz.dtype == torch.float32 and rgb.dtype == torch.float32
    n, cap = valid.shape[0], xyz.shape[1]
    assert n >= xyz.shape[0]
    assert sample_idx.dtype == torch.int64 and sample_idx.is_contiguous() and sample_idx.shape[0] == n
    assert valid.dtype == torch.int32 and valid.is_contiguous()
    assert counts is None or (counts.dtype == torch.int32 and counts.is_contiguous() and counts.shape[0] >= xyz.shape[0])
    npoint = sample_idx.shape[1]
    dev = xyz.device
    feats = torch.empty((n * npoint, 7), dtype=torch.float32, device=dev)
    coords = torch.empty((n * npoint, 4), dtype=torch.int64, device=dev)
    unit_a = (C.c_float * 3)(*[float(v) for v in unit])
    N.check(N.lib().dcl_crop_sample_valid(n, npoint, cap, N.ptr(xyz), N.ptr(rgb), N.ptr(sample_idx), N.ptr(counts), int(min_valid),
                                          N.ptr(valid), half_extent0, unit_a, int(voxel_limit), N.ptr(feats),
                                          N.ptr(coords), N.stream()), "crop_sample_valid")
    return feats, coords


def crop_sample_valid_host(xyz, rgb, sample_idx, counts, valid, half_extent0, unit, voxel_limit, min_valid=32):
    """the host twin of crop_sample_valid (dcl_crop_sample_valid_host, plain C++, no GPU call) on numpy arrays"""
    import numpy as np
    x = np.ascontiguousarray(np.asarray(xyz, np.float32))
    c = np.ascontiguousarray(np.asarray(rgb, np.float32))
    idx = np.ascontiguousarray(np.asarray(sample_idx).astype(np.int64))
    val = np.ascontiguousarray(np.asarray(valid).astype(np.int32))
    cnt = None if counts is None else np.ascontiguousarray(np.asarray(counts).astype(np.int32))
    n, cap = x.shape[0], x.shape[1]
    npoint = idx.shape[1]
    feats = np.zeros((n * npoint, 7), np.float32)
    coords = np.zeros((n * npoint, 4), np.int64)
    unit_a = (C.c_float * 3)(*[float(v) for v in unit])
    p = lambda a: C.c_void_p(0) if a is None else a.ctypes.data_as(C.c_void_p)
    N.check(N.lib().dcl_crop_sample_valid_host(n, npoint, cap, p(x), p(c), p(idx), p(cnt), int(min_valid), p(val),
                                               half_extent0, unit_a, int(voxel_limit), p(feats), p(coords)),
            "crop_sample_valid_host")
    return feats, coords


def mask_box(label, value=1, padding=0):
    """`get_bbox(mask_to_bbox(label == value, padding))` of the LineMOD / Occlusion-LineMOD loaders on the device
    (csrc/mask_box.hip).  label (H,W) or (n,H,W) i32 CUDA.  -> (n,10) i32 CUDA: box [x,y,w,h] of the 8-connected component
    with the largest bounding rectangle, the box row ops.crop_points takes (columns 4:8), the number of components and the
    winner's pixel count.  No host synchronisation; the workspace is a torch allocation."""
    N.need_cuda(label)
    assert label.dtype == torch.int32 and label.is_contiguous() and label.dim() in (2, 3)
    n = 1 if label.dim() == 2 else label.shape[0]
    H, W = label.shape[-2], label.shape[-1]
    out = torch.empty((n, 10), dtype=torch.int32, device=label.device)
    nb = N.query("dcl_mask_box_ws_bytes", n, H, W)
    ws = torch.empty(max(nb // 4, 1), dtype=torch.int32, device=label.device)
    N.check(N.lib().dcl_mask_box(N.ptr(label), n, H, W, int(value), int(padding), N.ptr(out), N.ptr(ws), nb,
                                 N.stream()), "mask_box")
    return out


def mask_box_host(label, value=1, padding=0):
    """the host twin of mask_box (dcl_mask_box_host: same semantics, sequential, no GPU call): label (H,W) or (n,H,W)
    integer numpy array -> (n,10) int32 numpy array."""
    import numpy as np
    lab = np.ascontiguousarray(np.asarray(label).astype(np.int32))
    assert lab.ndim in (2, 3)
    n = 1 if lab.ndim == 2 else lab.shape[0]
    out = np.zeros((n, 10), np.int32)
    N.check(N.lib().dcl_mask_box_host(lab.ctypes.data_as(C.c_void_p), n, lab.shape[-2], lab.shape[-1], int(value), int(padding),
                                      out.ctypes.data_as(C.c_void_p)), "mask_box_host")
    return out


def label_table(label, depth, n_classes):
    """Per-frame class table of the training loader (csrc/crops_train.hip: dcl_label_table).  label (n,H,W) i32 CUDA, depth
    (n,H,W) 16-bit storage CUDA -> (n, n_classes, 5) i32 CUDA: [pixels with label == c and depth != 0, min row, max row,
    min col, max col of label == c]; an absent class has count 0, min = 2^31 - 1 and max = -1.  No host synchronisation."""
    N.need_cuda(label, depth)
    assert label.dtype == torch.int32 and depth.dtype in (torch.int16, torch.uint16) and label.dim() == 3
    assert label.is_contiguous() and depth.is_contiguous() and depth.shape == label.shape
    n, H, W = label.shape
    out = torch.empty((n, int(n_classes), 5), dtype=torch.int32, device=label.device)
    N.check(N.lib().dcl_label_table(N.ptr(label), N.ptr(depth), n, H, W, int(n_classes), N.ptr(out), N.stream()), "label_table")
    return out


def label_table_host(label, depth, n_classes):
    """the host twin of label_table (dcl_label_table_host, plain C++, no GPU call): (n,H,W) integer numpy arrays ->
    (n, n_classes, 5) int32 numpy array."""
    import numpy as np
    lab = np.ascontiguousarray(np.asarray(label).astype(np.int32))
    dep = np.ascontiguousarray(np.asarray(depth).astype(np.uint16))
    assert lab.ndim == 3 and dep.shape == lab.shape
    n, H, W = lab.shape
    out = np.zeros((n, int(n_classes), 5), np.int32)
    N.check(N.lib().dcl_label_table_host(lab.ctypes.data_as(C.c_void_p), dep.ctypes.data_as(C.c_void_p), n, H, W, int(n_classes),
                                         out.ctypes.data_as(C.c_void_p)), "label_table_host")
    return out


def pose_rows(R0, t_gt, jitter, aug_r):
    """The pose rows dcl_crop_points_posed takes (include/dclnet_hip.h: 112 bytes per crop): R0 (n,3,3) and aug_r (n,3,3)
    rounded to float32, t_gt (n,3) kept float64, jitter (n,3) rounded to float32 -> (n,112) uint8 numpy array."""
    import numpy as np
    n = len(R0)
    rows = np.zeros(n, POSE_ROW)
    rows["t_gt"], rows["R0"] = np.asarray(t_gt, np.float64).reshape(n, 3), np.asarray(R0).astype(np.float32).reshape(n, 3, 3)
    rows["j"], rows["A"] = np.asarray(jitter).astype(np.float32).reshape(n, 3), np.asarray(aug_r).astype(np.float32).reshape(n, 3, 3)
    return rows.view(np.uint8).reshape(n, POSE_ROW_BYTES)


POSE_ROW_BYTES = N.define("DCL_CROP_POSE_ROW_BYTES")
POSE_ROW = [("t_gt", "<f8", (3,)), ("R0", "<f4", (3, 3)), ("j", "<f4", (3,)), ("A", "<f4", (3, 3)), ("pad", "<f4")]


def crop_points_posed(depth, label, rgb, frame_idx, src, cams, pose, rgb_mean, half_extent, min_valid=50, cap=None):
    """The training loader's masked back-projection, centring, re-pose and grid filter (YCBV/dataloader_train_YCBV.py:138-193;
    csrc/crops_train.hip).  depth / label (f,H,W), rgb (f,H,W,C) stacked frames; frame_idx: the crops' frames as a HOST
    sequence (checked against f by the call); src (n,6) i32 [rmin,rmax,cmin,cmax,class,frame], cams (n,5) f32
    [cx,cy,fx,fy,scale], pose (n,112) u8 (pose_rows) -- all CUDA.  -> xyz (n,cap,3) re-posed points inside the grid, rgb
    (n,cap,3), centroid (n,3), counts (n,3) i32 [masked, inside the grid, rows: 0 unless more than min_valid are inside],
    rot_gt (n,3,3), trans_gt (n,3).  No host synchronisation when cap is given."""
    import numpy as np
    N.need_cuda(depth, label, rgb, src, cams, pose)
    assert depth.dtype in (torch.int16, torch.uint16) and label.dtype == torch.int32 and rgb.dtype == torch.uint8
    assert depth.dim() == 3 and label.shape == depth.shape and rgb.dim() == 4 and rgb.shape[:3] == depth.shape
    assert depth.is_contiguous() and label.is_contiguous() and rgb.is_contiguous()
    n = src.shape[0]
    assert src.dtype == torch.int32 and src.is_contiguous() and tuple(src.shape) == (n, 6)
    assert cams.dtype == torch.float32 and cams.is_contiguous() and tuple(cams.shape) == (n, 5)
    assert pose.dtype == torch.uint8 and pose.is_contiguous() and tuple(pose.shape) == (n, POSE_ROW_BYTES)
    fidx = np.ascontiguousarray(np.asarray(frame_idx, np.int32).reshape(-1))
    assert fidx.shape[0] == n
    f, H, W = depth.shape
    dev = depth.device
    if cap is None:
        bx = src.cpu()
        cap = int(max(1, ((bx[:, 1] - bx[:, 0]).clamp(min=0) * (bx[:, 3] - bx[:, 2]).clamp(min=0)).max().item())) if n else 1
    raw_xyz = torch.empty((n, cap, 3), dtype=torch.float32, device=dev)
    raw_rgb = torch.empty((n, cap, 3), dtype=torch.float32, device=dev)
    xyz = torch.empty((n, cap, 3), dtype=torch.float32, device=dev)
    col = torch.empty((n, cap, 3), dtype=torch.float32, device=dev)
    centroid = torch.empty((n, 3), dtype=torch.float32, device=dev)
    counts = torch.zeros((n, 3), dtype=torch.int32, device=dev)
    rot_gt = torch.empty((n, 3, 3), dtype=torch.float32, device=dev)
    trans_gt = torch.empty((n, 3), dtype=torch.float32, device=dev)
    ws = torch.empty(max(N.query("dcl_crop_points_ws_ints", n, int(cap)), 1), dtype=torch.int32, device=dev)
    mean_a = (C.c_double * 3)(*[float(v) for v in rgb_mean])
    he_a = (C.c_float * 3)(*[float(v) for v in half_extent])
    N.check(N.lib().dcl_crop_points_posed(N.ptr(depth), N.ptr(label), N.ptr(rgb), f, H, W, rgb.shape[3], n,
                                          fidx.ctypes.data_as(C.c_void_p), N.ptr(src), N.ptr(cams), N.ptr(pose), mean_a, he_a,
                                          int(min_valid), int(cap), N.ptr(raw_xyz), N.ptr(raw_rgb), N.ptr(xyz), N.ptr(col),
                                          N.ptr(centroid), N.ptr(counts), N.ptr(rot_gt), N.ptr(trans_gt), N.ptr(ws), N.stream()),
            "crop_points_posed")
    return xyz, col, centroid, counts, rot_gt, trans_gt


def crop_repose_host(points, pose_row, centroid):
    """the host twin of the re-pose (dcl_crop_repose_host, plain C++ with the library's -ffp-contract=off): CENTRED points
    (n,3) float32, one pose row (112 bytes, pose_rows), centroid (3) float32 -> (re-posed points (n,3), R1 (3,3), t1 (3))."""
    import numpy as np
    pts = np.ascontiguousarray(np.asarray(points, np.float32).reshape(-1, 3))
    row = np.ascontiguousarray(np.asarray(pose_row, np.uint8).reshape(-1))
    cen = np.ascontiguousarray(np.asarray(centroid, np.float32).reshape(3))
    assert row.shape[0] == POSE_ROW_BYTES
    out, R1, t1 = np.empty_like(pts), np.empty((3, 3), np.float32), np.empty(3, np.float32)
    N.check(N.lib().dcl_crop_repose_host(pts.ctypes.data_as(C.c_void_p), row.ctypes.data_as(C.c_void_p),
                                         cen.ctypes.data_as(C.c_void_p), pts.shape[0], out.ctypes.data_as(C.c_void_p),
                                         R1.ctypes.data_as(C.c_void_p), t1.ctypes.data_as(C.c_void_p)), "crop_repose_host")
    return out, R1, t1


# ---- the LineMOD training loader's front end (csrc/crops_train_lm.hip)
PASTE_PLAN_INTS = N.define("DCL_PASTE_PLAN_INTS")
# columns of a paste plan row (include/dclnet_hip.h: dcl_occlude_paste)
PASTE_PLAN = ("enabled", "other", "py0", "px0", "ph", "pw", "ty0", "tx0", "th", "tw", "rep_y", "rep_x", "rmin", "rmax", "cmin", "cmax")
POSE_ROW64_BYTES = N.define("DCL_CROP_POSE_ROW64_BYTES")
POSE_ROW64 = [("t_gt", "<f8", (3,)), ("R0", "<f8", (3, 3)), ("j", "<f8", (3,)), ("A", "<f8", (3, 3))]


def extent_sums(extent):
    """the int64 mask sums behind columns 4:6 of mask_extent's rows: (n,6) int32 numpy array -> (n) int64"""
    import numpy as np
    return np.ascontiguousarray(np.asarray(extent, np.int32)[:, 4:6]).view(np.int64).reshape(-1)


def mask_extent(mask):
    """What `occlude_with_another_object` reduces of an object mask (LM/dataloader_train_LM.py:301-306,343; dcl_mask_extent).
    mask (n,H,W,3) u8 CUDA -> (n,6) i32 CUDA: [min row, max row, min col, max col of mask[..., 0] != 0 (2^31 - 1 / -1 when
    empty), and in columns 4:6 ONE int64: the sum of all bytes (extent_sums reads it)].  No host synchronisation."""
    N.need_cuda(mask)
    assert mask.dtype == torch.uint8 and mask.dim() == 4 and mask.shape[3] == 3 and mask.is_contiguous()
    n, H, W = mask.shape[:3]
    out = torch.empty((n, 6), dtype=torch.int32, device=mask.device)
    N.check(N.lib().dcl_mask_extent(N.ptr(mask), n, H, W, N.ptr(out), N.stream()), "mask_extent")
    return out


def mask_extent_host(mask):
    """the host twin of mask_extent (dcl_mask_extent_host, plain C++, no GPU call): (n,H,W,3) u8 numpy -> (n,6) int32 numpy"""
    import numpy as np
    m = np.ascontiguousarray(np.asarray(mask, np.uint8))
    assert m.ndim == 4 and m.shape[3] == 3
    out = np.zeros((m.shape[0], 6), np.int32)
    N.check(N.lib().dcl_mask_extent_host(m.ctypes.data_as(C.c_void_p), m.shape[0], m.shape[1], m.shape[2],
                                         out.ctypes.data_as(C.c_void_p)), "mask_extent_host")
    return out


def occlude_paste(rgb, depth, mask, other_rgb, other_depth, other_mask, plan_host, plan, extent):
    """The occlusion compositing of the LineMOD training loader with its commit / roll-back decision on the device
    (LM/dataloader_train_LM.py:335-346; dcl_occlude_paste).  rgb (n,H,W,C) u8, depth (n,H,W) 16-bit storage, mask (n,H,W,3) u8;
    other_* the occluder frames (k,H,W,3) / (k,H,W) / (k,H,W,3) (k may be 0); plan (n,16) i32 CUDA rows (crops.lm_paste_plan,
    columns PASTE_PLAN) and plan_host their host copy (checked by the call); extent: mask_extent(mask), CUDA.
    -> working copies rgb' (n,H,W,C) u8, depth' (n,H,W), label' (n,H,W) i32 = channel 0 of the mask afterwards, and info (n,4)
    i64 [committed, remaining mask sum, n_box_valid, removed].  The inputs are not modified; no host synchronisation."""
    import numpy as np
    N.need_cuda(rgb, depth, mask, other_rgb, other_depth, other_mask, plan, extent)
    assert rgb.dtype == torch.uint8 and mask.dtype == torch.uint8 and depth.dtype in (torch.int16, torch.uint16)
    assert rgb.dim() == 4 and depth.dim() == 3 and rgb.shape[:3] == depth.shape and tuple(mask.shape) == tuple(depth.shape) + (3,)
    assert rgb.is_contiguous() and depth.is_contiguous() and mask.is_contiguous()
    n, H, W = depth.shape
    k = other_depth.shape[0]
    assert other_rgb.dtype == torch.uint8 and other_mask.dtype == torch.uint8 and other_depth.dtype == depth.dtype
    assert tuple(other_rgb.shape) == (k, H, W, 3) and tuple(other_mask.shape) == (k, H, W, 3) and tuple(other_depth.shape) == (k, H, W)
    assert other_rgb.is_contiguous() and other_depth.is_contiguous() and other_mask.is_contiguous()
    assert plan.dtype == torch.int32 and plan.is_contiguous() and tuple(plan.shape) == (n, PASTE_PLAN_INTS)
    assert extent.dtype == torch.int32 and extent.is_contiguous() and tuple(extent.shape) == (n, 6)
    ph = np.ascontiguousarray(np.asarray(plan_host, np.int32).reshape(n, PASTE_PLAN_INTS))
    dev = rgb.device
    out_rgb, out_depth = torch.empty_like(rgb), torch.empty_like(depth)
    out_label = torch.empty((n, H, W), dtype=torch.int32, device=dev)
    info = torch.empty((n, 4), dtype=torch.int64, device=dev)
    N.check(N.lib().dcl_occlude_paste(N.ptr(rgb), N.ptr(depth), N.ptr(mask), n, H, W, rgb.shape[3], N.ptr(other_rgb),
                                      N.ptr(other_depth), N.ptr(other_mask), k, ph.ctypes.data_as(C.c_void_p), N.ptr(plan),
                                      N.ptr(extent), N.ptr(out_rgb), N.ptr(out_depth), N.ptr(out_label), N.ptr(info),
                                      N.stream()), "occlude_paste")
    return out_rgb, out_depth, out_label, info


def occlude_paste_host(rgb, depth, mask, other_rgb, other_depth, other_mask, plan, extent=None):
    """the host twin of occlude_paste (dcl_occlude_paste_host, plain C++, no GPU call) on numpy arrays; extent None:
    mask_extent_host(mask).  -> (rgb', depth' u16, label' i32, info (n,4) i64)"""
    import numpy as np
    rgb, mask = np.ascontiguousarray(np.asarray(rgb, np.uint8)), np.ascontiguousarray(np.asarray(mask, np.uint8))
    depth = np.ascontiguousarray(np.asarray(depth).astype(np.uint16))
    n, H, W = depth.shape
    o_rgb = np.ascontiguousarray(np.asarray(other_rgb, np.uint8).reshape(-1, H, W, 3))
    o_mask = np.ascontiguousarray(np.asarray(other_mask, np.uint8).reshape(-1, H, W, 3))
    o_depth = np.ascontiguousarray(np.asarray(other_depth).astype(np.uint16).reshape(-1, H, W))
    k = o_depth.shape[0]
    assert rgb.shape[:3] == (n, H, W) and mask.shape == (n, H, W, 3) and o_rgb.shape[0] == k == o_mask.shape[0]
    plan = np.ascontiguousarray(np.asarray(plan, np.int32).reshape(n, PASTE_PLAN_INTS))
    extent = mask_extent_host(mask) if extent is None else np.ascontiguousarray(np.asarray(extent, np.int32).reshape(n, 6))
    out_rgb, out_depth = np.empty_like(rgb), np.empty_like(depth)
    out_label, info = np.empty((n, H, W), np.int32), np.zeros((n, 4), np.int64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    N.check(N.lib().dcl_occlude_paste_host(p(rgb), p(depth), p(mask), n, H, W, rgb.shape[3], p(o_rgb), p(o_depth), p(o_mask), k,
                                           p(plan), p(extent), p(out_rgb), p(out_depth), p(out_label), p(info)),
            "occlude_paste_host")
    return out_rgb, out_depth, out_label, info


def pose_rows64(R0, t_gt, jitter, aug_r):
    """The pose rows dcl_crop_points_posed64 takes (include/dclnet_hip.h: 192 bytes per crop, everything float64 as the LineMOD
    training loader holds it): R0 (n,3,3), t_gt (n,3), jitter (n,3), aug_r (n,3,3) -> (n,192) uint8 numpy array."""
    import numpy as np
    n = len(R0)
    rows = np.zeros(n, POSE_ROW64)
    rows["t_gt"], rows["R0"] = np.asarray(t_gt, np.float64).reshape(n, 3), np.asarray(R0, np.float64).reshape(n, 3, 3)
    rows["j"], rows["A"] = np.asarray(jitter, np.float64).reshape(n, 3), np.asarray(aug_r, np.float64).reshape(n, 3, 3)
    return rows.view(np.uint8).reshape(n, POSE_ROW64_BYTES)


def crop_points_posed64(depth, label, rgb, frame_idx, src, cams, pose, rgb_mean, half_extent, min_valid=128, cap=None):
    """crop_points_posed in the precision of the LineMOD training loader (LM/dataloader_train_LM.py:157-209;
    csrc/crops_train_lm.hip): the re-pose and the grid test in float64, the results rounded to float32 once.  As
    crop_points_posed, except cams (n,6) f32 [cx,cy,fx,fy,scale,post_div], pose (n,192) u8 (pose_rows64), half_extent three
    float64.  -> xyz, rgb, centroid, counts, rot_gt, trans_gt.  No host synchronisation when cap is given."""
    import numpy as np
    N.need_cuda(depth, label, rgb, src, cams, pose)
    assert depth.dtype in (torch.int16, torch.uint16) and label.dtype == torch.int32 and rgb.dtype == torch.uint8
    assert depth.dim() == 3 and label.shape == depth.shape and rgb.dim() == 4 and rgb.shape[:3] == depth.shape
    assert depth.is_contiguous() and label.is_contiguous() and rgb.is_contiguous()
    n = src.shape[0]
    assert src.dtype == torch.int32 and src.is_contiguous() and tuple(src.shape) == (n, 6)
    assert cams.dtype == torch.float32 and cams.is_contiguous() and tuple(cams.shape) == (n, 6)
    assert pose.dtype == torch.uint8 and pose.is_contiguous() and tuple(pose.shape) == (n, POSE_ROW64_BYTES)
    fidx = np.ascontiguousarray(np.asarray(frame_idx, np.int32).reshape(-1))
    assert fidx.shape[0] == n
    f, H, W = depth.shape
    dev = depth.device
    if cap is None:
        bx = src.cpu()
        cap = int(max(1, ((bx[:, 1] - bx[:, 0]).clamp(min=0) * (bx[:, 3] - bx[:, 2]).clamp(min=0)).max().item())) if n else 1
    raw_xyz = torch.empty((n, cap, 3), dtype=torch.float32, device=dev)
    raw_rgb = torch.empty((n, cap, 3), dtype=torch.float32, device=dev)
    xyz = torch.empty((n, cap, 3), dtype=torch.float32, device=dev)
    col = torch.empty((n, cap, 3), dtype=torch.float32, device=dev)
    centroid = torch.empty((n, 3), dtype=torch.float32, device=dev)
    counts = torch.zeros((n, 3), dtype=torch.int32, device=dev)
    rot_gt = torch.empty((n, 3, 3), dtype=torch.float32, device=dev)
    trans_gt = torch.empty((n, 3), dtype=torch.float32, device=dev)
    ws = torch.empty(max(N.query("dcl_crop_points_ws_ints", n, int(cap)), 1), dtype=torch.int32, device=dev)
    mean_a = (C.c_double * 3)(*[float(v) for v in rgb_mean])
    he_a = (C.c_double * 3)(*[float(v) for v in half_extent])
    N.check(N.lib().dcl_crop_points_posed64(N.ptr(depth), N.ptr(label), N.ptr(rgb), f, H, W, rgb.shape[3], n,
                                            fidx.ctypes.data_as(C.c_void_p), N.ptr(src), N.ptr(cams), N.ptr(pose), mean_a, he_a,
                                            int(min_valid), int(cap), N.ptr(raw_xyz), N.ptr(raw_rgb), N.ptr(xyz), N.ptr(col),
                                            N.ptr(centroid), N.ptr(counts), N.ptr(rot_gt), N.ptr(trans_gt), N.ptr(ws), N.stream()),
            "crop_points_posed64")
    return xyz, col, centroid, counts, rot_gt, trans_gt


def crop_repose64_host(points, pose_row, centroid, half_extent=None):
    """the host twin of the float64 re-pose (dcl_crop_repose64_host, plain C++ with the library's -ffp-contract=off): CENTRED
    points (n,3) float32, one pose row (192 bytes, pose_rows64), centroid (3) float32 -> (re-posed points (n,3) float32, R1
    (3,3), t1 (3)), and with half_extent (3 float64) a fourth value: inside (n) bool, the grid test made on the float64 points."""
    import numpy as np
    pts = np.ascontiguousarray(np.asarray(points, np.float32).reshape(-1, 3))
    row = np.ascontiguousarray(np.asarray(pose_row, np.uint8).reshape(-1))
    cen = np.ascontiguousarray(np.asarray(centroid, np.float32).reshape(3))
    assert row.shape[0] == POSE_ROW64_BYTES
    out, R1, t1 = np.empty_like(pts), np.empty((3, 3), np.float32), np.empty(3, np.float32)
    he = None if half_extent is None else (C.c_double * 3)(*[float(v) for v in half_extent])
    inside = None if half_extent is None else np.zeros(pts.shape[0], np.uint8)
    N.check(N.lib().dcl_crop_repose64_host(pts.ctypes.data_as(C.c_void_p), row.ctypes.data_as(C.c_void_p),
                                           cen.ctypes.data_as(C.c_void_p), pts.shape[0], he, out.ctypes.data_as(C.c_void_p),
                                           None if inside is None else inside.ctypes.data_as(C.c_void_p),
                                           R1.ctypes.data_as(C.c_void_p), t1.ctypes.data_as(C.c_void_p)), "crop_repose64_host")
    return (out, R1, t1) if inside is None else (out, R1, t1, inside.astype(bool))


# ------------------------------------------------------------------------------------ training-side kernels
def rulebook_transpose(nbr, n_out, cap_in):
    """inv[k][i] = o for nbr[k][o] = i (csrc/backward.hip); nbr (kvol, cap_out) i32 -> (kvol, cap_in) i32."""
    N.need_cuda(nbr)
    kvol, cap_out = nbr.shape
    inv = torch.empty((kvol, max(cap_in, 1)), dtype=torch.int32, device=nbr.device)
    N.check(N.lib().dcl_rulebook_transpose(N.ptr(nbr), cap_out, N.vp(0), int(n_out), kvol, N.ptr(inv), max(cap_in, 1),
                                           N.stream()), "rulebook_transpose")
    return inv


CONV_PAIRS_SPLIT = N.define("DCL_CONV_PAIRS_SPLIT")  # the pairs of one split of sparse_conv_wgrad_pairs
CONV_PAIRS_HEAD = N.define("DCL_CONV_PAIRS_HEAD")
CONV_WGRAD_FORMS = ("rows", "pairs")


def check_conv_wgrad(value, what="wgrad"):
    if value not in CONV_WGRAD_FORMS:
        raise ValueError('%s must be "rows" or "pairs", got %r' % (what, value))
    return value


class ConvPairs(object):
    """the ordered pair list of a rulebook (conv_pairs): head (CONV_PAIRS_HEAD,) i32 -- count at [k], start at [32 + k], nsplit
    at [60], overflow at [61], an offset's first split at [64 + k]; pair_in / pair_out (max_pairs,) i32; split_tab (max_splits, 4)
    i32 rows (offset, first pair, length, 0).  All on the device; nothing here was read back."""
    __slots__ = ("head", "pair_in", "pair_out", "split_tab", "kvol", "n_out", "n_in", "max_pairs", "max_splits")

    def counts(self):
        """(count (kvol), start (kvol + 1), nsplit, overflow) -- a host read-back, for tests and tools"""
        h = self.head.cpu()
        return h[:self.kvol], h[32:33 + self.kvol], int(h[60]), int(h[61])


def conv_pairs(nbr, n_out, n_in, check=False):
    """The rulebook's pairs in a pinned order (csrc/conv_wgrad_pairs.hip): (k, o) is a pair iff o < n_out and 0 <= nbr[k][o] <
    n_in; offset k's pairs lie at start[k] .. start[k] + count[k] in ascending o, cut into splits of CONV_PAIRS_SPLIT pairs.
    Sized for kvol * min(n_in, n_out) pairs, which holds them all whenever an input row meets an offset at most once (the
    precondition of rulebook_transpose); pairs beyond it are counted, not stored, and check=True reads that count back and
    raises.  No read-back otherwise.  -> ConvPairs"""
    N.need_cuda(nbr)
    assert nbr.dtype == torch.int32 and nbr.dim() == 2 and nbr.is_contiguous()
    kvol, cap = nbr.shape
    n_out, n_in = int(n_out), int(n_in)
    assert 0 <= n_out <= cap and n_in >= 0
    dev = nbr.device
    P = ConvPairs()
    P.kvol, P.n_out, P.n_in = kvol, n_out, n_in
    P.max_pairs = kvol * min(n_in, n_out)
    P.max_splits = N.query("dcl_conv_pairs_max_splits", P.max_pairs, kvol, ctype=C.c_int32)
    wb = N.query("dcl_conv_pairs_ws_bytes", kvol, n_out)
    P.head = torch.empty(CONV_PAIRS_HEAD, dtype=torch.int32, device=dev)
    lists = torch.empty((2, max(P.max_pairs, 1)), dtype=torch.int32, device=dev)
    P.pair_in, P.pair_out = lists[0], lists[1]
    P.split_tab = torch.empty((P.max_splits, 4), dtype=torch.int32, device=dev)
    ws = torch.empty(max(wb // 4, 1), dtype=torch.int32, device=dev)
    N.check(N.lib().dcl_conv_pairs(N.ptr(nbr), cap, kvol, n_out, n_in, P.max_pairs, N.ptr(P.head), N.ptr(P.pair_in),
                                   N.ptr(P.pair_out), N.ptr(P.split_tab), N.ptr(ws), ws.numel() * 4, N.stream()),
            "conv_pairs")
    if check:
        over = int(P.head[61])
        if over:
            raise RuntimeError("conv_pairs: %d pairs beyond the %d that kvol * min(n_in, n_out) holds: an input row meets an "
                               "offset more than once" % (over, P.max_pairs))
    return P


def conv_pairs_host(nbr, n_out, n_in, max_pairs=None):
    """the host twin of conv_pairs (dcl_conv_pairs_host, plain C++, no GPU): nbr (kvol, cap) int32 numpy ->
    dict(head, pair_in, pair_out, split_tab, max_pairs, max_splits) of numpy arrays; entries past the stored pairs and past
    nsplit are left -1"""
    import numpy as np
    nbr = np.ascontiguousarray(nbr, np.int32)
    kvol, cap = nbr.shape
    if max_pairs is None:
        max_pairs = kvol * min(int(n_in), int(n_out))
    ms = N.query("dcl_conv_pairs_max_splits", int(max_pairs), kvol, ctype=C.c_int32)
    head = np.full(CONV_PAIRS_HEAD, -1, np.int32)
    pin, pout = np.full(max(max_pairs, 1), -1, np.int32), np.full(max(max_pairs, 1), -1, np.int32)
    tab = np.full((ms, 4), -1, np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    N.check(N.lib().dcl_conv_pairs_host(vp(nbr), cap, kvol, int(n_out), int(n_in), int(max_pairs), vp(head), vp(pin), vp(pout),
                                        vp(tab)), "conv_pairs_host")
    return dict(head=head, pair_in=pin, pair_out=pout, split_tab=tab, max_pairs=int(max_pairs), max_splits=ms)


def sparse_conv_wgrad_pairs(feat, dout, pairs, cin, cout):
    """dW (kvol, cin, cout) = sum over the listed pairs of feat[pair_in]^T dout[pair_out] on the fp32 MFMA, in the pinned order
    of csrc/conv_wgrad_pairs.hip: inside a split one accumulator per element fed by the pairs ascending, then an offset's splits
    ascending.  A function of the list and the rows it names alone; the same bits on every call.  Every element is written."""
    N.need_cuda(feat, dout)
    cin, cout = int(cin), int(cout)
    feat, dout = N.f32c(feat), N.f32c(dout)
    assert tuple(feat.shape) == (feat.shape[0], cin) and feat.shape[0] >= pairs.n_in
    assert tuple(dout.shape) == (dout.shape[0], cout) and dout.shape[0] >= pairs.n_out
    dev = feat.device
    dW = torch.empty((pairs.kvol, cin, cout), dtype=torch.float32, device=dev)
    partial = torch.empty(pairs.max_splits * cin * cout, dtype=torch.float32, device=dev)
    N.check(N.lib().dcl_sparse_conv_wgrad_pairs(N.ptr(feat), pairs.n_in, N.ptr(dout), pairs.n_out, cin, cout, pairs.kvol,
                                                N.ptr(pairs.head), N.ptr(pairs.pair_in), N.ptr(pairs.pair_out),
                                                N.ptr(pairs.split_tab), pairs.max_splits, N.ptr(partial), N.ptr(dW),
                                                N.stream()), "sparse_conv_wgrad_pairs")
    return dW


CONV_FWD_FORMS = ("tiles", "compact")
# the (cin, cout) of the DILATING (non-subm) backbone layers among 32 -> 32, 64 -> 64 and 128 -> 128 on which
# tools/bench_conv_fwd.py measured "compact" faster than "tiles" with disjoint block ranges on the layers of BOTH backbones
# (profiles/conv_fwd_compact.txt); Network(train_conv_fwd="compact") goes by this table.  EMPTY as measured: the compact form
# is 1.35-2.2 times slower than "tiles" on all three widths, so the switch changes no layer until the kernel earns a width
CONV_FWD_COMPACT_WIDTHS = frozenset()


def check_conv_fwd(value, what="fwd"):
    if value not in CONV_FWD_FORMS:
        raise ValueError('%s must be "tiles" or "compact", got %r' % (what, value))
    return value


def conv_fwd_form(cin, cout, subm, train_conv_fwd="compact"):
    """the forward form of a convolution of these widths under Network(train_conv_fwd=): by the widths and the kind of the
    layer alone, never by the data.  Subm layers and the stem always stay with "tiles"."""
    compact = check_conv_fwd(train_conv_fwd, "train_conv_fwd") == "compact"
    return "compact" if compact and not subm and (int(cin), int(cout)) in CONV_FWD_COMPACT_WIDTHS else "tiles"


def sparse_conv_compact(feat, nbr, n_out, W, subm):
    """out (n_out, cout) = sum_k sum_ci feat[nbr[k][o]][ci] W[k][ci][co] on csrc/conv_fwd_compact.hip: only the present (row,
    offset) pairs reach the matrix pipe.  An entry of nbr is a neighbour iff it names one of feat's rows.  Pinned order
    (csrc/conv_fwd_compact.h): per present offset a chain of its own over ci ascending, added with one fp32 add, offsets in the
    forward's visiting order; the same bits on every call.  Every element is written.  feat and W may be views that start off
    a 16-byte boundary (contiguous rows): the kernel then loads float by float, the same bits."""
    N.need_cuda(feat, nbr, W)
    assert nbr.dtype == torch.int32 and nbr.dim() == 2 and nbr.is_contiguous()
    kvol, cap = nbr.shape
    cin, cout = int(W.shape[-2]), int(W.shape[-1])
    n_out = int(n_out)
    assert feat.dtype == torch.float32 and W.dtype == torch.float32 and feat.is_contiguous() and W.is_contiguous()
    assert feat.dim() == 2 and feat.shape[1] == cin and W.numel() == kvol * cin * cout and 0 <= n_out <= cap
    out = torch.empty((n_out, cout), dtype=torch.float32, device=feat.device)
    N.check(N.lib().dcl_sparse_conv_fwd_compact(N.ptr(feat), int(feat.shape[0]), N.ptr(nbr), cap, n_out, N.ptr(W), cin, cout, kvol,
                                                int(bool(subm)), N.ptr(out), N.stream()), "sparse_conv_fwd_compact")
    return out


def sparse_conv_compact_host(feat, nbr, n_out, W, subm, n_in=None):
    """the host twin of sparse_conv_compact (dcl_sparse_conv_fwd_compact_host, plain C++, no GPU) on numpy arrays: the same
    steps, literally.  n_in: the rows of feat that count (default: all of them)."""
    import numpy as np
    nbr = np.ascontiguousarray(nbr, np.int32)
    kvol, cap = nbr.shape
    cin, cout = int(W.shape[-2]), int(W.shape[-1])
    feat = np.ascontiguousarray(feat, np.float32)
    W = np.ascontiguousarray(np.asarray(W, np.float32).reshape(kvol, cin, cout))
    n_in = feat.shape[0] if n_in is None else int(n_in)
    assert feat.ndim == 2 and feat.shape[1] == cin and n_in <= feat.shape[0] and int(n_out) <= cap
    out = np.full((int(n_out), cout), np.nan, np.float32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    N.check(N.lib().dcl_sparse_conv_fwd_compact_host(vp(feat), n_in, vp(nbr), cap, int(n_out), vp(W), cin, cout, kvol,
                                                     int(bool(subm)), vp(out)), "sparse_conv_fwd_compact_host")
    return out


CONV_DGRAD_FORMS = ("conv", "direct")
# the (cin, cout) of the backbone layers on which tools/bench_conv_dgrad.py measured "direct" faster than "conv" with disjoint
# block ranges on the layers of BOTH backbones (profiles/conv_dgrad.txt); Network(train_conv_dgrad="direct") goes by this table
CONV_DGRAD_DIRECT_WIDTHS = frozenset(((16, 32), (128, 256)))


def check_conv_dgrad(value, what="dgrad"):
    if value not in CONV_DGRAD_FORMS:
        raise ValueError('%s must be "conv" or "direct", got %r' % (what, value))
    return value


def conv_dgrad_form(cin, cout, train_conv_dgrad="direct"):
    """the dgrad of a convolution of these widths under Network(train_conv_dgrad=): by widths alone, never by the data"""
    direct = check_conv_dgrad(train_conv_dgrad, "train_conv_dgrad") == "direct"
    return "direct" if direct and (int(cin), int(cout)) in CONV_DGRAD_DIRECT_WIDTHS else "conv"


def sparse_conv_dgrad(dout, inv, n_in, W):
    """dX (n_in, cin) = sum_k sum_co dout[inv[k][i]][co] W[k][ci][co] on csrc/conv_dgrad.hip: inv (kvol, cap_in) from
    rulebook_transpose, W (kvol, cin, cout) as registered -- no transposed copy.  An entry of inv is a neighbour iff it names one
    of dout's rows.  Pinned order: one accumulator per element from +0, offsets ascending, channels ascending inside an offset;
    the same bits on every call, whatever n_in, cap_in or the other rows.  Every element is written."""
    N.need_cuda(dout, inv, W)
    assert inv.dtype == torch.int32 and inv.dim() == 2 and inv.is_contiguous()
    kvol, cap_in = inv.shape
    cin, cout = int(W.shape[-2]), int(W.shape[-1])
    n_in = int(n_in)
    dout = N.f32c(dout)
    W = N.f32c(W.reshape(kvol, cin, cout))
    assert dout.dim() == 2 and dout.shape[1] == cout and 0 <= n_in <= cap_in
    dx = torch.empty((n_in, cin), dtype=torch.float32, device=dout.device)
    N.check(N.lib().dcl_sparse_conv_dgrad(N.ptr(dout), int(dout.shape[0]), N.ptr(inv), cap_in, n_in, N.ptr(W), cin, cout, kvol,
                                          N.ptr(dx), N.stream()), "sparse_conv_dgrad")
    return dx


def sparse_conv_dgrad_host(dout, inv, n_in, W, n_out=None):
    """the host twin of sparse_conv_dgrad (dcl_sparse_conv_dgrad_host, plain C++, no GPU) on numpy arrays: the same chain,
    literally.  n_out: the rows of dout that count (default: all of them)."""
    import numpy as np
    inv = np.ascontiguousarray(inv, np.int32)
    kvol, cap_in = inv.shape
    cin, cout = int(W.shape[-2]), int(W.shape[-1])
    dout = np.ascontiguousarray(dout, np.float32)
    W = np.ascontiguousarray(np.asarray(W, np.float32).reshape(kvol, cin, cout))
    n_out = dout.shape[0] if n_out is None else int(n_out)
    assert dout.ndim == 2 and dout.shape[1] == cout and n_out <= dout.shape[0]
    dx = np.full((int(n_in), cin), np.nan, np.float32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    N.check(N.lib().dcl_sparse_conv_dgrad_host(vp(dout), n_out, vp(inv), cap_in, int(n_in), vp(W), cin, cout, kvol, vp(dx)),
            "sparse_conv_dgrad_host")
    return dx


def sparse_conv_backward(feat, W, dout, nbr, n_out, subm, need_dx=True, wgrad="rows", dgrad="conv"):
    """indice_conv_backward_fp32 (spconv_ops.h:351-438): -> (d_feat (V_in,Cin) or None, dW (kvol,Cin,Cout)).  wgrad: the form
    of the weight gradient -- "rows" (default; csrc/backward.hip walks every output row of every offset) or "pairs" (conv_pairs +
    sparse_conv_wgrad_pairs: only the pairs that exist, in a pinned order).  dgrad: the form of the input gradient -- "conv"
    (default: the forward dispatcher on the transposed rulebook and a transposed copy of W) or "direct" (sparse_conv_dgrad on
    the transposed rulebook and W as it is; always the new kernel, whatever the widths).  Neither switch touches the other's
    result."""
    check_conv_wgrad(wgrad)
    check_conv_dgrad(dgrad)
    N.need_cuda(feat, W, dout, nbr)
    kvol, cap = nbr.shape
    cin, cout = W.shape[-2], W.shape[-1]
    n_in = feat.shape[0]
    dev = feat.device
    dout = dout.contiguous()
    dx = None
    if wgrad == "pairs":                                           # (the list lives for this call only)
        dW = sparse_conv_wgrad_pairs(feat, dout, conv_pairs(nbr, n_out, n_in), cin, cout)
    else:
        dW = torch.zeros((kvol, cin, cout), dtype=torch.float32, device=dev)
        if n_out > 0 and n_in > 0:                                 # (no input rows: no pair, dW = 0 -- and no feat pointer)
            splits = N.query("dcl_sparse_conv_wgrad_splits", int(n_out), what="wgrad_splits", ctype=C.c_int32)
            partial = torch.empty(splits * kvol * cin * cout, dtype=torch.float32, device=dev)
            N.check(N.lib().dcl_sparse_conv_wgrad(N.ptr(feat), N.ptr(nbr), cap, int(n_out), N.ptr(dout), cin, cout, kvol,
                                                  N.ptr(partial), N.ptr(dW), N.stream()), "sparse_conv_wgrad")
    if need_dx:
        if n_in == 0 or n_out == 0:
            dx = torch.zeros((n_in, cin), dtype=torch.float32, device=dev)
        elif dgrad == "direct":
            dx = sparse_conv_dgrad(dout[:n_out], rulebook_transpose(nbr, n_out, n_in), n_in, W)
        else:
            inv = rulebook_transpose(nbr, n_out, n_in)
            Wt = W.reshape(kvol, cin, cout).transpose(1, 2).contiguous()          # per-offset W^T: (kvol, Cout, Cin)
            dx = sparse_conv(dout, inv, n_in, Wt, subm)
    return dx, dW


def sparse_avgpool_backward(dout, nbr, n_out, n_in, rf):
    """indice_avgpool_backward_fp32 (avgpool.cu:178-206) -> d_feat (V_in, C)."""
    N.need_cuda(dout, nbr, rf)
    c = dout.shape[1]
    din = torch.zeros((n_in, c), dtype=torch.float32, device=dout.device)
    if n_in == 0 or n_out == 0:
        return din
    inv = rulebook_transpose(nbr, n_out, n_in)
    N.check(N.lib().dcl_sparse_avgpool_bwd(N.ptr(dout.contiguous()), N.ptr(inv), inv.shape[1], int(n_in), N.ptr(rf), c,
                                           nbr.shape[0], N.ptr(din), N.stream()), "sparse_avgpool_bwd")
    return din


def three_interpolate_grad_sp(grad_out, idx, weight, m):
    """three_interpolate_grad_wrapper of libs/pointnet_sp -> grad_points (m, C): every row's contributions added in ascending
    flat position of idx (csrc/readout_grad.hip) -- numpy.add.at on float32, the same bits on every call.  grad_out (n, C) with
    unit channel stride and a row stride >= C (a column block of a wider tensor) is read where it lies."""
    N.need_cuda(grad_out, idx, weight)
    n, c = grad_out.shape
    m = int(m)
    if grad_out.dtype == torch.float32 and grad_out.stride(1) == 1 and grad_out.stride(0) >= c:
        stride = grad_out.stride(0)
    else:
        grad_out, stride = N.f32c(grad_out), c
    idx, weight = N.i32c(idx), N.f32c(weight)
    assert tuple(idx.shape) == (n, 3) and tuple(weight.shape) == (n, 3)
    gp = torch.empty((m, c), dtype=torch.float32, device=grad_out.device)
    ws, nb = _pn_grad_ws("dcl_three_interpolate_grad_sp_ws_bytes", (c, n, m), grad_out.device)
    N.check(N.lib().dcl_three_interpolate_grad_sp_ordered(c, n, m, N.ptr(grad_out), stride, N.ptr(idx),
                                                          N.ptr(weight), N.ptr(gp), N.ptr(ws), nb, N.stream()),
            "three_interpolate_grad_sp_ordered")
    return gp


def three_interpolate_grad_sp_atomic(grad_out, idx, weight, m):
    """The same gradient by the reference's atomic scatter (interpolate_gpu.cu:124-148; the order of a row's adds is
    whatever the hardware serves): what tools/bench_readout_grad.py and the tests compare the ordered form with."""
    N.need_cuda(grad_out, idx, weight)
    n, c = grad_out.shape
    gp = torch.zeros((m, c), dtype=torch.float32, device=grad_out.device)
    N.check(N.lib().dcl_three_interpolate_grad_sp(c, n, m, N.ptr(grad_out.contiguous()), N.ptr(idx), N.ptr(weight), N.ptr(gp),
                                                  N.stream()), "three_interpolate_grad_sp")
    return gp


def _pn_grad_ws(sym, sizes, dev):
    nbytes = N.query(sym, *sizes)
    return torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev), nbytes


def _pn_grad_points(grad_points, shape, dev):
    if grad_points is None:
        return torch.zeros(shape, dtype=torch.float32, device=dev)
    assert tuple(grad_points.shape) == shape and grad_points.dtype == torch.float32 and grad_points.is_contiguous()
    return grad_points


def group_points_grad(grad_out, idx, n, grad_points=None):
    """group_points_grad_wrapper of libs/pointnet_lib: grad_out (B,C,npoint,nsample), idx (B,npoint,nsample) i32 ->
    grad_points (B,C,n).  Adds into `grad_points` when one is given (zeros otherwise); deterministic (include/dclnet_hip.h)."""
    N.need_cuda(grad_out, idx, grad_points)
    grad_out, idx = N.f32c(grad_out), N.i32c(idx)
    B, c, npoint, ns = grad_out.shape
    assert tuple(idx.shape) == (B, npoint, ns)
    gp = _pn_grad_points(grad_points, (B, c, int(n)), grad_out.device)
    ws, nb = _pn_grad_ws("dcl_group_points_grad_ws_bytes", (B, c, int(n), npoint, ns), grad_out.device)
    N.check(N.lib().dcl_group_points_grad(B, c, int(n), npoint, ns, N.ptr(grad_out), N.ptr(idx), N.ptr(gp), N.ptr(ws),
                                          nb, N.stream()), "group_points_grad")
    return gp


def gather_points_grad(grad_out, idx, n, grad_points=None):
    """gather_points_grad_wrapper: grad_out (B,C,npoint), idx (B,npoint) i32 -> grad_points (B,C,n) (adds into it)."""
    N.need_cuda(grad_out, idx, grad_points)
    grad_out, idx = N.f32c(grad_out), N.i32c(idx)
    B, c, npoint = grad_out.shape
    assert tuple(idx.shape) == (B, npoint)
    gp = _pn_grad_points(grad_points, (B, c, int(n)), grad_out.device)
    ws, nb = _pn_grad_ws("dcl_gather_points_grad_ws_bytes", (B, c, int(n), npoint), grad_out.device)
    N.check(N.lib().dcl_gather_points_grad(B, c, int(n), npoint, N.ptr(grad_out), N.ptr(idx), N.ptr(gp), N.ptr(ws),
                                           nb, N.stream()), "gather_points_grad")
    return gp


def three_interpolate_grad(grad_out, idx, weight, m, grad_points=None):
    """three_interpolate_grad_wrapper of libs/pointnet_lib: grad_out (B,C,n), idx (B,n,3) i32, weight (B,n,3) ->
    grad_points (B,C,m) (adds into it).  No weight gradient, as in the reference."""
    N.need_cuda(grad_out, idx, weight, grad_points)
    grad_out, idx, weight = N.f32c(grad_out), N.i32c(idx), N.f32c(weight)
    B, c, n = grad_out.shape
    assert tuple(idx.shape) == (B, n, 3) and tuple(weight.shape) == (B, n, 3)
    gp = _pn_grad_points(grad_points, (B, c, int(m)), grad_out.device)
    ws, nb = _pn_grad_ws("dcl_three_interpolate_grad_ws_bytes", (B, c, n, int(m)), grad_out.device)
    N.check(N.lib().dcl_three_interpolate_grad(B, c, n, int(m), N.ptr(grad_out), N.ptr(idx), N.ptr(weight), N.ptr(gp),
                                               N.ptr(ws), nb, N.stream()), "three_interpolate_grad")
    return gp


def voxelize_bp(d_out, map_rule, n_points, mode=4):
    """PG_OP.voxelize_bp (pointgroup_ops.py:65-73) -> d_feats (N, C)."""
    N.need_cuda(d_out, map_rule)
    M, c = d_out.shape
    d_feats = torch.zeros((n_points, c), dtype=torch.float32, device=d_out.device)
    N.check(N.lib().dcl_voxelize_bp(N.ptr(d_out.contiguous()), N.ptr(map_rule), N.ptr(d_feats), M, map_rule.shape[1] - 1, c,
                                    int(mode == 4), N.stream()), "voxelize_bp")
    return d_feats


# ------------------------------------------------------------------------------------ Linear + ReLU stacks: training side
WGRAD_ROWS = N.define("DCL_WGRAD_ROWS")             # the rows of one split of linear_wgrad / relu_bwd


def linear_wgrad_splits(M):
    """how many row splits linear_wgrad / relu_bwd cut M rows into: max(1, ceil(M / WGRAD_ROWS)), a function of M alone
    (needs no GPU)"""
    return N.query("dcl_linear_wgrad_splits", int(M), ctype=C.c_int32)


def _rows2d(t, what):
    assert t.dim() == 2 and t.dtype == torch.float32 and t.is_cuda, "%s: a 2-D float32 CUDA tensor" % what
    assert t.stride(1) == 1 or t.shape[1] == 1, "%s: rows must be dense" % what
    return t


def linear_wgrad(a, b, out=None):
    """The weight gradient of a per-point linear layer (csrc/linear_bwd.hip): dW (P,Q) = a^T b = sum_j a[j,:]^T b[j,:] with
    a = dZ (M,P) and b = the layer's input (M,Q) -- the Conv1d weight's own (out, in) layout.  linear()'s conventions: 2-D
    tensors whose rows may be strided, `out=dW0[:, 3:]` writes a column block of a wider gradient in place.  Own fp32 MFMA
    kernel with a pinned order (rows ascending inside splits of WGRAD_ROWS rows, splits ascending): no atomics, the same bits
    on every call and for every pitch and alignment.  No vendor library."""
    N.need_cuda(a, b)
    _rows2d(a, "a")
    _rows2d(b, "b")
    M, P = a.shape
    assert b.shape[0] == M, "a and b must have the same rows"
    Q = b.shape[1]
    if out is None:
        out = torch.empty((P, Q), dtype=torch.float32, device=a.device)
    _rows2d(out, "out")
    assert tuple(out.shape) == (P, Q)
    partial = torch.empty(linear_wgrad_splits(M) * P * Q, dtype=torch.float32, device=a.device)
    N.check(N.lib().dcl_linear_wgrad(N.ptr(a), _pitch(a), N.ptr(b), _pitch(b), int(M), int(P), int(Q),
                                     N.ptr(partial), N.ptr(out), _pitch(out), N.stream()), "linear_wgrad")
    return out


WGRAD_FORMS = ("fp32", "split")
# {(P, Q): the fewest rows M} of the weight gradients that Network(train_wgrad="split") / Refiner(train_wgrad="split") send to
# linear_wgrad_split: a shape is listed only where tools/bench_linear_wgrad.py measured every block of the split kernel below
# every block of linear_wgrad (disjoint ranges, profiles/linear_wgrad_split.txt), from the fewest rows at which it was measured.
# That is every wide shape of the 32 x 1024 / 1024 step (split / fp32 time 0.76-0.85) and of the refiner at 20 / 32 x 1024
# (0.65-0.83); the refiner's xyz block (512, 3) is 10 % SLOWER on the split kernel and is not listed.  A shape outside the
# table keeps linear_wgrad.
WGRAD_SPLIT_SHAPES = {(64, 256): 32768, (128, 128): 32768, (128, 256): 32768, (256, 256): 32768, (1024, 480): 32768,
                      (512, 256): 20480, (512, 512): 20480, (1024, 512): 20480}


def check_linear_wgrad(value, what="train_wgrad"):
    if value not in WGRAD_FORMS:
        raise ValueError('%s must be "fp32" or "split", got %r' % (what, value))
    return value


def linear_wgrad_form(M, P, Q, train_wgrad="split"):
    """the weight-gradient form of a (P, Q) layer over M rows under train_wgrad=: by the shape alone (WGRAD_SPLIT_SHAPES), never
    by the data"""
    if check_linear_wgrad(train_wgrad) == "fp32":
        return "fp32"
    min_rows = WGRAD_SPLIT_SHAPES.get((int(P), int(Q)))
    return "split" if min_rows is not None and int(M) >= min_rows else "fp32"


def linear_wgrad_split_units(M):
    """the a-priori error bound of linear_wgrad_split over M rows in units of 2^-24 sum_j |a_jp| |b_jq| (include/dclnet_hip.h):
    one rounding per piece product of a split's rows, one per added split, 32 for the dropped products and the pieces' sizes"""
    return 6 * WGRAD_ROWS + linear_wgrad_splits(M) + 32


def linear_wgrad_split(a, b, out=None):
    """linear_wgrad on the bf16 matrix pipe (csrc/linear_wgrad_split.hip): the same arguments, conventions and pinned order
    (splits of WGRAD_ROWS rows, 16-row chunks ascending inside a split, splits ascending; the same bits on every call and for
    every pitch and alignment), every operand split in the kernel into three bf16 pieces and a product accumulated as its six
    piece products in fp32 -- fp32-sized errors (linear_wgrad_split_units), not linear_wgrad's bits.  Values of magnitude
    >= 3.3962e38, +-inf and NaN are not supported: they turn their whole row or column of dW into NaN.  No vendor library."""
    N.need_cuda(a, b)
    _rows2d(a, "a")
    _rows2d(b, "b")
    M, P = a.shape
    assert b.shape[0] == M, "a and b must have the same rows"
    Q = b.shape[1]
    if out is None:
        out = torch.empty((P, Q), dtype=torch.float32, device=a.device)
    _rows2d(out, "out")
    assert tuple(out.shape) == (P, Q)
    partial = torch.empty(linear_wgrad_splits(M) * P * Q, dtype=torch.float32, device=a.device)
    N.check(N.lib().dcl_linear_wgrad_split(N.ptr(a), _pitch(a), N.ptr(b), _pitch(b), int(M), int(P), int(Q),
                                           N.ptr(partial), N.ptr(out), _pitch(out), N.stream()), "linear_wgrad_split")
    return out


def linear_wgrad_as(form, a, b, out=None):
    """linear_wgrad (form "fp32") or linear_wgrad_split (form "split")"""
    return (linear_wgrad_split if check_linear_wgrad(form, "form") == "split" else linear_wgrad)(a, b, out=out)


def relu_bwd(h, g=None, roww=None, gpool=None, rows_per_crop=None, out=None):
    """ReLU mask + bias gradient of a Linear + ReLU layer whose OUTPUT is h (M,P) (csrc/linear_bwd.hip) -> (dz (M,P), db (P,)).
    relu_bwd(h, g): dz = where(h > 0, g, 0); `out=g` masks the arriving gradient in place.
    relu_bwd(h, roww=w, gpool=G, rows_per_crop=n): the pooled last layer, whose output went into shared[crop] = sum_j w[j] h[j]:
    dz[j] = where(h[j] > 0, w[j] * G[j // n], 0) with w (M,) and G (crops,P) the gradient of `shared`; `out=h` overwrites h.
    db = dz.sum(0) in linear_wgrad's order (rows ascending inside a split, splits ascending): the same bits on every call."""
    N.need_cuda(h, g, roww, gpool)
    _rows2d(h, "h")
    M, P = h.shape
    if out is None:
        out = torch.empty((M, P), dtype=torch.float32, device=h.device)
    _rows2d(out, "out")
    assert tuple(out.shape) == (M, P)
    if g is not None:
        assert roww is None and gpool is None, "either g or (roww, gpool, rows_per_crop)"
        _rows2d(g, "g")
        assert tuple(g.shape) == (M, P)
        form = (N.ptr(g), _pitch(g), None, None, 0, 0)
    else:
        assert roww is not None and gpool is not None and rows_per_crop, "either g or (roww, gpool, rows_per_crop)"
        _rows2d(gpool, "gpool")
        rows_per_crop = int(rows_per_crop)
        assert roww.dtype == torch.float32 and roww.is_contiguous() and roww.numel() == M
        assert gpool.shape[1] == P and gpool.shape[0] * rows_per_crop >= M
        form = (None, 0, N.ptr(roww), N.ptr(gpool), _pitch(gpool), rows_per_crop)
    partial = torch.empty(linear_wgrad_splits(M) * P, dtype=torch.float32, device=h.device)
    db = torch.empty(P, dtype=torch.float32, device=h.device)
    N.check(N.lib().dcl_relu_bwd(N.ptr(h), _pitch(h), *form, int(M), int(P), N.ptr(out), _pitch(out),
                                 N.ptr(partial), N.ptr(db), N.stream()), "relu_bwd")
    return out, db


def linear_pool_dma(x, Wt, bias, roww, relu=True, part=None, rows_per_crop=None, w_stride=0):
    """linear_pool on the fp32-MFMA core whatever the launch size and whether or not the weight has been prepared: what a
    training forward calls, whose weights change every step (no bf16 pieces to keep in step)."""
    N.need_cuda(x, Wt, roww)
    M, K = x.shape
    return _linear_pool(N.lib().dcl_linear_pool_fwd, "linear_pool_fwd", x, (N.ptr(Wt), _pitch(Wt)), K, Wt.shape[1],
                        bias, roww, relu, part, rows_per_crop, w_stride)
