"""Every kernel family inside poisoned guard bands (tests/guard_arena.py): which memory a kernel touches, not what it computes.

Each entry of CASES builds exactly-sized operands (no prefix view of a larger tensor), and guarded() runs the op plain, then once
under each poison with every input, output and scratch buffer between guard bands.  A damaged band, a written input or an output
bit that differs between the three runs fails the case.  Shapes are the smallest with a ragged last tile / row group / crop,
one on each side of every launcher switch; kernel variants are chosen through the diagnostic library's hooks, as
tests/test_gpu_ops.py does.  Nothing here has a tolerance."""
import numpy as np
import pytest
import torch

import guard_arena as GA

pytestmark = pytest.mark.gpu

CASES = {}            # name -> (builder(dcl) -> dict(fn, inputs[, inplace, valid]), hooks ((name, value, value afterwards), ...))


def case(name, hooks=()):
    def register(build):
        assert name not in CASES, name
        CASES[name] = (build, tuple(hooks))
        return build
    return register


def gen(*key):
    import zlib
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def randn(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).cuda()


def cuda(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def fresh(dcl, *shape, dtype=torch.float32):
    """an output the caller hands to an op: allocated like the op's own buffers (from the arena in a guarded run)"""
    return dcl.ops.torch.empty(shape, dtype=dtype, device="cuda")


def run_case(dcl, request, name, compare=True, entered=None):
    """one entry of CASES: with compare, guarded(); without, its "nan" pass alone (the coverage census of
    tests/test_gpu_guarded_paths.py)"""
    build, hooks = CASES[name]
    lib = None
    if hooks:
        import test_gpu_ops as TG
        lib = TG.enter_diag(dcl, request)
    k = build(dcl)
    mods = GA.allocating_modules(dcl)
    try:
        for hook, on, _ in hooks:
            getattr(lib, hook)(on)
        if lib is not None:
            lib.dcl_debug_launch_census_reset()
        if compare:
            GA.guarded(k["fn"], k["inputs"], valid=k.get("valid"), inplace=k.get("inplace", ()), modules=mods,
                       capacity=k.get("capacity"), entered=entered)
        else:
            GA.poison_pass(k["fn"], k["inputs"], "nan", modules=mods, capacity=k.get("capacity"), entered=entered)
        if "kernels" in k:
            check_kernels(lib, *k["kernels"])
    finally:
        for hook, _, off in hooks:
            getattr(lib, hook)(off)


def check_kernels(lib, wanted, family, allowed=()):
    """the launch census of the diagnostic library since the hooks were set: every kernel of `wanted` (name prefixes) ran, and no
    kernel of `family` other than those and `allowed` -- the hook selected the variant the case is named after"""
    import test_kernel_census as TC
    seen = {name: n for name, n in TC.census(lib).items() if n}
    for w in wanted:
        assert any(name.startswith(w) for name in seen), (w, sorted(seen))
    other = [name for name in seen if name.startswith(family) and not any(name.startswith(w) for w in tuple(wanted) + tuple(allowed))]
    assert not other, (other, wanted)


# ==================================================================================================== dense GEMM cores
# csrc/linear_dma.hip: tile 1, 2 = 128-row tiles, 3, 4, 5 = 64-row tiles (4, 5 split K over 2 / 4 waves), 0 = the launcher's choice
LINEAR_TILES = {0: 64, 1: 128, 2: 128, 3: 64, 4: 64, 5: 64}


def _linear_operands(M, K, n, tag):
    g = gen("linear", tag, M, K, n)
    return randn(g, M, K), randn(g, K, n, scale=0.05), randn(g, n)


for _tile, _bm in LINEAR_TILES.items():
    for _M in (1, _bm - 1, _bm + 1):
        @case("linear/tile%d/M%d" % (_tile, _M), hooks=[("dcl_debug_linear_tile", _tile, 0)])
        def _(dcl, M=_M, tile=_tile):
            x, Wt, bias = _linear_operands(M, 96, 72, tile)              # 3 chunks of K, columns end inside a 64-column tile
            return dict(fn=lambda x, Wt, bias: (dcl.ops.linear(x, Wt, bias, True), dcl.ops.linear(x, Wt)), inputs=[x, Wt, bias])


for _bias, _relu in ((True, True), (False, False)):
    @case("linear/out_column_block/bias%d" % _bias)
    def _(dcl, with_bias=_bias, relu=_relu):
        M, K, n = 129, 64, 40
        g = gen("linear block", with_bias)
        wide, Wt, bias = randn(g, M, K + 40), randn(g, K, n, scale=0.05), randn(g, n)
        buf = torch.full((M, n + 24), 7.0).cuda()
        return dict(fn=lambda x, Wt, bias, out: dcl.ops.linear(x, Wt, bias if with_bias else None, relu, out=out),
                    inputs=[wide[:, 8:8 + K], Wt, bias, buf[:, 16:16 + n]], inplace=(3,))


@case("linear_lt/K_not_32")
def _(dcl):
    x, Wt, bias = _linear_operands(37, 48, 9, "lt")                     # K no multiple of 32: the vendor path of linear()
    return dict(fn=lambda x, Wt, bias: dcl.ops.linear(x, Wt, bias, True), inputs=[x, Wt, bias])


def _split_shapes():
    return [(M, K, n) for M in (1, 255, 257) for K in (16, 48) for n in (96, 160)]


for _M, _K, _n in _split_shapes():
    @case("linear_split/%dx%dx%d" % (_M, _K, _n))
    def _(dcl, M=_M, K=_K, n=_n):
        x, Wt, bias = _linear_operands(M, K, n, "split")
        g = gen("split extra", M, K, n)
        roww = torch.rand(M, generator=g).cuda()
        w3, b3 = randn(g, n, 1), randn(g, 1)

        def fn(x, Wt, bias, roww, w3, b3):
            sw = dcl.ops.SplitWeight(Wt)
            out = [dcl.ops.linear_split(x, sw, bias, True), dcl.ops.linear_split(x, sw), dcl.ops.linear_split_pool(x, sw, bias, roww)]
            if n <= 128:
                out.append(dcl.ops.linear_split_rowdot(x, sw, bias, w3, b3))
            return out
        return dict(fn=fn, inputs=[x, Wt, bias, roww, w3, b3])


@case("linear_split/out_column_block")
def _(dcl):
    M, K, n = 257, 48, 96
    g = gen("split block")
    wide, Wt, bias = randn(g, M, K + 40), randn(g, K, n, scale=0.05), randn(g, n)
    buf = torch.full((M, n + 24), 7.0).cuda()
    return dict(fn=lambda x, Wt, bias, out: dcl.ops.linear_split(x, dcl.ops.SplitWeight(Wt), bias, True, out=out),
                inputs=[wide[:, 8:8 + K], Wt, bias, buf[:, 16:16 + n]], inplace=(3,))


for _n in (96, 160):
    @case("linear_split_vpieces/n%d" % _n)
    def _(dcl, n=_n):
        # rows = keys: every crop a multiple of 256 rows (the entry point's contract), two crops; the pieces go into a scratch
        # of attention_planes' size for a call whose crops all take the split kernel: csrc/dense.hip, kAttnTileBytes = 73728 bytes
        # per 32-key tile and crop
        b, nk, K = 2, 256, 48
        g = gen("vpieces", n)
        x, Wt, bias = randn(g, b * nk, K), randn(g, K, n, scale=0.05), randn(g, n)

        def fn(x, Wt, bias):
            planes = dcl.ops.torch.empty(b * (nk // 32) * 73728, dtype=torch.uint8, device=x.device)      # as attention_planes hands it out
            return dcl.ops.linear_split_vpieces(x, dcl.ops.SplitWeight(Wt), bias, planes, nk, relu=True)

        # csrc/linear_split.hip (EPI = 3): 16-key half tile ht = crop * nk / 16 + .. of 3 * 320 * 32 bytes, [piece][channel][slot][16
        # bytes]; the GEMM writes the channels below n, the attention's piece pass the others and the K tiles behind them
        def valid(outs):
            v = outs[0][:b * (nk // 16) * 30720].view(b * (nk // 16), 3, 320, 32)
            return [v[:, :, :n].contiguous()]
        return dict(fn=fn, inputs=[x, Wt, bias], valid=valid)


for _M in (127, 129, 300):
    @case("linear_pool_rowdot/M%d" % _M)
    def _(dcl, M=_M):
        g = gen("pool", M)
        x, Wt, bias = randn(g, M, 128), randn(g, 128, 96, scale=0.05), randn(g, 96)
        roww, w3, b3 = torch.rand(M, generator=g).cuda(), randn(g, 96, 1), randn(g, 1)
        return dict(fn=lambda x, Wt, bias, roww, w3, b3: (dcl.ops.linear_pool(x, Wt, bias, roww),
                                                         dcl.ops.linear_rowdot(x, Wt, bias, w3, b3)),
                    inputs=[x, Wt, bias, roww, w3, b3])


@case("linear_pool/rows_per_crop")
def _(dcl):
    b, n1, n2 = 3, 128, 256                                             # a direction's block of conf_softmax's (b, n1 + n2) weights
    g = gen("pool crops")
    x, Wt, bias = randn(g, b * n2, 64), randn(g, 64, 260, scale=0.05), randn(g, 260)
    w = torch.rand(b, n1 + n2, generator=g).cuda()
    return dict(fn=lambda x, Wt, bias, w: dcl.ops.linear_pool(x, Wt, bias, w[:, n1:], True, None, n2, n1 + n2), inputs=[x, Wt, bias, w])


for _M in (37, 257):
    @case("linear_group/M%d" % _M)
    def _(dcl, M=_M):
        g = gen("group", M)
        H = randn(g, M, 128 + 8)[:, 8:]                                 # a column block: 32-byte offset
        fuse = torch.full((M, 160), 7.0).cuda()
        W1, b1, W2, b2 = randn(g, 64, 96, scale=0.05), randn(g, 96), randn(g, 64, 64, scale=0.05), randn(g, 64)
        x3, W3 = randn(g, M, 128), randn(g, 128, 1, scale=0.1)

        def fn(H, fuse, W1, b1, W2, b2, x3, W3):
            return dcl.ops.linear_group([(H[:, :64], W1, b1, True, fuse[:, :96]), (H[:, 64:], W2, b2, True, None),
                                         (x3, dcl.ops.pad_linear_weight(W3), None, False, None)])
        return dict(fn=fn, inputs=[H, fuse, W1, b1, W2, b2, x3, W3], inplace=(1,))


for _M, _wide in ((1, False), (33, False), (257, True)):
    @case("mlp128_to1/M%d" % _M)
    def _(dcl, M=_M, wide=_wide):
        g = gen("mlp", M)
        x = randn(g, M, 160)[:, 32:] if wide else randn(g, M, 128)
        layers = [randn(g, 128, 128, scale=0.1), randn(g, 128), randn(g, 128, 128, scale=0.1), randn(g, 128), randn(g, 128, 1), randn(g, 1)]
        return dict(fn=lambda x, *l: dcl.ops.mlp128_to1(x, [(l[0], l[1]), (l[2], l[3]), (l[4], l[5])]), inputs=[x] + layers)


# prepared layers switch cores at 192 tiles of 256 x 128 (ops.SPLIT_MIN_TILES): n = 1024 columns are 8 tile columns, so 23 / 24
# row tiles sit on either side
for _M in (23 * 256, 23 * 256 + 1):
    @case("prepared_linear/M%d" % _M)
    def _(dcl, M=_M):
        g = gen("prepared", M)
        x, Wt, bias = randn(g, M, 32), randn(g, 32, 1024, scale=0.05), randn(g, 1024)

        def fn(x, Wt, bias):
            sw = dcl.ops.prepare_linear(Wt)
            assert sw is not None and (dcl.ops.prepared_linear(Wt, x) is not None) == (M > 23 * 256)
            return dcl.ops.linear(x, Wt, bias, True)
        return dict(fn=fn, inputs=[x, Wt, bias])


# ==================================================================================================== attention
ATTN_SHAPES = ((1, 1, 1), (2, 33, 31), (1, 300, 40), (3, 64, 96), (1, 200, 500))
# (hooks of the form; variant 3 = 8 waves, 4 = 4 waves of the LDS-DMA kernel; bf16 1 = the split-bf16 form)
ATTN_FORMS = {"fp32_8w": (3, 0), "fp32_4w": (4, 0), "split": (3, 1)}
ATTN_MAIN = {"fp32_8w": "k_cross_attn_dma<8>", "fp32_4w": "k_cross_attn_dma<4>", "split": "k_cross_attn_split"}


def _attn_inputs(b, nq, nk):
    import test_gpu_attention_grad as TA
    Q, K, V1, V2, dO1, dO2 = TA._inputs(b, nq, nk, 1.0)
    return Q.reshape(-1, 64), K.reshape(-1, 64), V1.reshape(-1, 256), dO1.reshape(-1, 256), dO2.reshape(-1, 64)


for _form, (_variant, _bf16) in ATTN_FORMS.items():
    for _split in (1, 2):
        for _b, _nq, _nk in ATTN_SHAPES:
            @case("cross_attention/%s/split%d/%dx%dx%d" % (_form, _split, _b, _nq, _nk),
                  hooks=[("dcl_debug_attention_variant", _variant, 0), ("dcl_debug_attention_bf16", _bf16, 1),
                         ("dcl_debug_attention_split", _split, 0)])
            def _(dcl, b=_b, nq=_nq, nk=_nk, form=_form, split=_split):
                import split_cases as SC
                Q, K, V1, _, _ = _attn_inputs(b, nq, nk)
                wanted = [ATTN_MAIN[form]]
                if form != "fp32_4w" and SC.effective_split(nk, split, b, nq) > 1:      # the 8-wave forms' rule (csrc/dense.hip: attn_key_split)
                    wanted.append("k_cross_attn_combine")

                def fn(Q, K, V1):                                     # V2 is K itself, as in the network
                    return dcl.ops.cross_attention(b, Q, K, V1, fresh(dcl, b * nq, 256), K, fresh(dcl, b * nq, 64))
                return dict(fn=fn, inputs=[Q, K, V1],
                            kernels=(wanted, "k_cross_attn", ("k_cross_attn_combine",) if form == "fp32_4w" else ()))


for _b, _nq, _nk in ((2, 33, 31), (1, 200, 500)):
    for _with in (True, False):
        @case("cross_attention_backward/%dx%dx%d/dO2_%d" % (_b, _nq, _nk, _with))
        def _(dcl, b=_b, nq=_nq, nk=_nk, with_dO2=_with):
            Q, K, V1, dO1, dO2 = _attn_inputs(b, nq, nk)

            def fn(Q, K, V1, dO1, dO2):
                O1, O2 = dcl.ops.cross_attention(b, Q, K, V1, fresh(dcl, b * nq, 256), K, fresh(dcl, b * nq, 64))
                return dcl.ops.cross_attention_backward(b, Q, K, V1, K, O1, O2, dO1, dO2 if with_dO2 else None)
            return dict(fn=fn, inputs=[Q, K, V1, dO1, dO2])


# ==================================================================================================== sparse front
def _voxels(b, S, per, seed):
    import test_gpu_ops as TG
    return cuda(TG.rand_voxels(np.random.default_rng(seed), b, S, per))


def _pair_sets(pairs):
    """(kvol, 2, n) pairs as one sorted key per pair and offset: the set of an offset's pairs without their order"""
    return (pairs[:, 0].long() * (1 << 31) + pairs[:, 1].long()).sort(dim=1).values


for _S, _st, _subm in ((16, 1, False), (16, 2, False), (8, 1, True)):
    @case("rulebook/S%d_s%d_subm%d" % (_S, _st, _subm))
    def _(dcl, S=_S, st=_st, subm=_subm):
        idx = _voxels(3, S, 129, S + st)

        def fn(idx):
            aset = dcl.ops.grid_from_indices(idx, 3, S)
            out, nbr = dcl.spconv.ops.build_rulebook(aset, 3, st, 1, subm)
            n_out = idx.shape[0] if subm else out.n
            pairs, num = dcl.ops.rulebook_to_pairs(nbr, n_out, idx.shape[0])
            order = dcl.ops.order_rows(out, aset.mask, subm) if st == 1 else ()
            return [aset.mask, aset.wprefix, aset.perm, out.indices, nbr, pairs, num] + list(order)
        # include/dclnet_hip.h at dcl_rulebook_to_pairs: "Pair order inside an offset is unspecified, as in the reference."
        return dict(fn=fn, inputs=[idx], valid=lambda outs: outs[:5] + [_pair_sets(outs[5])] + outs[6:])


def _conv_operands(dcl, cin, cout, subm, rows, seed):
    """feat, nbr (27, rows), W of a k3 / s1 / p1 layer with exactly `rows` output rows: the rulebook of a random scene, cut to size"""
    b, S = 2, 16
    idx = _voxels(b, S, max(rows // 2 + 1, 200), seed)
    aset = dcl.ops.grid_from_indices(idx, b, S)
    out, nbr = dcl.spconv.ops.build_rulebook(aset, 3, 1, 1, subm)
    n_all = idx.shape[0] if subm else out.n
    assert n_all >= rows, (n_all, rows)
    g = gen("conv", cin, cout, subm, rows)
    feat, W = randn(g, idx.shape[0], cin), randn(g, 27, cin, cout, scale=1.0 / (3.0 * cin ** 0.5))
    scale, shift = (torch.rand(cout, generator=g) + 0.5).cuda(), randn(g, cout)
    return feat, nbr[:, :rows].contiguous(), W, scale, shift


NOT_FEW = ("dcl_debug_conv_few_hint", 0, 24576)           # no launch counts as a few-row one: the many-row decompositions at small sizes
CONV_FORMS = {
    "few_rows": (),
    "split_k2": (NOT_FEW, ("dcl_debug_conv_split", 2, 0)),
    "split_k5": (NOT_FEW, ("dcl_debug_conv_split", 5, 0)),
    "stream_k": (NOT_FEW,),
    "whole_tiles": (NOT_FEW, ("dcl_debug_conv_split", -2, 0)),
}

for _formname, _hooks in CONV_FORMS.items():
    for _cin, _cout, _subm, _rows in ((32, 64, True, 385), (64, 128, False, 383), (128, 128, True, 257)):
        @case("sparse_conv/%s/%d_%d_subm%d_rows%d" % (_formname, _cin, _cout, _subm, _rows), hooks=_hooks)
        def _(dcl, cin=_cin, cout=_cout, subm=_subm, rows=_rows):
            feat, nbr, W, scale, shift = _conv_operands(dcl, cin, cout, subm, rows, cin + rows)
            return dict(fn=lambda feat, nbr, W, scale, shift: (dcl.ops.sparse_conv(feat, nbr, rows, W, subm),
                                                               dcl.ops.sparse_conv(feat, nbr, rows, W, subm, scale, shift, True)),
                        inputs=[feat, nbr, W, scale, shift])


for _cin, _rows in ((16, 385), (32, 383)):
    @case("sparse_conv/filter_resident/%d_32_rows%d" % (_cin, _rows), hooks=(NOT_FEW,))
    def _(dcl, cin=_cin, rows=_rows):
        feat, nbr, W, scale, shift = _conv_operands(dcl, cin, 32, True, rows, cin)
        return dict(fn=lambda feat, nbr, W, scale, shift: (dcl.ops.sparse_conv(feat, nbr, rows, W, True),
                                                           dcl.ops.sparse_conv(feat, nbr, rows, W, True, scale, shift, True)),
                    inputs=[feat, nbr, W, scale, shift], kernels=(["k_sparse_conv_wlds"], "k_sparse_conv"))


# the 7 -> 16 stem: four lanes per row up to 49 152 rows, a lane per row above.  The switch is taken BY SIZE here: the launcher
# compares the runner's form_rows, or an op-level call's exact row count, with a constant (csrc/sparse_conv.hip, DCL_CONV_STEM);
# dcl_debug_conv_few_hint does not reach it and ops.sparse_conv has no way to pass form_rows
for _rows in (385, 49153):
    @case("sparse_conv/stem/rows%d" % _rows)
    def _(dcl, rows=_rows):
        b, S = 4, 32
        idx = _voxels(b, S, max(rows // 4 + 1, 200), rows)
        aset = dcl.ops.grid_from_indices(idx, b, S)
        _, nbr = dcl.spconv.ops.build_rulebook(aset, 3, 1, 1, True)
        g = gen("stem", rows)
        feat, W = randn(g, idx.shape[0], 7), randn(g, 27, 7, 16, scale=0.1)
        return dict(fn=lambda feat, nbr, W: dcl.ops.sparse_conv(feat, nbr, rows, W, True), inputs=[feat, nbr[:, :rows].contiguous(), W])


@case("sparse_conv/ordered", hooks=(NOT_FEW,))
def _(dcl):
    b, S, cin, cout = 2, 16, 64, 64
    idx = _voxels(b, S, 321, 77)                                        # 642 rows: 642 % 128 = 2; the order needs the whole set
    g = gen("ordered")
    feat, W = randn(g, idx.shape[0], cin), randn(g, 27, cin, cout, scale=0.05)

    def fn(idx, feat, W):
        aset = dcl.ops.grid_from_indices(idx, b, S)
        _, nbr = dcl.spconv.ops.build_rulebook(aset, 3, 1, 1, True)
        order = dcl.ops.order_rows(aset, aset.mask, True)
        return dcl.ops.sparse_conv(feat, nbr, idx.shape[0], W, True, order=order)
    return dict(fn=fn, inputs=[idx, feat, W])


for _pieces in (False, True):
    @case("sparse_conv_sides/pieces%d" % _pieces)
    def _(dcl, pieces=_pieces):
        fa, na, Wa, sa, ta = _conv_operands(dcl, 64, 128, True, 385, 1)
        fb, nb, Wb, sb, tb = _conv_operands(dcl, 64, 128, True, 255, 2)

        def fn(fa, na, Wa, sa, ta, fb, nb, Wb, sb, tb):
            pcs = [dcl.ops.conv_split_weight(Wa), dcl.ops.conv_split_weight(Wb)] if pieces else None
            return dcl.ops.sparse_conv_sides([fa, fb], [na, nb], [385, 255], [Wa, Wb], True, pcs, [sa, sb], [ta, tb], True)
        return dict(fn=fn, inputs=[fa, na, Wa, sa, ta, fb, nb, Wb, sb, tb])


for _cin, _cout, _subm, _rows in ((32, 32, False, 385), (7, 16, False, 127)):
    @case("sparse_conv/compact/%d_%d_rows%d" % (_cin, _cout, _rows))
    def _(dcl, cin=_cin, cout=_cout, subm=_subm, rows=_rows):
        feat, nbr, W, _, _ = _conv_operands(dcl, cin, cout, subm, rows, 5)
        return dict(fn=lambda feat, nbr, W: dcl.ops.sparse_conv(feat, nbr, rows, W, subm, form="compact"), inputs=[feat, nbr, W])


for _c in (32, 7):
    @case("sparse_avgpool/c%d" % _c)
    def _(dcl, c=_c):
        idx = _voxels(2, 16, 200, c)
        aset = dcl.ops.grid_from_indices(idx, 2, 16)
        out, nbr = dcl.spconv.ops.build_rulebook(aset, 3, 2, 1, False)
        rows = out.n - (out.n - 1) % 128                               # the most rows with rows % 128 == 1
        feat = randn(gen("pool", c), idx.shape[0], c)
        return dict(fn=lambda feat, nbr: (dcl.ops.sparse_avgpool(feat, nbr, rows), dcl.ops.sparse_avgpool(feat, nbr, rows, want_rf=True)),
                    inputs=[feat, nbr[:, :rows].contiguous()])


@case("voxelize")
def _(dcl):
    rng = np.random.default_rng(5)
    b, n = 4, 257
    coords = cuda(np.concatenate([np.repeat(np.arange(b), n)[:, None], rng.integers(0, 16, (b * n, 3))], 1).astype(np.int64))
    feats = randn(gen("voxelize"), b * n, 7)

    def fn(coords, feats):
        oc, im, om = dcl.ops.voxelize_idx_gpu(coords, b, 16, 4)
        return oc, im, om, dcl.ops.voxelize_fp(feats, om, 4), dcl.ops.voxelize_fp(feats, om, 3)
    return dict(fn=fn, inputs=[coords, feats])


def _sp_operands(kind):
    import test_gpu_ops as TG
    rng = np.random.default_rng(4)
    if kind == "edge":                                                  # crop 1 has no voxels, crop 0 only two
        unk, kn = TG._sp_case(rng, 3, 70, 5)
        kn = kn[kn[:, 0] != 1]
        kn = np.concatenate([kn[:2], kn[5:]])
        seg = np.array([0, 2, 2, 7], np.int32)
    else:
        unk, kn = TG._sp_case(rng, 2, 257, 64)
        seg = np.array([0, 64, 128], np.int32)
    return cuda(unk), cuda(kn), cuda(seg)


for _kind in ("edge", "plain"):
    @case("three_nn_sp/%s" % _kind)
    def _(dcl, kind=_kind):
        unk, kn, seg = _sp_operands(kind)
        feats = randn(gen("sp", kind), kn.shape[0], 32)
        big = torch.zeros((unk.shape[0], 96)).cuda()

        def fn(unk, kn, seg, feats, big):
            d2, idx = dcl.ops.three_nn_sp(unk, kn)
            d2s, idxs = dcl.ops.three_nn_sp(unk, kn, seg)
            fused = dcl.ops.three_interpolate_sp(feats, idx, d2, from_dist2=True)
            w = torch.full_like(d2, 1.0 / 3.0)
            dcl.ops.three_interpolate_sp(feats, idx, w, out=big[:, 32:64])
            return d2, idx, d2s, idxs, fused
        return dict(fn=fn, inputs=[unk, kn, seg, feats, big], inplace=(4,))


@case("voxel_centres")
def _(dcl):
    rng = np.random.default_rng(6)
    idx = cuda(np.concatenate([rng.integers(0, 4, (257, 1)), rng.integers(0, 32, (257, 3))], 1).astype(np.int32))
    return dict(fn=lambda idx: dcl.ops.voxel_centres(idx, 0.012, -0.192), inputs=[idx])


def _backbone_net(dcl):
    net = dcl.DCL_Net.Network(dcl.synth.default_cfg(64, 64), mode="test")
    net.load_state_dict(dcl.synth.synth_state_dict(net, 5))
    return net.cuda().eval()


@case("backbone_run/edge_voxels")
def _(dcl):
    import test_gpu_ops as TG
    rng = np.random.default_rng(17)
    occ, b = TG._edge_voxels(rng)
    f = _backbone_net(dcl)._fold()
    vox = cuda(rng.normal(size=(occ.shape[0], 7)).astype(np.float32))
    n_per = 50
    pts = rng.uniform(-0.19, 0.19, (b * n_per, 3)).astype(np.float32)
    pb4 = cuda(np.concatenate([np.repeat(np.arange(b, dtype=np.float32), n_per)[:, None], pts], 1))
    unit = 0.006
    off = float(np.float32(-0.5 * unit * 64))
    extents = [float(np.float32(unit * sc)) for sc in (2, 4, 6, 8)]

    def fn(occ, vox, pb4):
        run = dcl.ops.BackboneRun(occ, b, 64)
        run.set_counts(run.counts_dev.cpu().tolist())
        levels = run.features(vox, *f["backbone_inp_ptrs"])
        d2, idx = run.point_neighbours(pb4, extents, off)
        return ([run.counts_dev] + [run.level_indices(m) for m in range(4)] + list(levels) +
                [d2, idx, run.point_interpolate(d2, idx), run.point_features(pb4, extents, off)])
    return dict(fn=fn, inputs=[cuda(occ), vox, pb4])


# ==================================================================================================== pointnet_lib
def _cloud(b, n, seed):
    import test_gpu_ops as TG
    return cuda(TG._cloud(np.random.default_rng(seed), b, n))


@case("fps/257_to_64")
def _(dcl):
    return dict(fn=lambda xyz: dcl.ops.furthest_point_sampling(xyz, 64), inputs=[_cloud(3, 257, 1)])


@case("ball_query_group_gather")
def _(dcl):
    rng = np.random.default_rng(8)
    xyz = _cloud(3, 333, 2)
    new = xyz[:, :77].contiguous() + 1e-3
    new[:, 0] = 9.0                                                     # a centre with no neighbour at all
    feats = randn(gen("group"), 3, 20, 333)
    gi = cuda(rng.integers(0, 333, (3, 123)).astype(np.int32))
    idx3 = cuda(rng.integers(0, 333, (3, 77, 3)).astype(np.int32))      # nsample no multiple of 4: the scalar kernel
    full = torch.full((3, 27, 77, 16), 7.0).cuda()

    def fn(xyz, new, feats, gi, idx3, full):
        idx = dcl.ops.ball_query(0.2, 16, xyz, new)
        dcl.ops.group_points(feats, idx, out=full[:, 3:23])
        return idx, dcl.ops.group_points(feats, idx), dcl.ops.group_points(feats, idx3), dcl.ops.gather_points(feats, gi)
    return dict(fn=fn, inputs=[xyz, new, feats, gi, idx3, full], inplace=(5,))


# dcl_group_points_into stages whole channel rows in the LDS once npoint * nsample >= 4096 (1 .. 4 rows per workgroup by row
# length; test_group_points_lds_staged_rows_bit_exact); below that every output fetches its own element
for _n, _c, _np, _ns in ((700, 20, 50, 16), (700, 9, 1024, 4), (5000, 7, 64, 64)):
    @case("group_points/n%d_c%d_%dx%d" % (_n, _c, _np, _ns))
    def _(dcl, n=_n, c=_c, npoint=_np, ns=_ns):
        rng = np.random.default_rng(n)
        feats = randn(gen("group", n), 2, c, n)
        idx = rng.integers(0, n, (2, npoint, ns)).astype(np.int32)
        idx[0, 0, :4] = [0, n - 1, 0, n - 1]
        full = torch.full((2, c + 5, npoint, ns), -7.0).cuda()

        def fn(feats, idx, full):
            dcl.ops.group_points(feats, idx, out=full[:, 3:3 + c])
            return dcl.ops.group_points(feats, idx)
        return dict(fn=fn, inputs=[feats, cuda(idx), full], inplace=(2,))


for _k in (1, 3, 5):
    @case("knn/k%d" % _k)
    def _(dcl, k=_k):
        return dict(fn=lambda u, kn: dcl.ops.knn(k, u, kn), inputs=[_cloud(2, 129, 3), _cloud(2, 65, 4)])


@case("three_nn/3x513x64")
def _(dcl):
    feats = randn(gen("interp"), 3, 20, 64)

    def fn(u, kn, feats):
        d2, idx = dcl.ops.three_nn(u, kn)
        w = 1.0 / (d2 + 1e-8)
        w = (w / w.sum(2, keepdim=True)).contiguous()
        return d2, idx, dcl.ops.three_interpolate(feats, idx, w)
    return dict(fn=fn, inputs=[_cloud(3, 513, 5), _cloud(3, 64, 6), feats])


@case("pointnet_grads")
def _(dcl):
    rng = np.random.default_rng(12)
    B, c, n, m, npoint, ns = 2, 20, 129, 65, 33, 5
    g = gen("pn grads")
    idx_g = cuda(rng.integers(0, n, (B, npoint, ns)).astype(np.int32))
    idx_t = cuda(rng.integers(0, n, (B, m)).astype(np.int32))
    idx_3 = cuda(rng.integers(0, m, (B, n, 3)).astype(np.int32))
    w = torch.rand(B, n, 3, generator=g).cuda()
    return dict(fn=lambda gg, gt, gi, idx_g, idx_t, idx_3, w: (dcl.ops.group_points_grad(gg, idx_g, n), dcl.ops.gather_points_grad(gt, idx_t, n),
                                                               dcl.ops.three_interpolate_grad(gi, idx_3, w, m)),
                inputs=[randn(g, B, c, npoint, ns), randn(g, B, c, m), randn(g, B, c, n), idx_g, idx_t, idx_3, w])


# ==================================================================================================== tail, refiner, data
for _b, _n1, _n2 in ((2, 2048, 2048), (2, 2048, 2049), (3, 5, 7)):      # 4096 logits: the last size of the 256-thread form
    @case("conf_softmax/%dx%dx%d" % (_b, _n1, _n2))
    def _(dcl, b=_b, n1=_n1, n2=_n2):
        import tail_cases as TC
        l1, l2 = TC.logits("gauss", b, n1, n2, 1)
        return dict(fn=lambda l1, l2: dcl.ops.conf_softmax(b, l1, l2), inputs=[l1.reshape(-1).cuda(), l2.reshape(-1).cuda()])


for _b, _n1, _n2, _c in ((3, 300, 170, 260), (9, 33, 31, 260), (1, 1, 257, 1024)):
    @case("conf_pool/%dx%dx%dx%d" % (_b, _n1, _n2, _c))
    def _(dcl, b=_b, n1=_n1, n2=_n2, c=_c):
        import tail_cases as TC
        k = TC._pool_operands(b, n1, n2, c, seed=7)
        F1 = torch.zeros(b * n1, c + TC.POOL_PAD)
        F1[:, TC.POOL_OFF:TC.POOL_OFF + c] = k["F1"].reshape(-1, c)
        ins = [k["l1"].reshape(-1).cuda(), k["l2"].reshape(-1).cuda(), F1.cuda()[:, TC.POOL_OFF:TC.POOL_OFF + c],
               k["F2"].reshape(-1, c).cuda()] + [a.cuda() for a in k["affine"]]

        def fn(l1, l2, F1, F2, *affine):
            conf, (ns, p1, p2, ws) = dcl.ops.conf_pool(b, l1, l2, F1, F2, affine, finish=False)
            return dcl.ops.conf_pool(b, l1, l2, F1, F2), dcl.ops.conf_pool(b, l1, l2, F1, F2, affine), conf, p1, p2, ws
        return dict(fn=fn, inputs=ins)


@case("ortho9d_to_matrix")
def _(dcl):
    return dict(fn=lambda o9: dcl.ops.ortho9d_to_matrix(o9), inputs=[randn(gen("o9"), 5, 9)])


@case("affine3_relu")
def _(dcl):
    g = gen("affine3")
    return dict(fn=lambda xyz, W3, term: dcl.ops.affine3_relu(xyz, W3, term), inputs=[randn(g, 257, 3), randn(g, 3, 72), randn(g, 257, 72)])


@case("pad_copy_many")
def _(dcl):
    g = torch.Generator().manual_seed(3)
    feats = torch.randn(300, 7, generator=g).cuda()
    occ = torch.randint(0, 64, (123, 4), generator=g, dtype=torch.int64).cuda()
    v2p = torch.randint(0, 300, (123, 5), generator=g, dtype=torch.int32).cuda()
    wide = torch.randn(40, 512, generator=g).cuda()
    src_r = torch.randn(4, 9, generator=g).cuda()
    dst = [torch.full((300, 7), 9.0).cuda(), torch.full((300, 4), 9, dtype=torch.int32).cuda(), torch.full((300, 33), 9, dtype=torch.int32).cuda(),
           torch.full((1,), 9, dtype=torch.int32).cuda(), torch.full((2, 20, 256), 9.0).cuda(), torch.full((4, 3, 3), 9.0).cuda()]

    def fn(feats, occ, v2p, wide, src_r, d):
        dcl.ops.pad_copy_many([(d[0], feats), (d[1], occ), (d[2], v2p), (d[3], 123), (d[4], wide[:, 256:]), (d[5], src_r)])
        return ()
    return dict(fn=fn, inputs=[feats, occ, v2p, wide, src_r, dst], inplace=(5,))


@case("chamfer/2x33x31")
def _(dcl):
    g = gen("chamfer")
    active = torch.tensor([1, 1], dtype=torch.int32).cuda()

    def fn(pred, target, g_pt, g_tp, active):
        d_pt, i_pt, d_tp, i_tp = dcl.ops.chamfer(pred, target)
        return (d_pt, i_pt, d_tp, i_tp) + tuple(dcl.ops.chamfer_backward(pred, target, i_pt, i_tp, g_pt, g_tp)) + \
            tuple(dcl.ops.chamfer(pred, target, active))
    return dict(fn=fn, inputs=[randn(g, 2, 33, 3), randn(g, 2, 31, 3), randn(g, 2, 33), randn(g, 2, 31), active])


def _bn_shapes():
    import bn_relu_cases as BC
    return ((BC.R + 1, 5), (BC.R + 3, 24))


for _i in (0, 1):
    @case("bn_relu/shape%d" % _i)
    def _(dcl, i=_i):
        rows, c = _bn_shapes()[i]
        g = gen("bn", rows, c)
        x, gamma, beta, grad = randn(g, rows, c), randn(g, c), randn(g, c), randn(g, rows, c)
        rm, rv = randn(g, c), torch.rand(c, generator=g).cuda() + 0.5

        def fn(x, gamma, beta, grad, rm, rv):
            z, mean, invstd = dcl.ops.bn_relu(x, gamma, beta, rm, rv)
            return (z, mean, invstd) + tuple(dcl.ops.bn_relu_backward(x, gamma, beta, mean, invstd, grad))
        return dict(fn=fn, inputs=[x, gamma, beta, grad, rm, rv], inplace=(4, 5))


@case("linear_wgrad_relu_bwd")
def _(dcl):
    g = gen("wgrad")
    a, b, h = randn(g, 257, 48), randn(g, 257, 72), randn(g, 257, 72)
    wide = randn(g, 48, 72 + 5)
    roww, gpool = torch.rand(258, generator=g).cuda(), randn(g, 2, 72)
    hp = randn(g, 258, 72)                                              # two crops of 129 rows: the pooled last layer's form

    def fn(a, b, h, wide, roww, gpool, hp):
        dcl.ops.linear_wgrad(a, b, out=wide[:, 3:75])
        return dcl.ops.linear_wgrad(a, b), dcl.ops.relu_bwd(h, b), dcl.ops.relu_bwd(hp, roww=roww, gpool=gpool, rows_per_crop=129)
    return dict(fn=fn, inputs=[a, b, h, wide, roww, gpool, hp], inplace=(3,))


# ==================================================================================================== heads and the refiner
def _head_layers(g, n_out):
    return [randn(g, 1024, 512, scale=0.03), randn(g, 512), randn(g, 512, 128, scale=0.05), randn(g, 128), randn(g, 128, n_out, scale=0.1),
            randn(g, n_out)]


def _pairs(flat):
    return [(flat[0], flat[1]), (flat[2], flat[3]), (flat[4], flat[5])]


for _b in (1, 3):
    @case("pose_heads/b%d" % _b)
    def _(dcl, b=_b):
        g = gen("heads", b)
        ns = 3
        ins = [randn(g, b, 1024), randn(g, b, ns, 1024), randn(g, b, ns, 1024), torch.rand(b, 2, generator=g).cuda()]
        affine, rot, trans = [randn(g, 1024) for _ in range(4)], _head_layers(g, 9), _head_layers(g, 3)

        def fn(pooled, p1, p2, ws, affine, rot, trans):
            rot, trans = _pairs(rot), _pairs(trans)
            return (dcl.ops.pose_heads(pooled, rot, trans), dcl.ops.pose_heads(pooled, rot, trans, with_rotation=True),
                    dcl.ops.pose_heads_parts((ns, p1, p2, ws), affine, rot, trans, with_rotation=True),
                    dcl.ops.pool_finish2(p1.reshape(b * ns, 1024), p2.reshape(b * ns, 1024), ws, affine))
        return dict(fn=fn, inputs=ins + [affine, rot, trans])


for _b, _T in ((1, 1), (3, 2)):
    @case("refine_heads/b%d_T%d" % (_b, _T))
    def _(dcl, b=_b, T=_T):
        import test_refine_loop_host as RH
        g = gen("refine heads", b, T)
        part, R_in, t_in = randn(g, b * T, 1024), RH.rotations(b, g).cuda(), randn(g, b, 3, scale=0.02)
        rot, trans = _head_layers(g, 9), _head_layers(g, 3)

        def fn(part, R_in, t_in, rot, trans):
            R_out, t_out = fresh(dcl, b, 3, 3), fresh(dcl, b, 3)
            return dcl.ops.refine_heads(part, T, _pairs(rot), _pairs(trans), R_in, t_in, R_out, t_out), R_out, t_out
        return dict(fn=fn, inputs=[part, R_in, t_in, rot, trans])


for _b, _n, _c in ((3, 33, 72), (2, 100, 512), (1, 64, 8)):
    @case("refine_first/%dx%dx%d" % (_b, _n, _c))
    def _(dcl, b=_b, n=_n, c=_c):
        import test_refine_loop_host as RH
        ins = [t.cuda() for t in RH.first_case(b, n, c, seed=5)]
        return dict(fn=lambda pts, R, t, W3, term: dcl.ops.refine_first(pts, R, t, W3, term), inputs=ins)


@case("add_s")
def _(dcl):
    import test_refine_loop_host as RH
    g = gen("add_s")
    b, P = 3, 257
    ins = [randn(g, b, P, 3, scale=0.05), RH.rotations(b, g).cuda(), randn(g, b, 3, scale=0.02), RH.rotations(b, g).cuda(),
           randn(g, b, 3, scale=0.02)]
    return dict(fn=lambda cld, Rp, tp, Rg, tg: (dcl.ops.add_s(cld, Rp, tp, Rg, tg), dcl.ops.add(cld, Rp, tp, Rg, tg)), inputs=ins)


# ==================================================================================================== training kernels
@case("rigid_points/2x33")
def _(dcl):
    import test_refine_loop_host as RH
    g = gen("rigid")
    ins = [randn(g, 2, 33, 3), RH.rotations(2, g).cuda(), randn(g, 2, 3), randn(g, 2, 33, 3)]
    return dict(fn=lambda pts, R, t, go: (dcl.ops.rigid_points(pts, R, t), dcl.ops.rigid_points(pts, R, t, inverse=True),
                                          dcl.ops.rigid_points_backward(pts, R, t, False, go, need_pts=True),
                                          dcl.ops.rigid_points_backward(pts, R, t, True, go)), inputs=ins)


@case("pose_objective/2x33")
def _(dcl):
    g = gen("objective")
    b, n = 2, 33
    clouds = [randn(g, b, n, 3, scale=0.1) for _ in range(6)]           # posed, posed_gt, Yc, cano_pred, cano_gt, Xo
    conf, sym = torch.rand(b, 2 * n, generator=g).cuda(), torch.tensor([0.0, 1.0]).cuda()
    halves = [torch.rand(b, n, generator=g).cuda() for _ in range(6)]
    g_packed = randn(g, 5)

    def fn(clouds, conf, sym, h, g_packed):
        posed, posed_gt, Yc, cano_pred, cano_gt, Xo = clouds
        packed, L = dcl.ops.pose_objective(posed, posed_gt, sym, (h[0], h[1]), Yc, cano_pred, cano_gt, Xo, conf, (h[2], h[3]), (h[4], h[5]))
        only, _ = dcl.ops.pose_objective(posed, posed_gt, sym, (h[0], h[1]))
        return (packed, L, only, dcl.ops.pose_objective_backward(g_packed, posed, posed_gt, sym, Yc, cano_pred, cano_gt, Xo, conf, L),
                dcl.ops.pose_objective_backward(g_packed, posed, posed_gt, sym))
    return dict(fn=fn, inputs=[clouds, conf, sym, halves, g_packed])


for _layout in ("pm", "cm"):
    @case("conf_pool_%s/3x257x130x72" % _layout)
    def _(dcl, layout=_layout):
        g = gen("conf pool", layout)
        b, n1, n2, c = 3, 257, 130, 72
        l1, l2 = randn(g, b * n1), randn(g, b * n2)
        F1, F2 = (randn(g, b * n1, c), randn(g, b * n2, c)) if layout == "pm" else (randn(g, b, c, n1), randn(g, b, c, n2))
        gp, gc = randn(g, b, c), randn(g, b, n1 + n2)
        fwd, bwd = getattr(dcl.ops, "conf_pool_" + layout), getattr(dcl.ops, "conf_pool_%s_backward" % layout)

        def fn(l1, l2, F1, F2, gp, gc):
            conf, w, _ = dcl.ops.conf_softmax(b, l1, l2)
            return fwd(w, F1, F2), bwd(conf, w, F1, F2, gp, gc), bwd(conf, w, F1, F2, gp, None, need_F=False)
        return dict(fn=fn, inputs=[l1, l2, F1, F2, gp, gc])


for _n in (1, 9):
    @case("linear_narrow/N%d" % _n)
    def _(dcl, n=_n):
        g = gen("narrow", n)
        M, K = 257, 48
        x, W, bias, go = randn(g, M, K + 8)[:, 4:4 + K], randn(g, n, K, 1, scale=0.1), randn(g, n), randn(g, M, n)
        return dict(fn=lambda x, W, bias, go: (dcl.ops.linear_narrow(x, W, bias), dcl.ops.linear_narrow_backward(x, W, go)),
                    inputs=[x, W, bias, go])


@case("pose_heads_train/b3")
def _(dcl):
    g = gen("heads train")
    b, d0, d1, d2 = 3, 72, 40, 24
    params = []
    for n_out in (9, 3):
        params += [randn(g, d1, d0, 1, scale=0.1), randn(g, d1), randn(g, d2, d1, 1, scale=0.1), randn(g, d2), randn(g, n_out, d2, 1, scale=0.1),
                   randn(g, n_out)]

    def fn(x, params, g9, g3):
        o9, t3, h1, h2 = dcl.ops.pose_heads_train(x, params)
        return o9, t3, h1, h2, dcl.ops.pose_heads_train_backward(x, params, h1, h2, g9, g3)
    return dict(fn=fn, inputs=[randn(g, b, d0), params, randn(g, b, 9), randn(g, b, 3)])


@case("ortho9d_backward")
def _(dcl):
    g = gen("o9 bwd")
    return dict(fn=lambda o9, gR: dcl.ops.ortho9d_backward(o9, gR), inputs=[randn(g, 5, 9), randn(g, 5, 3, 3)])


for _cin, _cout, _subm, _rows in ((32, 64, True, 385), (64, 64, False, 383), (7, 16, False, 129)):
    @case("sparse_conv_backward/%d_%d_subm%d_rows%d" % (_cin, _cout, _subm, _rows))
    def _(dcl, cin=_cin, cout=_cout, subm=_subm, rows=_rows):
        feat, nbr, W, _, _ = _conv_operands(dcl, cin, cout, subm, rows, 11)
        dout = randn(gen("conv bwd", cin, rows), rows, cout)

        def fn(feat, nbr, W, dout):
            return (dcl.ops.sparse_conv_backward(feat, W, dout, nbr, rows, subm),
                    dcl.ops.sparse_conv_backward(feat, W, dout, nbr, rows, subm, wgrad="pairs", dgrad="direct"))
        return dict(fn=fn, inputs=[feat, nbr, W, dout])


@case("sparse_avgpool_backward")
def _(dcl):
    idx = _voxels(2, 16, 200, 9)
    aset = dcl.ops.grid_from_indices(idx, 2, 16)
    out, nbr = dcl.spconv.ops.build_rulebook(aset, 3, 2, 1, False)
    rows = out.n - (out.n - 1) % 128
    g = gen("pool bwd")
    feat, dout = randn(g, idx.shape[0], 32), randn(g, rows, 32)

    def fn(feat, nbr, dout):
        _, rf = dcl.ops.sparse_avgpool(feat, nbr, rows, want_rf=True)
        return dcl.ops.sparse_avgpool_backward(dout, nbr, rows, feat.shape[0], rf)
    return dict(fn=fn, inputs=[feat, nbr[:, :rows].contiguous(), dout])


@case("readout_grad")
def _(dcl):
    rng = np.random.default_rng(21)
    g = gen("readout")
    n, m, c = 257, 65, 24
    wide = randn(g, n, 3 * c)
    idx = cuda(rng.integers(0, m, (n, 3)).astype(np.int32))
    w = torch.rand(n, 3, generator=g).cuda()
    # (a point belongs to one voxel: the rule's point lists are disjoint)
    rule = cuda(np.concatenate([np.full((m, 1), 2), rng.permutation(n)[:2 * m].reshape(m, 2)], 1).astype(np.int32))
    return dict(fn=lambda wide, idx, w, dv, rule: (dcl.ops.three_interpolate_grad_sp(wide[:, c:2 * c], idx, w, m), dcl.ops.voxelize_bp(dv, rule, n)),
                inputs=[wide, idx, w, randn(g, m, 7), rule])


@case("adam_autoclip_device")
def _(dcl):
    sizes = (1, dcl.optim.CHUNK - 1, dcl.optim.CHUNK + 1, 15)
    g = gen("adam")
    params = [randn(g, n) for n in sizes]
    grads = [[randn(g, n, scale=10.0 ** (-s % 3 - 2)) for n in sizes] for s in range(5)]

    def fn(params, grads):
        ps = [torch.nn.Parameter(p) for p in params]
        opt = dcl.optim.Adam(ps, lr=1e-3, betas=(0.5, 0.999), eps=1e-6)
        clip = dcl.optim.DeviceAutoClip(50, optimizer=opt, capacity=4)          # grows at the fifth step
        for step in grads:
            for p, gr in zip(ps, step):
                p.grad = gr
            clip(None)
            opt.step()
        return [opt.state[p][k] for p in ps for k in ("exp_avg", "exp_avg_sq")], clip._sorted[0][:5], clip._out
    return dict(fn=fn, inputs=[params, grads], inplace=(0,))


# ==================================================================================================== the crop builders' kernels
@case("voxelize_idx_crops")
def _(dcl):
    rng = np.random.default_rng(3)
    b, n_per = 3, 257
    coords = cuda(np.concatenate([np.repeat(np.arange(b), n_per)[:, None], rng.integers(20, 40, (b * n_per, 3))], 1).astype(np.int64))

    # include/dclnet_hip.h at dcl_voxelize_idx_crops: the rows behind the V live ones are zeroed -- whole buffers are compared
    return dict(fn=lambda coords: dcl.ops.voxelize_idx_crops(coords, b, n_per), inputs=[coords])


H_, W_ = 37, 70                          # no multiple of 32 and narrower than three words (tests/mask_cases.py)
CAM = (35.0, 18.0, 500.0, 500.0, 1000.0)
RGB_MEAN = (0.485, 0.456, 0.406)
HALF = [0.006 * 64 * 0.5] * 3
# rows [rmin, rmax, cmin, cmax, class, frame]: the whole frame, a box inside it, one pixel, a class no pixel has (an empty mask)
CROP_SRC = np.array([[0, H_, 0, W_, 1, 0], [5, 20, 10, 31, 2, 1], [7, 8, 9, 10, 3, 1], [0, H_, 0, W_, 9, 0], [3, 30, 2, 69, 3, 0]], np.int32)


def _crop_frames():
    """two frames of scattered labels 0..3 at about a metre, a tenth of the depths missing: the whole-frame crop spreads past
    the grid in z, so the filter drops points"""
    rng = np.random.default_rng(31)
    depth = rng.integers(700, 1100, (2, H_, W_)).astype(np.int16)
    depth[rng.random((2, H_, W_)) < 0.1] = 0
    label = rng.integers(0, 4, (2, H_, W_)).astype(np.int32)
    rgb = rng.integers(0, 256, (2, H_, W_, 3), dtype=np.uint8)
    return cuda(depth), cuda(label), cuda(rgb)


def _live(xyz, col, counts):
    """include/dclnet_hip.h at dcl_crop_points: counts = {masked pixels, points inside the grid, rows written} -- the rows
    of out_xyz / out_rgb behind the rows written are not specified"""
    keep = (torch.arange(xyz.shape[1], device=xyz.device)[None, :] < counts[:, 2:3])[:, :, None]
    zero = torch.zeros((), device=xyz.device)
    return [torch.where(keep, xyz, zero), torch.where(keep, col, zero)]


for _always in (False, True):
    @case("crop_points/always_filter%d" % _always)
    def _(dcl, always=_always):
        depth, label, rgb = _crop_frames()
        mine = CROP_SRC[CROP_SRC[:, 5] == 0]
        boxes, ids = cuda(mine[:, :4]), cuda(mine[:, 4])
        return dict(fn=lambda d, l, c, boxes, ids: dcl.ops.crop_points(d, l, c, boxes, ids, CAM, RGB_MEAN, HALF, 32, always, cap=H_ * W_),
                    inputs=[depth[0].contiguous(), label[0].contiguous(), rgb[0].contiguous(), boxes, ids],
                    valid=lambda o: _live(o[0], o[1], o[3]) + o[2:])


@case("crop_points_frames/rows_padded")
def _(dcl):
    depth, label, rgb = _crop_frames()
    n = len(CROP_SRC)

    def fn(d, l, c, src):
        return (dcl.ops.crop_points_frames(d, l, c, CROP_SRC[:, 5], src, CAM, RGB_MEAN, HALF, 32, cap=H_ * W_, rows=n + 2),
                dcl.ops.crop_points_frames(d, l, c, CROP_SRC[:, 5], src, CAM, RGB_MEAN, HALF, 32, cap=H_ * W_))
    return dict(fn=fn, inputs=[depth, label, rgb, cuda(CROP_SRC)],
                valid=lambda o: _live(o[0], o[1], o[3][:n]) + o[2:4] + _live(o[4], o[5], o[7]) + o[6:8])


def _pose_operands(dcl, wide):
    import test_refine_loop_host as RH
    g = gen("crop pose", wide)
    n = len(CROP_SRC)
    R0, A = RH.rotations(n, g).double().numpy(), RH.rotations(n, g).double().numpy()
    t_gt = np.tile(np.array([0.0, 0.0, 0.9]), (n, 1)) + torch.randn(n, 3, generator=g).double().numpy() * 0.01
    jitter = torch.randn(n, 3, generator=g).double().numpy() * 0.01
    rows = (dcl.ops.pose_rows64 if wide else dcl.ops.pose_rows)(list(R0), list(t_gt), list(jitter), list(A))
    cam = (CAM[:4] + (1.0, 1000.0)) if wide else CAM
    cams = torch.tensor([cam] * n, dtype=torch.float32).cuda()
    return cams, cuda(np.ascontiguousarray(rows))


for _wide in (False, True):
    @case("crop_points_posed%s" % ("64" if _wide else ""))
    def _(dcl, wide=_wide):
        depth, label, rgb = _crop_frames()
        cams, pose = _pose_operands(dcl, wide)
        op = dcl.ops.crop_points_posed64 if wide else dcl.ops.crop_points_posed
        return dict(fn=lambda d, l, c, src, cams, pose: op(d, l, c, CROP_SRC[:, 5], src, cams, pose, RGB_MEAN, HALF, 50, cap=H_ * W_),
                    inputs=[depth, label, rgb, cuda(CROP_SRC), cams, pose],
                    valid=lambda o: _live(o[0], o[1], o[3]) + o[2:])


# counts rows [masked, inside the grid, rows]: an empty mask, fewer points than min_valid, fewer than npoint, more than npoint
DRAW_COUNTS = np.array([[0, 0, 0], [10, 10, 10], [300, 200, 300], [40, 20, 40], [257, 257, 257], [5000, 4000, 4000]], np.int32)


@case("crop_draw")
def _(dcl):
    return dict(fn=lambda cnt: (dcl.ops.crop_draw(cnt, 257, 9, 3), dcl.ops.crop_draw(cnt, 257, 9, 3, keep_sparse=False),
                                dcl.ops.crop_draw(cnt, 1, 9, 0)), inputs=[cuda(DRAW_COUNTS)])


@case("crop_draw_keyed/rows_padded")
def _(dcl):
    n = len(DRAW_COUNTS)
    keys = cuda(np.stack([np.array([3, 3, 4, 4, 5, 2 ** 40], np.int64), np.array([0, 1, 0, 1, 0, 7], np.int64)], 1))
    counts = cuda(np.concatenate([DRAW_COUNTS, np.zeros((2, 3), np.int32)]))                # the zero rows of a padded batch
    return dict(fn=lambda cnt, keys: (dcl.ops.crop_draw_keyed(cnt, 257, 9, keys, rows=n + 2), dcl.ops.crop_draw_keyed(cnt, 257, 9, keys),
                                      dcl.ops.crop_draw_keyed(cnt, 257, 9, keys, keep_sparse=False)), inputs=[counts, keys])


@case("crop_sample")
def _(dcl):
    g = gen("crop sample")
    n, cap, npoint = 3, 257, 129
    xyz, col = randn(g, n, cap, 3, scale=0.1), torch.rand(n, cap, 3, generator=g).cuda()
    counts = cuda(np.array([[cap, cap, cap], [200, 20, 200], [cap, 100, cap]], np.int32))
    idx = torch.stack([torch.randint(0, m, (npoint,), generator=g) for m in (cap, 200, cap)]).cuda()
    return dict(fn=lambda xyz, col, idx, cnt: (dcl.ops.crop_sample(xyz, col, idx, cnt, HALF[0], [0.006] * 3, 64),
                                               dcl.ops.crop_sample(xyz, col, idx, None, HALF[0], [0.006] * 3, 64),
                                               dcl.ops.crop_sample(xyz, col, None, None, HALF[0], [0.006] * 3, 64)),
                inputs=[xyz, col, idx, counts])


@case("crop_sample_valid/rows_padded")
def _(dcl):
    g = gen("crop sample valid")
    cap, npoint = 300, 257
    counts = DRAW_COUNTS[:5]                                            # every row count within cap
    n = len(counts)
    xyz, col = randn(g, n, cap, 3, scale=0.1), torch.rand(n, cap, 3, generator=g).cuda()
    keys = cuda(np.stack([np.arange(n, dtype=np.int64) + 3, np.zeros(n, np.int64)], 1))

    def fn(xyz, col, cnt, keys):
        idx, valid = dcl.ops.crop_draw(cnt, npoint, 9, 3)
        idx_p, valid_p = dcl.ops.crop_draw_keyed(cnt, npoint, 9, keys, rows=n + 2)
        return (dcl.ops.crop_sample_valid(xyz, col, idx, cnt, valid, HALF[0], [0.006] * 3, 64),
                dcl.ops.crop_sample_valid(xyz, col, idx_p, None, valid_p, HALF[0], [0.006] * 3, 64))
    return dict(fn=fn, inputs=[xyz, col, cuda(counts), keys])


@case("mask_extent_occlude_paste/23x37")
def _(dcl):
    import test_train_lm_crops_abi as A
    import test_gpu_train_lm_crops as TL
    Hh, Ww, _, seed = A.PASTE_SIZES[0]
    n = 9
    rgb, depth, mask, o_rgb, o_depth, o_mask, starts, boxes = A.paste_cases(Hh, Ww, n, seed)
    plans = A.plans_of(dcl, Hh, Ww, mask, o_mask, starts, boxes)

    def fn(rgb, depth, mask, o_rgb, o_depth, o_mask, plan):
        extent = dcl.ops.mask_extent(mask)
        return extent, dcl.ops.mask_extent(mask[:1]), dcl.ops.occlude_paste(rgb, depth, mask, o_rgb, o_depth, o_mask, plans, plan, extent)
    return dict(fn=fn, inputs=[TL.dev(a) for a in (rgb, depth, mask, o_rgb, o_depth, o_mask, plans)])



# ==================================================================================================== data and evaluation kernels
@case("mask_box/37x70")
def _(dcl):
    import mask_cases as MC
    masks = np.stack([m for _, m in MC.mask_cases(37, 70)]).astype(np.int32)
    return dict(fn=lambda lab: (dcl.ops.mask_box(lab), dcl.ops.mask_box(lab[3], 1, 2)), inputs=[cuda(masks)])


@case("label_table/3x37x70")
def _(dcl):
    rng = np.random.default_rng(2)
    lab = cuda(rng.integers(0, 22, (3, 37, 70)).astype(np.int32))
    dep = cuda((rng.integers(0, 3, (3, 37, 70)) * 500).astype(np.int16))
    return dict(fn=lambda lab, dep: dcl.ops.label_table(lab, dep, 22), inputs=[lab, dep])


# "network": the forward's five blocks on 16-byte aligned rows; "base_off": destinations one float off (the float-by-float path)
for _n_tmp, _pitch, _name in ((5, 644, "network"), (517, 643, "base_off")):
    @case("template_rows/%s_n%d_pitch%d" % (_name, _n_tmp, _pitch))
    def _(dcl, n_tmp=_n_tmp, pitch=_pitch, name=_name):
        import template_cases as TC
        ids = TC.BATCHES[3]
        blocks, bufs = TC.BLOCK_SETS[name]
        flat = {k: torch.full((base + len(ids) * n_tmp * pt,), TC.SENTINEL).cuda() for k, (pt, base) in bufs.items()}
        keys = sorted(flat)
        store = torch.full((len(TC.CLASS_IDS), n_tmp, pitch), float("nan"))
        store[:, :, :TC.COLS] = torch.from_numpy(TC.cache_rows(n_tmp).copy())

        def fn(store, lut, cls, *dst):
            views = {k: d[bufs[k][1]:].view(len(ids) * n_tmp, bufs[k][0]) for k, d in zip(keys, dst)}
            return dcl.ops.template_rows(store[:, :, :TC.COLS], lut, cls, [(src_col, views[buf][:, dst_col:dst_col + width])
                                                                           for src_col, width, buf, dst_col in blocks])
        return dict(fn=fn, inputs=[store.cuda(), torch.from_numpy(TC.lut()).cuda(), torch.tensor(ids, dtype=torch.int32).cuda()] +
                    [flat[k] for k in keys], inplace=tuple(range(3, 3 + len(keys))))


for _mode in ("adds", "lm"):
    @case("metric_table/%s" % _mode)
    def _(dcl, mode=_mode):
        import metric_table_cases as MT
        T, b, P, C = 3, 5, 257, 21
        k = {n: v.cuda() for n, v in MT.pose_case(4, T, b, P, C).items()}
        diameter = torch.from_numpy(np.asarray(MT.diameters(C), np.float64)).cuda() if mode != "adds" else None

        def fn(cld, cls, Rp, tp, Rg, tg, sym):
            ta, tb = (dcl.ops.metric_table_arrays(mode, T, C, device="cuda") for _ in range(2))
            dis = dcl.ops.add_traj(cld, Rp, tp, Rg, tg, cls, sym if mode != "adds" else None)
            dcl.ops.metric_tabulate(ta, dis, cls, None, mode, diameter)
            dcl.ops.add_tabulate(tb, cld, cls, Rp, tp, Rg, tg, None, cls, sym if mode != "adds" else None, "adds", mode, diameter)
            return dis, [v for t in (ta, tb) for v in t.values() if v is not None]
        return dict(fn=fn, inputs=[k["cld"], k["cls"], k["Rp"], k["tp"], k["Rg"], k["tg"], k["sym"]])


# ==================================================================================================== the test
_FAULT = []           # the first case that ended in something other than a failed check: nothing runs on the GPU after it


@pytest.mark.parametrize("name", list(CASES))
def test_guarded(request, dcl, name):
    if _FAULT:
        pytest.fail("not run: case %s ended in an error of the runtime" % _FAULT[0])
    try:
        run_case(dcl, request, name)
    except AssertionError:
        raise
    except BaseException:
        _FAULT.append(name)
        raise
