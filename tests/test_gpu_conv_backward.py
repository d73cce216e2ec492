"""The sparse-conv and pool gradients (csrc/backward.hip; dX through csrc/sparse_conv.hip with the transposed rulebook) beyond
few-row launches, against the float64 / exact-integer references of tests/conv_grad_cases.py.

The shapes are the smallest that cross each switch of the launchers: 26000 rows (> kConvFewRowsHint = 24576: the dX route leaves
the few-row form -- 128x32 / 128x64 / 128x128 LDS-DMA tiles with aligned split-K, stream-K or whole tiles, the filter-resident
kernel for 32 -> 32, the general MFMA kernel for 256 -> 128, the VALU kernel for Cout' of 16 and 7), 5000 rows (few-row form above
kConvFewRows = 4096), 2049 / 2055 output rows (two wgrad splits, ragged tail), 65531 (32 splits, not a multiple of 8) and
163673 (the 64-split cap, rows_per_split 2560), and a stride-2 layer whose transposed rulebook has cap_in != cap_out.

Detection rests on exactly representable operands: with X, W, G from {-2, -1, 1, 2} every fp32 partial sum is an integer below
2^24, so the kernels must equal the integer gradient bit for bit whatever their order of summation.  The rounding behaviour is
bounded separately, on gaussian operands, by a multiple of the fp32 numpy oracle's own error against float64.

The first half of the file runs on the CPU (the references themselves); the second half needs the GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import conv_grad_cases as cg
from test_gpu_ops import cuda, enter_diag, rand_voxels

U = 2.0 ** -24


# ------------------------------------------------------------------------------------------- CPU: the references
def _small(oracle, subm, seed=0):
    rng = np.random.default_rng(seed)
    b, S = 2, 8
    idx = rand_voxels(rng, b, S, 150)
    out_idx, pairs, num, _ = oracle.get_indice_pairs(idx, b, [S] * 3, 3, 1, 1, 1, subm=subm)
    return rng, idx, pairs, num, (idx.shape[0] if subm else out_idx.shape[0])


@pytest.mark.parametrize("subm", [False, True])
def test_float64_reference_agrees_with_the_fp32_oracle(oracle, subm):
    """conv_backward_ref (no subm shortcut, float64) against oracle/backward.py (fp32, centre shortcut for subm): within the
    a-priori bound of an fp32 sum of n terms, (n + 1) 2^-24 sum |terms|, element by element; on exact operands bit for bit, and
    equal to an int64 scatter"""
    from oracle import backward as ob
    rng, idx, pairs, num, n_out = _small(oracle, subm)
    cin, cout = 5, 4
    if subm:
        assert int(np.argmax(num)) == 13 and int(num[13]) == idx.shape[0]      # the oracle's shortcut offset is the centre
    for k in range(27):                                                        # an input row appears once per offset at most
        assert np.unique(pairs[k, 0, :num[k]]).size == num[k]
    X, W, G = cg.gaussian_operands(("small", subm), idx.shape[0], n_out, cin, cout)
    dX, dW = cg.conv_backward_ref(X, W, G, pairs, num)
    magX, magW = cg.conv_backward_ref(np.abs(X), np.abs(W), np.abs(G), pairs, num)
    dx32, dw32 = ob.indice_conv_backward(X, W.reshape(3, 3, 3, cin, cout), G, pairs, num, subm)
    assert np.all(np.abs(dx32 - dX) <= (27 * cout + 1) * U * magX)
    assert np.all(np.abs(dw32.reshape(27, cin, cout) - dW) <= (int(num.max()) + 1) * U * magW)
    assert np.abs(dW).max() > 1.0 and np.abs(dX).max() > 0.1
    # exact operands: the fp32 oracle, the float64 reference and an int64 scatter give the same integers
    X, W, G = cg.exact_operands(("small", subm), idx.shape[0], n_out, cin, cout)
    dX, dW = cg.conv_backward_ref(X, W, G, pairs, num)
    Xi, Wi, Gi = X.astype(np.int64), W.astype(np.int64), G.astype(np.int64)
    iX, iW = np.zeros(X.shape, np.int64), np.zeros(W.shape, np.int64)
    for k in range(27):
        for j in range(int(num[k])):
            i, o = int(pairs[k, 0, j]), int(pairs[k, 1, j])
            iW[k] += np.outer(Xi[i], Gi[o])
            iX[i] += Wi[k] @ Gi[o]
    assert np.array_equal(dX, iX) and np.array_equal(dW, iW)
    dx32, dw32 = ob.indice_conv_backward(X, W.reshape(3, 3, 3, cin, cout), G, pairs, num, subm)
    assert np.array_equal(dx32, dX.astype(np.float32)) and np.array_equal(dw32.reshape(27, cin, cout), dW.astype(np.float32))


def test_float64_pool_reference_agrees_with_the_fp32_oracle(oracle):
    from oracle import backward as ob
    rng = np.random.default_rng(1)
    b, S, c = 2, 8, 12
    idx = rand_voxels(rng, b, S, 150)
    for padding in (1, 0):
        o_idx, pairs, num, _ = oracle.get_indice_pairs(idx, b, [S] * 3, 3, 2, padding, 1, subm=False)
        _, rf = oracle.indice_avgpool(np.zeros((idx.shape[0], 4), np.float32), pairs, num, o_idx.shape[0])
        G = rng.normal(size=(o_idx.shape[0], c)).astype(np.float32)
        want = ob.indice_avgpool_backward(idx.shape[0], G, pairs, num, rf)
        ref, mag = cg.avgpool_backward_ref(idx.shape[0], G, pairs, num, rf)
        assert np.all(np.abs(want - ref) <= 28 * U * mag)                     # <= 27 divisions and 26 additions per element
        assert np.abs(ref).max() > 0.1


def test_shapes_cross_the_switches_they_are_named_for(oracle):
    """the row counts the shape table promises, from the oracle's rulebooks (a changed seed or builder must not move a case to
    the other side of its switch unnoticed)"""
    g = cg.geometry(oracle, "mid", True)
    assert g["n_in"] == g["n_out"] == 26000 > 24576 and cg.wgrad_splits(26000) == (13, 2000)
    g = cg.geometry(oracle, "mid", False)
    assert g["n_in"] == 26000 and 63488 < g["n_out"] <= 65536 and g["n_out"] % 8 != 0
    assert cg.wgrad_splits(g["n_out"]) == (32, 2048)
    g = cg.geometry(oracle, "cap", False)
    assert g["n_in"] == 45000 and 131072 < g["n_out"] <= 163840 and cg.wgrad_splits(g["n_out"]) == (64, 2560)
    assert g["n_out"] % 2560 % 8 != 0                                          # the last split ends inside a step of 8 rows
    for shape, rows, tail in (("edge2049", 2049, 1017), ("edge2055", 2055, 1023)):
        g = cg.geometry(oracle, shape, True)
        assert g["n_out"] == rows and cg.wgrad_splits(rows) == (2, 1032) and rows - 1032 == tail
    g = cg.geometry(oracle, "few5000", True)
    assert 4096 < g["n_out"] == 5000 <= 24576 and cg.wgrad_splits(5000) == (3, 1672)
    g = cg.geometry(oracle, "stride2", False)
    assert g["n_in"] == 26000 and 6144 < g["n_out"] <= 8192 and cg.wgrad_splits(g["n_out"]) == (4, 2048)   # 2 x 16^3 cells
    # the pool case with orphans: kernel 3, stride 2, padding 0 -- inputs on the last plane of an axis reach no output
    g = cg.geometry(oracle, cg.POOL_SHAPE, False, padding=0)
    reached = np.zeros(g["n_in"], bool)
    for k in range(27):
        reached[g["pairs"][k, 0, :g["num"][k]]] = True
    assert 100 < int((~reached).sum()) < g["n_in"] // 4


@pytest.mark.parametrize("case", cg.CASES, ids=cg.case_id)
def test_exact_operands_stay_below_2_24(oracle, case):
    """every partial sum of the exact operands is an integer below 2^24 in any order: a priori (|x|, |w|, |g| <= 2: dW <= 4 pairs
    of one offset, dX <= 4 cout offsets of one row) and for the reference's own maxima"""
    c = cg.conv_case(oracle, case, "exact")
    for a in (c["X"], c["W"], c["G"]):
        assert a.dtype == np.float32 and np.isin(a, (-2.0, -1.0, 1.0, 2.0)).all()
    assert 4 * int(c["geo"]["num"].max()) < cg.EXACT_LIMIT and 4 * 27 * case[2] < cg.EXACT_LIMIT
    max_dw, max_dx = float(np.abs(c["dW"]).max()), float(np.abs(c["dX"]).max())
    print("%s: max|dW| %d  max|dX| %d" % (cg.case_id(case), max_dw, max_dx))
    assert 0 < max_dw < cg.EXACT_LIMIT and 0 < max_dx < cg.EXACT_LIMIT
    assert np.array_equal(c["dW"], np.rint(c["dW"])) and np.array_equal(c["dX"], np.rint(c["dX"]))
    assert np.array_equal(c["dW"].astype(np.float32).astype(np.float64), c["dW"])


def test_one_removed_pair_shows_in_the_reference(oracle):
    """the exact operands cannot hide a dropped row: without one pair of offset k, dW[k] differs in EVERY element (an outer product
    of non-zero integers) and nowhere else, and dX differs in that input row and in no other"""
    case = ("edge2055", 16, 32, True)
    c = cg.conv_case(oracle, case, "exact")
    geo = c["geo"]
    for k, j in ((5, 100), (13, 2054), (26, 0)):
        pairs, num, row_in, row_out = cg.without_pair(geo["pairs"], geo["num"], k, j)
        dX, dW = cg.conv_backward_ref(c["X"], c["W"], c["G"], pairs, num)
        assert np.all(dW[k] != c["dW"][k])
        assert np.array_equal(np.delete(dW, k, 0), np.delete(c["dW"], k, 0))
        assert np.array_equal(c["dW"][k] - dW[k], np.outer(c["X"][row_in], c["G"][row_out]))
        assert np.any(dX[row_in] != c["dX"][row_in])
        assert np.array_equal(np.delete(dX, row_in, 0), np.delete(c["dX"], row_in, 0))


def _splits(lib, n_out):
    s = C.c_int32(-1)
    assert lib.dcl_sparse_conv_wgrad_splits(int(n_out), C.byref(s)) == 0
    return s.value


def test_wgrad_split_counts(dcl):
    """ceil(n_out / 2048), capped at 64, at least 1 -- in both libraries, and as conv_grad_cases.wgrad_splits restates it"""
    for lib in (dcl._native.lib(), C.CDLL(dcl._native.DIAG_SO_PATH)):
        assert [_splits(lib, n) for n in (0, 2048, 2049, 131072, 131073)] == [1, 1, 2, 64, 64]
        for n in (1, 2055, 5000, 8192, 26000, 65535, 163716, 10 ** 6):
            assert _splits(lib, n) == cg.wgrad_splits(n)[0]
        assert lib.dcl_sparse_conv_wgrad_splits(-1, C.byref(C.c_int32(0))) != 0
        assert lib.dcl_sparse_conv_wgrad_splits(5, None) != 0


# ------------------------------------------------------------------------------------------- GPU: the kernels
_RULEBOOKS = {}


def _rulebook(dcl, geo, subm):
    """the device rulebook of a geometry (built once per process) -> (nbr, n_out)"""
    key = id(geo)
    if key not in _RULEBOOKS:
        aset = dcl.ops.grid_from_indices(cuda(geo["idx"]), geo["b"], geo["S"])
        out, nbr = dcl.spconv.ops.build_rulebook(aset, 3, geo["stride"], geo["padding"], subm)
        n_out = geo["n_in"] if subm else out.n
        assert n_out == geo["n_out"]
        _RULEBOOKS[key] = (nbr, n_out, geo)
    return _RULEBOOKS[key][:2]


def _where(got, want, names):
    """'' if equal, else where an array leaves its reference: how many elements, which leading indices"""
    bad = np.argwhere(got != want)
    if bad.size == 0:
        return ""
    lead = np.unique(bad[:, 0])
    return "%d of %d elements differ; %s %s%s (first: index %s got %r want %r)" % (
        bad.shape[0], got.size, names, lead[:12].tolist(), " ..." if lead.size > 12 else "", bad[0].tolist(),
        float(got[tuple(bad[0])]), float(want[tuple(bad[0])]))


def _device_case(dcl, oracle, case, operands):
    c = cg.conv_case(oracle, case, operands)
    nbr, n_out = _rulebook(dcl, c["geo"], case[3])
    return c, nbr, n_out, cuda(c["X"]), cuda(c["W"]), cuda(c["G"])


@pytest.mark.gpu
@pytest.mark.parametrize("case", cg.CASES, ids=cg.case_id)
def test_exact_operands_give_the_integer_gradient(dcl, oracle, case):
    """dx and dw equal the integer reference bit for bit; a second call, need_dx=False and the autograd route give the same bits"""
    c, nbr, n_out, f, W, g = _device_case(dcl, oracle, case, "exact")
    subm = case[3]
    want_dx, want_dw = c["dX"].astype(np.float32), c["dW"].astype(np.float32)
    dx, dw = dcl.ops.sparse_conv_backward(f, W, g, nbr, n_out, subm)
    splits, per = cg.wgrad_splits(n_out)
    assert _where(dw.cpu().numpy(), want_dw, "offsets k (%d splits of %d rows)" % (splits, per)) == ""
    assert _where(dx.cpu().numpy(), want_dx, "input rows") == ""
    dx2, dw2 = dcl.ops.sparse_conv_backward(f, W, g, nbr, n_out, subm)
    assert torch.equal(dx2, dx) and torch.equal(dw2, dw)
    none, dw3 = dcl.ops.sparse_conv_backward(f, W, g, nbr, n_out, subm, need_dx=False)
    assert none is None and torch.equal(dw3, dw)
    fa, wa = f.clone().requires_grad_(True), W.clone().requires_grad_(True)
    dcl.autograd.SparseConvFn.apply(fa, wa, nbr, n_out, subm).backward(g)
    assert torch.equal(fa.grad, dx) and torch.equal(wa.grad, dw)


@pytest.mark.gpu
@pytest.mark.parametrize("case", cg.CASES_FAMILY, ids=cg.case_id)
def test_exact_input_gradient_under_every_decomposition(dcl, oracle, request, case):
    """the dX launch forced to whole tiles (-2), to 2- and 3-way aligned split-K, to an 8-way split (which 204 row tiles do not get:
    1632 partial tiles do not fit the scratch, the launch falls back to whole tiles), the automatic choice (stream-K with the
    combine inside the launch), and the plain VALU kernel (diagnostic library): the integer gradient each time.  The 256 -> 128
    case runs the general MFMA kernel, which has one form, under every setting"""
    c, nbr, n_out, f, W, g = _device_case(dcl, oracle, case, "exact")
    want_dx, want_dw = c["dX"].astype(np.float32), c["dW"].astype(np.float32)
    lib = enter_diag(dcl, request)
    try:
        for ns in (-2, 2, 3, 8, 0):
            lib.dcl_debug_conv_split(ns)
            dx, dw = dcl.ops.sparse_conv_backward(f, W, g, nbr, n_out, case[3])
            assert _where(dx.cpu().numpy(), want_dx, "input rows (split %d)" % ns) == ""
            assert _where(dw.cpu().numpy(), want_dw, "offsets k (diagnostic library)") == ""
    finally:
        lib.dcl_debug_conv_split(0)
    lib.dcl_debug_force_valu_conv(1)
    try:
        dx, _ = dcl.ops.sparse_conv_backward(f, W, g, nbr, n_out, case[3])
    finally:
        lib.dcl_debug_force_valu_conv(0)
    assert _where(dx.cpu().numpy(), want_dx, "input rows (VALU kernel)") == ""


# err / e32 measured on an MI355X (err = max |kernel - float64|, e32 = max |fp32 numpy oracle - float64| on the same operands):
#   case (rows)                 dX route                          dX err / e32    dW kernel, splits      dW err / e32
#   mid    7 ->  16 conv        VALU (16 -> 7)                    1.00            VALU, 32               1.50
#   mid   16 ->  32 subm        VALU (32 -> 16)                   1.00            VALU, 13               1.70
#   mid   32 ->  32 conv        filter-resident (32 -> 32)        5.59            MFMA 32x32, 32         1.25
#   mid   32 ->  64 subm        LDS-DMA 128x32 (64 -> 32)         2.98            MFMA 32x32, 13         1.65
#   mid   64 ->  64 conv        LDS-DMA 128x64 (64 -> 64)         3.23            MFMA 64x64, 32         1.17
#   mid   64 -> 128 subm        LDS-DMA 128x64 (128 -> 64)        3.74            MFMA 64x64, 13         1.83
#   mid  128 -> 128 conv        LDS-DMA 128x128 (128 -> 128)      4.65            MFMA 64x64, 32         1.25
#   mid  128 -> 256 subm        general MFMA (256 -> 128)         7.46            MFMA 64x64, 13         2.11
#   cap   32 ->  32 conv        filter-resident (32 -> 32)        4.64            MFMA 32x32, 64         1.00
#   cap    7 ->  16 conv        VALU (16 -> 7)                    1.00            VALU, 64               1.14
# The bound is twice the largest ratio seen, rounded up to a power of two -- taken for dX and dW apart, which is tighter than one
# factor for both: 2 x 7.46 -> 16 and 2 x 2.11 -> 8.  The MFMA routes of dX carry ONE fp32 accumulator through all 27 Cin' / 2
# steps of v_mfma_f32_32x32x2f32 (up to 3456 roundings in a row), the oracle adds each offset's Cin' products in BLAS blocks and
# then at most 27 partial results: the ratio grows with Cin' as the square root of the chain length would have it, and on the
# VALU route, which adds in the oracle's order, it is 1.  Absolute figures: dX err <= 2.5e-5 (cap 1.6e-4 .. 2.6e-4), dW err <=
# 6.2e-4 (cap 2.8e-2 .. 4.3e-2): 16 e32 and 8 e32 stay 3 and 8 times inside the older caps.
ROUNDING_K_DX = 16.0
ROUNDING_K_DW = 8.0


@pytest.mark.gpu
@pytest.mark.parametrize("case", cg.CASES_GAUSSIAN, ids=cg.case_id)
def test_gaussian_operands_round_like_the_fp32_oracle(dcl, oracle, case):
    """max |gpu - float64| <= ROUNDING_K_DX e32 (dX) and ROUNDING_K_DW e32 (dW), inside the older caps 2e-5 max(1, |dX|max) and
    5e-5 max(1, |dW|max).  Both sides are of order sqrt(terms) 2^-24 |sum|; the kernel adds up to 2560 rows one after another
    inside a split where BLAS adds in blocks"""
    c, nbr, n_out, f, W, g = _device_case(dcl, oracle, case, "gaussian")
    e32_dx, e32_dw = cg.fp32_oracle_error(oracle, case)
    dx, dw = dcl.ops.sparse_conv_backward(f, W, g, nbr, n_out, case[3])
    err_dx = float(np.abs(dx.cpu().numpy() - c["dX"]).max())
    err_dw = float(np.abs(dw.cpu().numpy() - c["dW"]).max())
    cap_dx, cap_dw = 2e-5 * max(1.0, float(np.abs(c["dX"]).max())), 5e-5 * max(1.0, float(np.abs(c["dW"]).max()))
    print("%s: dX err %.3g e32 %.3g ratio %.2f cap %.3g | dW err %.3g e32 %.3g ratio %.2f cap %.3g (max|dW| %.1f)" % (
        cg.case_id(case), err_dx, e32_dx, err_dx / e32_dx, cap_dx, err_dw, e32_dw, err_dw / e32_dw, cap_dw,
        float(np.abs(c["dW"]).max())))
    assert e32_dx > 0 and e32_dw > 0
    assert ROUNDING_K_DX * e32_dx <= cap_dx and ROUNDING_K_DW * e32_dw <= cap_dw      # a yardstick past the old cap would be a finding
    assert err_dx <= ROUNDING_K_DX * e32_dx
    assert err_dw <= ROUNDING_K_DW * e32_dw


def _pool_problem(dcl, oracle, padding):
    geo = cg.geometry(oracle, cg.POOL_SHAPE, False, padding=padding)
    nbr, n_out = _rulebook(dcl, geo, False)
    _, rf = oracle.indice_avgpool(np.zeros((geo["n_in"], 4), np.float32), geo["pairs"], geo["num"], n_out)
    return geo, nbr, n_out, rf


def _pool_gradient(dcl, nbr, n_in, n_out, c, G):
    f = torch.zeros((n_in, c), dtype=torch.float32, device="cuda").requires_grad_(True)
    dcl.autograd.SparseAvgPoolFn.apply(f, nbr, n_out).backward(cuda(G))
    return f.grad.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("c", cg.POOL_CHANNELS)
def test_avgpool_backward_bit_exact_at_training_size(dcl, oracle, c):
    from oracle import backward as ob
    geo, nbr, n_out, rf = _pool_problem(dcl, oracle, 1)
    G = np.random.default_rng(c).normal(size=(n_out, c)).astype(np.float32)
    want = ob.indice_avgpool_backward(geo["n_in"], G, geo["pairs"], geo["num"], rf)
    got = _pool_gradient(dcl, nbr, geo["n_in"], n_out, c, G)
    assert _where(got, want, "input rows") == ""
    ref, mag = cg.avgpool_backward_ref(geo["n_in"], G, geo["pairs"], geo["num"], rf)
    assert np.all(np.abs(got - ref) <= 28 * U * mag)


@pytest.mark.gpu
def test_avgpool_backward_rows_without_an_output_get_zero(dcl, oracle):
    """kernel 3, stride 2, padding 0: input rows on the last plane of an axis reach no output -- every inv entry of such a row is
    -1 and its gradient is exactly zero; every other row is bit-exact"""
    from oracle import backward as ob
    c = 64
    geo, nbr, n_out, rf = _pool_problem(dcl, oracle, 0)
    reached = np.zeros(geo["n_in"], bool)
    for k in range(27):
        reached[geo["pairs"][k, 0, :geo["num"][k]]] = True
    assert (~reached).sum() > 100
    inv = dcl.ops.rulebook_transpose(nbr, n_out, geo["n_in"]).cpu().numpy()
    assert np.array_equal((inv >= 0).any(0), reached) and inv.max() == n_out - 1
    G = np.random.default_rng(7).normal(size=(n_out, c)).astype(np.float32)
    G[G == 0] = 1.0
    want = ob.indice_avgpool_backward(geo["n_in"], G, geo["pairs"], geo["num"], rf)
    got = _pool_gradient(dcl, nbr, geo["n_in"], n_out, c, G)
    assert not got[~reached].any() and np.all(got[reached] != 0)
    assert _where(got, want, "input rows") == ""


@pytest.mark.gpu
def test_empty_sides_give_zero_gradients(dcl):
    """n_out == 0 and n_in == 0: zeros of the right shapes, no launch on a null pointer"""
    cin, cout = 32, 64
    W = cuda(cg.exact_array(np.random.default_rng(0), (27, cin, cout)))
    none = torch.full((27, 1), -1, dtype=torch.int32, device="cuda")
    f = cuda(cg.exact_array(np.random.default_rng(1), (5, cin)))
    dx, dw = dcl.ops.sparse_conv_backward(f, W, torch.zeros((0, cout), device="cuda"), none, 0, False)
    assert dx.shape == (5, cin) and dw.shape == (27, cin, cout) and not dx.any() and not dw.any()
    none7 = torch.full((27, 7), -1, dtype=torch.int32, device="cuda")
    g = cuda(cg.exact_array(np.random.default_rng(2), (7, cout)))
    dx, dw = dcl.ops.sparse_conv_backward(torch.zeros((0, cin), device="cuda"), W, g, none7, 7, False)
    assert dx.shape == (0, cin) and dw.shape == (27, cin, cout) and not dw.any()
    dx, dw = dcl.ops.sparse_conv_backward(torch.zeros((0, cin), device="cuda"), W, torch.zeros((0, cout), device="cuda"), none, 0, True)
    assert dx.shape == (0, cin) and not dw.any()
    none_dx, dw = dcl.ops.sparse_conv_backward(f, W, torch.zeros((0, cout), device="cuda"), none, 0, False, need_dx=False)
    assert none_dx is None and not dw.any()
    # the pool gradient likewise
    din = dcl.ops.sparse_avgpool_backward(torch.zeros((0, cin), device="cuda"), none, 0, 5, torch.zeros(1, dtype=torch.int32, device="cuda"))
    assert din.shape == (5, cin) and not din.any()
