"""The direct sparse-conv input gradient without a GPU (csrc/conv_dgrad.hip): dcl_sparse_conv_dgrad and its host twin are
declared with the documented argument lists, exported by both libraries and refuse bad arguments; the host twin -- the pinned
order in plain C++ -- gives the integer gradient on exact operands, holds the neighbour rule on a hand-made table, and stays
within a multiple of the fp32 numpy oracle's own error on Gaussian operands; the dgrad switch exists on every layer above."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import conv_dgrad_cases as dc
import conv_grad_cases as cg
from test_conv_pairs_abi import declarations

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_ARGS = ["const float *dout", "int n_out", "const int32_t *inv", "int cap_in", "int n_in", "const float *W", "int cin", "int cout",
         "int kvol", "float *dx"]
WANT = {"dcl_sparse_conv_dgrad": _ARGS + ["dclStream_t stream"], "dcl_sparse_conv_dgrad_host": _ARGS}


def _libs(dcl):
    assert os.path.exists(dcl._native.DIAG_SO_PATH), "diagnostic library missing: build() makes it"
    return [("product", dcl._native.lib()), ("diag", C.CDLL(dcl._native.DIAG_SO_PATH))]


# ------------------------------------------------------------------------------------------- 1. the ABI
def test_header_declares_both_entries_and_the_abi_version_stays(dcl):
    decl = declarations()
    for name, args in WANT.items():
        assert name in decl, name
        assert decl[name] == args, (name, decl[name])
    header = open(os.path.join(ROOT, "include", "dclnet_hip.h")).read()
    assert re.search(r"^#define DCL_ABI_VERSION 2\s*$", header, flags=re.M)
    assert dcl._native.ABI_VERSION == 2
    for tag, lib in _libs(dcl):
        assert int(lib.dcl_abi_version()) == 2, tag


def test_both_libraries_export_them(dcl):
    for tag, lib in _libs(dcl):
        for name in WANT:
            assert hasattr(lib, name), (tag, name)
    for op in ("sparse_conv_dgrad", "sparse_conv_dgrad_host", "check_conv_dgrad"):
        assert callable(getattr(dcl.ops, op)), op
    assert dcl.ops.CONV_DGRAD_FORMS == ("conv", "direct")


_HOST = (C.c_int32 * 4096)()            # host memory stands in for device buffers: a refused call never dereferences them
_P = C.cast(_HOST, C.c_void_p)
_ODD = C.c_void_p(C.addressof(_HOST) + 2)


def _dgrad(L, host, dout=_P, n_out=8, inv=_P, cap_in=8, n_in=8, W=_P, cin=4, cout=4, kvol=27, dx=_P):
    a = (dout, n_out, inv, cap_in, n_in, W, cin, cout, kvol, dx)
    return L.dcl_sparse_conv_dgrad_host(*a) if host else L.dcl_sparse_conv_dgrad(*(a + (None,)))


_BAD = [dict(dout=None), dict(inv=None), dict(W=None), dict(dx=None), dict(kvol=0), dict(kvol=28), dict(n_out=-1), dict(n_in=-1),
        dict(cin=0), dict(cout=0), dict(cout=-3), dict(cap_in=7), dict(cap_in=0, n_in=0), dict(dout=_ODD), dict(inv=_ODD), dict(W=_ODD),
        dict(dx=_ODD), dict(cin=1 << 15, cout=1 << 15)]


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
@pytest.mark.parametrize("kw", _BAD, ids=lambda kw: ",".join(sorted(kw)))
def test_bad_arguments_return_einval_without_a_gpu(dcl, host, kw):
    for tag, lib in _libs(dcl):
        lib.dcl_last_error.restype = C.c_char_p
        assert _dgrad(lib, host, **kw) == -1, tag
        assert b"invalid argument" in lib.dcl_last_error(), tag


def test_empty_sides_are_not_errors(dcl):
    for tag, lib in _libs(dcl):
        # no input rows: nothing to write, on the device entry as well (it returns before any GPU work)
        assert _dgrad(lib, False, n_in=0, inv=None, dx=None) == 0, tag
        assert _dgrad(lib, True, n_in=0, inv=None, dx=None) == 0, tag
        assert _dgrad(lib, True, n_in=0, n_out=0, dout=None, inv=None, dx=None) == 0, tag
    # no dout rows: every entry is out of range, every element +0 -- and dout may be NULL
    inv = np.zeros((27, 8), np.int32)
    W = np.ones((27, 4, 4), np.float32)
    dx = np.full((8, 4), np.nan, np.float32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)                                  # noqa: E731
    assert dcl._native.lib().dcl_sparse_conv_dgrad_host(None, 0, vp(inv), 8, 8, vp(W), 4, 4, 27, vp(dx)) == 0
    assert not dx.any() and not np.signbit(dx).any()


# ------------------------------------------------------------------------------------------- 2. exact operands
@pytest.mark.parametrize("case", dc.CASES, ids=cg.case_id)
def test_host_twin_gives_the_integer_gradient(dcl, oracle, case):
    c = cg.conv_case(oracle, case, "exact")
    assert np.abs(c["dX"]).max() < cg.EXACT_LIMIT and np.abs(c["dX"]).max() > 0
    got = dc.twin(dcl, oracle, case, "exact")
    assert got.dtype == np.float32 and got.shape == c["dX"].shape
    assert np.array_equal(got, c["dX"].astype(np.float32))
    assert not np.signbit(got[got == 0]).any()


# ------------------------------------------------------------------------------------------- 3. the hand-made table
def test_hand_made_table_is_what_it_says():
    assert dc.HAND_INV.shape == (dc.HAND_KVOL, dc.HAND_N_IN)
    for i in range(dc.HAND_N_IN):
        col = dc.HAND_INV[:, i].astype(np.int64)
        assert [(k, int(o)) for k, o in enumerate(col) if 0 <= o < dc.HAND_N_OUT] == dc.HAND_NEIGHBOURS[i], i
    assert (dc.HAND_INV[:, 3] == -1).all() and (dc.HAND_INV[1] == -1).all()
    assert (dc.HAND_INV >= dc.HAND_N_OUT).sum() >= 3 and (dc.HAND_INV < -1).sum() >= 2


@pytest.mark.parametrize("cin,cout", [(16, 32), (5, 3), (1, 1), (33, 40), (128, 256)])
def test_host_twin_on_the_hand_made_table(dcl, cin, cout):
    W, G = dc.hand_operands(cin, cout, exact=True)
    assert np.isnan(G[dc.HAND_N_OUT:]).all()
    want = dc.hand_ref(W, np.nan_to_num(G)).astype(np.float32)
    got = dcl.ops.sparse_conv_dgrad_host(G, dc.HAND_INV, dc.HAND_N_IN, W, n_out=dc.HAND_N_OUT)
    assert np.isfinite(got).all()                                                # the NaN rows were never read
    assert np.array_equal(got, want)                                             # out-of-range entries took no part
    assert not got[3].any() and not np.signbit(got[3]).any()                     # the all -1 row: +0
    # the same table inside a larger cap_in, and with fewer rows asked for: the same bits
    Wg, Gg = dc.hand_operands(cin, cout, exact=False)
    first = dcl.ops.sparse_conv_dgrad_host(Gg, dc.HAND_INV, dc.HAND_N_IN, Wg, n_out=dc.HAND_N_OUT)
    assert np.isfinite(first).all() and np.abs(first - dc.hand_ref(Wg, np.nan_to_num(Gg))).max() < 1e-4
    wide = dc.hand_embedded(37, np.random.default_rng(5))
    assert np.array_equal(dcl.ops.sparse_conv_dgrad_host(Gg, wide, dc.HAND_N_IN, Wg, n_out=dc.HAND_N_OUT), first)
    assert np.array_equal(dcl.ops.sparse_conv_dgrad_host(Gg, wide, 5, Wg, n_out=dc.HAND_N_OUT), first[:5])


def test_host_twin_is_the_fmaf_chain_of_the_header(dcl):
    """one element by hand: offsets ascending, channels ascending, one fused step each -- in exact rational arithmetic rounded
    once per step (a float64 product of two float32 is exact; the sum is rounded to float32 through Python's exact fractions)"""
    from fractions import Fraction
    W, G = dc.hand_operands(5, 3, exact=False)
    got = dcl.ops.sparse_conv_dgrad_host(G, dc.HAND_INV, dc.HAND_N_IN, W, n_out=dc.HAND_N_OUT)

    def round32(fr):                                                             # nearest-even float32 of an exact fraction
        d = float(fr)                                                            # (correctly rounded to float64 by CPython)
        f = np.float32(d)
        lo, hi = np.nextafter(f, np.float32(-np.inf)), np.nextafter(f, np.float32(np.inf))
        best = min((abs(Fraction(float(c)) - fr), i) for i, c in enumerate((lo, f, hi)))
        ties = [c for c in (lo, f, hi) if abs(Fraction(float(c)) - fr) == best[0]]
        if len(ties) == 1:
            return ties[0]
        return [c for c in ties if (c.view(np.uint32) & 1) == 0][0]

    for i, ci in ((0, 0), (2, 4), (4, 1), (7, 3)):
        acc = np.float32(0)
        for k, o in dc.HAND_NEIGHBOURS[i]:
            for co in range(3):
                acc = round32(Fraction(float(G[o, co])) * Fraction(float(W[k, ci, co])) + Fraction(float(acc)))
        assert acc == got[i, ci], (i, ci)


# ------------------------------------------------------------------------------------------- 4. gaussian operands
# err / e32 of the host twin, measured on the CPU (err = max |twin - float64|, e32 = max |fp32 numpy oracle - float64| of dX on
# the same operands, conv_grad_cases.fp32_oracle_error); the largest ratio of each width over the seven geometries:
#   16 ->  32   6.18      32 ->  32   6.92      32 ->  64   8.45      64 ->  64   7.44      64 -> 128   8.11
#  128 -> 128  11.18     128 -> 256   9.13       7 ->  16   5.54       5 ->   3   2.25       1 ->   1   1.36      33 -> 40   5.96
# (77 cases; 2e-5 max(1, |dX|max) lies between 47 and 112 e32, so 32 e32 stays inside the older cap.)
# The twin carries ONE accumulator through all neighbours x cout steps (up to 27 * 256 roundings in a row); the oracle adds each
# offset's cout products in BLAS blocks and then at most 27 partial results: the ratio grows with cout.  The bound is twice the
# largest ratio seen, rounded up to a power of two, as for ROUNDING_K_DX of test_gpu_conv_backward.py: 2 x 11.18 -> 32.  The shapes
# here are small, so e32, a maximum over fewer elements, is smaller against the twin's than at training size (7.46 there).
ROUNDING_K = 32.0


@pytest.mark.parametrize("case", dc.CASES, ids=cg.case_id)
def test_host_twin_rounds_like_the_fp32_oracle(dcl, oracle, case):
    c = cg.conv_case(oracle, case, "gaussian")
    e32 = cg.fp32_oracle_error(oracle, case)[0]
    err = float(np.abs(dc.twin(dcl, oracle, case, "gaussian").astype(np.float64) - c["dX"]).max())
    cap = 2e-5 * max(1.0, float(np.abs(c["dX"]).max()))
    print("%s: dX err %.3g e32 %.3g ratio %.2f cap %.3g" % (cg.case_id(case), err, e32, err / e32, cap))
    assert e32 > 0
    assert ROUNDING_K * e32 <= cap                                               # a yardstick past the older cap would be a finding
    assert err <= ROUNDING_K * e32


# ------------------------------------------------------------------------------------------- 5. plumbing
def test_the_switch_exists_on_every_layer(dcl):
    with pytest.raises(ValueError):
        dcl.ops.check_conv_dgrad("rows")
    with pytest.raises(ValueError):
        dcl.ops.check_conv_dgrad(None)
    assert dcl.ops.check_conv_dgrad("direct") == "direct" and dcl.ops.check_conv_dgrad("conv") == "conv"
    assert inspect.signature(dcl.DCL_Net.Network.__init__).parameters["train_conv_dgrad"].default == "conv"
    assert dcl.spconv.SubMConv3d(4, 4, 3).dgrad == "conv" and dcl.spconv.SparseConv3d(4, 8, 3).dgrad == "conv"
    assert inspect.signature(dcl.autograd.SparseConvFn.forward).parameters["dgrad"].default == "conv"
    assert inspect.signature(dcl.ops.sparse_conv_backward).parameters["dgrad"].default == "conv"
    assert inspect.signature(dcl.ops.sparse_conv_backward).parameters["wgrad"].default == "rows"
    src = open(os.path.join(ROOT, "tools", "train_step.py")).read()
    assert re.search(r'add_argument\("--conv-dgrad", choices=\("conv", "direct"\), default="conv"\)', src)
    assert "train_conv_dgrad=args.conv_dgrad" in src


def test_network_sets_dgrad_by_the_width_table(dcl):
    cfg = dcl.synth.default_cfg(256, 256)
    with pytest.raises(ValueError):
        dcl.DCL_Net.Network(cfg, mode="train", train_conv_dgrad="nope")
    convs = lambda net: [m for m in net.modules() if isinstance(m, dcl.spconv.SparseConvolution)]      # noqa: E731
    net = dcl.DCL_Net.Network(cfg, mode="train")
    assert net.train_conv_dgrad == "conv" and len(convs(net)) == 16 and {m.dgrad for m in convs(net)} == {"conv"}
    net = dcl.DCL_Net.Network(cfg, mode="train", train_conv_dgrad="direct")
    assert net.train_conv_dgrad == "direct"
    table = dcl.ops.CONV_DGRAD_DIRECT_WIDTHS
    assert all(w in dc.BACKBONE_WIDTHS for w in table)
    for m in convs(net):
        want = "direct" if (m.in_channels, m.out_channels) in table else "conv"
        assert m.dgrad == want == dcl.ops.conv_dgrad_form(m.in_channels, m.out_channels), (m.in_channels, m.out_channels)
        assert m.wgrad == "rows"
    assert dcl.ops.conv_dgrad_form(16, 32, "conv") == "conv"
