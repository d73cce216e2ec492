"""The compact sparse-conv forward without a GPU (csrc/conv_fwd_compact.hip): dcl_sparse_conv_fwd_compact and its host twin are
declared with the documented argument lists, exported by both libraries and refuse bad arguments; the host twin -- the pinned
order in plain C++ -- replays the header's order step for step on a hand-made table, gives the integer result on exact operands
and stays within a multiple of the fp32 oracle's own error on Gaussian operands; the forward switch exists on every layer above."""
import ctypes as C
import inspect
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import conv_fwd_cases as fc
import conv_grad_cases as cg
from test_conv_pairs_abi import declarations

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_ARGS = ["const float *feat", "int n_in", "const int32_t *nbr", "int cap", "int n_out", "const float *W", "int cin", "int cout",
         "int kvol", "int subm", "float *out"]
WANT = {"dcl_sparse_conv_fwd_compact": _ARGS + ["dclStream_t stream"], "dcl_sparse_conv_fwd_compact_host": _ARGS}


def _libs(dcl):
    assert os.path.exists(dcl._native.DIAG_SO_PATH), "diagnostic library missing: build() makes it"
    return [("product", dcl._native.lib()), ("diag", C.CDLL(dcl._native.DIAG_SO_PATH))]


# ------------------------------------------------------------------------------------------- 1. the ABI
def test_header_declares_both_entries_and_both_libraries_export_them(dcl):
    decl = declarations()
    for name, args in WANT.items():
        assert name in decl, name
        assert decl[name] == args, (name, decl[name])
    for tag, lib in _libs(dcl):
        for name in WANT:
            assert hasattr(lib, name), (tag, name)
    for op in ("sparse_conv_compact", "sparse_conv_compact_host", "check_conv_fwd", "conv_fwd_form"):
        assert callable(getattr(dcl.ops, op)), op
    assert dcl.ops.CONV_FWD_FORMS == ("tiles", "compact")


_HOST = (C.c_int32 * 4096)()            # host memory stands in for device buffers: a refused call never dereferences them
_P = C.cast(_HOST, C.c_void_p)
_ODD = C.c_void_p(C.addressof(_HOST) + 2)


def _fwd(L, host, feat=_P, n_in=8, nbr=_P, cap=8, n_out=8, W=_P, cin=4, cout=4, kvol=27, subm=0, out=_P):
    a = (feat, n_in, nbr, cap, n_out, W, cin, cout, kvol, subm, out)
    return L.dcl_sparse_conv_fwd_compact_host(*a) if host else L.dcl_sparse_conv_fwd_compact(*(a + (None,)))


_BAD = [dict(kvol=0), dict(kvol=28), dict(cin=0), dict(cout=0), dict(cap=7), dict(feat=None), dict(nbr=None), dict(W=None),
        dict(out=None), dict(n_in=-1), dict(n_out=-1), dict(feat=_ODD), dict(nbr=_ODD), dict(W=_ODD), dict(out=_ODD),
        dict(cin=1 << 15, cout=1 << 15)]


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
@pytest.mark.parametrize("kw", _BAD, ids=lambda kw: ",".join(sorted(kw)))
def test_bad_arguments_return_einval_without_a_gpu(dcl, host, kw):
    for tag, lib in _libs(dcl):
        lib.dcl_last_error.restype = C.c_char_p
        assert _fwd(lib, host, **kw) == -1, tag
        assert b"invalid argument" in lib.dcl_last_error(), tag


def test_no_output_rows_return_zero_and_touch_nothing(dcl):
    for tag, lib in _libs(dcl):
        # the device entry too: it returns before any GPU work
        assert _fwd(lib, False, n_out=0, nbr=None, out=None) == 0, tag
        assert _fwd(lib, True, n_out=0, nbr=None, out=None) == 0, tag
        assert _fwd(lib, True, n_out=0, cap=0, n_in=0, feat=None, nbr=None, out=None) == 0, tag
    # no input rows: every entry is out of range, every element +0 -- and feat may be NULL
    nbr = np.zeros((27, 8), np.int32)
    W = np.ones((27, 4, 4), np.float32)
    out = np.full((8, 4), np.nan, np.float32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)                                  # noqa: E731
    assert dcl._native.lib().dcl_sparse_conv_fwd_compact_host(None, 0, vp(nbr), 8, 8, vp(W), 4, 4, 27, 0, vp(out)) == 0
    assert not out.any() and not np.signbit(out).any()


# ------------------------------------------------------------------------------------------- 2. the hand-made table
def test_hand_made_table_is_what_it_says():
    nbr, n_in = fc.HAND_NBR.astype(np.int64), fc.HAND_N_IN
    assert nbr.shape == (27, fc.HAND_N_OUT)
    ok = (nbr >= 0) & (nbr < n_in)
    assert np.array_equal(ok, fc.HAND_PRESENT)
    cnt = ok.sum(axis=1)
    # "every row" is every row but the one that has no neighbour at all: the two properties exclude each other in one row
    assert cnt[fc.HAND_ALL] == fc.HAND_N_OUT - 1 and cnt[fc.HAND_32] == 32 and cnt[fc.HAND_33] == 33 and cnt[fc.HAND_ONE] == 1
    assert all(cnt[k] == 0 for k in fc.HAND_NONE) and len(fc.HAND_NONE) >= 3
    assert ok[:, fc.HAND_EMPTY].sum() == 0 and (ok.sum(axis=0) > 0).sum() == fc.HAND_N_OUT - 1
    assert (nbr >= n_in).sum() >= 10 and (nbr < -1).sum() >= 10 and (nbr == 2 ** 30).sum() == 1
    assert ok[13].sum() > 0                                                      # the centre is present: subm visits it first


def round32(fr):
    """nearest-even float32 of an exact fraction"""
    d = float(fr)                                                                # (correctly rounded to float64 by CPython)
    f = np.float32(d)
    lo, hi = np.nextafter(f, np.float32(-np.inf)), np.nextafter(f, np.float32(np.inf))
    best = min(abs(Fraction(float(c)) - fr) for c in (lo, f, hi))
    ties = [c for c in (lo, f, hi) if abs(Fraction(float(c)) - fr) == best]
    if len(ties) == 1:
        return ties[0]
    return [c for c in ties if (c.view(np.uint32) & 1) == 0][0]


@pytest.mark.parametrize("subm", [False, True], ids=["conv", "subm"])
def test_host_twin_is_the_pinned_order_of_the_header(dcl, subm):
    """a handful of elements by hand: offsets in visiting order; per offset a chain of its own from +0, channels ascending, one
    fused step each; one fp32 add per offset -- in exact rational arithmetic rounded once per step"""
    cin, cout = 5, 3
    X, W = fc.hand_operands(cin, cout, exact=False)
    got = dcl.ops.sparse_conv_compact_host(X, fc.HAND_NBR, fc.HAND_N_OUT, W, subm, n_in=fc.HAND_N_IN)
    assert np.isfinite(got).all()                                                # the NaN rows were never read
    rows33 = np.flatnonzero(fc.HAND_PRESENT[fc.HAND_33])
    centre_rows = np.flatnonzero(fc.HAND_PRESENT[13] & (fc.HAND_PRESENT.sum(axis=0) >= 4))
    # the first pair of the 33-row offset, its 32nd and its 33rd (the block boundary), the one-row offset's row, a row with the centre
    picks = [(int(rows33[0]), 0), (int(rows33[31]), 2), (int(rows33[32]), 1), (fc.HAND_ONE_ROW, 2), (int(centre_rows[0]), 0),
             (int(centre_rows[-1]), 1)]
    for o, co in picks:
        acc = np.float32(0)
        nb = fc.hand_neighbours(o, subm)
        assert len(nb) >= 2
        for k, i in nb:
            part = np.float32(0)
            for ci in range(cin):
                part = round32(Fraction(float(X[i, ci])) * Fraction(float(W[k, ci, co])) + Fraction(float(part)))
            acc = round32(Fraction(float(acc)) + Fraction(float(part)))
        assert acc == got[o, co], (o, co)
    assert not got[fc.HAND_EMPTY].any() and not np.signbit(got[fc.HAND_EMPTY]).any()       # +0, sign bit included


@pytest.mark.parametrize("cin,cout", [(32, 32), (5, 3), (1, 1), (33, 40), (128, 128)])
def test_host_twin_on_the_hand_made_table(dcl, cin, cout):
    X, W = fc.hand_operands(cin, cout, exact=True)
    assert np.isnan(X[fc.HAND_N_IN:]).all()
    want = fc.hand_ref(np.nan_to_num(X), W).astype(np.float32)
    got = dcl.ops.sparse_conv_compact_host(X, fc.HAND_NBR, fc.HAND_N_OUT, W, False, n_in=fc.HAND_N_IN)
    assert np.isfinite(got).all()
    assert np.array_equal(got, want)                                             # out-of-range entries took no part
    assert not got[fc.HAND_EMPTY].any() and not np.signbit(got[fc.HAND_EMPTY]).any()
    # the same table inside a larger cap, and with fewer rows asked for: the same bits
    Xg, Wg = fc.hand_operands(cin, cout, exact=False)
    first = dcl.ops.sparse_conv_compact_host(Xg, fc.HAND_NBR, fc.HAND_N_OUT, Wg, True, n_in=fc.HAND_N_IN)
    wide = fc.hand_embedded(203, np.random.default_rng(5))
    assert np.array_equal(dcl.ops.sparse_conv_compact_host(Xg, wide, fc.HAND_N_OUT, Wg, True, n_in=fc.HAND_N_IN), first)
    assert np.array_equal(dcl.ops.sparse_conv_compact_host(Xg, wide, 33, Wg, True, n_in=fc.HAND_N_IN), first[:33])


# ------------------------------------------------------------------------------------------- 3. exact operands
@pytest.mark.parametrize("case", fc.CASES, ids=cg.case_id)
def test_host_twin_gives_the_integer_result(dcl, oracle, case):
    want = fc.ref(oracle, case, "exact")
    assert 0 < np.abs(want).max() < cg.EXACT_LIMIT
    got = fc.twin(dcl, oracle, case, "exact")
    assert got.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(got, want.astype(np.float32))
    assert not np.signbit(got[got == 0]).any()


# ------------------------------------------------------------------------------------------- 4. gaussian operands
# err / e32 of the host twin, measured on the CPU (err = max |twin - float64|, e32 = max |oracle.native.indice_conv in fp32 -
# float64| on the same operands, conv_fwd_cases.fp32_oracle_error); the largest ratio of each width over the seven geometries:
#   16 ->  32   1.00      32 ->  32   1.00      32 ->  64   1.00      64 ->  64   1.00      64 -> 128   1.00
#  128 -> 128   1.00     128 -> 256   1.00       7 ->  16   1.00       5 ->   3   1.00       1 ->   1   1.00      33 -> 40   1.00
# (77 cases; 2e-5 max(1, |out|max) lies between 61 and 251 e32.)  Every ratio is 1.00 because the pinned order IS the oracle's
# own association -- per offset an ascending-ci fmaf chain, then one fp32 add, offsets in the reference's visiting order -- so
# the twin meets the oracle's bits and its error is the oracle's.  The bound is twice the largest ratio seen, rounded up to a
# power of two -- the rule of test_conv_dgrad_abi.py and of ROUNDING_K_DX of test_gpu_conv_backward.py: 2 x 1.00 -> 2.
ROUNDING_K = 2.0


@pytest.mark.parametrize("case", fc.CASES, ids=cg.case_id)
def test_host_twin_rounds_like_the_fp32_oracle(dcl, oracle, case):
    want = fc.ref(oracle, case, "gaussian")
    e32 = fc.fp32_oracle_error(oracle, case)
    err = float(np.abs(fc.twin(dcl, oracle, case, "gaussian").astype(np.float64) - want).max())
    cap = 2e-5 * max(1.0, float(np.abs(want).max()))
    print("%s: err %.3g e32 %.3g ratio %.2f cap %.3g (%.1f e32)" % (cg.case_id(case), err, e32, err / e32, cap, cap / e32))
    assert e32 > 0
    assert ROUNDING_K * e32 <= cap                                               # a yardstick past the older cap would be a finding
    assert err <= ROUNDING_K * e32


# ------------------------------------------------------------------------------------------- 5. plumbing
def test_the_switch_exists_on_every_layer(dcl):
    with pytest.raises(ValueError):
        dcl.ops.check_conv_fwd("x")
    with pytest.raises(ValueError):
        dcl.ops.check_conv_fwd(None)
    assert dcl.ops.check_conv_fwd("tiles") == "tiles" and dcl.ops.check_conv_fwd("compact") == "compact"
    assert inspect.signature(dcl.DCL_Net.Network.__init__).parameters["train_conv_fwd"].default == "tiles"
    assert dcl.spconv.SparseConvolution.fwd == "tiles"
    assert dcl.spconv.SubMConv3d(4, 4, 3).fwd == "tiles" and dcl.spconv.SparseConv3d(4, 8, 3).fwd == "tiles"
    assert inspect.signature(dcl.autograd.SparseConvFn.forward).parameters["fwd"].default == "tiles"
    assert inspect.signature(dcl.ops.sparse_conv).parameters["form"].default == "tiles"
    src = open(os.path.join(ROOT, "tools", "train_step.py")).read()
    assert re.search(r'add_argument\("--conv-fwd", choices=\("tiles", "compact"\), default="tiles"\)', src)
    assert "train_conv_fwd=args.conv_fwd" in src


def test_the_width_table_holds_dilating_layers_only(dcl):
    table = dcl.ops.CONV_FWD_COMPACT_WIDTHS
    assert all(w in fc.DILATING_WIDTHS for w in table)
    for cin, cout in fc.WIDTHS + fc.DILATING_WIDTHS:
        assert dcl.ops.conv_fwd_form(cin, cout, True, "compact") == "tiles"                    # never a subm layer
        assert dcl.ops.conv_fwd_form(cin, cout, False, "tiles") == "tiles"
        want = "compact" if (cin, cout) in table else "tiles"
        assert dcl.ops.conv_fwd_form(cin, cout, False, "compact") == want, (cin, cout)
    assert dcl.ops.conv_fwd_form(7, 16, False, "compact") == "tiles"                           # the stem
    with pytest.raises(ValueError):
        dcl.ops.conv_fwd_form(32, 32, False, "x")


def test_network_sets_fwd_by_the_width_table(dcl):
    cfg = dcl.synth.default_cfg(256, 256)
    with pytest.raises(ValueError):
        dcl.DCL_Net.Network(cfg, mode="train", train_conv_fwd="x")
    convs = lambda net: [m for m in net.modules() if isinstance(m, dcl.spconv.SparseConvolution)]      # noqa: E731
    net = dcl.DCL_Net.Network(cfg, mode="train")
    assert net.train_conv_fwd == "tiles" and len(convs(net)) == 16 and {m.fwd for m in convs(net)} == {"tiles"}
    keys = list(net.state_dict().keys())
    net = dcl.DCL_Net.Network(cfg, mode="train", train_conv_fwd="compact")
    assert net.train_conv_fwd == "compact" and list(net.state_dict().keys()) == keys
    table = dcl.ops.CONV_FWD_COMPACT_WIDTHS
    for m in convs(net):
        compact = not m.subm and (m.in_channels, m.out_channels) in table
        assert m.fwd == ("compact" if compact else "tiles"), (m.in_channels, m.out_channels, m.subm)
        assert m.wgrad == "rows" and m.dgrad == "conv"                           # independent of the other switches
    assert sum(m.fwd == "compact" for m in convs(net)) == 2 * len(table)
