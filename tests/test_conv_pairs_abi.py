"""The pair-walking sparse-conv weight gradient's entry points (dcl_conv_pairs*, dcl_sparse_conv_wgrad_pairs;
csrc/conv_wgrad_pairs.hip) are declared with the documented argument lists, exported by both libraries, and answer their size
queries and bad arguments without a GPU; the host twin of the pair list holds the contract on a synthetic rulebook; Network's
train_conv_wgrad switch validates its value."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import conv_pairs_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_LIST = ["int32_t *head", "int32_t *pair_in", "int32_t *pair_out", "int32_t *split_tab"]
_TABLE = ["const int32_t *nbr", "int cap", "int kvol", "int n_out", "int n_in", "int max_pairs"]
WANT = {
    "dcl_conv_pairs_ws_bytes": ["int kvol", "int n_out", "int64_t *bytes_host"],
    "dcl_conv_pairs_max_splits": ["int max_pairs", "int kvol", "int32_t *splits_host"],
    "dcl_conv_pairs": _TABLE + _LIST + ["void *ws", "int64_t ws_bytes", "dclStream_t stream"],
    "dcl_conv_pairs_host": _TABLE + _LIST,
    "dcl_sparse_conv_wgrad_pairs": ["const float *feat", "int n_in", "const float *dout", "int n_out", "int cin", "int cout",
                                    "int kvol", "const int32_t *head", "const int32_t *pair_in", "const int32_t *pair_out",
                                    "const int32_t *split_tab", "int max_splits", "float *partial", "float *dW",
                                    "dclStream_t stream"],
}


def _header():
    return open(os.path.join(ROOT, "include", "dclnet_hip.h")).read()


def _define(name):
    m = re.search(r"^#define %s (\d+)\s*$" % name, _header(), flags=re.M)
    assert m, "include/dclnet_hip.h must define %s" % name
    return int(m.group(1))


def split_pairs():
    return _define("DCL_CONV_PAIRS_SPLIT")


def declarations():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    out = {}
    for m in re.finditer(r"\bint\s+(dcl_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        out[m.group(1)] = [re.sub(r"\s+", " ", a).strip() for a in m.group(2).split(",")]
    return out


def _libs(dcl):
    assert os.path.exists(dcl._native.DIAG_SO_PATH), "diagnostic library missing: build() makes it"
    return [("product", dcl._native.lib()), ("diag", C.CDLL(dcl._native.DIAG_SO_PATH))]


def test_header_declares_the_entries_and_the_split_constant(dcl):
    decl = declarations()
    for name, args in WANT.items():
        assert name in decl, name
        assert decl[name] == args, (name, decl[name])
    assert split_pairs() in (512, 1024)
    assert dcl.ops.CONV_PAIRS_SPLIT == split_pairs()
    assert dcl.ops.CONV_PAIRS_HEAD == _define("DCL_CONV_PAIRS_HEAD") == pc.HEAD


def test_both_libraries_export_them(dcl):
    for tag, lib in _libs(dcl):
        for name in WANT:
            assert hasattr(lib, name), (tag, name)
    for op in ("conv_pairs", "conv_pairs_host", "sparse_conv_wgrad_pairs"):
        assert callable(getattr(dcl.ops, op)), op


def test_workspace_and_split_bound_equal_their_formulas(dcl):
    S = split_pairs()
    for tag, lib in _libs(dcl):
        for max_pairs in (0, 1, S - 1, S, S + 1, 27 * 4096):
            for kvol in (27, 1):
                s = C.c_int32(-7)
                assert lib.dcl_conv_pairs_max_splits(max_pairs, kvol, C.byref(s)) == 0, (tag, max_pairs)
                assert s.value == max_pairs // S + kvol, (tag, max_pairs, kvol, s.value)
        for n_out in (0, 1, 1023, 1024, 1025, 4096, 163673):
            b = C.c_int64(-7)
            assert lib.dcl_conv_pairs_ws_bytes(27, n_out, C.byref(b)) == 0, (tag, n_out)
            assert b.value == 4 * 27 * max(1, -(-n_out // 1024)), (tag, n_out, b.value)


_HOST = (C.c_int32 * 1024)()            # host memory stands in for device buffers: a refused call never dereferences them
_P = C.cast(_HOST, C.c_void_p)
_ODD = C.c_void_p(C.addressof(_HOST) + 2)


def _pairs(L, host=False, nbr=_P, cap=8, kvol=27, n_out=8, n_in=8, max_pairs=16, head=_P, pin=_P, pout=_P, tab=_P, ws=_P,
           ws_bytes=4096):
    if host:
        return L.dcl_conv_pairs_host(nbr, cap, kvol, n_out, n_in, max_pairs, head, pin, pout, tab)
    return L.dcl_conv_pairs(nbr, cap, kvol, n_out, n_in, max_pairs, head, pin, pout, tab, ws, C.c_int64(ws_bytes), None)


def _wgrad(L, feat=_P, n_in=8, dout=_P, n_out=8, cin=8, cout=8, kvol=27, head=_P, pin=_P, pout=_P, tab=_P, max_splits=27,
           partial=_P, dW=_P):
    return L.dcl_sparse_conv_wgrad_pairs(feat, n_in, dout, n_out, cin, cout, kvol, head, pin, pout, tab, max_splits, partial, dW,
                                         None)


_BAD_LIST = [dict(nbr=None), dict(head=None), dict(pin=None), dict(pout=None), dict(tab=None), dict(kvol=0), dict(kvol=28),
             dict(n_out=-1), dict(n_in=-1), dict(cap=7), dict(max_pairs=-1), dict(max_pairs=1 << 30), dict(nbr=_ODD),
             dict(tab=_ODD)]


@pytest.mark.parametrize("call", [
    lambda L: L.dcl_conv_pairs_ws_bytes(0, 5, C.byref(C.c_int64(0))),
    lambda L: L.dcl_conv_pairs_ws_bytes(27, -1, C.byref(C.c_int64(0))),
    lambda L: L.dcl_conv_pairs_ws_bytes(27, 5, None),
    lambda L: L.dcl_conv_pairs_max_splits(-1, 27, C.byref(C.c_int32(0))),
    lambda L: L.dcl_conv_pairs_max_splits(5, 28, C.byref(C.c_int32(0))),
    lambda L: L.dcl_conv_pairs_max_splits(5, 27, None),
] + [lambda L, kw=kw: _pairs(L, **kw) for kw in _BAD_LIST] + [lambda L, kw=kw: _pairs(L, host=True, **kw) for kw in _BAD_LIST] + [
    lambda L: _pairs(L, ws=None),
    lambda L: _pairs(L, ws_bytes=4 * 27 - 1),                                   # a short workspace
    lambda L: _wgrad(L, feat=None),
    lambda L: _wgrad(L, dout=None),
    lambda L: _wgrad(L, head=None),
    lambda L: _wgrad(L, pin=None),
    lambda L: _wgrad(L, pout=None),
    lambda L: _wgrad(L, tab=None),
    lambda L: _wgrad(L, partial=None),
    lambda L: _wgrad(L, dW=None),
    lambda L: _wgrad(L, feat=_ODD),
    lambda L: _wgrad(L, cin=0),
    lambda L: _wgrad(L, cout=-2),
    lambda L: _wgrad(L, kvol=28),
    lambda L: _wgrad(L, n_in=-1),
    lambda L: _wgrad(L, max_splits=0),
])
def test_bad_arguments_return_einval_without_a_gpu(dcl, call):
    for tag, lib in _libs(dcl):
        lib.dcl_last_error.restype = C.c_char_p
        assert call(lib) == -1, tag
        assert b"invalid argument" in lib.dcl_last_error(), tag


def test_synthetic_rulebook_is_what_it_says():
    S = split_pairs()
    nbr, counts = pc.synthetic_nbr(S)
    assert nbr.shape == (27, pc.CAP) and nbr.dtype == np.int32
    assert counts[:10] == [0, 1, 2, 15, 16, 17, S - 1, S, S + 1, 2 * S + 1]
    live = nbr[:, :pc.N_OUT]
    ok = (live >= 0) & (live < pc.N_IN)
    assert ok.sum(1).tolist() == counts
    assert sorted(set(live[~ok].tolist())) == sorted(pc.NOT_A_PAIR)
    for k in range(27):                                                          # an input row meets an offset at most once
        assert np.unique(live[k][ok[k]]).size == counts[k]
    tail = nbr[:, pc.N_OUT:]
    assert ((tail >= 0) & (tail < pc.N_IN)).all()                                # valid-looking, and never pairs


def test_host_twin_holds_the_contract(dcl):
    S = split_pairs()
    nbr, counts = pc.synthetic_nbr(S)
    max_pairs = 27 * min(pc.N_IN, pc.N_OUT)
    want = pc.pairs_ref(nbr, pc.N_OUT, pc.N_IN, max_pairs, S)
    got = dcl.ops.conv_pairs_host(nbr, pc.N_OUT, pc.N_IN)
    assert got["max_pairs"] == max_pairs and got["max_splits"] == max_pairs // S + 27
    assert pc.same_list(got, want) == ""
    head = got["head"]
    assert head[:27].tolist() == counts and head[pc.HEAD_OVERFLOW] == 0
    assert head[pc.HEAD_START:pc.HEAD_START + 28].tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist()
    assert head[pc.HEAD_NSPLIT] == sum(-(-c // S) for c in counts) <= got["max_splits"]
    for k in range(27):                                                          # ascending o inside every offset
        lo, hi = head[pc.HEAD_START + k], head[pc.HEAD_START + k + 1]
        assert np.all(np.diff(got["pair_out"][lo:hi]) > 0)
        assert np.array_equal(nbr[k, got["pair_out"][lo:hi]], got["pair_in"][lo:hi])
    tab = got["split_tab"][:head[pc.HEAD_NSPLIT]]
    assert np.all(np.diff(tab[:, 0]) >= 0) and tab[:, 2].min() >= 1 and tab[:, 2].max() <= S
    assert int(tab[:, 2].sum()) == sum(counts)
    # nothing past the stored pairs or the used splits was written
    assert (got["pair_in"][sum(counts):] == -1).all() and (got["split_tab"][head[pc.HEAD_NSPLIT]:] == -1).all()
    # the same list whatever the pitch of the table
    wide = np.full((27, pc.CAP + 37), 5, np.int32)
    wide[:, :pc.CAP] = nbr
    assert pc.same_list(dcl.ops.conv_pairs_host(wide, pc.N_OUT, pc.N_IN), want) == ""


@pytest.mark.parametrize("max_pairs", ["0", "1", "S", "half", "all-1"])
def test_host_twin_counts_what_it_cannot_store(dcl, max_pairs):
    S = split_pairs()
    nbr, counts = pc.synthetic_nbr(S)
    total = sum(counts)
    max_pairs = {"0": 0, "1": 1, "S": S, "half": total // 2, "all-1": total - 1}[max_pairs]
    want = pc.pairs_ref(nbr, pc.N_OUT, pc.N_IN, max_pairs, S)
    got = dcl.ops.conv_pairs_host(nbr, pc.N_OUT, pc.N_IN, max_pairs=max_pairs)
    assert pc.same_list(got, want) == ""
    head = got["head"]
    assert head[pc.HEAD_OVERFLOW] == total - max_pairs and head[:27].tolist() == counts
    assert head[pc.HEAD_NSPLIT] <= max_pairs // S + 27
    tab = got["split_tab"][:head[pc.HEAD_NSPLIT]]
    assert int(tab[:, 2].sum()) == max_pairs and (max_pairs == 0 or int((tab[:, 1] + tab[:, 2]).max()) == max_pairs)
    assert (got["pair_in"][max_pairs:] == -1).all() and (got["pair_out"][max_pairs:] == -1).all()


def test_network_validates_train_conv_wgrad(dcl):
    cfg = dcl.synth.default_cfg(256, 256)
    with pytest.raises(ValueError):
        dcl.DCL_Net.Network(cfg, mode="train", train_conv_wgrad="nope")
    convs = lambda net: [m for m in net.modules() if isinstance(m, dcl.spconv.SparseConvolution)]      # noqa: E731
    net = dcl.DCL_Net.Network(cfg, mode="train")
    assert net.train_conv_wgrad == "rows" and len(convs(net)) == 16 and {m.wgrad for m in convs(net)} == {"rows"}
    net = dcl.DCL_Net.Network(cfg, mode="train", train_conv_wgrad="pairs")
    assert net.train_conv_wgrad == "pairs" and {m.wgrad for m in convs(net)} == {"pairs"}
    assert dcl.spconv.SubMConv3d(4, 4, 3).wgrad == "rows"
    with pytest.raises(ValueError):
        dcl.ops.check_conv_wgrad("columns")
