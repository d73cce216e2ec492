"""The Linear + ReLU training entry points (dcl_linear_wgrad_splits, dcl_linear_wgrad, dcl_relu_bwd; csrc/linear_bwd.hip) are
declared with the documented argument lists, exported by both libraries, and answer the split query and bad arguments
without a GPU; the Refiner's train_mlp switch validates its value."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WANT = {
    "dcl_linear_wgrad_splits": ["int M", "int32_t *splits_host"],
    "dcl_linear_wgrad": ["const float *a", "int64_t lda", "const float *b", "int64_t ldb", "int M", "int P", "int Q",
                         "float *partial", "float *dW", "int64_t lddw", "dclStream_t stream"],
    "dcl_relu_bwd": ["const float *h", "int64_t ldh", "const float *g", "int64_t ldg", "const float *roww",
                     "const float *gpool", "int64_t ldgp", "int rows_per_crop", "int M", "int P", "float *dz", "int64_t lddz",
                     "float *partial", "float *db", "dclStream_t stream"],
}


def _header():
    return open(os.path.join(ROOT, "include", "dclnet_hip.h")).read()


def wgrad_rows():
    m = re.search(r"^#define DCL_WGRAD_ROWS (\d+)\s*$", _header(), flags=re.M)
    assert m, "include/dclnet_hip.h must define DCL_WGRAD_ROWS"
    return int(m.group(1))


def declarations():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    out = {}
    for m in re.finditer(r"\bint\s+(dcl_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        out[m.group(1)] = [re.sub(r"\s+", " ", a).strip() for a in m.group(2).split(",")]
    return out


def test_header_declares_the_entries_and_the_split_constant(dcl):
    decl = declarations()
    for name, args in WANT.items():
        assert name in decl, name
        assert decl[name] == args, (name, decl[name])
    assert wgrad_rows() in (512, 1024)
    assert dcl.ops.WGRAD_ROWS == wgrad_rows()


def _libs(dcl):
    assert os.path.exists(dcl._native.DIAG_SO_PATH), "diagnostic library missing: build() makes it"
    return [("product", dcl._native.lib()), ("diag", C.CDLL(dcl._native.DIAG_SO_PATH))]


def test_both_libraries_export_them(dcl):
    for tag, lib in _libs(dcl):
        for name in WANT:
            assert hasattr(lib, name), (tag, name)
    for op in ("linear_wgrad", "relu_bwd", "linear_wgrad_splits"):
        assert callable(getattr(dcl.ops, op)), op
    assert hasattr(dcl.autograd.RefinerShareFn, "apply")


def test_splits_are_a_function_of_the_rows_alone(dcl):
    R = wgrad_rows()
    for tag, lib in _libs(dcl):
        for M in (0, 1, 2, R - 1, R, R + 1, 2 * R - 1, 2 * R, 2 * R + 1, 20480, 32768):
            s = C.c_int32(-7)
            assert lib.dcl_linear_wgrad_splits(M, C.byref(s)) == 0, (tag, M)
            assert s.value == max(1, -(-M // R)), (tag, M, s.value)
    assert dcl.ops.linear_wgrad_splits(20480) == 20480 // R


_HOST = (C.c_float * 64)()              # host memory stands in for device buffers: a refused call never dereferences them
_P = C.cast(_HOST, C.c_void_p)
_ODD = C.c_void_p(C.addressof(_HOST) + 2)


def _wgrad(L, a=_P, lda=8, b=_P, ldb=8, M=4, P=8, Q=8, partial=_P, dW=_P, lddw=8):
    return L.dcl_linear_wgrad(a, C.c_int64(lda), b, C.c_int64(ldb), M, P, Q, partial, dW, C.c_int64(lddw), None)


def _relu(L, h=_P, ldh=8, g=_P, ldg=8, roww=None, gpool=None, ldgp=0, rpc=0, M=4, P=8, dz=_P, lddz=8, partial=_P, db=_P):
    return L.dcl_relu_bwd(h, C.c_int64(ldh), g, C.c_int64(ldg), roww, gpool, C.c_int64(ldgp), rpc, M, P, dz, C.c_int64(lddz),
                          partial, db, None)


@pytest.mark.parametrize("call", [
    lambda L: L.dcl_linear_wgrad_splits(-1, C.byref(C.c_int32(0))),
    lambda L: L.dcl_linear_wgrad_splits(5, None),
    lambda L: _wgrad(L, a=None),
    lambda L: _wgrad(L, b=None),
    lambda L: _wgrad(L, partial=None),
    lambda L: _wgrad(L, dW=None),
    lambda L: _wgrad(L, a=_ODD),                      # not 4-byte aligned
    lambda L: _wgrad(L, M=-1),
    lambda L: _wgrad(L, P=0),
    lambda L: _wgrad(L, Q=-3),
    lambda L: _wgrad(L, lda=7),
    lambda L: _wgrad(L, ldb=7),
    lambda L: _wgrad(L, lddw=7),
    lambda L: _wgrad(L, M=0, dW=None),                # the zero-row call still needs somewhere to write
    lambda L: _relu(L, h=None),
    lambda L: _relu(L, dz=None),
    lambda L: _relu(L, db=None),
    lambda L: _relu(L, partial=None),
    lambda L: _relu(L, M=-1),
    lambda L: _relu(L, P=0),
    lambda L: _relu(L, ldh=7),
    lambda L: _relu(L, ldg=7),
    lambda L: _relu(L, lddz=7),
    lambda L: _relu(L, g=None),                                             # pooled form without its operands
    lambda L: _relu(L, g=None, roww=_P, gpool=None, ldgp=8, rpc=2),
    lambda L: _relu(L, g=None, roww=_P, gpool=_P, ldgp=7, rpc=2),
    lambda L: _relu(L, g=None, roww=_P, gpool=_P, ldgp=8, rpc=0),
])
def test_bad_arguments_return_einval_without_a_gpu(dcl, call):
    for tag, lib in _libs(dcl):
        lib.dcl_last_error.restype = C.c_char_p
        assert call(lib) == -1, tag
        assert b"invalid argument" in lib.dcl_last_error(), tag


def test_refiner_validates_train_mlp(dcl):
    with pytest.raises(ValueError):
        dcl.refiner.Refiner(train_mlp="nope")
    assert dcl.refiner.Refiner().train_mlp == "modules"
    r = dcl.refiner.Refiner(train_rotation="device", train_mlp="kernels")
    assert (r.train_mlp, r.train_rotation) == ("kernels", "device")
