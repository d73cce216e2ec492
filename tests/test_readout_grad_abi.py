"""The ordered read-out gradient (dcl_three_interpolate_grad_sp_ordered and its size query, csrc/readout_grad.hip) is declared
with the agreed argument lists, exported by both libraries beside the atomic form it replaces in autograd, keeps its
workspace linear in the problem, and answers size queries, bad arguments and empty problems without a GPU."""
import ctypes as C
import os
import re

import pytest

from test_pointnet_grad_abi import _libs, declarations

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WANT = {
    "dcl_three_interpolate_grad_sp_ws_bytes": ["int c", "int n", "int m", "int64_t *bytes_host"],
    "dcl_three_interpolate_grad_sp_ordered": ["int c", "int n", "int m", "const float *grad_out", "int64_t grad_stride",
                                              "const int32_t *idx", "const float *weight", "float *grad_points", "void *ws",
                                              "int64_t ws_bytes", "dclStream_t stream"],
}
ATOMIC = "dcl_three_interpolate_grad_sp"


def test_header_declares_both_functions():
    decl = declarations()
    for name, args in WANT.items():
        assert name in decl, name
        assert decl[name] == args, (name, decl[name])
    assert ATOMIC in decl
    text = open(os.path.join(ROOT, "include", "dclnet_hip.h")).read()
    assert re.search(r"#define DCL_ABI_VERSION 2\b", text)


def test_both_libraries_export_the_ordered_and_the_atomic_form(dcl):
    assert os.path.exists(dcl._native.DIAG_SO_PATH), "diagnostic library missing: build() makes it"
    for tag, lib in _libs(dcl):
        for name in list(WANT) + [ATOMIC]:
            assert hasattr(lib, name), (tag, name)
    assert callable(dcl.ops.three_interpolate_grad_sp) and callable(dcl.ops.three_interpolate_grad_sp_atomic)


@pytest.mark.parametrize("c,n,m", [(256, 32 * 12288, 400000), (32, 257, 64)])
def test_workspace_is_linear_in_the_problem_and_needs_no_gpu(dcl, c, n, m):
    for tag, lib in _libs(dcl):
        nb = C.c_int64(-7)
        assert lib.dcl_three_interpolate_grad_sp_ws_bytes(c, n, m, C.byref(nb)) == 0, tag
        # a list entry and its weight per position at least; no table of positions x rows or tiles x rows
        assert 8 * 3 * n <= nb.value <= 16 * 3 * n + 16 * (m + 1) + 4096, (tag, nb.value)


def _ordered(L, c, n, m, stride, bufs, ws, ws_bytes):
    g, i, w, gp = bufs
    return L.dcl_three_interpolate_grad_sp_ordered(c, n, m, g, C.c_int64(stride), i, w, gp, ws, C.c_int64(ws_bytes), None)


FAKE = C.c_void_p(4096)          # a non-null address that a call refusing its arguments never touches
ALL = (FAKE, FAKE, FAKE, FAKE)
BIG = 1 << 40


@pytest.mark.parametrize("call", [
    lambda L, nb: L.dcl_three_interpolate_grad_sp_ws_bytes(-1, 10, 10, C.byref(nb)),
    lambda L, nb: L.dcl_three_interpolate_grad_sp_ws_bytes(4, -10, 10, C.byref(nb)),
    lambda L, nb: L.dcl_three_interpolate_grad_sp_ws_bytes(4, 10, -10, C.byref(nb)),
    lambda L, nb: L.dcl_three_interpolate_grad_sp_ws_bytes(4, ((1 << 31) - 8192 + 2) // 3, 10, C.byref(nb)),   # 3n >= 2^31 - 8192
    lambda L, nb: L.dcl_three_interpolate_grad_sp_ws_bytes(4, 10, 1 << 30, C.byref(nb)),
    lambda L, nb: L.dcl_three_interpolate_grad_sp_ws_bytes(65536, 10, 10, C.byref(nb)),
    lambda L, nb: L.dcl_three_interpolate_grad_sp_ws_bytes(4, 10, 10, None),
    lambda L, nb: _ordered(L, -1, 10, 10, 4, ALL, FAKE, BIG),
    lambda L, nb: _ordered(L, 4, -10, 10, 4, ALL, FAKE, BIG),
    lambda L, nb: _ordered(L, 4, 10, -10, 4, ALL, FAKE, BIG),
    lambda L, nb: _ordered(L, 4, ((1 << 31) - 8192 + 2) // 3, 10, 4, ALL, FAKE, BIG),
    lambda L, nb: _ordered(L, 4, 10, 1 << 30, 4, ALL, FAKE, BIG),
    lambda L, nb: _ordered(L, 65536, 10, 10, 65536, ALL, FAKE, BIG),
    lambda L, nb: _ordered(L, 64, 10, 10, 63, ALL, FAKE, BIG),                                  # grad_stride < c
    lambda L, nb: _ordered(L, 4, 10, 10, 4, (None, FAKE, FAKE, FAKE), FAKE, BIG),               # a null buffer, each in turn
    lambda L, nb: _ordered(L, 4, 10, 10, 4, (FAKE, None, FAKE, FAKE), FAKE, BIG),
    lambda L, nb: _ordered(L, 4, 10, 10, 4, (FAKE, FAKE, None, FAKE), FAKE, BIG),
    lambda L, nb: _ordered(L, 4, 10, 10, 4, (FAKE, FAKE, FAKE, None), FAKE, BIG),
    lambda L, nb: _ordered(L, 4, 10, 10, 4, ALL, None, BIG),
    lambda L, nb: _ordered(L, 4, 0, 10, 4, (FAKE, FAKE, FAKE, None), FAKE, BIG),                # n == 0 still writes grad_points
    lambda L, nb: _ordered(L, 4, 10, 10, 4, ALL, FAKE, 8 * 30),                                 # short workspace
])
def test_bad_arguments_return_einval_without_a_gpu(dcl, call):
    for tag, lib in _libs(dcl):
        lib.dcl_last_error.restype = C.c_char_p
        nb = C.c_int64(0)
        assert call(lib, nb) == -1, tag
        assert b"invalid argument" in lib.dcl_last_error(), tag


def test_short_workspace_is_measured_against_the_size_query(dcl):
    for tag, lib in _libs(dcl):
        lib.dcl_last_error.restype = C.c_char_p
        nb = C.c_int64(0)
        assert lib.dcl_three_interpolate_grad_sp_ws_bytes(32, 257, 64, C.byref(nb)) == 0
        assert _ordered(lib, 32, 257, 64, 32, ALL, FAKE, nb.value - 1) == -1, tag
        assert b"invalid argument" in lib.dcl_last_error(), tag


def test_empty_problems_are_no_ops_without_a_gpu(dcl):
    for tag, lib in _libs(dcl):
        none = (None, None, None, None)
        assert _ordered(lib, 0, 10, 10, 0, none, None, 0) == 0, tag         # no channels
        assert _ordered(lib, 4, 10, 0, 4, none, None, 0) == 0, tag          # no rows to write
        assert _ordered(lib, 0, 0, 0, 0, none, None, 0) == 0, tag
        z = C.c_int64(-7)
        assert lib.dcl_three_interpolate_grad_sp_ws_bytes(0, 0, 0, C.byref(z)) == 0 and z.value >= 0, tag
