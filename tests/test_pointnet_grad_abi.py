"""The pointnet_lib gradient entry points (group_points_grad, gather_points_grad, three_interpolate_grad of
libs/pointnet_lib/src/pointnet2_api.cpp:14,17,24) are declared in the reference's argument order, exported by both
libraries, and answer size queries and bad arguments without a GPU."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# reference argument order, then (ws, ws_bytes, stream); size queries: the sizes, then the result pointer
WANT = {
    "dcl_group_points_grad": ["int b", "int c", "int n", "int npoints", "int nsample", "const float *grad_out",
                              "const int32_t *idx", "float *grad_points", "void *ws", "int64_t ws_bytes",
                              "dclStream_t stream"],
    "dcl_gather_points_grad": ["int b", "int c", "int n", "int npoints", "const float *grad_out", "const int32_t *idx",
                               "float *grad_points", "void *ws", "int64_t ws_bytes", "dclStream_t stream"],
    "dcl_three_interpolate_grad": ["int b", "int c", "int n", "int m", "const float *grad_out", "const int32_t *idx",
                                   "const float *weight", "float *grad_points", "void *ws", "int64_t ws_bytes",
                                   "dclStream_t stream"],
    "dcl_group_points_grad_ws_bytes": ["int b", "int c", "int n", "int npoints", "int nsample", "int64_t *bytes_host"],
    "dcl_gather_points_grad_ws_bytes": ["int b", "int c", "int n", "int npoints", "int64_t *bytes_host"],
    "dcl_three_interpolate_grad_ws_bytes": ["int b", "int c", "int n", "int m", "int64_t *bytes_host"],
}


def declarations():
    text = open(os.path.join(ROOT, "include", "dclnet_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for m in re.finditer(r"\bint\s+(dcl_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        out[m.group(1)] = [re.sub(r"\s+", " ", a).strip() for a in m.group(2).split(",")]
    return out


def test_header_declares_the_three_grads_in_reference_order():
    decl = declarations()
    for name, args in WANT.items():
        assert name in decl, name
        assert decl[name] == args, (name, decl[name])
    text = open(os.path.join(ROOT, "include", "dclnet_hip.h")).read()
    assert re.search(r"#define DCL_ABI_VERSION 2\b", text)


def _libs(dcl):
    libs = [("product", dcl._native.lib())]
    if os.path.exists(dcl._native.DIAG_SO_PATH):
        libs.append(("diag", C.CDLL(dcl._native.DIAG_SO_PATH)))
    return libs


def test_both_libraries_export_the_grads(dcl):
    assert os.path.exists(dcl._native.DIAG_SO_PATH), "diagnostic library missing: build() makes it"
    for tag, lib in _libs(dcl):
        for name in WANT:
            assert hasattr(lib, name), (tag, name)


def test_size_queries_need_no_gpu(dcl):
    for tag, lib in _libs(dcl):
        nb = C.c_int64(-7)
        assert lib.dcl_group_points_grad_ws_bytes(32, 64, 12288, 2048, 64, C.byref(nb)) == 0, tag
        # at least the inverse index itself: start offsets and one list entry per position
        assert nb.value >= 4 * (32 * 12289 + 32 * 2048 * 64), (tag, nb.value)
        ng = C.c_int64(-7)
        assert lib.dcl_gather_points_grad_ws_bytes(3, 20, 700, 123, C.byref(ng)) == 0 and ng.value >= 4 * 3 * 123, tag
        ni = C.c_int64(-7)
        assert lib.dcl_three_interpolate_grad_ws_bytes(32, 64, 12288, 2048, C.byref(ni)) == 0, tag
        assert ni.value >= 8 * 32 * 12288 * 3, (tag, ni.value)              # list entries and their weights
        z = C.c_int64(-7)
        assert lib.dcl_group_points_grad_ws_bytes(0, 0, 0, 0, 0, C.byref(z)) == 0 and z.value >= 0, tag


@pytest.mark.parametrize("call", [
    lambda L, nb: L.dcl_group_points_grad_ws_bytes(-1, 4, 100, 10, 4, C.byref(nb)),
    lambda L, nb: L.dcl_group_points_grad_ws_bytes(1, 4, 100, -10, 4, C.byref(nb)),
    lambda L, nb: L.dcl_group_points_grad_ws_bytes(1, 4, 100, 1 << 20, 1 << 12, C.byref(nb)),     # 2^32 positions
    lambda L, nb: L.dcl_group_points_grad_ws_bytes(1, 4, 100, 10, 4, None),
    lambda L, nb: L.dcl_gather_points_grad_ws_bytes(1, -4, 100, 10, C.byref(nb)),
    lambda L, nb: L.dcl_three_interpolate_grad_ws_bytes(1, 4, -5, 100, C.byref(nb)),
    lambda L, nb: L.dcl_three_interpolate_grad_ws_bytes(70000, 4, 5, 100, C.byref(nb)),
    # no buffers / no workspace for real work, before any device call
    lambda L, nb: L.dcl_group_points_grad(1, 4, 100, 10, 4, None, None, None, None, C.c_int64(0), None),
    lambda L, nb: L.dcl_gather_points_grad(2, 3, 50, 7, None, None, None, None, C.c_int64(0), None),
    lambda L, nb: L.dcl_three_interpolate_grad(2, 3, 50, 7, None, None, None, None, None, C.c_int64(0), None),
    lambda L, nb: L.dcl_group_points_grad(-1, 4, 100, 10, 4, None, None, None, None, C.c_int64(0), None),
    lambda L, nb: L.dcl_three_interpolate_grad(1, 4, 10, -1, None, None, None, None, None, C.c_int64(0), None),
])
def test_bad_arguments_return_einval_without_a_gpu(dcl, call):
    for tag, lib in _libs(dcl):
        lib.dcl_last_error.restype = C.c_char_p
        nb = C.c_int64(0)
        assert call(lib, nb) == -1, tag
        assert b"invalid argument" in lib.dcl_last_error(), tag


def test_empty_problems_are_no_ops_without_a_gpu(dcl):
    lib = dcl._native.lib()
    assert lib.dcl_group_points_grad(0, 4, 100, 10, 4, None, None, None, None, C.c_int64(0), None) == 0
    assert lib.dcl_gather_points_grad(2, 3, 50, 0, None, None, None, None, C.c_int64(0), None) == 0
    assert lib.dcl_three_interpolate_grad(2, 0, 50, 7, None, None, None, None, None, C.c_int64(0), None) == 0


def test_mirror_exports_the_reference_function_classes(dcl):
    import importlib
    pu = importlib.import_module("dcl-net_amd.libs.pointnet_lib.pointnet2_utils")
    for cls in ("GatherOperation", "GroupingOperation", "ThreeInterpolate"):
        assert hasattr(getattr(pu, cls), "apply"), cls
    assert pu.GroupingOperation is dcl.autograd.GroupPointsFn
    assert pu.GatherOperation is dcl.autograd.GatherPointsFn
    assert pu.ThreeInterpolate is dcl.autograd.ThreeInterpolateBatchedFn
    for f in ("group_points_grad", "gather_points_grad", "three_interpolate_grad"):
        assert callable(getattr(dcl.ops, f)), f
