"""The attention gradient entry points (dcl_cross_attention_bwd, dcl_cross_attention_bwd_ws_bytes) are declared with the
documented argument lists, exported by both libraries, and answer the size query and bad arguments without a GPU."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WANT = {
    "dcl_cross_attention_bwd_ws_bytes": ["int b", "int nq", "int nk", "int64_t *bytes_host"],
    "dcl_cross_attention_bwd": [
        "int b", "int nq", "int nk", "const float *Q", "int ldq", "const float *K", "int ldk",
        "const float *V1", "int dv1", "int ldv1", "const float *V2", "int dv2", "int ldv2",
        "const float *O1", "int ldo1", "const float *O2", "int ldo2",
        "const float *dO1", "int lddo1", "const float *dO2", "int lddo2",
        "float *dQ", "int lddq", "float *dK", "int lddk", "float *dV1", "int lddv1", "float *dV2", "int lddv2",
        "void *ws", "int64_t ws_bytes", "dclStream_t stream"],
}


def declarations():
    text = open(os.path.join(ROOT, "include", "dclnet_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for m in re.finditer(r"\bint\s+(dcl_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        out[m.group(1)] = [re.sub(r"\s+", " ", a).strip() for a in m.group(2).split(",")]
    return out


def test_header_declares_the_attention_gradient():
    decl = declarations()
    for name, args in WANT.items():
        assert name in decl, name
        assert decl[name] == args, (name, decl[name])
    text = open(os.path.join(ROOT, "include", "dclnet_hip.h")).read()
    assert re.search(r"#define DCL_ABI_VERSION 2\b", text)


def _libs(dcl):
    assert os.path.exists(dcl._native.DIAG_SO_PATH), "diagnostic library missing: build() makes it"
    return [("product", dcl._native.lib()), ("diag", C.CDLL(dcl._native.DIAG_SO_PATH))]


def _ws(lib, b, nq, nk):
    nb = C.c_int64(-7)
    assert lib.dcl_cross_attention_bwd_ws_bytes(b, nq, nk, C.byref(nb)) == 0, (b, nq, nk)
    return nb.value


def test_both_libraries_export_it(dcl):
    for tag, lib in _libs(dcl):
        for name in WANT:
            assert hasattr(lib, name), (tag, name)
    assert callable(dcl.ops.cross_attention_backward)
    assert hasattr(dcl.autograd.CrossAttentionFn, "apply")


def test_size_query_needs_no_gpu_and_does_not_grow_with_the_map(dcl):
    for tag, lib in _libs(dcl):
        assert _ws(lib, 1, 1, 1) > 0, tag
        assert _ws(lib, 32, 1024, 1024) >= 2 * 4 * 32 * 1024, tag             # lse and delta per query row
        n = 4096
        assert _ws(lib, 2, 2 * n, 2 * n) <= 2 * _ws(lib, 2, n, n) + 64 * 1024, tag
        assert _ws(lib, 32, 12288, 2048) < 32 * 12288 * 2048 * 4 // 64, tag
        assert _ws(lib, 32, 12288, 2048) == _ws(lib, 32, 12288, 7), tag        # no dependence on the key count at all


def _bwd(L, b=2, nq=100, nk=50, dv1=256, dv2=64, ws=None, ws_bytes=0):
    z = None
    return L.dcl_cross_attention_bwd(b, nq, nk, z, 64, z, 64, z, dv1, 256, z, dv2, 64, z, 256, z, 64, z, 256, z, 64,
                                     z, 64, z, 64, z, 256, z, 64, ws, C.c_int64(ws_bytes), None)


_HOST_WS = (C.c_char * 4096)()          # a host buffer stands in for a workspace that is too short: never dereferenced


@pytest.mark.parametrize("call", [
    lambda L, nb: L.dcl_cross_attention_bwd_ws_bytes(-1, 10, 10, C.byref(nb)),
    lambda L, nb: L.dcl_cross_attention_bwd_ws_bytes(1, -10, 10, C.byref(nb)),
    lambda L, nb: L.dcl_cross_attention_bwd_ws_bytes(1, 10, -10, C.byref(nb)),
    lambda L, nb: L.dcl_cross_attention_bwd_ws_bytes(70000, 10, 10, C.byref(nb)),
    lambda L, nb: L.dcl_cross_attention_bwd_ws_bytes(1, 10, 10, None),
    lambda L, nb: _bwd(L, b=-1),
    lambda L, nb: _bwd(L, nq=-5),
    lambda L, nb: _bwd(L, nk=-5),
    lambda L, nb: _bwd(L, dv1=128, ws=C.cast(_HOST_WS, C.c_void_p), ws_bytes=1 << 30),
    lambda L, nb: _bwd(L, dv2=32, ws=C.cast(_HOST_WS, C.c_void_p), ws_bytes=1 << 30),
    lambda L, nb: _bwd(L, dv1=64, dv2=256, ws=C.cast(_HOST_WS, C.c_void_p), ws_bytes=1 << 30),
    lambda L, nb: _bwd(L, ws=None, ws_bytes=1 << 30),                                       # NULL workspace
    lambda L, nb: _bwd(L, ws=C.cast(_HOST_WS, C.c_void_p), ws_bytes=16),                    # short workspace
    lambda L, nb: _bwd(L, nq=12288, nk=2048, ws=C.cast(_HOST_WS, C.c_void_p), ws_bytes=4096),
])
def test_bad_arguments_return_einval_without_a_gpu(dcl, call):
    for tag, lib in _libs(dcl):
        lib.dcl_last_error.restype = C.c_char_p
        nb = C.c_int64(0)
        assert call(lib, nb) == -1, tag
        assert b"invalid argument" in lib.dcl_last_error(), tag


def test_network_rejects_unknown_train_attention(dcl):
    cfg = dcl.synth.default_cfg(64, 64)
    with pytest.raises(ValueError):
        dcl.DCL_Net.Network(cfg, mode="train", train_attention="flash")
    assert dcl.DCL_Net.Network(cfg, mode="train").train_attention == "materialised"
    assert dcl.DCL_Net.Network(cfg, mode="train", train_attention="fused").train_attention == "fused"
