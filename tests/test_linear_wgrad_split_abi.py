"""dcl_linear_wgrad_split (csrc/linear_wgrad_split.hip) is declared with dcl_linear_wgrad's argument list, listed among the
version's later additions, exported by both libraries and refuses bad arguments without a GPU; the switches that lead to it
(ops.check_linear_wgrad, Network / Refiner train_wgrad) validate their values and their configurations, and TRAIN_KERNELS does
not name it."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "dcl_linear_wgrad_split"


def _header():
    return open(os.path.join(ROOT, "include", "dclnet_hip.h")).read()


def _declarations():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    return {m.group(1): [re.sub(r"\s+", " ", a).strip() for a in m.group(2).split(",")]
            for m in re.finditer(r"\bint\s+(dcl_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)}


def _libs(dcl):
    assert os.path.exists(dcl._native.DIAG_SO_PATH), "diagnostic library missing: build() makes it"
    return [("product", dcl._native.lib()), ("diag", C.CDLL(dcl._native.DIAG_SO_PATH))]


def test_header_declares_it_like_the_fp32_entry_and_lists_it():
    decl = _declarations()
    assert NAME in decl
    assert decl[NAME] == decl["dcl_linear_wgrad"]
    head = _header()
    listed = head[head.index("later additions"):head.index("#define DCL_ABI_VERSION")]
    assert NAME in listed
    assert re.search(r"^#define DCL_ABI_VERSION 2\s*$", head, flags=re.M)


def test_both_libraries_export_it_and_ops_has_the_op(dcl):
    for tag, lib in _libs(dcl):
        assert hasattr(lib, NAME), tag
    for op in ("linear_wgrad_split", "check_linear_wgrad", "linear_wgrad_form", "linear_wgrad_split_units"):
        assert callable(getattr(dcl.ops, op)), op
    # the a-priori bound of the header, in units: 6 roundings per row of a split, one per split, 32 for the rest
    R = dcl.ops.WGRAD_ROWS
    assert dcl.ops.linear_wgrad_split_units(0) == 6 * R + 1 + 32
    assert dcl.ops.linear_wgrad_split_units(3 * R + 1) == 6 * R + 4 + 32


_HOST = (C.c_float * 64)()              # host memory stands in for device buffers: a refused call never dereferences them
_P = C.cast(_HOST, C.c_void_p)
_ODD = C.c_void_p(C.addressof(_HOST) + 2)


def _wgrad(L, a=_P, lda=8, b=_P, ldb=8, M=4, P=8, Q=8, partial=_P, dW=_P, lddw=8):
    return L.dcl_linear_wgrad_split(a, C.c_int64(lda), b, C.c_int64(ldb), M, P, Q, partial, dW, C.c_int64(lddw), None)


@pytest.mark.parametrize("call", [
    lambda L: _wgrad(L, a=None),
    lambda L: _wgrad(L, b=None),
    lambda L: _wgrad(L, partial=None),
    lambda L: _wgrad(L, dW=None),
    lambda L: _wgrad(L, a=_ODD),                      # not 4-byte aligned
    lambda L: _wgrad(L, b=_ODD),
    lambda L: _wgrad(L, dW=_ODD),
    lambda L: _wgrad(L, partial=_ODD),
    lambda L: _wgrad(L, M=-1),
    lambda L: _wgrad(L, P=0),
    lambda L: _wgrad(L, Q=0),
    lambda L: _wgrad(L, Q=-3),
    lambda L: _wgrad(L, lda=7),
    lambda L: _wgrad(L, ldb=7),
    lambda L: _wgrad(L, lddw=7),
    lambda L: _wgrad(L, M=0, dW=None),                # the zero-row call still needs somewhere to write
])
def test_bad_arguments_return_einval_without_a_gpu(dcl, call):
    for tag, lib in _libs(dcl):
        lib.dcl_last_error.restype = C.c_char_p
        assert call(lib) == -1, tag
        assert b"invalid argument" in lib.dcl_last_error(), tag


def test_check_linear_wgrad_accepts_and_rejects(dcl):
    ops = dcl.ops
    assert ops.WGRAD_FORMS == ("fp32", "split")
    assert ops.check_linear_wgrad("fp32") == "fp32" and ops.check_linear_wgrad("split") == "split"
    for bad in ("bf16", "", None, 1, "Split"):
        with pytest.raises(ValueError):
            ops.check_linear_wgrad(bad)


def test_the_shape_table_decides_by_shape_alone(dcl, monkeypatch):
    ops = dcl.ops
    assert isinstance(ops.WGRAD_SPLIT_SHAPES, dict)
    for (P, Q), min_rows in ops.WGRAD_SPLIT_SHAPES.items():
        assert P >= 1 and Q >= 1 and min_rows >= 0
    monkeypatch.setattr(ops, "WGRAD_SPLIT_SHAPES", {(128, 256): 4096})
    assert ops.linear_wgrad_form(4096, 128, 256, "split") == "split"
    assert ops.linear_wgrad_form(4095, 128, 256, "split") == "fp32"
    assert ops.linear_wgrad_form(4096, 256, 128, "split") == "fp32"
    assert ops.linear_wgrad_form(4096, 128, 256, "fp32") == "fp32"
    with pytest.raises(ValueError):
        ops.linear_wgrad_form(4096, 128, 256, "nope")


def test_network_reads_the_switch_only_with_the_point_major_dense_half(dcl):
    net_mod = dcl.DCL_Net
    cfg = dcl.synth.default_cfg(256, 256)
    assert "train_wgrad" not in net_mod.TRAIN_KERNELS
    with pytest.raises(ValueError):
        net_mod.Network(cfg, mode="train", train_wgrad="split")                       # train_dense="modules"
    with pytest.raises(ValueError):
        net_mod.Network(cfg, mode="train", train_wgrad="nope", **net_mod.TRAIN_KERNELS)
    with pytest.raises(TypeError):
        net_mod.Network(cfg, mode="train", train_wgrads="split", **net_mod.TRAIN_KERNELS)     # no other extra keyword
    base = net_mod.Network(cfg, mode="train", **net_mod.TRAIN_KERNELS)
    assert base.train_wgrad == "fp32"
    net = net_mod.Network(cfg, mode="train", train_wgrad="split", **net_mod.TRAIN_KERNELS)
    assert net.train_wgrad == "split"
    assert list(net.state_dict().keys()) == list(base.state_dict().keys())


def test_refiner_reads_the_switch_only_with_its_kernels(dcl):
    Refiner = dcl.refiner.Refiner
    with pytest.raises(ValueError):
        Refiner(train_wgrad="split")                                                  # train_mlp="modules"
    with pytest.raises(ValueError):
        Refiner(train_mlp="kernels", train_wgrad="nope")
    assert Refiner().train_wgrad == "fp32"
    r = Refiner(train_mlp="kernels", train_wgrad="split")
    assert r.train_wgrad == "split"
    assert list(r.state_dict().keys()) == list(Refiner().state_dict().keys())
