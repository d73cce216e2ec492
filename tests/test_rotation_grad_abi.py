"""The rotation head's gradient (dcl_ortho9d_bwd, dcl_ortho9d_bwd_host) without a GPU: the entry points are declared with the
documented argument lists, exported by both libraries and answer bad arguments and an empty batch; the models take the
`train_rotation=` switch; and the host twin -- the kernel's own routine compiled for the host -- agrees with float64
references on every input class, stays finite on degenerate axes and keeps a non-finite crop to itself."""
import ctypes as C
import os
import re

import pytest
import torch

import rotation_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WANT = {
    "dcl_ortho9d_bwd": ["int b", "const float *o9", "const float *grad_R", "float *grad_o9", "dclStream_t stream"],
    "dcl_ortho9d_bwd_host": ["int b", "const float *o9", "const float *grad_R", "float *grad_o9"],
}


def declarations():
    text = open(os.path.join(ROOT, "include", "dclnet_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for m in re.finditer(r"\bint\s+(dcl_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        out[m.group(1)] = [re.sub(r"\s+", " ", a).strip() for a in m.group(2).split(",")]
    return out


def test_header_declares_the_entry_points():
    decl = declarations()
    for name, args in WANT.items():
        assert name in decl, name
        assert decl[name] == args, (name, decl[name])
    text = open(os.path.join(ROOT, "include", "dclnet_hip.h")).read()
    assert re.search(r"#define DCL_ABI_VERSION 2\b", text)


def _libs(dcl):
    assert os.path.exists(dcl._native.DIAG_SO_PATH), "diagnostic library missing: build() makes it"
    return [("product", dcl._native.lib()), ("diag", C.CDLL(dcl._native.DIAG_SO_PATH))]


def test_both_libraries_export_them_and_the_python_layers_exist(dcl):
    for tag, lib in _libs(dcl):
        for name in WANT:
            assert hasattr(lib, name), (tag, name)
    assert callable(dcl.ops.ortho9d_backward) and callable(dcl.ops.ortho9d_backward_host)
    assert hasattr(dcl.autograd.Ortho9dFn, "apply")


_BUF = (C.c_char * 64)()                 # host bytes standing in for device buffers: a rejected call never dereferences them
_P = C.cast(_BUF, C.c_void_p)


def _dev(L, b=2, o9=_P, grad_R=_P, grad_o9=_P):
    return L.dcl_ortho9d_bwd(b, o9, grad_R, grad_o9, None)


def _host(L, b=2, o9=_P, grad_R=_P, grad_o9=_P):
    return L.dcl_ortho9d_bwd_host(b, o9, grad_R, grad_o9)


@pytest.mark.parametrize("call", [
    lambda L: _dev(L, b=-1),
    lambda L: _dev(L, o9=None),
    lambda L: _dev(L, grad_R=None),
    lambda L: _dev(L, grad_o9=None),
    lambda L: _host(L, b=-1),
    lambda L: _host(L, o9=None),
    lambda L: _host(L, grad_R=None),
    lambda L: _host(L, grad_o9=None),
])
def test_bad_arguments_return_einval_without_a_gpu(dcl, call):
    for tag, lib in _libs(dcl):
        lib.dcl_last_error.restype = C.c_char_p
        assert call(lib) == -1, tag
        assert b"invalid argument" in lib.dcl_last_error(), tag


def test_an_empty_batch_is_not_an_error(dcl):
    for tag, lib in _libs(dcl):
        assert _dev(lib, b=0) == 0, tag
        assert _dev(lib, b=0, o9=None, grad_R=None, grad_o9=None) == 0, tag
        assert _host(lib, b=0) == 0, tag
    assert dcl.ops.ortho9d_backward_host(torch.zeros(0, 9), torch.zeros(0, 3, 3)).shape == (0, 9)


def test_models_validate_train_rotation_and_default_to_host(dcl):
    cfg = dcl.synth.default_cfg(256, 256)
    for make in (lambda **k: dcl.DCL_Net.Network(cfg, mode="train", **k), lambda **k: dcl.refiner.Refiner(cfg, **k)):
        with pytest.raises(ValueError, match="train_rotation"):
            make(train_rotation="x")
        with pytest.raises(ValueError, match="train_rotation"):
            make(train_rotation=None)
        assert make().train_rotation == "host"
        assert make(train_rotation="device").train_rotation == "device"


def test_ortho9dfn_refuses_cpu_tensors_with_a_clear_error(dcl):
    o9 = torch.randn(3, 9, requires_grad=True)
    with pytest.raises(RuntimeError, match="GPU"):
        dcl.autograd.Ortho9dFn.apply(o9)
    with pytest.raises(RuntimeError, match="GPU"):
        dcl.DCL_Net.ortho9d2matrix(o9[:, :3], o9[:, 3:6], o9[:, 6:], "device")
    with pytest.raises(RuntimeError, match="GPU"):
        dcl.ops.ortho9d_backward(o9.detach(), torch.zeros(3, 3, 3))


@pytest.mark.parametrize("cls", RC.ALL_CLASSES)
def test_host_twin_matches_the_float64_reference(dcl, cls):
    """Per crop, relative to that crop's max |reference|, all 64 crops: <= 1e-6 on the noisy-orthonormal classes, <= 2e-5 on
    the other autograd classes (float64 autograd of the reference composition on the same fp32 o9), <= 1e-5 on exactly
    orthonormal axes (float64 central differences, step 1e-6: autograd is NaN there)."""
    o9, G = RC.inputs(cls)
    got = dcl.ops.ortho9d_backward_host(o9, G)
    ratio = RC.worst_ratio(got, cls)
    print("rotation grad, host twin, %-18s worst error / max|grad| = %.3g (bound %.0e)" % (cls, ratio, RC.bound(cls)))
    assert torch.isfinite(got).all()
    assert ratio <= RC.bound(cls), (cls, ratio)


def test_degenerate_axes_give_finite_gradients(dcl):
    g = torch.Generator().manual_seed(3)
    v = torch.randn(8, 3, generator=g)
    w = torch.randn(8, 3, generator=g)
    z = torch.zeros(8, 3)
    cases = {
        "three parallel axes": torch.cat([v, 2 * v, -0.5 * v], 1),
        "three equal axes along x": torch.tensor([[1.0, 0, 0] * 3] * 8),
        "first axis zero": torch.cat([z, v, w], 1),
        "second axis zero": torch.cat([v, z, w], 1),
        "third axis zero": torch.cat([v, w, z], 1),
        "all zeros": torch.zeros(8, 9),
    }
    G = torch.randn(8, 3, 3, generator=g)
    for name, o9 in cases.items():
        got = dcl.ops.ortho9d_backward_host(o9.contiguous(), G)
        assert torch.isfinite(got).all(), (name, got)
    assert torch.equal(dcl.ops.ortho9d_backward_host(torch.zeros(8, 9), G), torch.zeros(8, 9))


@pytest.mark.parametrize("where,value", [("o9", float("nan")), ("o9", float("inf")), ("o9", float("-inf")),
                                         ("G", float("nan")), ("G", float("inf"))])
def test_a_non_finite_crop_keeps_to_itself(dcl, where, value):
    o9, G = [t.clone() for t in RC.inputs("gaussian", 7)]
    bad = 3
    (o9 if where == "o9" else G.view(-1, 9))[bad, 4] = value
    got = dcl.ops.ortho9d_backward_host(o9, G)
    assert torch.isnan(got[bad]).all()
    keep = [i for i in range(7) if i != bad]
    without = dcl.ops.ortho9d_backward_host(o9[keep].contiguous(), G[keep].contiguous())
    assert torch.isfinite(without).all() and torch.equal(got[keep], without)
