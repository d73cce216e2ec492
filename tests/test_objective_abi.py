"""The training-objective entry points (dcl_rigid_points*, dcl_pose_objective_*, and their host twins) are declared with the
documented argument lists, exported by both libraries and answer bad arguments and an empty batch without a GPU; the loss
modules take the `objective=` switch and default to the module composition."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_RIGID = ["int b", "int n", "const float *pts", "const float *R", "const float *t", "int inverse"]
_INPUTS = ["int b", "int n", "const float *posed", "const float *posed_gt", "const float *Yc", "const float *cano_pred",
           "const float *cano_gt", "const float *Xo", "const float *conf", "const float *sym"]
_HALVES = ["const float *cd_pose_pt", "const float *cd_pose_tp", "const float *cd_Xo_pt", "const float *cd_Xo_tp",
           "const float *cd_Yc_pt", "const float *cd_Yc_tp"]
_FWD_OUT = ["float *L", "float *crop_sums", "float *packed"]
_BWD = ["const float *L", "const float *g_packed", "float *g_posed", "float *g_Xo", "float *g_Yc", "float *g_conf",
        "float *g_cd_pose_pt", "float *g_cd_pose_tp", "float *g_cd_Xo_pt", "float *g_cd_Xo_tp", "float *g_cd_Yc_pt",
        "float *g_cd_Yc_tp"]
_S = ["dclStream_t stream"]
_RIGID_BWD = ["const float *g_out", "float *g_R", "float *g_t", "float *g_pts"]

WANT = {
    "dcl_rigid_points": _RIGID + ["float *out"] + _S,
    "dcl_rigid_points_host": _RIGID + ["float *out"],
    "dcl_rigid_points_bwd": _RIGID + _RIGID_BWD + _S,
    "dcl_rigid_points_bwd_host": _RIGID + _RIGID_BWD,
    "dcl_pose_objective_fwd": _INPUTS + _HALVES + _FWD_OUT + _S,
    "dcl_pose_objective_fwd_host": _INPUTS + _HALVES + _FWD_OUT,
    "dcl_pose_objective_bwd": _INPUTS + _BWD + _S,
    "dcl_pose_objective_bwd_host": _INPUTS + _BWD,
}


def declarations():
    text = open(os.path.join(ROOT, "include", "dclnet_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for m in re.finditer(r"\bint\s+(dcl_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        out[m.group(1)] = [re.sub(r"\s+", " ", a).strip() for a in m.group(2).split(",")]
    return out


def test_header_declares_the_objective_entry_points_and_keeps_the_abi_version():
    decl = declarations()
    for name, args in WANT.items():
        assert name in decl, name
        assert decl[name] == args, (name, decl[name])
    text = open(os.path.join(ROOT, "include", "dclnet_hip.h")).read()
    assert re.search(r"#define DCL_ABI_VERSION 2\b", text)
    section = text[text.index("training objective ---"):text.index("optimizer step ---")]
    assert "dcl_pose_objective_fwd" in section and "PINNED ORDER" in section and "strides 128" in section


def _libs(dcl):
    assert os.path.exists(dcl._native.DIAG_SO_PATH), "diagnostic library missing: build() makes it"
    return [("product", dcl._native.lib()), ("diag", C.CDLL(dcl._native.DIAG_SO_PATH))]


def test_both_libraries_export_them_and_the_python_layers_exist(dcl):
    for tag, lib in _libs(dcl):
        for name in WANT:
            assert hasattr(lib, name), (tag, name)
        assert int(lib.dcl_abi_version()) == 2 == dcl._native.ABI_VERSION, tag
    for fn in ("rigid_points", "rigid_points_backward", "pose_objective", "pose_objective_backward"):
        assert callable(getattr(dcl.ops, fn)) and callable(getattr(dcl.ops, fn + "_host")), fn
    assert hasattr(dcl.autograd.RigidPointsFn, "apply") and hasattr(dcl.autograd.PoseObjectiveFn, "apply")


_BUF = (C.c_char * 64)()                 # host bytes standing in for buffers: a rejected call never dereferences them
_P = C.cast(_BUF, C.c_void_p)
_FULL_IN = ("Yc", "cano_pred", "cano_gt", "Xo", "conf")
_FULL_CD = ("cd_Xo_pt", "cd_Xo_tp", "cd_Yc_pt", "cd_Yc_tp")
_FULL_G = ("g_Xo", "g_Yc", "g_conf", "g_cd_Xo_pt", "g_cd_Xo_tp", "g_cd_Yc_pt", "g_cd_Yc_tp")


def _call(lib, name, host, **over):
    """one call with every pointer set (or, with pose_only, the optional set NULL) and `over` applied on top"""
    pose_only = over.pop("pose_only", False)
    vals = {"b": 2, "n": 10, "inverse": 0}
    vals.update(over)
    args = []
    for a in WANT[name + ("_host" if host else "")]:
        key = a.split("*")[-1].split()[-1]
        if key in vals:
            args.append(vals[key])
        elif key == "stream" or (pose_only and key in _FULL_IN + _FULL_CD + _FULL_G + ("L",)):
            args.append(None)
        else:
            args.append(_P)
    return getattr(lib, name + ("_host" if host else ""))(*args)


BAD = [("dcl_rigid_points", dict(b=-1)), ("dcl_rigid_points", dict(n=0)), ("dcl_rigid_points", dict(n=-2)),
       ("dcl_rigid_points", dict(inverse=2)),
       ("dcl_rigid_points", dict(pts=None)), ("dcl_rigid_points", dict(R=None)), ("dcl_rigid_points", dict(t=None)),
       ("dcl_rigid_points", dict(out=None)),
       ("dcl_rigid_points_bwd", dict(b=-1)), ("dcl_rigid_points_bwd", dict(n=0)), ("dcl_rigid_points_bwd", dict(pts=None)),
       ("dcl_rigid_points_bwd", dict(R=None)), ("dcl_rigid_points_bwd", dict(t=None)),
       ("dcl_rigid_points_bwd", dict(g_out=None)), ("dcl_rigid_points_bwd", dict(g_R=None)),
       ("dcl_rigid_points_bwd", dict(g_t=None)),
       ("dcl_pose_objective_fwd", dict(b=-1)), ("dcl_pose_objective_fwd", dict(n=0)),
       ("dcl_pose_objective_fwd", dict(posed=None)), ("dcl_pose_objective_fwd", dict(posed_gt=None)),
       ("dcl_pose_objective_fwd", dict(sym=None)), ("dcl_pose_objective_fwd", dict(cd_pose_pt=None)),
       ("dcl_pose_objective_fwd", dict(cd_pose_tp=None)), ("dcl_pose_objective_fwd", dict(crop_sums=None)),
       ("dcl_pose_objective_fwd", dict(packed=None)), ("dcl_pose_objective_fwd", dict(pose_only=True, packed=None)),
       ("dcl_pose_objective_bwd", dict(b=-1)), ("dcl_pose_objective_bwd", dict(n=-1)),
       ("dcl_pose_objective_bwd", dict(posed=None)), ("dcl_pose_objective_bwd", dict(posed_gt=None)),
       ("dcl_pose_objective_bwd", dict(sym=None)), ("dcl_pose_objective_bwd", dict(g_packed=None)),
       ("dcl_pose_objective_bwd", dict(g_posed=None)), ("dcl_pose_objective_bwd", dict(g_cd_pose_pt=None)),
       ("dcl_pose_objective_bwd", dict(g_cd_pose_tp=None))]
# a partial set of the optional arrays: each one missing from the full form, each one present in the pose-only form
BAD += [("dcl_pose_objective_fwd", {k: None}) for k in _FULL_IN + _FULL_CD + ("L",)]
BAD += [("dcl_pose_objective_fwd", {"pose_only": True, k: _P}) for k in _FULL_IN + _FULL_CD + ("L",)]
BAD += [("dcl_pose_objective_bwd", {k: None}) for k in _FULL_IN + _FULL_G + ("L",)]
BAD += [("dcl_pose_objective_bwd", {"pose_only": True, k: _P}) for k in _FULL_IN + _FULL_G + ("L",)]


@pytest.mark.parametrize("name,over", BAD, ids=["%s-%s" % (n[4:], "-".join(sorted(o))) for n, o in BAD])
def test_bad_arguments_return_einval_without_a_gpu(dcl, name, over):
    for tag, lib in _libs(dcl):
        lib.dcl_last_error.restype = C.c_char_p
        for host in (False, True):
            assert _call(lib, name, host, **dict(over)) == -1, (tag, host)
            assert b"invalid argument" in lib.dcl_last_error(), (tag, host)


def test_an_empty_batch_is_not_an_error(dcl):
    for tag, lib in _libs(dcl):
        for name in ("dcl_rigid_points", "dcl_rigid_points_bwd", "dcl_pose_objective_fwd", "dcl_pose_objective_bwd"):
            for host in (False, True):
                assert _call(lib, name, host, b=0) == 0, (tag, name, host)
        assert _call(lib, "dcl_pose_objective_fwd", False, b=0, pose_only=True) == 0, tag
        assert _call(lib, "dcl_rigid_points_bwd", True, b=0, g_pts=None) == 0, tag


def test_g_pts_is_optional_on_the_host_twin(dcl):
    """the one optional pointer of the rigid-points gradient: NULL is accepted (here on the host twin, with real buffers)"""
    gen = torch.Generator().manual_seed(0)      # (unseeded draws made one sum in 230 cancel below allclose's relative bound)
    pts, g = torch.randn(2, 5, 3, generator=gen), torch.randn(2, 5, 3, generator=gen)
    R, t = torch.eye(3).repeat(2, 1, 1), torch.zeros(2, 3)
    g_R, g_t, g_p = dcl.ops.rigid_points_backward_host(pts, R, t, False, g, need_pts=False)
    assert g_p is None and torch.allclose(g_t, g.sum(dim=1))


def _case(b=3, n=40):
    g = torch.Generator().manual_seed(0)
    rot = lambda: torch.linalg.qr(torch.randn(b, 3, 3, generator=g))[0]                      # noqa: E731
    tmp, inp = torch.randn(b, n, 3, generator=g) * 0.05, torch.randn(b, n, 3, generator=g) * 0.05
    pred = {"rot_pred": rot(), "trans_pred": torch.randn(b, 3, generator=g) * 0.01,
            "sym_flag": torch.tensor([0.0, 1.0, 0.0]), "conf": torch.rand(b, 2 * n, generator=g) * 0.8 + 0.1,
            "Xo_pred": torch.randn(b, n, 3, generator=g) * 0.05, "Yc_pred": torch.randn(b, n, 3, generator=g) * 0.05}
    gt = {"rot_gt": rot(), "trans_gt": torch.randn(b, 3, generator=g) * 0.01, "points_tmp": tmp, "points_inp": inp}
    return pred, gt


def test_loss_modules_take_the_objective_switch(dcl):
    for cls in (dcl.DCL_Net.losses, dcl.refiner.losses_refiner):
        assert cls(None).objective == "module" and cls(None, objective="fused").objective == "fused"
        assert cls(None, chamfer="fused", objective="module").chamfer == "fused"
        with pytest.raises(ValueError):
            cls(None, objective="x")
    pred, gt = _case()
    with pytest.raises(RuntimeError, match="GPU"):
        dcl.DCL_Net.losses(None, objective="fused")(pred, gt)
    with pytest.raises(RuntimeError, match="GPU"):
        dcl.refiner.losses_refiner(None, objective="fused")(
            {"rot_pred": pred["rot_pred"], "trans_pred": pred["trans_pred"]}, pred["trans_pred"], pred["rot_pred"],
            gt["points_tmp"], pred["sym_flag"], gt)
    out = dcl.DCL_Net.losses(None)(pred, gt)                       # the default still runs on CPU tensors
    assert set(out) == {"loss_pose", "loss_Xo", "loss_Yc", "loss_conf", "loss_all"}


def test_the_train_step_tool_takes_the_objective_switch():
    text = open(os.path.join(ROOT, "tools", "train_step.py")).read()
    assert "--objective" in text and "module" in text and "fused" in text
