"""The fused Chamfer entry points (dcl_chamfer_fwd, dcl_chamfer_bwd) are declared with the documented argument lists, exported
by both libraries and answer bad arguments and an empty batch without a GPU; the loss modules take the `chamfer=` switch and
their default is the code it was before the switch existed."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WANT = {
    "dcl_chamfer_fwd": ["int b", "int n", "int m", "const float *pred", "const float *target", "const int32_t *active",
                        "float *dist_pt", "int32_t *idx_pt", "float *dist_tp", "int32_t *idx_tp", "dclStream_t stream"],
    "dcl_chamfer_bwd": ["int b", "int n", "int m", "const float *pred", "const float *target", "const int32_t *active",
                        "const int32_t *idx_pt", "const int32_t *idx_tp", "const float *g_pt", "const float *g_tp",
                        "float *grad_pred", "float *grad_target", "dclStream_t stream"],
}


def declarations():
    text = open(os.path.join(ROOT, "include", "dclnet_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for m in re.finditer(r"\bint\s+(dcl_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        out[m.group(1)] = [re.sub(r"\s+", " ", a).strip() for a in m.group(2).split(",")]
    return out


def test_header_declares_the_chamfer_entry_points():
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
    assert callable(dcl.ops.chamfer) and callable(dcl.ops.chamfer_backward)
    assert hasattr(dcl.autograd.ChamferFn, "apply")
    from importlib import import_module
    mod = import_module("dcl-net_amd.models.losses")
    assert callable(mod.cd_dis_fused) and callable(dcl.DCL_Net.losses.cd_dis_fused)
    assert dcl.DCL_Net.losses.CD_Dis is mod.cd_dis and dcl.refiner.losses_refiner.CD_Dis is mod.cd_dis


_BUF = (C.c_char * 64)()                 # host bytes standing in for device buffers: a rejected call never dereferences them
_P = C.cast(_BUF, C.c_void_p)


def _fwd(L, b=2, n=10, m=7, pred=_P, target=_P, dist_pt=_P, idx_pt=_P, dist_tp=_P, idx_tp=_P):
    return L.dcl_chamfer_fwd(b, n, m, pred, target, None, dist_pt, idx_pt, dist_tp, idx_tp, None)


def _bwd(L, b=2, n=10, m=7, pred=_P, target=_P, idx_pt=_P, idx_tp=_P, g_pt=_P, g_tp=_P, grad_pred=_P, grad_target=_P):
    return L.dcl_chamfer_bwd(b, n, m, pred, target, None, idx_pt, idx_tp, g_pt, g_tp, grad_pred, grad_target, None)


@pytest.mark.parametrize("call", [
    lambda L: _fwd(L, n=0),
    lambda L: _fwd(L, m=0),
    lambda L: _fwd(L, n=-3),
    lambda L: _fwd(L, b=-1),
    lambda L: _fwd(L, pred=None),
    lambda L: _fwd(L, target=None),
    lambda L: _fwd(L, dist_pt=None),
    lambda L: _fwd(L, idx_pt=None),
    lambda L: _fwd(L, dist_tp=None),
    lambda L: _fwd(L, idx_tp=None),
    lambda L: _bwd(L, n=0),
    lambda L: _bwd(L, m=-1),
    lambda L: _bwd(L, b=-1),
    lambda L: _bwd(L, pred=None),
    lambda L: _bwd(L, target=None),
    lambda L: _bwd(L, idx_pt=None),
    lambda L: _bwd(L, idx_tp=None),
    lambda L: _bwd(L, g_pt=None),
    lambda L: _bwd(L, g_tp=None),
    lambda L: _bwd(L, grad_pred=None, grad_target=None),
])
def test_bad_arguments_return_einval_without_a_gpu(dcl, call):
    for tag, lib in _libs(dcl):
        lib.dcl_last_error.restype = C.c_char_p
        assert call(lib) == -1, tag
        assert b"invalid argument" in lib.dcl_last_error(), tag


def test_an_empty_batch_is_not_an_error(dcl):
    for tag, lib in _libs(dcl):
        assert _fwd(lib, b=0) == 0, tag
        assert _bwd(lib, b=0) == 0, tag
        assert _bwd(lib, b=0, grad_target=None) == 0, tag


def test_loss_modules_reject_an_unknown_chamfer_mode(dcl):
    for cls in (dcl.DCL_Net.losses, dcl.refiner.losses_refiner):
        with pytest.raises(ValueError):
            cls(None, chamfer="x")
        assert cls(None).chamfer == "chunked" and cls(None, chamfer="fused").chamfer == "fused"


def _case(b=3, n=40):
    g = torch.Generator().manual_seed(0)
    rot = lambda: torch.linalg.qr(torch.randn(b, 3, 3, generator=g))[0]                      # noqa: E731
    tmp, inp = torch.randn(b, n, 3, generator=g) * 0.05, torch.randn(b, n, 3, generator=g) * 0.05
    pred = {"rot_pred": rot(), "trans_pred": torch.randn(b, 3, generator=g) * 0.01,
            "sym_flag": torch.tensor([0.0, 1.0, 0.0]), "conf": torch.rand(b, 2 * n, generator=g) * 0.8 + 0.1,
            "Xo_pred": torch.randn(b, n, 3, generator=g) * 0.05, "Yc_pred": torch.randn(b, n, 3, generator=g) * 0.05}
    gt = {"rot_gt": rot(), "trans_gt": torch.randn(b, 3, generator=g) * 0.01, "points_tmp": tmp, "points_inp": inp}
    return pred, gt


def test_the_default_loss_is_the_chunked_code_bit_for_bit_on_cpu_tensors(dcl):
    """losses(None) on CPU tensors against the module's formula as it stood before the switch, written out here on the same
    l2_dis / cd_dis in the same order: equal bits.  A regression guard by design: it passes before the switch exists too, and
    it checks the composition only -- cd_dis itself is pinned by tests/test_losses.py against the literal formula."""
    pred, gt = _case()
    crit = dcl.DCL_Net.losses(None)
    out = crit(pred, gt)
    L2, CD = crit.L2_Dis, crit.CD_Dis
    R, t, sym, conf = pred["rot_pred"], pred["trans_pred"], pred["sym_flag"], pred["conf"]
    R_gt, t_gt, tmp, inp = gt["rot_gt"], gt["trans_gt"], gt["points_tmp"], gt["points_inp"]
    s1 = sym.unsqueeze(1)
    posed = torch.bmm(tmp, R.transpose(1, 2)) + t.unsqueeze(1)
    posed_gt = torch.bmm(tmp, R_gt.transpose(1, 2)) + t_gt.unsqueeze(1)
    loss_pose = ((1 - s1) * L2(posed, posed_gt) + s1 * CD(posed, posed_gt)).mean(dim=1).mean()
    Xo, Yc = pred["Xo_pred"], pred["Yc_pred"]
    icp, icg = torch.bmm(inp - t.unsqueeze(1), R), torch.bmm(inp - t_gt.unsqueeze(1), R_gt)
    loss_Xo = (1 - s1) * L2(Xo, icg) + 0.5 * s1 * (CD(Xo, tmp) + L2(Xo, icp))
    loss_Yc = (1 - s1) * L2(Yc, posed_gt) + 0.5 * s1 * (CD(Yc, posed_gt) + L2(Yc, posed))
    loss_conf = torch.mean(torch.cat([loss_Xo, loss_Yc], dim=1) * conf - 0.01 * torch.log(conf))
    want = loss_pose + 5 * loss_Xo.mean() + 1 * loss_Yc.mean() + 1 * loss_conf
    assert torch.equal(out["loss_all"], want) and torch.equal(out["loss_pose"], loss_pose)
    assert torch.equal(out["loss_conf"], loss_conf)
    # the refiner loss likewise
    pr = {"rot_pred": pred["rot_pred"].transpose(1, 2).contiguous(), "trans_pred": pred["trans_pred"] * 0.5}
    lo = dcl.refiner.losses_refiner(None)(pr, t, R, tmp, sym, gt)
    refined = torch.bmm(torch.bmm(tmp, pr["rot_pred"].transpose(1, 2)) + pr["trans_pred"].unsqueeze(1), R.transpose(1, 2)) + t.unsqueeze(1)
    want_r = ((1 - s1) * L2(refined, posed_gt) + s1 * CD(refined, posed_gt)).mean(dim=1).mean()
    assert torch.equal(lo["loss_all"], want_r)


def test_the_fused_form_refuses_cpu_tensors_with_a_clear_error(dcl):
    pred, gt = _case()
    with pytest.raises(RuntimeError, match="GPU"):
        dcl.DCL_Net.losses(None, chamfer="fused")(pred, gt)
    with pytest.raises(RuntimeError, match="GPU"):
        dcl.DCL_Net.losses.cd_dis_fused(pred["Xo_pred"], gt["points_tmp"])
