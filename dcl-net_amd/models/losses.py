"""Training objectives of DCL-Net (`losses`, models/DCL_Net.py:261-318) and of the refiner (`losses_refiner`,
models/refiner.py:98-139) as plain torch modules over the GPU outputs of `Network` / `Refiner`.

Point-set terms: `L2_Dis` = per-point Euclidean distance between corresponding points, `CD_Dis` = symmetric
nearest-neighbour (Chamfer) distance for symmetric objects, from coordinate differences in row chunks (`cd_dis`, the
default) or, with chamfer="fused", from the library's own kernels without the pairwise matrix (`cd_dis_fused`).

objective="module" (the default) is the torch composition below.  objective="fused" evaluates the same formulas on
csrc/objective.hip: the rigid transforms (no vendor GEMM), the three Chamfer calls and one packed (5,) tensor of all loss
values with a deterministic one-launch backward; the returned dict holds 0-dim views of that tensor, kept as `self.packed`,
so a training loop logs every value with one `crit.packed.tolist()`."""
import torch
import torch.nn as nn

from .. import ops
from ..autograd import ChamferFn, PoseObjectiveFn, RigidPointsFn


def l2_dis(pred, target):
    """(b,n,3) x (b,n,3) -> (b,n) point-to-corresponding-point distance."""
    return torch.norm(pred - target, dim=2)


def cd_dis(pred, target, chunk=256):
    """(b,n,3) x (b,n,3) -> (b,n): 0.5 * (nearest target of every pred point + nearest pred point of every target point).
    The pairwise Euclidean matrix is formed from coordinate differences (as the reference does), `chunk` pred rows at a
    time, so the (b,N,M,3) difference tensor never exists in full."""
    near_t, near_p = [], None
    for s0 in range(0, pred.shape[1], chunk):
        d = torch.norm(pred[:, s0:s0 + chunk].unsqueeze(2) - target.unsqueeze(1), dim=3)      # (b, chunk, M)
        near_t.append(d.min(dim=2)[0])
        m = d.min(dim=1)[0]
        near_p = m if near_p is None else torch.minimum(near_p, m)
    return 0.5 * (torch.cat(near_t, dim=1) + near_p)


def cd_dis_fused(pred, target, active=None):
    """cd_dis on csrc/chamfer.hip (autograd.ChamferFn): no (b,N,M) intermediate in the forward or kept for the backward,
    which is deterministic.  active (b,) bool / int or None: crops whose flag is 0 are not computed; their rows are 0 and
    take no gradient.  CUDA tensors only."""
    assert pred.shape[1] == target.shape[1], "cd_dis adds the two directions point by point: n == m"
    if not (pred.is_cuda and target.is_cuda):
        raise RuntimeError("cd_dis_fused (chamfer='fused') runs on the GPU only: got %s / %s tensors; the chunked cd_dis "
                           "serves CPU tensors" % (pred.device, target.device))
    if active is not None:
        active = active.to(device=pred.device, dtype=torch.int32).contiguous()
    dist_pt, dist_tp = ChamferFn.apply(pred, target, active)
    return 0.5 * (dist_pt + dist_tp)


def get_cano_label(points_tmp, points_inp, rot_pred, trans_gt):
    """Observed points mapped to the canonical frame and snapped to their nearest template point (kNN, k = 1)."""
    cano = torch.bmm(points_inp - trans_gt, rot_pred)
    _, idx = ops.knn(1, cano.contiguous(), points_tmp.contiguous())
    return torch.gather(points_tmp, 1, idx.long().repeat(1, 1, 3))


class _PoseLoss(nn.Module):
    L2_Dis = staticmethod(l2_dis)
    CD_Dis = staticmethod(cd_dis)
    cd_dis_fused = staticmethod(cd_dis_fused)
    get_cano_label = staticmethod(get_cano_label)

    def __init__(self, chamfer="chunked", objective="module"):
        super().__init__()
        if chamfer not in ("chunked", "fused"):
            raise ValueError("chamfer must be 'chunked' or 'fused', got %r" % (chamfer,))
        if objective not in ("module", "fused"):
            raise ValueError("objective must be 'module' or 'fused', got %r" % (objective,))
        self.chamfer = chamfer
        self.objective = objective
        self.packed = None                         # objective="fused": [loss_pose, loss_Xo, loss_Yc, loss_conf, loss_all]

    def _cd(self, sym):
        """the Chamfer term for this batch: the chunked function, or the fused one restricted to the crops whose term the
        loss does not multiply by 0"""
        if self.chamfer == "chunked":
            return cd_dis
        active = (sym != 0).int()                  # the int32 flags the kernels read, made once per forward
        return lambda pred, target: cd_dis_fused(pred, target, active)

    @staticmethod
    def _fused_inputs(what, sym, *tensors):
        """objective='fused' runs on the GPU only.  -> (sym as the float multiplier of the formula, the int32 flags of the crops
        whose Chamfer terms it does not multiply by 0)"""
        bad = [str(t.device) for t in tensors if not t.is_cuda]
        if bad:
            raise RuntimeError("%s(objective='fused') runs on the GPU only: got %s tensors; objective='module' serves CPU "
                               "tensors" % (what, " / ".join(bad)))
        dev = tensors[0].device
        sym = sym.to(device=dev, dtype=torch.float32).contiguous()
        return sym, (sym != 0).int()

    def _pack(self, packed, keys):
        self.packed = packed
        return {k: packed[i] for k, i in keys}

    @staticmethod
    def _pose_term(posed, posed_gt, sym, cd):
        sym = sym.unsqueeze(1)
        return ((1 - sym) * l2_dis(posed, posed_gt) + sym * cd(posed, posed_gt)).mean(dim=1).mean()


class losses(_PoseLoss):
    """loss_all = loss_pose + 5 loss_Xo + loss_Yc + loss_conf (models/DCL_Net.py:264-304)."""

    def __init__(self, cfg=None, chamfer="chunked", objective="module"):
        super().__init__(chamfer, objective)

    def forward(self, pred, gt):
        if self.objective == "fused":
            return self._forward_fused(pred, gt)
        R, t, sym, conf = pred["rot_pred"], pred["trans_pred"], pred["sym_flag"], pred["conf"]
        dev = R.device
        R_gt, t_gt = gt["rot_gt"].to(dev), gt["trans_gt"].to(dev)
        tmp, inp = gt["points_tmp"], gt["points_inp"]
        s1, cd = sym.unsqueeze(1), self._cd(sym)
        posed = torch.bmm(tmp, R.transpose(1, 2)) + t.unsqueeze(1)
        posed_gt = torch.bmm(tmp, R_gt.transpose(1, 2)) + t_gt.unsqueeze(1)
        loss_pose = self._pose_term(posed, posed_gt, sym, cd)
        Xo, Yc = pred["Xo_pred"], pred["Yc_pred"]
        inp_cano_pred = torch.bmm(inp - t.unsqueeze(1), R).detach()
        inp_cano_gt = torch.bmm(inp - t_gt.unsqueeze(1), R_gt).detach()
        loss_Xo = (1 - s1) * l2_dis(Xo, inp_cano_gt) + 0.5 * s1 * (cd(Xo, tmp) + l2_dis(Xo, inp_cano_pred))
        loss_Yc = (1 - s1) * l2_dis(Yc, posed_gt) + 0.5 * s1 * (cd(Yc, posed_gt) + l2_dis(Yc, posed.detach()))
        loss_conf = torch.mean(torch.cat([loss_Xo, loss_Yc], dim=1).detach() * conf - 0.01 * torch.log(conf))
        out = {"loss_pose": loss_pose, "loss_Xo": loss_Xo.mean(), "loss_Yc": loss_Yc.mean(), "loss_conf": loss_conf}
        out["loss_all"] = out["loss_pose"] + 5 * out["loss_Xo"] + 1 * out["loss_Yc"] + 1 * out["loss_conf"]
        return out

    def _forward_fused(self, pred, gt):
        R, t, conf, Xo, Yc = pred["rot_pred"], pred["trans_pred"], pred["conf"], pred["Xo_pred"], pred["Yc_pred"]
        tmp, inp = gt["points_tmp"], gt["points_inp"]
        if tmp.shape[1] != inp.shape[1]:
            raise ValueError("losses(objective='fused') adds the template's and the observed points' terms point by point: "
                             "n == m wanted, got %d template and %d observed points" % (tmp.shape[1], inp.shape[1]))
        sym, active = self._fused_inputs("losses", pred["sym_flag"], R, t, conf, Xo, Yc, tmp, inp)
        f = lambda v: v.to(device=R.device, dtype=torch.float32).contiguous()                 # noqa: E731
        R_gt, t_gt, tmp, inp = f(gt["rot_gt"]), f(gt["trans_gt"]), f(tmp), f(inp)
        posed = RigidPointsFn.apply(tmp, R, t, False)
        with torch.no_grad():
            Rd, td = f(R.detach()), f(t.detach())
            posed_gt = ops.rigid_points(tmp, R_gt, t_gt, False)
            cano_pred = ops.rigid_points(inp, Rd, td, True)
            cano_gt = ops.rigid_points(inp, R_gt, t_gt, True)
        cd_pose = ChamferFn.apply(posed, posed_gt, active)
        cd_Xo = ChamferFn.apply(Xo, tmp, active)
        cd_Yc = ChamferFn.apply(Yc, posed_gt, active)
        packed = PoseObjectiveFn.apply(posed, posed_gt, sym, cd_pose[0], cd_pose[1], Yc, cano_pred, cano_gt, Xo, conf,
                                       cd_Xo[0], cd_Xo[1], cd_Yc[0], cd_Yc[1])
        return self._pack(packed, (("loss_pose", 0), ("loss_Xo", 1), ("loss_Yc", 2), ("loss_conf", 3), ("loss_all", 4)))


class losses_refiner(_PoseLoss):
    """Pose loss of the template posed by the refiner's delta and then by the current pose (models/refiner.py:101-125)."""

    def __init__(self, cfg=None, chamfer="chunked", objective="module"):
        super().__init__(chamfer, objective)

    def forward(self, pred_refiner, trans_cur, rot_cur, points_tmp, sym_flag, gt):
        dR, dt = pred_refiner["rot_pred"], pred_refiner["trans_pred"]
        if self.objective == "fused":
            sym, active = self._fused_inputs("losses_refiner", sym_flag, dR, dt, trans_cur, rot_cur, points_tmp)
            f = lambda v: v.to(device=dR.device, dtype=torch.float32).contiguous()            # noqa: E731
            tmp = f(points_tmp)
            posed_delta = RigidPointsFn.apply(tmp, dR, dt, False)
            refined = RigidPointsFn.apply(posed_delta, rot_cur, trans_cur, False)             # its gradient goes to its points
            with torch.no_grad():
                posed_gt = ops.rigid_points(tmp, f(gt["rot_gt"]), f(gt["trans_gt"]), False)
            cd_pose = ChamferFn.apply(refined, posed_gt, active)
            packed = PoseObjectiveFn.apply(refined, posed_gt, sym, cd_pose[0], cd_pose[1])
            return self._pack(packed, (("loss_pose", 0), ("loss_all", 4)))
        dev = dR.device
        R_gt, t_gt = gt["rot_gt"].to(dev), gt["trans_gt"].to(dev)
        posed_delta = torch.bmm(points_tmp, dR.transpose(1, 2)) + dt.unsqueeze(1)
        posed_gt = torch.bmm(points_tmp, R_gt.transpose(1, 2)) + t_gt.unsqueeze(1)
        refined = torch.bmm(posed_delta, rot_cur.transpose(1, 2)) + trans_cur.unsqueeze(1)
        loss_pose = self._pose_term(refined, posed_gt, sym_flag, self._cd(sym_flag))
        return {"loss_pose": loss_pose, "loss_all": loss_pose}
