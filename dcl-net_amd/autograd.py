"""torch.autograd Functions of the ops on DCL-Net's path, mirroring the reference's Function classes
(libs/spconv/spconv/functional.py:20-166, libs/pointnet_sp/pointnet2_utils.py:41-86,
libs/pointnet_lib/pointnet2_utils.py:40-76,144-238, libs/pointgroup_ops/functions/pointgroup_ops.py:42-75):
forward = the inference kernels, backward = csrc/backward.hip; and of the correspondence attention (CrossAttentionFn:
forward = dcl_cross_attention, backward = csrc/attention_bwd.hip), which the reference forms from bmm and softmax;
and of the losses' Chamfer distance (ChamferFn: csrc/chamfer.hip in both passes); and of the rotation head's projection
(Ortho9dFn: forward = dcl_ortho9d_to_matrix, backward = csrc/rotation_grad.hip); and of the stage-2 refiner's shared MLP
(RefinerShareFn: forward = the own GEMM core, backward = csrc/linear_bwd.hip + the same core); and of the point-major dense
half of stage 1 (PointLinearFn: the same core and csrc/linear_bwd.hip per layer; ConfPoolPmFn: csrc/conf_pool_pm.hip); and of what train_heads="kernels" switches (NarrowLinearFn: csrc/linear_narrow.hip,
the per-point heads' last layers; PoseHeadsFn: csrc/pose_heads_grad.hip, the two pose heads of stage 1 and stage 2).
Used by the module mirrors (spconv/, libs/) so that `Network(cfg, mode='train')` is trainable on the GPU."""
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import ops as _ops


class SparseConvFn(Function):
    """SparseConvFunction / SubMConvFunction (functional.py:20-88).  wgrad: the form of the weight gradient, "rows" (default) or
    "pairs" (ops.sparse_conv_backward); the pair list is built in the backward call and dies with it.  dgrad: the form of the
    input gradient, "conv" (default) or "direct" (ops.sparse_conv_dgrad).  fwd: the form of the forward, "tiles" (default) or
    "compact" (ops.sparse_conv_compact); the backward does not depend on it, and its dgrad="conv" route keeps re-entering the
    default forward dispatcher."""

    @staticmethod
    def forward(ctx, features, W, nbr, n_out, subm, wgrad="rows", dgrad="conv", fwd="tiles"):
        ctx.save_for_backward(features, W, nbr)
        ctx.n_out, ctx.subm, ctx.wgrad = int(n_out), bool(subm), _ops.check_conv_wgrad(wgrad)
        ctx.dgrad = _ops.check_conv_dgrad(dgrad)
        return _ops.sparse_conv(features, nbr, n_out, W, subm, form=_ops.check_conv_fwd(fwd))

    @staticmethod
    def backward(ctx, grad_output):
        features, W, nbr = ctx.saved_tensors
        dx, dW = _ops.sparse_conv_backward(features, W, grad_output, nbr, ctx.n_out, ctx.subm,
                                           need_dx=ctx.needs_input_grad[0], wgrad=ctx.wgrad, dgrad=ctx.dgrad)
        return dx, dW.view_as(W), None, None, None, None, None, None


class SparseAvgPoolFn(Function):
    """SparseAvgPoolFunction with use_gs=False (functional.py:137-166)."""

    @staticmethod
    def forward(ctx, features, nbr, n_out):
        out, rf = _ops.sparse_avgpool(features, nbr, n_out, want_rf=True)
        ctx.save_for_backward(nbr, rf)
        ctx.n_out, ctx.n_in = int(n_out), features.shape[0]
        return out

    @staticmethod
    def backward(ctx, grad_output):
        nbr, rf = ctx.saved_tensors
        return _ops.sparse_avgpool_backward(grad_output, nbr, ctx.n_out, ctx.n_in, rf), None, None


class ThreeInterpolateFn(Function):
    """ThreeInterpolate of libs/pointnet_sp (pointnet2_utils.py:41-86)."""

    @staticmethod
    def forward(ctx, features, idx, weight):
        ctx.save_for_backward(idx, weight)
        ctx.m = features.shape[0]
        return _ops.three_interpolate_sp(features, idx, weight)

    @staticmethod
    def backward(ctx, grad_out):
        idx, weight = ctx.saved_tensors
        return _ops.three_interpolate_grad_sp(grad_out, idx, weight, ctx.m), None, None


class GroupPointsFn(Function):
    """GroupingOperation of libs/pointnet_lib (pointnet2_utils.py:195-235): no gradient for idx."""

    @staticmethod
    def forward(ctx, features, idx):
        idx = idx.contiguous().int()
        ctx.save_for_backward(idx)
        ctx.n = features.shape[2]
        return _ops.group_points(features.contiguous(), idx)

    @staticmethod
    def backward(ctx, grad_out):
        (idx,) = ctx.saved_tensors
        return _ops.group_points_grad(grad_out, idx, ctx.n), None


class GatherPointsFn(Function):
    """GatherOperation of libs/pointnet_lib (pointnet2_utils.py:40-76): no gradient for idx."""

    @staticmethod
    def forward(ctx, features, idx):
        idx = idx.contiguous().int()
        ctx.save_for_backward(idx)
        ctx.n = features.shape[2]
        return _ops.gather_points(features.contiguous(), idx)

    @staticmethod
    def backward(ctx, grad_out):
        (idx,) = ctx.saved_tensors
        return _ops.gather_points_grad(grad_out, idx, ctx.n), None


class ThreeInterpolateBatchedFn(Function):
    """ThreeInterpolate of libs/pointnet_lib (pointnet2_utils.py:144-189): features (B,C,m); no gradient for idx or weight
    (the reference gives none either)."""

    @staticmethod
    def forward(ctx, features, idx, weight):
        idx, weight = idx.contiguous().int(), weight.contiguous()
        ctx.save_for_backward(idx, weight)
        ctx.m = features.shape[2]
        return _ops.three_interpolate(features.contiguous(), idx, weight)

    @staticmethod
    def backward(ctx, grad_out):
        idx, weight = ctx.saved_tensors
        return _ops.three_interpolate_grad(grad_out, idx, weight, ctx.m), None, None


class VoxelizationFn(Function):
    """Voxelization (pointgroup_ops.py:42-75)."""

    @staticmethod
    def forward(ctx, feats, map_rule, mode=4):
        ctx.save_for_backward(map_rule)
        ctx.mode, ctx.n = mode, feats.shape[0]
        return _ops.voxelize_fp(feats, map_rule, mode)

    @staticmethod
    def backward(ctx, d_out):
        (map_rule,) = ctx.saved_tensors
        return _ops.voxelize_bp(d_out, map_rule, ctx.n, ctx.mode), None, None


class CrossAttentionFn(Function):
    """One direction of the correspondence attention, Aligner.forward + the two following bmm (models/Modules.py:128-138,
    models/DCL_Net.py:961-964), without the attention map in either pass: Q (b, nq, 64), K (b, nk, 64), V1 (b, nk, 256),
    V2 (b, nk, 64) -> O1 (b, nq, 256), O2 (b, nq, 64) with O = softmax_keys(Q K^T) V.  Forward = ops.cross_attention (the
    same bits as the op itself), backward = ops.cross_attention_backward (deterministic).  K and V2 may be one tensor: its
    gradient is then dK + dV2."""

    @staticmethod
    def forward(ctx, Q, K, V1, V2):
        b, nq, nk = Q.shape[0], Q.shape[1], K.shape[1]
        Q2, K2 = _ops.N.f32c(Q).view(b * nq, -1), _ops.N.f32c(K).view(b * nk, -1)
        V12 = _ops.N.f32c(V1).view(b * nk, -1)
        V22 = K2 if V2 is K else _ops.N.f32c(V2).view(b * nk, -1)
        O1 = torch.empty((b, nq, V12.shape[1]), dtype=torch.float32, device=Q.device)
        O2 = torch.empty((b, nq, V22.shape[1]), dtype=torch.float32, device=Q.device)
        _ops.cross_attention(b, Q2, K2, V12, O1.view(b * nq, -1), V22, O2.view(b * nq, -1))
        ctx.save_for_backward(Q2, K2, V12, V22, O1, O2)
        ctx.set_materialize_grads(False)                  # an unused output arrives as None, not as a tensor of zeros
        ctx.b = b
        ctx.shapes = (Q.shape, K.shape, V1.shape, V2.shape)
        return O1, O2

    @staticmethod
    def backward(ctx, dO1, dO2):
        Q2, K2, V12, V22, O1, O2 = ctx.saved_tensors
        if (dO1 is None and dO2 is None) or not any(ctx.needs_input_grad):
            return None, None, None, None
        O1, O2 = O1.view(-1, O1.shape[2]), O2.view(-1, O2.shape[2])
        g1 = torch.zeros_like(O1) if dO1 is None else _ops.N.f32c(dO1).view(O1.shape)
        g2 = None if dO2 is None else _ops.N.f32c(dO2).view(O2.shape)
        grads = _ops.cross_attention_backward(ctx.b, Q2, K2, V12, V22, O1, O2, g1, g2)
        return tuple(g.view(s) if n else None for g, s, n in zip(grads, ctx.shapes, ctx.needs_input_grad))


class ChamferFn(Function):
    """Nearest-neighbour distances between two clouds in both directions, the two halves of the reference's CD_Dis
    (models/DCL_Net.py:306-312), without the pairwise matrix in either pass: pred (b,n,3), target (b,m,3), active (b,) i32 or
    None -> dist_pt (b,n), dist_tp (b,m).  Forward = ops.chamfer, backward = ops.chamfer_backward (deterministic).  Only the
    two clouds and the two index tensors are kept for the backward, and only the gradients that are asked for are computed."""

    @staticmethod
    def forward(ctx, pred, target, active=None):
        pred, target = _ops.N.f32c(pred), _ops.N.f32c(target)
        dist_pt, idx_pt, dist_tp, idx_tp = _ops.chamfer(pred, target, active)
        ctx.save_for_backward(pred, target, idx_pt, idx_tp)
        # the (b,) flag vector rides on ctx, not in save_for_backward: it is an int32 input that can never take a gradient and
        # no output of this Function, so the saved set stays the two clouds and the two index tensors
        ctx.active = active
        return dist_pt, dist_tp

    @staticmethod
    def backward(ctx, g_pt, g_tp):
        pred, target, idx_pt, idx_tp = ctx.saved_tensors
        need_pred, need_target = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_pred or need_target):
            return None, None, None
        grad_pred, grad_target = _ops.chamfer_backward(pred, target, idx_pt, idx_tp, _ops.N.f32c(g_pt), _ops.N.f32c(g_tp),
                                                       ctx.active, need_pred, need_target)
        return grad_pred, grad_target, None


class Ortho9dFn(Function):
    """ortho9d2matrix (models/DCL_Net.py:15-36) with its gradient on the device: o9 (b,9) -> R (b,3,3).  Forward =
    ops.ortho9d_to_matrix, so a train-mode rotation is the eval kernel's bit for bit; backward = ops.ortho9d_backward, the
    closed form of the polar factor's derivative (denominators s_i + s_j, about 2 for near-orthonormal axes; autograd through
    an SVD's U and V divides by s_i^2 - s_j^2).  Only o9 is kept, nothing is copied to the host, and the same inputs give the
    same bits.  CUDA tensors only."""

    @staticmethod
    def forward(ctx, o9):
        if not o9.is_cuda:
            raise RuntimeError("Ortho9dFn (train_rotation='device') runs on the GPU only: got a %s tensor; the 'host' "
                               "composition serves CPU tensors" % (o9.device,))
        o9 = _ops.N.f32c(o9)
        ctx.save_for_backward(o9)
        return _ops.ortho9d_to_matrix(o9)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_R):
        o9, = ctx.saved_tensors
        return _ops.ortho9d_backward(o9, _ops.N.f32c(grad_R))


class RigidPointsFn(Function):
    """Rigid transform of b clouds with its gradient on the device: pts (b,n,3), R (b,3,3), t (b,3), inverse -> (b,n,3);
    inverse False: R p + t, True: R^T (p - t).  Forward = ops.rigid_points, backward = ops.rigid_points_backward: g_R and g_t
    are sums over a crop's points in the pinned order (deterministic), the gradient of pts is formed only when it is asked
    for.  No vendor GEMM in either pass.  CUDA tensors only."""

    @staticmethod
    def forward(ctx, pts, R, t, inverse=False):
        if not (pts.is_cuda and R.is_cuda and t.is_cuda):
            raise RuntimeError("RigidPointsFn (objective='fused') runs on the GPU only: got %s / %s / %s tensors; the "
                               "'module' objective serves CPU tensors" % (pts.device, R.device, t.device))
        pts, R, t = _ops.N.f32c(pts), _ops.N.f32c(R), _ops.N.f32c(t)
        ctx.save_for_backward(pts, R, t)
        ctx.inverse = bool(inverse)
        return _ops.rigid_points(pts, R, t, ctx.inverse)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out):
        pts, R, t = ctx.saved_tensors
        need = ctx.needs_input_grad
        if not (need[0] or need[1] or need[2]):
            return None, None, None, None
        g_R, g_t, g_pts = _ops.rigid_points_backward(pts, R, t, ctx.inverse, _ops.N.f32c(g_out), need_pts=need[0])
        return g_pts, (g_R if need[1] else None), (g_t if need[2] else None), None


class PoseObjectiveFn(Function):
    """The per-point terms of the training objective and their ordered sums as ONE packed tensor (ops.pose_objective):
    apply(posed, posed_gt, sym, cd_pose_pt, cd_pose_tp[, Yc, cano_pred, cano_gt, Xo, conf, cd_Xo_pt, cd_Xo_tp, cd_Yc_pt,
    cd_Yc_tp]) -> packed (5,) = [loss_pose, loss_Xo, loss_Yc, loss_conf, loss_all].  Gradients go to posed, Xo, Yc, conf and
    the six Chamfer halves (one launch, ops.pose_objective_backward; the upstream gradient stays on the device); posed_gt,
    cano_pred, cano_gt and sym take none and ride on ctx.  Saved for the backward: the inputs it reads and the per-point rows
    L -- not packed, not the per-crop sums."""

    @staticmethod
    def forward(ctx, posed, posed_gt, sym, cd_pose_pt, cd_pose_tp, Yc=None, cano_pred=None, cano_gt=None, Xo=None, conf=None,
                cd_Xo_pt=None, cd_Xo_tp=None, cd_Yc_pt=None, cd_Yc_tp=None):
        c = _ops.N.f32c
        full = Xo is not None
        posed, posed_gt, sym = c(posed), c(posed_gt), c(sym)
        cd_pose = (c(cd_pose_pt), c(cd_pose_tp))
        if full:
            Yc, cano_pred, cano_gt, Xo, conf = c(Yc), c(cano_pred), c(cano_gt), c(Xo), c(conf)
            cd_Xo, cd_Yc = (c(cd_Xo_pt), c(cd_Xo_tp)), (c(cd_Yc_pt), c(cd_Yc_tp))
        else:
            cd_Xo = cd_Yc = None
        packed, L = _ops.pose_objective(posed, posed_gt, sym, cd_pose, Yc, cano_pred, cano_gt, Xo, conf, cd_Xo, cd_Yc)
        # the backward reads the clouds, conf and L; the Chamfer halves enter it only through sym (their gradients are
        # per-crop constants), so they are not kept
        ctx.save_for_backward(*((posed, Yc, Xo, conf, L) if full else (posed,)))
        ctx.fixed = (posed_gt, sym, cano_pred, cano_gt)
        ctx.full = full
        return packed

    @staticmethod
    @once_differentiable
    def backward(ctx, g_packed):
        posed_gt, sym, cano_pred, cano_gt = ctx.fixed
        g_packed = _ops.N.f32c(g_packed)
        if ctx.full:
            posed, Yc, Xo, conf, L = ctx.saved_tensors
        else:
            posed, = ctx.saved_tensors
            Yc = Xo = conf = L = None
        g_posed, g_Xo, g_Yc, g_conf, g_cdp, g_cdx, g_cdy = _ops.pose_objective_backward(
            g_packed, posed, posed_gt, sym, Yc, cano_pred, cano_gt, Xo, conf, L)
        if not ctx.full:
            return g_posed, None, None, g_cdp[0], g_cdp[1]
        return (g_posed, None, None, g_cdp[0], g_cdp[1], g_Yc, None, None, g_Xo, g_conf, g_cdx[0], g_cdx[1], g_cdy[0],
                g_cdy[1])


class RefinerShareFn(Function):
    """The stage-2 refiner's MLP_share (Conv1d 259 -> 512 -> 512 -> 1024, ReLU after each) with the confidence-weighted sum over
    the points, trained on the library's own GEMM kernels: apply(xyz_pm (M,3), F_pm (M,256), conf_w (b,n), W0, b0, W1, b1, W2,
    b2) -> shared (b,1024), M = b n, n a multiple of ops.LINEAR_POOL_TILE, the W* the Conv1d weights as registered (out, in, 1).
    Forward = the calls of Refiner.forward_pm up to `shared` on the fp32-MFMA core (ops.linear_dma, ops.affine3_relu,
    ops.linear_pool_dma + the tile sum); the split-bf16 core takes no part, the weights change every step.  Saved: the inputs,
    h1 and h2 -- not the (M,1024) activation, which the backward recomputes into scratch.  Backward: ops.relu_bwd (mask + bias
    gradient), ops.linear_wgrad (weight gradient) and ops.linear_dma with the registered weight as its (K,N) matrix (input
    gradient) per layer; layer 0 writes its two weight-gradient blocks (xyz | features) into one (512,259) tensor.  An optional
    trailing argument wgrad="split" sends all four weight gradients to ops.linear_wgrad_split (the bf16 matrix pipe, fp32-sized
    errors, its own pinned order) whatever their shapes (a tuple of four forms -- W0's xyz block, W0's feature block, W1, W2 -- chooses per
    gradient); everything else keeps its bits.  Every
    reduction has a pinned order: the same inputs give the same gradients bit for bit.  xyz_pm, F_pm and conf_w take no
    gradient (the training script detaches them): asking for one raises."""

    @staticmethod
    def forward(ctx, xyz_pm, F_pm, conf_w, W0, b0, W1, b1, W2, b2, wgrad="fp32"):
        forms = (wgrad,) * 4 if isinstance(wgrad, str) else tuple(wgrad)
        if len(forms) != 4:
            raise ValueError("RefinerShareFn: wgrad is one form or four (W0's xyz block, W0's feature block, W1, W2), got %r"
                             % (wgrad,))
        ctx.wgrad = tuple(_ops.check_linear_wgrad(f, "wgrad") for f in forms)
        if any(ctx.needs_input_grad[:3]):
            raise ValueError("RefinerShareFn: xyz_pm, F_pm and conf_w take no gradient (detach them)")
        for t in (xyz_pm, F_pm, conf_w, W0, b0, W1, b1, W2, b2):
            if not (t.is_cuda and t.dtype == torch.float32):
                raise RuntimeError("RefinerShareFn runs on float32 CUDA tensors only (got %s on %s)" % (t.dtype, t.device))
        b, n = conf_w.shape
        M = b * n
        if n % _ops.LINEAR_POOL_TILE:
            raise ValueError("RefinerShareFn: n %% %d == 0 required (the pooling tile), got n = %d" % (_ops.LINEAR_POOL_TILE, n))
        assert tuple(xyz_pm.shape) == (M, 3) and tuple(F_pm.shape) == (M, F_pm.shape[1]) and W0.shape[1] == 3 + F_pm.shape[1]
        xyz_pm, F_pm, conf_w = xyz_pm.contiguous(), F_pm.contiguous(), conf_w.contiguous()
        W0, W1, W2 = W0.contiguous(), W1.contiguous(), W2.contiguous()
        b0, b1, b2 = b0.contiguous(), b1.contiguous(), b2.contiguous()
        Wt0 = W0[:, :, 0].t()
        Wt0x, Wt0f = Wt0[:3].contiguous(), Wt0[3:].contiguous()
        Wt1, Wt2 = W1[:, :, 0].t().contiguous(), W2[:, :, 0].t().contiguous()
        feat_term = _ops.linear_dma(F_pm, Wt0f, b0)
        h1 = _ops.affine3_relu(xyz_pm, Wt0x, feat_term)
        h2 = _ops.linear_dma(h1, Wt1, b1, True)
        part = _ops.linear_pool_dma(h2, Wt2, b2, conf_w.reshape(-1), relu=True)
        ctx.save_for_backward(xyz_pm, F_pm, conf_w, W1, W2, b2, Wt2, h1, h2)
        return part.view(b, n // _ops.LINEAR_POOL_TILE, -1).sum(dim=1)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_shared):
        if any(ctx.needs_input_grad[:3]):
            raise ValueError("RefinerShareFn: xyz_pm, F_pm and conf_w take no gradient (detach them)")
        xyz_pm, F_pm, conf_w, W1, W2, b2, Wt2, h1, h2 = ctx.saved_tensors
        b, n = conf_w.shape
        g_shared = _ops.N.f32c(g_shared)
        # layer 2: the pooled activation again (scratch), masked and weighted in place
        h3 = _ops.linear_dma(h2, Wt2, b2, True)
        dz, db2 = _ops.relu_bwd(h3, roww=conf_w.reshape(-1), gpool=g_shared, rows_per_crop=n, out=h3)
        wgrad = ctx.wgrad
        dW2 = _ops.linear_wgrad_as(wgrad[3], dz, h2)
        dh = _ops.linear_dma(dz, W2[:, :, 0])
        del h3, dz
        # layer 1
        dz, db1 = _ops.relu_bwd(h2, dh, out=dh)
        dW1 = _ops.linear_wgrad_as(wgrad[2], dz, h1)
        dh = _ops.linear_dma(dz, W1[:, :, 0])
        # layer 0: no input gradient; the weight's two column blocks
        dz, db0 = _ops.relu_bwd(h1, dh, out=dh)
        dW0 = torch.empty((h1.shape[1], 3 + F_pm.shape[1]), dtype=torch.float32, device=dz.device)
        _ops.linear_wgrad_as(wgrad[0], dz, xyz_pm, out=dW0[:, :3])
        _ops.linear_wgrad_as(wgrad[1], dz, F_pm, out=dW0[:, 3:])
        # (one gradient per argument actually passed: the optional trailing `wgrad` takes None, and only when it was given)
        grads = (None, None, None, dW0.unsqueeze(2), db0, dW1.unsqueeze(2), db1, dW2.unsqueeze(2), db2)
        return grads + (None,) * (len(ctx.needs_input_grad) - len(grads))


class ConfPoolFn(Function):
    """The confidence-weighted pooling that ends stage 1's dense half (models/DCL_Net.py: conf_1 ... F_p_wei) on the library's
    own kernels: apply(logit1 (b,1,n1) or (b,n1), logit2 (b,1,n2) or (b,n2), F1 (b,C,n1), F2 (b,C,n2)) -> (conf (b, n1+n2) =
    sigmoid(cat[logit1, logit2]), pooled (b,C) = sum_j softmax(conf)[j] F[c][j]).  Forward = ops.conf_softmax, so a train-mode
    conf is the eval kernel's bit for bit, and ops.conf_pool_cm; backward = ops.conf_pool_cm_backward.  Neither pass makes
    cat[F1, F2], the weighted product or anything else of F's size; only the gradients that are asked for are computed.  Saved:
    conf, w, F1, F2.  Every sum has a pinned order (include/dclnet_hip.h): the same inputs give the same bits.  CUDA tensors
    only."""

    @staticmethod
    def forward(ctx, logit1, logit2, F1, F2):
        if not (logit1.is_cuda and logit2.is_cuda and F1.is_cuda and F2.is_cuda):
            raise RuntimeError("ConfPoolFn (train_pool='fused') runs on the GPU only: got %s / %s / %s / %s tensors; the "
                               "'modules' composition serves CPU tensors" % (logit1.device, logit2.device, F1.device, F2.device))
        b = F1.shape[0]
        ctx.logit_shapes = (logit1.shape, logit2.shape)
        logit1, logit2 = _ops.N.f32c(logit1).reshape(b, -1), _ops.N.f32c(logit2).reshape(b, -1)
        F1, F2 = _ops.N.f32c(F1), _ops.N.f32c(F2)
        assert F1.dim() == 3 and F2.dim() == 3 and logit1.shape[1] == F1.shape[2] and logit2.shape[1] == F2.shape[2], \
            (tuple(logit1.shape), tuple(logit2.shape), tuple(F1.shape), tuple(F2.shape))
        conf, w, _ = _ops.conf_softmax(b, logit1.reshape(-1), logit2.reshape(-1))
        pooled = _ops.conf_pool_cm(w, F1, F2)
        ctx.save_for_backward(conf, w, F1, F2)
        return conf, pooled

    @staticmethod
    @once_differentiable
    def backward(ctx, g_conf, g_pooled):
        conf, w, F1, F2 = ctx.saved_tensors
        need = ctx.needs_input_grad
        need_logits, need_F = need[0] or need[1], need[2] or need[3]
        if not (need_logits or need_F):
            return None, None, None, None
        dl1, dl2, dF1, dF2 = _ops.conf_pool_cm_backward(conf, w, F1, F2, _ops.N.f32c(g_pooled), _ops.N.f32c(g_conf),
                                                        need_logits=need_logits, need_F=need_F)
        s1, s2 = ctx.logit_shapes
        return (dl1.view(s1) if need[0] else None, dl2.view(s2) if need[1] else None,
                dF1 if need[2] else None, dF2 if need[3] else None)


class BnReluFn(Function):
    """Train-mode nn.BatchNorm1d -> nn.ReLU on the (rows, C) feature matrix of a sparse tensor as one function on the library's
    own kernels (models/Modules.py: BasicBlock_SPCONV.norm_form = "fused"): apply(x (rows,C), gamma (C,), beta (C,),
    running_mean, running_var (C,) or None, momentum, eps) -> z (rows,C).  Forward = ops.bn_relu, which also updates the running
    statistics in place (buffers outside the graph; num_batches_tracked stays with the caller); backward =
    ops.bn_relu_backward.  Saved: x, gamma, beta, mean, invstd -- not y or z: the ReLU mask is recomputed from x by the same
    expression, hence with the same bits.  Every sum is float64 in a pinned order
    (include/dclnet_hip.h): the same inputs give the same bits.  Only the gradients that are asked for are computed.  CUDA
    tensors only.  A trailing relu=False gives the BatchNorm alone (the dense half's Conv -> ReLU -> BN fusers,
    train_dense="point_major"): the kernels take the flag, and nothing else changes."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, momentum, eps, relu=True):
        if not (x.is_cuda and gamma.is_cuda and beta.is_cuda):
            raise RuntimeError("BnReluFn (train_norm='fused') runs on the GPU only: got %s / %s / %s tensors; the 'modules' "
                               "composition serves CPU tensors" % (x.device, gamma.device, beta.device))
        x, gamma, beta = _ops.N.f32c(x), _ops.N.f32c(gamma), _ops.N.f32c(beta)
        ctx.relu = bool(relu)
        z, mean, invstd = _ops.bn_relu(x, gamma, beta, running_mean, running_var, momentum, eps, relu=ctx.relu)
        ctx.save_for_backward(x, gamma, beta, mean, invstd)
        return z

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, gamma, beta, mean, invstd = ctx.saved_tensors
        need = ctx.needs_input_grad
        need_x, need_affine = need[0], need[1] or need[2]
        if not (need_x or need_affine):
            return (None,) * 8
        g = _ops.N.f32c(g)
        dx, dgamma, dbeta = _ops.bn_relu_backward(x, gamma, beta, mean, invstd, g, relu=ctx.relu, need_x=need_x,
                                                  need_affine=need_affine)
        return dx, dgamma if need[1] else None, dbeta if need[2] else None, None, None, None, None, None


class ConfPoolPmFn(Function):
    """ConfPoolFn on point-major activations (train_dense="point_major"): apply(logit1 (b,n1) or (b,1,n1), logit2 (b,n2) or
    (b,1,n2), F1 (b n1, C), F2 (b n2, C)) -> (conf (b, n1+n2) = sigmoid(cat[logit1, logit2]), pooled (b,C) = sum_j
    softmax(conf)[j] F[j][c]); crop i owns rows i n .. i n + n - 1 of F.  Forward = ops.conf_softmax, so a train-mode conf is the
    eval kernel's bit for bit, and ops.conf_pool_pm; backward = ops.conf_pool_pm_backward.  Neither pass makes cat[F1, F2], the
    weighted product or anything else of F's size; only the gradients that are asked for are computed.  Saved: conf, w, F1, F2.
    Every sum has a pinned order (include/dclnet_hip.h): the same inputs give the same bits.  CUDA tensors only."""

    @staticmethod
    def forward(ctx, logit1, logit2, F1, F2):
        if not (logit1.is_cuda and logit2.is_cuda and F1.is_cuda and F2.is_cuda):
            raise RuntimeError("ConfPoolPmFn (train_dense='point_major') runs on the GPU only: got %s / %s / %s / %s tensors; the "
                               "'modules' composition serves CPU tensors" % (logit1.device, logit2.device, F1.device, F2.device))
        b = logit1.shape[0]
        ctx.logit_shapes = (logit1.shape, logit2.shape)
        logit1, logit2 = _ops.N.f32c(logit1).reshape(b, -1), _ops.N.f32c(logit2).reshape(b, -1)
        F1, F2 = _ops.N.f32c(F1), _ops.N.f32c(F2)
        assert F1.dim() == 2 and F2.dim() == 2 and F1.shape[0] == logit1.numel() and F2.shape[0] == logit2.numel(), \
            (tuple(logit1.shape), tuple(logit2.shape), tuple(F1.shape), tuple(F2.shape))
        conf, w, _ = _ops.conf_softmax(b, logit1.reshape(-1), logit2.reshape(-1))
        pooled = _ops.conf_pool_pm(w, F1, F2)
        ctx.save_for_backward(conf, w, F1, F2)
        return conf, pooled

    @staticmethod
    @once_differentiable
    def backward(ctx, g_conf, g_pooled):
        conf, w, F1, F2 = ctx.saved_tensors
        need = ctx.needs_input_grad
        need_logits, need_F = need[0] or need[1], need[2] or need[3]
        if not (need_logits or need_F):
            return None, None, None, None
        dl1, dl2, dF1, dF2 = _ops.conf_pool_pm_backward(conf, w, F1, F2, _ops.N.f32c(g_pooled), _ops.N.f32c(g_conf),
                                                        need_logits=need_logits, need_F=need_F)
        s1, s2 = ctx.logit_shapes
        return (dl1.view(s1) if need[0] else None, dl2.view(s2) if need[1] else None,
                dF1 if need[2] else None, dF2 if need[3] else None)


def _rows_dense(t):
    """a 2-D fp32 tensor whose rows are dense (a column block of a wider matrix stays a view; anything else is copied)"""
    t = t if t.dtype == torch.float32 else t.float()
    return t if t.stride(1) == 1 or t.shape[1] == 1 else t.contiguous()


class PointLinearFn(Function):
    """A per-point linear layer (a Conv1d / Conv3d with a 1-sized kernel) of the point-major dense half, trained on the library's
    own GEMM kernels: apply(x (M,K), W, bias, relu) -> (M,N), W the convolution's weight as registered, (N, K, 1...).  Two forms:
    (bias=None, relu=False), the layers a BatchNorm follows, and (bias, relu=True); a bias without the ReLU raises ValueError (no
    layer of this path has one).  Forward = ops.linear_dma(x, W^T, bias, relu); backward = ops.relu_bwd (mask + bias gradient),
    dW = ops.linear_wgrad(dz, x) viewed to W's shape, dx = ops.linear_dma(dz, W2d) with the registered matrix as the (K', N')
    operand, as RefinerShareFn does.  An optional fifth argument wgrad="split" makes dW = ops.linear_wgrad_split(dz, x) (the bf16
    matrix pipe, fp32-sized errors, its own pinned order) whatever the shape; outputs, dx and db keep their bits.  Otherwise the
    split-bf16 core takes no part, and the vendor library never does; a shape linear_dma cannot take
    (K and N in whole 32-chunks, 16-byte aligned operands and row pitches) raises ValueError.  x and the gradient may be column
    blocks of wider matrices.  Saved: x, W, and the output when relu is set.  Every reduction has a pinned order: the same inputs
    give the same gradients bit for bit.  Only the gradients that are asked for are computed."""

    @staticmethod
    def forward(ctx, x, W, bias, relu, wgrad="fp32"):
        relu = bool(relu)
        ctx.wgrad = _ops.check_linear_wgrad(wgrad, "wgrad")
        if (bias is None) == relu:
            raise ValueError("PointLinearFn has two forms, (bias=None, relu=False) and (bias, relu=True): got bias %s, relu=%s"
                             % ("None" if bias is None else "given", relu))
        for t in (x, W) + (() if bias is None else (bias,)):
            if not (t.is_cuda and t.dtype == torch.float32):
                raise RuntimeError("PointLinearFn runs on float32 CUDA tensors only (got %s on %s)" % (t.dtype, t.device))
        assert x.dim() == 2 and W.dim() >= 2 and W.numel() == W.shape[0] * W.shape[1] and W.shape[1] == x.shape[1], \
            (tuple(x.shape), tuple(W.shape))
        x = _rows_dense(x)
        W2d = W.contiguous().view(W.shape[0], W.shape[1])
        Wt = W2d.t().contiguous()
        if not _ops.linear_dma_ok(x, Wt):
            raise ValueError("PointLinearFn: linear_dma cannot take x %s (row pitch %d) with W %s: K must be a multiple of 32 and "
                             "the operands and their row pitches 16-byte aligned" % (tuple(x.shape), x.stride(0), tuple(W.shape)))
        if W2d.shape[0] % 32:
            raise ValueError("PointLinearFn: the input gradient runs linear_dma with N = %d as its inner size: N must be a "
                             "multiple of 32" % W2d.shape[0])
        y = _ops.linear_dma(x, Wt, None if bias is None else bias.contiguous(), relu)
        ctx.relu = relu
        ctx.save_for_backward(x, W, *((y,) if relu else ()))
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, W = ctx.saved_tensors[:2]
        need = ctx.needs_input_grad
        extra = (None,) * (len(need) - 4)                    # the optional trailing `wgrad`, when it was passed
        if not any(need[:3]):
            return (None, None, None, None) + extra
        g = _rows_dense(g)
        if g.data_ptr() % 16 or (g.shape[0] > 1 and g.stride(0) % 4):
            g = g.contiguous()
        db = None
        if ctx.relu:
            dz, db = _ops.relu_bwd(ctx.saved_tensors[2], g)
        else:
            dz = g
        dW = _ops.linear_wgrad_as(ctx.wgrad, dz, x).view_as(W) if need[1] else None
        dx = None
        if need[0]:
            W2d = W.contiguous().view(W.shape[0], W.shape[1])
            dx = _ops.linear_dma(dz, W2d)
        return (dx, dW, db if need[2] else None, None) + extra


class NarrowLinearFn(Function):
    """The last layer of a per-point head (1 or 3 output columns, at most ops.NARROW_MAX_N) of the point-major dense half on the
    library's own streaming kernels (models/DCL_Net.py: train_heads="kernels"; csrc/linear_narrow.hip): apply(x (M,K), W, bias)
    -> (M,N) = x W^T + bias, W the convolution's weight as registered, (N,K) or (N,K,1...), bias (N,) or None.  Forward =
    ops.linear_narrow, backward = ops.linear_narrow_backward: x may be a column block of a wider matrix and is read where it
    lies, no transposed copy of W is made, and the arriving gradient is made dense if it is a view.  Saved: x, W.  Every sum has
    a pinned order (include/dclnet_hip.h): the same inputs give the same bits.  Only the gradients that are asked for are
    computed.  CUDA tensors only."""

    @staticmethod
    def forward(ctx, x, W, bias):
        for t in (x, W) + (() if bias is None else (bias,)):
            if not (t.is_cuda and t.dtype == torch.float32):
                raise RuntimeError("NarrowLinearFn (train_heads='kernels') runs on float32 CUDA tensors only (got %s on %s); the "
                                   "'modules' composition serves CPU tensors" % (t.dtype, t.device))
        x = _rows_dense(x)
        y = _ops.linear_narrow(x, W, bias)
        ctx.save_for_backward(x, W)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, W = ctx.saved_tensors
        need = ctx.needs_input_grad
        if not any(need[:3]):
            return None, None, None
        dx, dW, db = _ops.linear_narrow_backward(x, W, g.contiguous(), need_x=need[0], need_w=need[1], need_b=need[2])
        return dx, None if dW is None else dW.view_as(W), db


class PoseHeadsFn(Function):
    """The rotation and the translation head (1024 -> 512 -> 128 -> 9 | 3, Conv1d -> ReLU -> Conv1d -> ReLU -> Conv1d each) on the b
    pooled rows of a training step, on the library's own kernels (models/DCL_Net.py, models/refiner.py: train_heads="kernels";
    csrc/pose_heads_grad.hip): apply(x (b,1024), rot W0, b0, W1, b1, W2, b2, trans W0, b0, W1, b1, W2, b2) -> (o9 (b,9), t3 (b,3)),
    the weights as registered, (out, in, 1), read in that layout: nothing is folded, transposed or cached, so an optimizer step is
    seen at once.  Forward = ops.pose_heads_train (three launches for both heads), backward = ops.pose_heads_train_backward (at
    most six).  Saved: x, the parameters, the hidden activations h1 (2,b,512), h2 (2,b,128); the ReLU masks are h > 0.  Every sum
    has a pinned order (include/dclnet_hip.h): the same inputs give the same bits, and a crop gives the same bits alone as inside
    a batch.  The train-mode values are NOT the eval kernels' bits (ops.pose_heads reads folded, transposed weights in other slice
    orders).  Only the gradients that are asked for are computed.  CUDA tensors only."""

    @staticmethod
    def forward(ctx, x, *params):
        if len(params) != 12:
            raise ValueError("PoseHeadsFn.apply(x, rot W0, b0, W1, b1, W2, b2, trans W0, ..., b2): got %d parameters" % len(params))
        for t in (x,) + params:
            if not (t.is_cuda and t.dtype == torch.float32):
                raise RuntimeError("PoseHeadsFn (train_heads='kernels') runs on float32 CUDA tensors only (got %s on %s); the "
                                   "'modules' composition serves CPU tensors" % (t.dtype, t.device))
        x = x.contiguous()
        o9, t3, h1, h2 = _ops.pose_heads_train(x, params)
        ctx.save_for_backward(x, h1, h2, *params)
        return o9, t3

    @staticmethod
    @once_differentiable
    def backward(ctx, g_o9, g_t3):
        x, h1, h2 = ctx.saved_tensors[:3]
        params = ctx.saved_tensors[3:]
        need = ctx.needs_input_grad
        if not any(need):
            return (None,) * 13
        dx, grads = _ops.pose_heads_train_backward(x, params, h1, h2, g_o9.contiguous(), g_t3.contiguous(), need_x=need[0],
                                                   need_params=tuple(need[1:]))
        return (dx,) + tuple(None if g is None else g.view_as(p) for g, p in zip(grads, params))
