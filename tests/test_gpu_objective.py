"""The training objective on the device (csrc/objective.hip): every kernel against its host twin -- bit for bit where no
transcendental enters (the host and the device compile both take correctly rounded sqrtf and division, and the routines
are the same text under -ffp-contract=off), within the host test's bounds where logf does -- twice for equal bits, and the
loss modules with objective="fused" against the module composition and a float64 twin.  tests/objective_cases.py holds the
cases, the references and the bounds."""
import math

import pytest
import torch

import objective_cases as OC

pytestmark = pytest.mark.gpu
EPS = OC.EPS
GPU_SHAPES = OC.SHAPES + [(2, 2620)]                     # + the refiner's cloud


def _cuda(c):
    return OC.to(c, "cuda")


def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    return torch.equal(a.cpu(), b.cpu())


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("b,n", GPU_SHAPES)
def test_rigid_points_kernels_equal_their_host_twins_bit_for_bit(dcl, b, n, inverse):
    c = OC.case(b, n, "mixed")
    g = _cuda(c)
    out = dcl.ops.rigid_points(g["tmp"], g["R"], g["t"], inverse)
    assert _same(out, dcl.ops.rigid_points_host(c["tmp"], c["R"], c["t"], inverse))
    want = dcl.ops.rigid_points_backward_host(c["tmp"], c["R"], c["t"], inverse, c["g_out"], need_pts=True)
    got = dcl.ops.rigid_points_backward(g["tmp"], g["R"], g["t"], inverse, g["g_out"], need_pts=True)
    again = dcl.ops.rigid_points_backward(g["tmp"], g["R"], g["t"], inverse, g["g_out"], need_pts=True)
    for name, w, x, y in zip(("g_R", "g_t", "g_pts"), want, got, again):
        assert _same(x, w), name
        assert _same(x, y), name + " differs between two calls"
    assert _same(out, dcl.ops.rigid_points(g["tmp"], g["R"], g["t"], inverse))
    lean = dcl.ops.rigid_points_backward(g["tmp"], g["R"], g["t"], inverse, g["g_out"], need_pts=False)
    assert lean[2] is None and _same(lean[0], want[0]) and _same(lean[1], want[1])


@pytest.mark.parametrize("b,n,kind", [(b, n, k) for b, n in OC.SHAPES for k in OC.SYM_KINDS] + [(2, 2620, "mixed")])
def test_objective_kernels_against_their_host_twins(dcl, b, n, kind):
    """bit for bit: L, loss_pose, loss_Xo, loss_Yc, g_posed, g_Xo, g_Yc and the Chamfer-distance gradients.  Within the host
    test's bounds against float64: loss_conf and loss_all (logf) and g_conf.  The same call twice: equal bits everywhere."""
    c = OC.case(b, n, kind)
    g = _cuda(c)
    args, kw = OC.objective_args(c)
    gargs, gkw = OC.objective_args(g)
    packed_h, L_h = dcl.ops.pose_objective_host(*args, **kw)
    packed, L = dcl.ops.pose_objective(*gargs, **gkw)
    packed2, L2 = dcl.ops.pose_objective(*gargs, **gkw)
    assert _same(L, L_h) and _same(packed[:3], packed_h[:3])
    assert _same(L, L2) and _same(packed, packed2)
    ref = OC.forward64(c)["packed"]
    err = (packed.cpu().double() - ref).abs() / ref.abs().clamp_min(1e-300)
    print("b=%d n=%d %s: device scalar errors / eps = %s" % (b, n, kind, [round(float(e) / EPS, 2) for e in err]))
    assert bool((err <= OC.scalar_bound(b, n)).all())
    for up in ("all", "random"):
        g_up = OC.upstream(c, up)
        want = dcl.ops.pose_objective_backward_host(*OC.backward_args(c, g_up, L_h)[0], **OC.backward_args(c, g_up, L_h)[1])
        bargs, bkw = OC.backward_args(g, g_up.cuda(), L)
        got = dcl.ops.pose_objective_backward(*bargs, **bkw)
        again = dcl.ops.pose_objective_backward(*bargs, **bkw)
        for i, name in enumerate(("g_posed", "g_Xo", "g_Yc")):
            assert _same(got[i], want[i]), (name, up)
        for i in (4, 5, 6):
            assert _same(got[i][0], want[i][0]) and _same(got[i][1], want[i][1]), ("cd gradient", i, up)
        w = OC.weights_abs(g_up, b, n)
        L64, c64 = L_h.double(), c["conf"].double()
        conf64 = g_up.double()[3:].sum() / (2 * b * n) * (L64 - 0.01 / c64)
        assert bool(((got[3].cpu().double() - conf64).abs() <= 8 * EPS * w["conf"] * (L64.abs() + 0.01 / c64)).all())
        for x, y in zip(got[:4] + got[4] + got[5] + got[6], again[:4] + again[4] + again[5] + again[6]):
            assert _same(x, y), "two backward calls differ"
    # the pose-only form
    p_h, _ = dcl.ops.pose_objective_host(*OC.objective_args(c, full=False)[0])
    p_d, none = dcl.ops.pose_objective(*OC.objective_args(g, full=False)[0])
    assert none is None and _same(p_d, p_h) and _same(p_d[0], packed[0])
    g_up = OC.upstream(c, "random")
    want = dcl.ops.pose_objective_backward_host(g_up, c["posed"], c["posed_gt"], c["sym"])
    got = dcl.ops.pose_objective_backward(g_up.cuda(), g["posed"], g["posed_gt"], g["sym"])
    assert _same(got[0], want[0]) and _same(got[4][0], want[4][0]) and _same(got[4][1], want[4][1]) and got[1] is None


# ---- the loss modules ---------------------------------------------------------------------------------------------------
def _gather(cloud, idx):
    return torch.gather(cloud, 1, idx.clamp_min(0).long().unsqueeze(2).expand(-1, -1, 3))


def _cd64(pred, target, idx_pt, idx_tp, live):
    """the Chamfer term in float64 through the nearest-neighbour indices of the fp32 clouds"""
    pt = torch.norm(pred - _gather(target, idx_pt), dim=2)
    tp = torch.norm(_gather(pred, idx_tp) - target, dim=2)
    return 0.5 * (pt + tp) * live


def _indices(dcl, which, case_, active):
    """ops.chamfer's indices on the fp32 clouds of every Chamfer call of the module; asserts the input condition: in float64
    every point's nearest and second-nearest distances differ by >= 1e-5 relative, and the indices are the float64 argmins"""
    out = []
    for pred, target in OC.chamfer_pairs64(which, case_):
        gap, ipt64, itp64 = OC.nearest_gap(pred, target)
        assert gap >= OC.GAP, gap
        _, ipt, _, itp = dcl.ops.chamfer(pred.float().cuda().contiguous(), target.float().cuda().contiguous(), active)
        ipt, itp, live = ipt.cpu(), itp.cpu(), active.cpu().bool()
        assert torch.equal(ipt[live].long(), ipt64[live]) and torch.equal(itp[live].long(), itp64[live])
        assert bool((ipt[~live] == -1).all())
        out.append((ipt, itp))
    return out


def _compare(tag, ref_vals, ref_grads, fused, module):
    """err_fused <= max(2 err_module, 1e-6 max|ref64|) for every value and gradient: both are fp32 evaluations of one
    formula in different summation orders; the floor is there because the module's error can happen to be tiny"""
    for name in ref_vals:
        r = ref_vals[name].detach()
        ef = float((fused[0][name].detach().cpu().double() - r).abs().max())
        em = float((module[0][name].detach().cpu().double() - r).abs().max())
        print("%s %-10s ref %.9g  err fused %.3g  module %.3g" % (tag, name, float(r), ef, em))
        assert ef <= max(2 * em, 1e-6 * float(r.abs().max())), (name, ef, em)
    for name, r in ref_grads.items():
        ef = float((fused[1][name].cpu().double() - r).abs().max())
        em = float((module[1][name].cpu().double() - r).abs().max())
        print("%s d/d%-10s max|ref| %.3g  err fused %.3g  module %.3g" % (tag, name, float(r.abs().max()), ef, em))
        assert ef <= max(2 * em, 1e-6 * float(r.abs().max())), (name, ef, em)


LEAVES = ("rot_pred", "trans_pred", "Xo_pred", "Yc_pred", "conf")


def test_losses_fused_objective_against_the_module_and_float64(dcl):
    case_ = OC.module_case("losses")
    pred, gt = case_
    sym = pred["sym_flag"]
    idx = _indices(dcl, "losses", case_, (sym != 0).int().cuda())
    # float64 twin
    p64 = {k: (v.double().requires_grad_() if k in LEAVES else v.double()) for k, v in pred.items()}
    g64 = {k: v.double() for k, v in gt.items()}
    s, live = sym.double().unsqueeze(1), (sym != 0).double().unsqueeze(1)
    R, t, tmp, inp = p64["rot_pred"], p64["trans_pred"], g64["points_tmp"], g64["points_inp"]
    L2 = lambda a, c: torch.norm(a - c, dim=2)                                               # noqa: E731
    posed = torch.bmm(tmp, R.transpose(1, 2)) + t.unsqueeze(1)
    posed_gt = torch.bmm(tmp, g64["rot_gt"].transpose(1, 2)) + g64["trans_gt"].unsqueeze(1)
    cano_pred = torch.bmm(inp - t.unsqueeze(1), R).detach()
    cano_gt = torch.bmm(inp - g64["trans_gt"].unsqueeze(1), g64["rot_gt"])
    Xo, Yc = p64["Xo_pred"], p64["Yc_pred"]
    pose = ((1 - s) * L2(posed, posed_gt) + s * _cd64(posed, posed_gt, *idx[0], live)).mean(dim=1).mean()
    LXo = (1 - s) * L2(Xo, cano_gt) + 0.5 * s * (_cd64(Xo, tmp, *idx[1], live) + L2(Xo, cano_pred))
    LYc = (1 - s) * L2(Yc, posed_gt) + 0.5 * s * (_cd64(Yc, posed_gt, *idx[2], live) + L2(Yc, posed.detach()))
    conf = torch.mean(torch.cat([LXo, LYc], dim=1).detach() * p64["conf"] - 0.01 * torch.log(p64["conf"]))
    ref = {"loss_pose": pose, "loss_Xo": LXo.mean(), "loss_Yc": LYc.mean(), "loss_conf": conf}
    ref["loss_all"] = pose + 5 * ref["loss_Xo"] + ref["loss_Yc"] + conf
    ref["loss_all"].backward()
    ref_grads = {k: p64[k].grad for k in LEAVES}

    def run(crit):
        p = {k: (v.cuda().requires_grad_() if k in LEAVES else v.cuda()) for k, v in pred.items()}
        out = crit(p, {k: v.cuda() for k, v in gt.items()})
        out["loss_all"].backward()
        return out, {k: p[k].grad for k in LEAVES}

    fused = run(dcl.DCL_Net.losses(None, chamfer="fused", objective="fused"))
    module = run(dcl.DCL_Net.losses(None, chamfer="fused"))
    assert set(fused[0]) == set(module[0]) == set(ref)
    _compare("losses", ref, ref_grads, fused, module)
    again = run(dcl.DCL_Net.losses(None, objective="fused"))       # whatever chamfer= says; and the same bits
    assert all(_same(again[0][k], fused[0][k]) for k in ref) and all(_same(again[1][k], fused[1][k]) for k in LEAVES)


def test_refiner_fused_objective_against_the_module_and_float64(dcl):
    case_ = OC.module_case("refiner")
    pred, extra, gt = case_
    sym = extra["sym_flag"]
    (ipt, itp), = _indices(dcl, "refiner", case_, (sym != 0).int().cuda())
    p64 = {k: v.double().requires_grad_() for k, v in pred.items()}
    e64, g64 = {k: v.double() for k, v in extra.items()}, {k: v.double() for k, v in gt.items()}
    s, live = sym.double().unsqueeze(1), (sym != 0).double().unsqueeze(1)
    delta = torch.bmm(e64["points_tmp"], p64["rot_pred"].transpose(1, 2)) + p64["trans_pred"].unsqueeze(1)
    refined = torch.bmm(delta, e64["rot_cur"].transpose(1, 2)) + e64["trans_cur"].unsqueeze(1)
    posed_gt = torch.bmm(e64["points_tmp"], g64["rot_gt"].transpose(1, 2)) + g64["trans_gt"].unsqueeze(1)
    pose = ((1 - s) * torch.norm(refined - posed_gt, dim=2) + s * _cd64(refined, posed_gt, ipt, itp, live)).mean(dim=1).mean()
    pose.backward()
    ref, ref_grads = {"loss_pose": pose, "loss_all": pose}, {k: p64[k].grad for k in pred}

    def run(crit):
        p = {k: v.cuda().requires_grad_() for k, v in pred.items()}
        e = {k: v.cuda() for k, v in extra.items()}
        out = crit(p, e["trans_cur"], e["rot_cur"], e["points_tmp"], e["sym_flag"], {k: v.cuda() for k, v in gt.items()})
        out["loss_all"].backward()
        return out, {k: p[k].grad for k in pred}

    fused = run(dcl.refiner.losses_refiner(None, chamfer="fused", objective="fused"))
    module = run(dcl.refiner.losses_refiner(None, chamfer="fused"))
    assert set(fused[0]) == set(module[0]) == {"loss_pose", "loss_all"}
    _compare("refiner", ref, ref_grads, fused, module)


def test_the_five_values_are_views_of_one_packed_tensor(dcl):
    pred, gt = OC.module_case("losses")
    gt = {k: v.cuda() for k, v in gt.items()}
    crit = dcl.DCL_Net.losses(None, objective="fused")

    def fresh():
        p = {k: (v.cuda().requires_grad_() if k in LEAVES else v.cuda()) for k, v in pred.items()}
        return p, crit(p, gt)

    p, out = fresh()
    assert crit.packed.shape == (5,) and crit.packed.is_cuda
    base = crit.packed.untyped_storage().data_ptr()
    keys = ("loss_pose", "loss_Xo", "loss_Yc", "loss_conf", "loss_all")
    assert all(out[k].dim() == 0 and out[k].untyped_storage().data_ptr() == base for k in keys)
    assert crit.packed.tolist() == [float(out[k].detach()) for k in keys]
    out["loss_all"].backward()
    assert all(p[k].grad is not None and bool(torch.isfinite(p[k].grad).all()) and bool(p[k].grad.any()) for k in LEAVES)
    p, out = fresh()
    out["loss_pose"].backward()
    assert bool(p["rot_pred"].grad.any()) and bool(p["trans_pred"].grad.any())
    for k in ("Xo_pred", "Yc_pred", "conf"):
        assert p[k].grad is None or not bool(p[k].grad.any()), k
    with pytest.raises(ValueError, match="n == m"):
        crit(p, dict(gt, points_inp=gt["points_inp"][:, :100].contiguous()))


def test_full_training_step_with_the_fused_objective(dcl):
    """Network(mode='train') + losses(objective='fused'): every parameter gets a finite gradient, three steps give finite
    losses, and the step-1 loss_all agrees with the module composition on the same predictions"""
    n = 256
    net = dcl.DCL_Net.Network(dcl.synth.default_cfg(n, n), mode="train")
    net.load_state_dict(dcl.synth.synth_state_dict(net, 1))
    net = net.cuda().train()
    crit, crit_module = dcl.DCL_Net.losses(None, objective="fused"), dcl.DCL_Net.losses(None)
    data = dcl.synth.make_batch(4, n, n)
    data["flags"] = torch.tensor([0.0, 1.0, 0.0, 1.0])
    opt = torch.optim.Adam(net.parameters(), lr=1e-4)
    vals = []
    for step in range(3):
        opt.zero_grad()
        pred = net(data)
        loss = crit(pred, data["labels"])
        if step == 0:
            with torch.no_grad():
                want = float(crit_module(pred, data["labels"])["loss_all"])
            got = float(loss["loss_all"].detach())
            print("step-1 loss_all: fused %.9g, module %.9g" % (got, want))
            assert abs(got - want) <= 1e-5 * max(1.0, abs(want))
        loss["loss_all"].backward()
        bad = [k for k, p in net.named_parameters() if p.grad is None or not torch.isfinite(p.grad).all()]
        assert bad == []
        opt.step()
        vals.append(crit.packed.tolist())
    assert all(math.isfinite(v) for row in vals for v in row)
