"""The fused Chamfer distance (csrc/chamfer.hip: ops.chamfer / ops.chamfer_backward, autograd.ChamferFn, losses.cd_dis_fused,
losses(chamfer="fused")) against the literal reference formula (models/DCL_Net.py:307-311: norm of the (b,n,m,3) difference
tensor, min over either axis) evaluated in float64 on the CPU.

Bounds (eps = 2^-24, the fp32 unit round-off):
  values   |dist - dist64| <= 4 eps dist64: three rounded differences and the rounded sum of squares give <= 5 eps relative
           error on the squared distance, the square root halves that and adds one rounding, the minimum of the
           approximations keeps the bound.
  indices  not compared with the float64 argmin: the float64 distance to the returned index is <= (1 + 8 eps) x the float64
           minimum, for every point.
  backward max|d| <= 1e-5 max|grad64| per tensor against the two sums of include/dclnet_hip.h evaluated in float64 with the
           kernel's own indices (unit vectors carry a few eps, the ordered sums are a few tens of terms long)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
SHAPES = [(8, 1024, 1024), (3, 1000, 37), (2, 37, 1000), (1, 1, 1), (4, 12288, 2048)]


# ------------------------------------------------------------------------------------------------ float64 oracle (CPU)
def _nearest64(p, t):
    """p (b,n,3), t (b,m,3) float64 -> min_j |p_i - t_j| (b,n) and min_i (b,m): the literal formula, pred rows in chunks"""
    b, n, m = p.shape[0], p.shape[1], t.shape[1]
    d_pt, d_tp = torch.empty(b, n, dtype=torch.float64), torch.full((b, m), float("inf"), dtype=torch.float64)
    rows = max(1, (1 << 22) // m)
    for c in range(b):
        for s0 in range(0, n, rows):
            dis = torch.norm(p[c, s0:s0 + rows].unsqueeze(1) - t[c].unsqueeze(0), dim=2)
            d_pt[c, s0:s0 + rows] = dis.min(dim=1)[0]
            d_tp[c] = torch.minimum(d_tp[c], dis.min(dim=0)[0])
    return d_pt, d_tp


def _take(x, idx):
    return torch.gather(x, 1, idx.long().unsqueeze(2).expand(-1, -1, 3))


def _unit(a, c):
    d = a - c
    r = d.norm(dim=2, keepdim=True)
    return torch.where(r > 0, d / torch.where(r > 0, r, torch.ones_like(r)), torch.zeros_like(d))


def _grads64(p, t, idx_pt, idx_tp, g_pt, g_tp):
    """the two sums of the header in float64 with the given indices (no crop may be inactive)"""
    own_p = g_pt.unsqueeze(2) * _unit(p, _take(t, idx_pt))            # pair (i, idx_pt[i])
    own_t = g_tp.unsqueeze(2) * _unit(_take(p, idx_tp), t)            # pair (idx_tp[j], j)
    gp = own_p.clone().scatter_add_(1, idx_tp.long().unsqueeze(2).expand(-1, -1, 3), own_t)
    gt = (-own_t).scatter_add_(1, idx_pt.long().unsqueeze(2).expand(-1, -1, 3), -own_p)
    return gp, gt


def _clouds(b, n, m, seed, edits=False):
    g = torch.Generator().manual_seed(seed)
    p, t = torch.randn(b, n, 3, generator=g) * 0.05, torch.randn(b, m, 3, generator=g) * 0.05
    if edits:
        t[:, 100:104] = t[:, 200:204]          # duplicates: bit-equal squared distances, the lower index must win
        p[:, :16] = t[:, 5:21]                 # 16 pred points at distance exactly 0
    return p, t


def _check_values(p, t, out, tag):
    d_pt64, d_tp64 = _nearest64(p.double(), t.double())
    worst = {}
    for name, dist, idx, want, own, opp in (("pt", out[0], out[1], d_pt64, p, t), ("tp", out[2], out[3], d_tp64, t, p)):
        dist, idx = dist.cpu().double(), idx.cpu()
        assert int(idx.min()) >= 0 and int(idx.max()) < opp.shape[1]
        err = (dist - want).abs()
        rel = float((err / want.clamp_min(1e-300)).max())
        at_idx = (own.double() - _take(opp.double(), idx)).norm(dim=2)
        over = float((at_idx / want.clamp_min(1e-300))[want > 0].max()) - 1.0 if bool((want > 0).any()) else 0.0
        worst[name] = (rel / EPS, over / EPS)
        print("%s %s: max |dist - dist64| / dist64 = %.2f eps (bound 4), distance at the returned index over the minimum "
              "= 1 + %.2f eps (bound 8)" % (tag, name, rel / EPS, over / EPS))
        assert bool((err <= 4 * EPS * want).all()), (tag, name, rel / EPS)
        assert bool((at_idx <= (1 + 8 * EPS) * want).all()), (tag, name, over / EPS)
    return worst


# ------------------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("b,n,m", SHAPES)
def test_distances_and_indices_against_the_float64_formula(dcl, b, n, m):
    p, t = _clouds(b, n, m, seed=n + m)
    out = dcl.ops.chamfer(p.cuda(), t.cuda())
    assert out[0].shape == (b, n) and out[2].shape == (b, m) and out[1].dtype == torch.int32 and out[3].dtype == torch.int32
    _check_values(p, t, out, "%dx%dx%d" % (b, n, m))
    again = dcl.ops.chamfer(p.cuda(), t.cuda())
    assert all(torch.equal(a, c) for a, c in zip(out, again))


def test_ties_take_the_lowest_index_and_coincident_points_are_at_zero(dcl):
    b, n, m = SHAPES[0]
    p, t = _clouds(b, n, m, seed=7, edits=True)
    out = dcl.ops.chamfer(p.cuda(), t.cuda())
    _check_values(p, t, out, "ties")
    dist_pt, idx_pt, dist_tp, idx_tp = [o.cpu() for o in out]
    assert bool((dist_pt[:, :16] == 0).all()) and bool((idx_pt[:, :16] == torch.arange(5, 21, dtype=torch.int32)).all())
    assert bool((dist_tp[:, 5:21] == 0).all()) and bool((idx_tp[:, 5:21] == torch.arange(0, 16, dtype=torch.int32)).all())
    assert not bool(((idx_pt >= 200) & (idx_pt <= 203)).any())
    chose_dup = int(((idx_pt >= 100) & (idx_pt <= 103)).sum())
    print("pred points whose nearest target is one of the duplicated four: %d" % chose_dup)
    assert chose_dup > 0                                            # the tie rule was exercised


def test_inactive_crops_are_not_computed(dcl):
    b, n, m = SHAPES[0]
    p, t = _clouds(b, n, m, seed=7, edits=True)
    p, t = p.cuda(), t.cuda()
    active = (torch.arange(b) % 2 == 0).int().cuda()
    full, masked = dcl.ops.chamfer(p, t), dcl.ops.chamfer(p, t, active)
    on, off = active.bool(), ~active.bool()
    for f, k in zip(full, masked):
        assert torch.equal(f[on], k[on])
    assert bool((masked[0][off] == 0).all()) and bool((masked[2][off] == 0).all())
    assert bool((masked[1][off] == -1).all()) and bool((masked[3][off] == -1).all())
    g = torch.Generator().manual_seed(3)
    g_pt, g_tp = torch.randn(b, n, generator=g).cuda(), torch.randn(b, m, generator=g).cuda()
    gp_full, gt_full = dcl.ops.chamfer_backward(p, t, full[1], full[3], g_pt, g_tp)
    gp, gt = dcl.ops.chamfer_backward(p, t, masked[1], masked[3], g_pt, g_tp, active)
    assert torch.equal(gp[on], gp_full[on]) and torch.equal(gt[on], gt_full[on])
    assert bool((gp[off] == 0).all()) and bool((gt[off] == 0).all())


# ------------------------------------------------------------------------------------------------------------ backward
@pytest.mark.parametrize("b,n,m", SHAPES)
def test_backward_against_the_two_sums_in_float64(dcl, b, n, m):
    edits = (b, n, m) == SHAPES[0]
    p, t = _clouds(b, n, m, seed=11 + n + m, edits=edits)
    g = torch.Generator().manual_seed(5)
    g_pt, g_tp = torch.randn(b, n, generator=g), torch.randn(b, m, generator=g)
    pc, tc, g_ptc, g_tpc = p.cuda(), t.cuda(), g_pt.cuda(), g_tp.cuda()
    _, idx_pt, _, idx_tp = dcl.ops.chamfer(pc, tc)
    gp, gt = dcl.ops.chamfer_backward(pc, tc, idx_pt, idx_tp, g_ptc, g_tpc)
    want_p, want_t = _grads64(p.double(), t.double(), idx_pt.cpu(), idx_tp.cpu(), g_pt.double(), g_tp.double())
    longest = max(int(torch.stack([torch.bincount(r.long(), minlength=1).max() for r in idx_pt.cpu()]).max()),
                  int(torch.stack([torch.bincount(r.long(), minlength=1).max() for r in idx_tp.cpu()]).max()))
    for name, got, want in (("grad_pred", gp, want_p), ("grad_target", gt, want_t)):
        assert bool(torch.isfinite(got).all()), name
        err, scale = float((got.cpu().double() - want).abs().max()), float(want.abs().max())
        print("%dx%dx%d %s: max|d| = %.3g = %.3g of max|grad64| (bound 1e-5); longest incoming list %d"
              % (b, n, m, name, err, err / max(scale, 1e-300), longest))
        assert err <= 1e-5 * scale, (name, err, scale)
    if edits:                                                        # u = 0 at distance 0: only the incoming terms remain
        assert bool(torch.isfinite(gp[:, :16]).all())
        assert float((gp[:, :16].cpu().double() - want_p[:, :16]).abs().max()) <= 1e-5 * float(want_p.abs().max())
    # a gradient that is not asked for is skipped; the other one does not change
    only_p, none_t = dcl.ops.chamfer_backward(pc, tc, idx_pt, idx_tp, g_ptc, g_tpc, need_target=False)
    none_p, only_t = dcl.ops.chamfer_backward(pc, tc, idx_pt, idx_tp, g_ptc, g_tpc, need_pred=False)
    assert none_t is None and none_p is None and torch.equal(only_p, gp) and torch.equal(only_t, gt)
    # the same bits call after call
    gp2, gt2 = dcl.ops.chamfer_backward(pc, tc, idx_pt, idx_tp, g_ptc, g_tpc)
    assert torch.equal(gp2, gp) and torch.equal(gt2, gt)


def _runner_up_gap(p, t):
    """smallest relative gap between the nearest and the second nearest distance over both directions, float64"""
    dis = torch.norm(p.double().unsqueeze(2) - t.double().unsqueeze(1), dim=3)
    gap = float("inf")
    for dim in (2, 1):
        two = torch.topk(dis, 2, dim=dim, largest=False)[0]
        a, c = two.select(dim, 0), two.select(dim, 1)
        gap = min(gap, float(((c - a) / a).min()))
    return gap


def test_autograd_function_against_float64_autograd(dcl):
    b, n = 4, 256
    p, t = _clouds(b, n, n, seed=21)
    gap = _runner_up_gap(p, t)
    print("smallest nearest / runner-up gap: %.3g (needs > 1e-5)" % gap)
    assert gap > 1e-5                                                # fp32 and float64 pick the same neighbours
    g = torch.Generator().manual_seed(6)
    w_pt, w_tp = torch.randn(b, n, generator=g), torch.randn(b, n, generator=g)
    p64, t64 = p.double().requires_grad_(True), t.double().requires_grad_(True)
    dis = torch.norm(p64.unsqueeze(2) - t64.unsqueeze(1), dim=3)
    ((dis.min(dim=2)[0] * w_pt.double()).sum() + (dis.min(dim=1)[0] * w_tp.double()).sum()).backward()
    for target_grad in (False, True):
        pc, tc = p.cuda().requires_grad_(True), t.cuda().requires_grad_(target_grad)
        d_pt, d_tp = dcl.autograd.ChamferFn.apply(pc, tc, None)
        ((d_pt * w_pt.cuda()).sum() + (d_tp * w_tp.cuda()).sum()).backward()
        pairs = [("pred", pc.grad, p64.grad)] + ([("target", tc.grad, t64.grad)] if target_grad else [])
        assert target_grad or tc.grad is None
        for name, got, want in pairs:
            err, scale = float((got.cpu().double() - want).abs().max()), float(want.abs().max())
            print("ChamferFn d/d%s: max|d| = %.3g of max|grad64| (bound 1e-5)" % (name, err / scale))
            assert err <= 1e-5 * scale, name


# -------------------------------------------------------------------------------------------------------- loss modules
def _rand_rot(g, b):
    q, _ = torch.linalg.qr(torch.randn(b, 3, 3, generator=g))
    return q


def _loss_case(b=4, n=256, seed=0):
    """tests/test_losses.py's recipe"""
    g = torch.Generator().manual_seed(seed)
    tmp, inp = torch.randn(b, n, 3, generator=g) * 0.05, torch.randn(b, n, 3, generator=g) * 0.05
    pred = {"rot_pred": _rand_rot(g, b), "trans_pred": torch.randn(b, 3, generator=g) * 0.01,
            "sym_flag": torch.tensor([0.0, 1.0, 0.0, 1.0][:b]), "conf": torch.rand(b, 2 * n, generator=g) * 0.8 + 0.1,
            "Xo_pred": torch.randn(b, n, 3, generator=g) * 0.05, "Yc_pred": torch.randn(b, n, 3, generator=g) * 0.05}
    gt = {"rot_gt": _rand_rot(g, b), "trans_gt": torch.randn(b, 3, generator=g) * 0.01, "points_tmp": tmp, "points_inp": inp}
    pr = {"rot_pred": _rand_rot(g, b), "trans_pred": torch.randn(b, 3, generator=g) * 0.01}
    return pred, gt, pr


def _cd_literal(pred, target):
    dis = torch.norm(pred.unsqueeze(2) - target.unsqueeze(1), dim=3)
    return 0.5 * (torch.min(dis, 2)[0] + torch.min(dis, 1)[0])


def _l2(a, c):
    return torch.norm(a - c, dim=2)


def _literal_loss(pred, gt):
    """models/DCL_Net.py:264-304 written out (any dtype)"""
    R, t, s = pred["rot_pred"], pred["trans_pred"], pred["sym_flag"].unsqueeze(1)
    Rg, tg, tmp, inp = gt["rot_gt"], gt["trans_gt"], gt["points_tmp"], gt["points_inp"]
    pp = torch.bmm(tmp, R.transpose(1, 2)) + t.unsqueeze(1)
    pg = torch.bmm(tmp, Rg.transpose(1, 2)) + tg.unsqueeze(1)
    loss_pose = ((1 - s) * _l2(pp, pg) + s * _cd_literal(pp, pg)).mean(dim=1).mean()
    Xo, Yc = pred["Xo_pred"], pred["Yc_pred"]
    ip, ig = torch.bmm(inp - t.unsqueeze(1), R).detach(), torch.bmm(inp - tg.unsqueeze(1), Rg).detach()
    lXo = (1 - s) * _l2(Xo, ig) + 0.5 * s * (_cd_literal(Xo, tmp) + _l2(Xo, ip))
    lYc = (1 - s) * _l2(Yc, pg) + 0.5 * s * (_cd_literal(Yc, pg) + _l2(Yc, pp.detach()))
    lconf = torch.mean(torch.cat([lXo, lYc], dim=1).detach() * pred["conf"] - 0.01 * torch.log(pred["conf"]))
    return loss_pose + 5 * lXo.mean() + lYc.mean() + lconf


def _literal_refiner_loss(pr, t_cur, R_cur, tmp, s, gt):
    """models/refiner.py:101-125 written out"""
    pd = torch.bmm(tmp, pr["rot_pred"].transpose(1, 2)) + pr["trans_pred"].unsqueeze(1)
    pg = torch.bmm(tmp, gt["rot_gt"].transpose(1, 2)) + gt["trans_gt"].unsqueeze(1)
    rf = torch.bmm(pd, R_cur.transpose(1, 2)) + t_cur.unsqueeze(1)
    s = s.unsqueeze(1)
    return ((1 - s) * _l2(rf, pg) + s * _cd_literal(rf, pg)).mean(dim=1).mean()


def _leaves(d, names, f):
    """a copy of dict d through f with the named entries made leaves that require grad"""
    out = {k: f(v) for k, v in d.items()}
    for k in names:
        out[k] = out[k].detach().clone().requires_grad_(True)
    return out


LOSS_LEAVES = ("Xo_pred", "Yc_pred", "rot_pred", "trans_pred", "conf")


def test_loss_modules_with_the_fused_chamfer_against_the_float64_literal_loss(dcl):
    pred, gt, pr = _loss_case()
    # precondition, before any GPU work: at every point of the three Chamfer pairs (and the refiner's) the runner-up is more
    # than 1e-5 (relative) behind the nearest -- 20 times the 8 eps at which fp32 could pick another neighbour
    R, t, tmp = pred["rot_pred"].double(), pred["trans_pred"].double(), gt["points_tmp"].double()
    pp = torch.bmm(tmp, R.transpose(1, 2)) + t.unsqueeze(1)
    pg = torch.bmm(tmp, gt["rot_gt"].double().transpose(1, 2)) + gt["trans_gt"].double().unsqueeze(1)
    pd = torch.bmm(tmp, pr["rot_pred"].double().transpose(1, 2)) + pr["trans_pred"].double().unsqueeze(1)
    rf = torch.bmm(pd, R.transpose(1, 2)) + t.unsqueeze(1)
    gaps = [_runner_up_gap(a, c) for a, c in ((pp, pg), (pred["Xo_pred"], tmp), (pred["Yc_pred"], pg), (rf, pg))]
    print("nearest / runner-up gaps (pose, Xo, Yc, refiner): %s (need > 1e-5)" % " ".join("%.3g" % v for v in gaps))
    assert min(gaps) > 1e-5

    dbl, cu = (lambda v: v.double()), (lambda v: v.cuda())
    p64, gt64 = _leaves(pred, LOSS_LEAVES, dbl), {k: v.double() for k, v in gt.items()}
    want = _literal_loss(p64, gt64)
    want.backward()
    pcu, gtcu = _leaves(pred, LOSS_LEAVES, cu), {k: v.cuda() for k, v in gt.items()}
    out = dcl.DCL_Net.losses(None, chamfer="fused")(pcu, gtcu)
    out["loss_all"].backward()
    d = abs(float(out["loss_all"]) - float(want))
    print("losses(chamfer='fused'): |loss_all - float64 literal| = %.3g (bound 1e-6)" % d)
    assert d <= 1e-6
    for k in LOSS_LEAVES:
        err, scale = float((pcu[k].grad.cpu().double() - p64[k].grad).abs().max()), float(p64[k].grad.abs().max())
        print("  d loss_all / d %s: max|d| = %.3g of max|grad64| (bound 1e-5)" % (k, err / scale))
        assert err <= 1e-5 * scale, k
    # against the default (chunked) module on the same inputs
    base = dcl.DCL_Net.losses(None)({k: v.detach() for k, v in pcu.items()}, gtcu)
    for k in ("loss_all", "loss_pose", "loss_Xo", "loss_Yc", "loss_conf"):
        dk = abs(float(base[k]) - float(out[k]))
        print("  fused vs default %s: %.3g" % (k, dk))
        assert dk <= 1e-6, k

    # the refiner loss
    r64 = _leaves(pr, ("rot_pred", "trans_pred"), dbl)
    want_r = _literal_refiner_loss(r64, t, R, tmp, pred["sym_flag"].double(), gt64)
    want_r.backward()
    rcu = _leaves(pr, ("rot_pred", "trans_pred"), cu)
    args = (pred["trans_pred"].cuda(), pred["rot_pred"].cuda(), gt["points_tmp"].cuda(), pred["sym_flag"].cuda(), gtcu)
    lo = dcl.refiner.losses_refiner(None, chamfer="fused")(rcu, *args)
    lo["loss_all"].backward()
    d = abs(float(lo["loss_all"]) - float(want_r))
    print("losses_refiner(chamfer='fused'): |loss_all - float64 literal| = %.3g (bound 1e-6)" % d)
    assert d <= 1e-6
    for k in ("rot_pred", "trans_pred"):
        err, scale = float((rcu[k].grad.cpu().double() - r64[k].grad).abs().max()), float(r64[k].grad.abs().max())
        print("  d loss_all / d %s: max|d| = %.3g of max|grad64| (bound 1e-5)" % (k, err / scale))
        assert err <= 1e-5 * scale, k
    base_r = dcl.refiner.losses_refiner(None)({k: v.detach() for k, v in rcu.items()}, *args)
    assert abs(float(base_r["loss_all"]) - float(lo["loss_all"])) <= 1e-6


def test_full_training_step_with_the_fused_chamfer(dcl):
    """tests/test_losses.py's three-iteration Adam loop with losses(None, chamfer='fused')"""
    n = 256
    net = dcl.DCL_Net.Network(dcl.synth.default_cfg(n, n), mode="train")
    net.load_state_dict(dcl.synth.synth_state_dict(net, 1))
    net = net.cuda().train()
    crit = dcl.DCL_Net.losses(None, chamfer="fused")
    data = dcl.synth.make_batch(4, n, n)
    data["flags"] = torch.tensor([0.0, 1.0, 0.0, 1.0])
    opt = torch.optim.Adam(net.parameters(), lr=1e-4)
    vals = []
    for _ in range(3):
        opt.zero_grad()
        pred = net(data)
        loss = crit(pred, data["labels"])
        loss["loss_all"].backward()
        bad = [k for k, p in net.named_parameters() if p.grad is None or not torch.isfinite(p.grad).all()]
        assert bad == []
        opt.step()
        vals.append(float(loss["loss_all"].detach()))
    assert np.isfinite(vals).all()


def test_peak_memory_of_the_fused_chamfer_stays_far_below_one_map(dcl):
    """forward + backward of cd_dis_fused at the shipped batch shape: everything it allocates is O(b (n + m))"""
    b, n = 32, 1024
    p, t = _clouds(b, n, n, seed=2)
    p, t = p.cuda().requires_grad_(True), t.cuda()
    w = torch.randn(b, n, generator=torch.Generator().manual_seed(1)).cuda()
    one_map = b * n * n * 4
    crit = dcl.DCL_Net.losses

    def peak(fn):
        p.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        (fn(p, t) * w).sum().backward()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    fused = peak(crit.cd_dis_fused)
    chunked = peak(crit.CD_Dis)
    print("peak memory above the inputs, forward + backward at 32 x 1024 x 1024: fused %.2f MB = %.4f maps (bound 0.1), "
          "chunked %.1f MB = %.2f maps" % (fused / 1e6, fused / one_map, chunked / 1e6, chunked / one_map))
    assert fused < 0.1 * one_map
