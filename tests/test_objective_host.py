"""The host twins of the training objective (dcl_rigid_points*_host, dcl_pose_objective_*_host: the kernels' own routines from
csrc/objective.h compiled for the host, in the kernels' summation order) against float64 evaluations of the same formulas on
the same fp32 inputs.  No GPU.  tests/objective_cases.py holds the cases, the references and the derivation of the bounds."""
import math

import pytest
import torch

import objective_cases as OC

EPS = OC.EPS


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("b,n", OC.SHAPES)
def test_rigid_points_host_against_float64(dcl, b, n, inverse):
    """|out - out64| <= 4.1 eps (|R| |p| + |t|) component-wise (forward form: a product and three roundings behind it), and
    4.1 eps |R^T| (|p| + |t|) for the inverse form (the difference, the product, two fma roundings)"""
    c = OC.case(b, n, "mixed")
    got = dcl.ops.rigid_points_host(c["tmp"], c["R"], c["t"], inverse).double()
    want = OC.rigid64(c["tmp"], c["R"], c["t"], inverse)
    p, R, t = c["tmp"].double().abs(), c["R"].double().abs(), c["t"].double().abs()
    if inverse:
        bound = 4.1 * EPS * torch.bmm(p + t.unsqueeze(1), R)
    else:
        bound = 4.1 * EPS * (torch.bmm(p, R.transpose(1, 2)) + t.unsqueeze(1))
    assert bool(((got - want).abs() <= bound).all()), float(((got - want).abs() / bound).max())


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("b,n", OC.SHAPES)
def test_rigid_points_backward_host_against_float64(dcl, b, n, inverse):
    """g_R, g_t within (ceil(n/256) + 10) eps sum_i |g_i| |p_i| component-wise (objective_cases.rigid_grad_bounds); g_pts, a
    3-term product sum like the forward, within 4.1 eps |R| |g|; without need_pts no g_pts is made and g_R, g_t keep their bits"""
    c = OC.case(b, n, "mixed")
    g_R, g_t, g_p = dcl.ops.rigid_points_backward_host(c["tmp"], c["R"], c["t"], inverse, c["g_out"], need_pts=True)
    p64, R64, t64 = (c[k].double().requires_grad_() for k in ("tmp", "R", "t"))
    out = torch.bmm(p64 - t64.unsqueeze(1), R64) if inverse else torch.bmm(p64, R64.transpose(1, 2)) + t64.unsqueeze(1)
    out.backward(c["g_out"].double())
    bR, bt = OC.rigid_grad_bounds(c, inverse)
    eR, et = (g_R.double() - R64.grad).abs(), (g_t.double() - t64.grad).abs()
    print("rigid bwd b=%d n=%d inverse=%d: g_R %.3g, g_t %.3g of the bound" % (b, n, inverse, float((eR / bR).max()),
                                                                                float((et / bt).max())))
    assert bool((eR <= bR).all()) and bool((et <= bt).all())
    Ra, ga = c["R"].double().abs(), c["g_out"].double().abs()
    bp = 4.1 * EPS * (torch.bmm(ga, Ra.transpose(1, 2)) if inverse else torch.bmm(ga, Ra))
    assert bool(((g_p.double() - p64.grad).abs() <= bp).all())
    g_R2, g_t2, none = dcl.ops.rigid_points_backward_host(c["tmp"], c["R"], c["t"], inverse, c["g_out"], need_pts=False)
    assert none is None and torch.equal(g_R2, g_R) and torch.equal(g_t2, g_t)


@pytest.mark.parametrize("kind", OC.SYM_KINDS)
@pytest.mark.parametrize("b,n", OC.SHAPES)
def test_objective_forward_host_against_float64(dcl, b, n, kind):
    """Per-point L within 6 eps relative: a distance carries <= 4 eps (below), the Chamfer mean 0.5 (a + b) of two fp32 inputs
    1 eps, their sum + 1 -> 5, the product with 0.5 s (exact for s in {0, 1}) and the sum with the other, zero, term are exact
    for 0/1 flags; the s = 0 side is 1 * distance: 4 eps.  The five scalars within (20 + ceil(n/256) + b) eps relative --
    every term is non-negative; objective_cases.C_SUM has the derivation, capped at 128 eps.  With all flags 0 the rows of L
    ARE the distances |Xo - cano_gt| and |Yc - posed_gt|, and at (1, 1) loss_pose is |posed - posed_gt|: those are held to
    the distance bound 4 eps (three differences, fma(dz,dz, fma(dy,dy, dx*dx)): 5 eps on the square, halved by the root, + 1)."""
    c = OC.case(b, n, kind)
    args, kw = OC.objective_args(c)
    packed, L = dcl.ops.pose_objective_host(*args, **kw)
    ref = OC.forward64(c)
    assert packed.shape == (5,) and L.shape == (b, 2 * n) and bool(torch.isfinite(packed).all())
    eL = (L.double() - ref["L"]).abs()
    assert bool((eL <= 6 * EPS * ref["L"].abs()).all()), float((eL / ref["L"].abs().clamp_min(1e-300)).max() / EPS)
    if kind == "zeros":
        d = torch.cat([ref["dist"]["Xo_gt"], ref["dist"]["Yc_gt"]], dim=1)
        assert bool((eL <= 4 * EPS * d).all())
        if (b, n) == (1, 1):
            assert abs(float(packed[0]) - float(ref["dist"]["pose"])) <= 4 * EPS * float(ref["dist"]["pose"])
    bound = OC.scalar_bound(b, n)
    err = (packed.double() - ref["packed"]).abs() / ref["packed"].abs().clamp_min(1e-300)
    print("objective fwd b=%d n=%d %s: scalar errors / eps = %s (bound %.0f)" % (b, n, kind, [round(float(e) / EPS, 2) for e in err],
                                                                              bound / EPS))
    assert bool((ref["packed"] >= 0).all()) and bool((err <= bound).all())


@pytest.mark.parametrize("b,n", OC.SHAPES)
def test_pose_only_form_host(dcl, b, n):
    """the refiner's form: only the pose term, packed = [pose, 0, 0, 0, pose], no L"""
    c = OC.case(b, n, "mixed")
    args, kw = OC.objective_args(c, full=False)
    packed, L = dcl.ops.pose_objective_host(*args, **kw)
    full, _ = dcl.ops.pose_objective_host(*OC.objective_args(c)[0], **OC.objective_args(c)[1])
    ref = OC.forward64(c, full=False)["packed"]
    assert L is None and packed[1:4].tolist() == [0.0, 0.0, 0.0] and float(packed[4]) == float(packed[0])
    assert float(packed[0]) == float(full[0])                       # the same sum in the same order
    assert abs(float(packed[0]) - float(ref[0])) <= OC.scalar_bound(b, n) * float(ref[0])
    g = dcl.ops.pose_objective_backward_host(*OC.backward_args(c, OC.upstream(c, "random"), None, full=False)[0])
    want = OC.backward64(c, OC.upstream(c, "random"), full=False)
    w = OC.weights_abs(OC.upstream(c, "random"), b, n)
    assert g[1] is None and g[2] is None and g[3] is None and g[5] == (None, None) and g[6] == (None, None)
    assert bool(((g[0].double() - want["posed"]).abs() <= 8 * EPS * w["pose"]).all())
    assert bool(((g[4][0].double() - want["cd_pose"][0]).abs() <= 8 * EPS * w["pose"]).all())


@pytest.mark.parametrize("up", OC.UPSTREAM)
@pytest.mark.parametrize("kind", OC.SYM_KINDS)
@pytest.mark.parametrize("b,n", OC.SHAPES)
def test_objective_backward_host_against_float64(dcl, b, n, kind, up):
    """Per element within 8 eps |weight| of the float64 formula, |weight| = objective_cases.weights_abs.  A component is
    (k / r) d_c with k = W (1 - s) or W 0.5 s: W carries 2 eps (one fma or sum, one division), the product with a 0/1 flag
    is exact, r 3.5 eps, the quotient 1, d_c 1, the product 1: 8.5 eps |u_c| to first order with |u_c| = |d_c| / r <= 1 --
    and where |u_c| nears 1 the errors of r and d_c are the same error and cancel (5.5 eps at |u_c| = 1), so 8 eps holds.
    g_conf = W_conf (L - 0.01 / c): 2 + (1 constant, 1 division, 1 difference) + 1 product = 6 eps of W_conf (|L| + 0.01 / c).
    A point at distance exactly 0 takes gradient 0 (every case has one in each L2 term of every crop): nothing is NaN."""
    c = OC.case(b, n, kind)
    g_up = OC.upstream(c, up)
    _, L = dcl.ops.pose_objective_host(*OC.objective_args(c)[0], **OC.objective_args(c)[1])
    args, kw = OC.backward_args(c, g_up, L)
    g_posed, g_Xo, g_Yc, g_conf, g_cdp, g_cdx, g_cdy = dcl.ops.pose_objective_backward_host(*args, **kw)
    cl = dict(c)
    want = OC.backward64(cl, g_up)
    w = OC.weights_abs(g_up, b, n)
    for name, got, wt in (("posed", g_posed, w["pose"]), ("Xo", g_Xo, w["Xo"]), ("Yc", g_Yc, w["Yc"])):
        assert bool(torch.isfinite(got).all()), name
        err = (got.double() - want[name]).abs()
        assert bool((err <= 8 * EPS * wt).all()), (name, float(err.max()) / (EPS * max(wt, 1e-300)))
    # the reference differentiates through its own float64 L; the kernel reads the fp32 L it was given (6 eps off at most)
    scale = w["conf"] * (L.double().abs() + 0.01 / c["conf"].double())
    conf64 = g_up.double()[3:].sum() / (2 * b * n) * (L.double() - 0.01 / c["conf"].double())
    assert bool(((g_conf.double() - conf64).abs() <= 8 * EPS * scale).all())
    assert bool(((conf64 - want["conf"]).abs() <= 6 * EPS * scale + 1e-300).all())
    for name, got, wt in (("cd_pose", g_cdp, w["pose"]), ("cd_Xo", g_cdx, w["Xo"]), ("cd_Yc", g_cdy, w["Yc"])):
        for h in range(2):
            assert bool(((got[h].double() - want[name][h]).abs() <= 8 * EPS * wt).all()), name
    if up == "pose":                                               # loss_pose alone reaches nothing but posed and its Chamfer term
        assert not g_Xo.any() and not g_Yc.any() and not g_conf.any() and not g_cdx[0].any() and not g_cdy[1].any()
    zero = [k % n for k in range(5)]                               # the points at distance 0 (objective_cases.case)
    s = c["sym"]
    for crop in range(b):
        assert not g_posed[crop, zero[0]].any()
        if n >= 5 and s[crop] == 0:                                # only the term of the zero distance is live
            assert not g_Xo[crop, zero[1]].any() and not g_Yc[crop, zero[3]].any()


def test_host_twins_reject_gpu_free_misuse(dcl):
    """the host twins take CPU tensors only, the optional arrays go together, and shapes are checked before the call"""
    c = OC.case(3, 63, "mixed")
    args, kw = OC.objective_args(c)
    with pytest.raises(ValueError):
        dcl.ops.pose_objective_host(*args, **dict(kw, conf=None))
    with pytest.raises(AssertionError):
        dcl.ops.pose_objective_host(*args, **dict(kw, conf=c["conf"][:, :-1].contiguous()))
    with pytest.raises(AssertionError):
        dcl.ops.rigid_points_host(c["tmp"], c["R"][:2].contiguous(), c["t"])
    with pytest.raises(RuntimeError, match="GPU"):
        dcl.ops.rigid_points(c["tmp"], c["R"], c["t"])
    with pytest.raises(RuntimeError, match="GPU"):
        dcl.ops.pose_objective(*args, **kw)
    assert math.isclose(OC.scalar_bound(5, 1024), 29 * EPS)
