"""refine_loop(compose="device") on the GPU: the canonicalising first layer (k_refine_first) equals rigid_points + affine3_relu
and its host twin bit for bit; the heads fed with tile partials (k_heads_l1_tiles, k_heads_l23_compose) equal pose_heads on the
ascending chain of the partials and the host twin of the pose composition bit for bit; the loop repeats its bits eager, captured
and replayed, its trajectory is the shorter loops' results, it agrees with the "host" form and with the reference's goldens at
the project's tolerances, and one pass is exactly five launches of the library's own kernels (the diagnostic library's census,
the graph's node count).  tests/test_refine_loop_host.py holds the operands and the host twins' own checks."""
import os

import numpy as np
import pytest
import torch

import test_gpu_ops as TO
import test_kernel_census as KC
import test_refine_loop_host as RH
from conftest import load_golden_data
from test_gpu_network import R_TOL, T_TOL

pytestmark = pytest.mark.gpu


def _refiner(dcl, seed=2):
    ref = dcl.refiner.Refiner()
    ref.load_state_dict(dcl.synth.synth_state_dict(ref, seed))
    return ref.cuda().eval()


# ---------------------------------------------------------------------------------------------------- 4. the first layer
@pytest.mark.parametrize("shape", [(2, 128, 512), (3, 256, 512), (1, 64, 8), (2, 100, 512), (3, 33, 72)],
                         ids=lambda s: "b%d-n%d-c%d" % s)
def test_refine_first_equals_rigid_points_then_affine3_relu_and_the_host_twin(dcl, shape):
    """(2,100,512): crops that end inside a workgroup; (1,64,8), (3,33,72): c / 4 no multiple of 64, a wave spans rows (and crops):
    the kernel form whose row index is per lane"""
    b, n, c = shape
    pts, R, t, W3, term = RH.first_case(b, n, c, seed=5)
    dev = [x.cuda() for x in (pts, R, t, W3, term)]
    got = dcl.ops.refine_first(*dev)
    cur = dcl.ops.rigid_points(dev[0], dev[1], dev[2], inverse=True).view(b * n, 3)
    want = dcl.ops.affine3_relu(cur, dev[3], dev[4])
    assert RH.same_bits(got, want), float((got - want).abs().max())
    assert RH.same_bits(got, dcl.ops.refine_first_host(pts, R, t, W3, term))
    assert RH.same_bits(dcl.ops.refine_first(*dev), got)
    assert bool((got > 0).any()) and bool((got == 0).any())
    for x, x0 in zip(dev, (pts, R, t, W3, term)):                                             # inputs are read only
        assert torch.equal(x.cpu(), x0)


# ---------------------------------------------------------------------------------------------------- 5. the heads
@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("T", [1, 2, 8])
def test_refine_heads_equal_pose_heads_on_the_ascending_chain_and_the_composition_twin(dcl, T, b):
    f = _refiner(dcl)._fold()
    g = torch.Generator().manual_seed(100 * T + b)
    part = torch.randn(b * T, 1024, generator=g).cuda()
    R_in, t_in = RH.rotations(b, g).cuda(), RH.magnitudes((b, 3), g).cuda()
    R0, t0 = R_in.clone(), t_in.clone()
    R_out = torch.full((b, 3, 3), float("nan"), device="cuda")
    t_out = torch.full((b, 3), float("nan"), device="cuda")
    o9, dt, dR = dcl.ops.refine_heads(part, T, f["regressor_rot2"], f["regressor_trans2"], R_in, t_in, R_out, t_out)
    p3 = part.view(b, T, 1024)
    acc = p3[:, 0]
    for s in range(1, T):
        acc = acc + p3[:, s]                                                                  # one ascending fp32 chain from tile 0
    w9, wt, wR = dcl.ops.pose_heads(acc.contiguous(), f["regressor_rot2"], f["regressor_trans2"], with_rotation=True)
    assert RH.same_bits(o9, w9) and RH.same_bits(dt, wt) and RH.same_bits(dR, wR)
    wRo, wto = dcl.ops.pose_compose_host(R0.cpu(), t0.cpu(), dR.cpu(), dt.cpu())
    assert RH.same_bits(R_out, wRo), float((R_out.cpu() - wRo).abs().max())
    assert RH.same_bits(t_out, wto), float((t_out.cpu() - wto).abs().max())
    assert RH.same_bits(R_in, R0) and RH.same_bits(t_in, t0)                                  # the inputs are left as they are
    with pytest.raises(RuntimeError, match="invalid argument"):                               # in and out must be different arrays
        dcl.ops.refine_heads(part, T, f["regressor_rot2"], f["regressor_trans2"], R_in, t_in, R_in, t_out)


# ---------------------------------------------------------------------------------------------------- 6. the loop
def _loop_case(b, n, seed=11):
    g = torch.Generator().manual_seed(seed)
    F = torch.randn(b, 256, n, generator=g).cuda()
    pts = (torch.randn(b, n, 3, generator=g) * 0.05).cuda()
    conf = torch.rand(b, n, generator=g).cuda()                                               # (conf[:, :1024]: one per point)
    pred = {"rot_pred": RH.rotations(b, g).cuda(), "trans_pred": (torch.randn(b, 3, generator=g) * 0.02).cuda(),
            "F_Xo_p": F, "conf": conf}
    return pred, pts


def test_loop_repeats_its_bits_and_its_trajectory_is_the_shorter_loops(dcl):
    b, n = 2, 256
    ref = _refiner(dcl, 4)
    pred, pts = _loop_case(b, n)
    loop = dcl.refiner.refine_loop
    rot, trans, (rots, transs) = loop(ref, pred, pts, 3, compose="device", trajectory=True)
    assert tuple(rots.shape) == (4, b, 3, 3) and tuple(transs.shape) == (4, b, 3)
    assert RH.same_bits(rot, rots[-1]) and RH.same_bits(trans, transs[-1])
    assert RH.same_bits(rots[0], pred["rot_pred"]) and RH.same_bits(transs[0], pred["trans_pred"])
    assert not torch.equal(rots[1], rots[0]) and not torch.equal(rots[3], rots[2])
    for graph in (False, True, True, False):                                                  # eager, capture, replay, eager again
        r, t, (rs, ts) = loop(ref, pred, pts, 3, graph=graph, compose="device", trajectory=True)
        assert RH.same_bits(rs, rots) and RH.same_bits(ts, transs), graph
        assert RH.same_bits(r, rot) and RH.same_bits(t, trans), graph
    assert list(ref._graphs) == [(b, n, 3, n, "device")]
    for k in range(4):
        for graph in (False, True):
            r, t = loop(ref, pred, pts, k, graph=graph, compose="device")
            assert RH.same_bits(r, rots[k]) and RH.same_bits(t, transs[k]), (k, graph)
    # against the "host" form: other association orders of the same formulas
    for it in (1, 3):
        hr, ht = loop(ref, pred, pts, it)
        dR, dt = float((hr - rots[it]).abs().max()), float((ht - transs[it]).abs().max())
        print("device vs host form, iteration %d: |dR| %.3g (tol %.0e)  |dt| %.3g (tol %.0e)" % (it, dR, R_TOL, dt, T_TOL))
        assert dR <= R_TOL and dt <= T_TOL
    # the replay copies the call's own pose in: another incoming pose, the same graph
    pred2 = dict(pred, rot_pred=pred["rot_pred"].flip(0).contiguous(), trans_pred=pred["trans_pred"] * 0.5)
    want = loop(ref, pred2, pts, 3, compose="device")
    got = loop(ref, pred2, pts, 3, graph=True, compose="device")
    assert RH.same_bits(got[0], want[0]) and RH.same_bits(got[1], want[1]) and not torch.equal(got[0], rot)
    assert len(ref._graphs) == 4                                                              # iterations 3, 0, 1, 2 of the device form


# ---------------------------------------------------------------------------------------------------- 7. reference goldens
def test_device_form_matches_the_refiner_golden(dcl, golden_dir):
    z = np.load(os.path.join(golden_dir, "refiner_b2.npz"))
    ref = _refiner(dcl, 2)
    g = torch.Generator().manual_seed(int(z["gen_seed"][0]))
    bb, n = 2, 1024
    F = torch.randn(bb, 256, n, generator=g).cuda()
    pts = (torch.randn(bb, n, 3, generator=g) * 0.05).cuda()
    conf = torch.rand(bb, 2 * n, generator=g).cuda()
    pred = {"rot_pred": torch.from_numpy(z["rot0"]).cuda(), "trans_pred": torch.from_numpy(z["trans0"]).cuda(), "F_Xo_p": F,
            "conf": conf}
    for graph in (False, True, True):                        # eager, capture, replay
        rot, trans = dcl.refiner.refine_loop(ref, pred, pts, 2, graph=graph, compose="device")
        dR, dt = np.abs(rot.cpu().numpy() - z["rot_final"]).max(), np.abs(trans.cpu().numpy() - z["trans_final"]).max()
        print("refiner_b2 (graph=%s): |dR| %.3g (tol %.0e)  |dt| %.3g (tol %.0e)" % (graph, dR, R_TOL, dt, T_TOL))
        assert dR <= R_TOL and dt <= T_TOL


@pytest.mark.parametrize("graphed", [False, True])
def test_stage2_chain_device_form_matches_the_reference_golden(dcl, golden_dir, graphed):
    data, exp, (b, n_inp, n_tmp, wseed) = load_golden_data(os.path.join(golden_dir, "dclnet_b4_n1024_chain.npz"))
    cfg = dcl.synth.default_cfg(n_inp, n_tmp)
    net = dcl.DCL_Net.Network(cfg, mode="test", graph_max_batch=8 if graphed else 0)
    net.load_state_dict(dcl.synth.synth_state_dict(net, wseed))
    net = net.cuda().eval()
    ref = _refiner(dcl, int(exp["refiner_seed"][0]))
    for _ in range(2):                                                       # second round: graph replays
        d = {k: ({kk: vv.clone() for kk, vv in v.items()} if isinstance(v, dict) else v) for k, v in data.items()}
        rot, trans, pred, (rots, transs) = dcl.refiner.stage2_chain(net, ref, d, 2, graph=graphed, compose="device",
                                                                     trajectory=True)
        for name, got, key in (("final R", rot, "rot_final"), ("final t", trans, "trans_final"), ("iter1 R", rots[1], "rot_iter1"),
                               ("iter1 t", transs[1], "trans_iter1")):
            err, tol = np.abs(got.cpu().numpy() - exp[key]).max(), R_TOL if key.startswith("rot") else T_TOL
            print("chain golden (graphed=%s) %s: %.3g (tol %.0e)" % (graphed, name, err, tol))
            assert err <= tol, key
        assert RH.same_bits(rots[0], pred["rot_pred"]) and RH.same_bits(rots[2], rot)
        plain = dcl.refiner.stage2_chain(net, ref, d, 2, graph=graphed, compose="device")
        assert len(plain) == 3 and RH.same_bits(plain[0], rot) and RH.same_bits(plain[1], trans)
    if graphed:
        assert len(net._graphs) == 1 and list(ref._graphs) == [(b, n_inp, 2, 2 * n_inp, "device")]


# ---------------------------------------------------------------------------------------------------- 8. launch budget
def _census_of(lib, call):
    lib.dcl_debug_launch_census_reset()
    call()
    torch.cuda.synchronize()
    return KC.census(lib)


def test_one_pass_of_the_device_form_is_five_launches_of_own_kernels(request, dcl):
    lib = TO.enter_diag(dcl, request)
    b, n = 2, 256
    ref = _refiner(dcl, 4)
    pred, pts = _loop_case(b, n)
    loop = dcl.refiner.refine_loop
    loop(ref, pred, pts, 1, compose="device")                                                 # (lazy initialisations, weight pieces)
    loop(ref, pred, pts, 1)
    counts = {}
    for form in ("device", "host"):
        for it in (1, 3):
            counts[form, it] = _census_of(lib, lambda: loop(ref, pred, pts, it, compose=form))
    per_pass = {}
    for form in ("device", "host"):
        keys = set(counts[form, 1]) | set(counts[form, 3])
        per_pass[form] = {k: counts[form, 3].get(k, 0) - counts[form, 1].get(k, 0) for k in keys}
        per_pass[form] = {k: v for k, v in per_pass[form].items() if v}
        print("%s form: library launches per call, iteration 1 / 3: %d / %d; two more passes add %s"
              % (form, sum(counts[form, 1].values()), sum(counts[form, 3].values()), sorted(per_pass[form].items())))
    dev = per_pass["device"]
    assert sum(dev.values()) == 10 and all(k.startswith("k_") for k in dev), dev
    assert dev.get("k_refine_first<true>") == 2 and dev.get("k_heads_l1_tiles") == 2 and dev.get("k_heads_l23_compose") == 2, dev
    assert not {"k_affine3_relu", "k_rigid_points", "k_heads_l23", "k_heads_l1<false>", "k_heads_l1<true>"} & set(counts["device", 3])
    # the graphs: every node is a launch, torch's and the vendor library's included
    nodes = {}
    for form in ("device", "host"):
        for it in (1, 3):
            loop(ref, pred, pts, it, graph=True, compose=form)
            key = (b, n, it, n) + (("device",) if form == "device" else ())
            nodes[form, it] = dcl.DCL_Net.Network._graph_nodes(ref._graphs[key][0])
    print("graph nodes, iteration 1 / 3: device %s / %s, host %s / %s"
          % (nodes["device", 1], nodes["device", 3], nodes["host", 1], nodes["host", 3]))
    if nodes["device", 1] is not None and nodes["device", 3] is not None:                     # (where the runtime lets us ask)
        assert nodes["device", 3] - nodes["device", 1] == 10
        if nodes["host", 1] is not None and nodes["host", 3] is not None:
            assert nodes["host", 3] - nodes["host", 1] > 10


# ---------------------------------------------------------------------------------------------------- 9. refusals
def test_device_form_refuses_what_it_cannot_run(dcl):
    ref = _refiner(dcl, 4)
    pred, pts = _loop_case(2, 100)
    with pytest.raises(ValueError, match="n % 128 == 0"):
        dcl.refiner.refine_loop(ref, pred, pts, 2, compose="device")
    with pytest.raises(ValueError, match="n % 128 == 0"):
        dcl.refiner.refine_loop(ref, pred, pts, 2, graph=True, compose="device")
    assert not ref.__dict__.get("_graphs")
    pred, pts = _loop_case(2, 128)
    pred["conf"] = torch.cat([pred["conf"], pred["conf"]], 1)                                 # two confidences per point
    with pytest.raises(ValueError, match="confidence"):
        dcl.refiner.refine_loop(ref, pred, pts, 2, compose="device")
    with pytest.raises(ValueError, match="trajectory"):
        dcl.refiner.refine_loop(ref, pred, pts, 2, trajectory=True)
