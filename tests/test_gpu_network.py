"""End-to-end GPU parity of Network.forward / Refiner against the reference-generated golden vectors and
against the CPU oracle graph on fresh seeded crops.  Tolerances are BASELINE.json's: |dR| <= 1e-4,
|dt| <= 1e-5 m; integer outputs (voxel ids) bit-exact."""
import os

import numpy as np
import pytest
import torch

from conftest import load_golden_data, load_stress_golden

pytestmark = pytest.mark.gpu

R_TOL, T_TOL = 1e-4, 1e-5


def _net(dcl, n_inp, n_tmp, seed, fused=True, graph_max_batch=0):
    """eager by default: the whole-forward graph path of small batches has its own tests (graphed=True, forward_graphed)"""
    cfg = dcl.synth.default_cfg(n_inp, n_tmp)
    net = dcl.DCL_Net.Network(cfg, mode="test", fused=fused, graph_max_batch=graph_max_batch)
    sd = dcl.synth.synth_state_dict(net, seed)
    net.load_state_dict(sd)
    return net.cuda().eval(), sd, cfg


def _check(pred, exp_R, exp_t, exp_conf):
    assert np.abs(pred["rot_pred"].cpu().numpy() - exp_R).max() <= R_TOL
    assert np.abs(pred["trans_pred"].cpu().numpy() - exp_t).max() <= T_TOL
    assert np.abs(pred["conf"].cpu().numpy() - exp_conf).max() <= 1e-4


@pytest.mark.parametrize("fused", [True, False])
def test_forward_matches_reference_golden(dcl, golden_dir, fused):
    data, exp, (b, n_inp, n_tmp, wseed) = load_golden_data(os.path.join(golden_dir, "dclnet_b2_n256.npz"))
    net, _, _ = _net(dcl, n_inp, n_tmp, wseed, fused)
    with torch.no_grad():
        pred = net(data)
    _check(pred, exp["rot_pred"], exp["trans_pred"], exp["conf"])
    F = pred["F_Xo_p"]
    assert tuple(F.shape) == (b, 256, n_inp)
    sub = F[:, ::8, ::8].cpu().numpy()
    assert np.abs(sub - exp["F_Xo_p_sub"]).max() <= 1e-4 * max(1.0, np.abs(exp["F_Xo_p_sub"]).max())
    assert np.abs(F.double().sum(dim=2).cpu().numpy() - exp["F_Xo_p_sum"]).max() <= 1e-3 * max(
        1.0, np.abs(exp["F_Xo_p_sum"]).max())
    assert tuple(data["labels"]["points_inp"].shape) == (b, n_inp, 3)
    assert tuple(data["labels"]["points_tmp"].shape) == (b, n_tmp, 3)


@pytest.mark.parametrize("graph_max_batch", [0, 8])
def test_forward_matches_reference_golden_at_the_stress_shape(dcl, golden_dir, graph_max_batch):
    """ONE crop of BASELINE configs[1]'s shape (N = 12288 / M = 2048) against the reference's own Network run on the same
    procedural crop (tests/golden/dclnet_stress_b1.npz), launch by launch and as the default one-crop graph replay"""
    data, exp, (b, n_inp, n_tmp, wseed) = load_stress_golden(dcl, os.path.join(golden_dir, "dclnet_stress_b1.npz"))
    net, _, _ = _net(dcl, n_inp, n_tmp, wseed, graph_max_batch=graph_max_batch)
    with torch.no_grad():
        pred = net(data)
    _check(pred, exp["rot_pred"], exp["trans_pred"], exp["conf"])
    F = pred["F_Xo_p"]
    assert tuple(F.shape) == (b, 256, n_inp)
    sub = F[:, ::8, ::64].cpu().numpy()
    assert np.abs(sub - exp["F_Xo_p_sub"]).max() <= 1e-4 * max(1.0, np.abs(exp["F_Xo_p_sub"]).max())
    assert np.abs(F.double().sum(dim=2).cpu().numpy() - exp["F_Xo_p_sum"]).max() <= 1e-3 * max(
        1.0, np.abs(exp["F_Xo_p_sum"]).max())


@pytest.mark.parametrize("fixture", ["dclnet_s0_train.npz", "dclnet_nm384_train.npz"])
@pytest.mark.parametrize("fused", [True, False])
def test_train_mode_outputs_match_reference_golden(dcl, golden_dir, fixture, fused):
    """mode='train' forward (eval-mode BatchNorm) incl. Xo_pred / Yc_pred at BASELINE config 0's shape (N=2048, M=500, 5 mm
    voxels) and at N=M=384; on the latter the objectives reproduce the reference's loss values"""
    data, exp, (b, n_inp, n_tmp, wseed) = load_golden_data(os.path.join(golden_dir, fixture))
    cfg = dcl.synth.default_cfg(n_inp, n_tmp, unit=0.005)
    net = dcl.DCL_Net.Network(cfg, mode="train", fused=fused)
    net.load_state_dict(dcl.synth.synth_state_dict(net, wseed))
    net = net.cuda().eval()
    with torch.no_grad():
        pred = net(data)
    _check(pred, exp["rot_pred"], exp["trans_pred"], exp["conf"])
    for k in ("Xo_pred", "Yc_pred"):
        assert tuple(pred[k].shape) == exp[k].shape
        assert np.abs(pred[k].cpu().numpy() - exp[k]).max() <= 1e-4 * max(1.0, np.abs(exp[k]).max()), k
    if "losses" in exp:
        lo = dcl.DCL_Net.losses(None)(pred, data["labels"])
        got = np.array([float(lo[k]) for k in ("loss_pose", "loss_Xo", "loss_Yc", "loss_conf", "loss_all")])
        assert np.abs(got - exp["losses"]).max() <= 2e-4 * max(1.0, np.abs(exp["losses"]).max())


@pytest.mark.parametrize("b,n_inp,n_tmp,unit", [(3, 1024, 1024, 0.006), (1, 2048, 500, 0.005), (5, 512, 1024, 0.006),
                                               (8, 1024, 1024, 0.005), (1, 12288, 2048, 0.006), (2, 333, 517, 0.006)])
def test_forward_matches_oracle_graph(dcl, oracle, b, n_inp, n_tmp, unit):
    """fresh crops at the reference shape (N=M=1024), the plumbing shape S0 (N=2048, M=500, 5 mm), a ragged one, the
    LineMOD config (5 mm voxels, config_LM.yaml), one crop of the BASELINE stress shape (N=12288, M=2048) and point counts
    that are multiples of nothing -- each both ways a caller can get it: launch by launch, and as a default-constructed
    Network runs calls this small (whole-forward hipGraph replay)"""
    from oracle import graph as G
    cfg = dcl.synth.default_cfg(n_inp, n_tmp, unit)
    data = dcl.synth.make_batch(b, n_inp, n_tmp, unit=unit, first=40)
    ref_data = {k: ({kk: vv.clone() for kk, vv in v.items()} if isinstance(v, dict) else v) for k, v in data.items()}
    want = None
    for kw, graphs in (({"graph_max_batch": 0}, 0), ({}, 1)):
        net = dcl.DCL_Net.Network(cfg, mode="test", **kw)
        sd = dcl.synth.synth_state_dict(net, 3)
        net.load_state_dict(sd)
        net = net.cuda().eval()
        if want is None:
            want = G.forward(sd, dict(cfg), ref_data, mode="test")
        with torch.no_grad():
            pred = net(data)
        assert len(net.__dict__.get("_graphs", {})) == graphs
        _check(pred, want["rot_pred"].numpy(), want["trans_pred"].numpy(), want["conf"].numpy())
        got_F, want_F = pred["F_Xo_p"].cpu(), want["F_Xo_p"]
        assert float((got_F - want_F).abs().max()) <= 1e-4 * max(1.0, float(want_F.abs().max()))


def test_backbone_levels_and_indices_bit_exact(dcl, oracle):
    """voxel ids of every pooled level are bit-exact; features within fp32 GEMM tolerance"""
    from oracle import graph as G
    b, n = 2, 1024
    net, sd, cfg = _net(dcl, n, n, 4)
    data = dcl.synth.make_batch(b, n, n, first=7)
    occ = data["inp"]["occupied_voxels"].int()
    vox = oracle.voxelize_fp(data["inp"]["feats"].numpy(), data["inp"]["v2p_maps"].numpy(), 4)
    want = G.backbone(sd, "backbone_inp", vox, occ.numpy(), [64] * 3, b)
    run = dcl.ops.BackboneRun(occ.cuda().contiguous(), b, 64)
    run.set_counts(run.counts_dev.cpu().tolist())
    x = dcl.ops.voxelize_fp(data["inp"]["feats"].cuda(), data["inp"]["v2p_maps"].cuda(), 4)
    assert np.array_equal(x.cpu().numpy(), vox)
    levels = run.features(x, *net._fold()["backbone_inp_ptrs"])
    for m, (gx, (wx, wi)) in enumerate(zip(levels, want)):
        assert np.array_equal(run.level_indices(m).cpu().numpy(), wi)
        assert np.abs(gx.cpu().numpy() - wx).max() <= 1e-4 * max(1.0, np.abs(wx).max())


def test_refiner_matches_reference_golden(dcl, golden_dir):
    z = np.load(os.path.join(golden_dir, "refiner_b2.npz"))
    ref = dcl.refiner.Refiner()
    ref.load_state_dict(dcl.synth.synth_state_dict(ref, 2))
    ref = ref.cuda().eval()
    g = torch.Generator().manual_seed(int(z["gen_seed"][0]))
    bb, n = 2, 1024
    F = torch.randn(bb, 256, n, generator=g).cuda()
    pts = (torch.randn(bb, n, 3, generator=g) * 0.05).cuda()
    conf = torch.rand(bb, 2 * n, generator=g).cuda()
    rot0, trans0 = torch.from_numpy(z["rot0"]).cuda(), torch.from_numpy(z["trans0"]).cuda()
    cur = torch.bmm(pts - trans0.unsqueeze(1), rot0)
    out = ref({"input_features": torch.cat([cur.transpose(1, 2), F], 1), "conf": conf, "obj_idx": None})
    assert np.abs(out["trans_pred"].cpu().numpy() - z["dt_first"]).max() <= T_TOL
    assert np.abs(out["rot_pred"].cpu().numpy() - z["dR_first"]).max() <= R_TOL
    pred = {"rot_pred": rot0, "trans_pred": trans0, "F_Xo_p": F, "conf": conf}
    for graph in (False, True, True):                        # eager, capture, replay
        rot, trans = dcl.refiner.refine_loop(ref, pred, pts, 2, graph=graph)
        assert np.abs(rot.cpu().numpy() - z["rot_final"]).max() <= R_TOL
        assert np.abs(trans.cpu().numpy() - z["trans_final"]).max() <= T_TOL


@pytest.mark.parametrize("graphed", [False, True])
def test_reference_shape_and_stage2_chain_match_reference_golden(dcl, golden_dir, graphed):
    """N = M = 1024 (the shape config_YCBV_bs32.yaml defines), b = 4, vectors from the REFERENCE's Network + Refiner:
    stage-1 outputs, then BASELINE configs[4] -- model(data) -> (P - t) R -> cat[points, F_Xo_p] -> 2 x refiner with pose
    composition (tools/test_YCBV_stage2.py:204-225) -- as ONE pipeline (refiner.stage2_chain), eager and with the
    whole-forward / refine-loop hipGraphs; ADD-S of both poses through the fused metric kernel"""
    data, exp, (b, n_inp, n_tmp, wseed) = load_golden_data(os.path.join(golden_dir, "dclnet_b4_n1024_chain.npz"))
    cfg = dcl.synth.default_cfg(n_inp, n_tmp)
    net = dcl.DCL_Net.Network(cfg, mode="test", graph_max_batch=8 if graphed else 0)
    net.load_state_dict(dcl.synth.synth_state_dict(net, wseed))
    net = net.cuda().eval()
    ref = dcl.refiner.Refiner()
    ref.load_state_dict(dcl.synth.synth_state_dict(ref, int(exp["refiner_seed"][0])))
    ref = ref.cuda().eval()
    for _ in range(2):                                                       # second round: graph replays
        d = {k: ({kk: vv.clone() for kk, vv in v.items()} if isinstance(v, dict) else v) for k, v in data.items()}
        rot, trans, pred = dcl.refiner.stage2_chain(net, ref, d, 2, graph=graphed)
        _check(pred, exp["rot_pred"], exp["trans_pred"], exp["conf"])
        sub = pred["F_Xo_p"][:, ::8, ::8].cpu().numpy()
        assert np.abs(sub - exp["F_Xo_p_sub"]).max() <= 1e-4 * max(1.0, np.abs(exp["F_Xo_p_sub"]).max())
        assert np.abs(rot.cpu().numpy() - exp["rot_final"]).max() <= R_TOL
        assert np.abs(trans.cpu().numpy() - exp["trans_final"]).max() <= T_TOL
        rot1, trans1 = dcl.refiner.refine_loop(ref, pred, d["labels"]["points_inp"], 1, graph=graphed)
        assert np.abs(rot1.cpu().numpy() - exp["rot_iter1"]).max() <= R_TOL
        assert np.abs(trans1.cpu().numpy() - exp["trans_iter1"]).max() <= T_TOL
        cld = d["labels"]["points_tmp"]
        Rg, tg = torch.from_numpy(exp["rot_gt"]).cuda(), torch.from_numpy(exp["trans_gt"]).cuda()
        for (R, t), key in (((pred["rot_pred"], pred["trans_pred"]), "adds_stage1"), ((rot, trans), "adds_final")):
            got = dcl.ops.add_s(cld.contiguous(), R, t, Rg, tg).cpu().numpy()
            assert np.abs(got - exp[key]).max() <= 2e-5, key
    if graphed:
        assert len(net._graphs) == 1 and len(ref._graphs) == 2               # (iteration=2) and (iteration=1) loops


@pytest.mark.parametrize("path", ["launch by launch", "default"])
def test_bs40_config_forward(dcl, oracle, path):
    """BASELINE configs[2]'s per-GPU shape: 40 crops per call (config_YCBV_bs40.yaml: bs 40), N = M = 1024 -- launch by
    launch and as a default-constructed Network runs it (81920 points per call: whole-forward hipGraph replay).  Four crops
    spread over the batch are checked against the CPU oracle graph run on exactly those crops (crops are independent);
    all 40 get the size-independent checks (valid rotations, confidences in (0,1), determinism, no NaN) and the metric
    table of the batch reduces to 40 frames"""
    batch_of_reference_shape_crops_vs_oracle(dcl, oracle, 40, path)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("b,path", [(33, "launch by launch"), (33, "default"), (25, "default")])
def test_forward_of_a_batch_that_does_not_tile_the_chip(dcl, oracle, b, path):
    """33 crops of N = M = 1024: M = 33792 rows do not divide into whole rounds of GEMM tiles over 256 CUs -- the shape at
    which the GEMM library's first-choice algorithms exchange partial tiles between workgroups and two of them, side by side on
    the forward's two streams, hung the GPU (csrc/linear.cpp: get_plan; 25 crops: the same through torch's own call of the
    library, which the forward no longer makes -- models/DCL_Net.py: _lin_relu).  Same checks as the other batch sizes; 33 is
    also the batch at which the attention pair is issued as 32 + 1 crops.  tools/batch_sweep.py walks 1..48."""
    batch_of_reference_shape_crops_vs_oracle(dcl, oracle, b, path)


def batch_of_reference_shape_crops_vs_oracle(dcl, oracle, b, path):
    """b crops of N = M = 1024: four of them against the oracle graph, all of them the size-independent checks (also run at
    b = 32, the shape of profiles/*_ref_kernel_stats.csv, by tests/test_kernel_census.py)"""
    from oracle import graph as G
    n = 1024
    net, sd, cfg = _net(dcl, n, n, 1, graph_max_batch=8 if path == "default" else 0)
    assert (len(getattr(net, "_graphs", {})) == 0)
    data = dcl.synth.make_batch(b, n, n, first=100)
    with torch.no_grad():
        p1 = net(data)
        p2 = net(dcl.synth.make_batch(b, n, n, first=100))
    R = p1["rot_pred"].double()
    assert tuple(R.shape) == (b, 3, 3) and tuple(p1["conf"].shape) == (b, 2 * n) and tuple(p1["F_Xo_p"].shape) == (b, 256, n)
    assert float((R @ R.transpose(1, 2) - torch.eye(3, dtype=torch.float64, device="cuda")).abs().max()) <= 1e-5
    assert float((torch.linalg.det(R) - 1).abs().max()) <= 1e-5
    assert bool(((p1["conf"] > 0) & (p1["conf"] < 1)).all()) and bool(torch.isfinite(p1["F_Xo_p"]).all())
    for k in ("rot_pred", "trans_pred", "conf"):
        assert torch.equal(p1[k], p2[k]), k
    assert len(net.__dict__.get("_graphs", {})) == (1 if path == "default" else 0)      # the path that was meant ran
    for i in sorted({0, min(13, b - 1), min(27, b - 1), b - 1}):
        one = dcl.synth.make_batch(1, n, n, first=100 + i, voxelize_idx=lambda c, bs, mode: tuple(
            torch.from_numpy(a) for a in oracle.voxelize_idx(c.numpy(), bs, mode)))
        want = G.forward(sd, dict(cfg), one, mode="test")
        assert float((p1["rot_pred"][i].cpu() - want["rot_pred"][0]).abs().max()) <= R_TOL, i
        assert float((p1["trans_pred"][i].cpu() - want["trans_pred"][0]).abs().max()) <= T_TOL, i
        assert float((p1["conf"][i].cpu() - want["conf"][0]).abs().max()) <= 1e-4, i
        wF = want["F_Xo_p"][0]
        assert float((p1["F_Xo_p"][i].cpu() - wF).abs().max()) <= 1e-4 * max(1.0, float(wF.abs().max())), i
    d = dcl.sharding.add_s(data["labels"]["points_tmp"].contiguous(), p1["rot_pred"], p1["trans_pred"],
                           data["labels"]["rot_gt"].cuda(), data["labels"]["trans_gt"].cuda()).cpu().tolist()
    table = dcl.sharding.AddsTable()
    for c, x in zip(data["obj_idx"].tolist(), d):
        table.add(int(c), float(x))
    assert int(table.sums[:, 0].sum()) == b


def test_stress_shape_full_batch_properties(dcl, oracle):
    """BASELINE configs[1] at its full size (b = 32, N = 12288, M = 2048; what bench.py times): crops 0 / 3 / 17 / 30 of the
    batch against the CPU oracle graph run on each of them alone (the reference's arithmetic, oracle/graph.py), then the
    size-independent checks on all 32 -- valid rotations, finite outputs, determinism -- and batch invariance of the HIP path
    itself: crops 3 and 30 recomputed alone (4-wave attention kernel, other conv tilings) give the same pose"""
    from oracle import graph as G
    n_inp, n_tmp, b = 12288, 2048, 32
    cfg = dcl.synth.default_cfg(n_inp, n_tmp)
    net = dcl.DCL_Net.Network(cfg, mode="test", graph_max_batch=0)
    sd = dcl.synth.synth_state_dict(net, 1)
    net.load_state_dict(sd)
    net = net.cuda().eval()
    data = dcl.synth.make_batch(b, n_inp, n_tmp)
    with torch.no_grad():
        full = net(data)
        again = net(data)
    for i in (0, 3, 17, 30):
        one = dcl.synth.make_batch(1, n_inp, n_tmp, first=i, voxelize_idx=lambda c, bs, mode: tuple(
            torch.from_numpy(a) for a in oracle.voxelize_idx(c.numpy(), bs, mode)))
        want = G.forward(sd, dict(cfg), one, mode="test")
        assert float((full["rot_pred"][i].cpu() - want["rot_pred"][0]).abs().max()) <= R_TOL, i
        assert float((full["trans_pred"][i].cpu() - want["trans_pred"][0]).abs().max()) <= T_TOL, i
        assert float((full["conf"][i].cpu() - want["conf"][0]).abs().max()) <= 1e-4, i
        wF = want["F_Xo_p"][0]
        assert float((full["F_Xo_p"][i].cpu() - wF).abs().max()) <= 1e-4 * max(1.0, float(wF.abs().max())), i
    R = full["rot_pred"].double()
    assert float((R @ R.transpose(1, 2) - torch.eye(3, dtype=torch.float64, device="cuda")).abs().max()) <= 1e-5
    assert float((torch.linalg.det(R) - 1).abs().max()) <= 1e-5
    assert bool(torch.isfinite(full["F_Xo_p"]).all()) and bool(((full["conf"] > 0) & (full["conf"] < 1)).all())
    for k in ("rot_pred", "trans_pred", "conf"):
        assert torch.equal(full[k], again[k]), k
    with torch.no_grad():
        for i in (3, 30):
            one = net(dcl.synth.make_batch(1, n_inp, n_tmp, first=i))
            assert float((one["rot_pred"][0] - full["rot_pred"][i]).abs().max()) <= R_TOL
            assert float((one["trans_pred"][0] - full["trans_pred"][i]).abs().max()) <= T_TOL
            assert float((one["conf"][0] - full["conf"][i]).abs().max()) <= 1e-4


def test_full_size_properties(dcl):
    """BASELINE-size batch (b=32, N=M=1024): size-independent properties -- valid rotations, softmax-normalised
    confidences, determinism, and batch-composition invariance (crop i's pose does not depend on its batch mates)."""
    b, n = 32, 1024
    net, _, _ = _net(dcl, n, n, 1)
    data = dcl.synth.make_batch(b, n, n)
    with torch.no_grad():
        p1 = net(data)
        p2 = net(dcl.synth.make_batch(b, n, n))
    R = p1["rot_pred"].double()
    assert float((R @ R.transpose(1, 2) - torch.eye(3, dtype=torch.float64, device="cuda")).abs().max()) <= 1e-5
    assert float((torch.linalg.det(R) - 1).abs().max()) <= 1e-5
    assert bool(((p1["conf"] > 0) & (p1["conf"] < 1)).all())
    assert torch.equal(p1["rot_pred"], p2["rot_pred"]) and torch.equal(p1["trans_pred"], p2["trans_pred"])
    with torch.no_grad():
        sub = net(dcl.synth.make_batch(4, n, n, first=8))
    assert float((sub["rot_pred"] - p1["rot_pred"][8:12]).abs().max()) <= R_TOL
    assert float((sub["trans_pred"] - p1["trans_pred"][8:12]).abs().max()) <= T_TOL


def test_stress_shape_batch_invariance(dcl):
    """BASELINE stress shape (N=12288, M=2048): a 6-crop batch takes the 8-wave LDS-DMA attention kernel, single crops
    take the 4-wave one; each crop's pose must not depend on its batch mates or on the kernel variant"""
    n_inp, n_tmp = 12288, 2048
    cfg = dcl.synth.default_cfg(n_inp, n_tmp)
    net = dcl.DCL_Net.Network(cfg, mode="test", graph_max_batch=0)      # eager: the kernel variants are the subject
    net.load_state_dict(dcl.synth.synth_state_dict(net, 1))
    net = net.cuda().eval()
    with torch.no_grad():
        full = net(dcl.synth.make_batch(6, n_inp, n_tmp, first=20))
        for i in (0, 5):
            one = net(dcl.synth.make_batch(1, n_inp, n_tmp, first=20 + i))
            assert float((one["rot_pred"][0] - full["rot_pred"][i]).abs().max()) <= R_TOL
            assert float((one["trans_pred"][0] - full["trans_pred"][i]).abs().max()) <= T_TOL
            assert float((one["conf"][0] - full["conf"][i]).abs().max()) <= 1e-4


def test_whole_forward_hipgraph_matches_eager(dcl):
    """forward_graphed (capacity-mode sparse runner + dense part captured in one hipGraph) == forward, across replays
    with different crops (different voxel counts / maxActive)"""
    b, n = 3, 1024
    net, _, _ = _net(dcl, n, n, 1)
    for first in (0, 11, 40, 0):
        data = dcl.synth.make_batch(b, n, n, first=first)
        with torch.no_grad():
            want = net(dcl.synth.make_batch(b, n, n, first=first))
        got = net.forward_graphed(data)
        assert float((got["rot_pred"] - want["rot_pred"]).abs().max()) <= R_TOL
        assert float((got["trans_pred"] - want["trans_pred"]).abs().max()) <= T_TOL
        assert float((got["conf"] - want["conf"]).abs().max()) <= 1e-4
        assert float((got["F_Xo_p"] - want["F_Xo_p"]).abs().max()) <= 1e-4 * max(1.0, float(want["F_Xo_p"].abs().max()))
        assert tuple(data["labels"]["points_inp"].shape) == (b, n, 3)
    assert len(net._graphs) == 1
    # replays back to back and with unrelated kernels in between (a graph holding memset nodes faulted here on ROCm 7.2)
    scr = torch.zeros(4096, device="cuda")
    wants = {}
    for first in (5, 23):
        with torch.no_grad():
            wants[first] = net(dcl.synth.make_batch(b, n, n, first=first))
    for first in (5, 23, 23, 5):
        got = net.forward_graphed(dcl.synth.make_batch(b, n, n, first=first))
        scr.add_(1.0)
        assert float((got["rot_pred"] - wants[first]["rot_pred"]).abs().max()) <= R_TOL
        assert float((got["trans_pred"] - wants[first]["trans_pred"]).abs().max()) <= T_TOL


def test_forward_routes_small_batches_through_the_graph(dcl):
    b, n = 2, 256
    cfg = dcl.synth.default_cfg(n, n)
    net = dcl.DCL_Net.Network(cfg, mode="test", graph_max_batch=4, graph_max_points=0)      # the batch rule alone
    net.load_state_dict(dcl.synth.synth_state_dict(net, 1))
    net = net.cuda().eval()
    plain, _, _ = _net(dcl, n, n, 1)
    for first in (0, 7):
        got = net(dcl.synth.make_batch(b, n, n, first=first))
        with torch.no_grad():
            want = plain(dcl.synth.make_batch(b, n, n, first=first))
        assert float((got["rot_pred"] - want["rot_pred"]).abs().max()) <= R_TOL
        assert float((got["trans_pred"] - want["trans_pred"]).abs().max()) <= T_TOL
    assert len(net._graphs) == 1
    net(dcl.synth.make_batch(6, n, n))                                       # above the limit: eager path
    assert len(net._graphs) == 1
    # the points rule: a default-constructed Network replays a graph for 12 crops x 512 points too (more crops than
    # graph_max_batch = 8), an async_inputs one too (a replayed small call beats the pipelined one), a graph_max_batch = 0 one does not
    for kw, graphs in (({}, 1), ({"async_inputs": True}, 1), ({"graph_max_batch": 0}, 0)):
        other = dcl.DCL_Net.Network(cfg, mode="test", **kw)
        other.load_state_dict(dcl.synth.synth_state_dict(other, 1))
        other = other.cuda().eval()
        got = other(dcl.synth.make_batch(12, n, n, first=3))
        with torch.no_grad():
            want = plain(dcl.synth.make_batch(12, n, n, first=3))
        assert float((got["rot_pred"] - want["rot_pred"]).abs().max()) <= R_TOL
        assert len(other.__dict__.get("_graphs", {})) == graphs, kw


def test_pipelined_calls_give_the_same_results(dcl):
    """async_inputs=True: back-to-back calls overlap on the GPU (sparse half of call k+1 under the dense half of call k);
    every call must still return exactly what a serial call returns"""
    n = 512
    cfg = dcl.synth.default_cfg(n, n)
    nets = {}
    for flag in (False, True):
        net = dcl.DCL_Net.Network(cfg, mode="test", async_inputs=flag, graph_max_batch=0)
        net.load_state_dict(dcl.synth.synth_state_dict(net, 1))
        nets[flag] = net.cuda().eval()
    dev = torch.device("cuda")

    def on_device(d):
        return {k: ({kk: (vv.to(dev) if torch.is_tensor(vv) else vv) for kk, vv in v.items()} if isinstance(v, dict)
                    else (v.to(dev) if torch.is_tensor(v) and k != "voxel_num_limit" else v)) for k, v in d.items()}
    batches = [on_device(dcl.synth.make_batch(b, n, n, first=f)) for b, f in ((8, 0), (3, 20), (16, 33), (8, 60), (1, 90))]
    torch.cuda.synchronize()
    outs = {}
    for flag in (False, True):
        with torch.no_grad():
            outs[flag] = [nets[flag](d) for _ in range(3) for d in batches]       # 15 calls in flight, no sync in between
        torch.cuda.synchronize()
    for a, c in zip(outs[False], outs[True]):
        for k in ("rot_pred", "trans_pred", "conf", "F_Xo_p"):
            assert torch.equal(a[k], c[k]), k


def test_chunked_sparse_half_and_stream_switches_give_the_same_results(dcl):
    """the batch-window backbone passes (pipeline_chunks: crops k*b/K .. of one occupied-voxel array, re-based per pass) and
    the single-stream mode must return what the default schedule returns"""
    n = 384
    cfg = dcl.synth.default_cfg(n, n)
    net = dcl.DCL_Net.Network(cfg, mode="test", graph_max_batch=0)
    net.load_state_dict(dcl.synth.synth_state_dict(net, 1))
    net = net.cuda().eval()
    data = dcl.synth.make_batch(8, n, n)
    with torch.no_grad():
        ref = net(data)
        outs = {}
        for name, attr, val in (("chunks2", "pipeline_chunks", 2), ("chunks4", "pipeline_chunks", 4),
                                ("single", "single_stream", True), ("single_paired", "single_stream", True)):
            old = getattr(net, attr)                   # the switches are constructor arguments (plain attributes): no environment
            setattr(net, attr, val)
            net._pair_features = False if name == "single" else None     # None: one stream -> grouped launches of both sides
            outs[name] = net(data)
            setattr(net, attr, old)
            net._pair_features = None
    # one stream: the same kernels in the same order -> identical bits.  Chunked passes have other row counts per launch,
    # hence other split-K / GEMM tilings (other summation orders): equal within the parity tolerance of the path
    for k in ("rot_pred", "trans_pred", "conf", "F_Xo_p"):
        assert torch.equal(ref[k], outs["single"][k]), k
    # (on one stream the default groups both backbones' layers into common launches: other tile decompositions, like chunks)
    for name in ("chunks2", "chunks4", "single_paired"):
        assert float((ref["rot_pred"] - outs[name]["rot_pred"]).abs().max()) <= 1e-4, name          # the path's parity bar
        assert float((ref["trans_pred"] - outs[name]["trans_pred"]).abs().max()) <= 1e-5, name
        assert float((ref["conf"] - outs[name]["conf"]).abs().max()) <= 1e-4, name
        scale = float(ref["F_Xo_p"].abs().max())
        assert float((ref["F_Xo_p"] - outs[name]["F_Xo_p"]).abs().max()) <= 1e-4 * max(1.0, scale), name


def test_graph_cache_is_bounded(dcl, monkeypatch):
    """one captured graph per batch size, capacity-sized buffers each: the cache keeps the most recently used ones only"""
    n = 128
    net, _, _ = _net(dcl, n, n, 1, graph_max_batch=8)
    monkeypatch.setattr(type(net), "MAX_GRAPHS", 3)
    outs = {}
    for b in (1, 2, 3, 1):
        outs[b] = net(dcl.synth.make_batch(b, n, n, first=b))
    assert [k[0] for k in net._graphs] == [2, 3, 1]
    # the cache is full: a new batch size runs launch by launch until it has been seen GRAPH_ADMIT (3) times -- an eval loop
    # whose crop count varies per image must not recapture on every call -- then it evicts the least recently used size
    for rep in range(2):
        outs[4] = net(dcl.synth.make_batch(4, n, n, first=4))
        assert [k[0] for k in net._graphs] == [2, 3, 1], rep
    third = net(dcl.synth.make_batch(4, n, n, first=4))
    assert [k[0] for k in net._graphs] == [3, 1, 4]
    assert float((third["rot_pred"] - outs[4]["rot_pred"]).abs().max()) <= R_TOL  # graph replay vs launch by launch: other GEMM tilings
    net(dcl.synth.make_batch(1, n, n, first=1))                                   # 1 touched again: 3 is the LRU now
    for _ in range(3):
        again = net(dcl.synth.make_batch(2, n, n, first=2))                       # evicted earlier -> admitted on the 3rd call
    assert [k[0] for k in net._graphs] == [4, 1, 2]
    assert float((again["rot_pred"] - outs[2]["rot_pred"]).abs().max()) <= R_TOL
    # a column-sliced (non-contiguous) resident input takes the copy_() staging instead of tripping pad_copy_many's asserts
    d = dcl.synth.make_batch(1, n, n, first=1)
    wide = torch.zeros((d["inp"]["feats"].shape[0], 9), device="cuda")
    wide[:, :7] = d["inp"]["feats"].cuda()
    for s_ in ("inp", "tmp"):
        for k in ("feats", "v2p_maps", "occupied_voxels"):
            d[s_][k] = d[s_][k].cuda()
    d["inp"]["feats"] = wide[:, :7]
    sliced = net(d)
    assert torch.equal(sliced["rot_pred"], outs[1]["rot_pred"])


def test_graph_cache_follows_the_weights(dcl):
    """a captured forward must not outlive the weights it was captured with; the model stays deep-copyable"""
    import copy
    b, n = 2, 256
    net, _, _ = _net(dcl, n, n, 1)
    data = dcl.synth.make_batch(b, n, n)
    first = net.forward_graphed(data)
    net.load_state_dict(dcl.synth.synth_state_dict(net, 2))                 # new weights -> graphs and folds dropped
    with torch.no_grad():
        want = net(dcl.synth.make_batch(b, n, n))
    got = net.forward_graphed(dcl.synth.make_batch(b, n, n))
    assert float((got["rot_pred"] - want["rot_pred"]).abs().max()) <= R_TOL
    assert float((got["rot_pred"] - first["rot_pred"]).abs().max()) > 1e-3   # really different weights
    twin = copy.deepcopy(net)
    with torch.no_grad():
        again = twin(dcl.synth.make_batch(b, n, n))
    assert float((again["rot_pred"] - want["rot_pred"]).abs().max()) <= 1e-6


def test_ops_refuse_cpu_tensors(dcl):
    with pytest.raises(RuntimeError):
        dcl.ops.voxelize_fp(torch.zeros(4, 7), torch.zeros(2, 3, dtype=torch.int32))
    cfg = dcl.synth.default_cfg(64, 64)
    net = dcl.DCL_Net.Network(cfg, mode="test").eval()        # not moved to the GPU
    with pytest.raises(RuntimeError):
        net(dcl.synth.make_batch(1, 64, 64))


@pytest.mark.gpu
def test_tail_side_by_side_equals_serial_tail(dcl):
    """the dense tail's two directions on two streams (launch by launch) / as two graph branches give the bits of the
    serial tail: the same kernels on the same operands, only placed differently (Network._tail_parallel chooses by shape)"""
    n, b = 256, 10
    cfg = dcl.synth.default_cfg(n, n)
    res = {}
    for par in (False, True):
        for path in ("eager", "graph"):
            net = dcl.DCL_Net.Network(cfg, mode="test", graph_max_batch=0)
            net.load_state_dict(dcl.synth.synth_state_dict(net, 1))
            net = net.cuda().eval()
            net.PAR_TAIL = par
            with torch.no_grad():
                for _ in range(2):                                          # the second call: warm caches, captured graph
                    out = net(dcl.synth.make_batch(b, n, n, first=5)) if path == "eager" else \
                        net.forward_graphed(dcl.synth.make_batch(b, n, n, first=5))
            res[par, path] = {k: out[k].clone() for k in ("rot_pred", "trans_pred", "conf")}
    torch.cuda.synchronize()
    for path in ("eager", "graph"):
        for k in ("rot_pred", "trans_pred", "conf"):
            assert torch.equal(res[False, path][k], res[True, path][k]), (path, k)



def test_plain_bench_line_and_dumped_outputs(dcl, tmp_path):
    """bench.py without --full: the headline line alone, `steps` timed steps (value x ms_per_step = frames per step), and
    --dump-outputs writes what the last timed forward returned -- the same poses as a forward of the same seeded crops here"""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    b, steps = 4, 3
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
           "--shape", "ref", "--batch", str(b), "--dump-outputs", str(tmp_path / "out")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == steps and line["value"] > 0 and line["ms_per_step"] > 0
    v, ms = line["value"], line["ms_per_step"]                           # rounded to 2 and 3 decimals
    assert abs(v * ms - 1e3 * b) <= 0.0005 * v + 0.005 * ms + 1e-6
    assert not {"roofline", "rccl", "ref_shape", "cpu_baseline"} & set(line), "a plain run measures the headline only"
    got = {k: np.load(str(tmp_path / "out" / (k + ".npy"))) for k in ("rot_pred", "trans_pred", "conf", "F_Xo_p")}
    assert all(v.dtype == np.float32 for v in got.values())
    net, _, _ = _net(dcl, 1024, 1024, 1)
    with torch.no_grad():
        want = net(dcl.synth.make_batch(b, 1024, 1024))
    _check({k: torch.from_numpy(got[k]) for k in ("rot_pred", "trans_pred", "conf")},
           want["rot_pred"].reshape(got["rot_pred"].shape).cpu().numpy(), want["trans_pred"].cpu().numpy(),
           want["conf"].cpu().numpy())


def test_two_gpu_bench_over_rccl_when_the_box_has_two():
    """the first multi-GPU run must be boring.  On a lease with >= 2 GPUs this starts bench.py the way the
    driver does (torch.distributed.run, one rank per GPU, RCCL) for 3 steps and checks what the collective library saw: world 2,
    backend nccl, two distinct devices, and a metric all-reduce that lost no frame (2 x 32).  Skipped on a 1-GPU lease -- there
    the only RCCL path ever exercised is world = 1 (profiles/r2_rccl_smoke_world1.log)."""
    import json
    import socket
    import subprocess
    import sys
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs (this lease has %d)" % torch.cuda.device_count())
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--full",
           "--no-extras", "--no-traffic"]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=root)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    line = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert line["n_gpus"] == 2 and line["scaling"] == "weak" and line["value"] > 0
    rc = line["rccl"]
    assert rc["world"] == 2 and rc["backend"] == "nccl" and rc["initialized"]
    assert len(set(rc["device_per_rank"])) == 2
    assert line["metric_frames_reduced"] == 64


def test_a_captured_forward_never_keeps_the_cross_queue_mode(dcl):
    """Network._select_capture (models/DCL_Net.py): a new whole-forward graph is timed against a one-stream capture of the same
    launches and replaced when it replays slower (its second branch dealt onto another hardware queue than the launch stream: 1.3-4x
    slower for as long as the graph lives).  Whatever the runtime's deal was, the capture that is kept replays within 10 % of the
    one-stream yardstick or faster, the record of the tries is kept on the entry, and re-capturing (new weights) goes through the
    same selection; results are those of the launch-by-launch forward."""
    import time
    n, b = 256, 3
    net = dcl.DCL_Net.Network(dcl.synth.default_cfg(n, n), mode="test")
    net.load_state_dict(dcl.synth.synth_state_dict(net, 1))
    net = net.cuda().eval()
    data = dcl.synth.make_batch(b, n, n, first=2)
    eager = dcl.DCL_Net.Network(dcl.synth.default_cfg(n, n), mode="test", graph_max_batch=0, graph_max_points=0)
    eager.load_state_dict(net.state_dict())
    eager = eager.cuda().eval()
    with torch.no_grad():
        want = eager(dcl.synth.make_batch(b, n, n, first=2))
    for _ in range(3):                                                   # three captures in one process: the deal moves on each time
        with torch.no_grad():
            out = net.forward_graphed(data)
            ent = next(iter(net._graphs.values()))
            tries = dict((k, v) for k, v in reversed(ent["capture_ms"]))    # first entry of each kind
            assert "one stream" in tries and len(ent["capture_ms"]) >= 2
            for _ in range(3):
                ent["graph"].replay()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(20):
                ent["graph"].replay()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) / 20 * 1e3
        assert ms <= 1.10 * tries["one stream"] + 0.02, (ms, ent["capture_ms"])
        assert float((out["rot_pred"] - want["rot_pred"]).abs().max()) <= 1e-4
        assert float((out["trans_pred"] - want["trans_pred"]).abs().max()) <= 1e-5
        net._invalidate()
