"""The device-resident evaluation tables on the GPU (csrc/metric_table.hip): the trajectory distances have ops.add_s's bits pose
by pose, the tabulation kernel the host twin's bits on every edge case, the fused per-frame entry is two launches and equals its
two halves, a frame is added without a host synchronisation, and a builder -> stage-2 chain -> table run over synthetic frames
equals the host table fed per-frame read-backs."""
import numpy as np
import pytest
import torch

import metric_table_cases as MC

pytestmark = pytest.mark.gpu


def _cuda(p):
    return {k: v.cuda() for k, v in p.items()}


def _same(a, b):
    return MC.bits(a) == MC.bits(b)


# ------------------------------------------------------------------------------------------- 1. trajectory distances
@pytest.mark.parametrize("P", [1, 255, 256, 257, 513])
@pytest.mark.parametrize("T,b", [(1, 1), (3, 2), (3, 7), (4, 2), (5, 7)])       # (4, 5: a second group of one / two poses)
def test_trajectory_distances_have_add_s_bits_pose_by_pose(dcl, P, T, b):
    p = _cuda(MC.pose_case(100 + P + b, T, b, P, 5))
    own = p["cld"][p["cls"].long()].contiguous()                                   # without cls: cloud i for crop i
    for kw, ref_kw in ((dict(mode="adds"), dict(mode="adds")), (dict(mode="add"), dict(mode="add")),
                       (dict(sym_flag=p["sym"]), dict(sym_flag=p["sym"]))):
        for cld, cls in ((p["cld"], p["cls"]), (own, None)):
            got = dcl.ops.add_traj(cld, p["Rp"], p["tp"], p["Rg"], p["tg"], cls=cls, **kw)
            assert tuple(got.shape) == (T, b) and got.dtype == torch.float32
            for t in range(T):
                want = dcl.ops.add_s(cld, p["Rp"][t], p["tp"][t], p["Rg"], p["tg"], cls=cls, **ref_kw)
                assert _same(got[t], want), (kw.keys(), cls is None, t)
    one = dcl.ops.add_traj(p["cld"], p["Rp"][0], p["tp"][0], p["Rg"], p["tg"], cls=p["cls"])              # (b,3,3): one step
    assert tuple(one.shape) == (b,) and _same(one, dcl.ops.add_s(p["cld"], p["Rp"][0], p["tp"][0], p["Rg"], p["tg"], cls=p["cls"]))


def test_invalid_crops_get_inf_and_their_poses_are_not_read(dcl):
    T, b, P = 3, 7, 257
    p = _cuda(MC.pose_case(7, T, b, P, 4))
    valid = torch.tensor([1, 0, 1, 1, 0, 1, 0], dtype=torch.int32).cuda()
    keep = valid.bool()
    full = dcl.ops.add_traj(p["cld"], p["Rp"], p["tp"], p["Rg"], p["tg"], cls=p["cls"])
    out, scratch = torch.full((T, b), -1.0).cuda(), torch.empty(T, b, 2).cuda()
    got = dcl.ops.add_traj(p["cld"], p["Rp"], p["tp"], p["Rg"], p["tg"], cls=p["cls"], valid=valid, out=out, scratch=scratch)
    assert got.data_ptr() == out.data_ptr()
    assert torch.isposinf(got[:, ~keep]).all() and _same(got[:, keep], full[:, keep])
    # NaN poses, NaN ground truth and a cloud index far out of range on the invalid crops: every other output unchanged
    Rp, tp, Rg, tg, cls = (x.clone() for x in (p["Rp"], p["tp"], p["Rg"], p["tg"], p["cls"]))
    Rp[:, ~keep], tp[:, ~keep], Rg[~keep], tg[~keep] = float("nan"), float("nan"), float("nan"), float("nan")
    cls[~keep] = 1 << 30
    again = dcl.ops.add_traj(p["cld"], Rp, tp, Rg, tg, cls=cls, valid=valid)
    assert _same(again, got)
    # a cloud index outside [0, n_clouds) on a VALID crop reads no cloud: +inf, the rest unchanged
    cls2 = p["cls"].clone()
    cls2[0], cls2[2] = -1, 4
    oob = dcl.ops.add_traj(p["cld"], p["Rp"], p["tp"], p["Rg"], p["tg"], cls=cls2)
    assert torch.isposinf(oob[:, [0, 2]]).all() and _same(oob[:, [1, 3, 4, 5, 6]], full[:, [1, 3, 4, 5, 6]])
    none = dcl.ops.add_traj(p["cld"], p["Rp"], p["tp"], p["Rg"], p["tg"], cls=p["cls"], valid=torch.zeros_like(valid))
    assert torch.isposinf(none).all()


def test_trajectory_distances_match_the_reference_expression(dcl):
    """the harness expression (tools/test_YCBV_stage1.py:186-189) in fp64 per pose, at the class clouds' 2620 points; the
    tolerance of test_gpu_ops.test_add_s_matches_reference_expression"""
    T, b, P = 3, 5, 2620
    p = MC.pose_case(3, T, b, P, 7)
    d = _cuda(p)
    got = dcl.ops.add_traj(d["cld"], d["Rp"], d["tp"], d["Rg"], d["tg"], cls=d["cls"]).cpu().double()
    cur = p["cld"][p["cls"].long()].double()
    gt = torch.bmm(cur, p["Rg"].double().transpose(1, 2)) + p["tg"].double().unsqueeze(1)
    for t in range(T):
        pred = torch.bmm(cur, p["Rp"][t].double().transpose(1, 2)) + p["tp"][t].double().unsqueeze(1)
        want = torch.mean(torch.min(torch.norm(pred.unsqueeze(2) - gt.unsqueeze(1), dim=3), 2)[0], dim=1)
        assert float((got[t] - want).abs().max()) <= 1e-6
        assert _same(got[t].float(), dcl.ops.add_s(d["cld"], d["Rp"][t], d["tp"][t], d["Rg"], d["tg"], cls=d["cls"]))


# ------------------------------------------------------------------------------------------- 2. tabulation
def test_tabulation_kernel_equals_the_host_twin_on_every_edge_case(dcl):
    for case in MC.edge_cases():
        host = MC.new_arrays(dcl, case)
        dis, cls, valid, diam = MC.tensors(case)
        dcl.ops.metric_tabulate_host(host, dis, cls, valid, mode=case["mode"], diameter=diam)
        runs = []
        for _ in range(2):                                                        # a second identical run: the same bits
            dev = MC.new_arrays(dcl, case, "cuda")
            ddis, dcls, dvalid, ddiam = MC.tensors(case, "cuda")
            dcl.ops.metric_tabulate(dev, ddis, dcls, dvalid, mode=case["mode"], diameter=ddiam)
            dcl.ops.metric_tabulate(dev, ddis, dcls, dvalid, mode=case["mode"], diameter=ddiam)   # accumulates onto itself
            runs.append(dev)
        dcl.ops.metric_tabulate_host(host, dis, cls, valid, mode=case["mode"], diameter=diam)
        for dev in runs:
            for k in ("sums", "maxd", "counts", "bad"):
                assert (dev[k] is None) == (host[k] is None) and (dev[k] is None or _same(dev[k], host[k])), (case["name"], k)


def test_more_crops_than_one_staged_chunk(dcl):
    """b = 2500: the kernel stages crops 1024 at a time; the order of sum D runs across the chunks"""
    g = torch.Generator().manual_seed(1)
    b, C, T = 2500, 21, 2
    dis = (torch.rand(T, b, generator=g) * 0.12).float()
    cls = torch.randint(0, C, (b,), generator=g).int()
    valid = (torch.rand(b, generator=g) > 0.1).int()
    for mode in MC.MODES:
        diam = torch.from_numpy(MC.diameters(C))
        host, dev = dcl.ops.metric_table_arrays(mode, T, C), dcl.ops.metric_table_arrays(mode, T, C, "cuda")
        dcl.ops.metric_tabulate_host(host, dis, cls, valid, mode=mode, diameter=diam)
        dcl.ops.metric_tabulate(dev, dis.cuda(), cls.cuda(), valid.cuda(), mode=mode, diameter=diam.cuda())
        for k in ("sums", "maxd", "counts", "bad"):
            assert dev[k] is None or _same(dev[k], host[k]), (mode, k)


# ------------------------------------------------------------------------------------------- 3. the fused per-frame entry
def _tables(dcl, mode, C, T, device="cuda"):
    S = dcl.sharding
    if mode == "adds":
        return S.DeviceAddsTable(C, T, device)
    return (S.DeviceLmTable if mode == "lm" else S.DeviceLmoTable)(np.linspace(0.01, 0.2, C), T, device)


@pytest.mark.parametrize("mode", MC.MODES)
@pytest.mark.parametrize("T,b,P,C", [(1, 1, 1, 1), (3, 7, 257, 21), (3, 2, 513, 65), (1, 7, 255, 130)])
def test_add_frame_equals_add_traj_then_metric_tabulate_in_two_launches(request, dcl, mode, T, b, P, C):
    import test_gpu_ops as TO
    from test_kernel_census import census
    lib = TO.enter_diag(dcl, request)
    n_clouds = min(C, 6)
    p = _cuda(MC.pose_case(11 + b, T, b, P, n_clouds))
    valid = (torch.arange(b) % 3 != 1).int().cuda() if b > 1 else None
    sym = p["sym"] if mode != "adds" else None
    tab, want = _tables(dcl, mode, C, T), _tables(dcl, mode, C, T)
    for frame in range(2):                                                        # the second call reuses the first one's scratch
        lib.dcl_debug_launch_census_reset()
        tab.add_frame(p["cld"], p["cls"], p["Rp"], p["tp"], p["Rg"], p["tg"], valid=valid, sym_flag=sym)
        seen = census(lib)
        assert sum(seen.values()) == 2 and set(seen) == {"k_adds_traj_partial", "k_metric_tabulate"}, seen
        kw = dict(sym_flag=sym) if sym is not None else dict(mode="adds" if mode == "adds" else "add")
        dis = dcl.ops.add_traj(p["cld"], p["Rp"], p["tp"], p["Rg"], p["tg"], cls=p["cls"], valid=valid, **kw)
        dcl.ops.metric_tabulate(want.arrays, dis, p["cls"], valid, mode=mode, diameter=want.diameter)
    assert len(tab._buffers) == 1
    for k in ("sums", "maxd", "counts", "bad"):
        assert tab.arrays[k] is None or _same(tab.arrays[k], want.arrays[k]), k
    assert int(tab.bad.cpu()[0]) == 0
    # the fused entry can hand the distances out as well; per-crop clouds (cloud i for crop i) give the same table
    out = torch.empty(T, b).cuda()
    own = p["cld"][p["cls"].long()].contiguous()
    t2 = _tables(dcl, mode, C, T)
    dcl.ops.add_tabulate(t2.arrays, own, p["cls"], p["Rp"], p["tp"], p["Rg"], p["tg"], valid=valid, sym_flag=sym,
                         metric="adds" if mode == "adds" else "add", mode=mode, diameter=t2.diameter, out=out)
    assert _same(out, dis)
    t2.add_frame(own, p["cls"], p["Rp"], p["tp"], p["Rg"], p["tg"], valid=valid, sym_flag=sym, per_crop=True)
    for k in ("sums", "maxd", "counts"):
        assert tab.arrays[k] is None or _same(tab.arrays[k], t2.arrays[k]), k


def test_a_cloud_index_out_of_range_is_a_miss_and_raises_bad(dcl):
    T, b, P = 2, 3, 40
    p = _cuda(MC.pose_case(2, T, b, P, 4))
    cls = torch.tensor([1, 7, 2], dtype=torch.int32).cuda()                        # 7: a class of the table, but no cloud 7
    tab = dcl.sharding.DeviceAddsTable(21, T, "cuda")
    tab.add_frame(p["cld"], cls, p["Rp"], p["tp"], p["Rg"], p["tg"])
    assert int(tab.bad.cpu()[0]) == 1 and tab.sums[:, 7].cpu().tolist() == [[1.0, 0.0, 0.0, 0.0]] * T
    with pytest.raises(ValueError, match="class id"):
        tab.finalize()


# ------------------------------------------------------------------------------------------- 4. no synchronisation
def test_frames_are_added_without_a_host_synchronisation(dcl, monkeypatch):
    from test_gpu_crops_device_draws import SyncCount, _sync_debug_is_honoured
    T, b, P = 3, 7, 257
    p = _cuda(MC.pose_case(9, T, b, P, 5))
    valid = (torch.arange(b) % 3 != 1).int().cuda()
    dis = dcl.ops.add_traj(p["cld"], p["Rp"], p["tp"], p["Rg"], p["tg"], cls=p["cls"])
    tabs = [_tables(dcl, m, 21, T) for m in MC.MODES]
    for tab in tabs:                                                              # warm-up: the scratch of this (b, P)
        tab.add_frame(p["cld"], p["cls"], p["Rp"], p["tp"], p["Rg"], p["tg"], valid=valid)
        tab.add_distances(p["cls"], dis, valid)
    torch.cuda.synchronize()
    honoured = _sync_debug_is_honoured()
    count = SyncCount(monkeypatch)
    if honoured:
        torch.cuda.set_sync_debug_mode("error")
    try:
        for tab in tabs:
            tab.add_frame(p["cld"], p["cls"], p["Rp"], p["tp"], p["Rg"], p["tg"], valid=valid)
            tab.add_distances(p["cls"], dis, valid)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert count.calls == [], count.calls
    tabs[0].finalize()
    assert count.calls == ["cpu"], count.calls                                    # the one read-back
    monkeypatch.undo()
    print("torch.cuda.set_sync_debug_mode('error') honoured: %s" % honoured)


# ------------------------------------------------------------------------------------------- 5. end to end
def test_builder_to_stage2_chain_to_table_equals_per_frame_read_backs(dcl):
    from test_gpu_refine_loop import _refiner
    # (N = M = 1024: the device-composed refine loop takes one confidence per point out of conf[:, :1024])
    CFG = dict(input_size=1024, tmp_size=1024, unit_voxel_extent=[0.006] * 3, voxel_num_limit=[64] * 3, voxelization_mode=4)
    n, iteration = CFG["tmp_size"], 2
    frames = [dcl.synth.make_frame(700 + i, n_obj=3, tmp_size=n, empty=i % 3) for i in range(4)]
    builder = dcl.crops.CropBuilder(CFG, frames[0]["cad_pts"], frames[0]["cad_col"], device=torch.device("cuda"), draws="device",
                                    capacity=True, template_ids=True, draw_seed=2)
    net = dcl.DCL_Net.Network(dcl.synth.default_cfg(n, n), mode="test")
    net.load_state_dict(dcl.synth.synth_state_dict(net, 1))
    net, ref = net.cuda().eval(), _refiner(dcl)
    net.cache_templates(builder.templates(), CFG["voxel_num_limit"])
    table = dcl.sharding.DeviceAddsTable(22, steps=iteration + 1, device="cuda")
    hosts = [dcl.sharding.AddsTable(22) for _ in range(iteration + 1)]
    n_invalid = 0
    for f in frames:
        im, de, la = dcl.crops.CropBuilder.resident(f["img"], f["depth"], f["label"], torch.device("cuda"))
        data = builder.build(im, de, la, f["rois"], f["gt_obj"], poses=f["poses"])
        rot, trans, pred, (rots, transs) = dcl.refiner.stage2_chain(net, ref, data, iteration, graph=False, compose="device",
                                                                     trajectory=True)
        b = rots.shape[1]
        cld = data["labels"]["points_tmp"].reshape(b, n, 3)
        gt = (data["labels"]["rot_gt"], data["labels"]["trans_gt"])
        table.add_frame(cld, data["tmp_cls"], rots, transs, gt[0], gt[1], valid=data["valid"], per_crop=True)
        # the host form: every step's distances and the flags read back per frame
        valid, cls = data["valid"].cpu().tolist(), data["tmp_cls"].cpu().tolist()
        n_invalid += valid.count(0)
        for t in range(iteration + 1):
            d = dcl.ops.add_s(cld, rots[t], transs[t], gt[0], gt[1]).cpu().tolist()
            for i in range(b):
                hosts[t].add(int(cls[i]), float(d[i]) if valid[i] else float("inf"))
    assert n_invalid == 4                                                         # one empty mask per frame
    for t in range(iteration + 1):
        got = table.to_host(t)
        assert _same(got.sums, hosts[t].sums) and _same(got.maxd, hosts[t].maxd), t
        assert got.finalize()[:2] == hosts[t].finalize()[:2]
    assert float(table.sums[:, :, 0].sum().cpu()) == 3 * 12                        # every crop counted at every step
    assert table.finalize()[:2] == hosts[-1].finalize()[:2]
