"""CropBuilder(draws="device"): a frame from images to `data` without a host synchronisation, every candidate kept and marked by
data["valid"], the draws those of ops.crop_draw_host; the same crops as the default form once its draws are replaced by the
device picks; the LineMOD builders; the network and ADD-S on the device-form data."""
import numpy as np
import pytest
import torch

from crop_scene import make_scene

pytestmark = pytest.mark.gpu

CFG = dict(input_size=256, tmp_size=256, unit_voxel_extent=[0.006] * 3, voxel_num_limit=[64] * 3, voxelization_mode=4)
R_TOL, T_TOL = 1e-4, 1e-5
_SIDE = ("feats", "coords", "occupied_voxels", "p2v_maps", "v2p_maps")


def _scene(seed=41, **kw):
    """two good instances, one with an empty mask, one without a detection (unless overridden)"""
    kw = dict(dict(n_obj=4, empty=2, undetected=3), **kw)
    sc = make_scene(seed, tmp_size=CFG["tmp_size"], **kw)
    for c in sc["cad_pts"]:
        sc["cad_pts"][c] = sc["cad_pts"][c] * 0.8
    return sc


def _args(dcl, sc, resident=True):
    fr = dcl.crops.CropBuilder.resident(sc["img"], sc["depth"], sc["label"]) if resident else (sc["img"], sc["depth"], sc["label"])
    return fr + (sc["rois"], sc["gt_obj"])


def _builder(dcl, sc, **kw):
    return dcl.crops.CropBuilder(CFG, sc["cad_pts"], sc["cad_col"], **kw)


class SyncCount(object):
    """counts the calls that bring a CUDA tensor's contents to the host: Tensor.cpu / item / tolist / numpy / __bool__"""
    NAMES = ("cpu", "item", "tolist", "numpy", "__bool__")

    def __init__(self, monkeypatch):
        self.calls = []
        for name in self.NAMES:
            real = getattr(torch.Tensor, name)

            def patched(t, *a, _real=real, _name=name, **k):
                if t.is_cuda:
                    self.calls.append(_name)
                return _real(t, *a, **k)
            monkeypatch.setattr(torch.Tensor, name, patched)


def _sync_debug_is_honoured():
    probe = torch.ones(1, device="cuda")
    torch.cuda.set_sync_debug_mode("error")
    try:
        probe.item()
    except RuntimeError:
        return True
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return False


def _replay_picks(monkeypatch, dcl, rows):
    """np.random.choice and ops.legacy_choice_heads hand out `rows` (the device picks) in the order the loader draws"""
    rows = [np.asarray(r) for r in rows]

    def heads(ms, n):
        out = [rows.pop(0) for _ in ms]
        assert all(len(r) == n and r.max() < m for r, m in zip(out, ms))
        return np.stack(out)

    def choice(m, n):
        r = rows.pop(0)
        assert len(r) == n and r.max() < m
        return r
    monkeypatch.setattr(dcl.ops, "legacy_choice_heads", heads)
    monkeypatch.setattr(np.random, "choice", choice)
    return rows


# ------------------------------------------------------------------------------------------- 1. the builder
def test_a_frame_is_built_without_a_host_synchronisation(dcl, monkeypatch):
    sc = _scene()
    args = _args(dcl, sc)
    dev_b = _builder(dcl, sc, draws="device", capacity=True, template_ids=True, draw_seed=5)
    host_b = _builder(dcl, sc, capacity=True, template_ids=True)
    dev_b.build(*args, poses=sc["poses"])                       # (first call: the voxelisation's persistent words are made)
    host_b.build(*args, poses=sc["poses"])
    torch.cuda.synchronize()
    honoured = _sync_debug_is_honoured()
    count = SyncCount(monkeypatch)
    if honoured:
        torch.cuda.set_sync_debug_mode("error")
    try:
        data = dev_b.build(*args, poses=sc["poses"])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert count.calls == [], count.calls
    host_b.build(*args, poses=sc["poses"])
    assert count.calls == ["cpu"], count.calls                  # the default form: the counts, and nothing else
    monkeypatch.undo()
    print("torch.cuda.set_sync_debug_mode('error') honoured: %s" % honoured)
    b = 3
    assert data["valid"].is_cuda and data["valid"].dtype == torch.int32 and data["valid"].tolist() == [1, 1, 0]
    assert data["counts"].is_cuda and tuple(data["counts"].shape) == (b, 3)
    assert data["picks"].is_cuda and tuple(data["picks"].shape) == (b, CFG["input_size"]) and data["picks"].dtype == torch.int64
    assert data["all_flags"].tolist() == [1, 1, 1, 0] and not data["all_flags"].is_cuda       # candidates, on the host
    assert data["inp"]["feats"].shape[0] == b * CFG["input_size"] and data["tmp_cls"].tolist() == sc["gt_obj"][:3].tolist()
    assert int(data["inp"]["vi_info"][2]) == 0
    want, want_valid = dcl.ops.crop_draw_host(data["counts"].cpu().numpy(), CFG["input_size"], 5, 1, min_valid=32, keep_sparse=True)
    assert np.array_equal(data["picks"].cpu().numpy(), want) and want_valid.tolist() == [1, 1, 0]


def test_device_form_rows_equal_the_default_form_with_the_same_picks(dcl, monkeypatch):
    sc = _scene()
    args = _args(dcl, sc, resident=False)
    n = CFG["input_size"]
    for kw in (dict(capacity=True), dict(capacity=False, template_ids=True)):
        dev_d = _builder(dcl, sc, draws="device", draw_seed=3, **kw).build(*args, poses=sc["poses"])
        picks = dev_d["picks"].cpu().numpy()
        left = _replay_picks(monkeypatch, dcl, picks[:2])
        host_d = _builder(dcl, sc, **kw).build(*args, poses=sc["poses"])
        monkeypatch.undo()
        assert not left and host_d["all_flags"].tolist() == [1, 1, 0, 0]
        assert np.array_equal(host_d["counts"], dev_d["counts"].cpu().numpy()[:2])
        if kw["capacity"]:
            V = int(host_d["inp"]["vi_info"][0])
            assert int(dev_d["inp"]["vi_info"][0]) == V + n and int(dev_d["inp"]["vi_info"][2]) == 0      # + one voxel per dummy point
        else:
            V = host_d["inp"]["occupied_voxels"].shape[0]
            assert dev_d["inp"]["occupied_voxels"].shape[0] == V + n
        ma = min(host_d["inp"]["v2p_maps"].shape[1], dev_d["inp"]["v2p_maps"].shape[1])
        for k in ("feats", "coords", "p2v_maps"):
            assert torch.equal(dev_d["inp"][k][:2 * n], host_d["inp"][k][:2 * n]), k
        assert torch.equal(dev_d["inp"]["occupied_voxels"][:V], host_d["inp"]["occupied_voxels"][:V])
        assert torch.equal(dev_d["inp"]["v2p_maps"][:V, :ma], host_d["inp"]["v2p_maps"][:V, :ma])
        for k in ("rot_gt", "trans_gt"):
            assert torch.equal(dev_d["labels"][k][:2], host_d["labels"][k]), k
        assert torch.equal(dev_d["all_centroids"][:2], host_d["all_centroids"])
        if "tmp" in dev_d:
            assert torch.equal(dev_d["tmp"]["feats"][:2 * CFG["tmp_size"]], host_d["tmp"]["feats"])


def test_draw_frame_advances_and_a_reset_repeats_the_frame(dcl):
    sc = _scene()
    args = _args(dcl, sc)
    builder = _builder(dcl, sc, draws="device", capacity=True, draw_seed=9)
    assert builder.draw_frame == 0 and builder.draws == "device"
    state = np.random.get_state()[1].copy()
    first = builder.build(*args)
    assert builder.draw_frame == 1
    second = builder.build(*args)
    assert builder.draw_frame == 2 and not torch.equal(first["picks"], second["picks"])
    assert np.array_equal(np.random.get_state()[1], state)              # nothing of np.random is consumed
    builder.draw_frame = 0
    again = builder.build(*args)
    assert builder.draw_frame == 1 and torch.equal(again["picks"], first["picks"])
    for k in _SIDE:
        assert torch.equal(again["inp"][k], first["inp"][k]), k
    other = _builder(dcl, sc, draws="device", capacity=True, draw_seed=10).build(*args)
    assert not torch.equal(other["picks"], first["picks"])
    assert _builder(dcl, sc).draws == "host"
    for bad in ("x", None, "Device"):
        with pytest.raises(ValueError, match="draws"):
            _builder(dcl, sc, draws=bad)


def test_prefetcher_yields_the_serial_loops_crops(dcl):
    scenes = [_scene(50 + i, n_obj=3, empty=None if i else 1, undetected=None) for i in range(3)]
    builder = _builder(dcl, scenes[0], draws="device", capacity=True, draw_seed=2)
    order = [0, 1, 2, 1, 0]
    args = lambda i: _args(dcl, scenes[i], resident=False)  # noqa: E731
    want = [builder.build(*args(i)) for i in order]
    torch.cuda.synchronize()
    builder.draw_frame = 0
    n = 0
    with dcl.crops.CropPrefetcher(builder, (args(i) for i in order), depth=2) as feed:
        for got, ref in zip(feed, want):
            for k in _SIDE:
                assert torch.equal(got["inp"][k], ref["inp"][k]), (n, k)
            assert torch.equal(got["valid"], ref["valid"]) and torch.equal(got["picks"], ref["picks"])
            n += 1
    assert n == len(order) and builder.draw_frame == len(order)
    assert want[0]["valid"].tolist() == [1, 0, 1] and want[1]["valid"].tolist() == [1, 1, 1]


# ------------------------------------------------------------------------------------------- 2. the LineMOD builders
def _lm_case(seed, small=False):
    cfg = dict(CFG, unit_voxel_extent=[0.005] * 3)
    sc = make_scene(seed, n_obj=1, tmp_size=cfg["tmp_size"], tiny=0 if small else None)
    cls = int(sc["gt_obj"][0])
    mask = sc["label"] == cls
    depth = (sc["depth"].astype(np.float64) / 10).astype(np.uint16)
    ys, xs = np.nonzero(mask)
    bb = [int(xs.min()) - 3, int(ys.min()) - 2, int(xs.max() - xs.min()) + 7, int(ys.max() - ys.min()) + 5]
    return cfg, sc, cls, mask, depth, bb


@pytest.mark.parametrize("which", ["lm", "lm_eval", "lm_mask_box", "lmo"])
def test_lm_builders_never_return_none_and_say_valid(dcl, monkeypatch, which):
    cfg, sc, cls, mask, depth, bb = _lm_case(61)
    mk = lambda **kw: dcl.crops.CropBuilder(cfg, sc["cad_pts"], sc["cad_col"], camera=dcl.crops.LM_CAMERA, **kw)  # noqa: E731

    def build(b, mask_, depth_=depth):
        if which == "lmo":
            return b.build_lmo(sc["img"], depth_, mask_, cls)
        return b.build_lm(sc["img"], depth_, mask_, None if which == "lm_mask_box" else bb, cls, which != "lm")
    dev_b = mk(draws="device", draw_seed=4)
    seen, real_draw = {}, dcl.ops.crop_draw

    def spy(counts, *a, **k):
        seen["counts"] = counts
        seen["picks"], seen["valid"] = real_draw(counts, *a, **k)
        return seen["picks"], seen["valid"]
    monkeypatch.setattr(dcl.ops, "crop_draw", spy)
    good = build(dev_b, mask)
    monkeypatch.undo()
    assert len(good) == 6 and good[5].is_cuda and good[5].dtype == torch.int32 and good[5].tolist() == [1]
    assert dev_b.draw_frame == 1
    picks = seen["picks"].cpu().numpy()
    assert np.array_equal(picks, dcl.ops.crop_draw_host(seen["counts"].cpu().numpy(), cfg["input_size"], 4, 0, min_valid=0)[0])
    # the same sample from the default form, its draw replaced by the device picks
    host_b = mk()
    left = _replay_picks(monkeypatch, dcl, picks)
    want = build(host_b, mask)
    monkeypatch.undo()
    assert want is not None and not left
    for g, w in zip(good[:5], want):
        assert torch.equal(g, w)
    # an empty mask: the default form returns None, the device form a lattice dummy with valid = 0
    empty = build(dev_b, np.zeros_like(mask))
    assert build(host_b, np.zeros_like(mask)) is None
    assert empty[5].tolist() == [0] and tuple(empty[0].shape) == (cfg["input_size"], 7) and torch.isfinite(empty[0]).all()
    j = np.arange(cfg["input_size"])
    assert np.array_equal(empty[1].cpu().numpy(), np.stack([j % 64, (j // 64) % 64, j // 4096], 1))


def test_lm_valid_follows_the_min_valid_rule(dcl):
    """a tiny mask: at most 128 points inside the grid -- LineMOD's test mode gives the dummy, its eval mode keeps the sample"""
    cfg, sc, cls, mask, depth, bb = _lm_case(34, small=True)
    host_b = dcl.crops.CropBuilder(cfg, sc["cad_pts"], sc["cad_col"], camera=dcl.crops.LM_CAMERA)
    dev_b = dcl.crops.CropBuilder(cfg, sc["cad_pts"], sc["cad_col"], camera=dcl.crops.LM_CAMERA, draws="device")
    assert host_b.build_lm(sc["img"], depth, mask, bb, cls, False) is None
    assert dev_b.build_lm(sc["img"], depth, mask, bb, cls, False)[5].tolist() == [0]
    kept = dev_b.build_lm(sc["img"], depth, mask, bb, cls, True)
    assert (host_b.build_lm(sc["img"], depth, mask, bb, cls, True) is not None) == bool(kept[5].tolist()[0])
    assert dev_b.draw_frame == 2


# ------------------------------------------------------------------------------------------- 3. end to end
def _network(dcl):
    net = dcl.DCL_Net.Network(dcl.synth.default_cfg(CFG["input_size"], CFG["tmp_size"]), mode="test")       # default routing: graph replay
    net.load_state_dict(dcl.synth.synth_state_dict(net, 1))
    return net.cuda().eval()


def _adds(dcl, data, pred):
    b = pred["rot_pred"].shape[0]
    cld = data["tmp"]["feats"][:, 4:7].reshape(b, CFG["tmp_size"], 3)
    return dcl.sharding.add_s(cld, pred["rot_pred"], pred["trans_pred"], data["labels"]["rot_gt"], data["labels"]["trans_gt"])


def test_network_on_device_form_data(dcl, monkeypatch):
    net = _network(dcl)
    # (a) no empty mask: the device form's data IS the default form's data under the same picks -> the same bits
    sc = _scene(43, n_obj=3, empty=None, undetected=None)
    args = _args(dcl, sc)
    dev_d = _builder(dcl, sc, draws="device", capacity=True, draw_seed=1).build(*args, poses=sc["poses"])
    assert dev_d["valid"].tolist() == [1, 1, 1]
    _replay_picks(monkeypatch, dcl, dev_d["picks"].cpu().numpy())
    host_d = _builder(dcl, sc, capacity=True).build(*args, poses=sc["poses"])
    monkeypatch.undo()
    for side in ("inp", "tmp"):
        for k in _SIDE:
            assert torch.equal(dev_d[side][k], host_d[side][k]), (side, k)
    assert torch.equal(dev_d["inp"]["vi_info"], host_d["inp"]["vi_info"])
    with torch.no_grad():
        want = net(host_d)
        got = net(dev_d)
    assert net.replays_graph(3) and len(net._graphs) == 1
    for k in ("rot_pred", "trans_pred", "conf"):
        assert torch.equal(got[k], want[k]), k
    assert torch.equal(_adds(dcl, dev_d, got), _adds(dcl, host_d, want))
    # (b) a dummy crop in the batch: finite everywhere, the pitch flag down, the good crops as in the default form's batch of two
    sc = _scene()
    args = _args(dcl, sc)
    dev_d = _builder(dcl, sc, draws="device", capacity=True, draw_seed=1).build(*args, poses=sc["poses"])
    _replay_picks(monkeypatch, dcl, dev_d["picks"].cpu().numpy()[:2])
    host_d = _builder(dcl, sc, capacity=True).build(*args, poses=sc["poses"])
    monkeypatch.undo()
    with torch.no_grad():
        want = net(host_d)
        got = net(dev_d)
    assert got["rot_pred"].shape[0] == 3 and want["rot_pred"].shape[0] == 2
    for k in ("rot_pred", "trans_pred", "conf"):
        assert torch.isfinite(got[k]).all(), k
    assert int(dev_d["inp"]["vi_info"][2]) == 0 and int(got["crop_overflow"][0]) == 0
    dR = float((got["rot_pred"][:2] - want["rot_pred"]).abs().max())
    dt = float((got["trans_pred"][:2] - want["trans_pred"]).abs().max())
    print("good crops beside a dummy crop: |dR| %.3g (tol %.0e)  |dt| %.3g (tol %.0e)" % (dR, R_TOL, dt, T_TOL))
    assert dR <= R_TOL and dt <= T_TOL
    # ADD-S masked by `valid`, read together with the results: the default form's distances of the good crops
    dist, valid = _adds(dcl, dev_d, got), dev_d["valid"]
    both = torch.cat([dist, valid.float()]).cpu()                                       # one read-back
    d_dev, v = both[:3], both[3:] > 0
    d_host = _adds(dcl, host_d, want).cpu()
    assert v.tolist() == [True, True, False]
    err = float((d_dev[v] - d_host).abs().max())
    # a point moves by at most |dR|_F r + |dt|_2 <= 3 R_TOL r + sqrt(3) T_TOL (r = the template's radius: 0.8 * 90 mm * sqrt(3)
    # < 0.125 m), so does a mean of nearest-point distances; + 1e-6 for the float32 rounding of the distances themselves
    cap = 3 * R_TOL * 0.125 + 3 ** 0.5 * T_TOL + 1e-6
    print("ADD-S of the good crops: max difference %.3g (cap %.3g)" % (err, cap))
    assert err <= cap
