"""The training loader's front end on the device (csrc/crops_train.hip, crops.py::CropBuilder.build_train).

Kernels against their host twins, bit for bit: the per-frame class table, and the posed crop points on crops of 1, 4095, 4096
and 4097 masked pixels (the chunk size of the crop kernels is 4096), with the identity pose, a pose with zero jitter and
random poses, two cameras and several frames in one call.  `build_train` against the reference loader's outputs
(tests/golden/train_crops_ref.npz) to the rules of tests/test_train_crops_abi.py: everything the reference computes without a
BLAS product is equal; the re-posed coordinates lie within the derived bound and equal the host twin's bits; voxel rows may
differ only at points within that bound of a voxel border."""
import os
import warnings

import numpy as np
import pytest
import torch

import train_scene as TS
from test_train_crops_abi import ROT_BOUND, numpy_table, scene_frames, table_cases

pytestmark = pytest.mark.gpu

HALF = TS.CFG["unit_voxel_extent"][0] * TS.CFG["voxel_num_limit"][0] * 0.5
UNIT = TS.CFG["unit_voxel_extent"][0]
RGB_MEAN = (0.485, 0.456, 0.406)


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "train_crops_ref.npz"))


def cuda_frames(lab, dep):
    return torch.from_numpy(lab).cuda(), torch.from_numpy(dep.view(np.int16)).cuda()


# ------------------------------------------------------------------------------------------------------------ label table
def test_label_table_equals_the_host_twin(dcl):
    cases = table_cases()                                            # n = 1 and 3 at 37 x 70: tails in both directions
    lab, dep = scene_frames()                                        # 480 x 640
    cases += [("scenes 3", lab, dep, 22), ("scene 1", lab[:1], dep[:1], 22)]
    for name, lab, dep, ncls in cases:
        want = dcl.ops.label_table_host(lab, dep, ncls)
        got = dcl.ops.label_table(*cuda_frames(lab, dep), ncls).cpu().numpy()
        assert np.array_equal(got, want), name
    assert np.array_equal(want, numpy_table(lab, dep, ncls))


# ------------------------------------------------------------------------------------------------------ posed crop points
COUNTS = (1, 4095, 4096, 4097)


def chunk_frames():
    """one frame per count: the first K pixels (flat order) of the box rows 3 .. 103, columns 5 .. 105 carry class 5"""
    rng = np.random.default_rng(21)
    n = len(COUNTS)
    img = rng.integers(0, 256, (n, 120, 130, 3), dtype=np.uint8)
    dep = rng.integers(9000, 11000, (n, 120, 130)).astype(np.uint16)
    lab = np.zeros((n, 120, 130), np.int32)
    for f, K in enumerate(COUNTS):
        sub = np.zeros(100 * 100, np.int32)
        sub[:K] = 5
        lab[f, 3:103, 5:105] = sub.reshape(100, 100)
    lab[:, 0, 0] = 5                                                 # a pixel of the class outside the box takes no part
    return img, dep, lab


def posed_reference(dcl, img, dep, lab, src, cams, rows, min_valid):
    out = []
    for (r0, r1, c0, c1, cls, f), cam, row in zip(src, cams, rows):
        sc = {"label": lab[f], "depth": dep[f], "img": img[f], "meta": {"camera": tuple(float(v) for v in cam[:4])}}
        if not ((lab[f] == cls) & (dep[f] != 0))[r0:r1, c0:c1].any():
            out.append((None, None, None, (0, 0, 0), None, None))
            continue
        cloud, centroid, col = TS.frame_cloud(sc, cls, (r0, r1, c0, c1))
        posed, R1, t1 = dcl.ops.crop_repose_host(cloud, row, centroid)
        inside = (np.abs(posed) < np.float32(HALF)).all(1)
        m = int(inside.sum())
        wrote = m if m > min_valid else 0
        out.append((posed[inside][:wrote], col[inside][:wrote], centroid, (cloud.shape[0], m, wrote), R1, t1))
    return out


@pytest.mark.parametrize("min_valid", [0, 50])
def test_posed_crop_points_equal_the_host_twin(dcl, min_valid):
    img, dep, lab = chunk_frames()
    rng = np.random.default_rng(22)
    eye = np.eye(3)
    src, cams, poses = [], [], []
    # the centroid of every crop is near (x, y, 1.0): a ground-truth translation there keeps the re-posed cloud in the grid
    near = np.array([-0.24, -0.17, 1.0])
    for f in range(len(COUNTS)):
        src.append((3, 103, 5, 105, 5, f))
        cams.append(TS.CAMERAS[1 + f % 2] + (TS.FACTOR_DEPTH,))
        poses.append((TS._rotation(rng), near + rng.uniform(-0.02, 0.02, 3), rng.uniform(-0.03, 0.03, 3), dcl.crops.euler2mat(*rng.uniform(-0.087, 0.087, 3))))
    src.append((3, 103, 5, 105, 5, 3))                               # the identity pose: R0 = A = I, t_gt = 0, no jitter
    cams.append(TS.CAMERAS[1] + (TS.FACTOR_DEPTH,))
    poses.append((eye, np.zeros(3), np.zeros(3), eye))
    src.append((3, 103, 5, 105, 5, 2))                               # zero jitter, second camera
    cams.append(TS.CAMERAS[2] + (TS.FACTOR_DEPTH,))
    poses.append((TS._rotation(rng), near, np.zeros(3), dcl.crops.euler2mat(0.05, -0.08, 0.03)))
    src.append((0, 60, 0, 70, 5, 1))                                 # another box of frame 1 (takes in the pixel at (0, 0))
    cams.append(TS.CAMERAS[1] + (TS.FACTOR_DEPTH,))
    poses.append((TS._rotation(rng), near, rng.uniform(-0.03, 0.03, 3), eye))
    src.append((50, 50, 5, 105, 5, 0))                               # an empty box
    cams.append(TS.CAMERAS[1] + (TS.FACTOR_DEPTH,))
    poses.append((eye, near, np.zeros(3), eye))
    src_a, cam_a = np.asarray(src, np.int32), np.asarray(cams, np.float32)
    rows = dcl.ops.pose_rows(*[[p[k] for p in poses] for k in range(4)])
    d_t, l_t, i_t = torch.from_numpy(dep.view(np.int16)).cuda(), torch.from_numpy(lab).cuda(), torch.from_numpy(img).cuda()
    xyz, col, centroid, counts, rot, trans = dcl.ops.crop_points_posed(
        d_t, l_t, i_t, src_a[:, 5], torch.from_numpy(src_a).cuda(), torch.from_numpy(cam_a).cuda(), torch.from_numpy(rows).cuda(),
        RGB_MEAN, [HALF] * 3, min_valid, cap=10000)
    torch.cuda.synchronize()
    xyz, col, centroid, counts, rot, trans = (t.cpu().numpy() for t in (xyz, col, centroid, counts, rot, trans))
    want = posed_reference(dcl, img, dep, lab, src, cam_a, rows, min_valid)
    seen = set()
    for i, (wx, wc, wcen, wcnt, wR, wt) in enumerate(want):
        assert tuple(counts[i]) == wcnt, (i, counts[i], wcnt)
        seen.add(wcnt[0])
        if wcnt[0] == 0:
            assert not rot[i].any() and not trans[i].any() and not centroid[i].any()
            continue
        assert np.array_equal(centroid[i], wcen), i
        assert np.array_equal(rot[i], wR) and np.array_equal(trans[i], wt), i
        assert np.array_equal(xyz[i, :wcnt[2]], wx) and np.array_equal(col[i, :wcnt[2]], wc), i
    assert set(COUNTS) <= seen and 0 in seen
    assert all(w[3][1] > 50 for w in want[1:6]), "the big crops must keep their points inside the grid"
    assert (counts[0, 2] == 1) == (min_valid == 0)                   # the 1-point crop is a dummy under the loader's threshold


# ------------------------------------------------------------------------------------------------------------ build_train
class Replay(object):
    """the recorded draws of the golden scenes `seeds`, handed out in the order build_train asks for them"""

    def __init__(self, golden, seeds):
        self.picks = [int(p) for s in seeds for p in golden["t%d_picks" % s]]
        self.ang = [golden["t%d_angles" % s].tolist() for s in seeds if len(golden["t%d_angles" % s])]
        self.jit = [golden["t%d_jitter" % s].tolist() for s in seeds if len(golden["t%d_jitter" % s])]
        self.cho = [(int(golden["t%d_m" % s]), golden["t%d_choice" % s]) for s in seeds if "t%d_choice" % s in golden.files]

    def pick(self, k):
        return self.picks.pop(0)

    def angles(self):
        return self.ang.pop(0)

    def jitter(self):
        return self.jit.pop(0)

    def choice(self, m, n):
        want_m, idx = self.cho.pop(0)
        assert m == want_m and len(idx) == n
        return idx

    def done(self):
        return not (self.picks or self.ang or self.jit or self.cho)


def scene(seed):
    kw = [k for s, k, _ in TS.CASES if s == seed][0]
    return TS.make_train_scene(seed, tmp_size=TS.CFG["tmp_size"], **kw), kw


def frame_of(sc):
    return (sc["img"], sc["depth"], sc["label"])


@pytest.mark.parametrize("seed", [s for s, _, _ in TS.CASES])
def test_build_train_single_scene_against_the_reference_loader(dcl, golden, seed):
    sc, kw = scene(seed)
    tag = "t%d_" % seed
    builder = dcl.crops.CropBuilder(TS.CFG, sc["cad_pts"], sc["cad_col"])
    draw = Replay(golden, [seed])
    data = builder.build_train([frame_of(sc)], [sc["meta"]], draw=draw)
    torch.cuda.synchronize()
    assert draw.done()
    assert int(data["obj"][0]) == int(golden[tag + "obj"]) and tuple(data["boxes"][0]) == tuple(golden[tag + "box"])
    dummy = float(golden[tag + "flag"]) == -1
    assert bool(data["kept"][0]) == (not dummy)
    if dummy:
        assert "inp" not in data and data["flags"].numel() == 0
        return
    obj, box, idx = int(golden[tag + "obj"]), golden[tag + "box"], int(golden[tag + "picks"][-1])
    assert int(data["counts"][0, 1]) == int(golden[tag + "m"])                       # the number of points inside the grid
    # labels, flags, radius: equal (rot_gt: the reference's `@` differs in the last bit -- fixture rot_exact = 0 -- so it is
    # held to the bound of two evaluations of a 3-term dot product, and to the host twin's bits)
    P = sc["meta"]["poses"][:, :, idx]
    A = dcl.crops.euler2mat(*golden[tag + "angles"])
    cloud, centroid, colours = TS.frame_cloud(sc, obj, box)
    row = dcl.ops.pose_rows([P[:, 0:3]], [P[:, 3]], [golden[tag + "jitter"]], [A])[0]
    posed, R1, t1 = dcl.ops.crop_repose_host(cloud, row, centroid)
    rot = data["labels"]["rot_gt"].cpu().numpy()[0]
    assert np.array_equal(rot, R1)
    if int(golden["rot_exact"]):
        assert np.array_equal(rot, golden[tag + "rot_gt"])
    else:
        SR = np.abs(P[:, 0:3].astype(np.float32).astype(np.float64)) @ np.abs(A.astype(np.float32).astype(np.float64))
        assert (np.abs(golden[tag + "rot_gt"].astype(np.float64) - rot) <= ROT_BOUND * SR).all()
    assert np.array_equal(data["labels"]["trans_gt"].cpu().numpy()[0], golden[tag + "trans_gt"])
    assert np.array_equal(data["labels"]["obj_idx"].cpu().numpy()[0], golden[tag + "obj_idx"])
    assert np.array_equal(data["flags"].cpu().numpy(), golden[tag + "sym"])
    assert np.array_equal(data["radius"].cpu().numpy()[0], golden[tag + "radius"])
    assert np.array_equal(data["centroids"].cpu().numpy()[0], centroid)
    # the observed side: colours and the constant column equal; coordinates = the host twin's bits, within the bound of the
    # reference's
    feats, ref = data["inp"]["feats"].cpu().numpy(), golden[tag + "feat_inp"]
    choice = golden[tag + "choice"]
    inside = (np.abs(posed) < np.float32(HALF)).all(1)
    assert np.array_equal(feats[:, :4], ref[:, :4])
    assert np.array_equal(feats[:, 4:7], posed[inside][choice])
    t0 = (P[:, 3] - centroid.astype(np.float64)).astype(np.float32)
    bound = TS.repose_bound(cloud, P[:, 0:3].astype(np.float32), A.astype(np.float32), t0, t1)[0][inside][choice]
    assert (np.abs(feats[:, 4:7].astype(np.float64) - ref[:, 4:7]) <= bound).all()
    # voxel rows: equal except at points within the bound of a voxel border
    near = TS.near_voxel_border(feats[:, 4:7], bound, HALF, UNIT)
    assert near.sum() <= 0.01 * TS.CFG["input_size"]
    vox = data["inp"]["coords"].cpu().numpy()
    assert (vox[:, 0] == 0).all() and np.array_equal(vox[~near, 1:], golden[tag + "vox_inp"][~near])
    if not near.any():
        for k in ("occupied_voxels", "p2v_maps", "v2p_maps"):
            assert np.array_equal(data["inp"][k].cpu().numpy(), golden[tag + "inp_" + k]), k
    # the template side is constant per class: equal
    for k in ("feats", "occupied_voxels", "p2v_maps", "v2p_maps"):
        assert np.array_equal(data["tmp"][k].cpu().numpy(), golden[tag + "tmp_" + k]), k
    assert data["batch_offsets"].tolist() == [0, TS.CFG["input_size"]]


@pytest.fixture(scope="module")
def batch(dcl):
    scs = [scene(s)[0] for s, _, _ in TS.CASES]
    return scs, [frame_of(s) for s in scs], [s["meta"] for s in scs]


def rows_of(data, k, n_inp, n_tmp):
    """the bits of sample k of a batch that do not depend on its position"""
    return [data["inp"]["feats"][k * n_inp:(k + 1) * n_inp], data["inp"]["coords"][k * n_inp:(k + 1) * n_inp, 1:],
            data["tmp"]["feats"][k * n_tmp:(k + 1) * n_tmp], data["tmp"]["coords"][k * n_tmp:(k + 1) * n_tmp, 1:],
            data["labels"]["rot_gt"][k], data["labels"]["trans_gt"][k], data["labels"]["obj_idx"][k], data["flags"][k],
            data["radius"][k], data["centroids"][k]]


def test_build_train_batch_equals_its_single_samples_and_repeats(dcl, golden, batch):
    """all scenes at once (frames of two sizes: the tall one makes the others padded), the recorded draws replayed"""
    scs, frames, metas = batch
    seeds = [s for s, _, _ in TS.CASES]
    builder = dcl.crops.CropBuilder(TS.CFG, scs[0]["cad_pts"], scs[0]["cad_col"])
    n_inp, n_tmp = TS.CFG["input_size"], TS.CFG["tmp_size"]
    draw = Replay(golden, seeds)
    data = builder.build_train(frames, metas, draw=draw)
    assert draw.done()
    want_kept = [float(golden["t%d_flag" % s]) != -1 for s in seeds]
    assert data["kept"].tolist() == want_kept and sum(want_kept) == 5
    kept_seeds = [s for s, k in zip(seeds, want_kept) if k]
    assert data["flags"].cpu().tolist() == [float(int(golden["t%d_obj" % s]) - 1 in (12, 15, 18, 19, 20)) for s in kept_seeds]
    assert data["obj"].tolist() == [int(golden["t%d_obj" % s]) for s in seeds]
    b = len(kept_seeds)
    assert data["batch_offsets"].tolist() == [i * n_inp for i in range(b + 1)]
    assert data["inp"]["coords"][:, 0].cpu().tolist() == [i for i in range(b) for _ in range(n_inp)]
    k = 0
    for s, sc, keep in zip(seeds, scs, want_kept):
        one = builder.build_train([frame_of(sc)], [sc["meta"]], draw=Replay(golden, [s]))
        assert bool(one["kept"][0]) == keep
        if keep:
            for a, w in zip(rows_of(data, k, n_inp, n_tmp), rows_of(one, 0, n_inp, n_tmp)):
                assert torch.equal(a, w), s
            k += 1
    again = builder.build_train(frames, metas, draw=Replay(golden, seeds))
    for side in ("inp", "tmp"):
        for key in ("feats", "coords", "occupied_voxels", "p2v_maps", "v2p_maps"):
            assert torch.equal(again[side][key], data[side][key]), (side, key)
    for key in ("rot_gt", "trans_gt", "obj_idx"):
        assert torch.equal(again["labels"][key], data["labels"][key]), key


def test_build_train_synchronises_the_host_twice(dcl, golden, batch, monkeypatch):
    """a capacity-form builder on resident frames: the label table and the point counts come back, nothing else.  Counted two
    ways: every Tensor.cpu() / .item() / .tolist() of a CUDA tensor inside the call, and -- where this torch build honours it --
    the warnings of torch.cuda.set_sync_debug_mode("warn")."""
    scs, frames, metas = batch
    seeds = [s for s, _, _ in TS.CASES]
    builder = dcl.crops.CropBuilder(TS.CFG, scs[0]["cad_pts"], scs[0]["cad_col"], capacity=True)
    res = [dcl.crops.CropBuilder.resident(*f) for f in frames]
    builder.build_train(res, metas, draw=Replay(golden, seeds))      # first use: library load, the template tables' cache
    torch.cuda.synchronize()
    calls = []
    for name in ("cpu", "item", "tolist", "numpy"):
        orig = getattr(torch.Tensor, name)

        def counted(self, *a, _orig=orig, _name=name, **k):
            if self.is_cuda:
                calls.append(_name)
            return _orig(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, name, counted)
    prev = torch.cuda.get_sync_debug_mode()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            data = builder.build_train(res, metas, draw=Replay(golden, seeds))
            inside = len([w for w in caught if "called a synchronizing" in str(w.message)])
            torch.ones(1, device="cuda").cpu()                       # does the mode see a synchronisation at all?
            honoured = len([w for w in caught if "called a synchronizing" in str(w.message)]) > inside
        finally:
            torch.cuda.set_sync_debug_mode(prev)
    print("build_train: host read-backs %s; sync debug mode %s: %d warnings" % (calls[:-1], "honoured" if honoured else "NOT honoured", inside))
    assert calls[:-1] == ["cpu", "cpu"]
    if honoured:
        assert inside == 2
    assert "v0_dev" in data["inp"] and data["kept"].sum() == 5


def test_network_trains_on_a_build_train_batch(dcl):
    """Network(cfg, mode='train') takes the dict: one forward + backward at 2 x 256 / 64 points, finite gradients"""
    import random
    n_inp, n_tmp = 256, 64
    scs = [scene(51)[0], scene(52)[0]]
    cfg = dict(TS.CFG, input_size=n_inp)
    builder = dcl.crops.CropBuilder(cfg, scs[0]["cad_pts"], scs[0]["cad_col"])
    np.random.seed(5)
    random.seed(5)
    data = builder.build_train([frame_of(s) for s in scs], [s["meta"] for s in scs])
    assert data["kept"].all() and tuple(data["inp"]["feats"].shape) == (2 * n_inp, 7)
    net = dcl.DCL_Net.Network(dcl.synth.default_cfg(n_inp, n_tmp), mode="train")
    net.load_state_dict(dcl.synth.synth_state_dict(net, 1))
    net = net.cuda().train()
    out = net(data)
    loss = (out["rot_pred"] - data["labels"]["rot_gt"]).abs().mean() + (out["trans_pred"] - data["labels"]["trans_gt"]).abs().mean()
    loss.backward()
    assert torch.isfinite(loss)
    dead = ("regressor_Xo", "regressor_Yc")                           # heads that do not feed rot / trans
    bad = [k for k, p in net.named_parameters() if not k.startswith(dead) and (p.grad is None or not torch.isfinite(p.grad).all())]
    assert bad == []
    assert float(net.backbone_inp.module1[0].layers[0].weight.grad.abs().sum()) > 0
