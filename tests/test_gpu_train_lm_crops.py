"""The LineMOD training loader's front end on the device (csrc/crops_train_lm.hip, crops.py::CropBuilder.build_train_lm).

Kernels against their host twins, bit for bit: the mask extent, the occlusion paste with its commit / roll-back (the random
cases of tests/test_train_lm_crops_abi.py as ONE call per frame size, hand-made plans with repeated axes, the fixture scenes)
and the float64 posed crop points on crops of 1, 4095, 4096 and 4097 masked pixels (the chunk size of the crop kernels is 4096).
`build_train_lm` against the reference loader's outputs (tests/golden/train_lm_crops_ref.npz): points, rot_gt and trans_gt equal
bit for bit except where the float64 value lies within 8 * 2^-53 * sum|terms| of a float32 rounding boundary, where one ulp is
allowed (the reference's float64 `@` goes through a BLAS of unspecified order); everything else equal."""
import os
import random
import warnings

import numpy as np
import pytest
import torch

import train_lm_scene as LS
import test_train_lm_crops_abi as A

pytestmark = pytest.mark.gpu

RGB_MEAN = (0.485, 0.456, 0.406)
UNIT = LS.CFG["unit_voxel_extent"][0]
CAM6 = LS.LM_CAMERA + (1.0, 1000.0)


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "train_lm_crops_ref.npz"))


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def host(t):
    a = t.cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.int16 else a


# ------------------------------------------------------------------------------------------------------------ mask extent
def test_mask_extent_equals_the_host_twin(dcl):
    for name, m in A.extent_cases():                                 # 23 x 37, 48 x 64, 480 x 640: tails, more than one workgroup
        want = dcl.ops.mask_extent_host(m)
        assert np.array_equal(dcl.ops.mask_extent(dev(m)).cpu().numpy(), want), name
        assert np.array_equal(dcl.ops.mask_extent(dev(m[:1])).cpu().numpy(), want[:1]), name


# ------------------------------------------------------------------------------------------------------------ occlusion paste
def device_paste(dcl, rgb, depth, mask, o_rgb, o_depth, o_mask, plans):
    m_t = dev(mask)
    out = dcl.ops.occlude_paste(dev(rgb), dev(depth), m_t, dev(o_rgb), dev(o_depth), dev(o_mask), plans, dev(plans),
                                dcl.ops.mask_extent(m_t))
    torch.cuda.synchronize()
    return tuple(host(t) for t in out)


@pytest.mark.parametrize("H,W,n,seed", A.PASTE_SIZES)
def test_occlude_paste_equals_the_host_twin_on_the_random_cases(dcl, H, W, n, seed):
    rgb, depth, mask, o_rgb, o_depth, o_mask, starts, boxes = A.paste_cases(H, W, n, seed)
    plans = A.plans_of(dcl, H, W, mask, o_mask, starts, boxes)
    want = dcl.ops.occlude_paste_host(rgb, depth, mask, o_rgb, o_depth, o_mask, plans)
    got = device_paste(dcl, rgb, depth, mask, o_rgb, o_depth, o_mask, plans)
    for g, w, what in zip(got, want, ("rgb", "depth", "label", "info")):
        assert np.array_equal(g, w), what
    assert 0 < int(want[3][:, 0].sum()) < n and int(((plans[:, 0] == 1) & (want[3][:, 0] == 0)).sum()) > 0    # commits and roll-backs


def test_occlude_paste_repeated_axes_and_a_disagreeing_device_row(dcl):
    arrays = A.hand_made_plans()
    got = device_paste(dcl, *arrays)
    A.check_hand_made(got, arrays)
    for g, w in zip(got, dcl.ops.occlude_paste_host(*arrays)):
        assert np.array_equal(g, w)
    # a DEVICE row that disagrees with the checked host copy is clamped into both frames: the call completes and the pixels
    # outside the (clamped) rectangle are the originals
    rgb, depth, mask, o_rgb, o_depth, o_mask, plans = arrays
    wild = plans.copy()
    wild[0, 1:12] = (99, 10 ** 6, -5, 7, 7, -3, 10 ** 6, 2 ** 30, 2 ** 30, 0, 0)
    wild[1, 12:16] = (-7, 10 ** 6, -7, 10 ** 6)
    m_t = dev(mask)
    out = dcl.ops.occlude_paste(dev(rgb), dev(depth), m_t, dev(o_rgb), dev(o_depth), dev(o_mask), plans, dev(wild), dcl.ops.mask_extent(m_t))
    torch.cuda.synchronize()
    w_rgb, w_dep, w_lab, info = (host(t) for t in out)
    assert np.array_equal(w_rgb[0], rgb[0]) and np.array_equal(w_dep[0], depth[0])   # tx0 clamped to W: an empty rectangle
    assert np.array_equal(w_lab[0], mask[0, :, :, 0]) and int(info[0, 3]) == 0
    assert int(info[1, 2]) == int(((w_lab[1] == 255) & (w_dep[1] != 0)).sum())       # the box clamped to the whole frame


def scene_arrays(dcl, golden, seeds):
    """the fixture scenes as one call: stacked frames, the occluder frames of the scenes that have one, the plans"""
    scs = [A.scene(s) for s in seeds]
    others = [sc["other"] for sc in scs if sc["other"] is not None and sc["other"][0].shape[2] == 3]
    plans = np.stack([A.scene_plan(dcl, sc, golden, s) for sc, s in zip(scs, seeds)])
    k = 0
    for i, sc in enumerate(scs):
        if sc["other"] is not None and sc["other"][0].shape[2] == 3:
            plans[i, 1] = k
            k += 1
    return (scs, np.stack([sc["img"] for sc in scs]), np.stack([sc["depth"] for sc in scs]), np.stack([sc["mask"] for sc in scs]),
            np.stack([o[0] for o in others]), np.stack([o[1] for o in others]), np.stack([o[2] for o in others]), plans)


def test_occlude_paste_on_the_fixture_scenes(dcl, golden):
    scs, rgb, depth, mask, o_rgb, o_depth, o_mask, plans = scene_arrays(dcl, golden, A.SEEDS)
    got = device_paste(dcl, rgb, depth, mask, o_rgb, o_depth, o_mask, plans)
    want = dcl.ops.occlude_paste_host(rgb, depth, mask, o_rgb, o_depth, o_mask, plans)
    for g, w, what in zip(got, want, ("rgb", "depth", "label", "info")):
        assert np.array_equal(g, w), what
    for i, s in enumerate(A.SEEDS):
        tag = "l%d_" % s
        assert bool(got[3][i, 0]) == bool(golden[tag + "occluded"]) and int(got[3][i, 2]) == int(golden[tag + "n_choose"]), s
        assert A.box_crc(got[0][i], got[1][i], got[2][i], golden[tag + "box"]) == int(golden[tag + "crc"]), s


# ------------------------------------------------------------------------------------------------------ posed crop points
COUNTS = (1, 4095, 4096, 4097)


def chunk_frames():
    """one frame per count: the first K pixels (flat order) of the box rows 3 .. 103, columns 5 .. 105 carry label 255"""
    rng = np.random.default_rng(23)
    n = len(COUNTS)
    img = rng.integers(0, 256, (n, 120, 130, 3), dtype=np.uint8)
    dep = rng.integers(900, 1100, (n, 120, 130)).astype(np.uint16)
    lab = np.zeros((n, 120, 130), np.int32)
    for f, K in enumerate(COUNTS):
        sub = np.zeros(100 * 100, np.int32)
        sub[:K] = 255
        lab[f, 3:103, 5:105] = sub.reshape(100, 100)
    lab[:, 0, 0] = 255                                               # a pixel of the object outside the box takes no part
    return img, dep, lab


def posed64_reference(dcl, img, dep, lab, src, rows, min_valid):
    out = []
    for (r0, r1, c0, c1, cls, f), row in zip(src, rows):
        if not ((lab[f] == cls) & (dep[f] != 0))[r0:r1, c0:c1].any():
            out.append((None, None, None, (0, 0, 0), None, None))
            continue
        cloud, centroid, col = LS.frame_cloud(img[f], dep[f], lab[f], (r0, r1, c0, c1))
        posed, R1, t1, inside = dcl.ops.crop_repose64_host(cloud, row, centroid, A.HALF3)
        m = int(inside.sum())
        wrote = m if m > min_valid else 0
        out.append((posed[inside][:wrote], col[inside][:wrote], centroid, (cloud.shape[0], m, wrote), R1, t1))
    return out


@pytest.mark.parametrize("min_valid", [0, 128])
def test_posed64_crop_points_equal_the_host_twin(dcl, min_valid):
    img, dep, lab = chunk_frames()
    rng = np.random.default_rng(24)
    eye = np.eye(3)
    src, poses = [], []
    # the centroid of every crop is near (x, y, 1.0): a ground-truth translation there keeps the re-posed cloud in the grid
    near = np.array([-0.47, -0.33, 1.0])
    for f in range(len(COUNTS)):
        src.append((3, 103, 5, 105, 255, f))
        poses.append((LS.rotation(rng), near + rng.uniform(-0.02, 0.02, 3), rng.uniform(-0.03, 0.03, 3), dcl.crops.euler2mat(*rng.uniform(-0.087, 0.087, 3))))
    src.append((3, 103, 5, 105, 255, 3))                             # the identity pose: R0 = A = I, t_gt = 0, no jitter
    poses.append((eye, np.zeros(3), np.zeros(3), eye))
    src.append((0, 60, 0, 70, 255, 1))                               # another box of frame 1 (takes in the pixel at (0, 0))
    poses.append((LS.rotation(rng), near, rng.uniform(-0.03, 0.03, 3), eye))
    src.append((50, 50, 5, 105, 255, 0))                             # an empty box
    poses.append((eye, near, np.zeros(3), eye))
    src_a = np.asarray(src, np.int32)
    cam_a = np.tile(np.asarray(CAM6, np.float32), (len(src), 1))
    rows = dcl.ops.pose_rows64(*[[p[k] for p in poses] for k in range(4)])
    out = dcl.ops.crop_points_posed64(dev(dep), dev(lab), dev(img), src_a[:, 5], dev(src_a), dev(cam_a), dev(rows), RGB_MEAN,
                                      A.HALF3, min_valid, cap=10000)
    torch.cuda.synchronize()
    xyz, col, centroid, counts, rot, trans = (t.cpu().numpy() for t in out)
    want = posed64_reference(dcl, img, dep, lab, src, rows, min_valid)
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
    assert all(w[3][1] > 128 for w in want[1:5]), "the big crops must keep their points inside the grid"
    assert (counts[0, 2] == 1) == (min_valid == 0)                   # the 1-point crop is a dummy under the loader's threshold


# ------------------------------------------------------------------------------------------------------------ build_train_lm
class Replay(object):
    """the recorded draws of the golden scenes `seeds`, handed out in the order build_train_lm asks for them"""

    def __init__(self, golden, seeds):
        self.pas = [golden["l%d_paste" % s].tolist() for s in seeds if len(golden["l%d_paste" % s])]
        self.ang = [golden["l%d_angles" % s].tolist() for s in seeds if len(golden["l%d_angles" % s])]
        self.jit = [golden["l%d_jitter" % s].tolist() for s in seeds if len(golden["l%d_jitter" % s])]
        self.cho = [(int(golden["l%d_m" % s]), golden["l%d_choice" % s]) for s in seeds if "l%d_choice" % s in golden.files]

    def paste(self, lo_y, hi_y, lo_x, hi_x):
        sy, sx = self.pas.pop(0)
        assert lo_y <= sy < hi_y and lo_x <= sx < hi_x
        return sy, sx

    def angles(self):
        return self.ang.pop(0)

    def jitter(self):
        return self.jit.pop(0)

    def choice(self, m, n):
        want_m, idx = self.cho.pop(0)
        assert m == want_m and len(idx) == n
        return idx

    def done(self):
        return not (self.pas or self.ang or self.jit or self.cho)


def lm_builder(dcl, sc, **kw):
    return dcl.crops.CropBuilder(LS.CFG, sc["cad_pts"], sc["cad_col"], camera=dcl.crops.LM_CAMERA, **kw)


def check_against_the_fixture(dcl, golden, seed, sc, data, k=0):
    """sample k of `data` against the reference loader's item of scene `seed`"""
    tag = "l%d_" % seed
    n_inp, n_tmp = LS.CFG["input_size"], LS.CFG["tmp_size"]
    _, cloud, centroid, colours, row, R0, Aug, t_gt, jit = A.scene_pose(dcl, golden, seed)
    v64, wR1, wt1, T = LS.numpy_repose64(cloud, R0, Aug, t_gt, jit, centroid)
    inside = (np.abs(v64) < LS.HALF).all(1)
    choice = golden[tag + "choice"]
    assert int(data["counts"][k, 1]) == int(golden[tag + "m"]) == int(inside.sum())
    feats, ref = data["inp"]["feats"].cpu().numpy()[k * n_inp:(k + 1) * n_inp], golden[tag + "feat_inp"]
    assert np.array_equal(feats[:, :4], ref[:, :4])                                  # the constant column and the colours
    near = LS.near_f32_boundary(v64[inside][choice], T[inside][choice])
    assert LS.equal_under_the_rule(feats[:, 4:7], ref[:, 4:7], near).all()
    assert np.array_equal(feats[:, 4:7], dcl.ops.crop_repose64_host(cloud, row, centroid)[0][inside][choice])
    rot, trans = data["labels"]["rot_gt"].cpu().numpy()[k], data["labels"]["trans_gt"].cpu().numpy()[k]
    assert LS.equal_under_the_rule(rot, golden[tag + "rot_gt"], LS.near_f32_boundary(wR1, np.abs(R0) @ np.abs(Aug))).all()
    assert LS.equal_under_the_rule(trans, golden[tag + "trans_gt"], LS.near_f32_boundary(wt1, np.abs(wt1))).all()
    assert float(data["flags"].cpu()[k]) == float(golden[tag + "sym"][0])
    assert int(data["obj_idx"].cpu()[k]) == int(golden[tag + "obj_idx"][0])
    assert np.array_equal(data["centriods"].cpu().numpy()[k], golden[tag + "centroid"])
    vox = data["inp"]["coords"].cpu().numpy()[k * n_inp:(k + 1) * n_inp]
    same = (feats[:, 4:7] == ref[:, 4:7]).all(1)
    assert (vox[:, 0] == k).all() and np.array_equal(vox[same, 1:], golden[tag + "vox_inp"][same])
    return bool(same.all())


@pytest.mark.parametrize("seed", A.SEEDS)
def test_build_train_lm_single_scene_against_the_reference_loader(dcl, golden, seed):
    sc = A.scene(seed)
    tag = "l%d_" % seed
    builder = lm_builder(dcl, sc)
    draw = Replay(golden, [seed])
    data = builder.build_train_lm([LS.sample_of(sc)], draw=draw)
    torch.cuda.synchronize()
    assert draw.done()
    assert tuple(data["boxes"][0]) == tuple(golden[tag + "box"]) and bool(data["occluded"][0]) == bool(golden[tag + "occluded"])
    dummy = float(golden[tag + "flag"]) == -1
    assert bool(data["kept"][0]) == (not dummy)
    if dummy:
        assert "inp" not in data and data["flags"].numel() == 0 and data["batch_offsets"].tolist() == [0]
        return
    exact = check_against_the_fixture(dcl, golden, seed, sc, data)
    assert data["batch_offsets"].tolist() == [0, LS.CFG["input_size"]]
    if seed in (71, 80, 81):
        n_tmp = LS.CFG["tmp_size"]
        assert np.array_equal(data["tmp"]["feats"].cpu().numpy(), golden[tag + "feat_tmp"])
        assert np.array_equal(data["tmp"]["coords"].cpu().numpy()[:, 1:], golden[tag + "vox_tmp"]) and data["tmp"]["feats"].shape[0] == n_tmp
        for side in ("inp", "tmp"):
            for key in ("occupied_voxels", "p2v_maps", "v2p_maps"):
                if side == "tmp" or exact:
                    assert np.array_equal(data[side][key].cpu().numpy(), golden[tag + side + "_" + key]), (side, key)


@pytest.fixture(scope="module")
def batch(dcl):
    scs = [A.scene(s) for s in A.SEEDS]
    return scs, [LS.sample_of(sc) for sc in scs]


def rows_of(data, k, n_inp, n_tmp):
    """the bits of sample k of a batch that do not depend on its position"""
    return [data["inp"]["feats"][k * n_inp:(k + 1) * n_inp], data["inp"]["coords"][k * n_inp:(k + 1) * n_inp, 1:],
            data["tmp"]["feats"][k * n_tmp:(k + 1) * n_tmp], data["tmp"]["coords"][k * n_tmp:(k + 1) * n_tmp, 1:],
            data["labels"]["rot_gt"][k], data["labels"]["trans_gt"][k], data["obj_idx"][k], data["flags"][k], data["centriods"][k]]


def test_build_train_lm_batch_equals_the_fixture_and_repeats(dcl, golden, batch):
    """all scenes as one batch, the recorded draws replayed; two calls give the same bits"""
    scs, samples = batch
    builder = lm_builder(dcl, scs[0])
    n_inp, n_tmp = LS.CFG["input_size"], LS.CFG["tmp_size"]
    draw = Replay(golden, A.SEEDS)
    data = builder.build_train_lm(samples, draw=draw)
    assert draw.done()
    want_kept = [float(golden["l%d_flag" % s]) != -1 for s in A.SEEDS]
    assert data["kept"].tolist() == want_kept and sum(want_kept) == 10
    assert data["occluded"].tolist() == [bool(golden["l%d_occluded" % s]) for s in A.SEEDS]
    kept_seeds = [s for s, k in zip(A.SEEDS, want_kept) if k]
    b = len(kept_seeds)
    assert data["batch_offsets"].tolist() == [i * n_inp for i in range(b + 1)]
    assert data["flags"].cpu().tolist() == [float(golden["l%d_sym" % s][0]) for s in kept_seeds]
    for k, s in enumerate(kept_seeds):
        check_against_the_fixture(dcl, golden, s, scs[A.SEEDS.index(s)], data, k)
    again = builder.build_train_lm(samples, draw=Replay(golden, A.SEEDS))
    for k in range(b):
        for a, w in zip(rows_of(again, k, n_inp, n_tmp), rows_of(data, k, n_inp, n_tmp)):
            assert torch.equal(a, w), k
    for side in ("inp", "tmp"):
        for key in ("occupied_voxels", "p2v_maps", "v2p_maps"):
            assert torch.equal(again[side][key], data[side][key]), (side, key)


@pytest.mark.parametrize("seed", [71, 80])
def test_seeded_default_draws_give_the_loaders_item_and_generator_states(dcl, golden, seed):
    """one frame, the loader's own calls on np.random and random: the item of the fixture, and both generators end where the
    loader left them (the caller draws the other index first, as `occlude_with_another_object` does)"""
    sc = A.scene(seed)
    tag = "l%d_" % seed
    builder = lm_builder(dcl, sc)
    np.random.seed(seed)
    random.seed(seed)
    assert dcl.crops.lm_other_index(LS.DICT_INDEX(sc["obj"]), sc["obj"]) == 1
    data = builder.build_train_lm([LS.sample_of(sc)])
    nxt = (np.random.random_sample(), random.random())
    check_against_the_fixture(dcl, golden, seed, sc, data)
    np.random.seed(seed)
    random.seed(seed)
    random.choice([1])
    if len(golden[tag + "paste"]):
        own, _ = LS.numpy_extent(sc["mask"])
        oth, _ = LS.numpy_extent(sc["other"][2])
        np.random.randint(own[0] - (oth[1] - oth[0] + 1) + 1, own[1] + 1)
        np.random.randint(own[2] - (oth[3] - oth[2] + 1) + 1, own[3] + 1)
    for _ in range(3):
        np.random.uniform(-1, 1)
        random.uniform(-1, 1)
    m = int(golden[tag + "m"])
    np.random.choice(m, LS.CFG["input_size"], replace=m <= LS.CFG["input_size"])
    assert nxt == (np.random.random_sample(), random.random())


def test_build_train_lm_synchronises_the_host_three_times(dcl, golden, batch, monkeypatch):
    """a capacity-form builder on resident frames: the mask extents, the valid-pixel counts after the paste and the point counts
    come back, nothing else.  Counted two ways: every Tensor.cpu() / .item() / .tolist() / .numpy() of a CUDA tensor inside the
    call, and -- where this torch build honours it -- the warnings of torch.cuda.set_sync_debug_mode("warn")."""
    scs, samples = batch
    builder = lm_builder(dcl, scs[0], capacity=True)
    res = []
    for s in samples:
        r = dict(s)
        r["img"], r["depth"], r["mask"] = dcl.crops.CropBuilder.resident_lm(s["img"], s["depth"], s["mask"])
        if s["other"] is not None:
            r["other"] = dcl.crops.CropBuilder.resident_lm(*s["other"])
        res.append(r)
    builder.build_train_lm(res, draw=Replay(golden, A.SEEDS))         # first use: library load, the template tables' cache
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
            data = builder.build_train_lm(res, draw=Replay(golden, A.SEEDS))
            inside = len([w for w in caught if "called a synchronizing" in str(w.message)])
            torch.ones(1, device="cuda").cpu()                       # does the mode see a synchronisation at all?
            honoured = len([w for w in caught if "called a synchronizing" in str(w.message)]) > inside
        finally:
            torch.cuda.set_sync_debug_mode(prev)
    print("build_train_lm: host read-backs %s; sync debug mode %s: %d warnings" % (calls[:-1], "honoured" if honoured else "NOT honoured", inside))
    assert calls[:-1] == ["cpu", "cpu", "cpu"]
    if honoured:
        assert inside == 3
    assert "v0_dev" in data["inp"] and data["kept"].sum() == 10
