"""Several frames per builder call on the GPU: the two kernel forms against their per-frame selves, the
concatenation rule of CropBuilder.build_frames in its device and host forms, no host synchronisation, padding rows
(valid == -1) and the tables that skip them, the LineMOD forms, the chain from builder to table, and the prefetcher."""
import numpy as np
import pytest
import torch

import metric_table_cases as MC
from lmo_scene import CASES as LMO_CASES, make_lmo_scene
from test_gpu_crops_device_draws import CFG, SyncCount, _scene, _sync_debug_is_honoured

pytestmark = pytest.mark.gpu

R_TOL, T_TOL = 1e-4, 1e-5
N = CFG["input_size"]
_SIDE = ("feats", "coords", "occupied_voxels", "p2v_maps", "v2p_maps")
HALF = [0.006 * 64 * 0.5] * 3


def _same(a, b):
    return MC.bits(a) == MC.bits(b)


def _frames(tiny=False):
    """three frames: four objects of which one has an empty mask and one no detection; one object (beside a tiny one when
    `tiny`); six objects.  Three, one (two) and six crops."""
    return [_scene(41), _scene(52, n_obj=2 if tiny else 1, empty=None, undetected=None, tiny=1 if tiny else None),
            _scene(53, n_obj=6, empty=None, undetected=None)]


def _tuple(dcl, sc, resident=True, poses=True):
    fr = dcl.crops.CropBuilder.resident(sc["img"], sc["depth"], sc["label"]) if resident else (sc["img"], sc["depth"], sc["label"])
    return fr + (sc["rois"], sc["gt_obj"]) + ((sc["poses"],) if poses else ())


def _builder(dcl, scenes, **kw):
    return dcl.crops.CropBuilder(CFG, scenes[0]["cad_pts"], scenes[0]["cad_col"], **kw)          # one set of CAD clouds for all frames


def _serial(builder, tuples):
    return [builder.build(*t[:5], poses=t[5] if len(t) > 5 else None) for t in tuples]


def _rebased(per, key, n_per):
    """the per-frame coordinate rows with the crop column counting through the batch"""
    out, at = [], 0
    for d in per:
        c = d[key]["coords"].clone()
        c[:, 0] += at
        out.append(c)
        at += c.shape[0] // n_per
    return torch.cat(out)


def _assert_concatenation(dcl, data, per, device_form, template_ids):
    b = sum(d["inp"]["feats"].shape[0] // N for d in per)
    assert data["n_live"] == b and data["batch_offsets"].shape[0] == b + 1
    assert torch.equal(data["inp"]["feats"], torch.cat([d["inp"]["feats"] for d in per]))
    assert torch.equal(data["inp"]["coords"], _rebased(per, "inp", N))
    for k in ("rot_gt", "trans_gt"):
        assert torch.equal(data["labels"][k], torch.cat([d["labels"][k] for d in per])), k
    assert torch.equal(data["all_centroids"], torch.cat([d["all_centroids"] for d in per]))
    assert torch.equal(data["obj_idx"], torch.cat([d["obj_idx"] for d in per]))
    assert torch.equal(data["all_flags"], torch.cat([d["all_flags"] for d in per]))
    assert data["all_flags"].dtype == per[0]["all_flags"].dtype and data["obj_idx"].dtype == per[0]["obj_idx"].dtype
    if template_ids:
        assert torch.equal(data["tmp_cls"], torch.cat([d["tmp_cls"] for d in per])) and "tmp" not in data
    else:
        assert torch.equal(data["tmp"]["feats"], torch.cat([d["tmp"]["feats"] for d in per]))
        assert torch.equal(data["tmp"]["coords"], _rebased(per, "tmp", CFG["tmp_size"]))
        occ, p2v, v2p = dcl.ops.voxelize_idx_gpu(data["tmp"]["coords"], b, 64, 4)
        for k, w in (("occupied_voxels", occ), ("p2v_maps", p2v), ("v2p_maps", v2p)):
            assert torch.equal(data["tmp"][k], w), ("tmp", k)
    if device_form:
        for k in ("counts", "picks", "valid"):
            assert data[k].is_cuda and torch.equal(data[k], torch.cat([d[k] for d in per])), k
    else:
        assert np.array_equal(data["counts"], np.concatenate([d["counts"] for d in per]))
    offs, objs = [0], [0]
    for d in per:
        offs.append(offs[-1] + d["inp"]["feats"].shape[0] // N)
        objs.append(objs[-1] + d["obj_idx"].shape[0])
    assert data["frame_offsets"].tolist() == offs and data["frame_objects"].tolist() == objs
    assert not data["frame_offsets"].is_cuda and data["frame_offsets"].dtype == torch.int32
    # the observed side: ONE voxelisation over all crops
    exact = dcl.crops.exact_form(data)["inp"]
    occ, p2v, v2p = dcl.ops.voxelize_idx_gpu(data["inp"]["coords"], b, 64, 4)
    for k, w in (("occupied_voxels", occ), ("p2v_maps", p2v), ("v2p_maps", v2p)):
        assert torch.equal(exact[k], w), ("inp", k)


# ------------------------------------------------------------------------------------------- 1. the kernels
def _stacked(crops, scenes, small):
    """the frames stacked by hand, frame `small` cut to 400 x 600 and padded with depth 0 / label -1; per frame the boxes of
    its detected instances clipped to ITS size"""
    F = len(scenes)
    img, dep, lab = np.zeros((F, 480, 640, 3), np.uint8), np.zeros((F, 480, 640), np.uint16), np.full((F, 480, 640), -1, np.int32)
    own, src = [], []
    for f, sc in enumerate(scenes):
        h, w = (400, 600) if f == small else (480, 640)
        i, d, l = sc["img"][:h, :w], sc["depth"][:h, :w], sc["label"][:h, :w]
        img[f, :h, :w], dep[f, :h, :w], lab[f, :h, :w] = i, d, l
        rows = []
        for cls in sc["gt_obj"]:
            hit = np.where(sc["rois"][:, 1] == cls)[0]
            if hit.size:
                r0, r1, c0, c1 = crops.snap_box(sc["rois"], hit[0], h, w)
                rows.append((max(r0, 0), min(r1, h), max(c0, 0), min(c1, w), int(cls), f))
        src.extend(rows)
        own.append((np.ascontiguousarray(i), np.ascontiguousarray(d), np.ascontiguousarray(l), np.asarray(rows, np.int32)))
    to = lambda a: torch.from_numpy(a).cuda()                                                     # noqa: E731
    return (to(img), to(dep.view(np.int16)), to(lab)), np.asarray(src, np.int32), own


@pytest.mark.parametrize("lm", [False, True], ids=["ycbv", "lm_always_filter"])
def test_crop_points_frames_equals_crop_points_frame_by_frame(dcl, lm):
    scenes = _frames(tiny=True)
    (i_t, d_t, l_t), src, own = _stacked(dcl.crops, scenes, small=1)
    cam = dcl.crops.LM_CAMERA if lm else dcl.crops.YCBV_CAMERA
    kw = dict(min_valid=128 if lm else 32, always_filter=lm)
    area = lambda r: max(1, int(((r[:, 1] - r[:, 0]).clip(0) * (r[:, 3] - r[:, 2]).clip(0)).max()))  # noqa: E731
    src_t = torch.from_numpy(src).cuda()
    xyz, col, cen, cnt = dcl.ops.crop_points_frames(d_t, l_t, i_t, src[:, 5], src_t, cam, dcl.crops.RGB_MEAN, HALF, cap=area(src), **kw)
    torch.cuda.synchronize()
    counts = cnt.cpu().numpy()
    assert (counts[:, 0] == 0).sum() == 1 and ((counts[:, 0] > 0) & (counts[:, 0] <= 32)).sum() == 1      # the empty mask, the tiny one
    at = 0
    for f, (i, d, l, rows) in enumerate(own):
        ri, rd, rl = dcl.crops.CropBuilder.resident(i, d, l)
        rt = torch.from_numpy(rows).cuda()
        x1, c1, m1, n1 = dcl.ops.crop_points(rd, rl, ri, rt[:, :4].contiguous(), rt[:, 4].contiguous(), cam, dcl.crops.RGB_MEAN, HALF,
                                             cap=area(rows), **kw)
        k = len(rows)
        assert _same(cnt[at:at + k], n1) and _same(cen[at:at + k], m1), f
        for j in range(k):
            m = int(counts[at + j, 2])
            assert _same(xyz[at + j, :m], x1[j, :m]) and _same(col[at + j, :m], c1[j, :m]), (f, j)
        at += k
    assert at == len(src) == 3 + 2 + 6
    if lm:
        return
    # a HOST frame index outside the stack: refused before any device work
    bad = src[:, 5].copy()
    bad[4] = 3
    with pytest.raises(RuntimeError, match="invalid argument"):
        dcl.ops.crop_points_frames(d_t, l_t, i_t, bad, src_t, cam, dcl.crops.RGB_MEAN, HALF, cap=area(src), **kw)
    # a DEVICE row that names frame n_frames (its host copy does not): an empty crop, every other row as before
    off = src.copy()
    off[4, 5] = 3
    off[7, 5] = -1
    _, _, cen2, cnt2 = dcl.ops.crop_points_frames(d_t, l_t, i_t, src[:, 5], torch.from_numpy(off).cuda(), cam, dcl.crops.RGB_MEAN, HALF,
                                                  cap=area(src), **kw)
    c2 = cnt2.cpu().numpy()
    assert not c2[[4, 7]].any() and counts[[4, 7], 0].min() > 0
    keep = [k for k in range(len(src)) if k not in (4, 7)]
    assert np.array_equal(c2[keep], counts[keep]) and _same(cen2[keep], cen[keep])
    # the keyed draw on these counts: its host twin, and crop_draw frame by frame
    keys = np.stack([5 + src[:, 5].astype(np.int64), np.concatenate([np.arange(3), np.arange(2), np.arange(6)])], 1)
    picks, valid = dcl.ops.crop_draw_keyed(cnt, N, 9, torch.from_numpy(keys).cuda())
    want, want_valid = dcl.ops.crop_draw_keyed_host(counts, N, 9, keys)
    assert np.array_equal(picks.cpu().numpy(), want) and np.array_equal(valid.cpu().numpy(), want_valid)
    assert sorted(set(valid.tolist())) == [0, 1]
    at = 0
    for f, k in enumerate((3, 2, 6)):
        p1, v1 = dcl.ops.crop_draw(cnt[at:at + k].contiguous(), N, 9, 5 + f)
        assert torch.equal(picks[at:at + k], p1) and torch.equal(valid[at:at + k], v1), f
        at += k
    # rows=: padding rows behind the drawn ones
    p2, v2 = dcl.ops.crop_draw_keyed(cnt, N, 9, torch.from_numpy(keys).cuda(), rows=16)
    assert torch.equal(p2[:11], picks) and torch.equal(v2[:11], valid) and v2[11:].tolist() == [-1] * 5 and not p2[11:].any()


# ------------------------------------------------------------------------------------------- 2. the concatenation rule
@pytest.mark.parametrize("form", ["capacity_ids", "exact"])
def test_device_form_batch_is_the_concatenation_of_serial_builds(dcl, form):
    kw = dict(capacity=True, template_ids=True) if form == "capacity_ids" else dict(capacity=False)
    scenes = _frames(tiny=form == "exact")                      # (a tiny instance raises the capacity form's pitch flag by design)
    builder = _builder(dcl, scenes, draws="device", draw_seed=6, **kw)
    tuples = [_tuple(dcl, sc, resident=form != "exact") for sc in scenes]       # resident tensors / numpy arrays
    builder.draw_frame = 7
    per = _serial(builder, tuples)
    assert builder.draw_frame == 10
    builder.draw_frame = 7
    state = np.random.get_state()[1].copy()
    data = builder.build_frames(tuples)
    assert builder.draw_frame == 10                              # advanced by the number of frames
    assert np.array_equal(np.random.get_state()[1], state)
    _assert_concatenation(dcl, data, per, True, form == "capacity_ids")
    assert data["valid"].tolist() == [1, 1, 0] + [1] * (data["n_live"] - 3)
    if form == "capacity_ids":
        assert int(data["inp"]["vi_info"][2]) == 0 and "v0_dev" in data["inp"]
    # without poses: no labels, the same crops
    builder.draw_frame = 7
    bare = builder.build_frames([t[:5] for t in tuples])
    assert bare["labels"] == {} and torch.equal(bare["inp"]["feats"], data["inp"]["feats"])


def test_build_frames_refusals(dcl):
    scenes = _frames()
    builder = _builder(dcl, scenes, draws="device", capacity=True, template_ids=True)
    tuples = [_tuple(dcl, sc, resident=False) for sc in scenes]
    with pytest.raises(ValueError, match="at least one frame"):
        builder.build_frames([])
    lost = list(tuples[1])
    lost[3] = lost[3][-1:]                                       # only the detection of a class that is not in the frame
    with pytest.raises(ValueError, match="frame 1"):
        builder.build_frames([tuples[0], tuple(lost), tuples[2]])
    assert builder.draw_frame == 0                               # refused before any device work or draw
    rgba = _scene(52, n_obj=1, empty=None, undetected=None, rgba=True)
    with pytest.raises(ValueError, match="channels"):
        builder.build_frames([tuples[0], _tuple(dcl, rgba, resident=False)])
    with pytest.raises(ValueError, match="poses"):
        builder.build_frames([tuples[0], tuples[1][:5]])
    with pytest.raises(ValueError, match="VI_CROPS_MAX_BATCH"):
        builder.build_frames([tuples[2]] * 11)                   # 66 crops > 64: never a silent fall-back
    with pytest.raises(ValueError, match="VI_CROPS_MAX_BATCH"):
        builder.build_frames([tuples[2]] * 10, pad_to=33)        # 60 crops padded to 66
    assert builder.draw_frame == 0
    with pytest.raises(ValueError, match="pad_to"):
        builder.build_frames(tuples, pad_to=0)


# ------------------------------------------------------------------------------------------- 3. no host synchronisation
def test_a_padded_batch_is_built_without_a_host_synchronisation(dcl, monkeypatch):
    scenes = _frames()
    tuples = [_tuple(dcl, sc) for sc in scenes]
    dev_b = _builder(dcl, scenes, draws="device", capacity=True, template_ids=True, draw_seed=5)
    host_b = _builder(dcl, scenes, capacity=True, template_ids=True)
    dev_b.build_frames(tuples, pad_to=8)                         # (first call: the voxelisation's persistent words are made)
    host_b.build_frames(tuples)
    torch.cuda.synchronize()
    honoured = _sync_debug_is_honoured()
    count = SyncCount(monkeypatch)
    if honoured:
        torch.cuda.set_sync_debug_mode("error")
    try:
        data = dev_b.build_frames(tuples, pad_to=8)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert count.calls == [], count.calls
    host_b.build_frames(tuples)
    assert count.calls == ["cpu"], count.calls                   # the host form: all counts in ONE read-back, and nothing else
    monkeypatch.undo()
    print("torch.cuda.set_sync_debug_mode('error') honoured: %s" % honoured)
    assert data["valid"].shape[0] == 16 and data["n_live"] == 10 and dev_b.draw_frame == 6


# ------------------------------------------------------------------------------------------- 4. the host form
def test_host_form_batch_equals_serial_builds_under_the_same_seed(dcl):
    scenes = _frames(tiny=True)
    tuples = [_tuple(dcl, sc, resident=False) for sc in scenes]
    for kw in (dict(capacity=False), dict(capacity=False, template_ids=True)):
        builder = _builder(dcl, scenes, **kw)
        np.random.seed(77)
        per = _serial(builder, tuples)
        after = np.random.get_state()
        np.random.seed(77)
        data = builder.build_frames(tuples)
        now = np.random.get_state()
        assert now[0] == after[0] and np.array_equal(now[1], after[1]) and now[2:] == after[2:]
        _assert_concatenation(dcl, data, per, False, "template_ids" in kw)
        assert data["all_flags"].tolist() == [1, 1, 0, 0] + [1, 1] + [1] * 6 and data["n_live"] == 10
        assert "valid" not in data and "picks" not in data
    empty = _scene(60, n_obj=2, empty=None, undetected=None)
    empty["depth"] = np.zeros_like(empty["depth"])               # every mask of this frame is empty
    with pytest.raises(ValueError, match="frame 1 is empty"):
        builder.build_frames([tuples[0], _tuple(dcl, empty, resident=False), tuples[2]])


# ------------------------------------------------------------------------------------------- 5. padding
def test_padding_rows_are_lattice_crops_marked_minus_one(dcl):
    scenes = _frames()
    tuples = [_tuple(dcl, sc) for sc in scenes]
    for kw in (dict(capacity=True, template_ids=True), dict(capacity=True)):
        builder = _builder(dcl, scenes, draws="device", draw_seed=3, **kw)
        plain = builder.build_frames(tuples)
        builder.draw_frame = 0
        data = builder.build_frames(tuples, pad_to=8)
        b, live = 16, 10
        assert data["valid"].shape[0] == b and b % 8 == 0 and data["n_live"] == live and data["batch_offsets"].shape[0] == b + 1
        assert data["valid"][live:].tolist() == [-1] * (b - live) and torch.equal(data["valid"][:live], plain["valid"])
        assert data["frame_offsets"].tolist() == [0, 3, 4, 10]
        # the padding rows: the lattice dummy crop of the row's own crop index (the host twin's rows), zeros elsewhere
        zeros = np.zeros((b, 1, 3), np.float32)
        feats, coords = dcl.ops.crop_sample_valid_host(zeros, zeros, np.zeros((b, N), np.int64), None, np.full(b, -1, np.int32),
                                                       HALF[0], CFG["unit_voxel_extent"], 64)
        assert _same(data["inp"]["feats"][live * N:], feats[live * N:]) and _same(data["inp"]["coords"][live * N:], coords[live * N:])
        assert data["inp"]["coords"][live * N:, 0].reshape(b - live, N)[:, 0].tolist() == list(range(live, b))
        assert not data["counts"][live:].any() and not data["picks"][live:].any() and not data["all_centroids"][live:].any()
        eye = torch.eye(3, device="cuda").expand(b - live, 3, 3)
        assert torch.equal(data["labels"]["rot_gt"][live:], eye) and not data["labels"]["trans_gt"][live:].any()
        assert all(torch.isfinite(v).all() for v in data["labels"].values())
        assert int(data["inp"]["vi_info"][2]) == 0
        # the live rows: the bytes of the unpadded call
        for k in ("feats", "coords"):
            assert torch.equal(data["inp"][k][:live * N], plain["inp"][k]), k
        for k in ("counts", "picks", "all_centroids"):
            assert torch.equal(data[k][:live], plain[k]), k
        for k in ("rot_gt", "trans_gt"):
            assert torch.equal(data["labels"][k][:live], plain["labels"][k]), k
        assert torch.equal(data["all_flags"], plain["all_flags"]) and torch.equal(data["obj_idx"], plain["obj_idx"])
        if "tmp_cls" in data:
            first = int(plain["tmp_cls"][0])
            assert data["tmp_cls"].tolist() == plain["tmp_cls"].tolist() + [first] * (b - live)
        else:                                                    # a real template side for the padding rows: the first crop's class
            M = CFG["tmp_size"]
            assert torch.equal(data["tmp"]["feats"][:live * M], plain["tmp"]["feats"])
            assert torch.equal(data["tmp"]["feats"][live * M:], plain["tmp"]["feats"][:M].repeat(b - live, 1))
        occ, p2v, v2p = dcl.ops.voxelize_idx_gpu(data["inp"]["coords"], b, 64, 4)
        exact = dcl.crops.exact_form(data)["inp"]
        assert torch.equal(exact["occupied_voxels"], occ) and torch.equal(exact["p2v_maps"], p2v) and torch.equal(exact["v2p_maps"], v2p)
        # a crop count that is a multiple already: nothing is added
        builder.draw_frame = 0
        same = builder.build_frames(tuples, pad_to=5)
        assert same["valid"].shape[0] == live and torch.equal(same["inp"]["feats"], plain["inp"]["feats"])
    with pytest.raises(ValueError, match="pad_to"):
        _builder(dcl, scenes, capacity=True).build_frames(tuples, pad_to=8)


# ------------------------------------------------------------------------------------------- 6. the tables skip padding
def _table(dcl, mode, C, T):
    S = dcl.sharding
    if mode == "adds":
        return S.DeviceAddsTable(C, T, "cuda")
    return (S.DeviceLmTable if mode == "lm" else S.DeviceLmoTable)(np.linspace(0.01, 0.2, C), T, "cuda")


def _arrays_equal(a, b):
    return all(a.arrays[k] is None or _same(a.arrays[k], b.arrays[k]) for k in ("sums", "maxd", "counts", "bad"))


@pytest.mark.parametrize("mode", MC.MODES)
def test_tables_update_nothing_for_padding_rows(dcl, mode):
    T, b, P, C = 3, 7, 257, 21
    p = {k: v.cuda() for k, v in MC.pose_case(31, T, b, P, 5).items()}
    valid = torch.tensor([1, 0, 1, 1, 0, 1, 1], dtype=torch.int32).cuda()
    sym = p["sym"] if mode != "adds" else None
    # rows of valid < 0 between and behind the live ones: NaN poses and ground truth, class / cloud ids out of range
    B = b + 6
    live = [k for k in range(B) if k not in (0, 4, 5, 10, 11, 12)]

    def padded(x, fill, dim=0):
        shape = list(x.shape)
        shape[dim] = B
        out = torch.full(shape, fill, dtype=x.dtype, device=x.device)
        out.index_copy_(dim, torch.tensor(live, device=x.device), x)
        return out
    cls_p = padded(p["cls"], 0)
    cls_p[[0, 4, 5, 10, 11, 12]] = torch.tensor([99, -1, 1 << 30, 2, C, -(1 << 31)], dtype=torch.int32).cuda()
    valid_p = padded(valid, -1)
    valid_p[5], valid_p[12] = -7, -(1 << 31)
    Rp, tp = padded(p["Rp"], float("nan"), 1), padded(p["tp"], float("nan"), 1)
    Rg, tg = padded(p["Rg"], float("nan")), padded(p["tg"], float("nan"))
    sym_p = None if sym is None else padded(sym, 1)
    kw = dict(sym_flag=sym) if sym is not None else dict(mode="adds")
    kw_p = dict(sym_flag=sym_p) if sym is not None else dict(mode="adds")
    # add_traj: +inf on those rows, their poses never read, the live rows' bits
    dis = dcl.ops.add_traj(p["cld"], p["Rp"], p["tp"], p["Rg"], p["tg"], cls=p["cls"], valid=valid, **kw)
    dis_p = dcl.ops.add_traj(p["cld"], Rp, tp, Rg, tg, cls=cls_p, valid=valid_p, **kw_p)
    assert torch.isposinf(dis_p[:, [0, 4, 5, 10, 11, 12]]).all() and _same(dis_p[:, live], dis)
    # add_distances with the rows inserted (NaN distances on them)
    want, got = _table(dcl, mode, C, T), _table(dcl, mode, C, T)
    nan_p = padded(dis, float("nan"), 1)
    for _ in range(2):
        want.add_distances(p["cls"], dis, valid)
        got.add_distances(cls_p, nan_p, valid_p)
    assert _arrays_equal(got, want) and int(got.bad.cpu()[0]) == 0
    # add_frame on the padded batch against the live slice's
    want, got = _table(dcl, mode, C, T), _table(dcl, mode, C, T)
    for _ in range(2):
        want.add_frame(p["cld"], p["cls"], p["Rp"], p["tp"], p["Rg"], p["tg"], valid=valid, sym_flag=sym)
        got.add_frame(p["cld"], cls_p, Rp, tp, Rg, tg, valid=valid_p, sym_flag=sym_p)
    assert _arrays_equal(got, want) and int(got.bad.cpu()[0]) == 0
    got.finalize()
    # per-crop clouds, and a batch of nothing but padding
    own = padded(p["cld"][p["cls"].long()].contiguous(), float("nan"))
    got2 = _table(dcl, mode, C, T)
    for _ in range(2):
        got2.add_frame(own, cls_p, Rp, tp, Rg, tg, valid=valid_p, sym_flag=sym_p, per_crop=True)
    got2.add_frame(own, cls_p, Rp, tp, Rg, tg, valid=torch.full_like(valid_p, -1), sym_flag=sym_p, per_crop=True)
    assert _arrays_equal(got2, want)
    # the same rows as crops (valid = 1) DO count and raise bad: the rule is the sign of valid
    got2.add_distances(cls_p, nan_p, torch.ones_like(valid_p))
    assert int(got2.bad.cpu()[0]) == 1 and not _arrays_equal(got2, want)


# ------------------------------------------------------------------------------------------- 7. the LineMOD forms
LM_CFG = dict(CFG, unit_voxel_extent=[0.005] * 3)


def _lm_samples():
    out = []
    for seed, kw in LMO_CASES:
        sc = make_lmo_scene(seed, tmp_size=LM_CFG["tmp_size"], **kw)
        ys, xs = np.nonzero(sc["mask_label"])
        bb = [int(xs.min()) - 3, int(ys.min()) - 2, int(xs.max() - xs.min()) + 7, int(ys.max() - ys.min()) + 5] if ys.size else [200, 150, 90, 70]
        out.append((sc, bb))
    return out


def _lm_call(builder, which, sc, bb):
    if which == "lmo":
        return builder.build_lmo(sc["img"], sc["depth"], sc["mask_label"], sc["cls"])
    return builder.build_lm(sc["img"], sc["depth"], sc["mask_label"], bb if which == "lm" else None, sc["cls"], which != "lm")


def _lm_frames_call(builder, which, samples, **kw):
    rows = [(sc["img"], sc["depth"], sc["mask_label"], bb if which == "lm" else None, sc["cls"]) for sc, bb in samples]
    if which == "lmo":
        return builder.build_lmo_frames(rows, **kw)
    return builder.build_lm_frames(rows, eval_mode=which != "lm", **kw)


def _assert_lm_rows(data, row, want):
    """row `row` of the batch against build_lm's (feat_inp, voxel_inp, feat_tmp, voxel_tmp, centroid)"""
    M = LM_CFG["tmp_size"]
    assert torch.equal(data["inp"]["feats"][row * N:(row + 1) * N], want[0])
    assert torch.equal(data["inp"]["coords"][row * N:(row + 1) * N, 1:], want[1])
    assert (data["inp"]["coords"][row * N:(row + 1) * N, 0] == row).all()
    assert torch.equal(data["tmp"]["feats"][row * M:(row + 1) * M], want[2])
    assert torch.equal(data["tmp"]["coords"][row * M:(row + 1) * M, 1:], want[3])
    assert torch.equal(data["all_centroids"][row], want[4])


@pytest.mark.parametrize("which", ["lm", "lm_eval_mask_box", "lmo"])
def test_lm_frames_equal_the_per_sample_builders(dcl, which):
    samples = _lm_samples()
    sc0 = samples[0][0]
    mk = lambda **kw: dcl.crops.CropBuilder(LM_CFG, sc0["cad_pts"], sc0["cad_col"], camera=dcl.crops.LM_CAMERA, **kw)  # noqa: E731
    n = len(samples)
    # ---- device form: every sample stays
    dev_b = mk(draws="device", draw_seed=4)
    dev_b.draw_frame = 3
    per = [_lm_call(dev_b, which, sc, bb) for sc, bb in samples]
    assert dev_b.draw_frame == 3 + n
    dev_b.draw_frame = 3
    data = _lm_frames_call(dev_b, which, samples)
    assert dev_b.draw_frame == 3 + n and data["n_live"] == n and data["frame_offsets"].tolist() == list(range(n + 1))
    assert data["valid"].tolist() == [int(p[5][0]) for p in per] and data["valid"].tolist()[3:] == [0, 0] and 1 in data["valid"].tolist()
    for i, p in enumerate(per):
        _assert_lm_rows(data, i, p)
    assert data["obj"].tolist() == [sc["cls"] for sc, _ in samples] and data["all_flags"].tolist() == [1] * n
    occ, p2v, v2p = dcl.ops.voxelize_idx_gpu(data["inp"]["coords"], n, 64, 4)
    assert torch.equal(data["inp"]["occupied_voxels"], occ) and torch.equal(data["inp"]["p2v_maps"], p2v)
    # the scratch budget forced down to two instances per group: the same bytes
    dev_b.draw_frame = 3
    dev_b.FRAMES_SCRATCH_BYTES = 2 * 48 * 480 * 640
    split = _lm_frames_call(dev_b, which, samples, pad_to=4)
    assert split["valid"].tolist() == data["valid"].tolist() + [-1] * 3
    for k in ("feats", "coords"):
        assert torch.equal(split["inp"][k][:n * N], data["inp"][k]), k
    assert (split["inp"]["coords"][n * N:, 0].reshape(3, N)[:, 0].tolist()) == [5, 6, 7]
    for k in ("counts", "picks", "all_centroids"):
        assert torch.equal(split[k][:n], data[k]) and not split[k][n:].any(), k
    # ---- host form: the loader's dummy samples are dropped
    host_b = mk()
    np.random.seed(12)
    per = [_lm_call(host_b, which, sc, bb) for sc, bb in samples]
    after = np.random.get_state()
    kept = [i for i, p in enumerate(per) if p is not None]
    assert kept and len(kept) < n
    for budget in (512 << 20, 2 * 48 * 480 * 640):
        host_b.FRAMES_SCRATCH_BYTES = budget
        np.random.seed(12)
        data = _lm_frames_call(host_b, which, samples)
        now = np.random.get_state()
        assert np.array_equal(now[1], after[1]) and now[2:] == after[2:]
        assert data["n_live"] == len(kept) and data["all_flags"].tolist() == [int(i in kept) for i in range(n)]
        for row, i in enumerate(kept):
            _assert_lm_rows(data, row, per[i])
        assert "valid" not in data
    with pytest.raises(ValueError, match="pad_to"):
        _lm_frames_call(host_b, which, samples, pad_to=4)
    if which == "lm":
        rows = [(sc["img"], sc["depth"], sc["mask_label"], bb if k else None, sc["cls"]) for k, (sc, bb) in enumerate(samples)]
        with pytest.raises(ValueError, match="obj_bb"):
            host_b.build_lm_frames(rows)


# ------------------------------------------------------------------------------------------- 8. end to end
@pytest.mark.parametrize("routing", ["launch_by_launch", "default"])
def test_padded_batch_through_network_refiner_and_table(dcl, routing):
    """(N = M = 1024: the device-composed refine loop takes one confidence per point out of conf[:, :1024].)  The poses are not
    bit-equal between batch sizes: the GEMM core picks its kernels by row count."""
    from test_gpu_refine_loop import _refiner
    n, iteration = 1024, 2
    cfg = dict(CFG, input_size=n, tmp_size=n)
    frames = [dcl.synth.make_frame(700 + i, n_obj=k, tmp_size=n, empty=e) for i, (k, e) in enumerate(((2, None), (1, None), (3, 1)))]
    builder = dcl.crops.CropBuilder(cfg, frames[0]["cad_pts"], frames[0]["cad_col"], draws="device", capacity=True, template_ids=True,
                                    draw_seed=2)
    net = dcl.DCL_Net.Network(dcl.synth.default_cfg(n, n), mode="test", **(dict(graph_max_batch=0) if routing == "launch_by_launch" else {}))
    net.load_state_dict(dcl.synth.synth_state_dict(net, 1))
    net, ref = net.cuda().eval(), _refiner(dcl)
    cache = net.cache_templates(builder.templates(), cfg["voxel_num_limit"])
    tuples = [_tuple(dcl, f) for f in frames]
    T = iteration + 1

    def run(data, table):
        _, _, pred, (rots, transs) = dcl.refiner.stage2_chain(net, ref, data, iteration, graph=False, compose="device", trajectory=True)
        b = rots.shape[1]
        table.add_frame(data["labels"]["points_tmp"].reshape(b, n, 3), data["tmp_cls"], rots, transs, data["labels"]["rot_gt"],
                        data["labels"]["trans_gt"], valid=data["valid"], per_crop=True)
        return rots, transs, pred
    serial, batched = dcl.sharding.DeviceAddsTable(22, T, "cuda"), dcl.sharding.DeviceAddsTable(22, T, "cuda")
    per = [run(d, serial) for d in _serial(builder, tuples)]
    builder.draw_frame = 0
    data = builder.build_frames(tuples, pad_to=8)
    rots, transs, pred = run(data, batched)
    live = data["n_live"]
    assert live == 6 and rots.shape[1] == 8 and data["valid"].tolist() == [1, 1, 1, 1, 0, 1, -1, -1]
    assert net.replays_graph(8) == (routing == "default")
    assert int(pred["template_miss"].cpu()[0]) == 0 and int(cache.miss.cpu()[0]) == 0
    assert all(torch.isfinite(x).all() for x in (rots, transs, pred["conf"]))
    want_R, want_t = torch.cat([p[0] for p in per], 1), torch.cat([p[1] for p in per], 1)
    ok = data["valid"][:live] > 0                                # (a crop that is not valid has unspecified labels and centroid)
    for t in range(T):
        dR = float((rots[t, :live][ok] - want_R[t][ok]).abs().max())
        dt = float((transs[t, :live][ok] - want_t[t][ok]).abs().max())
        print("%s, pose %d of the trajectory: |dR| %.3g (tol %.0e)  |dt| %.3g (tol %.0e)" % (routing, t, dR, R_TOL, dt, T_TOL))
        assert dR <= R_TOL and dt <= T_TOL, t
    assert torch.equal(batched.sums[:, :, 0], serial.sums[:, :, 0])            # the table's n column: the padding rows are no crops
    assert float(batched.sums[:, :, 0].sum().cpu()) == T * live
    batched.finalize()
    serial.finalize()


# ------------------------------------------------------------------------------------------- 9. the prefetcher
def test_prefetcher_groups_frames_and_pads(dcl):
    scenes = [_scene(50 + i, n_obj=3, empty=None if i else 1, undetected=None) for i in range(3)]
    builder = _builder(dcl, scenes, draws="device", capacity=True, template_ids=True, draw_seed=2)
    order = [0, 1, 2, 1, 0]
    args = lambda i: _tuple(dcl, scenes[i], resident=False)  # noqa: E731
    want = [builder.build_frames([args(i) for i in order[k:k + 2]], pad_to=8) for k in (0, 2, 4)]
    torch.cuda.synchronize()
    assert [w["n_live"] for w in want] == [6, 6, 3] and builder.draw_frame == 5
    builder.draw_frame = 0
    feeds = (args(i)[:5] + ({"poses": args(i)[5]},) if i % 2 else args(i) for i in order)      # poses by keyword or by position
    n = 0
    with dcl.crops.CropPrefetcher(builder, feeds, depth=2, frames_per_call=2, pad_to=8) as feed:
        for got, ref in zip(feed, want):
            for k in _SIDE:
                assert torch.equal(got["inp"][k], ref["inp"][k]), (n, k)
            for k in ("valid", "picks", "counts", "tmp_cls"):
                assert torch.equal(got[k], ref[k]), (n, k)
            for k in ("rot_gt", "trans_gt"):
                assert torch.equal(got["labels"][k], ref["labels"][k]), (n, k)
            assert got["frame_offsets"].tolist() == ref["frame_offsets"].tolist() and got["valid"].shape[0] == 8
            n += 1
    assert n == 3 and builder.draw_frame == 5
    # frames_per_call=1 without padding keeps calling build()
    builder.draw_frame = 0
    with dcl.crops.CropPrefetcher(builder, (args(i) for i in order[:2]), depth=2) as feed:
        singles = list(feed)
    assert len(singles) == 2 and "frame_offsets" not in singles[0] and singles[0]["valid"].shape[0] == 3


def test_one_crop_frame_with_template_ids_replays_its_graph(dcl):
    """the serial baseline of the measurements: build(template_ids=True) of a ONE-candidate frame hands out its class id as a
    one-element view with a foreign stride, which the graph path's staging copy has to take"""
    sc = _scene(52, n_obj=1, empty=None, undetected=None)
    builder = _builder(dcl, [sc], draws="device", capacity=True, template_ids=True)
    net = dcl.DCL_Net.Network(dcl.synth.default_cfg(N, CFG["tmp_size"]), mode="test")
    net.load_state_dict(dcl.synth.synth_state_dict(net, 1))
    net = net.cuda().eval()
    net.cache_templates(builder.templates(), CFG["voxel_num_limit"])
    t = _tuple(dcl, sc)
    one = builder.build(*t[:5], poses=t[5])
    builder.draw_frame = 0
    batch = builder.build_frames([t])
    assert one["tmp_cls"].shape == (1,) and torch.equal(one["tmp_cls"], batch["tmp_cls"])
    with torch.no_grad():
        a = net(one)
        b = net(batch)
    assert net.replays_graph(1) and int(a["template_miss"].cpu()[0]) == 0
    for k in ("rot_pred", "trans_pred", "conf"):
        assert torch.equal(a[k], b[k]), k                        # the same crop, the same graph: the same bits
