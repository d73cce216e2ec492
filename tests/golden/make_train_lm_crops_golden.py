"""Generates tests/golden/train_lm_crops_ref.npz by running the REFERENCE's own LineMOD training loader -- the unmodified
`__getitem__` (mode 'train'), `occlude_with_another_object`, `get_other_idx`, `get_bbox` and `collate` of
LM/dataloader_train_LM.py -- on the synthetic frames of tests/train_lm_scene.py, the way make_train_crops_golden.py runs the
YCB-V training loader.

Runs only where the reference checkout that make_crops_golden.py names is present (nothing from it is copied).  Its file I/O is
replaced as there (`Image.open` returns the scene's arrays, the dataset object is made without `__init__`; the frame list holds
this frame and the other one, so `get_other_idx` has one index to choose -- a scene without another frame makes `Image.open`
fail for it, which the loader answers with the originals).  One more stub is WRITTEN HERE: `transforms3d.euler.euler2mat`,
because transforms3d is not installed --
    euler2mat(a1, a2, a3) = Rz(a3) Ry(a2) Rx(a1)      (the package's default axes 'sxyz'; NOT pinned against the package)
the form make_train_crops_golden.py states.  The random calls of the loader are wrapped to RECORD what each sample consumed;
`occlude_with_another_object` is wrapped on the instance to record what it returned.  They run unchanged.

The fixture stores only the loader's OUTPUTS, the draws, and what this generator measured:
  <tag>paste (the two starts, or empty), occluded, crc (zlib.crc32 of the composite colour / depth / mask channel 0 inside the
  crop box), mask_sum, n_choose, box, flag, angles, jitter, m_inside, [feat_inp, vox_inp, rot_gt, trans_gt, sym, obj_idx,
  centroid, m, choice; of the scenes COLLATED also feat_tmp, vox_tmp and inp_* / tmp_* {occupied_voxels, p2v_maps, v2p_maps} of
  collate([item])] -- integers in the narrowest type that holds them
  near_boundary              per scene: how many stored float32 elements (points, rot_gt, trans_gt) lie within
                             8 * 2^-53 * sum|terms| of a float32 rounding boundary -- there the reference's BLAS order and the
                             stated left-to-right order may round differently and one ulp is allowed; at most 0.1 % of a scene
  mismatches                 how many stored elements differ from the left-to-right float64 restatement at all
Every scene is asserted to be what tests/train_lm_scene.py::CASES claims.

    python tests/golden/make_train_lm_crops_golden.py
"""
import importlib
import os
import random
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import train_lm_scene as LS  # noqa: E402
import train_scene as TS  # noqa: E402
from make_crops_golden import install_stubs  # noqa: E402
from make_train_crops_golden import Recorder, euler2mat_stub  # noqa: E402


COLLATED = (71, 80, 81)


def box_crc(img, depth, label0, box):
    r0, r1, c0, c1 = [int(v) for v in box]
    crc = zlib.crc32(np.ascontiguousarray(img[r0:r1, c0:c1, :3]).tobytes())
    crc = zlib.crc32(np.ascontiguousarray(depth[r0:r1, c0:c1]).astype(np.uint16).tobytes(), crc)
    return zlib.crc32(np.ascontiguousarray(label0[r0:r1, c0:c1]).astype(np.int32).tobytes(), crc)


def make_dataset(mod, sc, cfg):
    ds = object.__new__(mod.Dataset)
    ds.npoint_inp, ds.npoint_tmp = cfg["input_size"], cfg["tmp_size"]
    ds.unit_voxel_extent = np.array(cfg["unit_voxel_extent"]).astype(float)
    ds.voxel_num_limit = np.array(cfg["voxel_num_limit"]).astype(float)
    ds.total_voxel_extent = ds.voxel_num_limit * ds.unit_voxel_extent
    ds.voxelization_mode, ds.mode, ds.root = cfg["voxelization_mode"], "train", "/scene"
    ds.objlist = list(LS.OBJLIST)
    ds.symmetry_obj_idx = [7, 8]
    obj = sc["obj"]
    ds.list_rgb, ds.list_depth, ds.list_label = ["rgb0", "rgb1"], ["depth0", "depth1"], ["mask0", "mask1"]
    ds.list_obj, ds.list_rank = [obj, 15], [0, 0]
    ds.dict_index_objs = LS.DICT_INDEX(obj)
    ds.meta = {obj: {0: [{"obj_bb": sc["obj_bb"], "cam_R_m2c": sc["cam_R_m2c"], "cam_t_m2c": sc["cam_t_m2c"], "obj_id": obj}]}}
    ds.list_pc_CAD, ds.list_rgb_CAD = sc["cad_pts"], sc["cad_col"]
    ds.xmap = np.array([[j for _ in range(640)] for j in range(480)])
    ds.ymap = np.array([[i for i in range(640)] for _ in range(480)])
    ds.cam_cx, ds.cam_cy, ds.cam_fx, ds.cam_fy = LS.LM_CAMERA
    files = {"rgb0": sc["img"], "depth0": sc["depth"], "mask0": sc["mask"]}
    if sc["other"] is not None:
        files.update({"rgb1": sc["other"][0], "depth1": sc["other"][1], "mask1": sc["other"][2]})
    mod.Image.open = lambda path: files[path]
    seen = {}
    inner = ds.occlude_with_another_object

    def recording(image, depth, mask, obj_id):
        res = inner(image, depth, mask, obj_id)
        seen["committed"] = res[0] is image
        seen["img"], seen["depth"], seen["mask"] = (np.array(a) for a in res)
        return res
    ds.occlude_with_another_object = recording
    return ds, seen


def main():
    install_stubs()
    sys.modules["transforms3d.euler"].euler2mat = euler2mat_stub
    mod = importlib.import_module("LM.dataloader_train_LM")
    cfg = LS.CFG
    half, unit = LS.HALF, cfg["unit_voxel_extent"][0]
    out, near_all, mism_all = {}, [], []
    for seed, kw, claim in LS.CASES:
        sc = LS.make_lm_scene(seed, tmp_size=cfg["tmp_size"], **kw)
        ds, seen = make_dataset(mod, sc, cfg)
        np.random.seed(seed)
        random.seed(seed)
        with Recorder() as rec:
            item = ds[0]
        tag = "l%d_" % seed
        flag = float(item[4][0])
        box = np.array(mod.get_bbox(sc["obj_bb"]), np.int32)
        label0 = seen["mask"][:, :, 0]
        n_choose = int(((label0 == 255) & (seen["depth"] != 0))[box[0]:box[1], box[2]:box[3]].sum())
        out[tag + "paste"], out[tag + "occluded"] = np.array(rec.picks, np.int64), np.int32(seen["committed"])
        out[tag + "crc"] = np.uint32(box_crc(seen["img"], seen["depth"], label0, box))
        out[tag + "mask_sum"], out[tag + "n_choose"] = np.int64(seen["mask"].sum(dtype=np.int64)), np.int64(n_choose)
        out[tag + "box"], out[tag + "flag"] = box, np.float32(flag)
        out[tag + "angles"], out[tag + "jitter"] = np.array(rec.angles, np.float64), np.array(rec.jitter, np.float64)
        # ---- the scene is what CASES claims
        changed = not (np.array_equal(seen["img"], sc["img"][:, :, :3]) and np.array_equal(seen["depth"], sc["depth"]) and
                       np.array_equal(seen["mask"], sc["mask"]))
        removed = int(sc["mask"].sum(dtype=np.int64)) - int(seen["mask"].sum(dtype=np.int64))
        assert changed == seen["committed"], seed
        own_ext, _ = LS.numpy_extent(sc["mask"])
        if sc["other"] is not None and not kw.get("empty_other"):
            oth_ext, _ = LS.numpy_extent(sc["other"][2])
            oh, ow = oth_ext[1] - oth_ext[0] + 1, oth_ext[3] - oth_ext[2] + 1
            assert len(rec.picks) == 2, (seed, rec.picks)
            sy, sx = rec.picks
            ey, ex = sy + oh, sx + ow
            rest = LS.numpy_occlude(sc["img"], sc["depth"], sc["mask"], sc["other"][0], sc["other"][1], sc["other"][2], sy, sx)
            assert rest[3] == seen["committed"] and np.array_equal(rest[0], seen["img"]) and np.array_equal(rest[2], seen["mask"]), seed
        else:
            assert len(rec.picks) == 0 and not seen["committed"], seed
            sy = sx = ey = ex = None
        inside_y, inside_x = sy is not None and sy >= 0 and ey <= 480, sx is not None and sx >= 0 and ex <= 480
        if seed == 71:
            assert seen["committed"] and inside_y and inside_x and 0 < removed < int(sc["mask"].sum(dtype=np.int64))
        if seed == 72:
            assert seen["committed"] and sy < 0 and inside_x and removed > 0
        if seed == 73:
            assert seen["committed"] and ey > 480 and inside_x and removed > 0
        if seed == 74:
            assert not seen["committed"] and sx < 0 and inside_y
        if seed == 175:
            assert not seen["committed"] and ex > 480 and sx >= 0 and inside_y
        if seed == 76:
            assert not seen["committed"] and not rest[4] and inside_y and inside_x       # pasted, the sum fell below 20, undone
        if seed == 77:
            assert kw["empty_other"] and len(rec.picks) == 0
        if seed == 278:
            assert seen["committed"] and n_choose == 0 and flag == -1 and len(rec.angles) == 0 and len(rec.jitter) == 0
        else:
            assert n_choose > 0 and len(rec.angles) == 3 and len(rec.jitter) == 3, seed
        if seed == 82:
            assert not seen["committed"] and len(rec.picks) == 2 and rest[4] and inside_y and inside_x and sc["other"][0].shape[2] == 4
        if seed in (81, 82):
            assert sc["obj"] in (10, 11)
        if n_choose == 0:
            print(tag, claim, "| paste", rec.picks)
            continue
        # ---- the left-to-right float64 restatement on the composite the loader made
        A = euler2mat_stub(*rec.angles)
        cloud, centroid, colours = LS.frame_cloud(seen["img"], seen["depth"], label0, box)
        R0, t_gt = np.resize(np.array(sc["cam_R_m2c"]), (3, 3)), np.array(sc["cam_t_m2c"]) / 1000.0
        posed, R1, t1, T = LS.numpy_repose64(cloud, R0, A, t_gt, rec.jitter, centroid)
        # no re-posed point within the bound of a grid face: the in-grid set is the same on every evaluation
        assert (np.abs(np.abs(posed) - half) > 8.0 * LS.U64 * T).all(), (seed, "a point lies on a grid face")
        inside = (np.abs(posed) < half).all(1)
        m = int(inside.sum())
        out[tag + "m_inside"] = np.int64(m)
        if seed == 79:
            assert flag == -1 and m <= 128, (seed, m)
            print(tag, claim, "| inside the grid", m)
            continue
        assert flag != -1 and m > 128 and m == rec.m, (seed, m, rec.m)
        assert (m <= cfg["input_size"]) == (seed == 80), (seed, m)
        ref_xyz = item[0].numpy()[:, 4:7]
        got64, T_sel = posed[inside][rec.choice], T[inside][rec.choice]
        SR = np.abs(R0) @ np.abs(A)
        near = [LS.near_f32_boundary(got64, T_sel), LS.near_f32_boundary(R1, SR), LS.near_f32_boundary(t1, np.abs(t1))]
        pairs = [(got64.astype(np.float32), ref_xyz), (R1.astype(np.float32), item[5].numpy()), (t1.astype(np.float32), item[6].numpy())]
        for (g, r), nb in zip(pairs, near):
            assert LS.equal_under_the_rule(g, r, nb).all(), (seed, "the reference differs from the restatement beyond the rule")
        n_near = int(sum(nb.sum() for nb in near))
        n_el = int(sum(nb.size for nb in near))
        n_mis = int(sum((g != r).sum() for g, r in pairs))
        assert n_near <= 0.001 * n_el, (seed, n_near, n_el)
        near_all.append(n_near)
        mism_all.append(n_mis)
        assert np.array_equal(item[0].numpy()[:, 1:4], colours[inside][rec.choice]), seed
        assert np.array_equal(item[9].numpy(), centroid), seed
        # voxel rows: equal where the point is; a point one ulp off may sit in the next voxel only within that ulp of a border
        same = (got64.astype(np.float32) == ref_xyz).all(1)
        vox = ((got64.astype(np.float32) + np.float32(half)) / np.float32(unit)).astype(np.int64)
        border = TS.near_voxel_border(ref_xyz, np.spacing(np.abs(ref_xyz)).astype(np.float64), half, unit)
        assert np.array_equal(vox[same | ~border], item[1].numpy()[same | ~border]), seed
        out[tag + "feat_inp"], out[tag + "vox_inp"] = item[0].numpy(), item[1].numpy().astype(np.int16)
        out[tag + "sym"], out[tag + "rot_gt"], out[tag + "trans_gt"] = item[4].numpy(), item[5].numpy(), item[6].numpy()
        out[tag + "obj_idx"], out[tag + "centroid"] = item[7].numpy(), item[9].numpy()
        out[tag + "m"], out[tag + "choice"] = np.int64(m), rec.choice.astype(np.int32)
        d = ds.collate([item])
        assert np.array_equal(d["inp"]["feats"].numpy(), item[0].numpy()) and np.array_equal(d["tmp"]["feats"].numpy(), item[2].numpy())
        if seed in COLLATED:                          # the template side and collate's maps: of three scenes (the file's size)
            out[tag + "feat_tmp"], out[tag + "vox_tmp"] = item[2].numpy(), item[3].numpy().astype(np.int16)
            for side in ("inp", "tmp"):
                for k in ("occupied_voxels", "p2v_maps", "v2p_maps"):
                    out[tag + side + "_" + k] = d[side][k].numpy().astype(np.int32)
        assert float(d["flags"][0]) == float(sc["obj"] in (10, 11)) and int(d["obj_idx"][0]) == LS.OBJLIST.index(sc["obj"])
        print(tag, claim, "| paste", rec.picks, "occluded", seen["committed"], "m", m, "near a rounding boundary", n_near,
              "differ from the restatement", n_mis)
    out["near_boundary"], out["mismatches"] = np.array(near_all, np.int64), np.array(mism_all, np.int64)
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "train_lm_crops_ref.npz"), **out)
    print("golden written: train_lm_crops_ref.npz", len(out), "arrays; near a rounding boundary %d, mismatches %d"
          % (sum(near_all), sum(mism_all)))


if __name__ == "__main__":
    main()
