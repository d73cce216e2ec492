"""Generates tests/golden/lmo_crops_ref.npz by running the REFERENCE's own Occlusion-LineMOD loader `__getitem__` (unmodified
code of LM/dataloader_test_LMO.py, its `mask_to_bbox` selection loop and `get_bbox` included) on the occluded frames of
tests/lmo_scene.py, the way make_crops_golden.py runs the LineMOD loader.

Runs only where the reference checkout that make_crops_golden.py names is present (nothing from it is copied).  One difference to
make_crops_golden.py: `cv2` is a stub WRITTEN HERE, because the loader's box comes from it and cv2 is not installed:
  findContours  one (N,1,2) array of (x, y) coordinates per 8-connected component (scipy.ndimage.label, 3 x 3 structure),
                in the order of the tie rule of csrc/mask_box.h: the component whose first pixel in raster order comes
                LAST is handed out first (OpenCV hands contours out in reverse order of discovery).  NOT pinned against cv2;
                it cannot matter here: every non-empty mask is asserted to have a unique largest rectangle
  boundingRect  (min x, min y, extent x, extent y)
The fixture stores only the loader's OUTPUTS (and the box / crop rows its own mask_to_bbox / get_bbox returned); the scenes
regenerate from their seeds.

    python tests/golden/make_lmo_crops_golden.py
"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from lmo_scene import CASES, CFG, make_lmo_scene  # noqa: E402
from make_crops_golden import install_stubs  # noqa: E402

MODES = {41: "eval", 42: "test", 43: "eval", 44: "test", 45: "eval"}


def install_cv2_stub():
    from scipy import ndimage
    cv2 = sys.modules["cv2"]
    cv2.RETR_TREE, cv2.CHAIN_APPROX_SIMPLE = 3, 2

    def findContours(mask, mode, method):
        lab, n = ndimage.label(mask != 0, structure=np.ones((3, 3), int))
        comps = []
        for k in range(1, n + 1):
            ys, xs = np.nonzero(lab == k)                                  # raster order: [0] is the first pixel
            comps.append((int(ys[0]) * mask.shape[1] + int(xs[0]), np.stack([xs, ys], 1)[:, None, :].astype(np.int32)))
        comps.sort(key=lambda c: -c[0])
        return None, [c[1] for c in comps], None

    def boundingRect(contour):
        x0, y0 = contour[:, 0, 0].min(), contour[:, 0, 1].min()
        return int(x0), int(y0), int(contour[:, 0, 0].max() - x0 + 1), int(contour[:, 0, 1].max() - y0 + 1)
    cv2.findContours, cv2.boundingRect = findContours, boundingRect


def lmo_item(mod, sc, cfg, seed, mode):
    ds = object.__new__(mod.Dataset)
    ds.npoint_inp, ds.npoint_tmp = cfg["input_size"], cfg["tmp_size"]
    ds.unit_voxel_extent = np.array(cfg["unit_voxel_extent"]).astype(float)
    ds.voxel_num_limit = np.array(cfg["voxel_num_limit"]).astype(float)
    ds.total_voxel_extent = ds.voxel_num_limit * ds.unit_voxel_extent
    ds.voxelization_mode, ds.mode = cfg["voxelization_mode"], mode
    cls = sc["cls"]
    ds.objlist, ds.symmetry_obj_idx = [cls], []
    ds.list_rgb, ds.list_depth, ds.list_label, ds.list_obj = ["rgb"], ["depth"], ["label"], [cls]
    ds.list_rot, ds.list_trans = [np.eye(3, dtype=np.float32)], [np.array([0.01, 0.02, 0.8], np.float32)]
    ds.list_pc_CAD, ds.list_rgb_CAD = sc["cad_pts"], sc["cad_col"]
    H, W = sc["depth"].shape
    ds.xmap = np.array([[j for _ in range(W)] for j in range(H)])
    ds.ymap = np.array([[i for i in range(W)] for _ in range(H)])
    ds.cam_cx, ds.cam_cy, ds.cam_fx, ds.cam_fy = 325.26110, 242.04899, 572.41140, 573.57043
    one = sc["mask_label"].astype(np.uint8)                                  # the dataset's mask png: 1 on the object
    label = one if mode == "eval" else one[:, :, None].repeat(3, axis=2)
    files = {"rgb": sc["img"], "depth": sc["depth"], "label": label}
    mod.Image.open = lambda path: files[path]
    np.random.seed(seed)
    return ds[0]


def main():
    from scipy import ndimage
    install_stubs()
    install_cv2_stub()
    mod = importlib.import_module("LM.dataloader_test_LMO")
    out = {}
    for seed, kw in CASES:
        sc = make_lmo_scene(seed, tmp_size=CFG["tmp_size"], **kw)
        m = sc["mask_label"]
        if m.any():
            lab, n = ndimage.label(m, structure=np.ones((3, 3), int))
            areas = sorted((s[0].stop - s[0].start) * (s[1].stop - s[1].start) for s in ndimage.find_objects(lab))
            assert n >= 3 and areas[-1] > areas[-2], (seed, n, areas[-3:])
        item = lmo_item(mod, sc, CFG, seed, MODES[seed])
        tag = "lmo%d_" % seed
        box = mod.mask_to_bbox(m, padding=0)
        out[tag + "box"] = np.array(box, np.int32)
        out[tag + "crop"] = np.array(mod.get_bbox(box), np.int32)
        out[tag + "flag"] = item[4].numpy()
        if float(item[4][0]) != -1:
            out[tag + "feat_inp"], out[tag + "vox_inp"] = item[0].numpy(), item[1].numpy()
            out[tag + "feat_tmp"], out[tag + "vox_tmp"] = item[2].numpy(), item[3].numpy()
            out[tag + "centroid"] = item[9].numpy()
        print(tag, MODES[seed], "box", box, "flag", item[4].tolist())
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "lmo_crops_ref.npz"), **out)
    print("golden written: lmo_crops_ref.npz", len(out), "arrays")


if __name__ == "__main__":
    main()
