"""Synthetic stand-in for one Occlusion-LineMOD test frame: the one-object frame of tests/crop_scene.py with its elliptical
mask OCCLUDED -- bars cut out of it leave three pieces of different sizes, and a few speckle pixels are set away from it --
so that the loader's `mask_to_bbox` has to choose among connected pieces.  Shared by the crop tests and
tests/golden/make_lmo_crops_golden.py (the fixture holds the reference loader's outputs only; the scenes regenerate from
their seeds)."""
import numpy as np

from crop_scene import make_scene

CFG = dict(input_size=128, tmp_size=64, unit_voxel_extent=[0.005] * 3, voxel_num_limit=[64] * 3, voxelization_mode=4)
# seed, keyword arguments: a plain occluded mask (twice), the largest piece on the image border, every mask pixel at depth
# 0 (the loader's first dummy return), an empty mask (box [0, 0, 0, 0])
CASES = [(41, {}), (42, {}), (43, dict(border=True)), (44, dict(zero_depth=True)), (45, dict(empty=True))]


def make_lmo_scene(seed, tmp_size=64, border=False, zero_depth=False, empty=False):
    """-> dict(img (H,W,3) u8, depth (H,W) u16 in millimetres, mask_label (H,W) bool, cls, cad_pts, cad_col)"""
    sc = make_scene(seed, n_obj=1, tmp_size=tmp_size)
    cls = int(sc["gt_obj"][0])
    img, label = sc["img"], sc["label"]
    depth = (sc["depth"].astype(np.float64) / 10).astype(np.uint16)              # ~0.6-1.4 m in millimetres
    ys, xs = np.nonzero(label == cls)
    if border:                                        # the whole frame moves left until the ellipse rests on column 0
        img, depth, label = (np.ascontiguousarray(np.roll(a, -int(xs.min()), axis=1)) for a in (img, depth, label))
        ys, xs = np.nonzero(label == cls)
    mask = label == cls
    H, W = mask.shape
    r0, c0, w = int(ys.min()), int(xs.min()), int(xs.max() - xs.min()) + 1
    h = int(ys.max()) - r0 + 1
    # two vertical bars, 3 px wide: pieces of about 0.55 w | 0.2 w | 0.2 w when the first piece has to be the largest (it
    # is the one on the border), else 0.22 w | 0.47 w | 0.25 w
    cuts = (0.55, 0.78) if border else (0.22, 0.72)
    for f in cuts:
        mask[:, c0 + int(f * w):c0 + int(f * w) + 3] = False
    rng = np.random.default_rng(1000 + seed)
    placed = 0
    while placed < 5:                                 # speckles: single pixels at least 4 px away from the object's rectangle
        y, x = int(rng.integers(0, H)), int(rng.integers(0, W))
        if r0 - 4 <= y <= r0 + h + 4 and c0 - 4 <= x <= c0 + w + 4:
            continue
        if mask[max(y - 1, 0):y + 2, max(x - 1, 0):x + 2].any():
            continue
        mask[y, x] = True
        placed += 1
    if zero_depth:
        depth = depth.copy()
        depth[mask] = 0
    if empty:
        mask = np.zeros_like(mask)
    return dict(img=img, depth=depth, mask_label=mask, cls=cls, cad_pts=sc["cad_pts"], cad_col=sc["cad_col"])
