"""Synthetic stand-ins for YCB-V TRAINING frames: `synth.make_frame` (tests/crop_scene.py) with the poses replaced by proper
rotations and translations that lie within a few centimetres of their object's back-projected centroid, so that the cloud the
training loader re-poses (YCBV/dataloader_train_YCBV.py:171-174) stays inside the 0.384 m voxel grid.  Shared by the
train-crop tests, tools/bench_train_crops.py and tests/golden/make_train_crops_golden.py (the fixture holds the reference
loader's outputs and the draws it consumed; the scenes regenerate from their seeds)."""
import numpy as np

from crop_scene import make_scene

CFG = dict(input_size=128, tmp_size=64, unit_voxel_extent=[0.006] * 3, voxel_num_limit=[64] * 3, voxelization_mode=4)
CAMERAS = {1: (312.9869, 241.3109, 1066.778, 1067.487), 2: (323.7872, 279.6921, 1077.836, 1078.189)}   # loader :83-91
FACTOR_DEPTH = 10000
# seed (also the seed of np.random / random for the loader run), keyword arguments, what the generator asserts of the scene
CASES = [
    (51, {}, "plain"),
    (52, dict(camera=2), "second camera"),
    (53, dict(repick=True), "the first pick has <= 50 valid pixels: the pick loop repeats"),
    (54, dict(tall=True), "fewer than 50 masked pixels inside the box: the dummy of :139"),
    (55, dict(far=True), "at most 50 points inside the grid after the re-pose: the dummy of :191"),
    (56, dict(small=True), "m <= input_size points: the choice is made with replacement"),
    (57, dict(border=True), "the box touches the image border"),
]


def _rotation(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def back_project(depth, rows, cols, cam, scale=FACTOR_DEPTH):
    """the loader's float32 back-projection (:146-154) of the given pixels -> (n,3) float32"""
    cx, cy, fx, fy = cam
    d = depth[rows, cols].astype(np.float32)
    pt2 = d / np.float32(scale)
    pt0 = (cols.astype(np.float32) - np.float32(cx)) * pt2 / np.float32(fx)
    pt1 = (rows.astype(np.float32) - np.float32(cy)) * pt2 / np.float32(fy)
    return np.stack([pt0, pt1, pt2], 1)


def make_train_scene(seed, tmp_size=64, camera=1, repick=False, tall=False, far=False, small=False, border=False, n_obj=4):
    """-> dict(img, depth u16, label i32, meta {cls_indexes, poses (3,4,k), factor_depth, camera}, cad_pts, cad_col)"""
    one = tall or small or border
    k = 1 if one else n_obj
    tiny = None
    if repick:                                        # the object np.random.seed(seed) picks FIRST gets a 24-pixel mask
        tiny = int(np.random.RandomState(seed).randint(0, k))
    if small:
        tiny = 0
    sc = make_scene(seed, n_obj=k, tmp_size=tmp_size, tiny=tiny)
    img, depth, label = sc["img"], sc["depth"], sc["label"]
    classes = sc["gt_obj"]
    rng = np.random.default_rng(5000 + seed)
    if small:                                         # the 4 x 6 mask grows to 9 x 12: 51 .. 108 valid pixels, fewer than input_size
        cls = int(classes[0])
        ys, xs = np.nonzero(label == cls)
        r0, c0 = min(int(ys.min()), label.shape[0] - 9), min(int(xs.min()), label.shape[1] - 12)
        label[label == cls] = 0
        label[r0:r0 + 9, c0:c0 + 12] = cls
        z0 = int(rng.integers(7000, 12000))
        sub = depth[r0:r0 + 9, c0:c0 + 12]
        holes = sub == 0
        sub[:] = (z0 + rng.normal(0, 15, sub.shape)).astype(np.uint16)
        sub[holes] = 0
    if border:                                        # the frame moves up and left until the mask rests on row 0 and column 0
        ys, xs = np.nonzero(label == int(classes[0]))
        img, depth, label = (np.ascontiguousarray(np.roll(a, (-int(ys.min()), -int(xs.min())), axis=(0, 1)))
                             for a in (img, depth, label))
    if tall:
        # a frame TALLER than the loader's 480 rows whose object lies mostly below row 480: get_bbox pushes the box back
        # above row 480 (:310-313), where 1 .. 49 masked pixels with depth are left
        cls = int(classes[0])
        mask = (label == cls) & (depth != 0)
        per_row = mask.sum(1)
        top = int(np.nonzero(label == cls)[0].min())
        rows_in = int(np.searchsorted(np.cumsum(per_row[top:]), 50, side="left"))      # rows of the mask with < 50 pixels in all
        assert rows_in >= 1 and 0 < per_row[top:top + rows_in].sum() < 50
        shift = 480 - (top + rows_in)                 # mask rows top .. top + rows_in - 1 end at row 479
        assert shift > 0

        def down(a, fill):
            out = np.full((shift + a.shape[0],) + a.shape[1:], fill, a.dtype)
            out[shift:] = a
            return out
        img, depth, label = down(img, 0), down(depth, 0), down(label, 0)
    cam = CAMERAS[camera]
    poses = np.zeros((3, 4, k))
    for i, cls in enumerate(classes):
        rows, cols = np.nonzero((label == int(cls)) & (depth != 0))
        cen = back_project(depth, rows, cols, cam).astype(np.float64).mean(0) if rows.size else np.array([0.0, 0.0, 0.8])
        poses[:, 0:3, i] = _rotation(rng)
        poses[:, 3, i] = cen + rng.uniform(-0.02, 0.02, 3)
        if far:                                       # the ground-truth translation 10 m off: the augmentation rotation then
            poses[0, 3, i] += 10.0                    # swings the re-posed cloud out of the grid
    meta = {"cls_indexes": classes.reshape(-1, 1).astype(np.uint8), "poses": poses,
            "factor_depth": np.array([[FACTOR_DEPTH]], np.uint16), "camera": cam}
    return dict(img=img, depth=depth, label=label, meta=meta, cad_pts=sc["cad_pts"], cad_col=sc["cad_col"])


# ------------------------------------------------------------------------------------------------ restatements for the checks
def frame_cloud(sc, cls, box):
    """the loader's masked cloud of class `cls` inside `box` (:138-158): (cloud centred (n,3) f32, centroid (3) f32,
    colours (n,3) f32), rows in ascending flat order of the box"""
    r0, r1, c0, c1 = [int(v) for v in box]
    mask = (sc["label"] == cls) & (sc["depth"] != 0)
    sub = mask[r0:r1, c0:c1]
    rows, cols = np.nonzero(sub)
    rows, cols = rows + r0, cols + c0
    cloud = back_project(sc["depth"], rows, cols, sc["meta"]["camera"])
    centroid = np.mean(cloud, axis=0)
    col = sc["img"][:, :, :3][rows, cols].astype(np.float32) / 255.0 - np.array([0.485, 0.456, 0.406])[np.newaxis, :]
    return cloud - centroid[np.newaxis, :], centroid, col.astype(np.float32)


U = 2.0 ** -24          # unit round-off of float32


def repose_bound(p, R0, A, t0, t1):
    """Per coordinate, how far two float32 evaluations of the loader's re-pose may lie apart when they evaluate the same
    subtraction, the same two 3-term dot products and the same addition but sum the dot products in a different order or
    with fused multiply-adds (torch's CPU `@` goes through a BLAS that specifies neither).  p (n,3) centred points.

      d = p - t0          one float32 operation on identical operands: identical on both sides.
      q_k = sum_m d_m R0[m][k]     any evaluation of a 3-term dot product lies within gamma_3 * S of the exact value,
                          S_k = sum_m |d_m| |R0[m][k]|, gamma_3 = 3u / (1 - 3u): two evaluations differ by <= 6u S_k (+ O(u^2))
      R1 = R0 A           the same for its nine elements: <= 6u SR[i][k], SR[i][k] = sum_m |R0[i][m]| |A[m][k]|
      r_i = sum_k q_k R1[i][k]     inherits sum_k |dq_k| |R1[i][k]| + sum_k |q_k| |dR1[i][k]| and adds its own 6u sum_k |q_k R1[i][k]|
      p'_i = r_i + t1_i   t1 = t0 + j is identical on both sides; one rounding per side: <= 2u (|r_i| + |t1_i|)
    Altogether <= 6u (sum_k S_k |R1[i][k]| + sum_k |q_k| SR[i][k] + sum_k |q_k R1[i][k]|) + 2u (|r_i| + |t1_i|); the bound
    is 8u * T_i with T_i the sum of all five magnitudes -- the factor 8 instead of 6 and 2 pays for the second-order terms.
    -> (bound (n,3), T (n,3)) float64"""
    p, R0, A, t0, t1 = (np.asarray(a, np.float64) for a in (p, R0, A, t0, t1))
    d = np.abs(p - t0)
    S = d @ np.abs(R0)
    q = np.abs((p - t0) @ R0)
    R1 = np.abs(R0 @ A)
    SR = np.abs(R0) @ np.abs(A)
    r = np.abs(((p - t0) @ R0) @ (R0 @ A).T)
    T = S @ R1.T + q @ SR.T + q @ R1.T + r + np.abs(t1)[None, :]
    return 8.0 * U * T, T


def near_voxel_border(xyz, bound, half, unit):
    """points whose voxel index `trunc((xyz + half) / unit)` (float32, :203) could differ when a coordinate moves by `bound`:
    the two float32 roundings of the index expression are added to the bound.  -> (n) bool"""
    x = np.asarray(xyz, np.float64)
    b = bound + 2.0 * U * (np.abs(x) + half) + 2.0 * U * np.abs(x + half)
    lo, hi = np.floor((x - b + half) / unit), np.floor((x + b + half) / unit)
    return (lo != hi).any(1)
