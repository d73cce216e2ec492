"""Synthetic stand-ins for LineMOD TRAINING frames (LM/dataloader_train_LM.py): colour, 16-bit depth in millimetres, an
(H,W,3) object mask of 0 / 255, the meta entry (obj_bb, cam_R_m2c, cam_t_m2c) and the frame of ANOTHER object that
`occlude_with_another_object` pastes over it -- at the loader's 480 x 640, which its xmap / ymap fix.  Shared by the train-LM
crop tests, tools/bench_train_lm_crops.py and tests/golden/make_train_lm_crops_golden.py (the fixture holds the reference
loader's outputs and the draws it consumed; the scenes regenerate from their seeds).

The random starts of the paste are drawn by the loader from np.random, seeded with the scene's seed: they are inputs of the
scene.  Each case places its object and sizes its occluder so that the branch it names is likely, and the seed was picked so that
it is reached; the generator asserts every claim."""
import numpy as np

H, W = 480, 640
CFG = dict(input_size=256, tmp_size=64, unit_voxel_extent=[0.006] * 3, voxel_num_limit=[64] * 3, voxelization_mode=4)
LM_CAMERA = (325.26110, 242.04899, 572.41140, 573.57043)          # cx, cy, fx, fy (loader :111-114)
OBJLIST = (1, 2, 4, 5, 6, 8, 9, 10, 11, 12, 13, 14, 15)           # loader :43
HALF = 64 * 0.006 * 0.5                                           # total_voxel_extent[0] * 0.5 as the loader forms it (:40,200)
U64 = 2.0 ** -53                                                  # unit round-off of float64

# seed (also the seed of np.random / random for the loader run), keyword arguments, claim (asserted by the generator)
CASES = [
    (71, dict(own=(180, 200, 110, 120), occ=(70, 80)), "plain: the paste covers part of the object and is kept"),
    (72, dict(own=(0, 150, 90, 110), occ=(120, 60)), "start_y < 0: the patch loses its first rows"),
    (73, dict(own=(385, 160, 95, 100), occ=(110, 60)), "end_y > 480: the patch loses its last rows"),
    (74, dict(own=(200, 0, 100, 90), occ=(60, 130)), "start_x < 0: rows are trimmed, the shapes differ -> originals, draws consumed"),
    (175, dict(own=(150, 430, 100, 120), occ=(60, 90)), "end_x > 480: the row-trim quirk -> originals"),
    (76, dict(own=(220, 250, 22, 24), occ=(170, 170), occ_solid=True), "the occluder covers the whole object: sum < 20 -> roll-back"),
    (77, dict(own=(200, 220, 100, 110), occ=(60, 60), empty_other=True), "empty occluder mask: no draw, originals"),
    (278, dict(own=(200, 220, 100, 110), occ=(60, 70), zero_depth=True), "the pixels left have depth 0 inside the box: dummy before the pose draws"),
    (79, dict(own=(190, 210, 100, 110), occ=(50, 60), far=True), "at most 128 points inside the grid: dummy after the pose draws"),
    (80, dict(own=(230, 260, 15, 15), no_other=True, solid=True), "128 < m <= input_size: choice with replacement; no other frame"),
    (81, dict(own=(170, 190, 110, 120), occ=(70, 70), obj=10), "a symmetric object"),
    (82, dict(own=(180, 200, 110, 120), occ=(70, 80), other_rgba=True, obj=11), "occluder colour with 4 channels: originals after the draws; symmetric"),
]


def rotation(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def back_project(depth, rows, cols):
    """the loader's float32 back-projection (:164-173) of the given pixels, metres -> (n,3) float32"""
    cx, cy, fx, fy = LM_CAMERA
    pt2 = depth[rows, cols].astype(np.float32) / 1.0
    pt0 = (cols.astype(np.float32) - cx) * pt2 / fx
    pt1 = (rows.astype(np.float32) - cy) * pt2 / fy
    out = np.stack([pt0, pt1, pt2], 1) / 1000.0
    assert out.dtype == np.float32
    return out


def make_frame(rng, r0, c0, h, w, solid=False, channels=3):
    """one frame with an elliptic (or solid rectangular) object mask of 255 in rows r0 .. r0+h, columns c0 .. c0+w"""
    img = rng.integers(0, 256, (H, W, channels), dtype=np.uint8)
    depth = rng.integers(600, 1400, (H, W)).astype(np.uint16)
    depth[rng.random((H, W)) < 0.1] = 0                                    # sensor holes
    yy, xx = np.mgrid[0:h, 0:w]
    blob = np.ones((h, w), bool) if solid else ((yy - h / 2) / (h / 2)) ** 2 + ((xx - w / 2) / (w / 2)) ** 2 <= 1.0
    mask = np.zeros((H, W, 3), np.uint8)
    mask[r0:r0 + h, c0:c0 + w][blob] = 255
    z0 = int(rng.integers(850, 1100))
    surf = (z0 + 20 * np.sin(yy / 17.0) + 15 * np.cos(xx / 23.0) + rng.normal(0, 2, (h, w))).astype(np.uint16)
    sub = depth[r0:r0 + h, c0:c0 + w]
    holes = sub == 0
    sub[blob] = surf[blob]
    sub[holes] = 0
    return img, depth, mask


def make_lm_scene(seed, own=(180, 200, 110, 120), occ=(70, 80), occ_solid=False, solid=False, empty_other=False, no_other=False,
                  zero_depth=False, far=False, other_rgba=False, obj=8, tmp_size=64):
    """-> dict(img, depth u16, mask (H,W,3) u8, obj, obj_bb [x,y,w,h], cam_R_m2c (9 floats), cam_t_m2c (3 floats, mm),
    other (img, depth, mask) or None, cad_pts, cad_col)"""
    rng = np.random.default_rng(7000 + seed)
    r0, c0, h, w = own
    img, depth, mask = make_frame(rng, r0, c0, h, w, solid=solid)
    if zero_depth:
        depth[mask[:, :, 0] != 0] = 0
    other = None
    if not no_other:
        oh, ow = occ
        orow, ocol = int(rng.integers(0, H - oh)), int(rng.integers(0, W - ow))
        other = make_frame(rng, orow, ocol, oh, ow, solid=occ_solid, channels=4 if other_rgba else 3)
        if empty_other:
            other[2][:] = 0
    rows, cols = np.nonzero((mask[:, :, 0] != 0) & (depth != 0))
    cen = back_project(depth, rows, cols).astype(np.float64).mean(0) if rows.size else np.array([0.0, 0.0, 1.0])
    t = (cen + rng.uniform(-0.015, 0.015, 3)) * 1000.0
    if far:
        t[0] += 10000.0                                                    # 10 m off: the augmentation swings the cloud out of the grid
    cad_pts = {c: rng.uniform(-90, 90, (tmp_size, 3)) for c in OBJLIST}
    cad_col = {c: rng.uniform(0, 1, (tmp_size, 3)) - np.array([0.485, 0.456, 0.406]) for c in OBJLIST}
    return dict(img=img, depth=depth, mask=mask, obj=obj, obj_bb=[c0, r0, w, h], cam_R_m2c=[float(v) for v in rotation(rng).flatten()],
                cam_t_m2c=[float(v) for v in t], other=other, cad_pts=cad_pts, cad_col=cad_col)


def sample_of(sc):
    """the mapping CropBuilder.build_train_lm takes"""
    return {k: sc[k] for k in ("img", "depth", "mask", "obj", "obj_bb", "cam_R_m2c", "cam_t_m2c", "other")}


DICT_INDEX = lambda obj: {obj: [0, 1], 15: [1, 2]}                         # noqa: E731  two frames: this one, the other one


# ------------------------------------------------------------------------------------------------ restatements for the checks
def numpy_extent(mask):
    """(min row, max row, min col, max col) of mask[:, :, 0] != 0 and mask.sum(), as the loader forms them (:301-306,343)"""
    ys, xs = np.nonzero(mask[:, :, 0])
    if ys.size == 0:
        return (2 ** 31 - 1, -1, 2 ** 31 - 1, -1), int(mask.sum(dtype=np.int64))
    return (int(ys.min()), int(ys.max()), int(xs.min()), int(xs.max())), int(mask.sum(dtype=np.int64))


def numpy_occlude(image, depth, mask, other_image, other_depth, other_mask, start_y, start_x):
    """`occlude_with_another_object` from the draws on (:307-346), restated with REAL numpy slicing and broadcasting: -> (image,
    depth, mask, committed, raised).  The arrays passed in are not modified."""
    orig = (image.copy(), depth.copy(), mask.copy())
    image, depth, mask = image.copy(), depth.copy(), mask.copy()
    other_image, other_depth, other_mask = other_image.copy(), other_depth.copy(), other_mask.copy()
    try:
        oys, oxs = np.nonzero(other_mask[:, :, 0])
        oy0, oy1, ox0, ox1 = np.min(oys), np.max(oys), np.min(oxs), np.max(oxs)
        other_mask = other_mask[oy0:oy1 + 1, ox0:ox1 + 1]
        other_image = other_image[oy0:oy1 + 1, ox0:ox1 + 1]
        other_depth = other_depth[oy0:oy1 + 1, ox0:ox1 + 1]
        end_y = start_y + other_mask.shape[0]
        end_x = start_x + other_mask.shape[1]
        if start_y < 0:
            other_mask, other_image, other_depth = other_mask[-start_y:], other_image[-start_y:], other_depth[-start_y:]
            start_y = 0
        if end_y > image.shape[0]:
            end_y = image.shape[0]
            other_mask, other_image, other_depth = other_mask[:end_y - start_y], other_image[:end_y - start_y], other_depth[:end_y - start_y]
        if start_x < 0:
            other_mask, other_image, other_depth = other_mask[-start_x:], other_image[-start_x:], other_depth[-start_x:]
            start_x = 0
        if end_x > image.shape[0]:
            end_x = image.shape[0]
            other_mask, other_image, other_depth = other_mask[:end_x - start_x], other_image[:end_x - start_x], other_depth[:end_x - start_x]
        outline = other_mask == 0
        image[start_y:end_y, start_x:end_x] *= outline
        depth[start_y:end_y, start_x:end_x] *= outline[:, :, 0]
        other_image[other_mask == 0] = 0
        other_depth[(other_mask == 0)[:, :, 0]] = 0
        image[start_y:end_y, start_x:end_x] += other_image
        depth[start_y:end_y, start_x:end_x] += other_depth
        mask[start_y:end_y, start_x:end_x] *= (other_mask == 0)
        if mask.sum() >= 20:
            return image, depth, mask, True, False
        return orig + (False, False)
    except (ValueError, IndexError):
        return orig + (False, True)


def frame_cloud(img, depth, label0, box):
    """the loader's masked cloud inside `box` (:143-176) from a (composited) frame: (cloud centred (n,3) f32, centroid (3) f32,
    colours (n,3) f32), rows in ascending flat order of the box; label0 = channel 0 of the mask"""
    r0, r1, c0, c1 = [int(v) for v in box]
    sub = ((label0 == 255) & (depth != 0))[r0:r1, c0:c1]
    rows, cols = np.nonzero(sub)
    rows, cols = rows + r0, cols + c0
    cloud = back_project(depth, rows, cols)
    centroid = np.mean(cloud, axis=0)
    col = img[:, :, :3][rows, cols].astype(np.float32) / 255.0 - np.array([0.485, 0.456, 0.406])[np.newaxis, :]
    return cloud - centroid[np.newaxis, :], centroid, col.astype(np.float32)


def numpy_repose64(p, R0, A, t_gt, jit, centroid):
    """the float64 re-pose step by step in the order include/dclnet_hip.h states (elementwise numpy float64: one rounding per
    operation, no matrix product) -> (points (n,3) f64, R1 (3,3) f64, t1 (3) f64, T (n,3): the sum of the magnitudes of all terms
    of a coordinate, what the parity rule's bound is taken of)"""
    R0, A, jit = np.asarray(R0, np.float64), np.asarray(A, np.float64), np.asarray(jit, np.float64)
    p = np.asarray(p, np.float32).astype(np.float64)
    t0 = np.asarray(t_gt, np.float64) - np.asarray(centroid, np.float32).astype(np.float64)
    t1 = t0 + jit
    R1 = np.array([[(R0[i, 0] * A[0, j] + R0[i, 1] * A[1, j]) + R0[i, 2] * A[2, j] for j in range(3)] for i in range(3)])
    d = p - t0[None, :]
    q = np.stack([(d[:, 0] * R0[0, j] + d[:, 1] * R0[1, j]) + d[:, 2] * R0[2, j] for j in range(3)], 1)
    r = np.stack([(q[:, 0] * R1[i, 0] + q[:, 1] * R1[i, 1]) + q[:, 2] * R1[i, 2] for i in range(3)], 1)
    S = np.abs(d) @ np.abs(R0)
    SR = np.abs(R0) @ np.abs(A)
    T = S @ np.abs(R1).T + np.abs(q) @ SR.T + np.abs(q) @ np.abs(R1).T + np.abs(r) + np.abs(t1)[None, :]
    return r + t1[None, :], R1, t1, T


def near_f32_boundary(v, T):
    """elements of the float64 array v that lie within 8 * 2^-53 * T of a float32 ROUNDING boundary (the midpoint of two
    neighbouring float32 numbers): two float64 evaluations that sum the same terms in another order, or fused, may round to
    different float32 numbers only there"""
    v = np.asarray(v, np.float64)
    f = v.astype(np.float32)
    up, dn = np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf))
    m_up, m_dn = (f.astype(np.float64) + up.astype(np.float64)) / 2, (f.astype(np.float64) + dn.astype(np.float64)) / 2
    return np.minimum(np.abs(v - m_up), np.abs(v - m_dn)) <= 8.0 * U64 * np.asarray(T, np.float64)


def equal_under_the_rule(got, ref, near):
    """bit for bit, except where `near`: there one float32 ulp is allowed"""
    got, ref = np.asarray(got, np.float32), np.asarray(ref, np.float32)
    ulp = (got == np.nextafter(ref, np.float32(np.inf))) | (got == np.nextafter(ref, np.float32(-np.inf)))
    return (got == ref) | (np.asarray(near, bool) & ulp)
