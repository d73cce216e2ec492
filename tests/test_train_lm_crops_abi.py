"""The LineMOD training loader's front end without a GPU (csrc/crops_train_lm.hip, crops.py::build_train_lm's host parts): the
entry points are declared with the agreed argument lists, exported by both libraries and refuse bad arguments -- a paste plan
that names a pixel outside either frame included -- before any device work; the host twins, what the GPU tests compare the
kernels with, give what numpy restatements with REAL slicing and broadcasting give (mask extent and sum; the paste with its
commit / roll-back on a few hundred random cases on small frames of generic H, every branch counted; the float64 re-pose bit for
bit); `crops.lm_paste_plan` raises / does not raise where numpy does and reproduces the reference loader's recorded outcomes
(tests/golden/train_lm_crops_ref.npz); `crops.lm_other_index` consumes Python's generator as `get_other_idx` does; and the default
draw object consumes np.random and random exactly as the reference loader did on every golden scene.

The parity rule of the float64 re-pose: the reference's float64 `@` goes through a BLAS of unspecified summation order, so points,
rot_gt and trans_gt are required equal bit for bit EXCEPT where the float64 value lies within 8 * 2^-53 * sum|terms| of a float32
rounding boundary; there one float32 ulp is allowed.  The generator counted such elements in the fixture: near_boundary."""
import ctypes as C
import os
import random
import re
import zlib

import numpy as np
import pytest

import train_lm_scene as LS
from test_pointnet_grad_abi import _libs, declarations

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

POSED64 = ["const uint16_t *depth", "const int32_t *label", "const uint8_t *rgb", "int n_frames", "int H", "int W",
           "int rgb_channels", "int n_inst", "const int32_t *frame_idx_host", "const int32_t *src", "const float *cams",
           "const void *pose", "const double *rgb_mean_host", "const double *half_extent_host", "int min_valid", "int cap",
           "float *raw_xyz", "float *raw_rgb", "float *out_xyz", "float *out_rgb", "float *centroid", "int32_t *counts",
           "float *rot_gt", "float *trans_gt", "int32_t *ws", "dclStream_t stream"]
PASTE = ["const uint8_t *rgb", "const uint16_t *depth", "const uint8_t *mask", "int n", "int H", "int W", "int rgb_channels",
         "const uint8_t *other_rgb", "const uint16_t *other_depth", "const uint8_t *other_mask", "int n_other"]
WANT = {
    "dcl_mask_extent": ["const uint8_t *mask", "int n", "int H", "int W", "int32_t *out", "dclStream_t stream"],
    "dcl_mask_extent_host": ["const uint8_t *mask", "int n", "int H", "int W", "int32_t *out"],
    "dcl_occlude_paste": PASTE + ["const int32_t *plan_host", "const int32_t *plan", "const int32_t *extent", "uint8_t *out_rgb",
                                  "uint16_t *out_depth", "int32_t *out_label", "int64_t *info", "dclStream_t stream"],
    "dcl_occlude_paste_host": PASTE + ["const int32_t *plan", "const int32_t *extent", "uint8_t *out_rgb", "uint16_t *out_depth",
                                       "int32_t *out_label", "int64_t *info"],
    "dcl_crop_points_posed64": POSED64,
    "dcl_crop_repose64_host": ["const float *points", "const void *pose_row", "const float *centroid", "int n",
                               "const double *half_extent", "float *out_xyz", "uint8_t *inside", "float *out_R1", "float *out_t1"],
}
SEEDS = [s for s, _, _ in LS.CASES]
HALF3 = [LS.HALF] * 3


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "train_lm_crops_ref.npz"))


def scene(seed):
    kw = [k for s, k, _ in LS.CASES if s == seed][0]
    return LS.make_lm_scene(seed, tmp_size=LS.CFG["tmp_size"], **kw)


def test_header_declares_the_entry_points_and_the_abi_version_stays(dcl):
    decl = declarations()
    for name, args in WANT.items():
        assert name in decl, name
        assert decl[name] == args, (name, decl[name])
    posed = decl["dcl_crop_points_posed"]
    assert [a for a in POSED64 if a not in posed] == ["const double *half_extent_host"] and len(posed) == len(POSED64)
    text = open(os.path.join(ROOT, "include", "dclnet_hip.h")).read()
    assert re.search(r"#define DCL_ABI_VERSION 2\b", text)
    assert re.search(r"#define DCL_CROP_POSE_ROW_BYTES 112\b", text) and re.search(r"#define DCL_CROP_POSE_ROW64_BYTES 192\b", text)
    assert re.search(r"#define DCL_PASTE_PLAN_INTS 16\b", text)
    diag = text[text.index("#ifdef DCL_DIAG"):text.index("#endif /* DCL_DIAG */")]
    assert not [n for n in WANT if n in diag]
    assert "dcl_debug" not in "".join(WANT)


def test_both_libraries_export_them(dcl):
    assert os.path.exists(dcl._native.DIAG_SO_PATH), "diagnostic library missing: build() makes it"
    for tag, lib in _libs(dcl):
        for name in WANT:
            assert hasattr(lib, name), (tag, name)
        assert lib.dcl_abi_version() == 2, tag
    for name in ("mask_extent", "mask_extent_host", "occlude_paste", "occlude_paste_host", "pose_rows64", "crop_points_posed64",
                 "crop_repose64_host"):
        assert callable(getattr(dcl.ops, name)), name
    for name in ("lm_paste_plan", "lm_other_index"):
        assert callable(getattr(dcl.crops, name)), name
    assert callable(dcl.crops.CropBuilder.build_train_lm) and callable(dcl.crops.LoaderDraw.paste)
    assert dcl.ops.POSE_ROW64_BYTES == 192 == np.dtype(dcl.ops.POSE_ROW64).itemsize
    assert dcl.ops.PASTE_PLAN_INTS == 16 == len(dcl.ops.PASTE_PLAN)
    assert dcl.crops.LM_OBJLIST == LS.OBJLIST and dcl.crops.LM_TRAIN_SYMMETRY_OBJ_IDX == (7, 8) and dcl.crops.LM_TRAIN_MIN_PT == 128


FAKE = C.c_void_p(4096)          # a non-null, 8-byte aligned address that a call refusing its arguments never touches
GOOD_ROW = dict(enabled=1, other=0, py0=3, px0=4, ph=5, pw=6, ty0=10, tx0=20, th=5, tw=6, rep_y=0, rep_x=0, rmin=0, rmax=23, cmin=0, cmax=37)


def plan_row(dcl, **kw):
    d = dict(GOOD_ROW, **kw)
    return [d[k] for k in dcl.ops.PASTE_PLAN]


def _paste(L, row, host=False, null=None, n=1, H=23, W=37, ch=3, n_other=1):
    plan = (C.c_int32 * 16)(*row)
    ptrs = [FAKE] * 12
    if null is not None:
        ptrs[null] = None
    a = ptrs[:6]
    plan_p = C.cast(plan, C.c_void_p)
    if host:
        return L.dcl_occlude_paste_host(a[0], a[1], a[2], n, H, W, ch, a[3], a[4], a[5], n_other, plan_p if null != 6 else None,
                                        ptrs[7], ptrs[8], ptrs[9], ptrs[10], ptrs[11])
    return L.dcl_occlude_paste(a[0], a[1], a[2], n, H, W, ch, a[3], a[4], a[5], n_other, plan_p if null != 6 else None, ptrs[6] if null != 6 else FAKE,
                               ptrs[7], ptrs[8], ptrs[9], ptrs[10], ptrs[11], None)


def _posed64(L, n_frames=2, frames=(0, 1), null=None, cap=4096, **kw):
    fidx = (C.c_int32 * len(frames))(*frames)
    ptrs = [FAKE] * 18
    ptrs[3] = C.cast(fidx, C.c_void_p)
    mean, he = (C.c_double * 3)(0.485, 0.456, 0.406), (C.c_double * 3)(0.192, 0.192, 0.192)
    ptrs[7], ptrs[8] = C.cast(mean, C.c_void_p), C.cast(he, C.c_void_p)
    if null is not None:
        ptrs[null] = None
    depth, label, rgb, fi, src, cams, pose, mean_p, he_p = ptrs[:9]
    return L.dcl_crop_points_posed64(depth, label, rgb, n_frames, kw.get("H", 480), kw.get("W", 640), kw.get("ch", 3),
                                     kw.get("n_inst", len(frames)), fi, src, cams, pose, mean_p, he_p, kw.get("min_valid", 128), cap,
                                     *ptrs[9:], None)


BAD_ROWS = [dict(other=1), dict(other=-1), dict(py0=-1), dict(py0=19), dict(px0=32), dict(ph=-1, th=-1), dict(ty0=-1), dict(ty0=19),
            dict(tx0=32), dict(tw=-1, pw=-1), dict(ph=4), dict(pw=5), dict(ph=1), dict(rep_y=1), dict(rep_x=1), dict(pw=1),
            dict(rmin=-1), dict(rmax=24), dict(cmin=-1), dict(cmax=38), dict(enabled=0, rmax=24)]


@pytest.mark.parametrize("call", [
    lambda L, d: L.dcl_mask_extent(FAKE, -1, 480, 640, FAKE, None),
    lambda L, d: L.dcl_mask_extent(FAKE, 1, 0, 640, FAKE, None),
    lambda L, d: L.dcl_mask_extent(FAKE, 1, 65536, 32768, FAKE, None),                   # H * W = 2^31
    lambda L, d: L.dcl_mask_extent(None, 1, 480, 640, FAKE, None),
    lambda L, d: L.dcl_mask_extent(FAKE, 1, 480, 640, None, None),
    lambda L, d: L.dcl_mask_extent_host(None, 1, 480, 640, FAKE),
    lambda L, d: L.dcl_mask_extent_host(FAKE, 1, 480, 640, None),
    lambda L, d: L.dcl_mask_extent_host(FAKE, 1, 480, 0, FAKE),
    lambda L, d: _paste(L, plan_row(d), ch=2),
    lambda L, d: _paste(L, plan_row(d), n=-1),
    lambda L, d: _paste(L, plan_row(d), n_other=0),                                       # an enabled row without occluder frames
    lambda L, d: _paste(L, plan_row(d), host=True, ch=2),
] + [(lambda L, d, kw=kw, host=host: _paste(L, plan_row(d, **kw), host=host)) for kw in BAD_ROWS for host in (False, True)] + [
    (lambda L, d, i=i, host=host: _paste(L, plan_row(d), host=host, null=i)) for i in range(12) for host in (False, True)
    if not (host and i == 6)
] + [
    lambda L, d: _posed64(L, frames=(0, 2)),                                             # frame_idx out of range
    lambda L, d: _posed64(L, frames=(-1, 1)),
    lambda L, d: _posed64(L, n_frames=0, frames=(0,)),
    lambda L, d: _posed64(L, cap=0),
    lambda L, d: _posed64(L, ch=2),
    lambda L, d: _posed64(L, min_valid=-1),
] + [(lambda L, d, i=i: _posed64(L, null=i)) for i in range(18)] + [
    lambda L, d: L.dcl_crop_repose64_host(None, FAKE, FAKE, 4, None, FAKE, None, FAKE, FAKE),
    lambda L, d: L.dcl_crop_repose64_host(FAKE, None, FAKE, 4, None, FAKE, None, FAKE, FAKE),
    lambda L, d: L.dcl_crop_repose64_host(FAKE, FAKE, None, 4, None, FAKE, None, FAKE, FAKE),
    lambda L, d: L.dcl_crop_repose64_host(FAKE, FAKE, FAKE, 4, None, None, None, FAKE, FAKE),
    lambda L, d: L.dcl_crop_repose64_host(FAKE, FAKE, FAKE, 4, FAKE, FAKE, None, FAKE, FAKE),   # a half extent without `inside`
    lambda L, d: L.dcl_crop_repose64_host(FAKE, FAKE, FAKE, -1, None, FAKE, None, FAKE, FAKE),
])
def test_bad_arguments_return_einval_without_a_gpu(dcl, call):
    for tag, lib in _libs(dcl):
        lib.dcl_last_error.restype = C.c_char_p
        assert call(lib, dcl) == -1, tag
        assert b"invalid argument" in lib.dcl_last_error(), tag


def test_empty_calls_are_no_ops_without_a_gpu(dcl):
    for tag, lib in _libs(dcl):
        assert lib.dcl_mask_extent(None, 0, 480, 640, None, None) == 0, tag
        assert lib.dcl_mask_extent_host(None, 0, 480, 640, None) == 0, tag
        assert _paste(lib, plan_row(dcl), n=0) == 0 and _paste(lib, plan_row(dcl), n=0, host=True) == 0, tag
        assert _posed64(lib, frames=(), n_inst=0) == 0, tag
    assert dcl.ops.mask_extent_host(np.zeros((0, 23, 37, 3), np.uint8)).shape == (0, 6)


# ------------------------------------------------------------------------------------------------------------ mask extent
def extent_cases():
    """(name, masks (n,H,W,3) u8): random sparse and dense masks whose channels differ, an empty one, a single pixel in each corner,
    a mask whose channel 0 is empty while the others are not; at 23 x 37, 48 x 64 and the loader's size"""
    rng = np.random.default_rng(4)
    cases = []
    for H, W in ((23, 37), (48, 64), (LS.H, LS.W)):
        n = 6
        m = np.zeros((n, H, W, 3), np.uint8)
        m[0] = rng.integers(0, 256, (H, W, 3)) * (rng.random((H, W, 1)) < 0.02)
        m[1] = rng.integers(0, 256, (H, W, 3))
        m[3, 0, 0], m[3, H - 1, W - 1] = (255, 0, 7), (1, 2, 3)
        m[4, H // 2, W - 1, 0] = 9
        m[5, :, :, 1:] = 255
        cases.append(("%dx%d" % (H, W), m))
    return cases


def numpy_extent_rows(masks):
    out = np.zeros((masks.shape[0], 6), np.int32)
    for f, m in enumerate(masks):
        ext, total = LS.numpy_extent(m)
        out[f, :4] = ext
        out[f, 4:6] = np.array([total], np.int64).view(np.int32)
    return out


def test_mask_extent_host_equals_numpy(dcl):
    for name, m in extent_cases():
        got = dcl.ops.mask_extent_host(m)
        assert np.array_equal(got, numpy_extent_rows(m)), name
        assert np.array_equal(dcl.ops.extent_sums(got), m.reshape(m.shape[0], -1).sum(1, dtype=np.int64)), name
    assert tuple(got[2, :4]) == (2 ** 31 - 1, -1, 2 ** 31 - 1, -1) and tuple(got[5, :4]) == (2 ** 31 - 1, -1, 2 ** 31 - 1, -1)


# ------------------------------------------------------------------------------------------------------------ occlusion paste
def blob_mask(rng, H, W, kind):
    """an (H,W,3) u8 mask: a random rectangle of mostly-set pixels; kind picks its shape"""
    m = np.zeros((H, W, 3), np.uint8)
    if kind == "empty":
        return m
    h = 1 if kind == "row" else int(rng.integers(1, H // 2 if kind != "big" else H))
    w = 1 if kind == "col" else int(rng.integers(1, W // 2 if kind != "big" else W))
    if kind == "big":
        h, w = max(h, H - 3), max(w, W - 3)
    r0, c0 = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
    sub = (rng.random((h, w, 1)) < 0.8) * np.where(rng.random((h, w, 3)) < 0.9, 255, rng.integers(0, 256, (h, w, 3)))
    if kind in ("big", "row", "col") or rng.random() < 0.5:
        sub = np.full((h, w, 3), 255)
    sub[0, 0, 0] = sub[-1, -1, 0] = 255                                    # the extent is the rectangle
    m[r0:r0 + h, c0:c0 + w] = sub
    return m


def paste_cases(H, W, n, seed):
    """n random (own frame, occluder frame, starts, box) cases at H x W; the starts are drawn from the loader's range.  ->
    (rgb (n,H,W,C), depth, mask, other rgb, other depth, other mask, starts (n,2), boxes (n,4))"""
    rng = np.random.default_rng(seed)
    C_ = 3 if seed % 2 else 4
    rgb = rng.integers(0, 256, (n, H, W, C_), dtype=np.uint8)
    o_rgb = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    depth = (rng.integers(0, 5, (n, H, W)) * rng.integers(1, 9000, (n, H, W))).astype(np.uint16)
    o_depth = rng.integers(0, 65536, (n, H, W)).astype(np.uint16)
    kinds_own = ["blob", "blob", "blob", "tiny", "empty"]
    kinds_oth = ["blob", "blob", "big", "row", "col", "empty"]
    mask = np.stack([blob_mask(rng, H, W, kinds_own[i % len(kinds_own)]) if kinds_own[i % len(kinds_own)] != "tiny"
                     else tiny_mask(rng, H, W) for i in range(n)])
    o_mask = np.stack([blob_mask(rng, H, W, kinds_oth[(i // 2) % len(kinds_oth)]) for i in range(n)])
    starts, boxes = np.zeros((n, 2), np.int64), np.zeros((n, 4), np.int32)
    for i in range(n):
        own, _ = LS.numpy_extent(mask[i])
        oth, _ = LS.numpy_extent(o_mask[i])
        if own[1] >= 0 and oth[1] >= 0:
            oh, ow = oth[1] - oth[0] + 1, oth[3] - oth[2] + 1
            starts[i] = rng.integers(own[0] - oh + 1, own[1] + 1), rng.integers(own[2] - ow + 1, own[3] + 1)
        r0, c0 = int(rng.integers(0, H)), int(rng.integers(0, W))
        boxes[i] = r0, int(rng.integers(r0, H + 1)), c0, int(rng.integers(c0, W + 1))
    return rgb, depth, mask, o_rgb, o_depth, o_mask, starts, boxes


def tiny_mask(rng, H, W):
    """two pixels: an occluder that covers them leaves a sum below 20"""
    m = np.zeros((H, W, 3), np.uint8)
    r, c = int(rng.integers(1, H - 1)), int(rng.integers(1, W - 2))
    m[r, c:c + 2] = 255
    return m


def plans_of(dcl, H, W, mask, o_mask, starts, boxes, channels=3):
    n = mask.shape[0]
    plans = np.zeros((n, 16), np.int32)
    for i in range(n):
        own, _ = LS.numpy_extent(mask[i])
        oth, _ = LS.numpy_extent(o_mask[i])
        row = dcl.crops.lm_paste_plan(H, W, own, oth, starts[i, 0], starts[i, 1], channels)
        if row is not None:
            plans[i] = row
            plans[i, 1] = i
        plans[i, 12:16] = boxes[i]
    return plans


def numpy_paste(rgb, depth, mask, o_rgb, o_depth, o_mask, starts, boxes):
    """the restatement for every case -> (rgb', depth', label', committed, raised, mask sum afterwards, n_box_valid)"""
    outs = []
    for i in range(mask.shape[0]):
        own, _ = LS.numpy_extent(mask[i])
        oth, _ = LS.numpy_extent(o_mask[i])
        if own[1] < 0 or oth[1] < 0:
            im, de, ma, com, raised = rgb[i, :, :, :3].copy(), depth[i].copy(), mask[i].copy(), False, True
        else:
            im, de, ma, com, raised = LS.numpy_occlude(rgb[i, :, :, :3], depth[i], mask[i], o_rgb[i], o_depth[i], o_mask[i],
                                                       int(starts[i, 0]), int(starts[i, 1]))
        full = rgb[i].copy()
        full[:, :, :3] = im
        r0, r1, c0, c1 = boxes[i]
        nv = int(((ma[:, :, 0] == 255) & (de != 0))[r0:r1, c0:c1].sum())
        outs.append((full, de, ma[:, :, 0].astype(np.int32), com, raised, int(ma.sum(dtype=np.int64)), nv))
    return outs


PASTE_SIZES = [(23, 37, 150, 1), (48, 64, 150, 2)]


def check_paste(dcl, got, want, plans, mask, H, starts, o_mask, tally=None):
    g_rgb, g_dep, g_lab, info = got
    for i, (w_rgb, w_dep, w_lab, com, raised, msum, nv) in enumerate(want):
        assert (plans[i, 0] == 0) == raised, (i, "lm_paste_plan and numpy disagree on raising")
        assert np.array_equal(g_rgb[i], w_rgb) and np.array_equal(g_dep[i], w_dep) and np.array_equal(g_lab[i], w_lab), i
        assert bool(info[i, 0]) == com and int(info[i, 2]) == nv, (i, info[i], com, nv)
        orig = int(mask[i].sum(dtype=np.int64))
        assert int(info[i, 1]) == orig - int(info[i, 3])
        if com:
            assert int(info[i, 1]) == msum >= 20
        elif not raised:
            assert int(info[i, 1]) < 20 and msum == orig                   # rolled back: the mask is the original again
        else:
            assert int(info[i, 3]) == 0
        if tally is not None and not raised:
            oth, _ = LS.numpy_extent(o_mask[i])
            oh, ow = oth[1] - oth[0] + 1, oth[3] - oth[2] + 1
            sy, sx = int(starts[i, 0]), int(starts[i, 1])
            for key, hit in (("commit", com), ("roll-back", not com), ("rep_y", plans[i, 10]), ("rep_x", plans[i, 11]),
                             ("top", sy < 0), ("bottom", sy + oh > H), ("removed", info[i, 3] > 0), ("empty target", plans[i, 8] == 0 or plans[i, 9] == 0)):
                tally[key] = tally.get(key, 0) + bool(hit)
        if tally is not None and raised:
            own, _ = LS.numpy_extent(mask[i])
            oth, _ = LS.numpy_extent(o_mask[i])
            if own[1] >= 0 and oth[1] >= 0:
                sx, ow = int(starts[i, 1]), oth[3] - oth[2] + 1
                for key, hit in (("raised", True), ("left", sx < 0), ("x-limit", sx + ow > H)):
                    tally[key] = tally.get(key, 0) + bool(hit)
            else:
                tally["empty mask"] = tally.get("empty mask", 0) + 1


def test_occlude_paste_host_equals_the_numpy_restatement(dcl):
    tally = {}
    for H, W, n, seed in PASTE_SIZES:
        rgb, depth, mask, o_rgb, o_depth, o_mask, starts, boxes = paste_cases(H, W, n, seed)
        plans = plans_of(dcl, H, W, mask, o_mask, starts, boxes)
        want = numpy_paste(rgb, depth, mask, o_rgb, o_depth, o_mask, starts, boxes)
        got = dcl.ops.occlude_paste_host(rgb, depth, mask, o_rgb, o_depth, o_mask, plans)
        check_paste(dcl, got, want, plans, mask, H, starts, o_mask, tally)
    print("branches of the random cases:", tally)
    # (the loader's own slicing reaches a repeated axis only with an EMPTY target: hand_made_plans below covers the repeats)
    for key in ("commit", "roll-back", "top", "bottom", "removed", "raised", "left", "x-limit", "empty mask"):
        assert tally.get(key, 0) > 0, (key, tally)


def hand_made_plans(H=23, W=37, seed=9):
    """plan rows written by hand, with patches of ONE row and / or column that numpy's broadcast repeats over the target, beside
    plain ones and a disabled one -> the arrays of paste_cases and the plans"""
    rng = np.random.default_rng(seed)
    shapes = [(1, 6, 5, 6), (4, 1, 4, 7), (1, 1, 6, 5), (3, 4, 3, 4), (1, 1, 1, 1), (1, 5, 1, 5), (2, 1, 2, 1), (1, 3, 7, 3), (1, 1, H, W)]
    n = len(shapes) + 1
    rgb = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    o_rgb = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    depth = rng.integers(0, 3000, (n, H, W)).astype(np.uint16)
    o_depth = rng.integers(0, 65536, (n, H, W)).astype(np.uint16)
    mask = (rng.random((n, H, W, 3)) < 0.5).astype(np.uint8) * 255
    o_mask = (rng.random((n, H, W, 3)) < 0.6).astype(np.uint8) * rng.integers(1, 256, (n, H, W, 3)).astype(np.uint8)
    plans = np.zeros((n, 16), np.int32)
    for i, (ph, pw, th, tw) in enumerate(shapes):
        py0, px0 = int(rng.integers(0, H - ph + 1)), int(rng.integers(0, W - pw + 1))
        ty0, tx0 = int(rng.integers(0, H - th + 1)), int(rng.integers(0, W - tw + 1))
        plans[i, :12] = (1, (i + 1) % n, py0, px0, ph, pw, ty0, tx0, th, tw, ph == 1 and th != 1, pw == 1 and tw != 1)
    o_mask[(len(shapes)) % n, :, :, :] = 255                                 # the occluder of the last enabled row: covers everything
    plans[:, 12:16] = (2, H - 1, 3, W - 2)
    return rgb, depth, mask, o_rgb, o_depth, o_mask, plans


def numpy_apply_plan(rgb, depth, mask, o_rgb, o_depth, o_mask, row):
    """one plan row with REAL numpy broadcasting -> (rgb', depth', label', committed, mask sum afterwards, n_box_valid)"""
    en, k, py0, px0, ph, pw, ty0, tx0, th, tw = (int(v) for v in row[:10])
    image, dep, msk = rgb.copy(), depth.copy(), mask.copy()
    com = False
    if en:
        om = o_mask[k][py0:py0 + ph, px0:px0 + pw]
        oi, od = o_rgb[k][py0:py0 + ph, px0:px0 + pw].copy(), o_depth[k][py0:py0 + ph, px0:px0 + pw].copy()
        outline = om == 0
        image[ty0:ty0 + th, tx0:tx0 + tw] *= outline
        dep[ty0:ty0 + th, tx0:tx0 + tw] *= outline[:, :, 0]
        oi[om == 0] = 0
        od[outline[:, :, 0]] = 0
        image[ty0:ty0 + th, tx0:tx0 + tw] += oi
        dep[ty0:ty0 + th, tx0:tx0 + tw] += od
        msk[ty0:ty0 + th, tx0:tx0 + tw] *= outline
        com = msk.sum() >= 20
        if not com:
            image, dep, msk = rgb.copy(), depth.copy(), mask.copy()
    r0, r1, c0, c1 = (int(v) for v in row[12:16])
    nv = int(((msk[:, :, 0] == 255) & (dep != 0))[r0:r1, c0:c1].sum())
    return image, dep, msk[:, :, 0].astype(np.int32), bool(com), int(msk.sum(dtype=np.int64)), nv


def check_hand_made(got, arrays):
    rgb, depth, mask, o_rgb, o_depth, o_mask, plans = arrays
    g_rgb, g_dep, g_lab, info = got
    seen = set()
    for i in range(plans.shape[0]):
        w_rgb, w_dep, w_lab, com, msum, nv = numpy_apply_plan(rgb[i], depth[i], mask[i], o_rgb, o_depth, o_mask, plans[i])
        assert np.array_equal(g_rgb[i], w_rgb) and np.array_equal(g_dep[i], w_dep) and np.array_equal(g_lab[i], w_lab), i
        assert bool(info[i, 0]) == com and int(info[i, 2]) == nv, (i, info[i])
        if com:
            assert int(info[i, 1]) == msum
        if plans[i, 0]:
            seen.add((bool(plans[i, 10]), bool(plans[i, 11]), com))
    assert {(True, False, True), (False, True, True), (True, True, True), (False, False, True), (True, True, False)} <= seen, seen


def test_occlude_paste_host_repeats_one_row_or_column_patches_as_numpy_broadcasts(dcl):
    arrays = hand_made_plans()
    check_hand_made(dcl.ops.occlude_paste_host(*arrays), arrays)


def scene_plan(dcl, sc, golden, seed):
    """the plan row of a golden scene from the RECORDED starts (None: originals), the box clipped as numpy clips it"""
    box = dcl.crops.lm_box(sc["obj_bb"])
    assert tuple(box) == tuple(golden["l%d_box" % seed])
    row = np.zeros(16, np.int32)
    paste = golden["l%d_paste" % seed]
    if len(paste):
        own, _ = LS.numpy_extent(sc["mask"])
        oth, _ = LS.numpy_extent(sc["other"][2])
        plan = dcl.crops.lm_paste_plan(LS.H, LS.W, own, oth, paste[0], paste[1], sc["other"][0].shape[2])
        if plan is not None:
            row = plan
    row[12:16] = (max(box[0], 0), min(box[1], LS.H), max(box[2], 0), min(box[3], LS.W))
    return row


def box_crc(rgb, depth, label, box):
    r0, r1, c0, c1 = [int(v) for v in box]
    crc = zlib.crc32(np.ascontiguousarray(rgb[r0:r1, c0:c1, :3]).tobytes())
    crc = zlib.crc32(np.ascontiguousarray(depth[r0:r1, c0:c1]).astype(np.uint16).tobytes(), crc)
    return zlib.crc32(np.ascontiguousarray(label[r0:r1, c0:c1]).astype(np.int32).tobytes(), crc)


def scene_paste_host(dcl, sc, golden, seed):
    row = scene_plan(dcl, sc, golden, seed)
    oth = sc["other"] if sc["other"] is not None and sc["other"][0].shape[2] == 3 else None
    o = [np.zeros((0, LS.H, LS.W, 3), np.uint8), np.zeros((0, LS.H, LS.W), np.uint16), np.zeros((0, LS.H, LS.W, 3), np.uint8)] \
        if oth is None else [a[None] for a in oth]
    return row, dcl.ops.occlude_paste_host(sc["img"][None], sc["depth"][None], sc["mask"][None], o[0], o[1], o[2], row[None])


@pytest.mark.parametrize("seed", SEEDS)
def test_paste_plan_and_host_twin_reproduce_the_loaders_recorded_outcome(dcl, golden, seed):
    sc = scene(seed)
    tag = "l%d_" % seed
    row, (w_rgb, w_dep, w_lab, info) = scene_paste_host(dcl, sc, golden, seed)
    assert bool(info[0, 0]) == bool(golden[tag + "occluded"])
    assert int(info[0, 2]) == int(golden[tag + "n_choose"])
    assert box_crc(w_rgb[0], w_dep[0], w_lab[0], golden[tag + "box"]) == int(golden[tag + "crc"])
    if info[0, 0]:
        assert int(info[0, 1]) == int(golden[tag + "mask_sum"])
    else:
        assert int(golden[tag + "mask_sum"]) == int(sc["mask"].sum(dtype=np.int64))
        assert np.array_equal(w_rgb[0], sc["img"]) and np.array_equal(w_dep[0], sc["depth"])
    if seed in (74, 175, 82):
        assert row[0] == 0 and len(golden[tag + "paste"]) == 2            # the loader raised after its draws
    if seed == 76:
        assert row[0] == 1 and not info[0, 0] and info[0, 1] < 20          # pasted, then rolled back
    if seed == 77:
        assert len(golden[tag + "paste"]) == 0


def test_other_index_consumes_pythons_generator_as_get_other_idx_does(dcl):
    table = {1: [0, 180], 2: [180, 400], 8: [400, 417], 15: [417, 1000]}
    for obj in (1, 2, 8, 15):
        for seed in range(5):
            random.seed(seed)
            got = dcl.crops.lm_other_index(table, obj)
            state = random.getstate()
            random.seed(seed)
            start, stop = table[obj]
            want = random.choice(list(range(start)) + list(range(stop, table[15][1])))
            assert got == want and state == random.getstate(), (obj, seed)
    for obj in (8, 10):
        random.seed(3)
        assert dcl.crops.lm_other_index(LS.DICT_INDEX(obj), obj) == 1


# ------------------------------------------------------------------------------------------------------------ float64 re-pose
def scene_pose(dcl, golden, seed):
    """the golden scene's composite cloud, pose row and parts, from the recorded draws"""
    sc = scene(seed)
    _, (w_rgb, w_dep, w_lab, _) = scene_paste_host(dcl, sc, golden, seed)
    A = dcl.crops.euler2mat(*golden["l%d_angles" % seed])
    jit = golden["l%d_jitter" % seed]
    cloud, centroid, colours = LS.frame_cloud(w_rgb[0], w_dep[0], w_lab[0], golden["l%d_box" % seed])
    R0, t_gt = np.resize(np.array(sc["cam_R_m2c"]), (3, 3)), np.array(sc["cam_t_m2c"]) / 1000.0
    row = dcl.ops.pose_rows64([R0], [t_gt], [jit], [A])[0]
    return sc, cloud, centroid, colours, row, R0, A, t_gt, jit


POSED = [s for s in SEEDS if s != 278]
KEPT = [s for s in POSED if s != 79]


@pytest.mark.parametrize("seed", POSED)
def test_repose64_host_equals_the_stepwise_float64_restatement_bit_for_bit(dcl, golden, seed):
    _, cloud, centroid, _, row, R0, A, t_gt, jit = scene_pose(dcl, golden, seed)
    got, R1, t1, inside = dcl.ops.crop_repose64_host(cloud, row, centroid, HALF3)
    want, wR1, wt1, _ = LS.numpy_repose64(cloud, R0, A, t_gt, jit, centroid)
    assert np.array_equal(R1, wR1.astype(np.float32)) and np.array_equal(t1, wt1.astype(np.float32))
    assert np.array_equal(got, want.astype(np.float32))
    assert np.array_equal(inside, (np.abs(want) < LS.HALF).all(1))
    assert int(inside.sum()) == int(golden["l%d_m_inside" % seed])
    again = dcl.ops.crop_repose64_host(cloud, row, centroid)
    assert len(again) == 3 and np.array_equal(again[0], got)


def test_repose64_host_differs_from_the_float32_repose_and_keeps_the_identity(dcl):
    """the float64 finding in one place: on the same operands the float32 re-pose (crop_repose_host) rounds elsewhere"""
    rng = np.random.default_rng(12)
    p = rng.uniform(-0.2, 0.2, (4096, 3)).astype(np.float32)
    cen = rng.uniform(-1, 1, 3).astype(np.float32)
    R0, A, t, jit = LS.rotation(rng), dcl.crops.euler2mat(0.08, -0.05, 0.02), rng.normal(size=3), rng.uniform(-0.03, 0.03, 3)
    got64 = dcl.ops.crop_repose64_host(p, dcl.ops.pose_rows64([R0], [t], [jit], [A])[0], cen)[0]
    got32 = dcl.ops.crop_repose_host(p, dcl.ops.pose_rows([R0], [t], [jit], [A])[0], cen)[0]
    assert np.array_equal(got64, LS.numpy_repose64(p, R0, A, t, jit, cen)[0].astype(np.float32))
    assert (got64 != got32).mean() > 0.2
    eye = np.eye(3)
    row = dcl.ops.pose_rows64([eye], [cen.astype(np.float64)], [np.zeros(3)], [eye])[0]
    assert np.array_equal(dcl.ops.crop_repose64_host(p, row, cen)[0], p)    # t0 = 0, R = I: the identity, exactly


@pytest.mark.parametrize("seed", KEPT)
def test_repose64_host_equals_the_reference_under_the_parity_rule(dcl, golden, seed):
    tag = "l%d_" % seed
    _, cloud, centroid, colours, row, R0, A, t_gt, jit = scene_pose(dcl, golden, seed)
    posed, R1, t1, inside = dcl.ops.crop_repose64_host(cloud, row, centroid, HALF3)
    assert int(inside.sum()) == int(golden[tag + "m"])
    choice = golden[tag + "choice"]
    v64, wR1, wt1, T = LS.numpy_repose64(cloud, R0, A, t_gt, jit, centroid)
    ref = golden[tag + "feat_inp"]
    near = LS.near_f32_boundary(v64[inside][choice], T[inside][choice])
    assert LS.equal_under_the_rule(posed[inside][choice], ref[:, 4:7], near).all()
    assert LS.equal_under_the_rule(R1, golden[tag + "rot_gt"], LS.near_f32_boundary(wR1, np.abs(R0) @ np.abs(A))).all()
    assert LS.equal_under_the_rule(t1, golden[tag + "trans_gt"], LS.near_f32_boundary(wt1, np.abs(wt1))).all()
    assert np.array_equal(ref[:, 1:4], colours[inside][choice]) and (ref[:, 0] == 1).all()
    assert np.array_equal(golden[tag + "centroid"], centroid)
    assert len(golden["near_boundary"]) == len(KEPT) and (golden["near_boundary"] <= 0.001 * (ref[:, 4:7].size + 12)).all()


# ------------------------------------------------------------------------------------------------------------ draw order
@pytest.mark.parametrize("seed", SEEDS)
def test_default_draw_consumes_both_generators_as_the_loader_did(dcl, golden, seed):
    tag = "l%d_" % seed
    sc = scene(seed)
    np.random.seed(seed)
    random.seed(seed)
    draw = dcl.crops.LoaderDraw()
    assert dcl.crops.lm_other_index(LS.DICT_INDEX(sc["obj"]), sc["obj"]) == 1          # the caller's draw comes first (:296)
    ranges = None
    if len(golden[tag + "paste"]):
        own, _ = LS.numpy_extent(sc["mask"])
        oth, _ = LS.numpy_extent(sc["other"][2])
        oh, ow = oth[1] - oth[0] + 1, oth[3] - oth[2] + 1
        ranges = (own[0] - oh + 1, own[1] + 1, own[2] - ow + 1, own[3] + 1)
        assert list(draw.paste(*ranges)) == golden[tag + "paste"].tolist()
    if len(golden[tag + "angles"]):
        assert draw.angles() == golden[tag + "angles"].tolist()
        assert draw.jitter() == golden[tag + "jitter"].tolist()
    if tag + "choice" in golden.files:
        got = draw.choice(int(golden[tag + "m"]), LS.CFG["input_size"])
        assert np.array_equal(got, golden[tag + "choice"])
    # ... and nothing more: the next numbers of both streams are the ones a fresh replay of the loader's calls gives
    nxt = (np.random.random_sample(), random.random())
    np.random.seed(seed)
    random.seed(seed)
    random.choice([1])
    if ranges:
        np.random.randint(ranges[0], ranges[1])
        np.random.randint(ranges[2], ranges[3])
    for _ in golden[tag + "angles"]:
        np.random.uniform(-1, 1)
        random.uniform(-1, 1)
    if tag + "choice" in golden.files:
        m = int(golden[tag + "m"])
        np.random.choice(m, LS.CFG["input_size"], replace=m <= LS.CFG["input_size"])
    assert nxt == (np.random.random_sample(), random.random())


def test_scenes_are_what_they_claim(golden):
    """the fixture's own record of the cases"""
    occluded = {s: int(golden["l%d_occluded" % s]) for s in SEEDS}
    assert occluded == {71: 1, 72: 1, 73: 1, 74: 0, 175: 0, 76: 0, 77: 0, 278: 1, 79: 1, 80: 0, 81: 1, 82: 0}
    assert golden["l72_paste"][0] < 0 and golden["l74_paste"][1] < 0 and len(golden["l77_paste"]) == 0 and len(golden["l80_paste"]) == 0
    assert float(golden["l278_flag"]) == -1 and len(golden["l278_angles"]) == 0 and int(golden["l278_n_choose"]) == 0
    assert float(golden["l79_flag"]) == -1 and len(golden["l79_angles"]) == 3 and int(golden["l79_m_inside"]) <= 128
    assert 128 < int(golden["l80_m"]) <= LS.CFG["input_size"] and len(np.unique(golden["l80_choice"])) < LS.CFG["input_size"]
    assert float(golden["l81_sym"][0]) == 1 and float(golden["l82_sym"][0]) == 1 and float(golden["l71_sym"][0]) == 0
    assert int(golden["mismatches"].sum()) <= int(golden["near_boundary"].sum())
