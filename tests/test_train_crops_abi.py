"""The training loader's front end without a GPU: the entry points of csrc/crops_train.hip are declared with the agreed argument
lists, exported by both libraries and refuse bad arguments before any device work; the host twins -- what the GPU tests compare
the kernels with -- give what numpy restatements give (the class table, the re-pose bit for bit); `crops.extent_box` returns
the reference `get_bbox`'s values; the host twin's re-posed coordinates lie within the derived bound of the reference loader's
(tests/golden/train_crops_ref.npz, tests/train_scene.py::repose_bound); and the default draw object consumes np.random and
random exactly as the reference loader did on every golden scene."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

import train_scene as TS
from test_pointnet_grad_abi import _libs, declarations

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WANT = {
    "dcl_label_table": ["const int32_t *label", "const uint16_t *depth", "int n", "int H", "int W", "int n_classes",
                        "int32_t *out", "dclStream_t stream"],
    "dcl_label_table_host": ["const int32_t *label", "const uint16_t *depth", "int n", "int H", "int W", "int n_classes",
                             "int32_t *out"],
    "dcl_crop_points_posed": ["const uint16_t *depth", "const int32_t *label", "const uint8_t *rgb", "int n_frames", "int H",
                              "int W", "int rgb_channels", "int n_inst", "const int32_t *frame_idx_host", "const int32_t *src",
                              "const float *cams", "const void *pose", "const double *rgb_mean_host",
                              "const float *half_extent_host", "int min_valid", "int cap", "float *raw_xyz", "float *raw_rgb",
                              "float *out_xyz", "float *out_rgb", "float *centroid", "int32_t *counts", "float *rot_gt",
                              "float *trans_gt", "int32_t *ws", "dclStream_t stream"],
    "dcl_crop_repose_host": ["const float *points", "const void *pose_row", "const float *centroid", "int n", "float *out_xyz",
                             "float *out_R1", "float *out_t1"],
}


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "train_crops_ref.npz"))


def test_header_declares_the_entry_points_and_the_abi_version_stays():
    decl = declarations()
    for name, args in WANT.items():
        assert name in decl, name
        assert decl[name] == args, (name, decl[name])
    text = open(os.path.join(ROOT, "include", "dclnet_hip.h")).read()
    assert re.search(r"#define DCL_ABI_VERSION 2\b", text)
    assert re.search(r"#define DCL_CROP_POSE_ROW_BYTES 112\b", text)
    diag = text[text.index("#ifdef DCL_DIAG"):text.index("#endif /* DCL_DIAG */")]
    assert "dcl_label_table" not in diag and "dcl_crop_points_posed" not in diag


def test_both_libraries_export_them(dcl):
    assert os.path.exists(dcl._native.DIAG_SO_PATH), "diagnostic library missing: build() makes it"
    for tag, lib in _libs(dcl):
        for name in WANT:
            assert hasattr(lib, name), (tag, name)
        assert lib.dcl_abi_version() == 2, tag
    for name in ("label_table", "label_table_host", "crop_points_posed", "crop_repose_host", "pose_rows"):
        assert callable(getattr(dcl.ops, name)), name
    assert callable(dcl.crops.extent_box) and callable(dcl.crops.CropBuilder.build_train)
    assert dcl.ops.POSE_ROW_BYTES == 112 == np.dtype(dcl.ops.POSE_ROW).itemsize


FAKE = C.c_void_p(4096)          # a non-null address that a call refusing its arguments never touches


def _posed(L, n_frames=2, frames=(0, 1), null=None, cap=4096, **kw):
    """dcl_crop_points_posed with fake device pointers; null: the index of a pointer argument to pass as NULL"""
    fidx = (C.c_int32 * len(frames))(*frames)
    ptrs = [FAKE] * 18
    ptrs[3] = C.cast(fidx, C.c_void_p)
    mean, he = (C.c_double * 3)(0.485, 0.456, 0.406), (C.c_float * 3)(0.192, 0.192, 0.192)
    ptrs[7], ptrs[8] = C.cast(mean, C.c_void_p), C.cast(he, C.c_void_p)
    if null is not None:
        ptrs[null] = None
    depth, label, rgb, fi, src, cams, pose, mean_p, he_p = ptrs[:9]
    return L.dcl_crop_points_posed(depth, label, rgb, n_frames, kw.get("H", 480), kw.get("W", 640), kw.get("ch", 3),
                                   kw.get("n_inst", len(frames)), fi, src, cams, pose, mean_p, he_p, kw.get("min_valid", 50), cap,
                                   *ptrs[9:], None)


@pytest.mark.parametrize("call", [
    lambda L: L.dcl_label_table(FAKE, FAKE, 1, 480, 640, 257, FAKE, None),               # n_classes > 256
    lambda L: L.dcl_label_table(FAKE, FAKE, 1, 480, 640, 0, FAKE, None),
    lambda L: L.dcl_label_table(FAKE, FAKE, -1, 480, 640, 22, FAKE, None),
    lambda L: L.dcl_label_table(FAKE, FAKE, 1, 0, 640, 22, FAKE, None),
    lambda L: L.dcl_label_table(FAKE, FAKE, 1, 65536, 32768, 22, FAKE, None),            # H * W = 2^31
    lambda L: L.dcl_label_table(None, FAKE, 1, 480, 640, 22, FAKE, None),                # a null pointer, each in turn
    lambda L: L.dcl_label_table(FAKE, None, 1, 480, 640, 22, FAKE, None),
    lambda L: L.dcl_label_table(FAKE, FAKE, 1, 480, 640, 22, None, None),
    lambda L: L.dcl_label_table_host(FAKE, FAKE, 1, 480, 640, 257, FAKE),
    lambda L: L.dcl_label_table_host(None, FAKE, 1, 480, 640, 22, FAKE),
    lambda L: L.dcl_label_table_host(FAKE, None, 1, 480, 640, 22, FAKE),
    lambda L: L.dcl_label_table_host(FAKE, FAKE, 1, 480, 640, 22, None),
    lambda L: _posed(L, frames=(0, 2)),                                                  # frame_idx out of range
    lambda L: _posed(L, frames=(-1, 1)),
    lambda L: _posed(L, n_frames=0, frames=(0,)),
    lambda L: _posed(L, cap=0),
    lambda L: _posed(L, ch=2),
    lambda L: _posed(L, min_valid=-1),
] + [(lambda L, i=i: _posed(L, null=i)) for i in range(18)] + [
    lambda L: L.dcl_crop_repose_host(None, FAKE, FAKE, 4, FAKE, FAKE, FAKE),
    lambda L: L.dcl_crop_repose_host(FAKE, None, FAKE, 4, FAKE, FAKE, FAKE),
    lambda L: L.dcl_crop_repose_host(FAKE, FAKE, None, 4, FAKE, FAKE, FAKE),
    lambda L: L.dcl_crop_repose_host(FAKE, FAKE, FAKE, 4, None, FAKE, FAKE),
    lambda L: L.dcl_crop_repose_host(FAKE, FAKE, FAKE, -1, FAKE, FAKE, FAKE),
])
def test_bad_arguments_return_einval_without_a_gpu(dcl, call):
    for tag, lib in _libs(dcl):
        lib.dcl_last_error.restype = C.c_char_p
        assert call(lib) == -1, tag
        assert b"invalid argument" in lib.dcl_last_error(), tag


def test_empty_calls_are_no_ops_without_a_gpu(dcl):
    for tag, lib in _libs(dcl):
        assert lib.dcl_label_table(None, None, 0, 480, 640, 22, None, None) == 0, tag
        assert lib.dcl_label_table_host(None, None, 0, 480, 640, 22, None) == 0, tag
        assert _posed(lib, frames=(), n_inst=0) == 0, tag
    assert dcl.ops.label_table_host(np.zeros((0, 37, 70), np.int32), np.zeros((0, 37, 70), np.uint16), 22).shape == (0, 22, 5)


def numpy_table(label, depth, n_classes):
    out = np.zeros((label.shape[0], n_classes, 5), np.int32)
    out[:, :, 1], out[:, :, 3], out[:, :, 2], out[:, :, 4] = 2 ** 31 - 1, 2 ** 31 - 1, -1, -1
    for f in range(label.shape[0]):
        for c in range(n_classes):
            m = label[f] == c
            out[f, c, 0] = int((m & (depth[f] != 0)).sum())
            if m.any():
                ys, xs = np.nonzero(m)
                out[f, c, 1:] = ys.min(), ys.max(), xs.min(), xs.max()
    return out


def table_cases():
    """(name, label (n,H,W) i32, depth (n,H,W) u16, n_classes): random label images, labels outside the range (negative and
    too large), an all-zero depth, a one-class image, and the golden scenes' frames"""
    rng = np.random.default_rng(3)
    cases = []
    for n, H, W in ((1, 37, 70), (3, 37, 70)):
        lab = rng.integers(0, 22, (n, H, W)).astype(np.int32)
        dep = (rng.integers(0, 3, (n, H, W)) * 500).astype(np.uint16)
        cases.append(("random %d" % n, lab, dep, 22))
        wild = rng.integers(-5, 40, (n, H, W)).astype(np.int32)
        wild[0, 0, 0], wild[0, -1, -1] = -2 ** 31, 2 ** 31 - 1
        cases.append(("outside the range %d" % n, wild, dep, 22))
        cases.append(("all-zero depth %d" % n, lab, np.zeros_like(dep), 22))
        cases.append(("256 classes %d" % n, rng.integers(0, 256, (n, H, W)).astype(np.int32), dep, 256))
        cases.append(("one class %d" % n, np.full((n, H, W), 7, np.int32), dep, 8))
    return cases


def scene_frames():
    scs = [TS.make_train_scene(seed, tmp_size=TS.CFG["tmp_size"], **kw) for seed, kw, _ in TS.CASES[:3]]
    return np.stack([s["label"] for s in scs]).astype(np.int32), np.stack([s["depth"] for s in scs])


def test_label_table_host_equals_numpy(dcl):
    for name, lab, dep, ncls in table_cases():
        assert np.array_equal(dcl.ops.label_table_host(lab, dep, ncls), numpy_table(lab, dep, ncls)), name
    lab, dep = scene_frames()
    assert np.array_equal(dcl.ops.label_table_host(lab, dep, 22), numpy_table(lab, dep, 22))


def test_extent_box_equals_the_reference_get_bbox(dcl, golden):
    for ext, want in zip(golden["bbox_extent"], golden["bbox_value"]):
        assert tuple(dcl.crops.extent_box(*ext)) == tuple(want), (ext.tolist(), want.tolist())
    for seed, kw, _ in TS.CASES:
        sc = TS.make_train_scene(seed, tmp_size=TS.CFG["tmp_size"], **kw)
        obj = int(golden["t%d_obj" % seed])
        ys, xs = np.nonzero(sc["label"] == obj)
        assert tuple(dcl.crops.extent_box(ys.min(), ys.max(), xs.min(), xs.max())) == tuple(golden["t%d_box" % seed]), seed


def numpy_repose(p, R0, A, t_gt, jit, centroid):
    """the re-pose step by step in numpy float32, in the order include/dclnet_hip.h states (no matrix product: numpy's would
    choose its own summation order)"""
    f = np.float32
    R0, A, jit, p = R0.astype(f), A.astype(f), np.asarray(jit).astype(f), p.astype(f)
    t0 = (np.asarray(t_gt, np.float64) - centroid.astype(np.float64)).astype(f)
    t1 = t0 + jit
    R1 = np.empty((3, 3), f)
    for i in range(3):
        for j in range(3):
            R1[i, j] = f(f(f(R0[i, 0] * A[0, j]) + f(R0[i, 1] * A[1, j])) + f(R0[i, 2] * A[2, j]))
    d = p - t0[None, :]
    q = np.stack([(d[:, 0] * R0[0, j] + d[:, 1] * R0[1, j]) + d[:, 2] * R0[2, j] for j in range(3)], 1)
    r = np.stack([(q[:, 0] * R1[i, 0] + q[:, 1] * R1[i, 1]) + q[:, 2] * R1[i, 2] for i in range(3)], 1)
    assert d.dtype == q.dtype == r.dtype == f
    return r + t1[None, :], R1, t1


def scene_pose(dcl, golden, seed, kw):
    """the golden scene's cloud, pose row and parts, from the recorded draws"""
    sc = TS.make_train_scene(seed, tmp_size=TS.CFG["tmp_size"], **kw)
    obj, box = int(golden["t%d_obj" % seed]), golden["t%d_box" % seed]
    idx = int(golden["t%d_picks" % seed][-1])
    P = sc["meta"]["poses"][:, :, idx]
    A = dcl.crops.euler2mat(*golden["t%d_angles" % seed])
    jit = golden["t%d_jitter" % seed]
    cloud, centroid, colours = TS.frame_cloud(sc, obj, box)
    row = dcl.ops.pose_rows([P[:, 0:3]], [P[:, 3]], [jit], [A])[0]
    return sc, cloud, centroid, colours, row, P, A, jit


POSED = [(seed, kw) for seed, kw, _ in TS.CASES if not kw.get("tall")]


@pytest.mark.parametrize("seed,kw", POSED)
def test_repose_host_equals_the_stepwise_float32_restatement_bit_for_bit(dcl, golden, seed, kw):
    _, cloud, centroid, _, row, P, A, jit = scene_pose(dcl, golden, seed, kw)
    got, R1, t1 = dcl.ops.crop_repose_host(cloud, row, centroid)
    want, wR1, wt1 = numpy_repose(cloud, P[:, 0:3], A, P[:, 3], jit, centroid)
    assert np.array_equal(R1, wR1) and np.array_equal(t1, wt1)
    assert np.array_equal(got, want)


def test_repose_host_on_adversarial_rows(dcl):
    """identity pose, zero jitter, and a random pose with large offsets: bit for bit against the restatement"""
    rng = np.random.default_rng(11)
    p = rng.uniform(-0.2, 0.2, (257, 3)).astype(np.float32)
    cen = rng.uniform(-1, 1, 3).astype(np.float32)
    eye = np.eye(3)
    for R0, A, t, jit in ((eye, eye, cen.astype(np.float64), np.zeros(3)), (TS._rotation(rng), eye, rng.normal(size=3), np.zeros(3)),
                          (TS._rotation(rng), dcl.crops.euler2mat(0.08, -0.05, 0.02), rng.normal(size=3) * 3, rng.uniform(-0.03, 0.03, 3))):
        row = dcl.ops.pose_rows([R0], [t], [jit], [A])[0]
        got, R1, t1 = dcl.ops.crop_repose_host(p, row, cen)
        want, wR1, wt1 = numpy_repose(p, R0, A, t, jit, cen)
        assert np.array_equal(got, want) and np.array_equal(R1, wR1) and np.array_equal(t1, wt1)
    row = dcl.ops.pose_rows([eye], [cen.astype(np.float64)], [np.zeros(3)], [eye])[0]
    assert np.array_equal(dcl.ops.crop_repose_host(p, row, cen)[0], p)        # t0 = 0, R = I: the identity, exactly


ROT_BOUND = 8.0 * TS.U      # times sum_m |R0[i][m]| |A[m][k]|: two evaluations of a 3-term dot product (repose_bound, `R1 = R0 A`)


@pytest.mark.parametrize("seed,kw", [(s, k) for s, k in POSED if not k.get("far")])
def test_repose_host_lies_within_the_derived_bound_of_the_reference(dcl, golden, seed, kw):
    """The reference's `@` products go through a BLAS whose summation order and use of fused multiply-adds are unspecified: its
    coordinates are not bit-comparable.  Colours, trans_gt, the in-grid count and the chosen rows are; rot_gt = R0 @ A was
    measured by the generator to differ from the left-to-right product in the last bit (fixture: rot_exact = 0), so it is
    held to the same kind of bound as the coordinates."""
    tag = "t%d_" % seed
    _, cloud, centroid, colours, row, P, A, jit = scene_pose(dcl, golden, seed, kw)
    posed, R1, t1 = dcl.ops.crop_repose_host(cloud, row, centroid)
    half = TS.CFG["unit_voxel_extent"][0] * TS.CFG["voxel_num_limit"][0] * 0.5
    inside = (np.abs(posed) < np.float32(half)).all(1)
    assert int(inside.sum()) == int(golden[tag + "m"])
    choice = golden[tag + "choice"]
    t0 = (P[:, 3] - centroid.astype(np.float64)).astype(np.float32)
    bound, _ = TS.repose_bound(cloud, P[:, 0:3].astype(np.float32), A.astype(np.float32), t0, t1)
    ref = golden[tag + "feat_inp"]
    err = np.abs(posed[inside][choice].astype(np.float64) - ref[:, 4:7])
    ratio = float((err / bound[inside][choice]).max())
    print("scene %d: worst |host twin - reference| / bound = %.3f (generator: %.3f over all scenes)" % (seed, ratio, float(golden["worst_ratio"])))
    assert (err <= bound[inside][choice]).all()
    assert np.array_equal(ref[:, 1:4], colours[inside][choice]) and (ref[:, 0] == 1).all()
    assert np.array_equal(golden[tag + "trans_gt"], t1)
    if int(golden["rot_exact"]):
        assert np.array_equal(golden[tag + "rot_gt"], R1)
    else:
        SR = np.abs(P[:, 0:3].astype(np.float32).astype(np.float64)) @ np.abs(A.astype(np.float32).astype(np.float64))
        assert (np.abs(golden[tag + "rot_gt"].astype(np.float64) - R1) <= ROT_BOUND * SR).all()
    assert float(golden["worst_ratio"]) <= 0.5


@pytest.mark.parametrize("seed,kw", [(s, k) for s, k, _ in TS.CASES])
def test_default_draw_consumes_both_generators_as_the_loader_did(dcl, golden, seed, kw):
    tag = "t%d_" % seed
    np.random.seed(seed)
    random.seed(seed)
    draw = dcl.crops.LoaderDraw()
    k = 1 if (kw.get("tall") or kw.get("small") or kw.get("border")) else 4
    assert [draw.pick(k) for _ in golden[tag + "picks"]] == golden[tag + "picks"].tolist()
    if len(golden[tag + "angles"]):
        assert draw.angles() == golden[tag + "angles"].tolist()
        assert draw.jitter() == golden[tag + "jitter"].tolist()
    if tag + "choice" in golden.files:
        got = draw.choice(int(golden[tag + "m"]), TS.CFG["input_size"])
        assert np.array_equal(got, golden[tag + "choice"])
    # ... and nothing more: the next numbers of both streams are the ones a fresh replay gives
    nxt = (np.random.random_sample(), random.random())
    np.random.seed(seed)
    random.seed(seed)
    for _ in golden[tag + "picks"]:
        np.random.randint(0, k)
    for _ in golden[tag + "angles"]:
        np.random.uniform(-1, 1)
        random.uniform(-1, 1)
    if tag + "choice" in golden.files:
        m = int(golden[tag + "m"])
        np.random.choice(m, TS.CFG["input_size"], replace=m <= TS.CFG["input_size"])
    assert nxt == (np.random.random_sample(), random.random())


def test_scenes_are_what_they_claim(golden):
    """the fixture's own record of the cases: a repeated pick, both dummies, a with-replacement choice, both cameras, a box on
    the border"""
    assert len(golden["t53_picks"]) > 1
    assert float(golden["t54_flag"]) == -1 and len(golden["t54_angles"]) == 0
    assert float(golden["t55_flag"]) == -1 and len(golden["t55_angles"]) == 3
    assert int(golden["t56_m"]) <= TS.CFG["input_size"] and len(np.unique(golden["t56_choice"])) < TS.CFG["input_size"]
    assert golden["t57_box"][0] == 0 and golden["t57_box"][2] == 0
    assert TS.CASES[1][1]["camera"] == 2
