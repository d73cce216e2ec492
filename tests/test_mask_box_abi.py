"""The mask-to-box entry points (dcl_mask_box, its size query and its host twin; csrc/mask_box.hip, csrc/mask_box.h) are
declared with the agreed argument lists, exported by both libraries, refuse bad arguments and treat n == 0 as a no-op
without a GPU; and the host twin -- what the GPU tests compare the kernels with -- gives the ten integers of an independent
restatement (scipy.ndimage.label with a 3 x 3 structure + find_objects + the selection and tie rule + crops.lm_box + the
clamp, tests/mask_cases.py) on every mask of the list, at both sizes, for padding 0, 4 and 5."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mask_cases as MC
from lmo_scene import CASES as LMO_CASES, make_lmo_scene
from test_pointnet_grad_abi import _libs, declarations

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WANT = {
    "dcl_mask_box_ws_bytes": ["int n", "int H", "int W", "int64_t *bytes_host"],
    "dcl_mask_box": ["const int32_t *label", "int n", "int H", "int W", "int32_t value", "int padding", "int32_t *out",
                     "void *ws", "int64_t ws_bytes", "dclStream_t stream"],
    "dcl_mask_box_host": ["const int32_t *label", "int n", "int H", "int W", "int32_t value", "int padding", "int32_t *out"],
}


def test_header_declares_the_entry_points_outside_the_diagnostic_block():
    decl = declarations()
    for name, args in WANT.items():
        assert name in decl, name
        assert decl[name] == args, (name, decl[name])
    text = open(os.path.join(ROOT, "include", "dclnet_hip.h")).read()
    assert re.search(r"#define DCL_ABI_VERSION 2\b", text)
    diag = text[text.index("#ifdef DCL_DIAG"):text.index("#endif /* DCL_DIAG */")]
    assert "dcl_mask_box" not in diag and "dcl_debug_mask" not in text


def test_both_libraries_export_them_and_the_abi_version_stays(dcl):
    assert os.path.exists(dcl._native.DIAG_SO_PATH), "diagnostic library missing: build() makes it"
    for tag, lib in _libs(dcl):
        for name in WANT:
            assert hasattr(lib, name), (tag, name)
        assert lib.dcl_abi_version() == 2, tag
    assert callable(dcl.ops.mask_box) and callable(dcl.ops.mask_box_host)


def test_workspace_covers_the_worst_mask_and_needs_no_gpu(dcl):
    for tag, lib in _libs(dcl):
        nb = C.c_int64(-7)
        assert lib.dcl_mask_box_ws_bytes(1, 480, 640, C.byref(nb)) == 0, tag
        # 153 600 runs (every other pixel of every row), at least start / end / label of each; no table per pixel pair
        assert 12 * 153600 <= nb.value <= 64 * 153600, (tag, nb.value)
        n3 = C.c_int64(-7)
        assert lib.dcl_mask_box_ws_bytes(3, 480, 640, C.byref(n3)) == 0 and n3.value == 3 * nb.value, tag
        z = C.c_int64(-7)
        assert lib.dcl_mask_box_ws_bytes(0, 480, 640, C.byref(z)) == 0 and z.value == 0, tag


FAKE = C.c_void_p(4096)          # a non-null address that a call refusing its arguments never touches
BIG = C.c_int64(1 << 40)


def _dev(L, label, n, H, W, padding, out, ws, ws_bytes):
    return L.dcl_mask_box(label, n, H, W, 1, padding, out, ws, ws_bytes, None)


@pytest.mark.parametrize("call", [
    lambda L, nb: L.dcl_mask_box_ws_bytes(-1, 480, 640, C.byref(nb)),
    lambda L, nb: L.dcl_mask_box_ws_bytes(1, 0, 640, C.byref(nb)),
    lambda L, nb: L.dcl_mask_box_ws_bytes(1, 480, 0, C.byref(nb)),
    lambda L, nb: L.dcl_mask_box_ws_bytes(1, 480, -640, C.byref(nb)),
    lambda L, nb: L.dcl_mask_box_ws_bytes(1, 65536, 32768, C.byref(nb)),          # H * W = 2^31
    lambda L, nb: L.dcl_mask_box_ws_bytes(1, 480, 640, None),
    lambda L, nb: _dev(L, FAKE, -1, 480, 640, 0, FAKE, FAKE, BIG),
    lambda L, nb: _dev(L, FAKE, 1, 0, 640, 0, FAKE, FAKE, BIG),
    lambda L, nb: _dev(L, FAKE, 1, 480, 0, 0, FAKE, FAKE, BIG),
    lambda L, nb: _dev(L, FAKE, 1, 65536, 32768, 0, FAKE, FAKE, BIG),
    lambda L, nb: _dev(L, FAKE, 1, 480, 640, -1, FAKE, FAKE, BIG),                # padding < 0
    lambda L, nb: _dev(L, None, 1, 480, 640, 0, FAKE, FAKE, BIG),                 # a null pointer, each in turn
    lambda L, nb: _dev(L, FAKE, 1, 480, 640, 0, None, FAKE, BIG),
    lambda L, nb: _dev(L, FAKE, 1, 480, 640, 0, FAKE, None, BIG),
    lambda L, nb: _dev(L, FAKE, 1, 480, 640, 0, FAKE, FAKE, C.c_int64(4096)),     # short workspace
    lambda L, nb: L.dcl_mask_box_host(None, 1, 480, 640, 1, 0, FAKE),
    lambda L, nb: L.dcl_mask_box_host(FAKE, 1, 480, 640, 1, 0, None),
    lambda L, nb: L.dcl_mask_box_host(FAKE, 1, 480, 640, 1, -1, FAKE),
    lambda L, nb: L.dcl_mask_box_host(FAKE, 1, 0, 640, 1, 0, FAKE),
    lambda L, nb: L.dcl_mask_box_host(FAKE, -1, 480, 640, 1, 0, FAKE),
])
def test_bad_arguments_return_einval_without_a_gpu(dcl, call):
    for tag, lib in _libs(dcl):
        lib.dcl_last_error.restype = C.c_char_p
        nb = C.c_int64(0)
        assert call(lib, nb) == -1, tag
        assert b"invalid argument" in lib.dcl_last_error(), tag


def test_short_workspace_is_measured_against_the_size_query(dcl):
    for tag, lib in _libs(dcl):
        nb = C.c_int64(0)
        assert lib.dcl_mask_box_ws_bytes(2, 37, 70, C.byref(nb)) == 0
        assert _dev(lib, FAKE, 2, 37, 70, 0, FAKE, FAKE, C.c_int64(nb.value - 1)) == -1, tag


def test_no_image_is_a_no_op_without_a_gpu(dcl):
    for tag, lib in _libs(dcl):
        assert _dev(lib, None, 0, 480, 640, 0, None, None, C.c_int64(0)) == 0, tag
        assert lib.dcl_mask_box_host(None, 0, 480, 640, 1, 0, None) == 0, tag
    assert dcl.ops.mask_box_host(np.zeros((0, 37, 70), np.int32)).shape == (0, 10)


@pytest.mark.parametrize("H,W", MC.SIZES)
def test_host_twin_equals_the_scipy_restatement(dcl, H, W):
    masks = MC.mask_cases(H, W)
    if (H, W) == (480, 640):
        masks += [("lmo scene %d" % seed, make_lmo_scene(seed, **kw)["mask_label"]) for seed, kw in LMO_CASES]
    for name, m in masks:
        won = MC.winner(m)
        for padding in (0, 4, 5):
            want = MC.restate(m, padding, dcl.crops.lm_box, won)
            got = dcl.ops.mask_box_host(m.astype(np.int32), 1, padding)[0]
            assert np.array_equal(got, want), (name, padding, got.tolist(), want.tolist())


def test_host_twin_handles_several_images_and_selects_one_id_of_three(dcl):
    rng = np.random.default_rng(5)
    lab = rng.integers(0, 4, (3, 37, 70)).astype(np.int32)                  # ids 1, 2, 3 on background 0
    lab[1, 10:20, 30:50] = 2
    for value in (1, 2, 3):
        got = dcl.ops.mask_box_host(lab, value, 4)
        for i in range(3):
            assert np.array_equal(got[i], MC.restate(lab[i] == value, 4, dcl.crops.lm_box)), (value, i)


def test_lmo_scene_masks_are_occluded_the_way_the_fixture_needs(dcl):
    """every non-empty scene mask: at least three pieces and a unique largest rectangle (no tie: the fixture does not
    depend on the unpinned rule); one scene's winner rests on the image border"""
    from scipy import ndimage
    on_border = 0
    for seed, kw in LMO_CASES:
        m = make_lmo_scene(seed, **kw)["mask_label"]
        if not m.any():
            assert kw.get("empty")
            continue
        lab, ncomp = ndimage.label(m, structure=np.ones((3, 3), int))
        areas = sorted((s[0].stop - s[0].start) * (s[1].stop - s[1].start) for s in ndimage.find_objects(lab))
        assert ncomp >= 3 and areas[-1] > areas[-2], (seed, ncomp, areas[-3:])
        on_border += int(dcl.ops.mask_box_host(m, 1, 0)[0][0] == 0)
    assert on_border == 1
