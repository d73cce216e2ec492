"""ops.mask_box (csrc/mask_box.hip: the loaders' get_bbox(mask_to_bbox(mask)) on the device) against its host twin
dcl_mask_box_host on the smallest masks on which a run-labelling kernel goes wrong (tests/mask_cases.py), at the loaders'
480 x 640 and at 37 x 70; all ten integers -- the component count and the winner's pixel count show a wrong merge that
leaves the largest box unchanged.  The twin itself is pinned against scipy's labelling in tests/test_mask_box_abi.py."""
import numpy as np
import pytest
import torch

import mask_cases as MC
from lmo_scene import CASES as LMO_CASES, make_lmo_scene

pytestmark = pytest.mark.gpu

_CACHE = {}


def cases(H, W):
    """[(name, int32 (H,W) label image)] with the twin's answer for padding 0, computed once"""
    if (H, W) not in _CACHE:
        masks = MC.mask_cases(H, W)
        if (H, W) == (480, 640):
            masks += [("lmo scene %d" % seed, make_lmo_scene(seed, **kw)["mask_label"]) for seed, kw in LMO_CASES]
        _CACHE[(H, W)] = [(name, np.ascontiguousarray(m.astype(np.int32))) for name, m in masks]
    return _CACHE[(H, W)]


@pytest.mark.parametrize("H,W", MC.SIZES)
def test_kernel_equals_the_host_twin_one_mask_per_call(dcl, H, W):
    for name, lab in cases(H, W):
        want = dcl.ops.mask_box_host(lab, 1, 0)
        got = dcl.ops.mask_box(torch.from_numpy(lab).cuda(), 1, 0).cpu().numpy()
        assert np.array_equal(got, want), (name, got.tolist(), want.tolist())


@pytest.mark.parametrize("H,W", MC.SIZES)
@pytest.mark.parametrize("padding", [0, 4, 5])
def test_kernel_equals_the_host_twin_three_different_masks_per_call(dcl, H, W, padding):
    cs = cases(H, W)
    for i in range(0, len(cs), 3):
        trio = [cs[(i + j) % len(cs)] for j in range(3)]
        lab = np.stack([l for _, l in trio])
        want = dcl.ops.mask_box_host(lab, 1, padding)
        got = dcl.ops.mask_box(torch.from_numpy(lab).cuda(), 1, padding).cpu().numpy()
        assert np.array_equal(got, want), ([n for n, _ in trio], got.tolist(), want.tolist())


def test_value_selects_one_id_of_three(dcl):
    rng = np.random.default_rng(5)
    lab = rng.integers(0, 4, (37, 70)).astype(np.int32)                     # ids 1, 2, 3 on background 0
    lab[10:20, 30:50] = 2
    dev = torch.from_numpy(lab).cuda()
    for value in (1, 2, 3):
        want = dcl.ops.mask_box_host(lab, value, 0)
        assert np.array_equal(want, dcl.ops.mask_box_host((lab == value).astype(np.int32), 1, 0))
        assert np.array_equal(dcl.ops.mask_box(dev, value, 0).cpu().numpy(), want), value


def test_equal_area_tie_takes_the_component_found_last(dcl):
    """the stated rule (csrc/mask_box.h: mb_better), not cv2: it is not pinned against cv2"""
    lab = dict(cases(480, 640))["tie"]
    got = dcl.ops.mask_box(torch.from_numpy(lab).cuda(), 1, 0).cpu().numpy()[0]
    assert got[:4].tolist() == [40, 20, 6, 10] and got[8] == 3 and got[9] == 60
    assert np.array_equal(got, dcl.ops.mask_box_host(lab, 1, 0)[0])


def test_two_calls_give_the_same_bits(dcl):
    for name in ("checkerboard", "bernoulli 0.41 seed 1", "spiral"):
        dev = torch.from_numpy(dict(cases(480, 640))[name]).cuda()
        a = dcl.ops.mask_box(dev, 1, 0)
        b = dcl.ops.mask_box(dev, 1, 0)
        assert torch.equal(a, b), name


def test_captured_call_replays_to_the_same_result(dcl):
    import ctypes as C
    N = dcl._native
    cs = dict(cases(480, 640))
    lab = torch.from_numpy(np.stack([cs["bernoulli 0.41 seed 2"], cs["lmo scene 41"]])).cuda()
    want = dcl.ops.mask_box(lab, 1, 4)
    n, H, W = lab.shape
    nb = C.c_int64(0)
    N.check(N.lib().dcl_mask_box_ws_bytes(n, H, W, C.byref(nb)))
    ws = torch.empty(nb.value // 4, dtype=torch.int32, device="cuda")
    out = torch.zeros((n, 10), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        N.check(N.lib().dcl_mask_box(N.ptr(lab), n, H, W, 1, 4, N.ptr(out), N.ptr(ws), C.c_int64(nb.value), N.stream()))
    for _ in range(2):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want)
    lab.copy_(torch.from_numpy(np.stack([cs["stripes"], cs["ring"]])).cuda())   # new contents, the same captured launches
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, dcl.ops.mask_box(lab, 1, 4))
