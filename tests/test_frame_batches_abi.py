"""The library entries behind the multi-frame eval builders on their HOST twins, no GPU: the keyed draw
(include/dclnet_hip.h: dcl_crop_draw_keyed) against the plain draw it is defined by, the refusals that come before any device
work, and the third state of `valid` -- a row with valid < 0 is not a crop and updates nothing of any table."""
import ctypes as C

import numpy as np
import pytest
import torch

import metric_table_cases as MT

NPOINT = 64
MS = (0, 1, NPOINT, NPOINT + 1, 5000)


# ---------------------------------------------------------------------------------------------- a. the keyed draw
def test_the_new_symbols_exist(dcl):
    lib = dcl._native.lib()
    for name in ("dcl_crop_points_frames", "dcl_crop_draw_keyed", "dcl_crop_draw_keyed_host"):
        assert hasattr(lib, name), name
    assert int(lib.dcl_abi_version()) == 2                      # additions only
    for name in ("crop_points_frames", "crop_draw_keyed", "crop_draw_keyed_host"):
        assert callable(getattr(dcl.ops, name)), name


@pytest.mark.parametrize("keep_sparse", [True, False])
def test_keyed_rows_equal_the_plain_draws_rows(dcl, keep_sparse):
    """row i of the keyed draw == row keys[i][1] of crop_draw_host(frame = keys[i][0]) on the same counts row: every m in MS (both
    streams: m > npoint draws without, 0 < m <= npoint with replacement), empty and sparse rows, scrambled (frame, inst) keys"""
    rng = np.random.default_rng(5)
    counts, keys = [], []
    for m in MS:
        for inside in (m, min(m, 20)):                         # a sparse row (at most 32 points inside the grid) of every m
            counts.append((m, inside, m))
    counts.append((40, 40, 0))                                 # masked pixels but no written row: never valid
    counts = np.asarray(counts, np.int32)
    n = len(counts)
    frames = [0, 7, 3, (1 << 40) + 11, 2]
    for i in range(n):
        keys.append((frames[int(rng.integers(0, len(frames)))], int(rng.integers(0, 9))))
    keys = np.asarray(keys, np.uint64)
    idx, valid = dcl.ops.crop_draw_keyed_host(counts, NPOINT, 0xFEDCBA9876543210, keys, min_valid=32, keep_sparse=keep_sparse)
    assert idx.shape == (n, NPOINT) and idx.dtype == np.int64 and valid.dtype == np.int32
    seen_valid = set()
    for i in range(n):
        frame, inst = int(keys[i, 0]), int(keys[i, 1])
        plain = np.zeros((inst + 1, 3), np.int32)
        plain[inst] = counts[i]
        want, want_valid = dcl.ops.crop_draw_host(plain, NPOINT, 0xFEDCBA9876543210, frame, min_valid=32, keep_sparse=keep_sparse)
        assert valid[i] == want_valid[inst], i
        assert np.array_equal(idx[i], want[inst]), i
        seen_valid.add(int(valid[i]))
        if not valid[i]:
            assert not idx[i].any()
    assert seen_valid == {0, 1}
    # the same key on the same counts row gives the same row wherever it stands; another key another row
    again, _ = dcl.ops.crop_draw_keyed_host(counts[::-1].copy(), NPOINT, 0xFEDCBA9876543210, keys[::-1].copy(), keep_sparse=keep_sparse)
    assert np.array_equal(again[::-1], idx)
    big = MS.index(5000) * 2
    other = keys.copy()
    other[big, 1] += np.uint64(1)
    moved, _ = dcl.ops.crop_draw_keyed_host(counts, NPOINT, 0xFEDCBA9876543210, other, keep_sparse=keep_sparse)
    assert not np.array_equal(moved[big], idx[big]) and np.array_equal(np.delete(moved, big, 0), np.delete(idx, big, 0))


def test_pinned_constants_hold_through_the_keyed_twin(dcl):
    """base(2,7,3,1) = 0x9fb95fa8ca6188d9 with keys 0xc1bed6510d07ff6c, 0x3c33370239554870 (the header): m = 5 <= npoint draws
    floor(key(j) * 5 / 2^64) on stream 1 -- through the key (frame 7, inst 3) on ROW 0"""
    idx, valid = dcl.ops.crop_draw_keyed_host([[5, 5, 5]], 8, 2, [[7, 3]])
    assert valid.tolist() == [1]
    assert idx[0, :2].tolist() == [(0xc1bed6510d07ff6c * 5) >> 64, (0x3c33370239554870 * 5) >> 64]
    assert idx[0].tolist() == [3, 1, 1, 1, 2, 3, 2, 1]          # tests/test_crop_draw_abi.py pins this row for crop_draw_host
    idx, _ = dcl.ops.crop_draw_keyed_host([[307200] * 3], 1024, 1, [[0, 0]])
    assert idx[0, :6].tolist() == [266847, 173930, 218072, 272930, 4592, 91144]       # base(1,0,0,0), without replacement


# ---------------------------------------------------------------------------------------------- b. refusals, before any GPU call
def test_bad_arguments_return_einval_without_touching_the_gpu(dcl):
    lib = dcl._native.lib()
    EINVAL = -1
    one = (C.c_int32 * 3)(5, 5, 5)
    key = (C.c_uint64 * 2)(7, 0)
    idx = (C.c_int64 * 4096)()
    val = (C.c_int32 * 1)()
    u = C.c_uint64(0)
    p, pk, null = C.cast(one, C.c_void_p), C.cast(key, C.c_void_p), C.c_void_p(0)
    pi, pv = C.cast(idx, C.c_void_p), C.cast(val, C.c_void_p)
    for fn, tail in ((lib.dcl_crop_draw_keyed, (null,)), (lib.dcl_crop_draw_keyed_host, ())):
        for npoint in (0, -3, 4097, 1 << 20):
            assert fn(1, npoint, p, 32, 1, u, pk, pi, pv, *tail) == EINVAL, (fn, npoint)
        assert fn(-1, 8, p, 32, 1, u, pk, pi, pv, *tail) == EINVAL
        for args in ((null, pk, pi, pv), (p, null, pi, pv), (p, pk, null, pv), (p, pk, pi, null)):
            assert fn(1, 8, args[0], 32, 1, u, args[1], args[2], args[3], *tail) == EINVAL
        assert fn(0, 8, null, 32, 1, u, null, null, null, *tail) == 0                       # an empty call
    assert b"invalid argument" in lib.dcl_last_error()
    # dcl_crop_points_frames: shapes, null pointers and the HOST frame indices are refused before any device work (the pointers
    # below are host memory no kernel may ever see)
    buf = (C.c_float * 64)()
    pf = C.cast(buf, C.c_void_p)
    cam = (C.c_float * 6)(320, 240, 1000, 1000, 10000, 1)
    mean = (C.c_double * 3)(0.485, 0.456, 0.406)
    he = (C.c_float * 3)(0.192, 0.192, 0.192)

    def call(n_frames=2, H=4, W=4, ch=3, n=1, fidx=(0,), depth=pf, src=pf, cam_=cam, cap=16, out=pf, ws=pf):
        f = (C.c_int32 * max(len(fidx), 1))(*fidx)
        return lib.dcl_crop_points_frames(depth, pf, pf, n_frames, H, W, ch, n, f, src, cam_, mean, he, 32, 0, cap, pf, pf, out, pf, pf,
                                          pf, ws, null)
    for bad in (dict(fidx=(2,)), dict(fidx=(-1,)), dict(n=2, fidx=(0, 5)), dict(n_frames=0), dict(H=0), dict(W=-1), dict(ch=2),
                dict(cap=0), dict(cap=1024 * 4096 + 1), dict(n=-1), dict(depth=null), dict(src=null), dict(out=null), dict(ws=null),
                dict(cam_=(C.c_float * 6)(320, 240, 1000, 1000, 0, 1))):
        assert call(**bad) == EINVAL, bad
    assert lib.dcl_crop_points_frames(null, null, null, 0, 4, 4, 3, 0, null, null, null, null, null, 32, 0, 16, null, null, null, null,
                                      null, null, null, null) == 0                           # an empty call
    with pytest.raises(RuntimeError, match="invalid argument"):
        dcl.ops.crop_draw_keyed_host([[5, 5, 5]], 4097, 0, [[0, 0]])
    with pytest.raises(RuntimeError, match="invalid argument"):
        dcl.ops.crop_draw_keyed_host([[5, 5, 5]], 8, 0, None)


# ---------------------------------------------------------------------------------------------- c. valid < 0 is not a crop
def _with_padding(case, seed):
    """the case with rows of valid = -1 inserted at random places: NaN / tiny distances and class ids in and OUT of range"""
    rng = np.random.default_rng(seed)
    b, T, C = case["b"], case["T"], case["C"]
    n_pad = 1 + b // 2
    where = np.sort(rng.integers(0, b + 1, n_pad))
    cls = np.insert(case["cls"], where, np.resize(np.array([0, -1, C, C - 1, 1 << 30, -(1 << 31)], np.int64), n_pad).astype(np.int32))
    dis = np.insert(case["dis"], where, np.resize(np.array([np.nan, 0.0, 0.01, np.inf], np.float32), n_pad), axis=1)
    valid = np.ones(b, np.int32) if case["valid"] is None else case["valid"]
    valid = np.insert(valid, where, np.resize(np.array([-1, -7, -(1 << 31)], np.int64), n_pad).astype(np.int32))
    return dict(case, b=b + n_pad, cls=cls.astype(np.int32), dis=np.ascontiguousarray(dis, np.float32), valid=valid.astype(np.int32))


def test_host_twin_updates_nothing_for_padding_rows(dcl):
    cases = MT.edge_cases()
    assert len(cases) > 100
    for k, case in enumerate(cases):
        padded = _with_padding(case, k)
        assert (padded["valid"] < 0).any()
        got, want = MT.new_arrays(dcl, padded), MT.new_arrays(dcl, case)
        for arrays, c in ((got, padded), (want, case)):
            dis, cls, valid, diam = MT.tensors(c)
            for _ in range(2):                                   # twice: the second call adds to what the first left
                dcl.ops.metric_tabulate_host(arrays, dis, cls, valid, mode=c["mode"], diameter=diam)
        for name in ("sums", "maxd", "counts", "bad"):
            if want[name] is not None:
                assert MT.bits(got[name]) == MT.bits(want[name]), (case["name"], name)
        MT.assert_equals_expected(want, _twice(dcl, case), case["mode"], case["name"])


def _twice(dcl, case):
    """the host classes fed the case's crops twice (per step), as two calls on one table do"""
    double = dict(case, b=2 * case["b"], cls=np.concatenate([case["cls"]] * 2), dis=np.concatenate([case["dis"]] * 2, 1),
                  valid=None if case["valid"] is None else np.concatenate([case["valid"]] * 2))
    return MT.expected(dcl, double)


def test_only_padding_leaves_the_table_and_bad_untouched(dcl):
    for mode in MT.MODES:
        case = dict(mode=mode, T=2, C=5, b=4)
        arrays = dcl.ops.metric_table_arrays(mode, 2, 5, "cpu")
        before = {k: v.clone() for k, v in arrays.items() if v is not None}
        dis = torch.tensor([[0.01, float("nan"), 0.0, 1.0]] * 2)
        cls = torch.tensor([0, 99, -3, 4], dtype=torch.int32)
        dcl.ops.metric_tabulate_host(arrays, dis, cls, torch.full((4,), -1, dtype=torch.int32), mode=mode,
                                     diameter=torch.from_numpy(MT.diameters(5)))
        for k, v in before.items():
            assert torch.equal(arrays[k], v), (case, k)
        assert int(arrays["bad"][0]) == 0
        # the same rows as real crops DO raise bad: the rule is about valid, not about these inputs
        dcl.ops.metric_tabulate_host(arrays, dis, cls, torch.ones(4, dtype=torch.int32), mode=mode,
                                     diameter=torch.from_numpy(MT.diameters(5)))
        assert int(arrays["bad"][0]) == 1
