"""The device draw of the crop builders (include/dclnet_hip.h: dcl_crop_draw) on its HOST twin, no GPU: the values the
definition pins, the refusals that come before any device work, the structure of a draw against a numpy draft of the same
definition, and its uniformity over frames."""
import ctypes as C

import numpy as np
import pytest

U64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15


# ---- a numpy / Python draft of the definition, written from the header's text alone
def mix(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & U64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & U64
    return z ^ (z >> 31)


def base_of(seed, frame, inst, s):
    return mix(mix(mix((seed + G) & U64) ^ ((frame + G) & U64)) ^ ((2 * inst + s + G) & U64))


def keys_of(base, n):
    with np.errstate(over="ignore"):
        z = np.uint64(base) + (np.arange(n, dtype=np.uint64) + np.uint64(1)) * np.uint64(G)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def draft(seed, frame, inst, m, npoint):
    if m > npoint:
        return np.argsort(keys_of(base_of(seed, frame, inst, 0), m), kind="stable")[:npoint].astype(np.int64)
    return np.array([(int(k) * m) >> 64 for k in keys_of(base_of(seed, frame, inst, 1), npoint)], np.int64)


def counts_with(inst, m):
    """a counts array whose row `inst` holds an instance of m rows; the rows in front of it are empty"""
    c = np.zeros((inst + 1, 3), np.int32)
    c[inst] = m
    return c


def draw(dcl, seed, frame, inst, m, npoint, **kw):
    idx, valid = dcl.ops.crop_draw_host(counts_with(inst, m), npoint, seed, frame, **kw)
    assert valid.tolist() == [0] * inst + [1 if m > 0 else 0] and not idx[:inst].any()
    return idx[inst]


# ---------------------------------------------------------------------------------------------- 1. pinned values
def test_generator_matches_the_pinned_values(dcl):
    b, k = dcl.ops.crop_draw_keys_host(1, 0, 0, 0, 2)
    assert b == 0x6df1421574b0d586 and [int(v) for v in k] == [0x96c9f513020798b9, 0xf7dd055ed9ec356f]
    b, k = dcl.ops.crop_draw_keys_host(2, 7, 3, 1, 2)
    assert b == 0x9fb95fa8ca6188d9 and [int(v) for v in k] == [0xc1bed6510d07ff6c, 0x3c33370239554870]
    assert base_of(1, 0, 0, 0) == 0x6df1421574b0d586 and base_of(2, 7, 3, 1) == 0x9fb95fa8ca6188d9      # the draft agrees
    assert [int(v) for v in keys_of(base_of(2, 7, 3, 1), 2)] == [0xc1bed6510d07ff6c, 0x3c33370239554870]


def test_draws_match_the_pinned_values(dcl):
    d = draw(dcl, 1, 0, 0, 307200, 1024)
    assert d[:6].tolist() == [266847, 173930, 218072, 272930, 4592, 91144] and d[-2:].tolist() == [248214, 67511]
    assert draw(dcl, 2, 7, 3, 1025, 1024)[:6].tolist() == [209, 361, 468, 27, 418, 796]
    assert draw(dcl, 2, 7, 3, 5, 8).tolist() == [3, 1, 1, 1, 2, 3, 2, 1]


# ---------------------------------------------------------------------------------------------- 2. refusals, before any GPU call
def test_bad_arguments_return_einval_without_touching_the_gpu(dcl):
    lib = dcl._native.lib()
    EINVAL = -1
    one = (C.c_int32 * 3)(5, 5, 5)
    idx = (C.c_int64 * 4096)()
    val = (C.c_int32 * 1)()
    u = C.c_uint64(0)
    p, null = C.cast(one, C.c_void_p), C.c_void_p(0)
    pi, pv = C.cast(idx, C.c_void_p), C.cast(val, C.c_void_p)
    for fn, tail in ((lib.dcl_crop_draw, (null,)), (lib.dcl_crop_draw_host, ())):
        for npoint in (0, -3, 4097, 1 << 20):
            assert fn(1, npoint, p, 32, 1, u, u, pi, pv, *tail) == EINVAL, (fn, npoint)
        assert fn(-1, 8, p, 32, 1, u, u, pi, pv, *tail) == EINVAL
        for args in ((null, pi, pv), (p, null, pv), (p, pi, null)):
            assert fn(1, 8, args[0], 32, 1, u, u, args[1], args[2], *tail) == EINVAL
        assert fn(0, 8, null, 32, 1, u, u, null, null, *tail) == 0                              # an empty call
    assert b"invalid argument" in lib.dcl_last_error()
    f = (C.c_float * 64)()
    unit = (C.c_float * 3)(0.006, 0.006, 0.006)
    pf, pu = C.cast(f, C.c_void_p), C.cast(unit, C.c_void_p)
    half = C.c_float(0.192)
    for fn, tail in ((lib.dcl_crop_sample_valid, (null,)), (lib.dcl_crop_sample_valid_host, ())):
        def call(n=1, npoint=8, cap=4, xyz=pf, rgb=pf, si=pi, valid=pv, unit_=pu, S=64, feats=pf, coords=pi):
            return fn(n, npoint, cap, xyz, rgb, si, null, 32, valid, half, unit_, S, feats, coords, *tail)
        for bad in (dict(npoint=0), dict(npoint=4097), dict(npoint=9, S=2), dict(npoint=28, S=3), dict(n=-1), dict(cap=0),
                    dict(cap=-4), dict(S=0), dict(xyz=null), dict(rgb=null), dict(si=null), dict(valid=null), dict(unit_=null),
                    dict(feats=null), dict(coords=null)):
            assert call(**bad) == EINVAL, (fn, bad)
        assert call(n=0, xyz=null, rgb=null, si=null, valid=null, feats=null, coords=null) == 0
    assert dcl.ops.CROP_DRAW_MAX_POINTS == 4096
    with pytest.raises(RuntimeError, match="invalid argument"):
        dcl.ops.crop_draw_host(counts_with(0, 10), 4097, 0, 0)


def test_builder_refuses_an_unknown_draws_value(dcl):
    cfg = dict(input_size=1024, tmp_size=8, unit_voxel_extent=[0.006] * 3, voxel_num_limit=[64] * 3, voxelization_mode=4)
    for bad in ("x", None, "Device", 1):
        with pytest.raises(ValueError, match="draws"):
            dcl.crops.CropBuilder(cfg, {}, {}, draws=bad)
    with pytest.raises(ValueError, match="input_size"):                  # past DCL_CROP_DRAW_MAX_POINTS: before any device work
        dcl.crops.CropBuilder(dict(cfg, input_size=4097), {}, {}, draws="device")


# ---------------------------------------------------------------------------------------------- 3. structure
@pytest.mark.parametrize("m,npoint", [(2, 1), (17, 16), (35, 16), (2051, 1024), (4097, 4096), (70001, 1000)])
def test_without_replacement_is_the_head_of_the_stable_argsort_of_the_keys(dcl, m, npoint):
    for seed, frame, inst in ((1, 0, 0), (9, 1 << 40, 2)):
        d = draw(dcl, seed, frame, inst, m, npoint)
        assert len(set(d.tolist())) == npoint and d.min() >= 0 and d.max() < m
        assert np.array_equal(d, draft(seed, frame, inst, m, npoint))


@pytest.mark.parametrize("m,npoint", [(1, 1), (1, 16), (5, 8), (15, 16), (16, 16), (1024, 1024), (100, 4096)])
def test_with_replacement_is_the_high_half_of_key_times_m(dcl, m, npoint):
    for seed, frame, inst in ((1, 0, 0), (9, 1 << 40, 2)):
        d = draw(dcl, seed, frame, inst, m, npoint)
        assert d.min() >= 0 and d.max() < m
        assert np.array_equal(d, draft(seed, frame, inst, m, npoint))


def test_instances_without_a_crop_get_zeros_and_valid_0(dcl):
    #            empty mask   sparse (valid <= 32)  good           sparse, a large one
    counts = [[0, 0, 0], [40, 20, 40], [5000, 4000, 4000], [3000, 32, 3000]]
    idx, valid = dcl.ops.crop_draw_host(counts, 16, 3, 5, min_valid=32, keep_sparse=False)
    assert valid.tolist() == [0, 0, 1, 0] and not idx[[0, 1, 3]].any() and idx[2].any()
    idx2, valid2 = dcl.ops.crop_draw_host(counts, 16, 3, 5, min_valid=32, keep_sparse=True)       # the YCB-V loader keeps them
    assert valid2.tolist() == [0, 1, 1, 1] and not idx2[0].any() and np.array_equal(idx2[2], idx[2])
    assert np.array_equal(idx2[1], draft(3, 5, 1, 40, 16)) and np.array_equal(idx2[3], draft(3, 5, 3, 3000, 16))
    # a row is a function of its own (seed, frame, row index, counts row): alone it needs the same row index
    alone, _ = dcl.ops.crop_draw_host(counts[:3], 16, 3, 5, keep_sparse=True)
    assert np.array_equal(alone, idx2[:3])


def test_lattice_dummy_and_sample_rows_of_the_host_twin(dcl):
    rng = np.random.default_rng(0)
    n, cap, npoint, S, unit, half = 3, 50, 16, 64, [0.006, 0.005, 0.007], 0.192
    xyz = rng.uniform(-0.25, 0.25, (n, cap, 3)).astype(np.float32)
    rgb = rng.uniform(-0.5, 0.5, (n, cap, 3)).astype(np.float32)
    counts = np.array([[50, 50, 50], [0, 0, 0], [50, 20, 50]], np.int32)
    idx, valid = dcl.ops.crop_draw_host(counts, npoint, 1, 0)
    assert valid.tolist() == [1, 0, 1]
    feats, coords = dcl.ops.crop_sample_valid_host(xyz, rgb, idx, counts, valid, half, unit, S)
    feats, coords = feats.reshape(n, npoint, 7), coords.reshape(n, npoint, 4)
    u = np.asarray(unit, np.float32)
    for i in (0, 2):
        p = xyz[i][idx[i]]
        assert np.array_equal(feats[i, :, 0], np.ones(npoint, np.float32)) and np.array_equal(feats[i, :, 1:4], rgb[i][idx[i]])
        assert np.array_equal(feats[i, :, 4:7], p)
        v = (p + np.float32(half)) / u
        if i == 2:                                                       # at most 32 points inside the grid: clamped first
            v = np.minimum(np.maximum(v, np.float32(0)), np.float32(S - 1))
        assert np.array_equal(coords[i, :, 1:], v.astype(np.int64)) and (coords[i, :, 0] == i).all()
    j = np.arange(npoint)
    lat = np.stack([j % S, (j // S) % S, j // (S * S)], 1)
    assert np.array_equal(coords[1], np.concatenate([np.full((npoint, 1), 1), lat], 1))
    want = (lat.astype(np.float32) + np.float32(0.5)) * u - np.float32(half)
    assert np.array_equal(feats[1, :, 4:7], want) and not feats[1, :, 1:4].any() and (feats[1, :, 0] == 1).all()
    # the centre of a voxel voxelises into that voxel
    assert np.array_equal(((want + np.float32(half)) / u).astype(np.int64), lat)


# ---------------------------------------------------------------------------------------------- 4. uniformity over frames
def _sigmas(count, trials, p):
    return np.abs(count - trials * p).max() / np.sqrt(trials * p * (1.0 - p))


@pytest.mark.parametrize("seed,inst,m,npoint,T", [(7, 3, 64, 16, 20000), (1, 0, 64, 16, 20000), (3, 1, 100, 99, 20000),
                                                  (4, 2, 1025, 1024, 2000)])
def test_without_replacement_every_index_is_equally_likely(dcl, seed, inst, m, npoint, T):
    """over frames 0 .. T-1 the number of draws that INCLUDE index i is Binomial(T, npoint / m) and the number that have it in
    slot 0 is Binomial(T, 1 / m): both within 5 sigma for every i (a cap, not a measurement)"""
    counts = counts_with(inst, m)
    incl, first = np.zeros(m), np.zeros(m)
    for f in range(T):
        d = dcl.ops.crop_draw_host(counts, npoint, seed, f)[0][inst]
        incl[d] += 1
        first[d[0]] += 1
    s_incl, s_first = _sigmas(incl, T, npoint / m), _sigmas(first, T, 1.0 / m)
    print("inclusion %.2f sigma, slot 0 %.2f sigma (cap 5)" % (s_incl, s_first))
    assert s_incl <= 5.0 and s_first <= 5.0


def test_with_replacement_every_value_is_equally_likely(dcl):
    seed, inst, m, npoint, T = 7, 3, 10, 16, 20000
    counts = counts_with(inst, m)
    hist = np.zeros(m)
    for f in range(T):
        hist += np.bincount(dcl.ops.crop_draw_host(counts, npoint, seed, f)[0][inst], minlength=m)
    s = _sigmas(hist, T * npoint, 1.0 / m)
    print("per-value count %.2f sigma (cap 5)" % s)
    assert s <= 5.0
