"""The device draw (csrc/crop_draw.hip: k_crop_draw) against its host twin, bit for bit, on every route to the result; the
valid-instance sample against crop_sample and the lattice dummy crop (k_crop_sample_valid)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def sizes(npoint):
    """the point counts at which the kernel takes another path: nothing, with replacement up to npoint, just past it (every
    index passes the first threshold), past the LDS list (8192), many passes"""
    return [0, 1, 5, npoint - 1, npoint, npoint + 1, 2 * npoint + 3, 4097, 70001, 300000]


def counts_of(ms):
    return np.repeat(np.asarray(ms, np.int32)[:, None], 3, 1)


_HOST = {}


def host_draw(dcl, npoint, seed, frame):
    """the host twin's draw of the sizes() batch, once per (npoint, seed, frame)"""
    key = (npoint, seed, frame)
    if key not in _HOST:
        _HOST[key] = dcl.ops.crop_draw_host(counts_of(sizes(npoint)), npoint, seed, frame)
    return _HOST[key]


@pytest.mark.parametrize("frame", [0, 1 << 40])
@pytest.mark.parametrize("seed", [1, 0xFEDCBA9876543210])
@pytest.mark.parametrize("npoint", [1, 16, 1000, 1024, 4096])
def test_kernel_equals_the_host_twin_bit_for_bit(dcl, npoint, seed, frame):
    ms = sizes(npoint)
    counts = torch.from_numpy(counts_of(ms)).cuda()
    want_idx, want_valid = host_draw(dcl, npoint, seed, frame)
    idx, valid = dcl.ops.crop_draw(counts, npoint, seed, frame)
    assert idx.dtype == torch.int64 and valid.dtype == torch.int32 and idx.shape == (len(ms), npoint)
    assert valid.cpu().tolist() == want_valid.tolist() == [int(m > 0) for m in ms]
    got = idx.cpu().numpy()
    for r, m in enumerate(ms):
        assert np.array_equal(got[r], want_idx[r]), (r, m)
        if m > npoint:
            assert len(set(got[r].tolist())) == npoint
        assert got[r].min() >= 0 and got[r].max() < max(m, 1)
    again, _ = dcl.ops.crop_draw(counts, npoint, seed, frame)                           # a second call: the same bits
    assert torch.equal(again, idx)


@pytest.mark.parametrize("npoint", [16, 1024, 4096])
def test_every_route_gives_the_same_bits(request, dcl, npoint):
    """the diagnostic library's switch forces each route of the selection: radix select alone, a guess far too small (widened),
    a guess of everything (the list overflows: radix select behind it)"""
    from test_gpu_ops import enter_diag
    lib = enter_diag(dcl, request)
    request.addfinalizer(lambda: lib.dcl_debug_crop_draw_route(0))
    counts = torch.from_numpy(counts_of(sizes(npoint))).cuda()
    want_idx, _ = host_draw(dcl, npoint, 1, 0)
    for route in (0, 1, 2, 3):
        lib.dcl_debug_crop_draw_route(route)
        idx, _ = dcl.ops.crop_draw(counts, npoint, 1, 0)
        assert np.array_equal(idx.cpu().numpy(), want_idx), route


def test_a_row_alone_equals_the_row_in_a_batch(dcl):
    npoint = 1024
    ms = sizes(npoint)
    counts = torch.from_numpy(counts_of(ms)).cuda()
    idx, _ = dcl.ops.crop_draw(counts, npoint, 5, 9)
    first, _ = dcl.ops.crop_draw(counts[:1].contiguous(), npoint, 5, 9)
    assert torch.equal(first[0], idx[0])
    for r in (4, 6, 9):                                   # a later row alone: its row index is part of its stream
        alone = torch.zeros_like(counts[:r + 1])
        alone[r] = counts[r]
        got, valid = dcl.ops.crop_draw(alone, npoint, 5, 9)
        assert torch.equal(got[r], idx[r]) and valid.cpu().tolist() == [0] * r + [1] and not got[:r].any()


def test_validity_rule_on_the_device(dcl):
    counts = np.array([[0, 0, 0], [40, 20, 40], [5000, 4000, 4000], [3000, 32, 3000], [9, 0, 0]], np.int32)
    for keep_sparse in (False, True):
        want_idx, want_valid = dcl.ops.crop_draw_host(counts, 16, 3, 5, min_valid=32, keep_sparse=keep_sparse)
        idx, valid = dcl.ops.crop_draw(torch.from_numpy(counts).cuda(), 16, 3, 5, min_valid=32, keep_sparse=keep_sparse)
        assert valid.cpu().tolist() == want_valid.tolist() == ([0, 1, 1, 1, 0] if keep_sparse else [0, 0, 1, 0, 0])
        assert np.array_equal(idx.cpu().numpy(), want_idx)


def _cloud(n, cap, seed=0):
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-0.25, 0.25, (n, cap, 3)).astype(np.float32)                      # some points outside the 0.384 m grid
    rgb = rng.uniform(-0.5, 0.5, (n, cap, 3)).astype(np.float32)
    return xyz, rgb


@pytest.mark.parametrize("npoint", [16, 1024])
def test_sample_valid_equals_crop_sample_and_the_lattice(dcl, npoint):
    ops = dcl.ops
    n, cap, S, unit, half = 4, 3000, 64, [0.006] * 3, 0.192
    xyz, rgb = _cloud(n, cap)
    xyz[[0, 3]] *= np.float32(0.75)                       # the filtered instances: every point inside the grid, as crop_points leaves them
    #               good             empty mask    sparse: clamped      fewer points than samples
    counts = np.array([[3000, 2500, 2500], [0, 0, 0], [3000, 20, 3000], [700, 700, 700]], np.int32)
    xyz_t, rgb_t, cnt_t = torch.from_numpy(xyz).cuda(), torch.from_numpy(rgb).cuda(), torch.from_numpy(counts).cuda()
    idx, valid = ops.crop_draw(cnt_t, npoint, 11, 3)
    assert valid.cpu().tolist() == [1, 0, 1, 1]
    feats, coords = ops.crop_sample_valid(xyz_t, rgb_t, idx, cnt_t, valid, half, unit, S)
    want_f, want_c = ops.crop_sample(xyz_t, rgb_t, idx, cnt_t, half, unit, S)            # (row 1: indices 0 of an unwritten cloud)
    F, Cc = feats.view(n, npoint, 7), coords.view(n, npoint, 4)
    for r in (0, 2, 3):
        assert torch.equal(F[r], want_f.view(n, npoint, 7)[r]) and torch.equal(Cc[r], want_c.view(n, npoint, 4)[r]), r
    j = np.arange(npoint)
    lat = np.stack([j % S, (j // S) % S, j // (S * S)], 1)
    assert np.array_equal(Cc[1].cpu().numpy(), np.concatenate([np.full((npoint, 1), 1), lat], 1))
    centre = (lat.astype(np.float32) + np.float32(0.5)) * np.asarray(unit, np.float32) - np.float32(half)
    want_row = np.concatenate([np.ones((npoint, 1), np.float32), np.zeros((npoint, 3), np.float32), centre], 1)
    assert np.array_equal(F[1].cpu().numpy(), want_row)
    host_f, host_c = ops.crop_sample_valid_host(xyz, rgb, idx.cpu().numpy(), counts, valid.cpu().numpy(), half, unit, S)
    assert np.array_equal(feats.cpu().numpy(), host_f) and np.array_equal(coords.cpu().numpy(), host_c)
    # the dummy crop in the one-launch voxelisation: one point per voxel, the pitch flag stays down
    occ, p2v, v2p, info = ops.voxelize_idx_crops(coords, n, npoint, S, 4, pitch=33)
    V, ma, err = info.cpu().tolist()
    assert err == 0
    assert int((occ[:V, 0] == 1).sum()) == npoint
