"""Gradients of pointnet_lib's group_points / gather_points / three_interpolate (csrc/backward.hip, include/dclnet_hip.h).

Contract: every element (b, c, j) of grad_points starts from its value on entry and gets the contributions that name j
added one at a time in ascending flat position order (p*nsample + s, p, i*3 + k; interpolation: fp32(grad_out * weight)
first).  That is numpy.add.at on float32 arrays, so numpy is a bit-exact oracle here.  No test passes an index outside
[0, n)."""
import importlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def add_at(init, idx_flat, vals):
    """init (B,C,N) f32, idx_flat (B,Q) int, vals (B,C,Q) f32 -> init + the scatter, sequential in q per element"""
    out = init.astype(np.float32).copy()
    for b in range(out.shape[0]):
        for c in range(out.shape[1]):
            np.add.at(out[b, c], idx_flat[b], vals[b, c])
    return out


def interp_vals(go, w):
    """fp32(grad_out[b,c,i] * weight[b,i,k]) at flat position i*3 + k"""
    B, C, n = go.shape
    return (go[:, :, :, None].astype(np.float32) * w[:, None, :, :].astype(np.float32)).reshape(B, C, 3 * n)


def _cloud(rng, b, n):
    return rng.uniform(-0.15, 0.15, (b, n, 3)).astype(np.float32)


def _ball_idx(dcl, rng, b, n, npoint, ns, r):
    """indices of a real ball_query: centres from the cloud, unused slots padded with the first hit"""
    xyz = _cloud(rng, b, n)
    new = np.ascontiguousarray(xyz[:, rng.choice(n, npoint, replace=False)])
    idx = dcl.ops.ball_query(r, ns, cuda(xyz), cuda(new)).cpu().numpy()
    return idx


# ------------------------------------------------------------------------------------------- bit-exact ops
@pytest.mark.parametrize("B,C,N,npoint,ns", [
    (1, 1, 700, 50, 1),          # one point per thread, nsample 1
    (3, 20, 700, 77, 3),         # positions per row not a multiple of 4 (scalar staging)
    (3, 20, 1500, 200, 16),      # two points per thread
    (1, 20, 4001, 200, 64),      # four points per thread, two walking tiles (12800 positions)
    (3, 1, 9000, 160, 64),       # eight points per thread
    (3, 20, 12287, 300, 16),     # twelve points per thread
    (1, 3, 13001, 150, 64),      # two point blocks
    (1, 3, 20000, 150, 64),      # two cursor windows of the inverse index
])
def test_group_points_grad_bit_exact_on_ball_query_indices(dcl, B, C, N, npoint, ns):
    rng = np.random.default_rng(N + ns)
    idx = _ball_idx(dcl, rng, B, N, npoint, ns, 0.04)
    assert (idx >= 0).all() and (idx < N).all()
    go = rng.normal(size=(B, C, npoint, ns)).astype(np.float32)
    want = add_at(np.zeros((B, C, N), np.float32), idx.reshape(B, -1), go.reshape(B, C, -1))
    got = dcl.ops.group_points_grad(cuda(go), cuda(idx), N).cpu().numpy()
    assert np.array_equal(bits(got), bits(want))
    # points no position names keep their value (here: zero)
    unused = np.ones((B, N), bool)
    for b in range(B):
        unused[b, np.unique(idx[b])] = False
    assert unused.any() and (got.transpose(0, 2, 1)[unused] == 0).all()


def test_group_points_grad_one_point_named_by_every_position_and_accumulation(dcl):
    """every position names point 5: one list of npoint*nsample entries, added in order; grad_points not zero on entry"""
    rng = np.random.default_rng(3)
    B, C, N, npoint, ns = 3, 20, 777, 130, 64
    idx = np.full((B, npoint, ns), 5, np.int32)
    idx[1] = rng.integers(0, N, (npoint, ns))                   # a plain random cloud beside it
    go = rng.normal(size=(B, C, npoint, ns)).astype(np.float32)
    init = rng.normal(size=(B, C, N)).astype(np.float32)
    want = add_at(init, idx.reshape(B, -1), go.reshape(B, C, -1))
    gp = cuda(init)
    out = dcl.ops.group_points_grad(cuda(go), cuda(idx), N, grad_points=gp)
    assert out.data_ptr() == gp.data_ptr()
    got = gp.cpu().numpy()
    assert np.array_equal(bits(got), bits(want))
    assert np.array_equal(bits(np.delete(got[0], 5, axis=1)), bits(np.delete(init[0], 5, axis=1)))


@pytest.mark.parametrize("B,C,N,npoint", [(1, 1, 700, 50), (3, 20, 1337, 123), (3, 20, 12288, 2048), (2, 5, 30001, 999)])
def test_gather_points_grad_bit_exact(dcl, B, C, N, npoint):
    rng = np.random.default_rng(N)
    idx = rng.integers(0, N, (B, npoint)).astype(np.int32)
    idx[:, :7] = 11                                             # repeats
    go = rng.normal(size=(B, C, npoint)).astype(np.float32)
    init = rng.normal(size=(B, C, N)).astype(np.float32)
    want = add_at(init, idx, go)
    gp = cuda(init)
    dcl.ops.gather_points_grad(cuda(go), cuda(idx), N, grad_points=gp)
    assert np.array_equal(bits(gp.cpu().numpy()), bits(want))
    fresh = dcl.ops.gather_points_grad(cuda(go), cuda(idx), N).cpu().numpy()
    assert np.array_equal(bits(fresh), bits(add_at(np.zeros_like(init), idx, go)))


@pytest.mark.parametrize("B,C,n,m", [(1, 1, 100, 7), (3, 20, 1001, 333), (3, 20, 5000, 2047), (2, 3, 4000, 13001)])
def test_three_interpolate_grad_bit_exact_on_three_nn_indices(dcl, B, C, n, m):
    rng = np.random.default_rng(n + m)
    unknown, known = _cloud(rng, B, n), _cloud(rng, B, m)
    d2, idx = dcl.ops.three_nn(cuda(unknown), cuda(known))
    w = (1.0 / (torch.sqrt(d2) + 1e-8))
    w = (w / w.sum(2, keepdim=True)).contiguous()
    idx, w = idx.cpu().numpy(), w.cpu().numpy()
    idx[0, :5] = [1, 1, 1]                                      # repeated neighbours inside one row
    go = rng.normal(size=(B, C, n)).astype(np.float32)
    init = rng.normal(size=(B, C, m)).astype(np.float32)
    want = add_at(init, idx.reshape(B, -1), interp_vals(go, w))
    gp = cuda(init)
    dcl.ops.three_interpolate_grad(cuda(go), cuda(idx), cuda(w), m, grad_points=gp)
    assert np.array_equal(bits(gp.cpu().numpy()), bits(want))


def test_group_points_grad_at_the_benchmarked_shape(dcl, oracle):
    """bench.py's primitive shape (B=32, C=64, N=12288, npoint=2048 FPS centres, nsample=64, r=0.03): two calls give the
    same bits; clouds 0 / 13 / 31 against numpy (the op is independent per cloud, as in test_gpu_ops' forward check)"""
    B, N, NP, NS, C, r = 32, 12288, 2048, 64, 64, 0.03
    data = dcl.synth.make_batch(B, N, 64)
    xyz = data["inp"]["feats"][:, 4:7].reshape(B, N, 3).contiguous()
    fps = dcl.ops.furthest_point_sampling(xyz.cuda(), NP)
    new_xyz = torch.gather(xyz, 1, fps.cpu().long().unsqueeze(-1).expand(-1, -1, 3)).contiguous()
    idx = dcl.ops.ball_query(r, NS, xyz.cuda(), new_xyz.cuda())
    g = torch.Generator(device="cuda").manual_seed(7)
    go = torch.randn(B, C, NP, NS, device="cuda", generator=g)
    a = dcl.ops.group_points_grad(go, idx, N)
    b = dcl.ops.group_points_grad(go, idx, N)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    idx_h = idx.cpu().numpy()
    for bi in (0, 13, 31):
        want = add_at(np.zeros((1, C, N), np.float32), idx_h[bi:bi + 1].reshape(1, -1),
                      go[bi:bi + 1].reshape(1, C, -1).cpu().numpy())
        assert np.array_equal(bits(a[bi:bi + 1].cpu().numpy()), bits(want)), bi
    # the interpolation backward at the same clouds: (32,64,12288) -> (32,64,2048)
    d2, i3 = dcl.ops.three_nn(xyz.cuda(), new_xyz.cuda())
    w = 1.0 / (torch.sqrt(d2) + 1e-8)
    w = (w / w.sum(2, keepdim=True)).contiguous()
    gi = torch.randn(B, C, N, device="cuda", generator=g)
    ia = dcl.ops.three_interpolate_grad(gi, i3, w, NP)
    ib = dcl.ops.three_interpolate_grad(gi, i3, w, NP)
    assert torch.equal(ia.view(torch.int32), ib.view(torch.int32))
    i3h, wh = i3.cpu().numpy(), w.cpu().numpy()
    for bi in (0, 31):
        want = add_at(np.zeros((1, C, NP), np.float32), i3h[bi:bi + 1].reshape(1, -1),
                      interp_vals(gi[bi:bi + 1].cpu().numpy(), wh[bi:bi + 1]))
        assert np.array_equal(bits(ia[bi:bi + 1].cpu().numpy()), bits(want)), bi


# ------------------------------------------------------------------------------------------- autograd
def _pu():
    return importlib.import_module("dcl-net_amd.libs.pointnet_lib.pointnet2_utils")


def _scatter64(vals, idx_flat, n):
    """float64 scatter of vals (B,C,Q) over idx_flat (B,Q) -> (B,C,n), and the same over |vals| (the tolerance scale)"""
    B, C, _ = vals.shape
    ix = idx_flat.long().unsqueeze(1).expand(B, C, -1)
    s = torch.zeros(B, C, n, dtype=torch.float64, device=vals.device).scatter_add_(2, ix, vals.double())
    a = torch.zeros(B, C, n, dtype=torch.float64, device=vals.device).scatter_add_(2, ix, vals.double().abs())
    return s, a


def _close(got, want, scale):
    err = (got.double() - want).abs()
    assert bool((err <= 1e-5 * scale + 1e-30).all()), float((err - 1e-5 * scale).max())


def test_mirror_functions_backward(dcl):
    pu = _pu()
    rng = np.random.default_rng(21)
    B, C, N, npoint, ns = 3, 20, 1500, 200, 16
    idx = cuda(_ball_idx(dcl, rng, B, N, npoint, ns, 0.04))
    f = cuda(rng.normal(size=(B, C, N)).astype(np.float32)).requires_grad_(True)
    with torch.no_grad():
        plain = pu.grouping_operation(f, idx)
    out = pu.grouping_operation(f, idx)
    assert out.grad_fn is not None and torch.equal(out.detach(), plain)
    go = torch.randn_like(out)
    out.backward(go)
    want, scale = _scatter64(go.reshape(B, C, -1), idx.reshape(B, -1), N)
    _close(f.grad, want, scale)
    # the reference class names, through .apply
    f.grad = None
    pu.GroupingOperation.apply(f, idx.long()).backward(go)
    _close(f.grad, want, scale)
    # gather_operation
    gidx = cuda(rng.integers(0, N, (B, 300)).astype(np.int32))
    f.grad = None
    o = pu.gather_operation(f, gidx)
    assert torch.equal(o.detach(), dcl.ops.gather_points(f.detach(), gidx))
    go2 = torch.randn_like(o)
    o.backward(go2)
    want, scale = _scatter64(go2, gidx, N)
    _close(f.grad, want, scale)
    # three_interpolate: gradient for features only
    n = 4000
    unknown = cuda(_cloud(rng, B, n))
    known = cuda(_cloud(rng, B, N))
    dist, i3 = pu.three_nn(unknown, known)
    w = (1.0 / (dist + 1e-8))
    w = (w / w.sum(2, keepdim=True)).contiguous().requires_grad_(True)
    f.grad = None
    o3 = pu.three_interpolate(f, i3, w)
    assert torch.equal(o3.detach(), dcl.ops.three_interpolate(f.detach(), i3, w.detach()))
    go3 = torch.randn_like(o3)
    o3.backward(go3)
    vals = (go3.double()[:, :, :, None] * w.detach().double()[:, None]).reshape(B, C, -1)
    want, scale = _scatter64(vals, i3.reshape(B, -1), N)
    _close(f.grad, want, scale)
    assert w.grad is None                                      # the reference gives no weight gradient either


def _group_grads64(G, idx, C, N, with_feats, feats_first):
    """float64 gradients of the reference composition: G (B, [C+]3, np, ns) -> (d features, d xyz (B,N,3), d new_xyz)"""
    B = G.shape[0]
    gf, gx = (G[:, :C], G[:, C:]) if feats_first else (G[:, 3:], G[:, :3])
    if not with_feats:
        gx = G
    dxs, dxa = _scatter64(gx.reshape(B, 3, -1), idx.reshape(B, -1), N)
    dnew = -gx.double().sum(-1).transpose(1, 2)
    dnew_scale = gx.double().abs().sum(-1).transpose(1, 2)
    out = dict(xyz=(dxs.transpose(1, 2), dxa.transpose(1, 2)), new_xyz=(dnew, dnew_scale))
    if with_feats:
        out["features"] = _scatter64(gf.reshape(B, C, -1), idx.reshape(B, -1), N)
    return out


@pytest.mark.parametrize("with_feats", [True, False])
def test_query_and_group_backward_and_fast_path_bits(dcl, with_feats):
    pu = _pu()
    rng = np.random.default_rng(5)
    B, C, N, npoint, ns, r = 2, 6, 2000, 128, 16, 0.05
    xyz0 = _cloud(rng, B, N)
    new0 = np.ascontiguousarray(xyz0[:, rng.choice(N, npoint, replace=False)] + 1e-3)
    f0 = rng.normal(size=(B, C, N)).astype(np.float32)
    qg = pu.QueryAndGroup(r, ns, use_xyz=True)
    with torch.no_grad():
        fast = qg(cuda(xyz0), cuda(new0), cuda(f0) if with_feats else None)
    xyz = cuda(xyz0).requires_grad_(True)
    new = cuda(new0).requires_grad_(True)
    f = cuda(f0).requires_grad_(True) if with_feats else None
    out = qg(xyz, new, f)
    assert out.grad_fn is not None
    assert torch.equal(out.detach().view(torch.int32), fast.view(torch.int32))      # same bits on both paths
    G = torch.randn_like(out)
    out.backward(G)
    idx = pu.ball_query(r, ns, cuda(xyz0), cuda(new0))
    want = _group_grads64(G, idx, C if with_feats else 0, N, with_feats, feats_first=True)
    _close(xyz.grad, *want["xyz"])
    _close(new.grad, *want["new_xyz"])
    if with_feats:
        _close(f.grad, *want["features"])


def test_knn_and_group_backward(dcl):
    pu = _pu()
    rng = np.random.default_rng(9)
    B, C, N, M, K = 2, 5, 1200, 100, 8
    xyz0 = _cloud(rng, B, N)
    new0 = np.ascontiguousarray(xyz0[:, rng.choice(N, M, replace=False)] + 1e-3)
    f0 = rng.normal(size=(B, C, N)).astype(np.float32)
    kg = pu.KNNAndGroup(0.1, K, use_xyz=True)
    with torch.no_grad():
        plain = kg(cuda(xyz0), cuda(new0), features=cuda(f0))
    xyz = cuda(xyz0).requires_grad_(True)
    new = cuda(new0).requires_grad_(True)
    f = cuda(f0).requires_grad_(True)
    out = kg(xyz, new, features=f)
    assert torch.equal(out.detach().view(torch.int32), plain.view(torch.int32))
    G = torch.randn_like(out)
    out.backward(G)
    _, idx = pu.knn(K, cuda(new0), cuda(xyz0))
    want = _group_grads64(G, idx, C, N, True, feats_first=False)
    _close(xyz.grad, *want["xyz"])
    _close(new.grad, *want["new_xyz"])
    _close(f.grad, *want["features"])


# ------------------------------------------------------------------------------------------- launch census
def test_forward_only_calls_launch_no_grad_kernel(request, dcl):
    import test_gpu_ops as TO
    import test_kernel_census as TC
    lib = TO.enter_diag(dcl, request)
    pu = _pu()
    rng = np.random.default_rng(2)
    B, C, N, npoint, ns = 2, 4, 900, 64, 16
    xyz, new = cuda(_cloud(rng, B, N)), cuda(_cloud(rng, B, npoint))
    f = cuda(rng.normal(size=(B, C, N)).astype(np.float32))
    fg = f.clone().requires_grad_(True)
    lib.dcl_debug_launch_census_reset()
    idx = pu.ball_query(0.05, ns, xyz, new)
    pu.grouping_operation(f, idx)
    pu.gather_operation(f, idx[:, :, 0].contiguous())
    dist, i3 = pu.three_nn(new, xyz)
    pu.three_interpolate(f, i3, dist.contiguous())
    pu.QueryAndGroup(0.05, ns)(xyz, new, f)
    pu.KNNAndGroup(0.05, ns)(xyz, new, features=f)
    with torch.no_grad():
        pu.QueryAndGroup(0.05, ns)(xyz, new, fg)
        pu.grouping_operation(fg, idx)
    pu.grouping_operation(fg, idx)                             # records a graph, runs no backward
    torch.cuda.synchronize()
    seen = TC.census(lib)
    assert any(k.startswith("k_group_points") for k in seen), seen              # the census did count the forwards
    grad_k = {k: v for k, v in seen.items() if k.startswith(("k_pn_inv", "k_pn_grad"))}
    assert not grad_k, grad_k
    # ... and a backward does launch them
    pu.grouping_operation(fg, idx).sum().backward()
    torch.cuda.synchronize()
    seen = TC.census(lib)
    assert seen.get("k_pn_inv_rank", 0) == 1 and sum(v for k, v in seen.items() if k.startswith("k_pn_grad_gather")) == 1
