"""The host twins of the refine loop's device form (refine_loop(compose="device"); include/dclnet_hip.h: dcl_refine_first_host,
dcl_pose_compose_host -- the kernels' own routines from csrc/refine_pose.h compiled for the host) against float64 under bounds
that count the roundings, and exactly on small integers; the new entry points' presence in both libraries and their refusals;
refine_loop's refusals that need no GPU.  tests/test_gpu_refine_loop.py compares the kernels with these twins bit for bit."""
import ctypes as C
import inspect
import os

import pytest
import torch

U = 2.0 ** -24                                           # unit roundoff of fp32

FIRST_SHAPES = [(1, 1, 4), (2, 128, 512), (3, 200, 8)]   # (b, n, c)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())


def rotations(b, g):
    """b random orthonormal matrices (QR of a Gaussian matrix), fp32"""
    q, _ = torch.linalg.qr(torch.randn(b, 3, 3, generator=g, dtype=torch.float64))
    return q.float().contiguous()


def magnitudes(shape, g, lo=0.05, hi=1.0):
    """entries with |x| in [lo, hi] and random signs"""
    mag = lo + (hi - lo) * torch.rand(shape, generator=g)
    sign = torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0)
    return (mag * sign).float().contiguous()


def first_case(b, n, c, seed=0, integers=False):
    """operands of refine_first: pts (b,n,3), R (b,3,3), t (b,3), W3 (3,c), term (b*n,c)"""
    g = torch.Generator().manual_seed(1000 * seed + 97 * b + 7 * n + c)
    if integers:
        ri = lambda shape, k: torch.randint(-k, k + 1, shape, generator=g).float()           # noqa: E731
        return ri((b, n, 3), 4), ri((b, 3, 3), 2), ri((b, 3), 4), ri((3, c), 3), ri((b * n, c), 50)
    return (magnitudes((b, n, 3), g), rotations(b, g), magnitudes((b, 3), g), torch.randn(3, c, generator=g),
            torch.randn(b * n, c, generator=g))


def first_float64(pts, R, t, W3, term):
    """relu(term + ((p - t) R) W3) in float64 and the magnitude S + |term| of the bound, S = sum_j sum_i |p_i - t_i| |R_ij| |W_jk|"""
    b, n, _ = pts.shape
    q = pts.double() - t.double().unsqueeze(1)
    cur = torch.bmm(q, R.double()).reshape(b * n, 3)
    ref = torch.relu(term.double() + cur @ W3.double())
    S = torch.bmm(q.abs(), R.double().abs()).reshape(b * n, 3) @ W3.double().abs()
    return ref, S + term.double().abs()


def compose_case(b, seed=0, integers=False):
    g = torch.Generator().manual_seed(31 * seed + b)
    if integers:
        ri = lambda shape, k: torch.randint(-k, k + 1, shape, generator=g).float()           # noqa: E731
        return ri((b, 3, 3), 3), ri((b, 3), 9), ri((b, 3, 3), 3), ri((b, 3), 9)
    return rotations(b, g), magnitudes((b, 3), g), rotations(b, g), magnitudes((b, 3), g, 0.001, 0.05)


# ---------------------------------------------------------------------------------------------------- 1. refine_first_host
@pytest.mark.parametrize("shape", FIRST_SHAPES, ids=lambda s: "b%d-n%d-c%d" % s)
def test_refine_first_host_against_float64(dcl, shape):
    """every element within 8 u (S + |term|): the subtraction (1), the three-rounding chain of the canonicalisation (3), the
    three-rounding chain of the layer (3), the addition of the term (1), to first order; ReLU is 1-Lipschitz"""
    pts, R, t, W3, term = first_case(*shape)
    got = dcl.ops.refine_first_host(pts, R, t, W3, term)
    ref, mag = first_float64(pts, R, t, W3, term)
    err = (got.double() - ref).abs()
    worst = float((err / mag.clamp_min(1e-300)).max()) / U
    print("refine_first_host %s: worst error %.3f u (S + |term|), bound 8" % (shape, worst))
    assert got.shape == term.shape and got.dtype == torch.float32
    assert bool((err <= 8 * U * mag).all())
    assert float(got.min()) >= 0.0


@pytest.mark.parametrize("shape", FIRST_SHAPES, ids=lambda s: "b%d-n%d-c%d" % s)
def test_refine_first_host_is_exact_on_small_integers(dcl, shape):
    pts, R, t, W3, term = first_case(*shape, integers=True)
    got = dcl.ops.refine_first_host(pts, R, t, W3, term)
    ref, _ = first_float64(pts, R, t, W3, term)
    assert torch.equal(got.double(), ref)
    assert bool((got > 0).any()) and bool((got == 0).any())


def test_refine_first_host_equals_rigid_points_host_then_the_layer(dcl):
    """the canonicalisation inside is dcl_rigid_points_host's routine: the same bits as composing the two by hand"""
    b, n, c = 2, 37, 12
    pts, R, t, W3, term = first_case(b, n, c, seed=3)
    cur = dcl.ops.rigid_points_host(pts, R, t, inverse=True).view(b * n, 3)
    z = torch.zeros(b, 3, 3)
    z[:] = torch.eye(3)
    again = dcl.ops.refine_first_host(cur.view(b, n, 3), z, torch.zeros(b, 3), W3, term)      # identity pose: cur passes through
    assert same_bits(dcl.ops.refine_first_host(pts, R, t, W3, term), again)


def test_refine_first_refusals(dcl):
    pts, R, t, W3, term = first_case(2, 8, 8)
    with pytest.raises(ValueError, match="c % 4"):
        dcl.ops.refine_first_host(pts, R, t, W3[:, :6].contiguous(), term[:, :6].contiguous())
    with pytest.raises(RuntimeError, match="GPU"):
        dcl.ops.refine_first(pts, R, t, W3, term)                                            # CPU tensors: no CPU fallback
    with pytest.raises(AssertionError):
        dcl.ops.refine_first_host(pts, R[:1], t, W3, term)


# ---------------------------------------------------------------------------------------------------- 2. pose_compose_host
@pytest.mark.parametrize("b", [1, 3])
def test_pose_compose_host_against_float64(dcl, b):
    """R_out within 4 u (|R| |dR|), t_out within 4 u (|R| |dt| + |t|), elementwise: a three-rounding chain (+ one addition)"""
    R, t, dR, dt = compose_case(b)
    R_out, t_out = dcl.ops.pose_compose_host(R, t, dR, dt)
    Rd, td, dRd, dtd = R.double(), t.double(), dR.double(), dt.double()
    eR = (R_out.double() - Rd @ dRd).abs()
    et = (t_out.double() - ((Rd @ dtd.unsqueeze(2)).squeeze(2) + td)).abs()
    mR = Rd.abs() @ dRd.abs()
    mt = (Rd.abs() @ dtd.abs().unsqueeze(2)).squeeze(2) + td.abs()
    print("pose_compose_host b=%d: worst %.3f u (R), %.3f u (t), bound 4" % (b, float((eR / mR).max()) / U, float((et / mt).max()) / U))
    assert bool((eR <= 4 * U * mR).all()) and bool((et <= 4 * U * mt).all())


@pytest.mark.parametrize("b", [1, 3])
def test_pose_compose_host_is_exact_on_small_integers(dcl, b):
    R, t, dR, dt = compose_case(b, integers=True)
    R_out, t_out = dcl.ops.pose_compose_host(R, t, dR, dt)
    assert torch.equal(R_out, R @ dR) and torch.equal(t_out, (R @ dt.unsqueeze(2)).squeeze(2) + t)
    assert torch.equal(R_out.double(), R.double() @ dR.double())


def test_pose_compose_host_row_major_known_answer(dcl):
    """R_out[i][j] = sum_k R[i][k] dR[k][j], t_out[i] = sum_k R[i][k] dt[k] + t[i] on a matrix that tells rows from columns"""
    R = torch.tensor([[[1.0, 2.0, 3.0], [4.0, 5.0, 6.0], [7.0, 8.0, 9.0]]])
    dR = torch.tensor([[[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]]])
    R_out, t_out = dcl.ops.pose_compose_host(R, torch.tensor([[10.0, 20.0, 30.0]]), dR, torch.tensor([[1.0, 0.0, -1.0]]))
    assert R_out.tolist() == [[[3.0, 1.0, 2.0], [6.0, 4.0, 5.0], [9.0, 7.0, 8.0]]]
    assert t_out.tolist() == [[8.0, 18.0, 28.0]]


# ---------------------------------------------------------------------------------------------------- 3. entries and refusals
NEW_ENTRIES = ("dcl_refine_first", "dcl_refine_first_host", "dcl_pose_compose_host", "dcl_refine_heads")


def test_entries_are_declared_exported_and_refuse_bad_arguments(dcl):
    import test_abi
    assert set(NEW_ENTRIES) <= set(test_abi.declared_symbols())
    libs = [("product", dcl._native.lib())]
    if os.path.exists(dcl._native.DIAG_SO_PATH):
        libs.append(("diagnostic", C.CDLL(dcl._native.DIAG_SO_PATH)))
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    for tag, lib in libs:
        assert all(hasattr(lib, s) for s in NEW_ENTRIES), tag
        assert int(lib.dcl_abi_version()) == 2, tag                                          # the entries join the ABI, the version stays
        # (every refusal below comes before any GPU call)
        assert lib.dcl_refine_first(1, 1, 6, p, p, p, p, p, p, None) == -1, tag              # c % 4
        assert lib.dcl_refine_first(1, 0, 4, p, p, p, p, p, p, None) == -1, tag              # n >= 1
        assert lib.dcl_refine_first(-1, 1, 4, p, p, p, p, p, p, None) == -1, tag
        assert lib.dcl_refine_first(65536, 1 << 14, 4, p, p, p, p, p, p, None) == -1, tag    # b * n * 3 beyond int32
        assert lib.dcl_refine_first(1, 1, 4, p, None, p, p, p, p, None) == -1, tag
        assert lib.dcl_refine_first(0, 1, 4, None, None, None, None, None, None, None) == 0, tag
        assert lib.dcl_refine_first_host(1, 1, 4, p, p, p, p, None, p) == -1, tag
        assert lib.dcl_pose_compose_host(-1, p, p, p, p, p, p) == -1, tag
        assert lib.dcl_pose_compose_host(1, p, p, None, p, p, p) == -1, tag
        assert lib.dcl_pose_compose_host(0, None, None, None, None, None, None) == 0, tag
        layers = (C.c_void_p * 6)(*[p.value] * 6)
        q = C.c_void_p(p.value + 128)
        assert lib.dcl_refine_heads(1, 0, p, layers, layers, p, p, p, q, q, p, p, p, None) == -1, tag       # T >= 1
        assert lib.dcl_refine_heads(65536, 1, p, layers, layers, p, p, p, q, q, p, p, p, None) == -1, tag
        assert lib.dcl_refine_heads(1, 1, p, layers, layers, p, p, p, p, q, p, p, p, None) == -1, tag       # R_out is R_in
        assert lib.dcl_refine_heads(1, 1, p, layers, layers, p, p, p, q, p, p, p, p, None) == -1, tag       # t_out is t_in
        assert lib.dcl_refine_heads(1, 1, None, layers, layers, p, p, p, q, q, p, p, p, None) == -1, tag
        assert lib.dcl_refine_heads(0, 1, None, None, None, None, None, None, None, None, None, None, None, None) == 0, tag
        assert lib.dcl_refine_heads(1, 0, p, layers, layers, p, p, p, q, q, p, p, p, None) == -1, tag
        lib.dcl_last_error.restype = C.c_char_p
        assert b"dcl_refine_heads: invalid argument" in lib.dcl_last_error(), tag


def test_refine_loop_refuses_bad_forms_before_any_gpu_call(dcl):
    """the form and the trajectory request are checked first: nothing of the arguments is touched (they are None here)"""
    with pytest.raises(ValueError, match="compose"):
        dcl.refiner.refine_loop(None, None, None, compose="gpu")
    with pytest.raises(ValueError, match="trajectory"):
        dcl.refiner.refine_loop(None, None, None, compose="host", trajectory=True)
    with pytest.raises(ValueError, match="trajectory"):
        dcl.refiner.refine_loop(None, None, None, trajectory=True)
    with pytest.raises(ValueError, match="compose"):
        dcl.refiner.stage2_chain(lambda data: None, None, {"labels": {"points_inp": None}}, compose="gpu")
    sig = inspect.signature(dcl.refiner.refine_loop).parameters
    assert sig["compose"].default == "host" and sig["trajectory"].default is False and sig["graph"].default is False
    assert inspect.signature(dcl.refiner.stage2_chain).parameters["compose"].default == "host"


def test_compose_is_read_by_the_loop_only(dcl):
    """eval Refiner.forward, train mode and Network never read the form"""
    for obj in (dcl.refiner.Refiner, dcl.DCL_Net.Network):
        assert "compose=" not in inspect.getsource(obj) and "COMPOSE_MODES" not in inspect.getsource(obj)
        assert "compose" not in inspect.signature(obj.__init__).parameters
