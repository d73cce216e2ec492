"""ops.linear_wgrad and ops.relu_bwd (csrc/linear_bwd.hip) on the GPU: against float64 within the bound that the pinned order
gives, exactly on small-integer operands, bit-identical call after call and for every pitch and alignment, and writing
nothing outside their output block."""
import importlib
import re
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = int(re.search(r"^#define DCL_WGRAD_ROWS (\d+)\s*$", open(os.path.join(ROOT, "include", "dclnet_hip.h")).read(),
                  flags=re.M).group(1))
U = 2.0 ** -24
POISON = -7777.25

WGRAD_CASES = [(1, 1, 1), (33, 5, 3), (R - 1, 32, 32), (R + 1, 130, 96), (2 * R + 7, 512, 3), (2048, 128, 160)]


def _operands(M, P, Q, kind, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "integers":
        a = torch.randint(-4, 5, (M, P), generator=g).float()
        b = torch.randint(-4, 5, (M, Q), generator=g).float()
    else:
        a, b = torch.randn(M, P, generator=g), torch.randn(M, Q, generator=g) * 3.0
    return a.cuda(), b.cuda()


def _block(t, left, right):
    """the same values as a column block of a wider buffer whose base is ONE float past an allocation's start: rows pitched
    by left + width + right floats, 4-byte but not 16-byte aligned"""
    rows, w = t.shape
    ld = left + w + right
    flat = torch.full((rows * ld + 1,), POISON, dtype=torch.float32, device=t.device)
    wide = flat[1:].view(rows, ld)
    wide[:, left:left + w] = t
    return wide, wide[:, left:left + w]


@pytest.fixture(scope="module")
def wgrad_runs():
    """every case and operand kind once: (dense result, a second dense launch, the strided / unaligned run, its poisoned frame,
    float64 result and float64 magnitude sum)"""
    dcl = importlib.import_module("dcl-net_amd")
    out = {}
    for i, (M, P, Q) in enumerate(WGRAD_CASES):
        for kind in ("random", "integers"):
            a, b = _operands(M, P, Q, kind, 100 + i)
            dense = dcl.ops.linear_wgrad(a, b)
            again = dcl.ops.linear_wgrad(a, b)
            _, ab = _block(a, 2, 3)
            _, bb = _block(b, 1, 2)
            assert ab.data_ptr() % 16 != 0 or bb.data_ptr() % 16 != 0
            frame, ob = _block(torch.full((P, Q), POISON, device="cuda"), 3, 4)
            got = dcl.ops.linear_wgrad(ab, bb, out=ob)
            assert got.data_ptr() == ob.data_ptr()
            want = a.double().t() @ b.double()
            mag = a.double().abs().t() @ b.double().abs()
            out[(M, P, Q, kind)] = tuple(t.cpu() for t in (dense, again, ob, frame, want, mag))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("case", WGRAD_CASES)
def test_wgrad_within_the_pinned_orders_bound_of_float64(dcl, wgrad_runs, case):
    M, P, Q = case
    splits = dcl.ops.linear_wgrad_splits(M)
    assert splits == max(1, -(-M // R))
    dense, _, _, _, want, mag = wgrad_runs[case + ("random",)]
    bound = (R + splits + 2) * U * mag
    err = (dense.double() - want).abs()
    print("wgrad %s: max error / bound = %.3g" % (case, float((err / bound.clamp_min(1e-300)).max())))
    assert bool((err <= bound).all())


@pytest.mark.parametrize("case", WGRAD_CASES)
def test_wgrad_is_exact_on_small_integers(wgrad_runs, case):
    dense, _, block, _, want, _ = wgrad_runs[case + ("integers",)]
    assert float(want.abs().max()) < 2 ** 24                       # every partial sum is representable
    assert torch.equal(dense.double(), want)
    assert torch.equal(block.double(), want)


@pytest.mark.parametrize("kind", ["random", "integers"])
@pytest.mark.parametrize("case", WGRAD_CASES)
def test_wgrad_same_bits_again_and_for_any_pitch_and_alignment(wgrad_runs, case, kind):
    M, P, Q = case
    dense, again, block, frame, _, _ = wgrad_runs[case + (kind,)]
    assert torch.equal(dense.view(torch.int32), again.view(torch.int32))
    assert torch.equal(dense.view(torch.int32), block.contiguous().view(torch.int32))
    outside = torch.ones_like(frame, dtype=torch.bool)
    outside[:, 3:3 + Q] = False
    assert bool((frame[outside] == POISON).all())                  # nothing beside the column block was written


def test_wgrad_of_no_rows_is_zero(dcl):
    out = torch.full((5, 7), POISON, device="cuda")
    dcl.ops.linear_wgrad(torch.empty((0, 5), device="cuda"), torch.empty((0, 7), device="cuda"), out=out)
    assert bool((out == 0).all())


RELU_CASES = [(R + 1, 96, 257), (2 * 128, 1024, 128)]              # (M, P, rows per crop): two crops each


def _relu_inputs(M, P, seed):
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(M, P, generator=g)
    h[torch.rand(M, P, generator=g) < 0.2] = 0.0                   # exact zeros: gradient 0
    h[0, 0], h[M - 1, P - 1] = 0.0, -0.0
    grad = torch.randn(M, P, generator=g)
    grad[torch.rand(M, P, generator=g) < 0.1] = 0.0
    assert bool((h < 0).any()) and bool((h == 0).any()) and bool((h > 0).any())
    return h.cuda(), grad.cuda()


@pytest.mark.parametrize("case", RELU_CASES)
@pytest.mark.parametrize("form", ["plain", "pooled"])
def test_relu_bwd(dcl, case, form):
    M, P, rpc = case
    h, grad = _relu_inputs(M, P, 7 + M)
    splits = dcl.ops.linear_wgrad_splits(M)
    if form == "plain":
        want = torch.where(h > 0, grad, torch.zeros_like(grad))
        dz, db = dcl.ops.relu_bwd(h, grad)
        g2 = grad.clone()
        dz_in, db_in = dcl.ops.relu_bwd(h, g2, out=g2)
        assert dz_in.data_ptr() == g2.data_ptr()
    else:
        g = torch.Generator().manual_seed(3)
        roww = torch.rand(M, generator=g).cuda()
        gpool = torch.randn(2, P, generator=g).cuda()
        crop = torch.arange(M, device="cuda") // rpc
        want = torch.where(h > 0, roww[:, None] * gpool[crop], torch.zeros_like(h))
        dz, db = dcl.ops.relu_bwd(h, roww=roww, gpool=gpool, rows_per_crop=rpc)
        h2 = h.clone()
        dz_in, db_in = dcl.ops.relu_bwd(h2, roww=roww, gpool=gpool, rows_per_crop=rpc, out=h2)
        assert dz_in.data_ptr() == h2.data_ptr()
    # dz: the torch expression bit for bit
    assert torch.equal(dz.view(torch.int32), want.view(torch.int32))
    assert bool((dz[h <= 0] == 0).all())
    # in place = out of place, and a column block of a wider buffer = dense, bit for bit
    assert torch.equal(dz_in.view(torch.int32), dz.view(torch.int32))
    assert torch.equal(db_in.view(torch.int32), db.view(torch.int32))
    _, hb = _block(h, 1, 2)
    frame, ob = _block(torch.full((M, P), POISON, device="cuda"), 3, 1)
    if form == "plain":
        dz_b, db_b = dcl.ops.relu_bwd(hb, _block(grad, 2, 2)[1], out=ob)
    else:
        dz_b, db_b = dcl.ops.relu_bwd(hb, roww=roww, gpool=_block(gpool, 1, 1)[1], rows_per_crop=rpc, out=ob)
    assert torch.equal(dz_b.contiguous().view(torch.int32), dz.view(torch.int32))
    assert torch.equal(db_b.view(torch.int32), db.view(torch.int32))
    outside = torch.ones_like(frame, dtype=torch.bool)
    outside[:, 3:3 + P] = False
    assert bool((frame[outside] == POISON).all())
    # db: the pinned order's bound against float64
    want_db = want.double().sum(0)
    bound = (R + splits) * U * want.double().abs().sum(0)
    err = (db.double() - want_db).abs()
    print("relu_bwd %s %s: db max error / bound = %.3g" % (form, case, float((err / bound.clamp_min(1e-300)).max())))
    assert bool((err <= bound).all())
    # run to run
    if form == "plain":
        dz2, db2 = dcl.ops.relu_bwd(h, grad)
    else:
        dz2, db2 = dcl.ops.relu_bwd(h, roww=roww, gpool=gpool, rows_per_crop=rpc)
    assert torch.equal(dz2.view(torch.int32), dz.view(torch.int32)) and torch.equal(db2.view(torch.int32), db.view(torch.int32))
