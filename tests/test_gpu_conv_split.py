"""The split-bf16 form of the LDS-DMA sparse-conv kernel (csrc/conv_body.h, SPLIT; ops.sparse_conv_sides(pieces=...)) against the
fp32 form of the same launch and against float64, on small shapes at which the kernel can still go wrong: one and two crops of a
16^3 grid, row counts that are no multiple of the 128-row tile (129 = one tile plus one row: the second tile has ONE live
row), rows with all 27 neighbours and rows with only the centre (the zero line), both backbones in one launch, natural and
ordered rows, few-row stream-K with its deferred combine, forced split-K with the in-launch ticket combine.

Error unit: 2^-24 sum |x| |w| per output (tests/split_cases.py).  The yardstick of the error tests is the EXISTING fp32 kernel's
error against float64 on the same operands, the bound 1.5 x that (DESIGN 5c's factor for the split GEMM against the fp32 chain).
Measured (profiles/conv_split.txt): see the per-case ratios there."""
import functools

import numpy as np
import pytest
import torch

import conv_split_cases as CS
from test_gpu_ops import cuda, enter_diag

pytestmark = pytest.mark.gpu

S = 16


@functools.lru_cache(maxsize=None)
def _geometry(dcl, b, n_per_crop, subm, seed):
    """voxel set -> (n_in, n_out, gather table on the device, the table on the host, (set, input mask) for order_rows)"""
    idx = CS.voxel_set(b, S, n_per_crop, seed)
    aset = dcl.ops.grid_from_indices(cuda(idx), b, S)
    out, nbr = dcl.spconv.ops.build_rulebook(aset, 3, 1, 1, subm)
    n_out = idx.shape[0] if subm else out.n
    return idx.shape[0], n_out, nbr, nbr.cpu().numpy(), ((aset if subm else out), aset.mask)


def _both(dcl, sides, subm, orders=None, **kw):
    """sides: [(x, w, nbr, n_out)] on the device -> (fp32 form outputs, split form outputs) of ONE launch over all sides"""
    feats, Ws, nbrs, n_outs = ([s[i] for s in sides] for i in range(4))
    pieces = [dcl.ops.conv_split_weight(w) for w in Ws]
    fp32 = dcl.ops.sparse_conv_sides(feats, nbrs, n_outs, Ws, subm, None, orders=orders, **kw)
    split = dcl.ops.sparse_conv_sides(feats, nbrs, n_outs, Ws, subm, pieces, orders=orders, **kw)
    return fp32, split


def _side(dcl, b, n_per_crop, cin, cout, subm, kind, seed, exact=True):
    n_in, n_out, nbr, nbr_h, oset = _geometry(dcl, b, n_per_crop, subm, seed)
    x, w = (CS.exact_operands if exact else CS.error_operands)(kind, n_in, cin, cout, seed)
    return (cuda(x), cuda(w), nbr, n_out), (x, w, nbr_h, n_out), oset


# ------------------------------------------------------------------------------------------------------ prepared pieces
@pytest.mark.parametrize("cin,cout", [(32, 64), (64, 128), (128, 256), (64, 64), (128, 128)])
def test_prepared_pieces_sum_to_the_filter_exactly_and_sit_in_kernel_order(dcl, cin, cout):
    rng = np.random.default_rng(cin + cout)
    w = (rng.normal(size=(27, cin, cout)) * 2.0 ** rng.integers(-30, 30, (27, cin, cout))).astype(np.float32)
    planes = dcl.ops.conv_split_weight(cuda(w))
    assert planes.numel() == 27 * cin * cout * 6
    back = dcl.ops.conv_split_planes(planes, cin, cout).cpu()
    assert torch.equal(back.double().sum(0), torch.from_numpy(w).double())
    model = CS.model_planes(w).to(torch.bfloat16).contiguous().view(torch.uint8).reshape(-1)
    assert torch.equal(planes.cpu(), model)                                   # bit for bit the host model's layout and split


# ------------------------------------------------------------------------------------------------------- exact operands
@pytest.mark.parametrize("cin,cout,subm", CS.WIDTHS)
@pytest.mark.parametrize("kind", ["hh", "x3", "w3", "mm"])
def test_exact_operands_split_equals_fp32_bit_for_bit(dcl, cin, cout, subm, kind):
    """one crop of 129 rows (one tile plus one row) and two crops of 333: few-row launches, stream-K with the deferred combine"""
    for b, n_per in ((1, 129), (2, 333)):
        dev, host, _ = _side(dcl, b, n_per, cin, cout, subm, kind, 7 + b)
        if subm:
            assert dev[3] == b * n_per and dev[3] % 128 != 0
        (fp32,), (split,) = _both(dcl, [dev], subm)
        val, _ = CS.reference64(*host)
        assert torch.equal(fp32.cpu().double(), val), "the operands are not exact for the fp32 form"
        assert torch.equal(split, fp32), (b, float((split - fp32).abs().max()))


@pytest.mark.parametrize("cin,cout,subm", [(32, 64, True), (128, 256, True), (128, 128, False)])
def test_exact_operands_both_backbones_in_one_launch_with_epilogue(dcl, cin, cout, subm):
    """two problems of different sizes and filters in one launch, folded BatchNorm + ReLU epilogue"""
    a, _, _ = _side(dcl, 1, 129, cin, cout, subm, "mm", 11)
    b_, _, _ = _side(dcl, 2, 333, cin, cout, subm, "x3", 12)
    rng = np.random.default_rng(1)
    sc = [cuda((2.0 ** rng.integers(-1, 2, cout)).astype(np.float32)) for _ in range(2)]
    sh = [cuda(rng.integers(-4, 5, cout).astype(np.float32)) for _ in range(2)]
    fp32, split = _both(dcl, [a, b_], subm, scales=sc, shifts=sh, relu=True)
    plain, _ = _both(dcl, [a, b_], subm)
    for i in range(2):
        assert torch.equal(split[i], fp32[i]), i
        assert torch.equal(fp32[i], torch.relu(plain[i] * sc[i] + sh[i])), i
        assert float(split[i].abs().max()) > 0


@pytest.mark.parametrize("cin,cout,subm", [(32, 64, True), (64, 128, True)])
def test_exact_operands_ordered_rows_beyond_the_few_row_launches(dcl, cin, cout, subm):
    """8 crops of 800 rows (6400: past the few-row launches, which take no order): natural order by the cost model's
    decomposition, and the runner's row order with used-chunk dealing -- stream-K, partial tiles combined inside the launch by
    the last arriver.  The same bits as the fp32 form and as float64 either way."""
    dev, host, (oset, in_mask) = _side(dcl, 8, 800, cin, cout, subm, "mm", 21)
    assert dev[3] == 6400
    val, _ = CS.reference64(*host)
    (fp32,), (split,) = _both(dcl, [dev], subm)
    assert torch.equal(fp32.cpu().double(), val) and torch.equal(split, fp32)
    order = dcl.ops.order_rows(oset, in_mask, subm)
    (fp32_o,), (split_o,) = _both(dcl, [dev], subm, orders=[order])
    assert torch.equal(fp32_o.cpu().double(), val) and torch.equal(split_o, fp32_o)


@pytest.mark.parametrize("cin,cout,subm", [(64, 128, True), (128, 256, True), (64, 64, False)])
def test_exact_operands_forced_split_k(request, dcl, cin, cout, subm):
    """aligned split-K forced through the diagnostic library's hook: partial tiles published and combined inside the launch (ticket
    per tile), the same bits as the fp32 form, and reproducible back to back (the tickets are left at zero)"""
    dev, host, _ = _side(dcl, 2, 333, cin, cout, subm, "mm", 21)
    val, _ = CS.reference64(*host)
    lib = enter_diag(dcl, request)
    try:
        for ns in (2, 5):
            lib.dcl_debug_conv_split(ns)
            (fp32,), (split,) = _both(dcl, [dev], subm)
            assert torch.equal(fp32.cpu().double(), val) and torch.equal(split, fp32), ns
            again = [_both(dcl, [dev], subm)[1][0] for _ in range(4)]                  # the tickets are left at zero
            assert all(torch.equal(a, split) for a in again), ns
    finally:
        lib.dcl_debug_conv_split(0)


# -------------------------------------------------------------------------------------------------- error against float64
@pytest.mark.parametrize("cin,cout,subm", [(32, 64, True), (64, 128, True), (128, 256, True), (128, 128, False)])
@pytest.mark.parametrize("kind", ["gauss", "cancel", "range"])
def test_error_against_float64_within_one_and_a_half_of_the_fp32_kernel(dcl, cin, cout, subm, kind):
    dev, host, _ = _side(dcl, 2, 333, cin, cout, subm, kind, 31, exact=False)
    val, mag = CS.reference64(*host)
    (fp32,), (split,) = _both(dcl, [dev], subm)
    assert bool(torch.isfinite(split).all())
    u_fp32 = float(CS.units(fp32.cpu(), val, mag).max())
    u_split = float(CS.units(split.cpu(), val, mag).max())
    print("conv split error units: %d->%d subm=%d %-6s fp32 %.3f split %.3f ratio %.3f"
          % (cin, cout, subm, kind, u_fp32, u_split, u_split / u_fp32))
    assert u_fp32 > 0
    assert u_split <= 1.5 * u_fp32, (u_split, u_fp32)


# ------------------------------------------------------------------------------------------------------ non-finite values
def test_non_finite_values_poison_only_the_outputs_that_read_them(dcl):
    cin, cout, subm = 64, 128, True
    dev, host, _ = _side(dcl, 2, 333, cin, cout, subm, "gauss", 41, exact=False)
    x, w, nbr, n_out = dev
    nbr_h = host[2]
    (_,), (clean,) = _both(dcl, [dev], subm)
    # an inf / NaN feature row: the outputs that gather it are poisoned, every other output keeps its bits
    for bad_row, value in ((5, float("inf")), (n_out - 1, float("nan"))):
        xb = x.clone()
        xb[bad_row, 3] = value
        (_,), (got,) = _both(dcl, [(xb, w, nbr, n_out)], subm)
        readers = torch.from_numpy((nbr_h[:, :n_out] == bad_row).any(0))
        assert int(readers.sum()) >= 1 and not bool(readers.all())
        assert not bool(torch.isfinite(got.cpu()[readers]).all(1).any())
        assert torch.equal(got.cpu()[~readers], clean.cpu()[~readers])
    # an inf / NaN filter column (under the centre offset, which every row has): that output column is poisoned, the others keep their bits
    for col, value in ((0, float("nan")), (cout - 1, float("-inf"))):
        wb = w.clone()
        wb[13, 7, col] = value
        (_,), (got,) = _both(dcl, [(x, wb, nbr, n_out)], subm)
        keep = torch.ones(cout, dtype=torch.bool)
        keep[col] = False
        assert not bool(torch.isfinite(got.cpu()[:, col]).any())
        assert torch.equal(got.cpu()[:, keep], clean.cpu()[:, keep])


# ------------------------------------------------------------------------------------------------ whole-network agreement
def _forward(dcl, graph_max_batch, b=2, n=256):
    cfg = dcl.synth.default_cfg(n, n)
    net = dcl.DCL_Net.Network(cfg, mode="test", graph_max_batch=graph_max_batch)
    net.load_state_dict(dcl.synth.synth_state_dict(net, 1))
    net = net.cuda().eval()
    with torch.no_grad():
        pred = net(dcl.synth.make_batch(b, n, n))
    torch.cuda.synchronize()
    return {k: pred[k].clone() for k in ("rot_pred", "trans_pred", "conf")}


def test_whole_network_agrees_with_the_switch_off_and_graph_replay_with_launch_by_launch(dcl, monkeypatch):
    """every width the split kernel takes, from the first row on (the product's table keeps few-row launches on fp32): the forward
    with ops.CONV_SPLIT on against the forward with it off within the goldens' tolerances (1e-4 / 1e-5); graph replay and launch
    by launch take the same forms (the table goes by crops, not by live rows) and agree with each other as they do with the
    switch off -- bit for bit where they do so there"""
    ops = dcl.ops
    monkeypatch.setattr(ops, "CONV_SPLIT_WIDTHS", {w: 0 for w in CS.WIDTHS})
    res = {}
    for on in (False, True):
        monkeypatch.setattr(ops, "CONV_SPLIT", on)
        res[on, "eager"] = _forward(dcl, 0)
        res[on, "graph"] = _forward(dcl, 8)
    for path in ("eager", "graph"):
        assert float((res[True, path]["rot_pred"] - res[False, path]["rot_pred"]).abs().max()) <= 1e-4
        assert float((res[True, path]["trans_pred"] - res[False, path]["trans_pred"]).abs().max()) <= 1e-5
        assert float((res[True, path]["conf"] - res[False, path]["conf"]).abs().max()) <= 1e-4
    assert not all(torch.equal(res[True, "eager"][k], res[False, "eager"][k]) for k in res[True, "eager"]), "the split form did not run"
    for on in (False, True):
        assert float((res[on, "graph"]["rot_pred"] - res[on, "eager"]["rot_pred"]).abs().max()) <= 1e-4
        assert float((res[on, "graph"]["trans_pred"] - res[on, "eager"]["trans_pred"]).abs().max()) <= 1e-5
    same_off = all(torch.equal(res[False, "graph"][k], res[False, "eager"][k]) for k in res[False, "eager"])
    same_on = all(torch.equal(res[True, "graph"][k], res[True, "eager"][k]) for k in res[True, "eager"])
    assert same_on or not same_off
