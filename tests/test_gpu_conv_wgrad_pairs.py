"""ops.conv_pairs and ops.sparse_conv_wgrad_pairs (csrc/conv_wgrad_pairs.hip) on the GPU: the device pair list against its host
twin, the weight gradient against the integer gradient (exact operands, bit for bit) and against float64 within the bound its
pinned order gives, its invariances, and the wgrad="pairs" switch from autograd.SparseConvFn up to Network.

The bound: an element of a split's result is one chain of at most S = DCL_CONV_PAIRS_SPLIT fused steps from +0, and an offset's
splits_k = ceil(count_k / S) results are added one rounded add each, so |dW - exact| <= (S + splits_k + 2) 2^-24 sum |x| |g|,
element by element, as derived for linear_wgrad (include/dclnet_hip.h).  Worst ratio error / bound measured on an MI355X: see
DESIGN.md section 9."""
import numpy as np
import pytest
import torch

import conv_grad_cases as cg
import conv_pairs_cases as pc
from test_gpu_ops import cuda

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
WIDTHS = tuple((ci, co) for ci, co, _ in cg.BACKBONE) + ((5, 4), (33, 65))
DEVICE_CASES = (tuple((s, ci, co, True) for s in ("edge2049", "edge2055") for ci, co in ((16, 32), (32, 64), (64, 64)))
                + (("few5000", 128, 256, True), ("stride2", 32, 32, False), ("mid", 32, 32, False)))


def _S(dcl):
    return dcl.ops.CONV_PAIRS_SPLIT


def _list_np(P):
    return dict(head=P.head.cpu().numpy(), pair_in=P.pair_in.cpu().numpy(), pair_out=P.pair_out.cpu().numpy(),
                split_tab=P.split_tab.cpu().numpy())


_SYN = {}


def _synthetic(dcl):
    """the synthetic rulebook on the device, as it is (for "pairs") and with every non-pair as -1 (for "rows", which takes any
    entry >= 0 for a row), and its pairs in the layout of conv_grad_cases.conv_backward_ref"""
    if not _SYN:
        nbr, counts = pc.synthetic_nbr(_S(dcl))
        clean = np.where((nbr >= 0) & (nbr < pc.N_IN), nbr, -1).astype(np.int32)
        pairs, num = pc.oracle_style_pairs(nbr, pc.N_OUT, pc.N_IN)
        _SYN.update(nbr=nbr, dev=cuda(nbr), rows=cuda(clean), counts=counts, pairs=pairs, num=num)
    return _SYN


_RULEBOOKS = {}


def _rulebook(dcl, geo, subm):
    key = id(geo)
    if key not in _RULEBOOKS:
        aset = dcl.ops.grid_from_indices(cuda(geo["idx"]), geo["b"], geo["S"])
        out, nbr = dcl.spconv.ops.build_rulebook(aset, 3, geo["stride"], geo["padding"], subm)
        n_out = geo["n_in"] if subm else out.n
        assert n_out == geo["n_out"]
        _RULEBOOKS[key] = (nbr, n_out, geo)
    return _RULEBOOKS[key][:2]


def _where(got, want):
    bad = np.argwhere(got != want)
    if bad.size == 0:
        return ""
    return "%d of %d elements differ; offsets %s (first: index %s got %r want %r)" % (
        bad.shape[0], got.size, np.unique(bad[:, 0])[:12].tolist(), bad[0].tolist(), float(got[tuple(bad[0])]),
        float(want[tuple(bad[0])]))


# ------------------------------------------------------------------------------------------- 1. the pair list
def test_device_list_equals_the_host_twin_on_the_synthetic_rulebook(dcl):
    syn = _synthetic(dcl)
    P = dcl.ops.conv_pairs(syn["dev"], pc.N_OUT, pc.N_IN, check=True)
    want = dcl.ops.conv_pairs_host(syn["nbr"], pc.N_OUT, pc.N_IN)
    assert (P.max_pairs, P.max_splits) == (want["max_pairs"], want["max_splits"]) == (27 * pc.N_IN, 27 * pc.N_IN // _S(dcl) + 27)
    assert pc.same_list(_list_np(P), want) == ""
    count, start, nsplit, overflow = P.counts()
    assert count.tolist() == syn["counts"] and overflow == 0 and nsplit == sum(-(-c // _S(dcl)) for c in syn["counts"])
    again = dcl.ops.conv_pairs(syn["dev"], pc.N_OUT, pc.N_IN)
    assert pc.same_list(_list_np(again), _list_np(P)) == ""


@pytest.mark.parametrize("shape,subm", [("edge2055", True), ("stride2", False)])
def test_device_list_equals_the_host_twin_on_device_rulebooks(dcl, oracle, shape, subm):
    geo = cg.geometry(oracle, shape, subm)
    nbr, n_out = _rulebook(dcl, geo, subm)
    P = dcl.ops.conv_pairs(nbr, n_out, geo["n_in"], check=True)
    want = dcl.ops.conv_pairs_host(nbr.cpu().numpy(), n_out, geo["n_in"])
    assert pc.same_list(_list_np(P), want) == ""
    count = P.counts()[0].numpy()
    assert np.array_equal(count, geo["num"])                                    # the oracle's rulebook holds as many pairs
    # ... and the same ones: per offset the same (in, out) set
    h = want["head"]
    for k in (0, 13, 26):
        lo, hi = h[pc.HEAD_START + k], h[pc.HEAD_START + k + 1]
        mine = set(zip(want["pair_in"][lo:hi].tolist(), want["pair_out"][lo:hi].tolist()))
        assert mine == set(zip(geo["pairs"][k, 0, :hi - lo].tolist(), geo["pairs"][k, 1, :hi - lo].tolist()))


def test_pairs_beyond_the_bound_are_counted_and_check_raises(dcl):
    """an input row that meets an offset more than once breaks the sizing rule: nothing past max_pairs is stored, the device word
    says how many are missing, and check=True raises"""
    nbr = np.zeros((27, 8), np.int32)                                           # every output row names input row 0
    nbr[:, 5] = 1
    P = dcl.ops.conv_pairs(cuda(nbr), 8, 2)
    assert P.max_pairs == 54
    want = dcl.ops.conv_pairs_host(nbr, 8, 2)
    assert pc.same_list(_list_np(P), want) == ""
    assert P.counts()[3] == 27 * 8 - 54 and P.counts()[0].tolist() == [8] * 27
    with pytest.raises(RuntimeError):
        dcl.ops.conv_pairs(cuda(nbr), 8, 2, check=True)


# ------------------------------------------------------------------------------------------- 2. exact operands
@pytest.mark.parametrize("cin,cout", WIDTHS)
def test_exact_operands_give_the_integer_gradient_on_the_synthetic_rulebook(dcl, cin, cout):
    syn = _synthetic(dcl)
    X, W, G = cg.exact_operands(("synthetic",), pc.N_IN, pc.N_OUT, cin, cout)
    _, want = cg.conv_backward_ref(X, W, G, syn["pairs"], syn["num"])
    assert np.abs(want).max() < cg.EXACT_LIMIT
    want = want.astype(np.float32)
    f, w, g = cuda(X), cuda(W), cuda(G)
    P = dcl.ops.conv_pairs(syn["dev"], pc.N_OUT, pc.N_IN)
    dw = dcl.ops.sparse_conv_wgrad_pairs(f, g, P, cin, cout)
    assert _where(dw.cpu().numpy(), want) == ""
    for k, c in enumerate(syn["counts"]):                                       # an offset without pairs: +0, written
        if c == 0:
            assert not dw[k].any() and not torch.signbit(dw[k]).any()
    _, dw_op = dcl.ops.sparse_conv_backward(f, w, g, syn["dev"], pc.N_OUT, False, need_dx=False, wgrad="pairs")
    assert torch.equal(dw_op, dw)
    _, dw_rows = dcl.ops.sparse_conv_backward(f, w, g, syn["rows"], pc.N_OUT, False, need_dx=False)
    assert torch.equal(dw_rows, dw)


@pytest.mark.parametrize("case", DEVICE_CASES, ids=cg.case_id)
def test_exact_operands_give_the_integer_gradient_on_device_rulebooks(dcl, oracle, case):
    c = cg.conv_case(oracle, case, "exact")
    nbr, n_out = _rulebook(dcl, c["geo"], case[3])
    f, w, g = cuda(c["X"]), cuda(c["W"]), cuda(c["G"])
    _, dw = dcl.ops.sparse_conv_backward(f, w, g, nbr, n_out, case[3], need_dx=False, wgrad="pairs")
    assert _where(dw.cpu().numpy(), c["dW"].astype(np.float32)) == ""
    _, dw_rows = dcl.ops.sparse_conv_backward(f, w, g, nbr, n_out, case[3], need_dx=False, wgrad="rows")
    assert torch.equal(dw_rows, dw)
    if case[0] == "mid":                                                        # the training-size case
        pairs, nsplit = int(c["geo"]["num"].sum()), dcl.ops.conv_pairs(nbr, n_out, c["geo"]["n_in"]).counts()[2]
        print("mid: %d pairs in %d splits" % (pairs, nsplit))
        assert pairs > 600000 and nsplit > 1000


def test_empty_sides_give_a_written_zero_gradient(dcl):
    """no output rows, no input rows, or a table without a pair: every element of dW is written, +0"""
    cin, cout = 32, 64
    W = cuda(cg.exact_array(np.random.default_rng(0), (27, cin, cout)))
    f = cuda(cg.exact_array(np.random.default_rng(1), (5, cin)))
    g = cuda(cg.exact_array(np.random.default_rng(2), (7, cout)))
    none1 = torch.full((27, 1), -1, dtype=torch.int32, device="cuda")
    none7 = torch.full((27, 7), -1, dtype=torch.int32, device="cuda")
    for feat, dout, nbr, n_out in ((f, torch.zeros((0, cout), device="cuda"), none1, 0),
                                   (torch.zeros((0, cin), device="cuda"), g, none7, 7), (f, g, none7, 7)):
        dx, dw = dcl.ops.sparse_conv_backward(feat, W, dout, nbr, n_out, False, wgrad="pairs")
        assert dw.shape == (27, cin, cout) and not dw.any() and not torch.signbit(dw).any()
        assert dx.shape == (feat.shape[0], cin) and not dx.any()
        assert dcl.ops.conv_pairs(nbr, n_out, feat.shape[0], check=True).counts()[2:] == (0, 0)


# ------------------------------------------------------------------------------------------- 3. gaussian operands
def _bound_check(dcl, tag, dw, X, W, G, pairs, num):
    S = _S(dcl)
    _, want = cg.conv_backward_ref(X, W, G, pairs, num)
    _, mag = cg.conv_backward_ref(np.abs(X), np.abs(W), np.abs(G), pairs, num)
    splits = -(-np.asarray(num, np.int64) // S)
    bound = (S + splits + 2)[:, None, None] * U * mag
    err = np.abs(dw.cpu().numpy().astype(np.float64) - want)
    ratio = float((err / np.maximum(bound, 1e-300))[mag > 0].max())
    print("wgrad pairs %s: max error / bound = %.3g (max |dW| %.3g)" % (tag, ratio, float(np.abs(want).max())))
    assert np.all(err <= bound)
    assert np.abs(want).max() > 1.0


@pytest.mark.parametrize("cin,cout", [(7, 16), (32, 64), (128, 256)])
def test_gaussian_operands_within_the_pinned_orders_bound_on_the_synthetic_rulebook(dcl, cin, cout):
    syn = _synthetic(dcl)
    X, W, G = cg.gaussian_operands(("synthetic",), pc.N_IN, pc.N_OUT, cin, cout)
    P = dcl.ops.conv_pairs(syn["dev"], pc.N_OUT, pc.N_IN)
    dw = dcl.ops.sparse_conv_wgrad_pairs(cuda(X), cuda(G), P, cin, cout)
    _bound_check(dcl, "synthetic %d -> %d" % (cin, cout), dw, X, W, G, syn["pairs"], syn["num"])


@pytest.mark.parametrize("cin,cout", [(16, 32), (64, 64)])
def test_gaussian_operands_within_the_pinned_orders_bound_on_edge2055(dcl, oracle, cin, cout):
    case = ("edge2055", cin, cout, True)
    c = cg.conv_case(oracle, case, "gaussian")
    nbr, n_out = _rulebook(dcl, c["geo"], True)
    _, dw = dcl.ops.sparse_conv_backward(cuda(c["X"]), cuda(c["W"]), cuda(c["G"]), nbr, n_out, True, need_dx=False, wgrad="pairs")
    _bound_check(dcl, cg.case_id(case), dw, c["X"], c["W"], c["G"], c["geo"]["pairs"], c["geo"]["num"])


# ------------------------------------------------------------------------------------------- 4. invariance
@pytest.mark.parametrize("cin,cout", [(7, 16), (64, 128)])
def test_same_bits_again_for_any_cap_and_whatever_the_unnamed_rows_hold(dcl, cin, cout):
    syn = _synthetic(dcl)
    nbr = syn["nbr"]
    X, _, G = cg.gaussian_operands(("synthetic", "invariance"), pc.N_IN, pc.N_OUT, cin, cout)
    f, g = cuda(X), cuda(G)

    def run(table, n_out, feat, dout):
        return dcl.ops.sparse_conv_wgrad_pairs(feat, dout, dcl.ops.conv_pairs(cuda(table), n_out, pc.N_IN, check=True), cin, cout)

    first = run(nbr, pc.N_OUT, f, g)
    assert torch.isfinite(first).all() and float(first.abs().max()) > 1.0
    assert torch.equal(run(nbr, pc.N_OUT, f, g), first)                         # a second call
    rng = np.random.default_rng(3)
    wide = rng.integers(0, pc.N_IN, size=(27, pc.CAP + 123)).astype(np.int32)   # a larger cap, valid-looking junk behind it
    wide[:, :pc.N_OUT] = nbr[:, :pc.N_OUT]
    assert torch.equal(run(wide, pc.N_OUT, f, g), first)
    # all-empty output rows interleaved: output row o moves to 2 o + 1, the rows between hold no pair and a NaN gradient
    gaps = rng.integers(0, pc.N_IN, size=(27, 2 * pc.CAP)).astype(np.int32)
    gaps[:, 0:2 * pc.N_OUT:2] = np.array(pc.NOT_A_PAIR, np.int64)[rng.integers(0, 4, size=(27, pc.N_OUT))].astype(np.int32)
    gaps[:, 1:2 * pc.N_OUT:2] = nbr[:, :pc.N_OUT]
    G2 = np.full((2 * pc.N_OUT, cout), np.nan, np.float32)
    G2[1::2] = G
    assert torch.equal(run(gaps, 2 * pc.N_OUT, f, cuda(G2)), first)
    # NaN in every X row that no pair names: the rows behind n_in (which the table's non-pairs point at) and any below it
    named = np.zeros(pc.N_IN + 100, bool)
    for k in range(27):
        named[syn["pairs"][k, 0, :syn["num"][k]]] = True
    X2 = np.full((pc.N_IN + 100, cin), np.nan, np.float32)
    X2[:pc.N_IN][named[:pc.N_IN]] = X[named[:pc.N_IN]]
    assert int((~named).sum()) >= 100 and np.isnan(X2[pc.N_IN]).all()
    assert torch.equal(run(nbr, pc.N_OUT, cuda(X2), g), first)


# ------------------------------------------------------------------------------------------- 5. autograd
def test_autograd_function_takes_the_form_and_keeps_its_five_argument_call(dcl, oracle):
    case = ("edge2055", 16, 32, True)
    c = cg.conv_case(oracle, case, "gaussian")
    nbr, n_out = _rulebook(dcl, c["geo"], True)
    f, w, g = cuda(c["X"]), cuda(c["W"]), cuda(c["G"])
    grads = {}
    for form, args in (("pairs", ("pairs",)), ("rows", ("rows",)), ("five", ())):
        fa, wa = f.clone().requires_grad_(True), w.clone().requires_grad_(True)
        dcl.autograd.SparseConvFn.apply(fa, wa, nbr, n_out, True, *args).backward(g)
        grads[form] = (fa.grad, wa.grad)
    _, dw = dcl.ops.sparse_conv_backward(f, w, g, nbr, n_out, True, need_dx=False, wgrad="pairs")
    assert torch.equal(grads["pairs"][1], dw)
    assert torch.equal(grads["pairs"][0], grads["rows"][0])                     # the dX route is untouched
    assert torch.equal(grads["five"][0], grads["rows"][0]) and torch.equal(grads["five"][1], grads["rows"][1])
    with pytest.raises(ValueError):
        dcl.autograd.SparseConvFn.apply(f, w, nbr, n_out, True, "nope")


# ------------------------------------------------------------------------------------------- 6. the network
def test_network_step_with_pairs_changes_the_conv_weight_gradients_only(dcl):
    b, n = 2, 256
    data = dcl.synth.make_batch(b, n, n)
    data["flags"] = torch.tensor([0.0, 1.0])
    crit = dcl.DCL_Net.losses(None)

    def step(form):
        net = dcl.DCL_Net.Network(dcl.synth.default_cfg(n, n), mode="train", train_conv_wgrad=form)
        net.load_state_dict(dcl.synth.synth_state_dict(net, 1))
        net = net.cuda().train()
        loss = crit(net(data), data["labels"])["loss_all"]
        loss.backward()
        torch.cuda.synchronize()
        conv_w = {id(m.weight) for m in net.modules() if isinstance(m, dcl.spconv.SparseConvolution)}
        named = {k: p for k, p in net.named_parameters() if p.grad is not None}
        return (loss.detach().clone(), {k: p.grad.clone() for k, p in named.items() if id(p) not in conv_w},
                {k: p.grad.clone() for k, p in named.items() if id(p) in conv_w})

    loss_r, other_r, conv_r = step("rows")
    loss_p, other_p, conv_p = step("pairs")
    loss_q, other_q, conv_q = step("pairs")
    assert len(conv_r) == len(conv_p) == 16 and len(other_r) > 50 and other_r.keys() == other_p.keys()
    assert torch.equal(loss_p, loss_r) and torch.isfinite(loss_r)
    for k in other_r:
        assert torch.equal(other_p[k], other_r[k]), k
    for k in conv_r:
        assert torch.equal(conv_p[k], conv_q[k]), k
        assert torch.isfinite(conv_p[k]).all() and float(conv_p[k].abs().max()) > 0, k
