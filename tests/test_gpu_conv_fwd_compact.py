"""ops.sparse_conv(form="compact") (csrc/conv_fwd_compact.hip) on the GPU: the kernel against its host twin BIT FOR BIT on Gaussian
operands -- which carries the float64 bound of tests/test_conv_fwd_compact_abi.py over to the kernel without a tolerance of its
own --, against the integer result and the "tiles" form on exact operands, what it writes and what it leaves alone, and the
forward switch from ops.sparse_conv through autograd.SparseConvFn and the spconv modules up to Network."""
import numpy as np
import pytest
import torch

import conv_fwd_cases as fc
import conv_grad_cases as cg
from test_gpu_ops import cuda

pytestmark = pytest.mark.gpu

_RULEBOOKS = {}


def _rulebook(dcl, oracle, case):
    """the device rulebook of a case's geometry: (nbr, n_out)"""
    key = (case[0], case[3])
    if key not in _RULEBOOKS:
        geo = cg.geometry(oracle, case[0], case[3])
        aset = dcl.ops.grid_from_indices(cuda(geo["idx"]), geo["b"], geo["S"])
        out, nbr = dcl.spconv.ops.build_rulebook(aset, 3, geo["stride"], geo["padding"], case[3])
        n_out = geo["n_in"] if case[3] else out.n
        assert n_out == geo["n_out"] and nbr.shape[1] >= n_out
        # the device rulebook names the same neighbours as the oracle's pair lists
        dev, want = nbr[:, :n_out].cpu().numpy(), fc.forward_table(geo)
        assert np.array_equal((dev >= 0) & (dev < geo["n_in"]), want >= 0) and np.array_equal(dev[want >= 0], want[want >= 0])
        _RULEBOOKS[key] = (nbr, n_out)
    return _RULEBOOKS[key]


def _where(got, want):
    bad = np.argwhere(got != want)
    if bad.size == 0:
        return ""
    return "%d of %d elements differ; rows %s (first: index %s got %r want %r)" % (
        bad.shape[0], got.size, np.unique(bad[:, 0])[:12].tolist(), bad[0].tolist(), float(got[tuple(bad[0])]),
        float(want[tuple(bad[0])]))


def _compact(dcl, f, nbr, n_out, w, subm):
    return dcl.ops.sparse_conv(f, nbr, n_out, w, subm, form="compact")


# ------------------------------------------------------------------------------------------- 1. kernel = host twin
@pytest.mark.parametrize("case", fc.CASES, ids=cg.case_id)
def test_kernel_equals_the_host_twin_bit_for_bit_on_gaussian_operands(dcl, oracle, case):
    c = cg.conv_case(oracle, case, "gaussian")
    nbr, n_out = _rulebook(dcl, oracle, case)
    got = _compact(dcl, cuda(c["X"]), nbr, n_out, cuda(c["W"]), case[3])
    want = fc.twin(dcl, oracle, case, "gaussian")
    assert got.shape == want.shape and float(np.abs(want).max()) > 0.1
    assert _where(got.cpu().numpy(), want) == ""


# ------------------------------------------------------------------------------------------- 2. the hand-made table
@pytest.mark.parametrize("subm", [False, True], ids=["conv", "subm"])
@pytest.mark.parametrize("cin,cout", fc.WIDTHS)
def test_kernel_equals_the_host_twin_on_the_hand_made_table(dcl, cin, cout, subm):
    X, W = fc.hand_operands(cin, cout, exact=False)
    want = dcl.ops.sparse_conv_compact_host(X, fc.HAND_NBR, fc.HAND_N_OUT, W, subm, n_in=fc.HAND_N_IN)
    # the kernel takes n_in from the rows it is given: the NaN rows lie behind the tensor it sees, in the same allocation
    x, w = cuda(X), cuda(W)
    got = _compact(dcl, x[:fc.HAND_N_IN], cuda(fc.HAND_NBR), fc.HAND_N_OUT, w, subm)
    assert torch.isfinite(got).all()
    assert _where(got.cpu().numpy(), want) == ""
    assert not got[fc.HAND_EMPTY].any() and not torch.signbit(got[fc.HAND_EMPTY]).any()
    # the same table inside a wider one with junk behind the n_out rows; guard rows behind out[:n_out] keep their fill
    wide = cuda(fc.hand_embedded(203, np.random.default_rng(cin)))
    buf = torch.full((fc.HAND_N_OUT + 67, cout), float("nan"), dtype=torch.float32, device="cuda")
    vp = dcl._native.vp
    dcl._native.check(dcl._native.lib().dcl_sparse_conv_fwd_compact(
        vp(x.data_ptr()), fc.HAND_N_IN, vp(wide.data_ptr()), wide.shape[1], fc.HAND_N_OUT, vp(w.data_ptr()), cin, cout, 27,
        int(subm), vp(buf.data_ptr()), dcl._native.stream()), "sparse_conv_fwd_compact")
    assert torch.equal(buf[:fc.HAND_N_OUT], got)
    assert torch.isnan(buf[fc.HAND_N_OUT:]).all()


# ------------------------------------------------------------------------------------------- 3. exact operands
@pytest.mark.parametrize("case", fc.CASES, ids=cg.case_id)
def test_exact_operands_give_the_integer_result_and_the_tiles_forms_bits(dcl, oracle, case):
    c = cg.conv_case(oracle, case, "exact")
    nbr, n_out = _rulebook(dcl, oracle, case)
    f, w = cuda(c["X"]), cuda(c["W"])
    got = _compact(dcl, f, nbr, n_out, w, case[3])
    assert _where(got.cpu().numpy(), fc.ref(oracle, case, "exact").astype(np.float32)) == ""
    assert torch.equal(dcl.ops.sparse_conv(f, nbr, n_out, w, case[3], form="tiles"), got)


# ------------------------------------------------------------------------------------------- 4. repeatability and alignment
@pytest.mark.parametrize("case", [("tail100", 16, 32, True), ("edge2049", 33, 40, False), ("two1500", 128, 256, True),
                                  ("stride2s", 64, 64, False), ("two1500", 32, 32, False), ("edge2049", 128, 128, False)],
                         ids=cg.case_id)
def test_the_same_bits_again_and_from_operands_off_a_16_byte_boundary(dcl, oracle, case):
    c = cg.conv_case(oracle, case, "gaussian")
    nbr, n_out = _rulebook(dcl, oracle, case)
    f, w = cuda(c["X"]), cuda(c["W"])
    a, b = _compact(dcl, f, nbr, n_out, w, case[3]), _compact(dcl, f, nbr, n_out, w, case[3])
    assert torch.equal(a, b)

    def off4(t):                                                                 # the same values, 4 bytes off the allocation's start
        buf = torch.empty(t.numel() + 1, dtype=torch.float32, device="cuda")
        v = buf[1:].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return v

    assert f.data_ptr() % 16 == 0 and w.data_ptr() % 16 == 0
    assert torch.equal(_compact(dcl, off4(f), nbr, n_out, off4(w), case[3]), a)
    assert _where(a.cpu().numpy(), fc.twin(dcl, oracle, case, "gaussian")) == ""


# ------------------------------------------------------------------------------------------- 5. empty input
def test_empty_sides(dcl):
    W = cuda(cg.exact_array(np.random.default_rng(0), (27, 32, 64)))
    nbr = torch.full((27, 5), -1, dtype=torch.int32, device="cuda")
    f = torch.ones((3, 32), device="cuda")
    assert _compact(dcl, f, nbr, 0, W, False).shape == (0, 64)                   # no output rows
    out = _compact(dcl, f, nbr, 5, W, False)                                     # an all-absent rulebook: written zeros
    assert out.shape == (5, 64) and not out.any() and not torch.signbit(out).any()
    out = _compact(dcl, torch.zeros((0, 32), device="cuda"), torch.zeros_like(nbr), 5, W, True)       # no input rows
    assert out.shape == (5, 64) and not out.any() and not torch.signbit(out).any()


# ------------------------------------------------------------------------------------------- 6. the op-level switch
def test_op_level_switch(dcl, oracle):
    case = ("tail100", 32, 32, False)
    c = cg.conv_case(oracle, case, "gaussian")
    nbr, n_out = _rulebook(dcl, oracle, case)
    f, w = cuda(c["X"]), cuda(c["W"])
    one = torch.ones(32, device="cuda")
    for kw in (dict(scale=one, shift=one), dict(scale=one), dict(relu=True),
               dict(order=(torch.arange(n_out, dtype=torch.int32, device="cuda"),) * 3)):
        with pytest.raises(ValueError):
            dcl.ops.sparse_conv(f, nbr, n_out, w, False, form="compact", **kw)
    with pytest.raises(ValueError):
        dcl.ops.sparse_conv(f, nbr, n_out, w, False, form="pairs")
    assert torch.equal(dcl.ops.sparse_conv(f, nbr, n_out, w, False, form="tiles"), dcl.ops.sparse_conv(f, nbr, n_out, w, False))
    assert torch.equal(dcl.ops.sparse_conv(f, nbr, n_out, w, False, relu=True, form="tiles"),
                       dcl.ops.sparse_conv(f, nbr, n_out, w, False, relu=True))


# ------------------------------------------------------------------------------------------- 7. autograd and modules
def test_autograd_function_takes_the_form_and_keeps_its_shorter_calls(dcl, oracle):
    case = ("edge2049", 32, 32, False)
    c = cg.conv_case(oracle, case, "gaussian")
    nbr, n_out = _rulebook(dcl, oracle, case)
    f, w, g = cuda(c["X"]), cuda(c["W"]), cuda(c["G"])
    outs, grads = {}, {}
    for form, args in (("compact", ("rows", "conv", "compact")), ("tiles", ("rows", "conv", "tiles")), ("seven", ("rows", "conv")),
                       ("six", ("rows",)), ("five", ())):
        fa, wa = f.clone().requires_grad_(True), w.clone().requires_grad_(True)
        outs[form] = dcl.autograd.SparseConvFn.apply(fa, wa, nbr, n_out, False, *args)
        outs[form].backward(g)
        grads[form] = (fa.grad, wa.grad)
    assert _where(outs["compact"].detach().cpu().numpy(), fc.twin(dcl, oracle, case, "gaussian")) == ""
    for form in ("seven", "six", "five"):
        assert torch.equal(outs[form], outs["tiles"])
    for form in ("compact", "seven", "six", "five"):                             # the backward does not depend on the forward's form
        assert torch.equal(grads[form][0], grads["tiles"][0]) and torch.equal(grads[form][1], grads["tiles"][1])
    with pytest.raises(ValueError):
        dcl.autograd.SparseConvFn.apply(f, w, nbr, n_out, False, "rows", "conv", "nope")


def test_spconv_modules_with_compact_give_the_tiles_results_on_exact_operands(dcl, oracle):
    """SparseConv3d 16 -> 32 followed by SubMConv3d 32 -> 32: with exact operands every sum is an integer (|out1| <= 27 * 16 * 4,
    |out2| <= 27 * 32 * 2 * 1728 < 2^24), so both forms must give the same bits, forward and backward"""
    geo = cg.geometry(oracle, "two1500", False)
    rng = np.random.default_rng(77)
    X = cg.exact_array(rng, (geo["n_in"], 16))
    W1, W2 = cg.exact_array(rng, (27, 16, 32)), cg.exact_array(rng, (27, 32, 32))
    G = cg.exact_array(rng, (geo["n_out"], 32))
    res = {}
    for form in ("tiles", "compact"):
        m1 = dcl.spconv.SparseConv3d(16, 32, 3, padding=1, bias=False).cuda()
        m2 = dcl.spconv.SubMConv3d(32, 32, 3, padding=1, bias=False).cuda()
        with torch.no_grad():
            m1.weight.copy_(cuda(W1).view_as(m1.weight))
            m2.weight.copy_(cuda(W2).view_as(m2.weight))
        m1.fwd = m2.fwd = form
        x = cuda(X).requires_grad_(True)
        out = m2(m1(dcl.spconv.SparseConvTensor(x, cuda(geo["idx"]), [geo["S"]] * 3, geo["b"])))
        assert out.features.shape == G.shape
        out.features.backward(cuda(G))
        res[form] = (out.features.detach().clone(), x.grad.clone(), m1.weight.grad.clone(), m2.weight.grad.clone())
    assert float(res["tiles"][0].abs().max()) > 0
    for a, b in zip(res["compact"], res["tiles"]):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------- 8. Network
def _count_forms(dcl, monkeypatch):
    calls = []
    real = dcl.ops.sparse_conv

    def counting(feat, nbr, n_out, W, subm, *a, **kw):
        calls.append((kw.get("form", "tiles"), int(W.shape[-2]), int(W.shape[-1]), bool(subm)))
        return real(feat, nbr, n_out, W, subm, *a, **kw)

    monkeypatch.setattr(dcl.ops, "sparse_conv", counting)
    return calls


@pytest.mark.parametrize("table", ["committed", "all three"])
def test_network_step_with_compact(dcl, monkeypatch, table):
    """`committed`: ops.CONV_FWD_COMPACT_WIDTHS as measured; `all three`: the table set to the three dilating widths for this test,
    so that a training step through the kernel is checked whatever the measurement left in the table"""
    if table == "all three":
        monkeypatch.setattr(dcl.ops, "CONV_FWD_COMPACT_WIDTHS", frozenset(fc.DILATING_WIDTHS))
    widths = dcl.ops.CONV_FWD_COMPACT_WIDTHS
    b, n = 2, 256
    data = dcl.synth.make_batch(b, n, n)
    data["flags"] = torch.tensor([0.0, 1.0])
    crit = dcl.DCL_Net.losses(None)
    calls = _count_forms(dcl, monkeypatch)

    def make(**kw):
        net = dcl.DCL_Net.Network(dcl.synth.default_cfg(n, n), mode="train", graph_max_batch=0, **kw)
        net.load_state_dict(dcl.synth.synth_state_dict(net, 1))
        return net.cuda().train()

    default = make()
    net = make(train_conv_fwd="compact")
    assert list(net.state_dict().keys()) == list(default.state_dict().keys())
    del calls[:]
    pred = net(data)
    fwd_calls = list(calls)
    compact = [c for c in fwd_calls if c[0] == "compact"]
    assert len(compact) == 2 * len(widths)                                       # both backbones
    assert all(not c[3] and (c[1], c[2]) in widths for c in compact)             # never the stem, never a subm layer
    assert len(fwd_calls) == 16
    loss = crit(pred, data["labels"])["loss_all"]
    loss.backward()
    torch.cuda.synchronize()
    assert torch.isfinite(loss)
    grads = {k: p.grad for k, p in net.named_parameters() if p.grad is not None}
    assert len(grads) > 60
    for k, gd in grads.items():
        assert torch.isfinite(gd).all(), k
    assert sum(c[0] == "compact" for c in calls) == 2 * len(widths)              # the backward re-enters the default form only
    # a default Network and eval mode never call it
    del calls[:]
    crit(default(data), data["labels"])["loss_all"].backward()
    assert len(calls) >= 16 and not [c for c in calls if c[0] == "compact"]
    del calls[:]
    net.eval()
    with torch.no_grad():
        net(data)
    torch.cuda.synchronize()
    assert not [c for c in calls if c[0] == "compact"]
