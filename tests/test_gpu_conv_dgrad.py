"""ops.sparse_conv_dgrad (csrc/conv_dgrad.hip) on the GPU: the kernel against its host twin BIT FOR BIT on Gaussian operands --
which carries the float64 bound of tests/test_conv_dgrad_abi.py over to the kernel without a tolerance of its own --, against
the integer gradient and the "conv" route on exact operands, what it writes and what it leaves alone, and the dgrad="direct"
switch from ops.sparse_conv_backward through autograd.SparseConvFn and the spconv modules up to Network."""
import numpy as np
import pytest
import torch

import conv_dgrad_cases as dc
import conv_grad_cases as cg
from test_gpu_ops import cuda

pytestmark = pytest.mark.gpu

_RULEBOOKS = {}


def _rulebook(dcl, oracle, case):
    """the device rulebook of a case's geometry and its transpose: (nbr, n_out, inv)"""
    key = (case[0], case[3])
    if key not in _RULEBOOKS:
        geo = cg.geometry(oracle, case[0], case[3])
        aset = dcl.ops.grid_from_indices(cuda(geo["idx"]), geo["b"], geo["S"])
        out, nbr = dcl.spconv.ops.build_rulebook(aset, 3, geo["stride"], geo["padding"], case[3])
        n_out = geo["n_in"] if case[3] else out.n
        assert n_out == geo["n_out"]
        inv = dcl.ops.rulebook_transpose(nbr, n_out, geo["n_in"])
        # the device transpose names the same neighbours as the oracle's pair lists
        assert np.array_equal(inv.cpu().numpy(), dc.inverse_table(geo))
        _RULEBOOKS[key] = (nbr, n_out, inv)
    return _RULEBOOKS[key]


def _where(got, want):
    bad = np.argwhere(got != want)
    if bad.size == 0:
        return ""
    return "%d of %d elements differ; rows %s (first: index %s got %r want %r)" % (
        bad.shape[0], got.size, np.unique(bad[:, 0])[:12].tolist(), bad[0].tolist(), float(got[tuple(bad[0])]),
        float(want[tuple(bad[0])]))


# ------------------------------------------------------------------------------------------- 1. kernel = host twin
@pytest.mark.parametrize("case", dc.CASES, ids=cg.case_id)
def test_kernel_equals_the_host_twin_bit_for_bit_on_gaussian_operands(dcl, oracle, case):
    c = cg.conv_case(oracle, case, "gaussian")
    _, n_out, inv = _rulebook(dcl, oracle, case)
    got = dcl.ops.sparse_conv_dgrad(cuda(c["G"]), inv, c["geo"]["n_in"], cuda(c["W"]))
    want = dc.twin(dcl, oracle, case, "gaussian")
    assert got.shape == want.shape and float(np.abs(want).max()) > 0.1
    assert _where(got.cpu().numpy(), want) == ""


@pytest.mark.parametrize("cin,cout", dc.WIDTHS)
def test_kernel_equals_the_host_twin_on_the_hand_made_table(dcl, cin, cout):
    W, G = dc.hand_operands(cin, cout, exact=False)
    want = dcl.ops.sparse_conv_dgrad_host(G, dc.HAND_INV, dc.HAND_N_IN, W, n_out=dc.HAND_N_OUT)
    # the kernel takes n_out from the rows it is given: the NaN rows lie behind the tensor it sees, in the same allocation
    g = cuda(G)
    got = dcl.ops.sparse_conv_dgrad(g[:dc.HAND_N_OUT], cuda(dc.HAND_INV), dc.HAND_N_IN, cuda(W))
    assert torch.isfinite(got).all()
    assert _where(got.cpu().numpy(), want) == ""
    assert not got[3].any() and not torch.signbit(got[3]).any()
    wide = dc.hand_embedded(203, np.random.default_rng(cin))
    assert torch.equal(dcl.ops.sparse_conv_dgrad(g[:dc.HAND_N_OUT], cuda(wide), dc.HAND_N_IN, cuda(W)), got)


# ------------------------------------------------------------------------------------------- 2. exact operands
@pytest.mark.parametrize("case", dc.CASES, ids=cg.case_id)
def test_exact_operands_give_the_integer_gradient_and_the_conv_routes_bits(dcl, oracle, case):
    c = cg.conv_case(oracle, case, "exact")
    nbr, n_out, inv = _rulebook(dcl, oracle, case)
    f, w, g = cuda(c["X"]), cuda(c["W"]), cuda(c["G"])
    got = dcl.ops.sparse_conv_dgrad(g, inv, c["geo"]["n_in"], w)
    assert _where(got.cpu().numpy(), c["dX"].astype(np.float32)) == ""
    dx_conv, _ = dcl.ops.sparse_conv_backward(f, w, g, nbr, n_out, case[3], dgrad="conv")
    dx_direct, _ = dcl.ops.sparse_conv_backward(f, w, g, nbr, n_out, case[3], dgrad="direct")
    assert torch.equal(dx_direct, got) and torch.equal(dx_conv, got)


# ------------------------------------------------------------------------------------------- 3. what is written
@pytest.mark.parametrize("case", [("tail100", 16, 32, True), ("edge2049", 33, 40, False), ("two1500", 128, 256, True),
                                  ("stride2s", 64, 64, False)], ids=cg.case_id)
def test_all_rows_written_guard_rows_untouched_and_the_same_bits_again(dcl, oracle, case):
    c = cg.conv_case(oracle, case, "gaussian")
    _, n_out, inv = _rulebook(dcl, oracle, case)
    n_in, cin, cout, guard = c["geo"]["n_in"], case[1], case[2], 67
    g, w = cuda(c["G"]), cuda(c["W"])
    vp = dcl._native.vp

    def run():
        buf = torch.full((n_in + guard, cin), float("nan"), dtype=torch.float32, device="cuda")
        dcl._native.check(dcl._native.lib().dcl_sparse_conv_dgrad(
            vp(g.data_ptr()), n_out, vp(inv.data_ptr()), inv.shape[1], n_in, vp(w.data_ptr()), cin, cout, 27, vp(buf.data_ptr()),
            dcl._native.stream()), "sparse_conv_dgrad")
        return buf

    a, b = run(), run()
    assert torch.isfinite(a[:n_in]).all()
    assert torch.isnan(a[n_in:]).all()
    assert torch.equal(a[:n_in], b[:n_in])
    assert _where(a[:n_in].cpu().numpy(), dc.twin(dcl, oracle, case, "gaussian")) == ""


def test_empty_sides_give_written_zeros(dcl):
    W = cuda(cg.exact_array(np.random.default_rng(0), (27, 32, 64)))
    inv = torch.full((27, 5), -1, dtype=torch.int32, device="cuda")
    dx = dcl.ops.sparse_conv_dgrad(torch.zeros((0, 64), device="cuda"), inv, 5, W)             # no dout rows
    assert dx.shape == (5, 32) and not dx.any() and not torch.signbit(dx).any()
    assert dcl.ops.sparse_conv_dgrad(torch.ones((3, 64), device="cuda"), inv, 0, W).shape == (0, 32)


# ------------------------------------------------------------------------------------------- 4. dW is untouched
@pytest.mark.parametrize("case", [("edge2049", 16, 32, True), ("stride2s", 32, 64, False), ("two1500", 128, 256, True)],
                         ids=cg.case_id)
@pytest.mark.parametrize("wgrad", ["rows", "pairs"])
def test_the_switch_leaves_the_weight_gradient_alone(dcl, oracle, case, wgrad):
    c = cg.conv_case(oracle, case, "gaussian")
    nbr, n_out, _ = _rulebook(dcl, oracle, case)
    f, w, g = cuda(c["X"]), cuda(c["W"]), cuda(c["G"])
    dx_c, dw_c = dcl.ops.sparse_conv_backward(f, w, g, nbr, n_out, case[3], wgrad=wgrad, dgrad="conv")
    dx_d, dw_d = dcl.ops.sparse_conv_backward(f, w, g, nbr, n_out, case[3], wgrad=wgrad, dgrad="direct")
    assert torch.equal(dw_d, dw_c)
    assert _where(dx_d.cpu().numpy(), dc.twin(dcl, oracle, case, "gaussian")) == ""
    with pytest.raises(ValueError):
        dcl.ops.sparse_conv_backward(f, w, g, nbr, n_out, case[3], dgrad="pairs")


# ------------------------------------------------------------------------------------------- 5. autograd
@pytest.mark.parametrize("subm", [True, False], ids=["SubMConv3d", "SparseConv3d"])
def test_spconv_modules_with_direct_give_the_conv_gradients_on_exact_operands(dcl, oracle, subm):
    case = ("two1500", 16, 32, subm)
    c = cg.conv_case(oracle, case, "exact")
    geo = c["geo"]
    cls = dcl.spconv.SubMConv3d if subm else dcl.spconv.SparseConv3d
    grads = {}
    for form in ("conv", "direct"):
        m = cls(16, 32, 3, padding=1, bias=False).cuda()
        with torch.no_grad():
            m.weight.copy_(cuda(c["W"]).view_as(m.weight))
        m.dgrad = form
        x = cuda(c["X"]).requires_grad_(True)
        out = m(dcl.spconv.SparseConvTensor(x, cuda(geo["idx"]), [geo["S"]] * 3, geo["b"]))
        assert out.features.shape == c["G"].shape
        out.features.backward(cuda(c["G"]))
        grads[form] = (x.grad.clone(), m.weight.grad.clone())
    assert _where(grads["direct"][0].cpu().numpy(), c["dX"].astype(np.float32)) == ""
    assert torch.equal(grads["direct"][0], grads["conv"][0]) and torch.equal(grads["direct"][1], grads["conv"][1])
    assert _where(grads["direct"][1].reshape(27, 16, 32).cpu().numpy(), c["dW"].astype(np.float32)) == ""


def test_autograd_function_takes_the_form_and_keeps_its_shorter_calls(dcl, oracle):
    case = ("edge2049", 16, 32, True)
    c = cg.conv_case(oracle, case, "gaussian")
    nbr, n_out, _ = _rulebook(dcl, oracle, case)
    f, w, g = cuda(c["X"]), cuda(c["W"]), cuda(c["G"])
    grads = {}
    for form, args in (("direct", ("rows", "direct")), ("conv", ("rows", "conv")), ("six", ("rows",)), ("five", ())):
        fa, wa = f.clone().requires_grad_(True), w.clone().requires_grad_(True)
        dcl.autograd.SparseConvFn.apply(fa, wa, nbr, n_out, True, *args).backward(g)
        grads[form] = (fa.grad, wa.grad)
    assert _where(grads["direct"][0].cpu().numpy(), dc.twin(dcl, oracle, case, "gaussian")) == ""
    for form in ("six", "five"):
        assert torch.equal(grads[form][0], grads["conv"][0]) and torch.equal(grads[form][1], grads["conv"][1])
    assert torch.equal(grads["direct"][1], grads["conv"][1])
    with pytest.raises(ValueError):
        dcl.autograd.SparseConvFn.apply(f, w, nbr, n_out, True, "rows", "nope")


def test_network_step_with_direct_keeps_the_loss_bits_and_gives_finite_gradients(dcl):
    b, n = 2, 256
    data = dcl.synth.make_batch(b, n, n)
    data["flags"] = torch.tensor([0.0, 1.0])
    crit = dcl.DCL_Net.losses(None)
    table = dcl.ops.CONV_DGRAD_DIRECT_WIDTHS

    def step(form):
        net = dcl.DCL_Net.Network(dcl.synth.default_cfg(n, n), mode="train", train_conv_dgrad=form)
        net.load_state_dict(dcl.synth.synth_state_dict(net, 1))
        net = net.cuda().train()
        convs = [m for m in net.modules() if isinstance(m, dcl.spconv.SparseConvolution)]
        assert len(convs) == 16
        for m in convs:
            direct = form == "direct" and (m.in_channels, m.out_channels) in table
            assert m.dgrad == ("direct" if direct else "conv"), (form, m.in_channels, m.out_channels)
        loss = crit(net(data), data["labels"])["loss_all"]
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach().clone(), {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}, len(
            [m for m in convs if m.dgrad == "direct"])

    loss_c, grads_c, n_c = step("conv")
    loss_d, grads_d, n_d = step("direct")
    assert n_c == 0 and n_d == 2 * len(table)
    assert torch.isfinite(loss_c) and torch.equal(loss_d, loss_c)                # the forward is untouched
    assert grads_d.keys() == grads_c.keys() and len(grads_d) > 60
    for k, gd in grads_d.items():
        assert torch.isfinite(gd).all(), k
