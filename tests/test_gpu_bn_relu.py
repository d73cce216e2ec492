"""The sparse-conv BatchNorm + ReLU and its gradient on the GPU (csrc/bn_relu.hip): the kernels against their host twins bit for
bit, aligned against 4-byte-aligned views, exact operands against float64, autograd.BnReluFn against the module composition and
float64 under the project's rule (the backward's reference with the mask of the forward under test, the mask itself under
its own cap), determinism, in-place dx, selective gradients, non-contiguous inputs, and the `train_norm="fused"` wiring of
Network.  tests/bn_relu_cases.py holds the shapes, the operands and the CPU references, built once."""
import pytest
import torch

import bn_relu_cases as BN

pytestmark = pytest.mark.gpu

OUT = BN.FWD + BN.BWD
_HOST = {}


def host_run(dcl, i, kind, relu=True):
    """the host twins' outputs of random_case(i, kind), computed once"""
    key = (i, kind, relu)
    if key not in _HOST:
        k = BN.random_case(i, kind)
        rm, rv = k["running_mean"].clone(), k["running_var"].clone()
        z, mean, invstd = dcl.ops.bn_relu_host(k["x"], k["gamma"], k["beta"], rm, rv, BN.MOMENTUM, BN.EPS, relu)
        dx, dgamma, dbeta = dcl.ops.bn_relu_backward_host(k["x"], k["gamma"], k["beta"], mean, invstd, k["g"], relu)
        _HOST[key] = dict(z=z, mean=mean, invstd=invstd, running_mean=rm, running_var=rv, dx=dx, dgamma=dgamma, dbeta=dbeta)
    return _HOST[key]


def one_float_in(t):
    """the same values in a view that starts one float into a larger buffer: 4-byte alignment only"""
    buf = torch.empty(t.numel() + 8, dtype=torch.float32, device="cuda")
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def dev_run(dcl, k, relu=True, eps=BN.EPS, momentum=BN.MOMENTUM, unaligned=False, **need):
    """one forward + backward of the kernels -> every output, the running statistics updated on clones"""
    place = one_float_in if unaligned else (lambda t: t.cuda())
    x, g = place(k["x"]), place(k["g"])
    gamma, beta, rm, rv = (k[n].cuda() for n in ("gamma", "beta", "running_mean", "running_var"))
    z, mean, invstd = dcl.ops.bn_relu(x, gamma, beta, rm, rv, momentum, eps, relu)
    out = one_float_in(k["x"]) if unaligned and need.get("need_x", True) else None
    dx, dgamma, dbeta = dcl.ops.bn_relu_backward(x, gamma, beta, mean, invstd, g, relu, out=out, **need)
    torch.cuda.synchronize()
    return dict(z=z, mean=mean, invstd=invstd, running_mean=rm, running_var=rv, dx=dx, dgamma=dgamma, dbeta=dbeta)


@pytest.mark.parametrize("kind", BN.KINDS)
@pytest.mark.parametrize("i", range(len(BN.SHAPES)), ids=BN.IDS)
def test_kernels_equal_their_host_twins_bit_for_bit(dcl, i, kind):
    got, want = dev_run(dcl, BN.random_case(i, kind)), host_run(dcl, i, kind)
    for name in OUT:
        assert BN.same_bits(got[name], want[name]), (BN.IDS[i], kind, name, float((got[name].cpu() - want[name]).abs().max()))


def test_kernels_equal_their_host_twins_without_the_relu(dcl):
    got, want = dev_run(dcl, BN.random_case(4, "conv"), relu=False), host_run(dcl, 4, "conv", relu=False)
    assert bool((got["z"] < 0).any())
    for name in OUT:
        assert BN.same_bits(got[name], want[name]), name


@pytest.mark.parametrize("i", [0, 3, 4, 6, 8, 10], ids=[BN.IDS[i] for i in (0, 3, 4, 6, 8, 10)])
def test_aligned_and_one_float_offset_views_give_the_same_bits(dcl, i):
    """C % 4 == 0: the aligned call moves 16 bytes per lane, the offset one floats one by one, x, g and dx alike"""
    k = BN.random_case(i, "conv")
    assert k["x"].shape[1] % 4 == 0
    got, want = dev_run(dcl, k, unaligned=True), host_run(dcl, i, "conv")
    for name in OUT:
        assert BN.same_bits(got[name], want[name]), (BN.IDS[i], name)


def test_the_same_call_twice_gives_the_same_bits(dcl):
    k = BN.random_case(9, "offset")
    a, b = dev_run(dcl, k), dev_run(dcl, k)
    for name in OUT:
        assert BN.same_bits(a[name], b[name]), name


@pytest.mark.parametrize("i", range(len(BN.EXACT_SHAPES)), ids=BN.EXACT_IDS)
def test_exact_operands_equal_float64_on_the_device(dcl, i):
    k = BN.exact_case(i)
    V = k["x"].shape[0]
    ref = BN.formulas64(k["x"], k["gamma"], k["beta"], k["g"], 0.0, BN.EXACT_MOMENTUM, k["running_mean"], k["running_var"])
    got = dev_run(dcl, k, eps=0.0, momentum=BN.EXACT_MOMENTUM)
    for name in ["z", "mean", "invstd", "running_mean", "dgamma", "dbeta"] + (["dx"] if V == 2048 else []):
        assert bool((got[name].cpu().double() == ref[name]).all()), (BN.EXACT_IDS[i], name)
    # gradient 0 at y == 0: channel 0's lower half has y = 0 under g >= 1
    hit = ref["z"][:, 0] == 0
    assert int(hit.sum()) == V // 2 and bool((got["dbeta"][0].cpu().double() == k["g"][~hit, 0].double().sum()))


def fn_run(dcl, k, need_x=True, need_affine=True):
    """one BnReluFn forward + backward on the device -> outputs and the gradients that were asked for"""
    x = k["x"].cuda().requires_grad_(need_x)
    gamma, beta = (k[n].cuda().requires_grad_(need_affine) for n in ("gamma", "beta"))
    rm, rv = k["running_mean"].cuda(), k["running_var"].cuda()
    z = dcl.autograd.BnReluFn.apply(x, gamma, beta, rm, rv, BN.MOMENTUM, BN.EPS)
    z.backward(k["g"].cuda())
    torch.cuda.synchronize()
    return dict(z=z.detach(), running_mean=rm, running_var=rv, dx=x.grad, dgamma=gamma.grad, dbeta=beta.grad)


@pytest.mark.parametrize("kind", BN.KINDS)
@pytest.mark.parametrize("i", [4, 5, 9, 10], ids=[BN.IDS[i] for i in (4, 5, 9, 10)])
def test_bn_relu_fn_against_the_module_composition_and_float64(dcl, i, kind):
    k = BN.random_case(i, kind)
    got = fn_run(dcl, k)
    _, m32, m32_ref = BN.module_refs(i, kind)
    ref = BN.case_formulas64(k, mask=got["z"].cpu() > 0)          # the backward's reference takes the mask under test
    BN.compare("%s %s" % (BN.IDS[i], kind), got, ref, m32, m32_ref, ("z", "running_mean", "running_var") + BN.BWD)
    n = BN.mask_differences(got["z"], ref)
    print("mask differences %d of %d (module: %d)" % (n, got["z"].numel(), BN.mask_differences(m32["z"], ref)))
    assert n <= BN.MASK_CAP * got["z"].numel()
    want = host_run(dcl, i, kind)                                 # and the function is the ops: the twins' bits
    for name in ("z", "running_mean", "running_var") + BN.BWD:
        assert BN.same_bits(got[name], want[name]), name


def test_dx_written_over_g_gives_the_bits_of_the_out_of_place_call(dcl):
    k = BN.random_case(4, "conv")
    want = host_run(dcl, 4, "conv")
    x, gamma, beta, g = (k[n].cuda() for n in ("x", "gamma", "beta", "g"))
    dx, dgamma, dbeta = dcl.ops.bn_relu_backward(x, gamma, beta, want["mean"].cuda(), want["invstd"].cuda(), g, out=g)
    assert dx is g
    for name, t in (("dx", g), ("dgamma", dgamma), ("dbeta", dbeta)):
        assert BN.same_bits(t, want[name]), name


def test_selective_gradients(dcl):
    k = BN.random_case(6, "conv")
    full = fn_run(dcl, k)
    only_x = fn_run(dcl, k, need_affine=False)
    assert only_x["dgamma"] is None and only_x["dbeta"] is None and BN.same_bits(only_x["dx"], full["dx"])
    only_affine = fn_run(dcl, k, need_x=False)
    assert only_affine["dx"] is None
    assert BN.same_bits(only_affine["dgamma"], full["dgamma"]) and BN.same_bits(only_affine["dbeta"], full["dbeta"])
    got = dev_run(dcl, k, need_x=False)
    assert got["dx"] is None and BN.same_bits(got["dgamma"], full["dgamma"])
    got = dev_run(dcl, k, need_affine=False)
    assert got["dgamma"] is None and got["dbeta"] is None and BN.same_bits(got["dx"], full["dx"])


def test_non_contiguous_inputs_are_copied_not_misread(dcl):
    k = BN.random_case(6, "conv")
    want = fn_run(dcl, k)
    t = dict(k)
    t["x"] = k["x"].t().contiguous().t()                          # the same values behind other strides
    t["g"] = k["g"].t().contiguous().t()
    assert not t["x"].is_contiguous() and not t["g"].is_contiguous()
    got = fn_run(dcl, t)
    for name in ("z", "running_mean", "running_var") + BN.BWD:
        assert BN.same_bits(got[name], want[name]), name
    wide = torch.zeros(k["x"].shape[0], 2 * k["x"].shape[1], device="cuda")
    wide[:, ::2] = k["x"].cuda()
    z, _, _ = dcl.ops.bn_relu(wide[:, ::2], k["gamma"].cuda(), k["beta"].cuda())
    assert BN.same_bits(z, want["z"])


def _net(dcl, n, mode, **kw):
    net = dcl.DCL_Net.Network(dcl.synth.default_cfg(n, n), mode=mode, **kw)
    net.load_state_dict(dcl.synth.synth_state_dict(net, 1))
    return net.cuda()


def test_network_wiring_of_train_norm_fused(dcl):
    """no tolerance: what a block hands on is what a stand-alone BnReluFn makes of the captured conv output, and the running
    statistics after the step are what it leaves in clones of those before"""
    b, n = 2, 1024
    net = _net(dcl, n, "train", train_norm="fused").train()
    data = dcl.synth.make_batch(b, n, n)
    data["flags"] = torch.tensor([0.0, 1.0])
    blocks = [(name, m) for name, m in net.named_modules() if isinstance(m, dcl.Modules.BasicBlock_SPCONV)]
    assert len(blocks) == 16 and all(name.startswith("backbone_") and m.norm_form == "fused" for name, m in blocks)
    before = {name: (m.layers[1].running_mean.clone(), m.layers[1].running_var.clone(), int(m.layers[1].num_batches_tracked))
              for name, m in blocks}
    seen, hooks = {}, []
    for name, m in blocks:
        hooks.append(m.layers[0].register_forward_hook(
            lambda mod, a, out, name=name: seen.setdefault(name + ".conv", []).append(out.features.detach().clone())))
        hooks.append(m.register_forward_hook(
            lambda mod, a, out, name=name: seen.setdefault(name + ".out", []).append(out.features.detach().clone())))
    pred = net(data)
    for h in hooks:
        h.remove()
    for name, m in blocks:
        bn = m.layers[1]
        assert len(seen[name + ".conv"]) == 1 and len(seen[name + ".out"]) == 1, name
        x, out = seen[name + ".conv"][0], seen[name + ".out"][0]
        assert x.shape[0] > 1 and x.shape[1] == m.dim_out
        rm, rv, nbt = before[name]
        z = dcl.autograd.BnReluFn.apply(x, bn.weight.detach(), bn.bias.detach(), rm, rv, bn.momentum, bn.eps)
        assert BN.same_bits(out, z), name
        assert BN.same_bits(bn.running_mean, rm) and BN.same_bits(bn.running_var, rv), name
        assert nbt == 0 and int(bn.num_batches_tracked) == 1, name
    loss = dcl.DCL_Net.losses(None)(pred, data["labels"])["loss_all"]
    loss.backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss))
    bad = [name for name, p in net.named_parameters() if p.grad is None or not bool(torch.isfinite(p.grad).all())]
    assert bad == []
    for name, m in blocks:
        assert float(m.layers[1].weight.grad.abs().sum()) > 0 and float(m.layers[1].bias.grad.abs().sum()) > 0, name


def test_eval_mode_does_not_read_train_norm(dcl):
    b, n = 2, 256
    outs = []
    for form in ("modules", "fused"):
        net = _net(dcl, n, "test", train_norm=form, graph_max_batch=0).eval()
        with torch.no_grad():
            pred = net(dcl.synth.make_batch(b, n, n))
        torch.cuda.synchronize()
        outs.append({name: v.clone() for name, v in pred.items() if torch.is_tensor(v)})
    assert outs[0].keys() == outs[1].keys() and {"rot_pred", "trans_pred", "conf"} <= set(outs[0])
    for name in outs[0]:
        assert BN.same_bits(outs[0][name].float(), outs[1][name].float()), name
