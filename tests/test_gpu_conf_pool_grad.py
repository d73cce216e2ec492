"""The channel-major confidence pooling and its gradient on the GPU (csrc/conf_pool_grad.hip): the kernels against their host
twins bit for bit, exact operands against float64, autograd.ConfPoolFn against the module composition and a float64 twin under
the project's rule, determinism, selective gradients, non-contiguous inputs, and the `train_pool="fused"` wiring of Network.
tests/conf_pool_cases.py holds the shapes, the operands and the CPU references, built once."""
import pytest
import torch

import conf_pool_cases as CP

pytestmark = pytest.mark.gpu

_IN = ("conf", "w", "F1", "F2", "g_pooled", "g_conf")


def _dev(k, names=_IN):
    return {n: k[n].cuda() for n in names}


def _kernels(dcl, d, g_conf, **need):
    out = {"pooled": dcl.ops.conf_pool_cm(d["w"], d["F1"], d["F2"])}
    got = dcl.ops.conf_pool_cm_backward(d["conf"], d["w"], d["F1"], d["F2"], d["g_pooled"], g_conf, **need)
    out.update(zip(("dlogit1", "dlogit2", "dF1", "dF2"), got))
    return out


def _host(dcl, k, g_conf):
    out = {"pooled": dcl.ops.conf_pool_cm_host(k["w"], k["F1"], k["F2"])}
    got = dcl.ops.conf_pool_cm_backward_host(k["conf"], k["w"], k["F1"], k["F2"], k["g_pooled"], g_conf)
    out.update(zip(("dlogit1", "dlogit2", "dF1", "dF2"), got))
    return out


@pytest.mark.parametrize("with_g_conf", [True, False], ids=["g_conf", "no_g_conf"])
@pytest.mark.parametrize("i", range(len(CP.SHAPES)), ids=CP.IDS)
def test_kernels_equal_their_host_twins_bit_for_bit(dcl, i, with_g_conf):
    k = CP.random_case(i)
    d = _dev(k)
    got = _kernels(dcl, d, d["g_conf"] if with_g_conf else None)
    want = _host(dcl, k, k["g_conf"] if with_g_conf else None)
    for name in CP.OUTPUTS:
        assert CP.same_bits(got[name], want[name]), (CP.IDS[i], name, float((got[name].cpu() - want[name]).abs().max()))


@pytest.mark.parametrize("i", [1, 2, 3, 5], ids=CP.IDS[1:4] + CP.IDS[5:])
def test_exact_operands_equal_float64_on_the_device(dcl, i):
    k = CP.exact_case(i)
    d = _dev(k)
    ref = CP.formulas64(k["conf"], k["w"], k["F1"], k["F2"], k["g_pooled"], k["g_conf"])
    got = _kernels(dcl, d, d["g_conf"])
    for name in CP.OUTPUTS:
        assert bool((got[name].cpu().double() == ref[name]).all()), (CP.IDS[i], name)


def _fn(dcl, k, logits=True, F=True, g_conf=True, g_pooled=True):
    """one ConfPoolFn forward + backward on the device -> outputs and the gradients that were asked for"""
    l1, l2 = (k[n].cuda().requires_grad_(logits) for n in ("logit1", "logit2"))
    F1, F2 = (k[n].cuda().requires_grad_(F) for n in ("F1", "F2"))
    conf, pooled = dcl.autograd.ConfPoolFn.apply(l1, l2, F1, F2)
    outs, grads = [], []
    if g_conf:
        outs.append(conf), grads.append(k["g_conf"].cuda())
    if g_pooled:
        outs.append(pooled), grads.append(k["g_pooled"].cuda())
    torch.autograd.backward(outs, grads)
    return dict(conf=conf.detach(), pooled=pooled.detach(), dlogit1=None if l1.grad is None else l1.grad.squeeze(1),
                dlogit2=None if l2.grad is None else l2.grad.squeeze(1), dF1=F1.grad, dF2=F2.grad)


@pytest.mark.parametrize("i", [1, 2, 3], ids=CP.IDS[1:4])
def test_conf_pool_fn_against_the_module_composition_and_float64(dcl, i):
    k = CP.random_case(i)
    ref64, mod32 = CP.module_refs(i)
    got = _fn(dcl, k)
    CP.compare(CP.IDS[i], got, ref64, mod32, ("conf",) + CP.OUTPUTS)
    b = k["F1"].shape[0]
    conf, _, _ = dcl.ops.conf_softmax(b, k["logit1"].cuda().reshape(-1), k["logit2"].cuda().reshape(-1))
    assert CP.same_bits(got["conf"], conf)                                    # the train-mode conf is the eval kernel's


def test_the_same_call_twice_gives_the_same_bits(dcl):
    k = CP.random_case(3)
    a, b = _fn(dcl, k), _fn(dcl, k)
    for name in ("conf",) + CP.OUTPUTS:
        assert CP.same_bits(a[name], b[name]), name


def test_a_crop_gives_the_same_bits_alone_as_inside_a_batch(dcl):
    k = CP.random_case(2)                                                     # three crops, one unaligned direction
    full = _kernels(dcl, _dev(k), k["g_conf"].cuda())
    for c in range(3):
        one = {n: k[n][c:c + 1].contiguous().cuda() for n in _IN}
        alone = _kernels(dcl, one, one["g_conf"])
        for name in CP.OUTPUTS:
            assert CP.same_bits(alone[name], full[name][c:c + 1]), (c, name)


def test_selective_gradients(dcl):
    k = CP.random_case(2)
    full = _fn(dcl, k)
    no_F = _fn(dcl, k, F=False)
    assert no_F["dF1"] is None and no_F["dF2"] is None
    assert CP.same_bits(no_F["dlogit1"], full["dlogit1"]) and CP.same_bits(no_F["dlogit2"], full["dlogit2"])
    no_l = _fn(dcl, k, logits=False)
    assert no_l["dlogit1"] is None and no_l["dlogit2"] is None
    assert CP.same_bits(no_l["dF1"], full["dF1"]) and CP.same_bits(no_l["dF2"], full["dF2"])
    # pooled unused: d = dot = 0, so ds = g_conf exactly and dlogit = (g_conf * s) * (1 - s) as the header writes it
    unused = _fn(dcl, k, g_pooled=False)
    assert not bool(unused["dF1"].any()) and not bool(unused["dF2"].any())
    s, g, n1 = unused["conf"], k["g_conf"].cuda(), k["F1"].shape[2]
    want = (g * s) * (1.0 - s)
    assert CP.same_bits(unused["dlogit1"], want[:, :n1]) and CP.same_bits(unused["dlogit2"], want[:, n1:])


def test_non_contiguous_inputs_are_copied_not_misread(dcl):
    k = CP.random_case(2)
    want = _fn(dcl, k)
    t = dict(k)
    t["F1"] = k["F1"].transpose(1, 2).contiguous().transpose(1, 2)            # the same values behind other strides
    t["F2"] = k["F2"].transpose(1, 2).contiguous().transpose(1, 2)
    assert not t["F1"].is_contiguous() and not t["F2"].is_contiguous()
    got = _fn(dcl, t)
    for name in ("conf",) + CP.OUTPUTS:
        assert CP.same_bits(got[name], want[name]), name
    d = _dev(t)
    assert not d["F1"].is_contiguous()
    assert CP.same_bits(dcl.ops.conf_pool_cm(d["w"], d["F1"], d["F2"]), dcl.ops.conf_pool_cm(*(k[n].cuda() for n in ("w", "F1", "F2"))))


def _net(dcl, n, mode, **kw):
    net = dcl.DCL_Net.Network(dcl.synth.default_cfg(n, n), mode=mode, **kw)
    net.load_state_dict(dcl.synth.synth_state_dict(net, 1))
    return net.cuda()


def test_network_wiring_of_train_pool_fused(dcl):
    """no tolerance: what Network hands on is what a stand-alone ConfPoolFn makes of the captured tensors"""
    b, n = 2, 1024
    net = _net(dcl, n, "train", train_pool="fused").train()
    data = dcl.synth.make_batch(b, n, n)
    data["flags"] = torch.tensor([0.0, 1.0])
    seen = {}
    hooks = [getattr(net, name).register_forward_hook(lambda m, a, out, name=name: seen.__setitem__(name, out.detach().clone()))
             for name in ("regressor_conf", "regressor_conf_bi", "neck_fuser", "neck_fuser_bi")]
    hooks.append(net.regressor_rot.register_forward_pre_hook(lambda m, a: seen.__setitem__("rot_in", a[0].detach().clone())))
    pred = net(data)
    for h in hooks:
        h.remove()
    assert tuple(seen["neck_fuser"].shape) == (b, 1024, n) and tuple(seen["regressor_conf"].shape) == (b, 1, n)
    conf, pooled = dcl.autograd.ConfPoolFn.apply(seen["regressor_conf"], seen["regressor_conf_bi"], seen["neck_fuser"],
                                                 seen["neck_fuser_bi"])
    assert tuple(pred["conf"].shape) == (b, 2 * n) and CP.same_bits(pred["conf"], conf)
    assert tuple(seen["rot_in"].shape) == (b, 1024, 1) and CP.same_bits(seen["rot_in"], pooled.unsqueeze(2))
    loss = dcl.DCL_Net.losses(None)(pred, data["labels"])["loss_all"]
    loss.backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss))
    bad = [name for name, p in net.named_parameters() if p.grad is None or not bool(torch.isfinite(p.grad).all())]
    assert bad == []
    assert float(net.neck_fuser.layers[0].weight.grad.abs().sum()) > 0 and float(net.regressor_conf.layers[0].weight.grad.abs().sum()) > 0


def test_eval_mode_does_not_read_train_pool(dcl):
    b, n = 2, 256
    outs = []
    for form in ("modules", "fused"):
        net = _net(dcl, n, "test", train_pool=form, graph_max_batch=0).eval()
        with torch.no_grad():
            pred = net(dcl.synth.make_batch(b, n, n))
        torch.cuda.synchronize()
        outs.append({name: v.clone() for name, v in pred.items() if torch.is_tensor(v)})
    assert outs[0].keys() == outs[1].keys() and {"rot_pred", "trans_pred", "conf"} <= set(outs[0])
    for name in outs[0]:
        assert CP.same_bits(outs[0][name].float(), outs[1][name].float()), name
