"""The point-major dense half of the training path on the GPU (Network(train_dense="point_major")): autograd.PointLinearFn
and the BatchNorm without ReLU against float64 under the project's rule, one side's merged disengage stacks and one fuser
against the module stacks, the wiring of Network without a tolerance, and the constructor's rules.
tests/train_dense_cases.py holds the shapes, the operands and the float64 twins."""
import pytest
import torch

import bn_relu_cases as BN
import train_dense_cases as TD

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------- PointLinearFn
def _linear(dcl, k, relu, strided=False, need=(True, True, True)):
    """one PointLinearFn forward + backward on the device; strided: x and g are column blocks of wider matrices"""
    x, W, bias, g = (k[n].cuda() for n in ("x", "W", "bias", "g"))
    if strided:
        x = torch.cat([torch.zeros_like(x[:, :32]), x, torch.ones_like(x[:, :4])], dim=1)[:, 32:32 + x.shape[1]]
        g = torch.cat([torch.ones_like(g[:, :64]), g], dim=1)[:, 64:]
        assert not x.is_contiguous() and not g.is_contiguous()
    x = x.detach().requires_grad_(need[0])
    W = W.detach().requires_grad_(need[1])
    bias = bias.detach().requires_grad_(need[2]) if relu else None
    if strided:
        wide = torch.zeros((g.shape[0], g.shape[1] + 64), device="cuda")
        y = dcl.autograd.PointLinearFn.apply(x, W, bias, relu)
        (torch.cat([wide[:, :64], y], dim=1) * torch.cat([wide[:, :64], g], dim=1)).sum().backward()   # the gradient arrives as a view
    else:
        y = dcl.autograd.PointLinearFn.apply(x, W, bias, relu)
        y.backward(g)
    return dict(y=y.detach(), dx=x.grad, dW=W.grad, db=None if bias is None else bias.grad)


@pytest.mark.parametrize("relu", [False, True], ids=["plain", "bias_relu"])
@pytest.mark.parametrize("i", range(len(TD.LINEAR_SHAPES)), ids=TD.LINEAR_IDS)
def test_point_linear_fn_against_float64(dcl, i, relu):
    k = TD.linear_case(i)
    got = _linear(dcl, k, relu)
    assert got["dW"].shape == k["W"].shape
    mod32 = TD.linear_form(k, relu, torch.float32)
    ref_got = TD.linear_form(k, relu, torch.float64, mask=(got["y"].cpu() > 0) if relu else None)
    ref_mod = TD.linear_form(k, relu, torch.float64, mask=mod32["mask"])
    names = ("y", "dx", "dW") + (("db",) if relu else ())
    TD.compare(TD.LINEAR_IDS[i], got, ref_got, mod32, ref_mod, names)
    again = _linear(dcl, k, relu)
    for name in names:
        assert TD.same_bits(got[name], again[name]), name
    strided = _linear(dcl, k, relu, strided=True)
    for name in names:                                       # the pinned orders do not depend on a pitch
        assert TD.same_bits(got[name], strided[name]), name


def test_point_linear_fn_computes_only_what_is_asked_for(dcl):
    k = TD.linear_case(3)
    full = _linear(dcl, k, True)
    only_w = _linear(dcl, k, True, need=(False, True, False))
    assert only_w["dx"] is None and only_w["db"] is None and TD.same_bits(only_w["dW"], full["dW"])
    only_x = _linear(dcl, k, True, need=(True, False, False))
    assert only_x["dW"] is None and TD.same_bits(only_x["dx"], full["dx"])


def test_point_linear_fn_refusals(dcl):
    x, W, bias = torch.randn(64, 64, device="cuda"), torch.randn(32, 64, 1, device="cuda"), torch.randn(32, device="cuda")
    with pytest.raises(ValueError, match="two forms"):
        dcl.autograd.PointLinearFn.apply(x, W, bias, False)                  # a bias without the ReLU
    with pytest.raises(ValueError, match="multiple of 32"):
        dcl.autograd.PointLinearFn.apply(x[:, :48].contiguous(), W[:, :48].contiguous(), None, False)     # K = 48
    with pytest.raises(ValueError, match="16-byte|multiple of 32"):
        dcl.autograd.PointLinearFn.apply(torch.randn(64, 67, device="cuda")[:, 1:65], W, None, False)     # an odd pitch
    with pytest.raises(ValueError, match="multiple of 32"):
        dcl.autograd.PointLinearFn.apply(x, W[:3].contiguous(), None, False)                              # N = 3


# ---------------------------------------------------------------------------------------------------- BatchNorm without ReLU
@pytest.mark.parametrize("i", [4, 5], ids=[BN.IDS[4], BN.IDS[5]])
def test_bn_without_relu_kernels_equal_their_host_twins(dcl, i):
    k = BN.random_case(i, "conv")
    d = {n: v.cuda() for n, v in k.items()}
    rm_h, rv_h, rm_d, rv_d = k["running_mean"].clone(), k["running_var"].clone(), d["running_mean"].clone(), d["running_var"].clone()
    zh, mh, ih = dcl.ops.bn_relu_host(k["x"], k["gamma"], k["beta"], rm_h, rv_h, BN.MOMENTUM, BN.EPS, relu=False)
    zd, md, idv = dcl.ops.bn_relu(d["x"], d["gamma"], d["beta"], rm_d, rv_d, BN.MOMENTUM, BN.EPS, relu=False)
    assert bool((zd < 0).any())                                           # no ReLU was applied
    for a, b in ((zd, zh), (md, mh), (idv, ih), (rm_d, rm_h), (rv_d, rv_h)):
        assert BN.same_bits(a, b)
    want = dcl.ops.bn_relu_backward_host(k["x"], k["gamma"], k["beta"], mh, ih, k["g"], relu=False)
    got = dcl.ops.bn_relu_backward(d["x"], d["gamma"], d["beta"], md, idv, d["g"], relu=False)
    for a, b in zip(got, want):
        assert BN.same_bits(a, b)


def test_bn_without_relu_under_autograd_against_float64(dcl):
    k = BN.random_case(4, "conv")
    x, gamma, beta = (k[n].cuda().requires_grad_(True) for n in ("x", "gamma", "beta"))
    rm, rv = k["running_mean"].cuda(), k["running_var"].cuda()
    z = dcl.autograd.BnReluFn.apply(x, gamma, beta, rm, rv, BN.MOMENTUM, BN.EPS, False)
    z.backward(k["g"].cuda())
    got = dict(z=z.detach(), running_mean=rm, running_var=rv, dx=x.grad, dgamma=gamma.grad, dbeta=beta.grad)
    ref = BN.case_formulas64(k, relu=False)
    BN.compare(BN.IDS[4], got, ref, BN.module_form(k, torch.float32, relu=False), ref, tuple(got))
    # the default is still BatchNorm + ReLU, through seven arguments
    z7 = dcl.autograd.BnReluFn.apply(k["x"].cuda(), k["gamma"].cuda(), k["beta"].cuda(), None, None, BN.MOMENTUM, BN.EPS)
    assert torch.equal(z7, torch.relu(z.detach()))


# ---------------------------------------------------------------------------------------------------- stacks of Network
def _net(dcl, n, mode="train", **kw):
    net = dcl.DCL_Net.Network(dcl.synth.default_cfg(n, n), mode=mode, **kw)
    net.load_state_dict(dcl.synth.synth_state_dict(net, 1))
    return net.cuda()


def _pm_net(dcl, n, **kw):
    return _net(dcl, n, train_dense="point_major", train_attention="fused", **kw).train()


def _record(dcl, monkeypatch, *names):
    recs = {}
    for name in names:
        recs[name] = TD.Recorder(getattr(dcl.autograd, name))
        monkeypatch.setattr(dcl.DCL_Net, name, recs[name])
    return recs


def _disengage_run(dcl, net, P, x, g):
    """the merged form on a net whose disengage parameters and buffers are reset to P -> the flat dict of TD.disengage_form"""
    with torch.no_grad():
        for t in TD.STACKS:
            st = getattr(net, "disengage_Xc_" + t)
            for l in (0, 1):
                bn = st[l].layers[1]
                bn.running_mean.copy_(P["%s.%d.rm" % (t, l)]), bn.running_var.copy_(P["%s.%d.rv" % (t, l)])
                bn.num_batches_tracked.zero_()
    net.zero_grad(set_to_none=True)
    xd = x.cuda().requires_grad_(True)
    out = net._pm_disengage("Xc", xd)
    torch.autograd.backward([out[t] for t in TD.STACKS], [g[t].cuda() for t in TD.STACKS])
    res = {"dx": xd.grad}
    for t in TD.STACKS:
        res["out." + t] = out[t].detach()
        st = getattr(net, "disengage_Xc_" + t)
        for l in (0, 1):
            conv, bn = st[l].layers[0], st[l].layers[1]
            res["%s.%d.W" % (t, l)], res["%s.%d.gamma" % (t, l)], res["%s.%d.beta" % (t, l)] = conv.weight.grad, bn.weight.grad, bn.bias.grad
            res["%s.%d.rm" % (t, l)], res["%s.%d.rv" % (t, l)] = bn.running_mean.clone(), bn.running_var.clone()
            assert int(bn.num_batches_tracked) == 1, (t, l)
    return res


def test_disengage_stacks_merged_against_the_four_module_stacks(dcl, monkeypatch):
    b, n = 2, 192
    net = _pm_net(dcl, n)
    P = TD.disengage_params(net, "Xc")
    gen = torch.Generator().manual_seed(7)
    x = torch.randn(b * n, 480, generator=gen).relu_()
    g = {t: torch.randn(b * n, 256 if t[0] == "p" else 64, generator=gen) * 0.1 for t in TD.STACKS}
    recs = _record(dcl, monkeypatch, "BnReluFn")
    got = _disengage_run(dcl, net, P, x, g)
    calls = recs["BnReluFn"].calls
    assert len(calls) == 5 and tuple(calls[0][1].shape) == (b * n, 1024)      # ONE first layer, then the four second layers
    masks = {"first": calls[0][1].detach().cpu() > 0}
    masks.update({t: calls[1 + k][1].detach().cpu() > 0 for k, t in enumerate(TD.STACKS)})
    mod32 = TD.disengage_form(P, x, g, torch.float32)
    ref_got = TD.disengage_form(P, x, g, torch.float64, masks)
    ref_mod = TD.disengage_form(P, x, g, torch.float64, mod32["masks"])
    names = tuple(n_ for n_ in ref_got if n_ != "masks")
    assert len(names) == 4 + 1 + 4 * 2 * 5
    TD.compare("disengage", got, ref_got, mod32, ref_mod, names)
    again = _disengage_run(dcl, net, P, x, g)
    for name in names:
        assert TD.same_bits(got[name], again[name]), name


def _fuser_run(dcl, net, P, x, g):
    fuser = net.neck_fuser
    with torch.no_grad():
        for l in range(3):
            bn = fuser.layers[3 * l + 2]
            bn.running_mean.copy_(P["%d.rm" % l]), bn.running_var.copy_(P["%d.rv" % l])
            bn.num_batches_tracked.zero_()
    net.zero_grad(set_to_none=True)
    xd = x.cuda().requires_grad_(True)
    out = net._pm_fuser(fuser, xd)
    out.backward(g.cuda())
    res = {"out": out.detach(), "dx": xd.grad}
    for l in range(3):
        conv, bn = fuser.layers[3 * l], fuser.layers[3 * l + 2]
        res["%d.W" % l], res["%d.b" % l], res["%d.gamma" % l], res["%d.beta" % l] = conv.weight.grad, conv.bias.grad, bn.weight.grad, bn.bias.grad
        res["%d.rm" % l], res["%d.rv" % l] = bn.running_mean.clone(), bn.running_var.clone()
        assert int(bn.num_batches_tracked) == 1, l
    return res


def test_a_fuser_against_its_module_stack(dcl, monkeypatch):
    M = 2 * 130
    net = _pm_net(dcl, 64)
    P = TD.fuser_params(net.neck_fuser)
    gen = torch.Generator().manual_seed(8)
    x, g = torch.randn(M, 512, generator=gen), torch.randn(M, 1024, generator=gen) * 0.1
    recs = _record(dcl, monkeypatch, "PointLinearFn")
    got = _fuser_run(dcl, net, P, x, g)
    calls = recs["PointLinearFn"].calls
    assert len(calls) == 3 and all(c[0][3] is True for c in calls)
    masks = [c[1].detach().cpu() > 0 for c in calls]
    mod32 = TD.fuser_form(P, x, g, torch.float32)
    ref_got = TD.fuser_form(P, x, g, torch.float64, masks)
    ref_mod = TD.fuser_form(P, x, g, torch.float64, mod32["masks"])
    names = tuple(n_ for n_ in ref_got if n_ != "masks")
    assert len(names) == 2 + 3 * 6
    TD.compare("fuser", got, ref_got, mod32, ref_mod, names)
    again = _fuser_run(dcl, net, P, x, g)
    for name in names:
        assert TD.same_bits(got[name], again[name]), name


def test_network_wiring_of_train_dense_point_major(dcl, monkeypatch):
    """no tolerance: what the point-major path hands to the attention, the pooling and the heads, recomputed stand-alone"""
    b, n = 2, 256
    net = _pm_net(dcl, n)
    data = dcl.synth.make_batch(b, n, n)
    data["flags"] = torch.tensor([0.0, 1.0])
    recs = _record(dcl, monkeypatch, "CrossAttentionFn", "ConfPoolPmFn")
    heads = []
    pm_head = net._pm_head
    monkeypatch.setattr(net, "_pm_head", lambda head, x: heads.append((head, x, pm_head(head, x))) or heads[-1][2])
    seen = {}
    hook = net.regressor_rot.register_forward_pre_hook(lambda m, a: seen.__setitem__("rot_in", a[0].detach().clone()))
    pred = net(data)
    hook.remove()
    A = dcl.autograd
    # the attention: two calls on (b, n, C) views, keys as the second values
    att = recs["CrossAttentionFn"].calls
    assert len(att) == 2
    for args, (o1, o2) in att:
        q, k_, v1, v2 = args
        assert tuple(q.shape) == (b, n, 64) and tuple(v1.shape) == (b, n, 256) and v2 is k_ and q.is_contiguous() and v1.is_contiguous()
        w1, w2 = A.CrossAttentionFn.apply(q.detach().clone(), k_.detach().clone(), v1.detach().clone(), k_.detach().clone())
        assert TD.same_bits(o1, w1) and TD.same_bits(o2, w2)
    assert tuple(pred["F_Xo_p"].shape) == (b, 256, n) and TD.same_bits(pred["F_Xo_p"], att[0][1][0].transpose(1, 2))
    # the heads: conf, conf_bi, Xo, Yc, each the stand-alone composition of its captured input
    assert [h[0] for h in heads] == [net.regressor_conf, net.regressor_conf_bi, net.regressor_Xo, net.regressor_Yc]
    for head, x, out in heads:
        assert x.dim() == 2 and x.shape[0] == b * n
        assert TD.same_bits(out, pm_head(head, x.detach().clone()))
    assert TD.same_bits(heads[0][1][:, 64:], att[0][1][1].reshape(b * n, 64))           # cat[Xc_m1, F_Xo_m]
    assert TD.same_bits(heads[1][1][:, :64], att[1][1][1].reshape(b * n, 64))           # cat[F_Yc_m, Yo_m2]
    assert TD.same_bits(heads[2][1], att[0][1][0].reshape(b * n, 256)) and TD.same_bits(heads[3][1], att[1][1][0].reshape(b * n, 256))
    assert TD.same_bits(pred["Xo_pred"], heads[2][2].view(b, n, 3)) and TD.same_bits(pred["Yc_pred"], heads[3][2].view(b, n, 3))
    # the pooling
    (pool,) = recs["ConfPoolPmFn"].calls
    l1, l2, F1, F2 = pool[0]
    assert tuple(l1.shape) == (b, n) and tuple(F1.shape) == (b * n, 1024) and tuple(F2.shape) == (b * n, 1024)
    assert TD.same_bits(l1, heads[0][2].view(b, n)) and TD.same_bits(l2, heads[1][2].view(b, n))
    conf, pooled = A.ConfPoolPmFn.apply(*(t.detach().clone() for t in pool[0]))
    assert tuple(pred["conf"].shape) == (b, 2 * n) and TD.same_bits(pred["conf"], conf)
    assert tuple(seen["rot_in"].shape) == (b, 1024, 1) and TD.same_bits(seen["rot_in"], pooled.unsqueeze(2))
    # keys, shapes and dtypes of a "modules" instance
    ref_net = _net(dcl, n, train_attention="fused").train()
    data2 = dcl.synth.make_batch(b, n, n)
    data2["flags"] = torch.tensor([0.0, 1.0])
    want = ref_net(data2)
    assert list(pred.keys()) == list(want.keys())
    for name in want:
        assert tuple(pred[name].shape) == tuple(want[name].shape) and pred[name].dtype == want[name].dtype, name
    assert list(net.state_dict().keys()) == list(ref_net.state_dict().keys())
    loss = dcl.DCL_Net.losses(None)(pred, data["labels"])["loss_all"]
    loss.backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss))
    bad = [name for name, p in net.named_parameters() if p.grad is None or not bool(torch.isfinite(p.grad).all())]
    assert bad == []
    for m in (net.neck_fuser.layers[0], net.neck_fuser_bi.layers[6], net.disengage_Xc_p1[0].layers[0], net.disengage_Yo_m2[1].layers[0],
              net.regressor_conf.layers[0]):
        assert float(m.weight.grad.abs().sum()) > 0
    assert int(net.disengage_Xc_p1[0].layers[1].num_batches_tracked) == int(ref_net.disengage_Xc_p1[0].layers[1].num_batches_tracked)


def test_constructor_rules(dcl):
    cfg = dcl.synth.default_cfg(64, 64)
    with pytest.raises(ValueError, match="train_attention"):
        dcl.DCL_Net.Network(cfg, train_dense="point_major", train_attention="materialised")
    with pytest.raises(ValueError, match="train_dense"):
        dcl.DCL_Net.Network(cfg, train_dense="channel_minor", train_attention="fused")


def test_eval_mode_does_not_read_train_dense(dcl):
    b, n = 2, 256
    for fused in (True, False):
        outs = []
        for form in ("modules", "point_major"):
            net = _net(dcl, n, "test", train_dense=form, train_attention="fused", graph_max_batch=0, fused=fused).eval()
            with torch.no_grad():
                pred = net(dcl.synth.make_batch(b, n, n))
            torch.cuda.synchronize()
            outs.append({name: v.clone() for name, v in pred.items() if torch.is_tensor(v)})
        assert outs[0].keys() == outs[1].keys() and {"rot_pred", "trans_pred", "conf"} <= set(outs[0])
        for name in outs[0]:
            assert TD.same_bits(outs[0][name].float(), outs[1][name].float()), (fused, name)
