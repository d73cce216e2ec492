"""train_heads="kernels" on the GPU: the narrow per-point layer (csrc/linear_narrow.hip) and the two pose heads in training
(csrc/pose_heads_grad.hip) equal their host twins bit for bit and repeat bit for bit; autograd.NarrowLinearFn / PoseHeadsFn
against float64 under the project's rule; the pose heads' launch budget through the diagnostic library's census; the wiring of
Network and Refiner without a tolerance; eval mode never reads the switch.  tests/heads_cases.py holds the shapes, the operands
and the float64 twins; the host twins' own checks are in tests/test_heads_abi.py."""
import pytest
import torch

import heads_cases as H
import test_heads_abi as HA
import train_dense_cases as TD

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------- the narrow layer
def _narrow_gpu(dcl, k, form="dense", need=(True, True, True)):
    x = H.narrow_x(k["x"].cuda(), form)
    W, bias, g = k["W"].cuda(), k["bias"].cuda(), k["g"].cuda()
    out = {"y": dcl.ops.linear_narrow(x, W, bias)}
    dx, dW, db = dcl.ops.linear_narrow_backward(x, W, g, *need)
    out.update(dx=dx, dW=None if dW is None else dW.view_as(W), db=db)
    return out


@pytest.mark.parametrize("exact", [False, True], ids=["random", "exact"])
@pytest.mark.parametrize("i", range(len(H.NARROW_SHAPES)), ids=H.NARROW_IDS)
def test_narrow_kernels_equal_the_host_twin_in_every_form_and_repeat(dcl, i, exact):
    """16-byte accesses (dense), float-by-float ones (a pitch that is no multiple of 4, an address off 16-byte alignment) and the
    host twin give the same bits; so does a second call"""
    k = H.narrow_case(i, exact)
    want = HA.narrow_host(dcl, k)
    for form in H.NARROW_FORMS:
        got, again = _narrow_gpu(dcl, k, form), _narrow_gpu(dcl, k, form)
        for name in H.NARROW_OUT:
            assert H.same_bits(got[name], want[name]), (form, name, float((got[name].cpu() - want[name]).abs().max()))
            assert H.same_bits(again[name], got[name]), (form, name)


@pytest.mark.parametrize("i", [3, 4], ids=H.NARROW_IDS[3:5])
def test_narrow_kernels_give_each_subset_of_gradients_the_full_call_s_bits(dcl, i):
    k = H.narrow_case(i)
    full = _narrow_gpu(dcl, k)
    for need in ((True, False, False), (False, True, False), (False, False, True), (True, True, False), (False, True, True)):
        for form in ("dense", "strided"):
            got = _narrow_gpu(dcl, k, form, need)
            for name, want in zip(("dx", "dW", "db"), need):
                assert (got[name] is not None) == want and (not want or H.same_bits(got[name], full[name])), (need, form, name)
    assert H.same_bits(dcl.ops.linear_narrow(k["x"].cuda(), k["W"].cuda(), None) + k["bias"].cuda(), full["y"])


def _narrow_fn(dcl, k, form="dense", need=(True, True, True), view_grad=False):
    x = H.narrow_x(k["x"].cuda(), form).detach().requires_grad_(need[0])
    W, bias = k["W"].cuda().requires_grad_(need[1]), k["bias"].cuda().requires_grad_(need[2])
    y = dcl.autograd.NarrowLinearFn.apply(x, W, bias)
    g = k["g"].cuda()
    if view_grad:                                            # the gradient arrives as a column block of a wider matrix
        pad = torch.zeros((g.shape[0], 5), device="cuda")
        (torch.cat([pad, y], dim=1) * torch.cat([pad, g], dim=1)).sum().backward()
    else:
        y.backward(g)
    return dict(y=y.detach(), dx=x.grad, dW=W.grad, db=bias.grad)


@pytest.mark.parametrize("i", range(len(H.NARROW_SHAPES)), ids=H.NARROW_IDS)
def test_narrow_linear_fn_against_float64(dcl, i):
    k = H.narrow_case(i)
    got = _narrow_fn(dcl, k)
    assert got["dW"].shape == k["W"].shape
    ref = H.narrow_form(k, torch.float64)
    H.compare(H.NARROW_IDS[i], got, ref, H.narrow_form(k, torch.float32), ref, H.NARROW_OUT)
    for other in (_narrow_fn(dcl, k), _narrow_fn(dcl, k, "strided"), _narrow_fn(dcl, k, view_grad=True)):
        for name in H.NARROW_OUT:
            assert H.same_bits(other[name], got[name]), name
    only_w = _narrow_fn(dcl, k, need=(False, True, False))
    assert only_w["dx"] is None and only_w["db"] is None and H.same_bits(only_w["dW"], got["dW"])
    W2 = k["W"][:, :, 0].cuda().requires_grad_(True)          # W as (N, K)
    dcl.autograd.NarrowLinearFn.apply(k["x"].cuda(), W2, None).backward(k["g"].cuda())
    assert W2.grad.shape == W2.shape and H.same_bits(W2.grad, got["dW"][:, :, 0])


# ---------------------------------------------------------------------------------------------------- the pose heads
def _pose_gpu(dcl, k, need_x=True, need_params=True):
    P = [p.cuda() for p in H.pose_params(k)]
    x = k["x"].cuda()
    o9, t3, h1, h2 = dcl.ops.pose_heads_train(x, P)
    dx, grads = dcl.ops.pose_heads_train_backward(x, P, h1, h2, k["g_o9"].cuda(), k["g_t3"].cuda(), need_x, need_params)
    out = {"o9": o9, "t3": t3, "dx": dx, "h1": h1, "h2": h2}
    out.update({"d_" + n: g for n, g in zip(H.PARAMS, grads)})
    return out


@pytest.mark.parametrize("exact", [False, True], ids=["random", "exact"])
@pytest.mark.parametrize("b", H.POSE_B, ids=H.POSE_IDS)
def test_pose_kernels_equal_the_host_twin_and_repeat(dcl, b, exact):
    k = H.pose_case(b, exact)
    want, got, again = HA.pose_host(dcl, k), _pose_gpu(dcl, k), _pose_gpu(dcl, k)
    for name in H.POSE_OUT + ("h1", "h2"):
        assert H.same_bits(got[name], want[name]), (name, float((got[name].cpu() - want[name]).abs().max()))
        assert H.same_bits(again[name], got[name]), name


def test_pose_kernels_subsets_and_a_crop_alone(dcl):
    k = H.pose_case(33)
    full = _pose_gpu(dcl, k)
    only_x = _pose_gpu(dcl, k, need_params=False)
    assert H.same_bits(only_x["dx"], full["dx"]) and all(only_x["d_" + n] is None for n in H.PARAMS)
    need = tuple(n in ("rW2", "tb1", "tW0", "rb0") for n in H.PARAMS)
    some = _pose_gpu(dcl, k, need_x=False, need_params=need)
    assert some["dx"] is None
    for n, want in zip(H.PARAMS, need):
        assert (some["d_" + n] is not None) == want and (not want or H.same_bits(some["d_" + n], full["d_" + n])), n
    last = _pose_gpu(dcl, k, need_x=False, need_params=tuple(n[1:] in ("W2", "b2") for n in H.PARAMS))
    assert H.same_bits(last["d_rW2"], full["d_rW2"]) and H.same_bits(last["d_tb2"], full["d_tb2"])
    for c in (0, 17, 32):
        alone = _pose_gpu(dcl, H.pose_crop(k, c))
        for name in ("o9", "t3", "dx"):
            assert H.same_bits(alone[name], full[name][c:c + 1]), (c, name)


def _pose_fn(dcl, k, view_grad=False):
    x = k["x"].cuda().requires_grad_(True)
    P = [p.cuda().requires_grad_(True) for p in H.pose_params(k)]
    o9, t3 = dcl.autograd.PoseHeadsFn.apply(x, *P)
    g9, g3 = k["g_o9"].cuda(), k["g_t3"].cuda()
    if view_grad:                                            # both gradients arrive as column blocks of one wider matrix
        (torch.cat([o9, t3], dim=1) * torch.cat([g9, g3], dim=1)).sum().backward()
    else:
        torch.autograd.backward([o9, t3], [g9, g3])
    out = {"o9": o9.detach(), "t3": t3.detach(), "dx": x.grad}
    out.update({"d_" + n: p.grad for n, p in zip(H.PARAMS, P)})
    return out


@pytest.mark.parametrize("b", H.POSE_B, ids=H.POSE_IDS)
def test_pose_heads_fn_against_float64(dcl, b):
    k = H.pose_case(b)
    got = _pose_fn(dcl, k)
    for n in H.PARAMS:
        assert got["d_" + n].shape == k[n].shape, n
    _, _, h1, h2 = dcl.ops.pose_heads_train(k["x"].cuda(), [p.cuda() for p in H.pose_params(k)])
    mod32 = H.pose_form(k, torch.float32)
    H.compare("b%d" % b, got, H.pose_form(k, torch.float64, H.pose_masks(h1, h2)), mod32,
              H.pose_form(k, torch.float64, mod32["masks"]), H.POSE_OUT)
    for other in (_pose_fn(dcl, k), _pose_fn(dcl, k, view_grad=True)):
        for name in H.POSE_OUT:
            assert H.same_bits(other[name], got[name]), name


def test_pose_heads_fn_launch_budget(request, dcl):
    """counted through the diagnostic library's launch census: at most 3 library launches forward, 6 backward"""
    import test_gpu_ops as TO
    import test_kernel_census as TC
    k = H.pose_case(33)
    x = k["x"].cuda().requires_grad_(True)
    P = [p.cuda().requires_grad_(True) for p in H.pose_params(k)]
    g9, g3 = k["g_o9"].cuda(), k["g_t3"].cuda()
    lib = TO.enter_diag(dcl, request)
    lib.dcl_debug_launch_census_reset()
    o9, t3 = dcl.autograd.PoseHeadsFn.apply(x, *P)
    torch.cuda.synchronize()
    fwd = {name: c for name, c in TC.census(lib).items() if c > 0}
    assert 1 <= sum(fwd.values()) <= 3 and all(name.startswith("k_ph_") for name in fwd), fwd
    lib.dcl_debug_launch_census_reset()
    torch.autograd.backward([o9, t3], [g9, g3])
    torch.cuda.synchronize()
    bwd = {name: c for name, c in TC.census(lib).items() if c > 0}
    assert 1 <= sum(bwd.values()) <= 6 and all(name.startswith("k_ph_") for name in bwd), bwd
    assert x.grad is not None and all(p.grad is not None for p in P)


# ---------------------------------------------------------------------------------------------------- wiring
def _net(dcl, n, mode="train", **kw):
    net = dcl.DCL_Net.Network(dcl.synth.default_cfg(n, n), mode=mode, **kw)
    net.load_state_dict(dcl.synth.synth_state_dict(net, 1))
    return net.cuda()


def _record(dcl, monkeypatch, module, *names):
    recs = {}
    for name in names:
        recs[name] = TD.Recorder(getattr(dcl.autograd, name))
        monkeypatch.setattr(module, name, recs[name])
    return recs


def test_network_wiring_of_train_heads_kernels(dcl, monkeypatch):
    """no tolerance: what the switch hands to NarrowLinearFn and PoseHeadsFn, recomputed stand-alone"""
    b, n = 2, 256
    net = _net(dcl, n, train_dense="point_major", train_attention="fused", train_heads="kernels").train()
    data = dcl.synth.make_batch(b, n, n)
    data["flags"] = torch.tensor([0.0, 1.0])
    recs = _record(dcl, monkeypatch, dcl.DCL_Net, "NarrowLinearFn", "PoseHeadsFn", "ConfPoolPmFn")
    called = []
    hooks = [m.register_forward_pre_hook(lambda m, a: called.append(m)) for m in (net.regressor_rot, net.regressor_trans)]
    pred = net(data)
    for h in hooks:
        h.remove()
    assert called == []                                       # the registered pose-head modules are not called
    A = dcl.autograd
    narrow = recs["NarrowLinearFn"].calls
    assert len(narrow) == 4
    for (x, W, bias), y in narrow:
        assert x.dim() == 2 and x.shape[0] == b * n and tuple(y.shape) == (b * n, W.shape[0])
        assert TD.same_bits(y, A.NarrowLinearFn.apply(x.detach().clone(), W.detach().clone(), bias.detach().clone()))
    heads = (net.regressor_conf, net.regressor_conf_bi, net.regressor_Xo, net.regressor_Yc)
    for ((x, W, bias), y), head in zip(narrow, heads):
        assert W is head.layers[4].weight and bias is head.layers[4].bias
    (pool,) = recs["ConfPoolPmFn"].calls
    assert TD.same_bits(pool[0][0], narrow[0][1].view(b, n)) and TD.same_bits(pool[0][1], narrow[1][1].view(b, n))
    assert TD.same_bits(pred["Xo_pred"], narrow[2][1].view(b, n, 3)) and TD.same_bits(pred["Yc_pred"], narrow[3][1].view(b, n, 3))
    (pose,) = recs["PoseHeadsFn"].calls
    args, (o9, t3) = pose
    assert TD.same_bits(args[0], pool[1][1]) and tuple(args[0].shape) == (b, 1024)           # on pooled
    want = dcl.DCL_Net.pose_head_params(net.regressor_rot, net.regressor_trans)
    assert len(args) == 13 and all(u is v for u, v in zip(args[1:], want))                   # the registered tensors: no copies
    w9, w3 = A.PoseHeadsFn.apply(*(t.detach().clone() for t in args))
    assert TD.same_bits(o9, w9) and TD.same_bits(t3, w3) and TD.same_bits(pred["trans_pred"], t3)
    assert TD.same_bits(pred["rot_pred"], dcl.DCL_Net.ortho9d2matrix(o9[:, :3], o9[:, 3:6], o9[:, 6:]).detach())
    # keys, shapes and dtypes of a "modules" instance
    ref_net = _net(dcl, n, train_dense="point_major", train_attention="fused").train()
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
    for m in [h.layers[4] for h in heads] + [net.regressor_rot.layers[0], net.regressor_trans.layers[0]]:
        assert float(m.weight.grad.abs().sum()) > 0


@pytest.mark.parametrize("mlp", ["modules", "kernels"])
def test_refiner_wiring_of_train_heads_kernels(dcl, monkeypatch, mlp):
    b, n = 2, 128
    mk = lambda **kw: dcl.refiner.Refiner(train_rotation="device", train_mlp=mlp, **kw)       # noqa: E731
    ref = mk(train_heads="kernels")
    ref.load_state_dict(dcl.synth.synth_state_dict(ref, 2))
    ref = ref.cuda().train()
    g = torch.Generator().manual_seed(3)
    x = torch.cat([torch.randn(b, 3, n, generator=g) * 0.05, torch.randn(b, 256, n, generator=g)], 1).cuda()
    conf = torch.rand(b, n, generator=g).cuda()
    rec = TD.Recorder(dcl.autograd.PoseHeadsFn)
    monkeypatch.setattr(dcl.autograd, "PoseHeadsFn", rec)
    called = []
    hooks = [m.register_forward_pre_hook(lambda m, a: called.append(m)) for m in (ref.regressor_rot2, ref.regressor_trans2)]
    out = ref({"input_features": x, "conf": conf, "obj_idx": None})
    for h in hooks:
        h.remove()
    assert called == [] and len(rec.calls) == 1
    args, (o9, t3) = rec.calls[0]
    assert tuple(args[0].shape) == (b, 1024)
    want = dcl.DCL_Net.pose_head_params(ref.regressor_rot2, ref.regressor_trans2)
    assert len(args) == 13 and all(u is v for u, v in zip(args[1:], want))
    w9, w3 = rec.fn.apply(*(t.detach().clone() for t in args))
    assert TD.same_bits(o9, w9) and TD.same_bits(t3, w3) and TD.same_bits(out["trans_pred"], t3)
    assert TD.same_bits(out["rot_pred"], dcl.DCL_Net.ortho9d2matrix(o9[:, :3], o9[:, 3:6], o9[:, 6:], "device").detach())
    other = mk()
    other.load_state_dict(ref.state_dict())
    other = other.cuda().train()
    want_out = other({"input_features": x, "conf": conf, "obj_idx": None})
    assert list(out.keys()) == list(want_out.keys()) and list(ref.state_dict().keys()) == list(other.state_dict().keys())
    for name in want_out:
        assert tuple(out[name].shape) == tuple(want_out[name].shape) and out[name].dtype == want_out[name].dtype, name
    (out["trans_pred"].sum() + out["rot_pred"].sum()).backward()
    torch.cuda.synchronize()
    bad = [name for name, p in ref.named_parameters() if p.grad is None or not bool(torch.isfinite(p.grad).all())]
    assert bad == []
    assert float(ref.regressor_rot2.layers[0].weight.grad.abs().sum()) > 0
    assert float(ref.regressor_trans2.layers[0].weight.grad.abs().sum()) > 0
    # an optimizer step is seen at once: no cached weights
    with torch.no_grad():
        ref.regressor_trans2.layers[4].bias.add_(1.0)
    moved = ref({"input_features": x, "conf": conf, "obj_idx": None})
    assert float((moved["trans_pred"] - out["trans_pred"] - 1.0).detach().abs().max()) < 1e-5


def test_eval_mode_does_not_read_train_heads(dcl):
    b, n = 2, 256
    outs = []
    for form in ("modules", "kernels"):
        net = _net(dcl, n, "test", train_dense="point_major", train_attention="fused", train_heads=form, graph_max_batch=0).eval()
        with torch.no_grad():
            pred = net(dcl.synth.make_batch(b, n, n))
        torch.cuda.synchronize()
        outs.append({name: v.clone() for name, v in pred.items() if torch.is_tensor(v)})
    assert outs[0].keys() == outs[1].keys() and {"rot_pred", "trans_pred", "conf"} <= set(outs[0])
    for name in outs[0]:
        assert TD.same_bits(outs[0][name].float(), outs[1][name].float()), name
    g = torch.Generator().manual_seed(5)
    x = torch.cat([torch.randn(b, 3, n, generator=g) * 0.05, torch.randn(b, 256, n, generator=g)], 1).cuda()
    conf = torch.rand(b, n, generator=g).cuda()              # one confidence per point: conf[:, :1024] is the whole row
    outs = []
    for form in ("modules", "kernels"):
        ref = dcl.refiner.Refiner(train_heads=form)
        ref.load_state_dict(dcl.synth.synth_state_dict(ref, 2))
        ref = ref.cuda().eval()
        outs.append(ref({"input_features": x, "conf": conf, "obj_idx": None}))
    for name in outs[0]:
        assert TD.same_bits(outs[0][name], outs[1][name]), name
