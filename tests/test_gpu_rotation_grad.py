"""The rotation head's gradient on the GPU (csrc/rotation_grad.hip behind autograd.Ortho9dFn): the forward is the eval kernel
bit for bit, the gradient meets the float64 references of tests/rotation_cases.py on every input class and batch size, is
repeatable, takes a strided upstream gradient, never synchronises the host, and trains Network and Refiner to the same
gradients as the host composition where that one is still sound."""
import pytest
import torch

import rotation_cases as RC

pytestmark = pytest.mark.gpu

BATCHES = (1, 63, 64, 65, 130)          # a partial wave, a full one, a second workgroup of one lane, two full ones and a tail


def _device_grad(dcl, o9, G):
    leaf = o9.cuda().requires_grad_(True)
    R = dcl.autograd.Ortho9dFn.apply(leaf)
    R.backward(G.cuda())
    return R.detach(), leaf.grad


@pytest.mark.parametrize("cls", RC.ALL_CLASSES)
def test_forward_is_the_eval_kernel_bit_for_bit(dcl, cls):
    o9, _ = RC.inputs(cls, 65)
    leaf = o9.cuda().requires_grad_(True)
    R = dcl.autograd.Ortho9dFn.apply(leaf)
    assert R.requires_grad and torch.equal(R.detach(), dcl.ops.ortho9d_to_matrix(o9.cuda()))
    x = o9.cuda().requires_grad_(True)
    via_model = dcl.DCL_Net.ortho9d2matrix(x[:, :3], x[:, 3:6], x[:, 6:], "device")
    assert via_model.requires_grad and torch.equal(via_model.detach(), R.detach())


@pytest.mark.parametrize("b", BATCHES)
def test_device_gradient_matches_the_float64_references(dcl, b):
    """same references, classes and bounds as tests/test_rotation_grad_abi.py; every crop counts"""
    twin = 0.0
    for cls in RC.ALL_CLASSES:
        o9, G = RC.inputs(cls, b)
        _, got = _device_grad(dcl, o9, G)
        got = got.cpu()
        ratio = RC.worst_ratio(got, cls, b)
        host = dcl.ops.ortho9d_backward_host(o9, G)
        twin = max(twin, float(((got - host).abs().amax(dim=1) / host.abs().amax(dim=1)).max()))
        print("rotation grad, device, b = %3d, %-18s worst error / max|grad| = %.3g (bound %.0e)" % (b, cls, ratio, RC.bound(cls)))
        assert torch.isfinite(got).all(), cls
        assert ratio <= RC.bound(cls), (cls, b, ratio)
    print("rotation grad, device vs host twin, b = %3d: largest difference / max|grad| = %.3g" % (b, twin))


def test_two_calls_give_the_same_bits(dcl):
    for cls in ("gaussian", "ortho_noise_1e-6", "left_handed"):
        o9, G = [t.cuda() for t in RC.inputs(cls, 130)]
        a = dcl.ops.ortho9d_backward(o9, G)
        b = dcl.ops.ortho9d_backward(o9, G)
        assert torch.equal(a, b), cls
        assert torch.equal(_device_grad(dcl, o9, G)[1], a), cls


def test_a_transposed_upstream_gradient_is_handled(dcl):
    o9, G = [t.cuda() for t in RC.inputs("gaussian", 65)]
    want = dcl.ops.ortho9d_backward(o9, G)
    leaf = o9.clone().requires_grad_(True)
    Gt = G.transpose(1, 2).contiguous().transpose(1, 2)          # the same values behind a transposed view
    assert not Gt.is_contiguous() and torch.equal(Gt, G)
    dcl.autograd.Ortho9dFn.apply(leaf).backward(Gt)
    assert torch.equal(leaf.grad, want)
    # and produced by autograd itself: the loss reads R^T
    leaf2 = o9.clone().requires_grad_(True)
    (dcl.autograd.Ortho9dFn.apply(leaf2).transpose(1, 2) * G.transpose(1, 2)).sum().backward()
    assert torch.equal(leaf2.grad, want)


def test_non_finite_crops_and_degenerate_axes_on_the_device(dcl):
    o9, G = [t.clone() for t in RC.inputs("gaussian", 70)]
    o9[3, 4] = float("nan")
    o9[66, 0] = float("inf")
    o9[10] = 0.0                                                  # all zeros
    o9[11, 3:] = o9[11, :3].repeat(2)                             # three parallel axes
    o9[12, 3:6] = 0.0                                             # one zero axis
    got = dcl.ops.ortho9d_backward(o9.cuda(), G.cuda()).cpu()
    assert torch.isnan(got[3]).all() and torch.isnan(got[66]).all()
    keep = [i for i in range(70) if i not in (3, 66)]
    assert torch.isfinite(got[keep]).all()
    assert torch.equal(got[keep], dcl.ops.ortho9d_backward(o9[keep].cuda(), G[keep].cuda()).cpu())


def _steps(dcl, b=65):
    o9, G = [t.cuda() for t in RC.inputs("gaussian", b)]

    def device_step(leaf=None):
        leaf = o9.clone().requires_grad_(True) if leaf is None else leaf
        R = dcl.autograd.Ortho9dFn.apply(leaf)
        R.backward(G)
        return R.detach(), leaf.grad

    def host_step():
        leaf = o9.clone().requires_grad_(True)
        R = dcl.DCL_Net.ortho9d2matrix(leaf[:, :3], leaf[:, 3:6], leaf[:, 6:], "host")
        R.backward(G)
        return R.detach(), leaf.grad

    return o9, device_step, host_step


def assert_capturable(dcl):
    """forward + backward of Ortho9dFn in one single-stream graph: capture succeeds and a replay equals the eager result"""
    o9, device_step, _ = _steps(dcl)
    want_R, want_g = device_step()
    static = o9.clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            static.grad = None
            device_step(static)
    torch.cuda.current_stream().wait_stream(side)
    static.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        R, g = device_step(static)
    R.zero_()
    g.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(R, want_R) and torch.equal(g, want_g)


def test_forward_and_backward_never_synchronise_the_host(dcl):
    """Under set_sync_debug_mode("error") the device path runs clean and the host composition raises (its .cpu() copy), which
    shows the mode sees a synchronisation.  Where this torch build does not honour the mode, capturability stands in."""
    _, device_step, host_step = _steps(dcl)
    want_R, want_g = device_step()                                # (first use outside the checked region: library load)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got_R, got_g = device_step()
        try:
            host_step()
            honoured = False
        except RuntimeError:
            honoured = True
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert torch.equal(got_R, want_R) and torch.equal(got_g, want_g)
    print("rotation grad: sync debug mode %s by this torch build" % ("honoured" if honoured else "NOT honoured: graph capture instead"))
    if not honoured:
        assert_capturable(dcl)


def _conditioning(o9):
    """singular values of the normalised axes of every crop, (b, 3) -- for the report when a comparison with the host mode fails"""
    m = o9.detach().double().cpu().view(-1, 3, 3)
    m = m / (m.norm(dim=2, keepdim=True) + 1e-8)
    return torch.linalg.svdvals(m)


def _compare_modes(make, run, head):
    """make(mode) -> module on the GPU in train(); run(module) -> rot_pred after loss.backward().  The device instance against
    the host instance: rot_pred within 1e-5, all gradients finite, a second run bit-identical, the rotation head's three
    layers within 1e-4 max|grad_host| (generic, well-conditioned o9: the host composition is sound there)."""
    seen = {}
    nets = {}
    for mode in ("host", "device"):
        net = make(mode)
        hook = getattr(net, head).register_forward_hook(lambda mod, inp, out, mode=mode: seen.__setitem__(mode, out.detach()))
        rot = run(net)
        hook.remove()
        nets[mode] = (net, rot.detach().clone(), {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None})
    net_d, rot_d, grads_d = nets["device"]
    _, rot_h, grads_h = nets["host"]
    assert float((rot_d - rot_h).abs().max()) <= 1e-5
    assert len(grads_d) == len(list(net_d.parameters())) and sorted(grads_d) == sorted(grads_h)
    assert all(bool(torch.isfinite(g).all()) for g in grads_d.values())
    for p in net_d.parameters():
        p.grad = None
    run(net_d)
    again = {k: p.grad for k, p in net_d.named_parameters()}
    differ = [k for k in grads_d if not torch.equal(grads_d[k], again[k])]
    assert differ == [], differ
    names = [k for k in grads_d if k.startswith(head + ".")]
    assert len(names) == 6, names                                 # weight and bias of the head's three layers
    worst = 0.0
    for k in names:
        scale = float(grads_h[k].abs().max())
        assert scale > 0, k
        worst = max(worst, float((grads_d[k] - grads_h[k]).abs().max()) / scale)
    print("rotation grad, %s: device vs host mode, largest difference / max|grad_host| = %.3g (bound 1e-4)" % (head, worst))
    assert worst <= 1e-4, (worst, "singular values of the normalised axes per crop:", _conditioning(seen["device"]).tolist())


def test_network_trains_with_the_device_rotation_gradient(dcl):
    b, n = 2, 256
    data = dcl.synth.make_batch(b, n, n)
    data["flags"] = torch.tensor([0.0, 1.0])
    crit = dcl.DCL_Net.losses(None)

    def make(mode):
        net = dcl.DCL_Net.Network(dcl.synth.default_cfg(n, n), mode="train", train_rotation=mode)
        net.load_state_dict(dcl.synth.synth_state_dict(net, 1))
        return net.cuda().train()

    def run(net):
        pred = net(data)
        crit(pred, data["labels"])["loss_all"].backward()
        torch.cuda.synchronize()
        return pred["rot_pred"]

    _compare_modes(make, run, "regressor_rot")


def test_refiner_trains_with_the_device_rotation_gradient(dcl):
    b, n = 2, 1024
    g = torch.Generator().manual_seed(4)
    rot = lambda: torch.linalg.qr(torch.randn(b, 3, 3, generator=g))[0]                  # noqa: E731
    x = torch.cat([torch.randn(b, 3, n, generator=g) * 0.05, torch.randn(b, 256, n, generator=g)], 1).cuda()
    conf = torch.rand(b, 2 * n, generator=g).cuda()
    R, t = rot().cuda(), (torch.randn(b, 3, generator=g) * 0.01).cuda()
    gt = {"rot_gt": rot().cuda(), "trans_gt": (torch.randn(b, 3, generator=g) * 0.01).cuda()}
    tmp, sym = (torch.randn(b, 500, 3, generator=g) * 0.05).cuda(), torch.tensor([0.0, 1.0]).cuda()
    crit = dcl.refiner.losses_refiner(None)

    def make(mode):
        ref = dcl.refiner.Refiner(train_rotation=mode)
        ref.load_state_dict(dcl.synth.synth_state_dict(ref, 2))
        return ref.cuda().train()

    def run(ref):
        out = ref({"input_features": x, "conf": conf, "obj_idx": None})
        crit(out, t, R, tmp, sym, gt)["loss_all"].backward()
        torch.cuda.synchronize()
        return out["rot_pred"]

    _compare_modes(make, run, "regressor_rot2")
