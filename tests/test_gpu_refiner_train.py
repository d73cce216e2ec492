"""Refiner(train_mlp="kernels") on the GPU: the shared MLP trained through autograd.RefinerShareFn (own GEMM core forward,
own weight-gradient GEMM and ReLU / bias kernels backward) against the registered-module composition and against a
float64 run of it; determinism, accumulation, optimizer steps being seen, the refusals, and eval mode left alone."""
import copy
import importlib

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(2, 128, 128), (3, 256, 256), (2, 1024, 2048)]          # (b, n, width of conf)


def _inputs(b, n, nconf, seed=4):
    g = torch.Generator().manual_seed(seed)
    rot = lambda: torch.linalg.qr(torch.randn(b, 3, 3, generator=g))[0]                  # noqa: E731
    x = torch.cat([torch.randn(b, 3, n, generator=g) * 0.05, torch.randn(b, 256, n, generator=g)], 1).cuda()
    conf = torch.rand(b, nconf, generator=g).cuda()
    R, t = rot().cuda(), (torch.randn(b, 3, generator=g) * 0.01).cuda()
    gt = {"rot_gt": rot().cuda(), "trans_gt": (torch.randn(b, 3, generator=g) * 0.01).cuda()}
    tmp = (torch.randn(b, 500, 3, generator=g) * 0.05).cuda()
    sym = torch.tensor([0.0, 1.0, 0.0][:b]).cuda()
    return x, conf, (t, R, tmp, sym, gt)


def _make(dcl, train_mlp, state=None, rotation="device"):
    ref = dcl.refiner.Refiner(train_rotation=rotation, train_mlp=train_mlp)
    ref.load_state_dict(state if state is not None else dcl.synth.synth_state_dict(ref, 2))
    return ref.cuda().train()


def _step(dcl, ref, x, conf, labels, zero=True, dtype=torch.float32):
    """forward + losses_refiner + backward -> (outputs, gradients by name)"""
    if zero:
        for p in ref.parameters():
            p.grad = None
    cast = lambda v: v.to(dtype) if torch.is_tensor(v) else {k: w.to(dtype) for k, w in v.items()}     # noqa: E731
    out = ref({"input_features": x.to(dtype), "conf": conf.to(dtype), "obj_idx": None})
    dcl.refiner.losses_refiner(None)(out, *[cast(v) for v in labels])["loss_all"].backward()
    torch.cuda.synchronize()
    return ({k: v.detach().clone() for k, v in out.items()}, {k: p.grad.clone() for k, p in ref.named_parameters()})


@pytest.fixture(scope="module")
def runs():
    """per shape, once: both forms' outputs and gradients and the float64 gradients of the module composition"""
    dcl = importlib.import_module("dcl-net_amd")
    res = {}
    for b, n, nconf in SHAPES:
        x, conf, labels = _inputs(b, n, nconf)
        r = {"inputs": (x, conf, labels)}
        for form in ("modules", "kernels"):
            ref = _make(dcl, form)
            r[form] = _step(dcl, ref, x, conf, labels)
            if form == "kernels":
                r["kernels again"] = _step(dcl, ref, x, conf, labels)
                r["ref"] = ref
        ref64 = _make(dcl, "modules", rotation="host").double()
        r["float64"] = _step(dcl, ref64, x, conf, labels, dtype=torch.float64)
        res[(b, n, nconf)] = r
    return res


@pytest.mark.parametrize("shape", SHAPES)
def test_outputs_match_the_module_form(runs, shape):
    out_m, out_k = runs[shape]["modules"][0], runs[shape]["kernels"][0]
    d_rot = float((out_k["rot_pred"] - out_m["rot_pred"]).abs().max())
    d_t = float((out_k["trans_pred"] - out_m["trans_pred"]).abs().max())
    scale = float(out_m["trans_pred"].abs().max())
    print("refiner train %s: |d rot| = %.3g (1e-5), |d trans| / max|trans| = %.3g (1e-4)" % (shape, d_rot, d_t / scale))
    assert d_rot <= 1e-5
    assert d_t <= 1e-4 * scale


@pytest.mark.parametrize("shape", SHAPES)
def test_all_gradients_match_float64(runs, shape):
    g64 = runs[shape]["float64"][1]
    assert len(g64) == 18
    for form in ("kernels", "modules"):
        grads = runs[shape][form][1]
        assert sorted(grads) == sorted(g64)
        worst, where = 0.0, None
        for k, g in grads.items():
            assert g.shape == g64[k].shape and g.dtype == torch.float32 and bool(torch.isfinite(g).all()), k
            scale = float(g64[k].abs().max())
            assert scale > 0, k
            ratio = float((g.double() - g64[k]).abs().max()) / scale
            if ratio > worst:
                worst, where = ratio, k
        print("refiner train %s, %s: worst |grad - grad64| / max|grad64| = %.3g at %s (bound 1e-4)" % (shape, form, worst, where))
        assert worst <= 1e-4, (form, where, worst)


@pytest.mark.parametrize("shape", SHAPES)
def test_gradients_are_bit_identical_run_to_run(runs, shape):
    first, again = runs[shape]["kernels"][1], runs[shape]["kernels again"][1]
    differ = [k for k in first if not torch.equal(first[k].view(torch.int32), again[k].view(torch.int32))]
    assert differ == [], differ


def test_two_iterations_accumulate_the_sum_of_their_gradients(dcl, runs):
    shape = SHAPES[1]
    ref = runs[shape]["ref"]
    x, conf, labels = runs[shape]["inputs"]
    x2 = x.clone()
    x2[:, :3] = x2[:, :3] * 0.5 + 0.01                               # the second iteration sees other points
    _, g1 = _step(dcl, ref, x, conf, labels)
    _, g2 = _step(dcl, ref, x2, conf, labels)
    for p in ref.parameters():
        p.grad = None
    _step(dcl, ref, x, conf, labels, zero=False)
    _, both = _step(dcl, ref, x2, conf, labels, zero=False)
    assert any(float((g1[k] - g2[k]).abs().max()) > 0 for k in g1)
    differ = [k for k in both if not torch.equal(both[k].view(torch.int32), (g1[k] + g2[k]).view(torch.int32))]
    assert differ == [], differ


@pytest.mark.parametrize("optimizer", ["dcl.optim.Adam", "torch.optim.Adam"])
def test_an_optimizer_step_is_seen(dcl, runs, optimizer):
    shape = SHAPES[0]
    x, conf, labels = runs[shape]["inputs"]
    ref = _make(dcl, "kernels")
    inp = {"input_features": x, "conf": conf, "obj_idx": None}
    before = ref(inp)["trans_pred"].detach().clone()
    _step(dcl, ref, x, conf, labels)
    opt = dcl.optim.Adam(ref.parameters(), lr=1e-3) if optimizer == "dcl.optim.Adam" else torch.optim.Adam(ref.parameters(), lr=1e-3)
    opt.step()
    after = {k: v.detach() for k, v in ref(inp).items()}              # no train() / eval() call in between
    fresh = _make(dcl, "kernels", state={k: v.detach().cpu() for k, v in ref.state_dict().items()})
    want = fresh(inp)
    for k in ("rot_pred", "trans_pred"):
        assert torch.equal(after[k].view(torch.int32), want[k].detach().view(torch.int32)), k
    assert float((after["trans_pred"] - before).abs().max()) > 1e-6


def test_refusals(dcl):
    ref = _make(dcl, "kernels")
    x, conf, _ = _inputs(2, 100, 100)
    with pytest.raises(ValueError, match="128"):
        ref({"input_features": x, "conf": conf, "obj_idx": None})
    x, conf, _ = _inputs(2, 128, 128)
    with pytest.raises(ValueError, match="require grad"):
        ref({"input_features": x.clone().requires_grad_(), "conf": conf, "obj_idx": None})
    F = dcl.autograd.RefinerShareFn
    L = ref.MLP_share.layers
    params = [L[0].weight, L[0].bias, L[2].weight, L[2].bias, L[4].weight, L[4].bias]
    xyz = torch.zeros(256, 3, device="cuda", requires_grad=True)
    with pytest.raises(ValueError, match="no gradient"):
        F.apply(xyz, torch.zeros(256, 256, device="cuda"), torch.zeros(2, 128, device="cuda"), *params)


def test_eval_mode_is_unchanged_by_the_switch(dcl, runs):
    x, conf, _ = runs[SHAPES[2]]["inputs"]
    inp = {"input_features": x, "conf": conf, "obj_idx": None}
    state = dcl.synth.synth_state_dict(dcl.refiner.Refiner(), 2)
    outs = [_make(dcl, form, state=copy.deepcopy(state)).eval()(inp) for form in ("modules", "kernels")]
    for k in ("rot_pred", "trans_pred"):
        assert torch.equal(outs[0][k].view(torch.int32), outs[1][k].view(torch.int32)), k
