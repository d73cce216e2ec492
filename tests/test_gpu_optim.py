"""dcl.optim on the GPU (csrc/optim.hip: ops.grad_sqnorm / ops.adam_step, optim.Adam, optim.AutoClip): the norm against exact
float64 sums, the update bit for bit against the five documented fp32 lines written out in numpy, the optimizer against
torch.optim.Adam (accuracy and state dicts, both ways), the version counters that Refiner._fold is keyed on, AutoClip in both
forms, and one real training step of Network.

Tensor set S: sizes that are 1, 3, 5 elements, one short of / exactly / one past a chunk, three chunks and a tail, and the
largest parameter of Network (216 chunks); the three-chunk tensor is a contiguous view that starts one element into its
storage (no 16-byte alignment: the scalar path on full chunks), and a further parameter never has a gradient."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
SIZES = [1, 3, 5, 4095, 4096, 4097, 3 * 4096 + 7, 884736]
VIEW = 6                                  # index of the parameter that is a view at element offset 1
U = 2.0 ** -53
SHIPPED = dict(lr=1e-3, betas=(0.5, 0.999), eps=1e-6)      # tools/train_YCBV_stage1.py's optimizer
f32 = np.float32


def make_params(seed=0):
    """S on the device (+ one parameter that never gets a gradient, last) and the same values as numpy arrays"""
    g = torch.Generator().manual_seed(seed)
    host = [torch.randn(n, generator=g) * 0.1 for n in SIZES] + [torch.randn(100, generator=g)]
    values = [h.numpy().copy() for h in host]
    params = []
    for i, h in enumerate(host):
        if i == VIEW:
            base = torch.zeros(h.numel() + 1, device=DEV)
            base[1:] = h.to(DEV)
            p = base[1:].detach().requires_grad_(True)
            assert p.data_ptr() % 16 == 4 and p.is_contiguous()
        else:
            p = h.clone().to(DEV).requires_grad_(True)
        params.append(p)
    return params, values


def make_grads(steps, seed=1, lo=-6.0):
    """a fixed gradient sequence: [step][tensor] numpy fp32, magnitudes from 1e-6 to 1 across tensors and steps"""
    g = torch.Generator().manual_seed(seed)
    mags = 10.0 ** np.linspace(lo, 0.0, len(SIZES))
    out = []
    for s in range(steps):
        out.append([(torch.randn(n, generator=g) * float(mags[(i + s) % len(SIZES)])).numpy() for i, n in enumerate(SIZES)])
    return out


def set_grads(params, grads_dev, skip=()):
    """a FRESH gradient allocation for every tensor (device-to-device copies: nothing here waits for the GPU)"""
    for i, p in enumerate(params):
        p.grad = None if (i >= len(grads_dev) or i in skip) else grads_dev[i].clone()


def upload(grads):
    return [[torch.from_numpy(a).to(DEV) for a in row] for row in grads]


def twin_step(p, g, m, v, t, lr, betas, eps, scale=1.0):
    """include/dclnet_hip.h at dcl_adam_step, written out: numpy fp32 arrays, every operation rounded on its own"""
    step_size = f32(lr / (1.0 - betas[0] ** t))
    bc2_sqrt = f32(math.sqrt(1.0 - betas[1] ** t))
    beta1, beta2, eps, scale = f32(betas[0]), f32(betas[1]), f32(eps), f32(scale)
    omb1, omb2 = f32(1.0 - float(beta1)), f32(1.0 - float(beta2))
    gs = g * scale
    m = m * beta1 + gs * omb1
    v = v * beta2 + (gs * gs) * omb2
    d = np.sqrt(v) / bc2_sqrt + eps
    p = p - step_size * (m / d)
    assert p.dtype == m.dtype == v.dtype == np.float32
    return p, m, v


class Twin(object):
    """the optimizer's state in numpy, stepped by twin_step"""

    def __init__(self, host, hyper):
        self.p = [h.copy() for h in host]
        self.m = [np.zeros_like(h) for h in host]
        self.v = [np.zeros_like(h) for h in host]
        self.t = [0] * len(host)
        self.hyper = hyper

    def step(self, grads, scale=1.0, skip=()):
        for i, g in enumerate(grads):
            if i in skip or g is None:
                continue
            self.t[i] += 1
            self.p[i], self.m[i], self.v[i] = twin_step(self.p[i], g, self.m[i], self.v[i], self.t[i], self.hyper["lr"],
                                                        self.hyper["betas"], self.hyper["eps"], scale)


def adam64(host, grads, hyper, steps=None):
    """torch.optim.Adam's formulas in float64 on the fp32 inputs"""
    lr, (b1, b2), eps = hyper["lr"], hyper["betas"], hyper["eps"]
    p = [h.astype(np.float64) for h in host[:len(SIZES)]]
    m = [np.zeros_like(x) for x in p]
    v = [np.zeros_like(x) for x in p]
    for t, row in enumerate(grads[:steps], 1):
        for i, g in enumerate(row):
            g = g.astype(np.float64)
            m[i] = b1 * m[i] + (1 - b1) * g
            v[i] = b2 * v[i] + (1 - b2) * g * g
            p[i] = p[i] - lr / (1 - b1 ** t) * m[i] / (np.sqrt(v[i]) / math.sqrt(1 - b2 ** t) + eps)
    return p


def deviation(params, ref64):
    """max |p - p64| over all tensors"""
    return max(float(np.abs(np.asarray(a, dtype=np.float64) - b).max()) for a, b in zip(params, ref64))


def cpu(ts):
    return [t.detach().cpu().numpy() for t in ts]


def exact_sq(g):
    """sum of g^2, correctly rounded: the products of fp32 values are exact in float64, fsum adds them exactly"""
    g = np.asarray(g, dtype=np.float64).ravel()
    return math.fsum((g * g).tolist())


@pytest.fixture(scope="module")
def torch_reference():
    """20 steps with the shipped hyper-parameters: the float64 run after 10 and 20 steps, and how far the installed
    torch.optim.Adam(foreach=False) in fp32 (on the CPU: the same figure on every machine) ends from it"""
    _, host = make_params()
    grads = make_grads(20)
    ref = {10: adam64(host, grads, SHIPPED, 10), 20: adam64(host, grads, SHIPPED, 20)}
    ps = [torch.from_numpy(h.copy()).requires_grad_(True) for h in host[:len(SIZES)]]
    opt = torch.optim.Adam(ps, foreach=False, **SHIPPED)
    dev = {}
    for s, row in enumerate(grads, 1):
        for p, g in zip(ps, row):
            p.grad = torch.from_numpy(g.copy())
        opt.step()
        if s in ref:
            dev[s] = deviation(cpu(ps), ref[s])
    return {"host": host, "grads": grads, "ref64": ref, "torch_dev": dev}


def test_norm_against_exact_float64_sums(dcl):
    params, _ = make_params()
    grads = make_grads(1)[0]
    set_grads(params, upload([grads])[0])
    opt = dcl.optim.Adam(params, **SHIPPED)
    sq, norm = opt.grad_norm()
    sq2, norm2 = opt.grad_norm()
    assert sq.dtype == torch.float64 and sq.shape == (len(SIZES),), "the parameter without a gradient is absent"
    got, got_norm = sq.cpu().numpy(), float(norm.cpu()[0])
    want = [exact_sq(g) for g in grads]
    for i, (n, g) in enumerate(zip(SIZES, grads)):
        rel = abs(got[i] - want[i]) / want[i]
        rel_np = abs(got[i] - float(np.sum(g.astype(np.float64) ** 2))) / want[i]
        print("numel %7d: rel. error %.3g against the exact sum, %.3g against numpy's float64 sum (bound %.3g)"
              % (n, rel, rel_np, n * U))
        assert rel <= n * U and rel_np <= n * U, n
    total = sum(SIZES)
    want_norm = math.sqrt(math.fsum(want))
    rel = abs(got_norm - want_norm) / want_norm
    print("norm: rel. error %.3g (bound %.3g)" % (rel, total * U))
    assert rel <= total * U
    assert torch.equal(sq, sq2) and torch.equal(norm, norm2), "two calls give the same bits"
    # the same data at another alignment gives the same bits: the scalar path keeps the vector path's summation order
    i = SIZES.index(4096)
    shifted = torch.zeros(4097, device=DEV)
    shifted[1:] = params[i].grad
    q = shifted[1:].detach().requires_grad_(True)
    q.grad = shifted[1:]
    sq_q, _ = dcl.optim.Adam([q], **SHIPPED).grad_norm()
    assert float(sq_q.cpu()[0]) == got[i]


def test_norm_of_a_table_past_the_finish_kernels_staging(dcl):
    """more chunks (6144) and more tensors (1024) than the second launch stages in LDS: the same ordered sums, from memory"""
    O = dcl.optim
    n_small, big = 6145, 3 * 4096 + 5
    g = torch.randn(n_small + big, generator=torch.Generator().manual_seed(7))
    gd = g.to(DEV)
    numels = [1] * n_small + [big]
    lay = O._Layout(numels, [len(numels)])
    assert lay.n_chunks == n_small + 4 and lay.n_tensors == n_small + 1
    host = lay.template.copy()
    tab = host[:lay.n_tensors * O.TENSOR_DTYPE.itemsize].view(O.TENSOR_DTYPE)
    tab["grad"] = gd.data_ptr() + 4 * np.arange(n_small + 1, dtype=np.uint64)
    tab["numel"] = numels
    sq, norm = dcl.ops.grad_sqnorm(*lay.views(torch.from_numpy(host).to(DEV)))
    sq, g64 = sq.cpu().numpy(), g.numpy().astype(np.float64)
    assert np.array_equal(sq[:n_small], g64[:n_small] ** 2), "one element: the exact square"
    want_big = exact_sq(g64[n_small:])
    assert abs(sq[-1] - want_big) <= big * U * want_big
    want = math.sqrt(exact_sq(g64))
    assert abs(float(norm.cpu()[0]) - want) <= len(g64) * U * want


@pytest.mark.parametrize("scale", [1.0, 0.37])
def test_update_is_the_documented_arithmetic_bit_for_bit(dcl, scale):
    params, host = make_params()
    grads = make_grads(3, seed=2)
    dev_grads = upload(grads)
    hyper = dict(lr=3e-3, betas=(0.9, 0.99), eps=1e-8)
    opt = dcl.optim.Adam(params, **hyper)
    twin = Twin(host, hyper)
    no_grad_in_step_2 = SIZES.index(4097)
    torch.cuda.synchronize()
    for s in range(3):                                                   # nothing in this loop waits for the GPU
        skip = (no_grad_in_step_2,) if s == 1 else ()
        set_grads(params, dev_grads[s], skip)
        opt.set_grad_scale(scale)
        opt.step()
        twin.step(grads[s], scale, skip)
    assert [int(opt.state[p]["step"]) for p in params[:len(SIZES)]] == twin.t[:len(SIZES)] and twin.t[no_grad_in_step_2] == 2
    assert params[-1] not in opt.state or len(opt.state[params[-1]]) == 0
    for i, p in enumerate(params[:len(SIZES)]):
        st = opt.state[p]
        for name, got, want in (("p", p, twin.p[i]), ("exp_avg", st["exp_avg"], twin.m[i]), ("exp_avg_sq", st["exp_avg_sq"], twin.v[i])):
            got = got.detach().cpu().numpy()
            bad = int((got.view(np.int32) != want.view(np.int32)).sum())
            assert bad == 0, "%s of numel %d: %d elements differ, max |d| %.3g" % (name, SIZES[i], bad, np.abs(got - want).max())
    assert np.array_equal(params[-1].detach().cpu().numpy(), host[-1])
    # the gradients were read only, and a scale handed over lasts for one step
    for p, g in zip(params[:len(SIZES)], grads[2]):
        assert np.array_equal(p.grad.cpu().numpy(), g)
    assert opt._grad_scale == 1.0


def test_twenty_steps_against_torch_adam(dcl, torch_reference):
    R = torch_reference
    params, _ = make_params()
    dev_grads = upload(R["grads"])
    opt = dcl.optim.Adam(params, **SHIPPED)
    for s in range(20):
        set_grads(params, dev_grads[s])
        opt.step()
    ours = deviation(cpu(params[:len(SIZES)]), R["ref64"][20])
    print("max |p - p64| after 20 steps: dcl.optim.Adam %.3g, torch.optim.Adam(foreach=False) %.3g, ratio %.3f (bound 2)"
          % (ours, R["torch_dev"][20], ours / R["torch_dev"][20]))
    assert ours <= 2.0 * R["torch_dev"][20]


def test_state_dicts_move_between_the_two_classes(dcl, torch_reference):
    R = torch_reference
    dev_grads = upload(R["grads"][:10])
    bound = 2.0 * R["torch_dev"][10]

    def run(first, second):
        params, _ = make_params()
        params = params[:len(SIZES)]
        a = first(params)
        for s in range(5):
            set_grads(params, dev_grads[s])
            a.step()
        b = second(params)
        b.load_state_dict(a.state_dict())
        for s in range(5, 10):
            set_grads(params, dev_grads[s])
            b.step()
        return params, b

    ours = lambda ps: dcl.optim.Adam(ps, **SHIPPED)                                   # noqa: E731
    theirs = lambda ps: torch.optim.Adam(ps, foreach=False, **SHIPPED)                # noqa: E731
    params, _ = run(ours, theirs)
    d = deviation(cpu(params), R["ref64"][10])
    print("5 steps dcl.optim.Adam -> state_dict -> 5 steps torch.optim.Adam: max |p - p64| %.3g (bound %.3g)" % (d, bound))
    assert d <= bound
    for make_theirs in (theirs, lambda ps: torch.optim.Adam(ps, fused=True, **SHIPPED)):
        params, opt = run(make_theirs, ours)
        d = deviation(cpu(params), R["ref64"][10])
        print("5 steps torch.optim.Adam -> state_dict -> 5 steps dcl.optim.Adam: max |p - p64| %.3g (bound %.3g)" % (d, bound))
        assert d <= bound
        # the loaded moments live in the flat buffers again, the step counts on the host
        for flat, name in zip(opt._flat, ("exp_avg", "exp_avg_sq")):
            lo, hi = flat.data_ptr(), flat.data_ptr() + 4 * flat.numel()
            ptrs = [opt.state[p][name].data_ptr() for p in params]
            assert all(lo <= q < hi for q in ptrs) and ptrs == sorted(ptrs) and len(set(ptrs)) == len(ptrs)
            assert all(opt.state[p][name]._base is flat for p in params)
        assert all(opt.state[p]["step"].device.type == "cpu" and int(opt.state[p]["step"]) == 10 for p in params)
        assert all(g["fused"] is None and g["foreach"] is None for g in opt.param_groups)


def test_a_step_moves_the_version_counters_and_folded_weights_follow(dcl):
    ref = dcl.refiner.Refiner()
    ref.load_state_dict(dcl.synth.synth_state_dict(ref, 2))
    ref = ref.to(DEV).eval()
    g = torch.Generator().manual_seed(5)
    b, n = 2, 1024
    inp = {"input_features": torch.cat([torch.randn(b, 3, n, generator=g) * 0.05, torch.randn(b, 256, n, generator=g)], 1).to(DEV),
           "conf": torch.rand(b, 2 * n, generator=g).to(DEV), "obj_idx": None}
    before = {k: v.clone() for k, v in ref(inp).items()}                 # folds the weights
    assert ref._folded is not None
    for p in ref.parameters():
        p.grad = torch.randn(p.shape, generator=g).to(DEV)
    versions = [p._version for p in ref.parameters()]
    dcl.optim.Adam(ref.parameters(), lr=1e-3).step()
    assert all(p._version > v for p, v in zip(ref.parameters(), versions))
    after = ref(inp)                                                     # no eval() / train() call in between
    fresh = dcl.refiner.Refiner()
    fresh.load_state_dict({k: v.detach().cpu() for k, v in ref.state_dict().items()})
    want = fresh.to(DEV).eval()(inp)
    for k in ("rot_pred", "trans_pred"):
        assert torch.equal(after[k], want[k]), k
    assert float((after["trans_pred"] - before["trans_pred"]).abs().max()) > 1e-6


class _Holder(torch.nn.Module):
    def __init__(self, params):
        super().__init__()
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(p.detach()) for p in params])


def test_autoclip_with_the_optimizer_and_alone(dcl):
    params, host = make_params()
    grads = make_grads(6, seed=3, lo=-2.0)
    dev_grads = upload(grads)
    opt = dcl.optim.Adam(params, **SHIPPED)
    clip = dcl.optim.AutoClip(50, optimizer=opt)
    twin = Twin(host, SHIPPED)
    total = sum(SIZES)
    scales = []
    for s in range(6):
        set_grads(params, dev_grads[s])
        clip(None)
        opt.step()
        want_norm = math.sqrt(math.fsum(exact_sq(g) for g in grads[s]))
        assert abs(clip.history[s] - want_norm) <= total * U * want_norm
        # the factor the host formula gives from that history
        scale = min(1.0, float(np.percentile(clip.history, 50)) / (clip.history[s] + 1e-6))
        scales.append(scale)
        twin.step(grads[s], scale)
        for p, g in zip(params, grads[s]):
            assert np.array_equal(p.grad.cpu().numpy(), g), "the fused form does not rewrite p.grad"
    print("AutoClip factors of the six steps:", ", ".join("%.4f" % x for x in scales))
    assert len(clip.history) == 6 and scales[5] < 0.9, "the last step is clipped in earnest"
    for i, p in enumerate(params[:len(SIZES)]):
        got = p.detach().cpu().numpy()
        assert np.array_equal(got.view(np.int32), twin.p[i].view(np.int32)), SIZES[i]
    # stand-alone: the same measurement, the gradients scaled in place
    model = _Holder(params[:len(SIZES)])
    alone = dcl.optim.AutoClip(50)
    alone.history = list(clip.history[:5])
    for p, g in zip(model.parameters(), dev_grads[5]):
        p.grad = g.clone()
    alone(model)
    assert alone.history[5] == clip.history[5]
    scale = min(1.0, float(np.percentile(alone.history, 50)) / (alone.history[5] + 1e-6))
    assert scale == scales[5]
    for p, g in zip(model.parameters(), grads[5]):
        assert np.array_equal(p.grad.cpu().numpy(), g * f32(scale))


def test_one_real_training_step_of_the_network(dcl):
    b, n = 2, 1024
    net = dcl.DCL_Net.Network(dcl.synth.default_cfg(n, n), mode="train")
    net.load_state_dict(dcl.synth.synth_state_dict(net, 1))
    net = net.to(DEV).train()
    names = [k for k, _ in net.named_parameters()]
    frozen = names[-1]
    dict(net.named_parameters())[frozen].requires_grad_(False)           # a parameter without a gradient
    crit = dcl.DCL_Net.losses(None)
    data = dcl.synth.make_batch(b, n, n)
    data["flags"] = torch.zeros(b)
    opt = dcl.optim.Adam(net.parameters(), **SHIPPED)
    clip = dcl.optim.AutoClip(50, optimizer=opt)
    crit(net(data), data["labels"])["loss_all"].backward()
    before = {k: p.detach().cpu().numpy().copy() for k, p in net.named_parameters()}
    grads = {k: p.grad.detach().cpu().numpy().copy() for k, p in net.named_parameters() if p.grad is not None}
    assert frozen not in grads and len(grads) >= len(names) - 1 and all(np.isfinite(g).all() for g in grads.values())
    clip(net)
    opt.step()
    want_norm = math.sqrt(math.fsum(exact_sq(g) for g in grads.values()))
    assert abs(clip.history[0] - want_norm) <= sum(g.size for g in grads.values()) * U * want_norm
    scale = min(1.0, clip.history[0] / (clip.history[0] + 1e-6))
    for k, p in net.named_parameters():
        got = p.detach().cpu().numpy()
        if k in grads:
            want, _, _ = twin_step(before[k], grads[k], np.zeros_like(before[k]), np.zeros_like(before[k]), 1, SHIPPED["lr"],
                                   SHIPPED["betas"], SHIPPED["eps"], scale)
            assert np.array_equal(got.view(np.int32), want.view(np.int32)), k
            assert int(opt.state[p]["step"]) == 1
        else:
            assert np.array_equal(got, before[k]) and len(opt.state.get(p, {})) == 0, k
