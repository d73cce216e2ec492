"""AutoClip's device form on the GPU (csrc/optim.hip: dcl_autoclip_observe, dcl_adam_step_dev; dcl.optim.DeviceAutoClip): the
two kernels against the host twin bit for bit on all four outputs at the workgroup edges, the class against dcl.optim.AutoClip
over 40 steps with growth from capacity 4 (parameters and both moments after every step), a clip + step without a host
synchronisation, state dicts in both directions, non-finite norms, and one training configuration of Network under both
clippers.  Everything that is compared is compared as bytes."""
import warnings

import numpy as np
import pytest
import torch

import autoclip_cases as AC

pytestmark = pytest.mark.gpu

DEV = "cuda"
SHIPPED = dict(lr=1e-3, betas=(0.5, 0.999), eps=1e-6)      # tools/train_YCBV_stage1.py's optimizer
SIZES = [1, 5, 4097, 2 * 4096 + 7, 300]
VIEW = 3                                                    # the parameter that is a view at element offset 1
GROUPS = ([0, 1, 2], [3, 4])                                # two parameter groups, the second with its own lr
BLOCK = 256                                                 # the insertion's workgroup


# ------------------------------------------------------------------------------------------- 1. kernels against the twin
def _held(n, seed):
    """n ascending norms with runs of ties in them"""
    rng = np.random.default_rng(seed)
    return np.sort(np.round(rng.lognormal(0.0, 1.0, n), 1) + 0.5)


@pytest.mark.parametrize("n", [0, 1, 2, BLOCK - 1, BLOCK, BLOCK + 1, 4 * BLOCK - 1, 4 * BLOCK + 1])
def test_kernels_equal_the_host_twin_on_all_four_outputs(dcl, n):
    ops = dcl.ops
    held = _held(n, n)
    tie = held[n // 2] if n else 1.0
    assert n < 3 * BLOCK or (held == tie).sum() >= 2, "the middle value is a run of ties"
    places = {"below": 0.25, "above": (held[-1] + 1.0) if n else 2.0, "ties": tie,
              "middle": np.nextafter(tie, np.inf), "equal_to_the_last": held[-1] if n else 3.0}
    pad = 300
    for k, (where, x) in enumerate(sorted(places.items())):
        q = AC.PERCENTILES[k % len(AC.PERCENTILES)]
        got = []
        for device, fn in (("cpu", ops.autoclip_observe_host), (DEV, ops.autoclip_observe)):
            src = torch.from_numpy(held.copy()).to(device)
            dst = torch.full((n + 1 + pad,), float("nan"), dtype=torch.float64, device=device)
            arrival = torch.full((n + 1 + pad,), float("nan"), dtype=torch.float64, device=device)
            arrival[:n] = torch.arange(n, dtype=torch.float64)
            out = torch.full((AC.OUT_DOUBLES,), float("nan"), dtype=torch.float64, device=device)
            norm = torch.tensor([x], dtype=torch.float64).to(device)
            fn(n, src, dst, arrival, norm, q, out)
            got.append((AC.bits(dst), AC.bits(arrival), AC.bits(out[:3]), AC.bits(out.view(torch.float32)[AC.SCALE_F32_INDEX]),
                        AC.bits(src)))
            if device == "cpu":
                want = np.insert(held, np.searchsorted(held, x, side="right"), x)
                assert AC.bits(dst[:n + 1]) == AC.bits(want), where
                assert AC.bits(dst[n + 1:]) == AC.bits(np.full(pad, np.nan)) and AC.bits(arrival[n + 1:]) == AC.bits(np.full(pad, np.nan))
                assert float(arrival[n]) == x and AC.bits(src) == AC.bits(held)
        for what, a, b in zip(("sorted", "arrival", "out", "fp32 factor", "source"), got[0], got[1]):
            assert a == b, (n, where, what)


# ------------------------------------------------------------------------------------------- 2. class against class
def make_params(seed=0):
    g = torch.Generator().manual_seed(seed)
    params = []
    for i, n in enumerate(SIZES):
        h = torch.randn(n, generator=g) * 0.1
        if i == VIEW:
            base = torch.zeros(n + 1, device=DEV)
            base[1:] = h.to(DEV)
            p = base[1:].detach().requires_grad_(True)
            assert p.data_ptr() % 16 == 4 and p.is_contiguous()
        else:
            p = h.to(DEV).requires_grad_(True)
        params.append(p)
    return params


def make_optimizer(dcl, params):
    return dcl.optim.Adam([dict(params=[params[i] for i in GROUPS[0]]), dict(params=[params[i] for i in GROUPS[1]], lr=3e-4)],
                          **SHIPPED)


def make_grads(steps, seed=1):
    """a fixed gradient sequence on the device, [step][tensor]; the magnitudes wander over two decades, so that some steps are
    clipped in earnest and others not at all"""
    g = torch.Generator().manual_seed(seed)
    rng = np.random.default_rng(seed)
    mags = 10.0 ** rng.uniform(-3.0, -1.0, steps)
    return [[(torch.randn(n, generator=g) * float(mags[s])).to(DEV) for n in SIZES] for s in range(steps)]


def set_grads(params, grads):
    for p, g in zip(params, grads):
        p.grad = g.clone()


def same(a, b):
    return torch.equal(a.detach().contiguous().view(torch.int32), b.detach().contiguous().view(torch.int32))


def assert_same_state(opt_a, params_a, opt_b, params_b, step):
    for i, (pa, pb) in enumerate(zip(params_a, params_b)):
        assert same(pa, pb), (step, SIZES[i], "param")
        for key in ("exp_avg", "exp_avg_sq"):
            assert same(opt_a.state[pa][key], opt_b.state[pb][key]), (step, SIZES[i], key)
        assert float(opt_a.state[pa]["step"]) == float(opt_b.state[pb]["step"]) == step + 1


def test_forty_steps_equal_the_host_class_bit_for_bit(dcl):
    steps = 40
    grads = make_grads(steps)
    pa, pb = make_params(), make_params()
    opt_a, opt_b = make_optimizer(dcl, pa), make_optimizer(dcl, pb)
    host = dcl.optim.AutoClip(50, optimizer=opt_a)
    dev = dcl.optim.DeviceAutoClip(50, optimizer=opt_b, capacity=4)
    capacities, scales = [], []
    for s in range(steps):
        set_grads(pa, grads[s])
        set_grads(pb, grads[s])
        host(None)
        opt_a.step()
        dev(None)
        opt_b.step()
        assert_same_state(opt_a, pa, opt_b, pb, s)
        capacities.append(dev.capacity)
        if s % 13 == 5:
            scales.append(dev.scale)                                    # a documented read-back
    assert sorted(set(capacities)) == [4, 8, 16, 32, 64] and capacities[4] == 8 and capacities[32] == 64   # grew at 4, 8, 16, 32
    assert len(dev) == steps == len(host.history)
    assert AC.bits(np.array(dev.history)) == AC.bits(np.array(host.history))
    assert AC.bits(np.float64(dev.clip_value)) == AC.bits(np.float64(host.clip_value))
    assert dev.state_dict() == host.state_dict() and list(dev.state_dict()) == ["percentile", "history"]
    assert AC.bits(dev._sorted[0][:steps]) == AC.bits(np.sort(host.history))
    norms = np.array(host.history)
    factors = np.minimum(1.0, np.array([np.percentile(norms[:i + 1], 50) for i in range(steps)]) / (norms + 1e-6))
    assert (factors < 0.5).any() and (factors == 1.0).sum() >= 5, "steps clipped in earnest and steps not clipped at all"
    assert all(0.0 <= x <= 1.0 for x in scales)
    # the factor is spent: a step without a clipper in front of it runs at 1.0, as the host form's does
    set_grads(pa, grads[0])
    set_grads(pb, grads[0])
    opt_a.step()
    opt_b.step()
    assert_same_state(opt_a, pa, opt_b, pb, steps)


def test_adam_step_dev_has_adam_steps_bits_at_an_equal_factor(dcl):
    grads = make_grads(3, seed=5)
    for k, scale in enumerate((1.0, 0.37, 0.0)):
        pa, pb = make_params(), make_params()
        opt_a, opt_b = make_optimizer(dcl, pa), make_optimizer(dcl, pb)
        set_grads(pa, grads[k])
        set_grads(pb, grads[k])
        opt_a.set_grad_scale(scale)
        opt_b.set_grad_scale(torch.tensor([scale], dtype=torch.float32, device=DEV))
        opt_a.step()
        opt_b.step()
        assert_same_state(opt_a, pa, opt_b, pb, 0)
        assert opt_b._grad_scale == 1.0
    with pytest.raises(TypeError, match="fp32"):
        opt_b.set_grad_scale(torch.ones(1, dtype=torch.float64, device=DEV))
    with pytest.raises(TypeError, match="fp32"):
        opt_b.set_grad_scale(torch.ones(1))


# ------------------------------------------------------------------------------------------- 3. no synchronisation
def test_clip_and_step_run_without_a_host_synchronisation(dcl, monkeypatch):
    from test_gpu_crops_device_draws import SyncCount, _sync_debug_is_honoured
    grads = make_grads(12, seed=2)
    pa, pb = make_params(), make_params()
    opt_a, opt_b = make_optimizer(dcl, pa), make_optimizer(dcl, pb)
    host = dcl.optim.AutoClip(50, optimizer=opt_a)
    dev = dcl.optim.DeviceAutoClip(50, optimizer=opt_b, capacity=4)
    for s in range(6):                                                  # warm-up: the pinned staging ring, the first growth
        for ps, clip, opt in ((pa, host, opt_a), (pb, dev, opt_b)):
            set_grads(ps, grads[s])
            clip(None)
            opt.step()
    torch.cuda.synchronize()
    honoured = _sync_debug_is_honoured()
    count = SyncCount(monkeypatch)
    if honoured:
        torch.cuda.set_sync_debug_mode("error")
    try:
        for s in range(6, 10):                                          # n = 6 .. 9: the growth at 8 lies inside
            set_grads(pb, grads[s])
            dev(None)
            opt_b.step()
        assert dev.capacity == 16
        assert count.calls == [], count.calls
        set_grads(pa, grads[6])
        if honoured:
            with pytest.raises(RuntimeError):
                host(None)
        else:
            host(None)
        assert count.calls == ["item"], count.calls                     # the host class's one read-back
    finally:
        torch.cuda.set_sync_debug_mode("default")
    dev.clip_value
    assert count.calls == ["item", "cpu"], count.calls                  # a read-out is a read-back, and says so
    monkeypatch.undo()
    print("torch.cuda.set_sync_debug_mode('error') honoured: %s" % honoured)


# ------------------------------------------------------------------------------------------- 4. state dicts
def test_state_dicts_move_between_the_two_classes(dcl):
    grads = make_grads(16, seed=3)
    pa, pb = make_params(), make_params()
    opt_a, opt_b = make_optimizer(dcl, pa), make_optimizer(dcl, pb)
    host = dcl.optim.AutoClip(50, optimizer=opt_a)
    dev = dcl.optim.DeviceAutoClip(50, optimizer=opt_b, capacity=4)

    def run(clip_a, clip_b, first, last):
        for s in range(first, last):
            set_grads(pa, grads[s])
            set_grads(pb, grads[s])
            clip_a(None)
            opt_a.step()
            clip_b(None)
            opt_b.step()
            assert_same_state(opt_a, pa, opt_b, pb, s)
    run(host, dev, 0, 6)
    # each class continues from the other's dict: side a goes on with a device clipper, side b with a host one
    dev2 = dcl.optim.DeviceAutoClip(25, optimizer=opt_a, capacity=4)
    dev2.load_state_dict(host.state_dict())
    host2 = dcl.optim.AutoClip(75, optimizer=opt_b)
    host2.load_state_dict(dev.state_dict())
    assert dev2.percentile == 50 == host2.percentile and len(dev2) == 6 and dev2.capacity == 8 and dev2.clip_value is None
    assert AC.bits(np.array(dev2.history)) == AC.bits(np.array(host.history)) == AC.bits(np.array(host2.history))
    run(dev2, host2, 6, 16)
    assert dev2.state_dict() == host2.state_dict() and len(host2.history) == 16
    assert AC.bits(np.float64(dev2.clip_value)) == AC.bits(np.float64(host2.clip_value))
    # NaN and inf travel; an entry with the sign bit set is not a norm
    dev2.load_state_dict({"percentile": 37.5, "history": [2.0, float("nan"), float("inf"), 0.0]})
    assert AC.bits(dev2._sorted[0][:4]) == AC.bits(np.array([0.0, 2.0, np.inf, np.nan])) and dev2.percentile == 37.5
    assert AC.bits(np.array(dev2.history)) == AC.bits(np.array([2.0, np.nan, np.inf, 0.0]))
    for bad in (-1.0, -0.0, float("-inf")):
        with pytest.raises(ValueError, match="sign bit"):
            dev2.load_state_dict({"percentile": 50, "history": [1.0, bad]})
    assert len(dev2) == 4                                                # a refused dict changes nothing


# ------------------------------------------------------------------------------------------- 5. non-finite norms
@pytest.mark.parametrize("name", ["nan_at_5", "one_inf", "two_inf", "one_then_inf"])
def test_non_finite_norms_equal_the_host_twin(dcl, name):
    seq = AC.sequences()[name]
    for q in AC.PERCENTILES:
        twin = AC.HostClip(dcl.ops, q, capacity=2)
        dev = AC.HostClip(dcl.ops, q, capacity=2, device=DEV)
        for step, x in enumerate(seq):
            twin.observe(float(x))
            dev.observe(float(x))
            assert twin.everything() == dev.everything(), (q, step)
    assert not np.isfinite(seq).all()


# ------------------------------------------------------------------------------------------- 6. Network
def test_two_training_steps_of_the_network_equal_under_both_clippers(dcl):
    """tools/train_step.py --kernels at its smallest shape (tests/step_replay.py: b = 2, 256 points), --autoclip host against
    --autoclip device from the same seed: loss and parameters bit for bit, over two steps so that the second forward runs on
    weights the first clipped update wrote"""
    import step_replay as SR

    def run(device_clip):
        torch.manual_seed(0)
        net = SR.make_net(dcl, 256, **dcl.DCL_Net.TRAIN_KERNELS)
        crit = dcl.DCL_Net.losses(None, chamfer="fused", objective="fused")
        opt = dcl.optim.Adam(net.parameters(), **SR.SHIPPED_ADAM)
        clip = (dcl.optim.DeviceAutoClip if device_clip else dcl.optim.AutoClip)(50, optimizer=opt)
        data = SR.make_data(dcl, 2, 256)
        losses = []
        for _ in range(2):
            opt.zero_grad()
            loss = crit(net(data), data["labels"])["loss_all"]
            loss.backward()
            clip(net)
            opt.step()
            losses.append(loss.detach().clone())
        return net, losses, clip
    net_a, loss_a, host = run(False)
    net_b, loss_b, dev = run(True)
    assert AC.bits(torch.stack(loss_a)) == AC.bits(torch.stack(loss_b))
    assert float(loss_a[0]) != float(loss_a[1]) and np.isfinite(host.history).all()
    assert AC.bits(np.array(dev.history)) == AC.bits(np.array(host.history))
    for (k, p), (_, w) in zip(net_b.named_parameters(), net_a.named_parameters()):
        assert same(p, w), k
