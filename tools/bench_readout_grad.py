"""The gradient of the multi-scale voxel read-out (ops.three_interpolate_grad_sp, the backward of pointnet_sp's
three_interpolate inside Ops_GetPointFeat_spconv) in its two forms, on the indices a real batch produces:

  ordered   dcl_three_interpolate_grad_sp_ordered (csrc/readout_grad.hip): index build + gather, reads the column block of
            the (n, 480) gradient where it lies, writes every output row; the package's default
  atomic    what the op did before: a contiguous copy of the column block, a zero-fill of the output and the reference's
            atomic scatter (ops.three_interpolate_grad_sp_atomic) -- the BASELINE of every ratio below

  python tools/bench_readout_grad.py [--iters 50] [--step-iters 10] [--warmup 3]

Shapes: 32 x 1024 / 1024 (the training shape) and 4 x 12288 / 2048 crops x observed / template points from
dcl.synth.make_batch.  One train-mode forward of Network records idx, weight, m and c of the eight read-out calls (four
levels of the observed side, four of the template side).  Per call: median and maximum contributors per output row, and the
time of both forms on a column block of an (n, 480) gradient; then all eight calls in a row; then forward + backward of the
whole network with the read-out gradient in each form (the atomic form by routing the op to the atomic wrapper inside this
process).  Timing: a host clock around a block of calls ended by a device synchronise, at least `iters` of them and
at least a quarter of a second's worth, in six blocks that alternate the two forms in both orders; reported are the median of
a form's three block means and their range.  Last, the training step is run
twice on the same batch and all parameter gradients are compared bit for bit, with train_attention="fused" and with the
default, in both forms of the read-out gradient.  profiles/readout_grad.txt holds one run's output."""
import argparse
import importlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

SHAPES = [(32, 1024, 1024), (4, 12288, 2048)]


def block_ms(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


MIN_BLOCK_S = 0.25          # a timed block lasts at least this long: shorter windows time the clock and the scheduler


def compare(forms, iters, warmup):
    """{name: fn} for two forms -> {name: (median of its three block means, lowest, highest)}; both forms run the same
    number of calls per block, at least `iters` and enough for the slower one to fill MIN_BLOCK_S"""
    a, c = list(forms)
    for _ in range(warmup):
        for fn in forms.values():
            fn()
    slowest = max(block_ms(fn, iters) for fn in forms.values())
    iters = max(iters, int(MIN_BLOCK_S * 1e3 / slowest) + 1)
    blocks = [(name, block_ms(forms[name], iters)) for order in ((a, c, a), (c, a, c)) for name in order]
    out = {}
    for n in forms:
        v = sorted(t for k, t in blocks if k == n)
        out[n] = (v[len(v) // 2], v[0], v[-1])
    return out


def line(what, res):
    (o, olo, ohi), (p, plo, phi) = res["ordered"], res["atomic"]
    verdict = "slower" if olo > phi else "faster" if ohi < plo else "within the spread"
    print("  %-34s ordered %8.4f ms [%.4f .. %.4f]   atomic %8.4f ms [%.4f .. %.4f]   ordered / atomic %.2f  (%s)" %
          (what, o, olo, ohi, p, plo, phi, o / p, verdict))


def record_readout_calls(dcl, net, data):
    """one train-mode forward; -> [(idx, weight, m, c)] of the read-out's three_interpolate calls, in call order"""
    calls, real = [], dcl.ops.three_interpolate_sp

    def spy(features, idx, weight, *a, **k):
        calls.append((idx, weight, int(features.shape[0]), int(features.shape[1])))
        return real(features, idx, weight, *a, **k)
    dcl.ops.three_interpolate_sp = spy
    try:
        with torch.no_grad():
            net(data)
    finally:
        dcl.ops.three_interpolate_sp = real
    torch.cuda.synchronize()
    return calls


def loss_of(out):
    return sum(out[k].abs().mean() for k in ("rot_pred", "trans_pred", "conf", "Xo_pred", "Yc_pred"))


def make_step(net, data):
    def step():
        torch.manual_seed(0)
        for p in net.parameters():
            p.grad = None
        loss_of(net(data)).backward()
    return step


class atomic_form(object):
    """inside the block the package's read-out gradient is the parent's: copy, zero-fill, atomic scatter"""

    def __init__(self, dcl):
        self.ops = dcl.ops

    def __enter__(self):
        self.real = self.ops.three_interpolate_grad_sp
        self.ops.three_interpolate_grad_sp = self.ops.three_interpolate_grad_sp_atomic

    def __exit__(self, *exc):
        self.ops.three_interpolate_grad_sp = self.real
        return False


def grads_of(net, step):
    step()
    torch.cuda.synchronize()
    return [(k, None if p.grad is None else p.grad.clone()) for k, p in net.named_parameters()]


def repeat_check(net, step):
    a, b = grads_of(net, step), grads_of(net, step)
    differing = [k for (k, x), (_, y) in zip(a, b) if (x is None) != (y is None) or (x is not None and not torch.equal(x, y))]
    with_grad = sum(x is not None for _, x in a)
    if not differing:
        return "all %d parameter gradients bit-identical" % with_grad
    return "%d of %d parameter gradients differ, the first: %s" % (len(differing), with_grad, differing[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--step-iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_readout_grad: needs the GPU (no CPU timing is meaningful)")
    dcl = importlib.import_module("dcl-net_amd")
    print("read-out gradient: ordered (csrc/readout_grad.hip, index build + gather) vs atomic (copy + zero-fill + atomic scatter)")
    print("device: %s, torch %s; blocks of at least %d calls / %d steps and %.2f s, six alternating blocks after %d warm-up rounds" %
          (torch.cuda.get_device_name(0), torch.__version__, args.iters, args.step_iters, MIN_BLOCK_S, args.warmup))
    for b, n_inp, n_tmp in SHAPES:
        print("\n== %d crops x %d observed / %d template points" % (b, n_inp, n_tmp))
        cfg = dcl.synth.default_cfg(n_inp, n_tmp)
        net = dcl.DCL_Net.Network(cfg, mode="train")
        sd = dcl.synth.synth_state_dict(net, 1)
        net.load_state_dict(sd)
        net = net.cuda().train()
        data = dcl.synth.make_batch(b, n_inp, n_tmp)
        data["flags"] = torch.zeros(b, dtype=torch.int32)
        calls = record_readout_calls(dcl, net, data)
        assert len(calls) == 8, len(calls)
        g = torch.Generator().manual_seed(b + n_inp)
        wide = {n: torch.randn(n, 480, generator=g).cuda() for n in {b * n_inp, b * n_tmp}}
        per_call, col = [], 0
        for i, (idx, w, m, c) in enumerate(calls):
            if i % 4 == 0:
                col = 0
            n = idx.shape[0]
            block = wide[n][:, col:col + c]
            col += c
            cnt = np.bincount(idx.reshape(-1).cpu().numpy(), minlength=m)
            forms = {"ordered": lambda: dcl.ops.three_interpolate_grad_sp(block, idx, w, m),
                     "atomic": lambda: dcl.ops.three_interpolate_grad_sp_atomic(block, idx, w, m)}
            same = float((forms["ordered"]() - forms["atomic"]()).abs().max())
            res = compare(forms, args.iters, args.warmup)
            print(" %s level %d: n %d, m %d, c %d; contributors per row: median %d, mean %.1f, max %d, rows without any %d; "
                  "max |ordered - atomic| %.3g" % ("observed" if i < 4 else "template", i % 4 + 1, n, m, c, int(np.median(cnt)),
                                                   cnt.mean(), int(cnt.max()), int((cnt == 0).sum()), same))
            line("this call", res)
            per_call.append((block, idx, w, m))

        def all_calls(fn):
            return lambda: [fn(*a) for a in per_call]
        print(" all eight calls in a row")
        line("eight calls", compare({"ordered": all_calls(dcl.ops.three_interpolate_grad_sp),
                                     "atomic": all_calls(dcl.ops.three_interpolate_grad_sp_atomic)}, args.iters, args.warmup))

        step = make_step(net, data)

        def atomic_step():
            with atomic_form(dcl):
                step()
        print(" forward + backward of Network(mode=\"train\"), every parameter's gradient")
        line("whole step", compare({"ordered": step, "atomic": atomic_step}, args.step_iters, args.warmup))

        print(" the same step twice on the same batch")
        for att in ("fused", "materialised"):
            net2 = dcl.DCL_Net.Network(cfg, mode="train", train_attention=att)
            net2.load_state_dict(sd)
            net2 = net2.cuda().train()
            step2 = make_step(net2, data)
            print("  train_attention=%-14s ordered read-out gradient: %s" % ('"%s",' % att, repeat_check(net2, step2)))
            with atomic_form(dcl):
                print("  train_attention=%-14s atomic read-out gradient:  %s" % ('"%s",' % att, repeat_check(net2, step2)))
            del net2, step2
        del net, step, per_call, wide, calls
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
