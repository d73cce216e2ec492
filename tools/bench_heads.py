#!/usr/bin/env python3
"""What Network / Refiner(train_heads=) switches, each block in its two forms, alternating in one job:
tools/bench_heads.py [--min-block 0.25] [--iters 20]
tools/bench_heads.py --trace-diff MODULES_KERNEL_STATS.csv KERNELS_KERNEL_STATS.csv --steps 13

  narrow layer   the last layer of a per-point head, y (M, N) = x (M, K) W^T + bias, forward + backward with all three gradients
      modules    torch.nn.functional.linear on the registered parameters (vendor GEMMs: the forward and its two gradients)
      kernels    autograd.NarrowLinearFn (csrc/linear_narrow.hip)
    at (32 768, 128, 1), (32 768, 128, 3): 32 crops of 1024 points, the confidence and the coordinate heads; (393 216, 128, 3):
    32 crops of 12 288 points
  pose heads     regressor_rot + regressor_trans on the pooled (b, 1024) rows, forward + backward with every gradient
      modules    two Head_MultiLayerPerceptron modules (nn.Conv1d + nn.ReLU)
      kernels    autograd.PoseHeadsFn (csrc/pose_heads_grad.hip)
    at b = 32 and b = 40

The forms alternate inside one process; every figure is the median of three blocks of at least --min-block seconds each (host
clock around calls that end in a device synchronise), printed with the range of the three.  Then the library calls alone, by
device events (median of --iters): us, the bytes that MUST move (computed from the shapes: every operand once), and that over
the time as a share of the copy rate profiles/optim.txt measured (6.3 TB/s).  An operand set smaller than the 256 MiB last-level
cache can stay resident between calls: its share then says nothing about HBM, and the line is marked.

--trace-diff: two rocprofv3 --kernel-trace --stats summaries of the same step (tools/train_step.py or the stage-2 step), the first
with --heads modules, the second with --heads kernels: kernel time and launches per step, the vendor GEMMs (Cijk_*) of each, and
every kernel whose launch count differs."""
import argparse
import csv
import importlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

COPY_RATE = 6.3e12
CACHE = 256 << 20
NARROW = ((32768, 128, 1), (32768, 128, 3), (393216, 128, 3))
POSE_B = (32, 40)


def trace_diff(paths, steps):
    tabs = []
    for path in paths:
        tab = {}
        for row in csv.DictReader(open(path)):
            t, c = tab.get(row["Name"], (0.0, 0))
            tab[row["Name"]] = (t + float(row["TotalDurationNs"]) / 1e3, c + int(row["Calls"]))
        tabs.append(tab)
    for form, tab in zip(("modules", "kernels"), tabs):
        vend = [v for k, v in tab.items() if k.startswith("Cijk_")]
        print("  --heads %-8s kernel time per step %8.2f ms in %7.1f launches; vendor GEMMs (Cijk_*): %7.1f us in %5.1f launches per step"
              % (form, sum(t for t, _ in tab.values()) / steps / 1e3, sum(c for _, c in tab.values()) / steps,
                 sum(t for t, _ in vend) / steps, sum(c for _, c in vend) / steps))
    print("  every kernel whose launch count differs: us per step (launches per step) modules, kernels, difference")
    names = [k for k in set(tabs[0]) | set(tabs[1]) if tabs[0].get(k, (0, 0))[1] != tabs[1].get(k, (0, 0))[1]]
    for k in sorted(names, key=lambda k: tabs[1].get(k, (0, 0))[0] - tabs[0].get(k, (0, 0))[0]):
        (t0, c0), (t1, c1) = tabs[0].get(k, (0.0, 0)), tabs[1].get(k, (0.0, 0))
        print("  %9.1f (%5.1f)  %9.1f (%5.1f)  %+9.1f  %s" % (t0 / steps, c0 / steps, t1 / steps, c1 / steps, (t1 - t0) / steps,
                                                             k.replace("(anonymous namespace)::", "")[:110]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace-diff", nargs=2, default=None)
    ap.add_argument("--steps", type=int, default=13)
    ap.add_argument("--min-block", type=float, default=0.25)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    if args.trace_diff:
        return trace_diff(args.trace_diff, args.steps)

    import torch
    import torch.nn.functional as Fn
    from bench_chamfer import events_ms
    dcl = importlib.import_module("dcl-net_amd")
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    ops, A = dcl.ops, dcl.autograd
    gen = torch.Generator(device="cuda").manual_seed(11)
    r = lambda *s: torch.randn(*s, device="cuda", generator=gen)                              # noqa: E731

    def block(fn, iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / iters

    def measure(fns):
        iters, t = {}, {name: [] for name in fns}
        for name, fn in fns.items():                                             # warm up and size the blocks
            block(fn, 3)
            iters[name] = max(3, int(args.min_block / block(fn, 5)) + 1)
        for _ in range(3):
            for name, fn in fns.items():
                t[name].append(block(fn, iters[name]) * 1e6)
        return {name: sorted(v) for name, v in t.items()}

    cell = lambda v: "%9.1f [%9.1f - %9.1f]" % (v[1], v[0], v[2])                 # noqa: E731

    def verdict(t):
        k, m = t["kernels"], t["modules"]
        return "disjoint, kernels below" if k[2] < m[0] else ("disjoint, modules below" if m[2] < k[0] else "overlap")

    def alone(name, fn, nbytes):
        us = events_ms(fn, args.iters, 3) * 1e3
        rate = nbytes / (us * 1e-6)
        print("    %-34s %8.1f us  %8.2f MB  %7.1f GB/s  %5.1f %%%s" % (
            name, us, nbytes / 1e6, rate / 1e9, 100.0 * rate / COPY_RATE, "  (fits the cache: not an HBM rate)" if nbytes < CACHE else ""))

    print("train_heads: us per forward + backward, median of 3 blocks >= %.2f s [range]; NARROW_ROWS %d; device %s" %
          (args.min_block, ops.NARROW_ROWS, torch.cuda.get_device_name(0)))
    for M, K, N in NARROW:
        x, W, bias, g = r(M, K).requires_grad_(True), (r(N, K, 1) / K ** 0.5).requires_grad_(True), r(N).requires_grad_(True), r(M, N)

        def modules():
            return torch.autograd.grad(Fn.linear(x, W.view(N, K), bias), (x, W, bias), g)

        def kernels():
            return torch.autograd.grad(A.NarrowLinearFn.apply(x, W, bias), (x, W, bias), g)

        for name, u, v in zip(("dx", "dW", "db"), modules(), kernels()):
            rel = float((u - v).abs().max()) / max(float(u.abs().max()), 1e-30)
            assert rel < 1e-4, (name, rel)                                        # the same gradients, up to the order of summation
        t = measure({"modules": modules, "kernels": kernels})
        print("narrow layer (%d, %d, %d):" % (M, K, N))
        for name in ("modules", "kernels"):
            print("  %-8s %s us" % (name, cell(t[name])))
        print("  kernels / modules = %.3f; block ranges %s" % (t["kernels"][1] / t["modules"][1], verdict(t)))
        with torch.no_grad():
            xd, Wd = x.detach(), W.detach()
            xb, yb, small = 4.0 * M * K, 4.0 * M * N, 4.0 * (N * K + N)
            chunks = -(-M // ops.NARROW_ROWS)
            alone("forward  (k_ln_fwd)", lambda: ops.linear_narrow(xd, Wd, bias.detach()), xb + yb + small)
            alone("backward (k_ln_bwd, k_ln_finish)", lambda: ops.linear_narrow_backward(xd, Wd, g),
                  2 * xb + yb + small + 2 * 4.0 * chunks * (N * K + N))
            alone("backward, dx alone (k_ln_bwd)", lambda: ops.linear_narrow_backward(xd, Wd, g, need_w=False, need_b=False),
                  xb + yb + small)
        del x, W, bias, g

    for b in POSE_B:
        heads = [dcl.DCL_Net._mlp3([1024, 512, 128, n]).cuda() for n in (9, 3)]
        params = dcl.DCL_Net.pose_head_params(*heads)
        x, g9, g3 = r(b, 1024).requires_grad_(True), r(b, 9), r(b, 3)

        def modules():
            xs = x.unsqueeze(2)
            return torch.autograd.grad([heads[0](xs).squeeze(-1), heads[1](xs).squeeze(-1)], [x] + params, [g9, g3])

        def kernels():
            return torch.autograd.grad(A.PoseHeadsFn.apply(x, *params), [x] + params, [g9, g3])

        for i, (u, v) in enumerate(zip(modules(), kernels())):
            rel = float((u - v).abs().max()) / max(float(u.abs().max()), 1e-30)
            assert rel < 1e-3, (i, rel)
        t = measure({"modules": modules, "kernels": kernels})
        print("pose heads, b = %d:" % b)
        for name in ("modules", "kernels"):
            print("  %-8s %s us" % (name, cell(t[name])))
        print("  kernels / modules = %.3f; block ranges %s" % (t["kernels"][1] / t["modules"][1], verdict(t)))
        with torch.no_grad():
            P = [p.detach() for p in params]
            wbytes = 4.0 * sum(p.numel() for p in P)
            act = 4.0 * b * (1024 + 2 * (512 + 128) + 12)
            o9, t3, h1, h2 = ops.pose_heads_train(x.detach(), P)
            alone("forward  (k_ph_fwd x 3)", lambda: ops.pose_heads_train(x.detach(), P), wbytes + act)
            alone("backward (k_ph_bwd_layer / _sum x 3)", lambda: ops.pose_heads_train_backward(x.detach(), P, h1, h2, g9, g3),
                  2 * wbytes + 2 * act)
        del heads, params, x


if __name__ == "__main__":
    main()
