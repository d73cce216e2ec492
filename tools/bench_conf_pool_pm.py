#!/usr/bin/env python3
"""The confidence-weighted pooling of the training path in its two layouts, in one job:
tools/bench_conf_pool_pm.py [b] [N] [M] [--channels 1024] [--min-block 0.25] [--lib PATH]

  cm  channel-major, F (b, C, n): autograd.ConfPoolFn   = ops.conf_softmax + csrc/conf_pool_grad.hip (train_pool="fused")
  pm  point-major,   F (b n, C): autograd.ConfPoolPmFn = ops.conf_softmax + csrc/conf_pool_pm.hip   (train_dense="point_major")

Both take the same logits and the same fuser outputs (the point-major ones are the transposed copies), requiring gradients, and
upstream gradients on conf and on the pooled feature.  The forms alternate inside one process; every figure is the median of
three blocks of at least --min-block seconds each (host clock around launches that end in a device synchronise), printed with
the range of the three.  The last lines time the kernels of both layouts alone (forward; backward for the logits only; backward
for F only) and give bytes that must move / time, also as a share of the copy rate profiles/optim.txt measured (6.3 TB/s).
--lib: call into another build of the library (the same sources with another DCL_POOL_PM_ROWS) through
_native.diagnostic_library."""
import argparse
import importlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_RATE = 6.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("b", type=int, nargs="?", default=32)
    ap.add_argument("n", type=int, nargs="?", default=1024)
    ap.add_argument("m", type=int, nargs="?", default=1024)
    ap.add_argument("--channels", type=int, default=1024)
    ap.add_argument("--min-block", type=float, default=0.25)
    ap.add_argument("--lib", default=None)
    args = ap.parse_args()

    import torch
    dcl = importlib.import_module("dcl-net_amd")
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    ops = dcl.ops
    ctx = dcl._native.diagnostic_library(args.lib) if args.lib else None
    if ctx:
        ctx.__enter__()
    b, n, m, c = args.b, args.n, args.m, args.channels
    L = n + m
    gen = torch.Generator(device="cuda").manual_seed(7)
    r = lambda *s: torch.randn(*s, device="cuda", generator=gen)                              # noqa: E731
    l1, l2 = r(b, n).requires_grad_(True), r(b, m).requires_grad_(True)
    F1, F2 = r(b, c, n).relu_(), r(b, c, m).relu_()
    P1 = F1.transpose(1, 2).reshape(b * n, c).contiguous().requires_grad_(True)
    P2 = F2.transpose(1, 2).reshape(b * m, c).contiguous().requires_grad_(True)
    F1.requires_grad_(True), F2.requires_grad_(True)
    g_conf, g_pool = r(b, L) * 0.01, r(b, c) * 0.1

    def cm():
        out = dcl.autograd.ConfPoolFn.apply(l1, l2, F1, F2)
        return torch.autograd.grad(out, (l1, l2, F1, F2), [g_conf, g_pool])

    def pm():
        out = dcl.autograd.ConfPoolPmFn.apply(l1, l2, P1, P2)
        return torch.autograd.grad(out, (l1, l2, P1, P2), [g_conf, g_pool])

    forms = {"cm": cm, "pm": pm}
    ga, gb = cm(), pm()
    gb = (gb[0], gb[1], gb[2].view(b, n, c).transpose(1, 2), gb[3].view(b, m, c).transpose(1, 2))
    for name, x, y in zip(("dlogit1", "dlogit2", "dF1", "dF2"), ga, gb):
        rel = float((x - y).abs().max()) / max(float(x.abs().max()), 1e-30)
        assert rel < 1e-4, (name, rel)                                          # the same gradients, up to the order of summation
    del ga, gb

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
    fbytes = 4.0 * b * c * L
    print("confidence pooling, b = %d, C = %d, N = %d, M = %d (F1 | F2: %.1f MB), library %s, DCL_POOL_PM_ROWS of the product header "
          "%d; us per forward + backward: median of 3 blocks >= %.2f s [range]" % (b, c, n, m, fbytes / 1e6, args.lib or "product",
                                                                                  ops.POOL_PM_ROWS, args.min_block))
    t = measure(forms)
    for name in forms:
        print("  %-4s %s us" % (name, cell(t[name])))
    print("  pm / cm = %.3f; block ranges %s" % (
        t["pm"][1] / t["cm"][1], "disjoint, pm below" if t["pm"][2] < t["cm"][0] else
        ("disjoint, cm below" if t["cm"][2] < t["pm"][0] else "overlap")))

    with torch.no_grad():
        conf, w, _ = ops.conf_softmax(b, l1.detach().reshape(-1), l2.detach().reshape(-1))
        f1, f2, p1, p2 = F1.detach(), F2.detach(), P1.detach(), P2.detach()
        small = 4.0 * b * (L + c)
        # bytes that must move: F once (read or written) + the small vectors; the logits' gradient also writes and reads d
        kernels = {
            "cm forward  (k_cpg_pool)": (lambda: ops.conf_pool_cm(w, f1, f2), fbytes + small),
            "pm forward  (k_cpp_pool)": (lambda: ops.conf_pool_pm(w, p1, p2), fbytes + small),
            "cm logits   (k_cpg_d, k_cpg_logits)": (
                lambda: ops.conf_pool_cm_backward(conf, w, f1, f2, g_pool, g_conf, need_F=False), fbytes + small + 4.0 * b * L * 5),
            "pm logits   (k_cpp_d x 2, k_cpg_logits)": (
                lambda: ops.conf_pool_pm_backward(conf, w, p1, p2, g_pool, g_conf, need_F=False), fbytes + small + 4.0 * b * L * 5),
            "cm dF       (k_cpg_dF)": (lambda: ops.conf_pool_cm_backward(conf, w, f1, f2, g_pool, g_conf, need_logits=False), fbytes + small),
            "pm dF       (k_cpp_dF x 2)": (lambda: ops.conf_pool_pm_backward(conf, w, p1, p2, g_pool, g_conf, need_logits=False), fbytes + small),
        }
        tk = measure({name: fn for name, (fn, _) in kernels.items()})
    print("the kernels alone (us per call incl. the call's allocations; bytes that must move / time; share of 6.3 TB/s):")
    for name, (_, nbytes) in kernels.items():
        rate = nbytes / (tk[name][1] * 1e-6)
        print("  %-42s %s us  %8.1f MB  %7.1f GB/s  %5.1f %%" % (name, cell(tk[name]), nbytes / 1e6, rate / 1e9, 100.0 * rate / COPY_RATE))
    if ctx:
        ctx.__exit__(None, None, None)


if __name__ == "__main__":
    main()
