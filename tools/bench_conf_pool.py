#!/usr/bin/env python3
"""The confidence-weighted pooling that ends stage 1's dense half, forward + backward, in its two forms:
tools/bench_conf_pool.py [b] [N] [M] [--channels 1024] [--min-block 0.25] [--lib PATH]

  modules  the four lines of Network._forward_compat (train_pool="modules"): sigmoid, softmax, cat, broadcast product, sum,
           differentiated by autograd
  fused    train_pool="fused": autograd.ConfPoolFn = ops.conf_softmax + csrc/conf_pool_grad.hip

Both take logits (b,1,N), (b,1,M) and fuser outputs (b,C,N), (b,C,M) that require gradients, and upstream gradients on conf
and on the pooled feature.  The forms alternate inside one process; every figure is the median of three blocks of at least
--min-block seconds each (host clock around launches that end in a device synchronise), printed with the range of the three.
Peak memory is what one forward + backward allocates on top of its inputs.  The last lines time the new kernels alone
(ops.conf_pool_cm; ops.conf_pool_cm_backward for the logits only = the d kernel + the per-crop kernel; for F only = the dF
kernel) and give bytes moved / time, also as a share of the copy rate profiles/optim.txt measured (6.3 TB/s).  --lib: call into another
build of the library (the same sources with another DCL_CPG_CHUNK) through _native.diagnostic_library."""
import argparse
import ctypes
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
    l1, l2 = r(b, 1, n).requires_grad_(True), r(b, 1, m).requires_grad_(True)
    F1, F2 = r(b, c, n).relu_().requires_grad_(True), r(b, c, m).relu_().requires_grad_(True)
    g_conf, g_pool = r(b, 1, L) * 0.01, r(b, c, 1) * 0.1
    leaves = (l1, l2, F1, F2)

    def modules():
        conf = torch.sigmoid(torch.cat([l1, l2], dim=2))
        conf_softmax = torch.softmax(conf, dim=2)
        F_p = torch.cat([F1, F2], dim=2)
        F_p_wei = torch.sum(F_p * conf_softmax, dim=2, keepdim=True)
        return torch.autograd.grad([conf, F_p_wei], leaves, [g_conf, g_pool])

    def fused():
        out = dcl.autograd.ConfPoolFn.apply(l1, l2, F1, F2)
        return torch.autograd.grad([out[0].unsqueeze(1), out[1].unsqueeze(2)], leaves, [g_conf, g_pool])

    forms = {"modules": modules, "fused": fused}
    ga, gb = modules(), fused()
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

    def peak(fn):
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        return (torch.cuda.max_memory_allocated() - base) / 1e6

    cell = lambda v: "%9.1f [%9.1f - %9.1f]" % (v[1], v[0], v[2])                 # noqa: E731
    fbytes = 4.0 * b * c * L
    print("confidence pooling, b = %d, C = %d, N = %d, M = %d (F1 | F2: %.1f MB), library %s; us per forward + backward: median of 3 "
          "blocks >= %.2f s [range]" % (b, c, n, m, fbytes / 1e6, args.lib or "product", args.min_block))
    t = measure(forms)
    mem = {name: peak(fn) for name, fn in forms.items()}
    for name in forms:
        print("  %-8s %s us   peak memory above the inputs %9.1f MB" % (name, cell(t[name]), mem[name]))
    print("  fused / modules = %.3f; block ranges %s" % (
        t["fused"][1] / t["modules"][1], "disjoint, fused below" if t["fused"][2] < t["modules"][0] else
        ("disjoint, modules below" if t["modules"][2] < t["fused"][0] else "overlap")))

    with torch.no_grad():
        conf, w, _ = ops.conf_softmax(b, l1.detach().reshape(-1), l2.detach().reshape(-1))
        f1, f2, gp, gc = F1.detach(), F2.detach(), g_pool.reshape(b, c).contiguous(), g_conf.reshape(b, L).contiguous()
        q = ctypes.c_int64(0)
        dcl._native.check(dcl._native.lib().dcl_conf_pool_cm_bwd_ws_bytes(b, c, n, m, ctypes.byref(q)), "conf_pool_cm_bwd_ws_bytes")
        ws_bytes = float(q.value)                                                # the chunks' partials and d: written, then read
        kernels = {
            "pool (k_cpg_pool)": (lambda: ops.conf_pool_cm(w, f1, f2), fbytes + 4.0 * b * (L + c)),
            "d + per-crop (k_cpg_d, k_cpg_logits)": (
                lambda: ops.conf_pool_cm_backward(conf, w, f1, f2, gp, gc, need_F=False), fbytes + 2.0 * ws_bytes + 4.0 * b * L * 4),
            "dF (k_cpg_dF)": (lambda: ops.conf_pool_cm_backward(conf, w, f1, f2, gp, gc, need_logits=False), fbytes),
        }
        tk = measure({name: fn for name, (fn, _) in kernels.items()})
    print("the new kernels alone (us per call incl. the call's allocations; bytes moved / time; share of 6.3 TB/s):")
    for name, (_, nbytes) in kernels.items():
        rate = nbytes / (tk[name][1] * 1e-6)
        print("  %-38s %s us  %8.1f MB  %7.1f GB/s  %5.1f %%" % (name, cell(tk[name]), nbytes / 1e6, rate / 1e9, 100.0 * rate / COPY_RATE))
    if ctx:
        ctx.__exit__(None, None, None)


if __name__ == "__main__":
    main()
