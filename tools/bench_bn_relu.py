#!/usr/bin/env python3
"""The backbones' BatchNorm1d + ReLU pairs in their two forms, layer by layer, on the feature matrices of a training batch:
tools/bench_bn_relu.py [b] [N] [--min-block 0.25] [--lib PATH] [--fused-only]

  modules  nn.BatchNorm1d -> nn.ReLU in train mode, differentiated by autograd (Network(train_norm="modules"))
  fused    autograd.BnReluFn: ops.bn_relu + ops.bn_relu_backward (csrc/bn_relu.hip; Network(train_norm="fused"))

The layers are the 16 BasicBlock_SPCONV calls of one train-mode forward of Network on synth.make_batch(b, N, N) -- both
backbones, recorded with their conv outputs, so every form runs on the real rows and the real values.  One call = forward +
backward with gradients for x, gamma and beta, the running statistics updated.  The forms alternate inside one process; every
figure is the median of three blocks of at least --min-block seconds each (host clock around launches that end in a device
synchronise), printed with the range of the three.  Then the fused form's calls alone, summed over the 16 layers, with the
bytes they have to move (x twice and z once forward; x and g once for the sums, both once more and dx for the input
gradient) against the 6.3 TB/s copy rate, and the layers on which "fused" is not faster with disjoint block ranges.
--lib: call into another build of the library (the same sources with -DDCL_BN_ROWS=n or -DDCL_BN_NT=1) through
_native.diagnostic_library; --fused-only: skip the module form (for those builds)."""
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
    ap.add_argument("--min-block", type=float, default=0.25)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--fused-only", action="store_true")
    args = ap.parse_args()

    import torch
    dcl = importlib.import_module("dcl-net_amd")
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    ops = dcl.ops
    b, n = args.b, args.n
    net = dcl.DCL_Net.Network(dcl.synth.default_cfg(n, n), mode="train")
    net.load_state_dict(dcl.synth.synth_state_dict(net, 1))
    net = net.cuda().train()
    data = dcl.synth.make_batch(b, n, n)
    data["flags"] = torch.zeros(b)
    layers, hooks = [], []
    for name, m in net.named_modules():
        if isinstance(m, dcl.Modules.BasicBlock_SPCONV):
            hooks.append(m.layers[0].register_forward_hook(
                lambda mod, a, out, name=name, bn=m.layers[1]: layers.append((name, out.features.detach().clone(), bn))))
    with torch.no_grad():
        net(data)
    for h in hooks:
        h.remove()
    torch.cuda.synchronize()
    assert len(layers) == 16, len(layers)
    ctx = dcl._native.diagnostic_library(args.lib) if args.lib else None
    if ctx:
        ctx.__enter__()
    gen = torch.Generator(device="cuda").manual_seed(5)

    def block(fn, iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / iters

    def measure(forms):
        iters = {}
        for name, fn in forms.items():                                           # warm up and size the blocks
            block(fn, 3)
            iters[name] = max(3, int(args.min_block / block(fn, 5)) + 1)
        t = {name: [] for name in forms}
        for _ in range(3):
            for name, fn in forms.items():
                t[name].append(block(fn, iters[name]) * 1e6)
        for name in forms:
            t[name].sort()
        return t

    cell = lambda v: "%7.1f [%6.1f-%6.1f]" % (v[1], v[0], v[2])                   # noqa: E731
    print("sparse-conv BatchNorm + ReLU, b = %d, N = M = %d, library %s, DCL_BN_ROWS of the package %d; us per forward + backward: "
          "median of 3 blocks >= %.2f s [range]" % (b, n, args.lib or "product", ops.BN_ROWS, args.min_block))
    print("%2s %-28s %7s %4s %6s | %22s | %22s | %s" % ("#", "block", "rows", "C", "MB", "modules", "fused", "fused / modules"))
    names = ("fused",) if args.fused_only else ("modules", "fused")
    parts = ("fwd", "bwd sums", "bwd all")
    sums = {k: [0.0, 0.0, 0.0] for k in names + parts}
    part_bytes = {k: 0.0 for k in parts}
    not_faster, total = [], 0
    for li, (name, x, bn) in enumerate(layers):
        V, C = x.shape
        total += V * C
        g = torch.randn((V, C), device="cuda", generator=gen) * 0.1
        xr = x.clone().requires_grad_(True)
        w, bias = bn.weight.detach().clone().requires_grad_(True), bn.bias.detach().clone().requires_grad_(True)
        rm, rv = bn.running_mean.clone(), bn.running_var.clone()
        mod = torch.nn.BatchNorm1d(C, eps=bn.eps, momentum=bn.momentum).cuda().train()
        with torch.no_grad():
            mod.weight.copy_(w), mod.bias.copy_(bias)

        def modules_form():
            xr.grad = mod.weight.grad = mod.bias.grad = None
            torch.relu(mod(xr)).backward(g)

        def fused_form():
            xr.grad = w.grad = bias.grad = None
            dcl.autograd.BnReluFn.apply(xr, w, bias, rm, rv, bn.momentum, bn.eps).backward(g)

        forms = {"modules": modules_form, "fused": fused_form}
        forms = {k: forms[k] for k in names}
        t = measure(forms)
        xd, wd, bd = x, w.detach(), bias.detach()
        _, mean, invstd = ops.bn_relu(xd, wd, bd)
        tp = measure({"fwd": lambda: ops.bn_relu(xd, wd, bd, rm, rv, bn.momentum, bn.eps),
                      "bwd sums": lambda: ops.bn_relu_backward(xd, wd, bd, mean, invstd, g, need_x=False),
                      "bwd all": lambda: ops.bn_relu_backward(xd, wd, bd, mean, invstd, g)})
        for k, passes in (("fwd", 3), ("bwd sums", 2), ("bwd all", 5)):
            part_bytes[k] += passes * 4.0 * V * C
        for k in list(t) + list(tp):
            for i in range(3):
                sums[k][i] += (t[k] if k in t else tp[k])[i]
        if args.fused_only:
            print("%2d %-28s %7d %4d %6.1f | %22s | %s |" % (li, name, V, C, V * C * 4e-6, "", cell(t["fused"])))
            continue
        ratio = t["fused"][1] / t["modules"][1]
        print("%2d %-28s %7d %4d %6.1f | %s | %s | %.3f" % (li, name, V, C, V * C * 4e-6, cell(t["modules"]), cell(t["fused"]), ratio))
        if not t["fused"][2] < t["modules"][0]:
            not_faster.append("%d (%s, %d x %d)" % (li, name, V, C))
    print("sum over the 16 blocks (%.1f M floats, %.1f MB):" % (total * 1e-6, total * 4e-6))
    for k in names:
        print("  %-8s %8.1f us  [sums of the blocks' minima and maxima: %.1f - %.1f]" % (k, sums[k][1], sums[k][0], sums[k][2]))
    print("the fused form's calls alone, summed over the 16 blocks (us incl. the call's allocations; bytes that have to move / "
          "time; share of 6.3 TB/s):")
    for k, what in (("fwd", "k_bn_sums, k_bn_finish, k_bn_apply"), ("bwd sums", "k_bn_sums, k_bn_finish"),
                    ("bwd all", "k_bn_sums, k_bn_finish, k_bn_dx")):
        rate = part_bytes[k] / (sums[k][1] * 1e-6)
        print("  %-9s (%-34s) %8.1f [%8.1f - %8.1f] us  %8.1f MB  %7.1f GB/s  %5.1f %%" % (
            k, what, sums[k][1], sums[k][0], sums[k][2], part_bytes[k] * 1e-6, rate * 1e-9, 100.0 * rate / COPY_RATE))
    if not args.fused_only:
        print("blocks on which \"fused\" is not faster with disjoint block ranges: %s" % (", ".join(not_faster) or "none"))
    if ctx:
        ctx.__exit__(None, None, None)


if __name__ == "__main__":
    main()
