#!/usr/bin/env python3
"""The sparse-conv weight gradient in its two forms, layer by layer, on the rulebooks of a training batch:
tools/bench_conv_wgrad.py [b] [N] [--min-block 0.25] [--lib PATH]
tools/bench_conv_wgrad.py --trace-stats KERNEL_STATS.csv --steps 13

  rows    ops.sparse_conv_backward(need_dx=False, wgrad="rows"): csrc/backward.hip walks every output row of every offset
  pairs   wgrad="pairs": ops.conv_pairs (the ordered pair list, built in the call) + ops.sparse_conv_wgrad_pairs
          (csrc/conv_wgrad_pairs.hip)
  list    ops.conv_pairs alone

The layers are the 16 sparse-convolution calls of one train-mode forward of Network on synth.make_batch(b, N, N) -- both
backbones, recorded with their input features, rulebooks and row counts.  The three forms alternate inside one process; every
figure is the median of three blocks of at least --min-block seconds each (host clock around launches that end in a device
synchronise), printed with the range of the three.  Useful TFLOP/s = 2 pairs cin cout / t.  --lib: call into another build of the
library (the same sources with another DCL_CONV_PAIRS_SPLIT) through _native.diagnostic_library.

--trace-stats: the 15 largest kernel families (template arguments folded) of a rocprofv3 --kernel-trace --stats run of
tools/train_step.py, by summed time per step."""
import argparse
import csv
import importlib
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def trace_stats(path, steps):
    fam = {}
    for row in csv.DictReader(open(path)):
        name = row["Name"].replace("(anonymous namespace)::", "")
        name = re.sub(r"^void ", "", name).split("(")[0]
        name = re.sub(r"<.*", "", name).strip()
        t, c = fam.get(name, (0.0, 0))
        fam[name] = (t + float(row["TotalDurationNs"]), c + int(row["Calls"]))
    total = sum(t for t, _ in fam.values())
    print("kernel time per step: %.2f ms over %d steps; the 15 largest kernel families:" % (total / steps / 1e6, steps))
    print("  %-58s %10s %9s %7s" % ("family", "us / step", "calls/st", "share"))
    for name, (t, c) in sorted(fam.items(), key=lambda kv: -kv[1][0])[:15]:
        print("  %-58s %10.1f %9.1f %6.1f%%" % (name[:58], t / steps / 1e3, c / steps, 100.0 * t / total))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("b", type=int, nargs="?", default=32)
    ap.add_argument("n", type=int, nargs="?", default=1024)
    ap.add_argument("--min-block", type=float, default=0.25)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--trace-stats", default=None)
    ap.add_argument("--steps", type=int, default=13)
    args = ap.parse_args()
    if args.trace_stats:
        return trace_stats(args.trace_stats, args.steps)

    import torch
    dcl = importlib.import_module("dcl-net_amd")
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    ops = dcl.ops
    conv_mod = importlib.import_module("dcl-net_amd.spconv.conv")
    real = conv_mod.SparseConvFn
    calls = []

    class Recorder(object):
        @staticmethod
        def apply(features, W, nbr, n_out, subm, *forms):
            calls.append((features.detach(), W.detach(), nbr, int(n_out), bool(subm)))
            return real.apply(features, W, nbr, n_out, subm, *forms)

    b, n = args.b, args.n
    net = dcl.DCL_Net.Network(dcl.synth.default_cfg(n, n), mode="train")
    net.load_state_dict(dcl.synth.synth_state_dict(net, 1))
    net = net.cuda().train()
    data = dcl.synth.make_batch(b, n, n)
    data["flags"] = torch.zeros(b)
    conv_mod.SparseConvFn = Recorder
    try:
        with torch.no_grad():
            net(data)
    finally:
        conv_mod.SparseConvFn = real
    torch.cuda.synchronize()
    assert len(calls) == 16, len(calls)

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

    print("sparse-conv weight gradient, b = %d, N = M = %d, library %s; us per call: median of 3 blocks >= %.2f s [range]" % (
        b, n, args.lib or "product", args.min_block))
    print("%2s %-9s %4s %7s %7s %8s %7s | %21s | %21s | %19s | %7s" % (
        "#", "layer", "subm", "n_in", "rows", "pairs", "fill", "rows form", "pairs form (with list)", "list alone", "TFLOP/s"))
    sums = {"rows": [0.0, 0.0, 0.0], "pairs": [0.0, 0.0, 0.0], "list": [0.0, 0.0, 0.0]}
    slower = []
    for li, (f, W, nbr, n_out, subm) in enumerate(calls):
        cin, cout = W.shape[-2], W.shape[-1]
        n_in = f.shape[0]
        f = f.contiguous()
        W = W.reshape(-1, cin, cout).contiguous()
        g = torch.randn((n_out, cout), device="cuda", generator=gen)
        P = ops.conv_pairs(nbr, n_out, n_in, check=True)
        npairs = int(P.counts()[1][-1])
        forms = {
            "rows": lambda: ops.sparse_conv_backward(f, W, g, nbr, n_out, subm, need_dx=False, wgrad="rows"),
            "pairs": lambda: ops.sparse_conv_backward(f, W, g, nbr, n_out, subm, need_dx=False, wgrad="pairs"),
            "list": lambda: ops.conv_pairs(nbr, n_out, n_in),
        }
        a, c = forms["rows"]()[1], forms["pairs"]()[1]
        rel = float((a - c).abs().max()) / max(float(a.abs().max()), 1e-30)
        assert rel < 1e-4, (li, rel)                                             # the same gradient, up to the order of summation
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
            for i in range(3):
                sums[name][i] += t[name][i]
        cell = lambda v: "%7.1f [%5.1f-%6.1f]" % (v[1], v[0], v[2])               # noqa: E731
        print("%2d %3d->%-4d %4s %7d %7d %8d %6.1f%% | %s | %s | %s | %7.2f" % (
            li, cin, cout, "yes" if subm else "no", n_in, n_out, npairs, 100.0 * npairs / (27.0 * max(n_out, 1)), cell(t["rows"]),
            cell(t["pairs"]), cell(t["list"])[2:], 2.0 * npairs * cin * cout / (t["pairs"][1] * 1e-6) / 1e12))
        if t["pairs"][1] >= t["rows"][1]:
            slower.append("layer %d (%d -> %d): rows %.1f us, pairs %.1f us" % (li, cin, cout, t["rows"][1], t["pairs"][1]))
    for name in ("rows", "pairs", "list"):
        print("sum of the 16 calls, %-5s: %8.1f us  [sums of the blocks' minima and maxima: %.1f - %.1f]" % (
            name, sums[name][1], sums[name][0], sums[name][2]))
    disjoint = sums["pairs"][2] < sums["rows"][0] or sums["rows"][2] < sums["pairs"][0]
    print("pairs / rows = %.3f (block ranges %s)" % (sums["pairs"][1] / sums["rows"][1], "disjoint" if disjoint else "OVERLAP"))
    print("layers on which \"pairs\" is not faster: %s" % ("; ".join(slower) if slower else "none"))
    if ctx:
        ctx.__exit__(None, None, None)


if __name__ == "__main__":
    main()
