#!/usr/bin/env python3
"""The sparse-conv input gradient in its two forms, layer by layer, on the rulebooks of a training batch:
tools/bench_conv_dgrad.py [b] [N] [--min-block 0.25] [--lib PATH]

  conv    what ops.sparse_conv_backward(dgrad="conv") runs for dX: ops.rulebook_transpose, the per-offset transposed copy of W,
          and the forward dispatcher on both (csrc/sparse_conv.hip)
  direct  dgrad="direct": ops.rulebook_transpose + ops.sparse_conv_dgrad (csrc/conv_dgrad.hip), W as registered
  inv     ops.rulebook_transpose alone, which both forms contain

The layers are the 16 sparse-convolution calls of one train-mode forward of Network on synth.make_batch(b, N, N) -- both
backbones, recorded with their rulebooks and row counts, as tools/bench_conv_wgrad.py records them; the first call of each
backbone has no input gradient and is left out.  The forms alternate inside one process; every figure is the median of three
blocks of at least --min-block seconds each (host clock around launches that end in a device synchronise), printed with the
range of the three.  Useful TFLOP/s = 2 pairs cin cout / t.  The last lines list, width by width, whether "direct" was faster
with disjoint block ranges on the layers of BOTH backbones: those widths belong in ops.CONV_DGRAD_DIRECT_WIDTHS.  --lib: call into
another build of the library (the same sources with other tile shapes) through _native.diagnostic_library."""
import argparse
import importlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("b", type=int, nargs="?", default=32)
    ap.add_argument("n", type=int, nargs="?", default=1024)
    ap.add_argument("--min-block", type=float, default=0.25)
    ap.add_argument("--lib", default=None)
    args = ap.parse_args()

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
            calls.append((features.shape[0], W.detach(), nbr, int(n_out), bool(subm), bool(features.requires_grad)))
            return real.apply(features, W, nbr, n_out, subm, *forms)

    b, n = args.b, args.n
    net = dcl.DCL_Net.Network(dcl.synth.default_cfg(n, n), mode="train")
    net.load_state_dict(dcl.synth.synth_state_dict(net, 1))
    net = net.cuda().train()
    data = dcl.synth.make_batch(b, n, n)
    data["flags"] = torch.zeros(b)
    conv_mod.SparseConvFn = Recorder
    try:
        net(data)                                                                # (with autograd: which calls need a dX)
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

    print("sparse-conv input gradient, b = %d, N = M = %d, library %s; us per call: median of 3 blocks >= %.2f s [range]" % (
        b, n, args.lib or "product", args.min_block))
    print("%2s %-9s %4s %7s %7s %8s | %22s | %22s | %19s | %14s" % (
        "#", "layer", "subm", "n_in", "n_out", "pairs", "conv (inv + W^T + fwd)", "direct (inv + kernel)", "inv alone",
        "TFLOP/s cv / di"))
    names = ("conv", "direct", "inv")
    sums = {k: [0.0, 0.0, 0.0] for k in names}
    verdict = {}
    for li, (n_in, W, nbr, n_out, subm, need_dx) in enumerate(calls):
        cin, cout = W.shape[-2], W.shape[-1]
        if not need_dx:
            print("%2d %3d->%-4d %4s %7d %7d          (no input gradient: the features are data)" % (
                li, cin, cout, "yes" if subm else "no", n_in, n_out))
            continue
        W = W.reshape(-1, cin, cout).contiguous()
        kvol = W.shape[0]
        g = torch.randn((n_out, cout), device="cuda", generator=gen)
        npairs = int(((nbr[:, :n_out] >= 0) & (nbr[:, :n_out] < n_in)).sum())

        def conv_form():
            inv = ops.rulebook_transpose(nbr, n_out, n_in)
            Wt = W.reshape(kvol, cin, cout).transpose(1, 2).contiguous()
            return ops.sparse_conv(g, inv, n_in, Wt, subm)

        def direct_form():
            return ops.sparse_conv_dgrad(g, ops.rulebook_transpose(nbr, n_out, n_in), n_in, W)

        forms = {"conv": conv_form, "direct": direct_form, "inv": lambda: ops.rulebook_transpose(nbr, n_out, n_in)}
        a, c = forms["conv"](), forms["direct"]()
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
        cell = lambda v: "%7.1f [%6.1f-%6.1f]" % (v[1], v[0], v[2])               # noqa: E731
        flop = 2.0 * npairs * cin * cout
        print("%2d %3d->%-4d %4s %7d %7d %8d | %s | %s | %s | %6.2f / %6.2f" % (
            li, cin, cout, "yes" if subm else "no", n_in, n_out, npairs, cell(t["conv"]), cell(t["direct"]), cell(t["inv"])[1:],
            flop / (t["conv"][1] * 1e-6) / 1e12, flop / (t["direct"][1] * 1e-6) / 1e12))
        faster = t["direct"][2] < t["conv"][0]                                   # disjoint ranges, "direct" below
        verdict.setdefault((cin, cout), []).append((li, faster, t["conv"][1], t["direct"][1]))
    for name in names:
        print("sum of the calls with a dX, %-6s: %8.1f us  [sums of the blocks' minima and maxima: %.1f - %.1f]" % (
            name, sums[name][1], sums[name][0], sums[name][2]))
    print("width table (\"direct\" faster with disjoint block ranges on every layer of the width):")
    for (cin, cout), rows in verdict.items():
        print("  %3d -> %-3d  %-3s  %s" % (cin, cout, "yes" if all(r[1] for r in rows) else "no", "; ".join(
            "layer %d: conv %.1f, direct %.1f us" % (r[0], r[2], r[3]) for r in rows)))
    table = sorted(w for w, rows in verdict.items() if all(r[1] for r in rows))
    print("measured table: %s; ops.CONV_DGRAD_DIRECT_WIDTHS: %s" % (table, sorted(ops.CONV_DGRAD_DIRECT_WIDTHS)))
    if ctx:
        ctx.__exit__(None, None, None)


if __name__ == "__main__":
    main()
