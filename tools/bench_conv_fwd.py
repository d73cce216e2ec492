#!/usr/bin/env python3
"""The sparse-conv forward in its two forms, layer by layer, on the rulebooks of a training batch:
tools/bench_conv_fwd.py [b] [N] [--min-block 0.25]
tools/bench_conv_fwd.py --trace-diff TILES_KERNEL_STATS.csv COMPACT_KERNEL_STATS.csv --steps 13     (or the two results.db files)

  tiles       ops.sparse_conv(form="tiles"): the dispatcher of csrc/sparse_conv.hip, as the differentiable path calls it (no
              epilogue, no row order), its scratch allocation included
  compact64   ops.sparse_conv(form="compact") (csrc/conv_fwd_compact.hip) with 64 output rows per tile
  compact128  the same with 128 rows per tile

The layers are the 16 sparse-convolution calls of one train-mode forward of Network on synth.make_batch(b, N, N) -- the eight
layers of both backbones, recorded with their rulebooks and row counts, as tools/bench_conv_dgrad.py records them.  All three
run in the DIAGNOSTIC library (tools/_bin/libdclnet_hip_diag.so: the same sources; dcl_debug_conv_fwd_compact_bm picks the rows
per tile) and alternate inside one process; every figure is the median of three blocks of at least --min-block seconds each,
timed with device events around the block's launches, printed with the range of the three.  density = present pairs / the (row,
offset) slots the 128-row tiles of "tiles" execute (every offset that any row of a tile has, for all 128 rows).  Useful TFLOP/s
= 2 pairs cin cout / t.  The last lines list, for the three dilating widths 32 -> 32, 64 -> 64 and 128 -> 128, whether the
compact form at the library's own choice of rows per tile was faster with disjoint block ranges on the layers of BOTH backbones:
those widths belong in ops.CONV_FWD_COMPACT_WIDTHS.
--trace-diff: two rocprofv3 --kernel-trace --stats summaries of the same training step (tools/train_step.py), the first with
--conv-fwd tiles and the second with compact: kernel time per step, and every kernel whose launch count differs."""
import argparse
import csv
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DILATING = ((32, 32), (64, 64), (128, 128))


def trace_diff(paths, steps):
    tabs = []
    for path in paths:
        tab = {}
        if path.endswith(".db"):                                                 # the profiler's database form of the same summary
            import sqlite3
            for name, calls, ns in sqlite3.connect(path).execute('select name, count(*), sum("end" - start) from kernels group by name'):
                tab[name] = (float(ns) / 1e3, int(calls))
        else:
            for row in csv.DictReader(open(path)):
                t, c = tab.get(row["Name"], (0.0, 0))
                tab[row["Name"]] = (t + float(row["TotalDurationNs"]) / 1e3, c + int(row["Calls"]))
        tabs.append(tab)
    for form, tab in zip(("tiles", "compact"), tabs):
        conv = [v for k, v in tab.items() if "k_sparse_conv" in k or "k_conv_fwd_compact" in k]
        print("  --conv-fwd %-8s kernel time per step %8.2f ms in %7.1f launches; forward-conv kernels (k_sparse_conv*, k_conv_fwd_compact): "
              "%7.1f us in %5.1f launches per step" % (form, sum(t for t, _ in tab.values()) / steps / 1e3,
                                                       sum(c for _, c in tab.values()) / steps, sum(t for t, _ in conv) / steps,
                                                       sum(c for _, c in conv) / steps))
    print("  every kernel whose launch count differs: us per step (launches per step) tiles, compact, difference")
    names = [k for k in set(tabs[0]) | set(tabs[1]) if tabs[0].get(k, (0, 0))[1] != tabs[1].get(k, (0, 0))[1]]
    for k in sorted(names, key=lambda k: tabs[1].get(k, (0, 0))[0] - tabs[0].get(k, (0, 0))[0]):
        (t0, c0), (t1, c1) = tabs[0].get(k, (0.0, 0)), tabs[1].get(k, (0.0, 0))
        print("  %9.1f (%5.1f)  %9.1f (%5.1f)  %+9.1f  %s" % (t0 / steps, c0 / steps, t1 / steps, c1 / steps, (t1 - t0) / steps,
                                                             k.replace("(anonymous namespace)::", "")[:110]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace-diff", nargs=2, default=None)
    ap.add_argument("--steps", type=int, default=13)
    ap.add_argument("b", type=int, nargs="?", default=32)
    ap.add_argument("n", type=int, nargs="?", default=1024)
    ap.add_argument("--min-block", type=float, default=0.25)
    args = ap.parse_args()
    if args.trace_diff:
        return trace_diff(args.trace_diff, args.steps)

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

    def block(fn, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / iters

    with dcl._native.diagnostic_library() as lib:
        default_bm = lambda cout: 128 if cout <= 32 else 64                      # noqa: E731  (csrc/conv_fwd_compact.hip)
        print("sparse-conv forward, b = %d, N = M = %d; us per call: median of 3 blocks >= %.2f s [range], device events" % (
            b, n, args.min_block))
        print("%2s %-9s %4s %7s %7s %8s %7s | %22s | %22s | %22s | %20s" % (
            "#", "layer", "subm", "n_in", "n_out", "pairs", "density", "tiles", "compact, 64-row tiles", "compact, 128-row tiles",
            "TFLOP/s ti / 64 / 128"))
        names = ("tiles", "compact64", "compact128")
        sums = {k: [0.0, 0.0, 0.0] for k in names}
        verdict = {}
        for li, (feat, W, nbr, n_out, subm) in enumerate(calls):
            cin, cout = int(W.shape[-2]), int(W.shape[-1])
            n_in = int(feat.shape[0])
            feat = feat.contiguous()
            W = W.reshape(-1, cin, cout).contiguous()
            present = (nbr[:, :n_out] >= 0) & (nbr[:, :n_out] < n_in)
            npairs = int(present.sum())
            pad = (-n_out) % 128
            tiles = torch.nn.functional.pad(present, (0, pad)).reshape(present.shape[0], -1, 128)
            density = npairs / max(1.0, float(tiles.any(dim=2).sum()) * 128)

            def compact(bm):
                def run():
                    lib.dcl_debug_conv_fwd_compact_bm(bm)
                    return ops.sparse_conv(feat, nbr, n_out, W, subm, form="compact")
                return run

            forms = {"tiles": lambda: ops.sparse_conv(feat, nbr, n_out, W, subm), "compact64": compact(64),
                     "compact128": compact(128)}
            a = forms["tiles"]()
            for name in ("compact64", "compact128"):
                c = forms[name]()
                rel = float((a - c).abs().max()) / max(float(a.abs().max()), 1e-30)
                assert rel < 1e-4, (li, name, rel)                               # the same result, up to the order of summation
            iters = {}
            for name, fn in forms.items():                                       # warm up and size the blocks
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
            cell = lambda v: "%7.1f [%6.1f-%6.1f]" % (v[1], v[0], v[2])           # noqa: E731
            flop = 2.0 * npairs * cin * cout
            print("%2d %3d->%-4d %4s %7d %7d %8d %7.3f | %s | %s | %s | %5.2f / %5.2f / %5.2f" % (
                li, cin, cout, "yes" if subm else "no", n_in, n_out, npairs, density, cell(t["tiles"]), cell(t["compact64"]),
                cell(t["compact128"]), flop / (t["tiles"][1] * 1e-6) / 1e12, flop / (t["compact64"][1] * 1e-6) / 1e12,
                flop / (t["compact128"][1] * 1e-6) / 1e12))
            if not subm and (cin, cout) in DILATING:
                own = t["compact%d" % default_bm(cout)]
                verdict.setdefault((cin, cout), []).append((li, own[2] < t["tiles"][0], t["tiles"][1], own[1], default_bm(cout)))
        lib.dcl_debug_conv_fwd_compact_bm(0)
        for name in names:
            print("sum of the 16 calls, %-10s: %8.1f us  [sums of the blocks' minima and maxima: %.1f - %.1f]" % (
                name, sums[name][1], sums[name][0], sums[name][2]))
        print("width table (\"compact\" faster with disjoint block ranges on every layer of the width):")
        for (cin, cout), rows in verdict.items():
            print("  %3d -> %-3d  %-3s  %s" % (cin, cout, "yes" if all(r[1] for r in rows) else "no", "; ".join(
                "layer %d: tiles %.1f, compact (%d rows) %.1f us" % (r[0], r[2], r[4], r[3]) for r in rows)))
        table = sorted(w for w, rows in verdict.items() if all(r[1] for r in rows))
        print("measured table: %s; ops.CONV_FWD_COMPACT_WIDTHS: %s" % (table, sorted(ops.CONV_FWD_COMPACT_WIDTHS)))


if __name__ == "__main__":
    main()
