#!/usr/bin/env python3
"""The eval refine loop (models/refiner.py: refine_loop) in its two forms -- compose="host" (torch expressions and vendor GEMMs
compose the pose between the iterations) and compose="device" (the pose stays in device arrays, five launches of the library's
own kernels per iteration) -- alternating in ONE process on the same refiner, weights and inputs.

  tools/bench_refine_loop.py [--crops 1 6 32] [--blocks 5] [--reps 50]
  tools/bench_refine_loop.py --trace-diff [--crops 32] [--steps 20]
  tools/bench_refine_loop.py --trace-run host|device --crops B --steps K     (what --trace-diff runs under the profiler)

Timing: iteration = 2, n = 1024 points per crop, every b of --crops, launch by launch (graph=False) and as a graph replay
(graph=True).  Per case `blocks` blocks, each `reps` calls of the "host" form, then `reps` calls of the "device" form, each timed
from the first call to a device synchronisation behind the last; reported is the median block of each form with the range over
the blocks, and the graphs' node counts where the runtime tells them.  One form is called faster only where the two ranges are
disjoint.  The result is also checked: both forms must agree within 1e-4 / 1e-5 (rotation / translation).

--trace-diff: per form two `rocprofv3 --kernel-trace --stats` runs (no counters) of --trace-run, with K steps and with 0 steps,
each a fresh child process under its own `timeout -k 10`; the 0-step run (warm-up, weight preparation) is subtracted, so what is
left is K calls of the loop and nothing else.  Listed: launches and kernel time per loop, the vendor GEMMs' (Cijk_*) share, and
every kernel of a call.  The parent process never opens the GPU; after a child that fails no further child is started."""
import argparse
import csv
import glob
import importlib
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_POINTS, ITERATION = 1024, 2
FORMS = ("host", "device")
R_TOL, T_TOL = 1e-4, 1e-5


def kernel_key(name):
    n = name.replace("(anonymous namespace)::", "")
    n = re.sub(r"^void ", "", n)
    return n.split("(")[0].strip()


def setup(dcl, torch, b, n=N_POINTS, seed=1):
    ref = dcl.refiner.Refiner()
    ref.load_state_dict(dcl.synth.synth_state_dict(ref, 2))
    ref = ref.cuda().eval()
    g = torch.Generator().manual_seed(seed)
    q, _ = torch.linalg.qr(torch.randn(b, 3, 3, generator=g, dtype=torch.float64))
    pred = {"rot_pred": q.float().cuda(), "trans_pred": (torch.randn(b, 3, generator=g) * 0.02).cuda(),
            "F_Xo_p": torch.randn(b, 256, n, generator=g).cuda(), "conf": torch.rand(b, 2 * n, generator=g).cuda()}
    pts = (torch.randn(b, n, 3, generator=g) * 0.05).cuda()
    return ref, pred, pts


def trace_run(form, b, steps, warmup):
    import torch
    dcl = importlib.import_module("dcl-net_amd")
    ref, pred, pts = setup(dcl, torch, b)
    for _ in range(warmup + steps):
        dcl.refiner.refine_loop(ref, pred, pts, ITERATION, compose=form)
    torch.cuda.synchronize()
    print("trace-run %s: %d warm-up + %d calls of the loop, %d x %d, iteration %d, launch by launch" % (form, warmup, steps, b, N_POINTS,
                                                                                                    ITERATION))


def read_stats(path):
    tab = {}
    for row in csv.DictReader(open(path)):
        k = kernel_key(row["Name"])
        c, ns = tab.get(k, (0, 0))
        tab[k] = (c + int(row["Calls"]), ns + int(row["TotalDurationNs"]))
    return tab


def profiled(form, b, steps, warmup, limit):
    """kernel_stats of one child run under the profiler, or None when the child failed"""
    with tempfile.TemporaryDirectory(prefix="refine_loop_trace_") as d:
        cmd = ["timeout", "-k", "10", str(limit), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
               sys.executable, os.path.abspath(__file__), "--trace-run", form, "--crops", str(b), "--steps", str(steps), "--warmup",
               str(warmup)]
        rc = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if rc.returncode != 0:
            print("the %s run (%d steps) ended with status %d:\n%s" % (form, steps, rc.returncode, rc.stdout[-2000:]))
            return None
        found = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if len(found) != 1:
            print("the %s run (%d steps) left %d kernel_stats files" % (form, steps, len(found)))
            return None
        return read_stats(found[0])


def trace_diff(b, steps, warmup, limit):
    steps = max(1, steps)
    tabs = {}
    for form in FORMS:
        full = profiled(form, b, steps, warmup, limit)
        base = profiled(form, b, 0, warmup, limit) if full is not None else None
        if full is None or base is None:
            return 1                                         # no further child after one that failed
        tabs[form] = {k: (full.get(k, (0, 0))[0] - base.get(k, (0, 0))[0], full.get(k, (0, 0))[1] - base.get(k, (0, 0))[1])
                      for k in set(full) | set(base)}
    print("kernel trace, %d x %d, iteration %d, launch by launch: %d calls of the loop per form, the 0-call runs subtracted"
          % (b, N_POINTS, ITERATION, steps))
    for form in FORMS:
        tab = tabs[form]
        calls, ns = sum(c for c, _ in tab.values()), sum(t for _, t in tab.values())
        vc, vns = sum(c for k, (c, _) in tab.items() if k.startswith("Cijk_")), sum(t for k, (_, t) in tab.items() if k.startswith("Cijk_"))
        print("%-7s %6.1f launches and %8.1f us of kernel time per loop; of these Cijk_* (vendor GEMM): %5.1f launches, %7.1f us"
              % (form, calls / steps, ns / steps / 1e3, vc / steps, vns / steps / 1e3))
    print("kernels of a call (launches per loop, us per loop: host -> device):")
    keys = set(tabs["host"]) | set(tabs["device"])
    for k in sorted(keys, key=lambda k: -max(tabs["host"].get(k, (0, 0))[1], tabs["device"].get(k, (0, 0))[1])):
        (c0, n0), (c1, n1) = tabs["host"].get(k, (0, 0)), tabs["device"].get(k, (0, 0))
        if c0 or c1:
            print("  %-64s %5.1f -> %5.1f   %7.1f -> %7.1f" % (k[:64], c0 / steps, c1 / steps, n0 / steps / 1e3, n1 / steps / 1e3))
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--crops", nargs="*", type=int, default=None)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--trace-run", choices=FORMS, default=None)
    ap.add_argument("--trace-diff", action="store_true")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds a profiled child run may take")
    args = ap.parse_args()
    if args.trace_run:
        return trace_run(args.trace_run, (args.crops or [32])[0], args.steps, args.warmup)
    if args.trace_diff:
        return trace_diff((args.crops or [32])[0], args.steps, args.warmup, args.limit)
    if args.blocks < 3:
        ap.error("--blocks: at least 3 (a median with a range)")

    import torch
    dcl = importlib.import_module("dcl-net_amd")
    loop = dcl.refiner.refine_loop

    def timed(ref, pred, pts, form, graph, reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            loop(ref, pred, pts, ITERATION, graph=graph, compose=form)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps * 1e3

    print("ms per call of refine_loop (iteration %d, n = %d): median of %d blocks of %d calls [min .. max]; forms alternate block by "
          "block in one process" % (ITERATION, N_POINTS, args.blocks, args.reps))
    for b in (args.crops or [1, 6, 32]):
        ref, pred, pts = setup(dcl, torch, b)
        for graph in (False, True):
            t = {f: [] for f in FORMS}
            out = {}
            for f in FORMS:                                                      # captures, lazy initialisation, allocator
                for _ in range(5):
                    out[f] = loop(ref, pred, pts, ITERATION, graph=graph, compose=f)
            dR, dt = float((out["host"][0] - out["device"][0]).abs().max()), float((out["host"][1] - out["device"][1]).abs().max())
            assert dR <= R_TOL and dt <= T_TOL, (dR, dt)
            for _ in range(args.blocks):
                for f in FORMS:
                    t[f].append(timed(ref, pred, pts, f, graph, args.reps))
            print("b = %2d  %-16s" % (b, "graph replay" if graph else "launch by launch"), end="")
            for f in FORMS:
                print("  %s %7.4f [%7.4f .. %7.4f]" % (f, statistics.median(t[f]), min(t[f]), max(t[f])), end="")
            disjoint = max(t["device"]) < min(t["host"]) or max(t["host"]) < min(t["device"])
            delta = statistics.median(t["device"]) / statistics.median(t["host"]) - 1.0
            print("  device/host %+6.1f %%  ranges %s  (|dR| %.1e, |dt| %.1e)" % (100 * delta, "disjoint" if disjoint else
                                                                                "OVERLAP: no claim", dR, dt))
            if graph:
                nodes = {("device" if k[-1] == "device" else "host"): dcl.DCL_Net.Network._graph_nodes(e[0])
                         for k, e in ref._graphs.items()}
                print("%-24s graph nodes: host %s, device %s" % ("", nodes.get("host"), nodes.get("device")))
        del ref, pred, pts
        torch.cuda.empty_cache()


if __name__ == "__main__":
    sys.exit(main())
