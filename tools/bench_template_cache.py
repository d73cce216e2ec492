#!/usr/bin/env python3
"""The eval forward with and without the per-class template cache (Network.cache_templates, data["tmp_cls"]), both forms
alternating in ONE process on the same network, weights and crops.

  tools/bench_template_cache.py [--cases NAME ...] [--blocks 5] [--reps 20]
  tools/bench_template_cache.py --trace-run plain|cached --steps K       (the subject of a rocprofv3 --kernel-trace --stats run)
  tools/bench_template_cache.py --trace-diff PLAIN.csv CACHED.csv --steps K [--trace-base PLAIN0.csv CACHED0.csv]

cases (N / M = points of the observed / template side):
  ref32_lbl      32 x 1024 / 1024, launch by launch (graph_max_batch=0)      ref32      the same under default routing (graph replay)
  six_lbl         6 x 1024 / 1024, launch by launch                           six        the same under default routing (graph replay)
  lm1             1 x 1024 / 1024, 5 mm voxels: the LineMOD stream's call (graph replay)
  stress32       32 x 12288 / 2048 (default routing = launch by launch at this size)
Per case: `blocks` blocks, each `reps` calls of the plain form, then `reps` calls of the cached form, each timed from the first
call to a device synchronisation behind the last; reported is the median block of each form with the range over the blocks, and
the graphs' node counts where a form replays one.  A gain is CLAIMED only where the two ranges are disjoint.
Also: the template_rows launch alone (device events) at every case's shape -- bytes moved (read + written) and the rate beside
the 6.3 TB/s the chip copies at (tools/bw_probe.py) -- and the cache's size beside the 256 MB last-level cache.

--trace-run: W warm-up calls and K timed-like calls of ONE form at 32 x 1024 / 1024, launch by launch -- run it under
`rocprofv3 --kernel-trace --stats` (no counters), once per form, each as a process of its own.
--trace-diff: the two runs' kernel_stats summaries -> kernel time and launches per step and every kernel whose launch count
differs.  A summary holds the warm-up and (cached form) the cache's one-time fill as well: --trace-base takes the summaries of
two more runs with FEWER steps (--steps 0), which are subtracted, so that what is left is K steps and nothing else."""
import argparse
import csv
import importlib
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {
    "ref32_lbl": (32, 1024, 1024, 0.006, {"graph_max_batch": 0}),
    "ref32": (32, 1024, 1024, 0.006, {}),
    "six_lbl": (6, 1024, 1024, 0.006, {"graph_max_batch": 0}),
    "six": (6, 1024, 1024, 0.006, {}),
    "lm1": (1, 1024, 1024, 0.005, {}),
    "stress32": (32, 12288, 2048, 0.006, {}),
}
COPY_RATE = 6.3e12            # bytes / s of a device-to-device copy on this chip (tools/bw_probe.py), read + written counted once each
LLC_BYTES = 256 << 20


def kernel_key(name):
    n = name.replace("(anonymous namespace)::", "")
    n = re.sub(r"^void ", "", n)
    return n.split("(")[0].strip()


def read_stats(path):
    tab = {}
    for row in csv.DictReader(open(path)):
        k = kernel_key(row["Name"])
        c, ns = tab.get(k, (0, 0))
        tab[k] = (c + int(row["Calls"]), ns + int(row["TotalDurationNs"]))
    return tab


def trace_diff(paths, base, steps):
    tabs = [read_stats(p) for p in paths]
    if base:
        for tab, p in zip(tabs, base):
            for k, (c, ns) in read_stats(p).items():
                c0, ns0 = tab.get(k, (0, 0))
                tab[k] = (c0 - c, ns0 - ns)
    steps = max(1, steps)
    names = ("plain", "cached")
    for name, tab in zip(names, tabs):
        calls, ns = sum(c for c, _ in tab.values()), sum(ns for _, ns in tab.values())
        print("%-7s %8.3f ms of kernel time and %7.1f launches per step (%d steps%s)"
              % (name, ns / steps / 1e6, calls / steps, steps, ", baseline runs subtracted" if base else ""))
    d_ns = sum(ns for _, ns in tabs[1].values()) - sum(ns for _, ns in tabs[0].values())
    print("cached - plain: %+.3f ms of kernel time per step" % (d_ns / steps / 1e6))
    print("kernels whose launch count differs (launches per step, us per step: plain -> cached):")
    for k in sorted(set(tabs[0]) | set(tabs[1]), key=lambda k: -abs(tabs[0].get(k, (0, 0))[1] - tabs[1].get(k, (0, 0))[1])):
        (c0, n0), (c1, n1) = tabs[0].get(k, (0, 0)), tabs[1].get(k, (0, 0))
        if c0 != c1:
            print("  %-64s %6.1f -> %6.1f   %8.1f -> %8.1f" % (k[:64], c0 / steps, c1 / steps, n0 / steps / 1e3, n1 / steps / 1e3))


def setup(dcl, torch, b, n_inp, n_tmp, unit, kw):
    dev = torch.device("cuda:0")
    net = dcl.DCL_Net.Network(dcl.synth.default_cfg(n_inp, n_tmp, unit), mode="test", **kw)
    net.load_state_dict(dcl.synth.synth_state_dict(net, 1))
    net = net.to(dev).eval()
    data = dcl.synth.make_batch(b, n_inp, n_tmp, unit=unit)
    classes = sorted(set(data["obj_idx"].tolist()))
    net.cache_templates({c: dcl.synth.class_template_side(c, n_tmp, unit) for c in classes}, [64, 64, 64])
    move = lambda v: v.to(dev) if torch.is_tensor(v) else v                      # noqa: E731
    plain = {k: ({kk: move(vv) for kk, vv in v.items()} if isinstance(v, dict) else v) for k, v in data.items()}
    cached = {k: v for k, v in plain.items() if k != "tmp"}
    cached["labels"] = dict(plain["labels"])
    cached["tmp_cls"] = data["obj_idx"].to(dev).int()
    return net, plain, cached


def scatter_alone(dcl, torch, net, b, reps=50):
    """the one template_rows launch of a call of b crops, alone: ms, bytes read + written, rate"""
    cache = net.template_cache
    dev = cache.rows.device
    n = net.n_tmp
    act = net._disengage_buffers("Yo", b * n, dev, fuse=None)
    pts = torch.empty((b * n, 3), dtype=torch.float32, device=dev)
    cls = torch.tensor([cache.class_ids[i % len(cache.class_ids)] for i in range(b)], dtype=torch.int32, device=dev)
    blocks = net._template_blocks(act, pts)
    for _ in range(5):
        dcl.ops.template_rows(cache.rows, cache.lut, cls, blocks, cache.miss)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        dcl.ops.template_rows(cache.rows, cache.lut, cls, blocks, cache.miss)
    ev[1].record()
    torch.cuda.synchronize()
    ms = ev[0].elapsed_time(ev[1]) / reps
    nbytes = 2 * b * n * 643 * 4
    return ms, nbytes


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", nargs="*", default=list(CASES), choices=list(CASES))
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trace-run", choices=("plain", "cached"), default=None)
    ap.add_argument("--trace-diff", nargs=2, default=None)
    ap.add_argument("--trace-base", nargs=2, default=None)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if args.trace_diff:
        return trace_diff(args.trace_diff, args.trace_base, args.steps)
    if args.blocks < 3:
        ap.error("--blocks: at least 3 (a median with a range)")

    import torch
    dcl = importlib.import_module("dcl-net_amd")

    if args.trace_run:
        b, n_inp, n_tmp, unit, kw = CASES["ref32_lbl"]
        net, plain, cached = setup(dcl, torch, b, n_inp, n_tmp, unit, kw)
        d = plain if args.trace_run == "plain" else cached
        with torch.no_grad():
            for _ in range(args.warmup + args.steps):
                net(d)
        torch.cuda.synchronize()
        print("trace-run %s: %d warm-up + %d steps of %d x %d / %d launch by launch" % (args.trace_run, args.warmup, args.steps, b,
                                                                                     n_inp, n_tmp))
        return

    def timed(net, d, reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            net(d)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps * 1e3

    print("ms per call: median of %d blocks of %d calls [min .. max]; forms alternate block by block in one process" % (args.blocks,
                                                                                                                  args.reps))
    for name in args.cases:
        b, n_inp, n_tmp, unit, kw = CASES[name]
        reps = max(3, args.reps // 4) if n_inp > 4096 else args.reps
        net, plain, cached = setup(dcl, torch, b, n_inp, n_tmp, unit, kw)
        t = {"plain": [], "cached": []}
        with torch.no_grad():
            for d in (plain, cached):                                            # captures, lazy initialisation, allocator
                for _ in range(10 if net.replays_graph(b) else 3):
                    net(d)
            for _ in range(args.blocks):
                t["plain"].append(timed(net, plain, reps))
                t["cached"].append(timed(net, cached, reps))
        assert int(net.template_cache.miss.cpu()[0]) == 0
        route = "graph replay" if net.replays_graph(b) else "launch by launch"
        print("%-10s %2d x %5d / %4d  %-16s" % (name, b, n_inp, n_tmp, route), end="")
        for form in ("plain", "cached"):
            print("  %s %7.3f [%7.3f .. %7.3f]" % (form, statistics.median(t[form]), min(t[form]), max(t[form])), end="")
        disjoint = max(t["cached"]) < min(t["plain"]) or max(t["plain"]) < min(t["cached"])
        delta = statistics.median(t["cached"]) / statistics.median(t["plain"]) - 1.0
        print("  cached/plain %+6.1f %%  ranges %s" % (100 * delta, "disjoint" if disjoint else "OVERLAP: no claim"))
        graphs = net.__dict__.get("_graphs", {})
        if graphs:
            nodes = {("cached" if len(k) == 5 else "plain"): e.get("nodes") for k, e in graphs.items()}
            print("%-10s graph nodes: plain %s, cached %s" % ("", nodes.get("plain"), nodes.get("cached")))
        ms, nbytes = scatter_alone(dcl, torch, net, b)
        cache = net.template_cache
        print("%-10s template_rows alone: %.1f us for %.1f MB read + written = %.2f TB/s (%.0f %% of the %.1f TB/s copy rate); cache "
              "%d classes = %.1f MB, %s the %d MB last-level cache"
              % ("", ms * 1e3, nbytes / 1e6, nbytes / ms / 1e9, 100 * nbytes / (ms * 1e-3) / COPY_RATE, COPY_RATE / 1e12,
                 len(cache.class_ids), cache.nbytes() / 1e6, "inside" if cache.nbytes() <= LLC_BYTES else "beyond", LLC_BYTES >> 20))
        del net, plain, cached
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
