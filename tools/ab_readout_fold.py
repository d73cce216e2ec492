#!/usr/bin/env python3
"""Same-job A/B of ops.READOUT_FOLD (0 = read-out of 480 columns + K = 480 GEMM; 1 / 2 = the deepest one / two read-out levels folded
through the first disengage GEMM) on the PRODUCT library: whole launch-by-launch forwards of b crops at the stress shape,
alternating 0 / 1 / 2 in one process, `rounds` rounds; then the reference shape launch by launch, which the selection rule leaves
unfolded (its three columns show that nothing else moved).  Prints the pooled levels' row counts of the stress batch, every
round, and the verdict of the issue's condition: every round of a folded value faster than every round of 0, and the median gain
at least three times the larger of the two forms' round-to-round spreads.
usage: ab_readout_fold.py [rounds=5] [b=32]"""
import importlib, os, statistics, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench
dcl = importlib.import_module("dcl-net_amd")
ops = dcl.ops
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
b = int(sys.argv[2]) if len(sys.argv) > 2 else 32
dev = torch.device("cuda:0")
default = ops.READOUT_FOLD

counts = []
_set_counts = ops.BackboneRun.set_counts
def set_counts(self, c):
    counts.append([int(v) for v in c])
    return _set_counts(self, c)
ops.BackboneRun.set_counts = set_counts

def run(shape, steps, warm):
    n_inp, n_tmp = bench.SHAPES[shape]
    data = bench.to_device(dcl.synth.make_batch(b, n_inp, n_tmp), dev)
    net = dcl.DCL_Net.Network(dcl.synth.default_cfg(n_inp, n_tmp), mode="test", graph_max_batch=0)
    net.load_state_dict(dcl.synth.synth_state_dict(net, 1))
    net = net.to(dev).eval()
    res = {0: [], 1: [], 2: []}
    for rep in range(rounds):
        for fold in (0, 1, 2):
            ops.READOUT_FOLD = fold
            with torch.no_grad():
                for _ in range(warm):
                    net(data)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    net(data)
                torch.cuda.synchronize()
            res[fold].append((time.perf_counter() - t0) / steps * 1e3)
            if rep == 0 and fold == 0 and shape == "stress":
                for side, c in zip(("observed", "template"), counts[-2:]):
                    print("level rows, %s side, b=%d: conv sets %s, pooled levels (32, 64, 128, 256 channels) %s"
                          % (side, b, c[0::2], c[1::2]))
    ops.READOUT_FOLD = default
    for fold in (0, 1, 2):
        print("READOUT_FOLD=%d b=%d N=%d M=%d launch by launch: %s ms  (median %.3f, spread %.3f)"
              % (fold, b, n_inp, n_tmp, " ".join("%.3f" % x for x in res[fold]), statistics.median(res[fold]), max(res[fold]) - min(res[fold])))
    return res

res = run("stress", 10, 3)
for fold in (1, 2):
    gain = statistics.median(res[0]) - statistics.median(res[fold])
    spread = max(max(res[0]) - min(res[0]), max(res[fold]) - min(res[fold]))
    print("READOUT_FOLD=%d against 0: every round faster: %s; median gain %.3f ms (%.1f %%) = %.1f x the larger spread (%.3f ms): %s"
          % (fold, max(res[fold]) < min(res[0]), gain, 100 * gain / statistics.median(res[0]), gain / spread if spread else float("inf"), spread,
             "wins" if max(res[fold]) < min(res[0]) and gain >= 3 * spread else "does not clear the condition"))
run("ref", 40, 5)
