#!/usr/bin/env python3
"""The weight gradient of the per-point linear layers in its two forms, shape by shape:
tools/bench_linear_wgrad.py [--min-block 0.25] [--check] [--only P,Q] [--counters]

  fp32   ops.linear_wgrad        csrc/linear_bwd.hip: v_mfma_f32_32x32x2_f32 on register-staged fp32 slabs
  split  ops.linear_wgrad_split  csrc/linear_wgrad_split.hip: both operands split into three bf16 pieces on the way to LDS, six
                                 piece products per product on v_mfma_f32_32x32x16_bf16 through transposed LDS reads

The shapes (M, P, Q) are recorded, not typed in: every ops.linear_wgrad call of one training step of
Network(**DCL_Net.TRAIN_KERNELS) at 32 x 1024 / 1024 points (autograd.PointLinearFn) and of one forward + backward of
Refiner(train_mlp="kernels") at 20 x 1024 and 32 x 1024 points (autograd.RefinerShareFn), with how often each occurs.  Both
forms include their k_split_sum launch.  The forms alternate inside one process; every figure is the median of three blocks of at
least --min-block seconds each (host clock around launches that end in a device synchronise), printed with the range of the
three.  TFLOP/s = 2 M P Q / t, fp32-equivalent.  --check adds the worst error of both forms against float64 in units of
2^-24 sum_j |a_jp| |b_jq| on the same random operands.  The last lines list the shapes on which "split" was faster with disjoint
block ranges: those belong in ops.WGRAD_SPLIT_SHAPES.  --counters: nothing is timed, every recorded shape runs the split form a
few times -- the subject of a counters-only profiler run (SQ_LDS_BANK_CONFLICT)."""
import argparse
import importlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def recorded_shapes(dcl, torch):
    """{(M, P, Q): [count, who]} of the ops.linear_wgrad calls of the step and the refiner passes named above"""
    ops = dcl.ops
    real = ops.linear_wgrad
    shapes, who = {}, [None]

    def recording(a, b, out=None):
        key = (int(a.shape[0]), int(a.shape[1]), int(b.shape[1]))
        shapes.setdefault(key, [0, who[0]])[0] += 1
        return real(a, b, out=out)
    ops.linear_wgrad = recording
    try:
        b, n = 32, 1024
        who[0] = "Network 32 x 1024 / 1024"
        net = dcl.DCL_Net.Network(dcl.synth.default_cfg(n, n), mode="train", **dcl.DCL_Net.TRAIN_KERNELS)
        net.load_state_dict(dcl.synth.synth_state_dict(net, 1))
        net = net.cuda().train()
        data = dcl.synth.make_batch(b, n, n)
        data["flags"] = torch.zeros(b)
        crit = dcl.DCL_Net.losses(None, chamfer="fused", objective="fused")
        crit(net(data), data["labels"])["loss_all"].backward()
        del net, data, crit
        for b in (20, 32):
            who[0] = "Refiner %d x 1024" % b
            ref = dcl.refiner.Refiner(train_rotation="device", train_mlp="kernels")
            ref.load_state_dict(dcl.synth.synth_state_dict(ref, 2))
            ref = ref.cuda().train()
            g = torch.Generator().manual_seed(4)
            x = torch.cat([torch.randn(b, 3, n, generator=g) * 0.05, torch.randn(b, 256, n, generator=g)], 1).cuda()
            conf = torch.rand(b, 2 * n, generator=g).cuda()
            out = ref({"input_features": x, "conf": conf, "obj_idx": None})
            (out["trans_pred"].sum() + out["rot_pred"].sum()).backward()
            del ref, out
    finally:
        ops.linear_wgrad = real
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return shapes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min-block", type=float, default=0.25)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--only", default=None, help="P,Q: that shape alone")
    ap.add_argument("--counters", action="store_true")
    args = ap.parse_args()

    import torch
    dcl = importlib.import_module("dcl-net_amd")
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    ops = dcl.ops
    shapes = recorded_shapes(dcl, torch)
    if args.only:
        P0, Q0 = (int(v) for v in args.only.split(","))
        shapes = {k: v for k, v in shapes.items() if k[1:] == (P0, Q0)}
    gen = torch.Generator(device="cuda").manual_seed(5)

    def block(fn, iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / iters

    if args.counters:
        for (M, P, Q) in sorted(shapes):
            a, b = torch.randn((M, P), device="cuda", generator=gen), torch.randn((M, Q), device="cuda", generator=gen)
            for _ in range(3):
                ops.linear_wgrad_split(a, b)
        torch.cuda.synchronize()
        print("ran ops.linear_wgrad_split three times on each of %d recorded shapes" % len(shapes))
        return

    print("linear weight gradient, %s; DCL_WGRAD_ROWS = %d; us per call: median of 3 blocks >= %.2f s [range]" % (
        torch.cuda.get_device_name(0), ops.WGRAD_ROWS, args.min_block))
    print("%6s %5s %4s %3s  %-24s | %25s %7s | %25s %7s | %6s%s" % (
        "M", "P", "Q", "x", "from", "fp32 (linear_wgrad)", "TFLOP/s", "split (linear_wgrad_split)", "TFLOP/s", "sp/fp",
        " | units of 2^-24 sum|a||b|: fp32, split" if args.check else ""))
    names = ("fp32", "split")
    sums = {k: [0.0, 0.0, 0.0] for k in names}
    table = {}
    for (M, P, Q), (count, who) in sorted(shapes.items()):
        a, b = torch.randn((M, P), device="cuda", generator=gen), torch.randn((M, Q), device="cuda", generator=gen)
        forms = {"fp32": lambda: ops.linear_wgrad(a, b), "split": lambda: ops.linear_wgrad_split(a, b)}
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
                sums[name][i] += count * t[name][i]
        check = ""
        if args.check:
            want, mag = a.double().t() @ b.double(), a.double().abs().t() @ b.double().abs()
            units = [float(((fn().double() - want).abs() / (mag * 2.0 ** -24)).max()) for fn in forms.values()]
            check = " | %6.2f, %6.2f" % tuple(units)
            del want, mag
        cell = lambda v: "%7.1f [%7.1f-%7.1f]" % (v[1], v[0], v[2])              # noqa: E731
        flop = 2.0 * M * P * Q
        print("%6d %5d %4d %3d  %-24s | %s %7.1f | %s %7.1f | %6.3f%s" % (
            M, P, Q, count, who, cell(t["fp32"]), flop / (t["fp32"][1] * 1e-6) / 1e12, cell(t["split"]),
            flop / (t["split"][1] * 1e-6) / 1e12, t["split"][1] / t["fp32"][1], check))
        table.setdefault((P, Q), []).append((M, t["split"][2] < t["fp32"][0]))    # disjoint ranges, "split" below
        del a, b
    for name in names:
        print("sum over the recorded calls, %-5s: %9.1f us  [sums of the blocks' minima and maxima: %.1f - %.1f]" % (
            name, sums[name][1], sums[name][0], sums[name][2]))
    measured = {}
    for key, rows in table.items():                                              # the fewest rows from which every recorded M won
        for M, faster in sorted(rows, reverse=True):
            if not faster:
                break
            measured[key] = M
    print("measured table {(P, Q): fewest rows}: %s; ops.WGRAD_SPLIT_SHAPES: %s" % (measured, dict(ops.WGRAD_SPLIT_SHAPES)))


if __name__ == "__main__":
    main()
