"""Forward + backward of the losses' Chamfer term: losses.cd_dis_fused (autograd.ChamferFn on csrc/chamfer.hip, no pairwise
matrix) against the chunked losses.cd_dis the loss modules use by default (coordinate differences 256 pred rows at a time,
torch autograd, fp32), same inputs, gradient with respect to pred only -- as in the loss, where the target never needs one.

  python tools/bench_chamfer.py [--iters 20] [--warmup 3]

Shapes: 32 x 1024 x 1024 (the shipped batch) with every crop active and with the YCB-V mix of symmetric objects (5 of 21
classes: 8 of 32 crops active; the chunked form has no way to skip a crop and is the same call in both rows), and
4 x 2048 x 2048.  Per shape: median ms of a device-synchronised forward + backward over `iters` repetitions, in blocks that
alternate the two forms in both orders inside one process; the peak of torch.cuda.max_memory_allocated above what was
allocated before the step, in units of one (b, n, m) fp32 map; and the two library calls alone (device events).  Then the
whole losses(...) module, forward + backward, in both modes at 32 x 1024 with the same mix of symmetric crops.
profiles/chamfer.txt holds one run's output."""
import argparse
import importlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

SHAPES = [(32, 1024, 1024, 32, "all crops active"), (32, 1024, 1024, 8, "5/21 of the crops active"),
          (4, 2048, 2048, 4, "all crops active")]


def median_ms(step, iters):
    """host clock around `iters` single steps, each ended by a device synchronise"""
    ts = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        step()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def peak_above_base(step):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    step()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def events_ms(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, z in ev:
        a.record()
        fn()
        z.record()
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(z) for a, z in ev)[len(ev) // 2]


def compare(forms, iters, warmup):
    """{name: step} for two forms -> ({name: median of its three block medians}, blocks in run order)"""
    a, c = list(forms)
    for _ in range(warmup):
        for fn in forms.values():
            fn()
    blocks = []
    for order in ((a, c, a), (c, a, c)):
        for name in order:
            blocks.append((name, median_ms(forms[name], iters)))
    per = {n: sorted(t for k, t in blocks if k == n) for n in forms}
    return {n: v[len(v) // 2] for n, v in per.items()}, per, blocks


def report(mid, per, blocks):
    a, c = list(mid)
    print("  blocks in run order (median ms of forward + backward): " + ", ".join("%s %.3f" % bl for bl in blocks))
    for n in (a, c):
        print("  %-8s %.3f ms (blocks %s)" % (n, mid[n], " ".join("%.3f" % t for t in per[n])))
    print("  %s / %s time = %.3f" % (a, c, mid[a] / mid[c]))


def rand_rot(g, b):
    return torch.linalg.qr(torch.randn(b, 3, 3, generator=g))[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    assert args.iters >= 20, "at least 20 timed repetitions per block"
    if not torch.cuda.is_available():
        raise SystemExit("bench_chamfer: needs the GPU (no CPU timing is meaningful)")
    dcl = importlib.import_module("dcl-net_amd")
    L = dcl.DCL_Net.losses
    print("Chamfer term, forward + backward (gradient to pred): fused (cd_dis_fused, csrc/chamfer.hip) vs chunked (cd_dis, autograd)")
    print("device: %s, torch %s, %d timed repetitions per block after %d warm-up steps" %
          (torch.cuda.get_device_name(0), torch.__version__, args.iters, args.warmup))
    for b, n, m, n_active, what in SHAPES:
        g = torch.Generator().manual_seed(n + m + n_active)
        pred = (torch.randn(b, n, 3, generator=g) * 0.05).cuda().requires_grad_(True)
        target = (torch.randn(b, m, 3, generator=g) * 0.05).cuda()
        sym = torch.zeros(b)
        sym[torch.randperm(b, generator=g)[:n_active]] = 1.0
        sym = sym.cuda()
        active = None if n_active == b else sym != 0
        w = (torch.randn(b, n, generator=g).cuda() * sym.unsqueeze(1)).contiguous()     # the loss multiplies by sym_flag

        def fused():
            pred.grad = None
            (L.cd_dis_fused(pred, target, active) * w).sum().backward()

        def chunked():
            pred.grad = None
            (L.CD_Dis(pred, target) * w).sum().backward()

        forms = {"fused": fused, "chunked": chunked}
        mid, per, blocks = compare(forms, args.iters, args.warmup)
        mem = {name: peak_above_base(fn) for name, fn in forms.items()}
        with torch.no_grad():
            p, act = pred.detach(), None if active is None else active.int()
            t_fwd = events_ms(lambda: dcl.ops.chamfer(p, target, act), args.iters, args.warmup)
            _, idx_pt, _, idx_tp = dcl.ops.chamfer(p, target, act)
            g_tp = torch.randn(b, m, generator=g).cuda()
            t_bwd = events_ms(lambda: dcl.ops.chamfer_backward(p, target, idx_pt, idx_tp, w, g_tp, act, need_target=False),
                              args.iters, args.warmup)
        one_map = b * n * m * 4
        print("\nshape b x n x m = %d x %d x %d, %s   (one (b,n,m) fp32 map: %.1f MiB)" % (b, n, m, what, one_map / 2 ** 20))
        report(mid, per, blocks)
        print("  peak memory above the inputs: fused %.2f MiB (%.4f maps), chunked %.1f MiB (%.2f maps)" %
              (mem["fused"] / 2 ** 20, mem["fused"] / one_map, mem["chunked"] / 2 ** 20, mem["chunked"] / one_map))
        print("  library calls alone (device events): dcl_chamfer_fwd %.4f ms, dcl_chamfer_bwd (grad_pred only) %.4f ms; "
              "%.1f G distance evaluations / s in the forward" % (t_fwd, t_bwd, 2.0 * n_active * n * m / t_fwd / 1e6))
        del pred, target, w
        torch.cuda.empty_cache()

    # the whole loss module: losses(...)(pred, gt)["loss_all"].backward() with tests/test_losses.py's inputs at the shipped shape
    b, n, n_active = 32, 1024, 8
    g = torch.Generator().manual_seed(0)
    sym = torch.zeros(b)
    sym[torch.randperm(b, generator=g)[:n_active]] = 1.0
    names = ("rot_pred", "trans_pred", "conf", "Xo_pred", "Yc_pred")
    pred = {"rot_pred": rand_rot(g, b), "trans_pred": torch.randn(b, 3, generator=g) * 0.01, "sym_flag": sym,
            "conf": torch.rand(b, 2 * n, generator=g) * 0.8 + 0.1,
            "Xo_pred": torch.randn(b, n, 3, generator=g) * 0.05, "Yc_pred": torch.randn(b, n, 3, generator=g) * 0.05}
    pred = {k: v.cuda().requires_grad_(k in names) for k, v in pred.items()}
    gt = {"rot_gt": rand_rot(g, b), "trans_gt": torch.randn(b, 3, generator=g) * 0.01,
          "points_tmp": torch.randn(b, n, 3, generator=g) * 0.05, "points_inp": torch.randn(b, n, 3, generator=g) * 0.05}
    gt = {k: v.cuda() for k, v in gt.items()}
    crit = {mode: L(None, chamfer=mode) for mode in ("fused", "chunked")}

    def module_step(mode):
        def step():
            for k in names:
                pred[k].grad = None
            crit[mode](pred, gt)["loss_all"].backward()
        return step

    forms = {mode: module_step(mode) for mode in crit}
    mid, per, blocks = compare(forms, args.iters, args.warmup)
    mem = {name: peak_above_base(fn) for name, fn in forms.items()}
    one_map = b * n * n * 4
    print("\nlosses(None, chamfer=...) forward + backward, %d x %d points, %d of %d crops symmetric" % (b, n, n_active, b))
    report(mid, per, blocks)
    print("  peak memory above the inputs: fused %.2f MiB (%.4f maps), chunked %.1f MiB (%.2f maps)" %
          (mem["fused"] / 2 ** 20, mem["fused"] / one_map, mem["chunked"] / 2 ** 20, mem["chunked"] / one_map))


if __name__ == "__main__":
    main()
