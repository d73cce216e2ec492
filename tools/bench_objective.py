"""The training objective, forward + backward: losses(..., objective="fused") (csrc/objective.hip: rigid transforms, packed
loss and every gradient on own kernels) against objective="module" (the torch composition), both with chamfer="fused", same
inputs, in one process.

  python tools/bench_objective.py [--iters 20] [--warmup 3] [--no-step] [--launches]

Shapes: `losses` at 32 x 1024 points with half the crops symmetric, `losses_refiner` at 32 x 2620.  Per shape: median ms of a
device-synchronised forward + backward over `iters` repetitions, in blocks that alternate the two forms in both orders
(bench_chamfer.compare).  Then a whole training step, `tools/train_step.py 32 1024 --optim fused --autoclip --chamfer fused`
with each --objective, each in a process of its own, twice in alternation.  --launches: one forward + backward of each form
under torch's profiler, kernel launches counted by name (vendor GEMMs are the Cijk_* rows).  The comparison is against the
module path of the same build.  profiles/objective.txt holds one run's output."""
import argparse
import importlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from bench_chamfer import compare, rand_rot, report  # noqa: E402

LEAVES = ("rot_pred", "trans_pred", "conf", "Xo_pred", "Yc_pred")


def losses_case(dcl, b, n, n_sym):
    g = torch.Generator().manual_seed(0)
    sym = torch.zeros(b)
    sym[torch.randperm(b, generator=g)[:n_sym]] = 1.0
    pred = {"rot_pred": rand_rot(g, b), "trans_pred": torch.randn(b, 3, generator=g) * 0.01, "sym_flag": sym,
            "conf": torch.rand(b, 2 * n, generator=g) * 0.8 + 0.1,
            "Xo_pred": torch.randn(b, n, 3, generator=g) * 0.05, "Yc_pred": torch.randn(b, n, 3, generator=g) * 0.05}
    pred = {k: v.cuda().requires_grad_(k in LEAVES) for k, v in pred.items()}
    gt = {"rot_gt": rand_rot(g, b), "trans_gt": torch.randn(b, 3, generator=g) * 0.01,
          "points_tmp": torch.randn(b, n, 3, generator=g) * 0.05, "points_inp": torch.randn(b, n, 3, generator=g) * 0.05}
    gt = {k: v.cuda() for k, v in gt.items()}
    crit = {mode: dcl.DCL_Net.losses(None, chamfer="fused", objective=mode) for mode in ("fused", "module")}

    def make(mode):
        def step():
            for k in LEAVES:
                pred[k].grad = None
            crit[mode](pred, gt)["loss_all"].backward()
        return step
    return {mode: make(mode) for mode in crit}


def refiner_case(dcl, b, n, n_sym):
    g = torch.Generator().manual_seed(1)
    sym = torch.zeros(b)
    sym[torch.randperm(b, generator=g)[:n_sym]] = 1.0
    pred = {"rot_pred": rand_rot(g, b).cuda().requires_grad_(), "trans_pred": (torch.randn(b, 3, generator=g) * 0.01).cuda().requires_grad_()}
    rot_cur, trans_cur = rand_rot(g, b).cuda(), (torch.randn(b, 3, generator=g) * 0.01).cuda()
    tmp, sym = (torch.randn(b, n, 3, generator=g) * 0.05).cuda(), sym.cuda()
    gt = {"rot_gt": rand_rot(g, b).cuda(), "trans_gt": (torch.randn(b, 3, generator=g) * 0.01).cuda()}
    crit = {mode: dcl.refiner.losses_refiner(None, chamfer="fused", objective=mode) for mode in ("fused", "module")}

    def make(mode):
        def step():
            for v in pred.values():
                v.grad = None
            crit[mode](pred, trans_cur, rot_cur, tmp, sym, gt)["loss_all"].backward()
        return step
    return {mode: make(mode) for mode in crit}


def launches(step):
    """kernel launches of one step by name (torch's profiler; the step has run before, so nothing is compiled or tuned here)"""
    from torch.profiler import ProfilerActivity, profile
    step()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        step()
        torch.cuda.synchronize()
    rows = [(e.key, e.count) for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA
            and not e.key.lower().startswith(("memcpy", "memset"))]
    return sorted(rows, key=lambda r: (-r[1], r[0]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-step", action="store_true", help="skip the whole-training-step runs")
    ap.add_argument("--launches", action="store_true", help="count the kernel launches of one forward + backward")
    args = ap.parse_args()
    assert args.iters >= 20, "at least 20 timed repetitions per block"
    if not torch.cuda.is_available():
        raise SystemExit("bench_objective: needs the GPU (no CPU timing is meaningful)")
    dcl = importlib.import_module("dcl-net_amd")
    print("Training objective, forward + backward: objective='fused' (csrc/objective.hip) vs 'module' (torch), both chamfer='fused'")
    print("device: %s, torch %s, %d timed repetitions per block after %d warm-up steps" %
          (torch.cuda.get_device_name(0), torch.__version__, args.iters, args.warmup))
    for what, forms in (("losses, 32 x 1024 points, 16 of 32 crops symmetric", losses_case(dcl, 32, 1024, 16)),
                        ("losses_refiner, 32 x 2620 points, 16 of 32 crops symmetric", refiner_case(dcl, 32, 2620, 16))):
        print("\n" + what)
        mid, per, blocks = compare(forms, args.iters, args.warmup)
        report(mid, per, blocks)
        if args.launches:
            for mode, step in forms.items():
                rows = launches(step)
                total, vendor = sum(c for _, c in rows), sum(c for k, c in rows if k.startswith("Cijk_"))
                print("  launches of one forward + backward, %s: %d kernels, %d of them vendor GEMMs (Cijk_*)" % (mode, total, vendor))
                for k, c in rows:
                    print("    %3d  %s" % (c, k[:150]))
    if not args.no_step:
        print("\nwhole training step: tools/train_step.py 32 1024 --optim fused --autoclip --chamfer fused --objective ...")
        for mode in ("module", "fused", "module", "fused"):            # a process each, alternating
            out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "train_step.py"), "32", "1024", "--optim", "fused",
                                  "--autoclip", "--chamfer", "fused", "--objective", mode], capture_output=True, text=True, timeout=600)
            if out.returncode != 0:
                raise SystemExit("train_step.py --objective %s failed (exit %d):\n%s" % (mode, out.returncode, out.stderr[-2000:]))
            print("  " + out.stdout.strip().replace("\n", "\n  "))


if __name__ == "__main__":
    main()
