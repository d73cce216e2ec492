"""Stage-2 training of the Refiner with its shared MLP in the two forms of Refiner(train_mlp=):

  modules  the registered nn.Conv1d / nn.ReLU modules: vendor GEMMs for the forward, the input and the weight gradients --
           the default, and the BASELINE of every ratio below
  kernels  autograd.RefinerShareFn: the own GEMM core forward (csrc/linear_dma.hip), dcl_linear_wgrad / dcl_relu_bwd
           (csrc/linear_bwd.hip) and the same core backward; every reduction in a pinned order

Parts, each a process of its own so that a fault in one ends the chain there (every GPU step under its own time limit):

  timeout -k 10 300 python tools/bench_refiner_grad.py --part accuracy &&
  timeout -k 10 300 python tools/bench_refiner_grad.py --part kernels &&
  timeout -k 10 300 python tools/bench_refiner_grad.py --part op &&
  timeout -k 10 600 python tools/bench_refiner_grad.py --part step &&
  timeout -k 10 300 python tools/bench_refiner_grad.py --part launches

  accuracy  all 18 parameter gradients of one forward + losses_refiner + backward at 2 x 1024 and 3 x 256 points: the worst
            error per tensor relative to max |float64 gradient| of the module composition on the same fp32 parameters
  kernels   the library calls of one backward alone (device events) at 20 x 1024 rows, beside torch's matmul / sum
  op        forward + backward of refiner(inp), both forms, at 20 x 1024 (the reference's bs 40 / 2 iterations) and 32 x 1024
  step      a stage-2 step at the same shapes: eval-mode Network forward, two refinement iterations of refiner +
            losses_refiner(chamfer="fused", objective="fused") + backward, then AutoClip + dcl.optim.Adam; the pose arithmetic
            between the iterations is ops.rigid_points and broadcast products (no torch.bmm), in every form
  launches  kernel launches of one forward + backward of each form by name (vendor GEMMs are the Cijk_* rows) and the
            peak memory above what was allocated before it
  trace     13 stage-2 steps (3 warm-up + 10) at 32 x 1024 with train_mlp="kernels" and the given --heads alone, nothing timed:
            the subject of a `rocprofv3 --kernel-trace --stats` run of its own per --heads value

Timing: bench_rotation_grad.compare -- a host clock around a block of calls ended by a device synchronise, blocks of at
least a quarter of a second, six blocks that alternate the two forms in both orders, in one process; reported are the
median of a form's three block means and their range.  profiles/refiner_grad.txt holds one run's output.

--heads modules|kernels: Refiner(train_heads=) of BOTH forms -- the two pose heads as the registered modules (default) or as one
autograd.PoseHeadsFn (csrc/pose_heads_grad.hip); profiles/train_heads.txt compares the two.
--wgrad fp32|split: Refiner(train_wgrad=) of the "kernels" form -- its weight gradients on csrc/linear_bwd.hip (default) or, on the
shapes of ops.WGRAD_SPLIT_SHAPES, on csrc/linear_wgrad_split.hip; --wgrad-all (measurement only) makes that table name every
shape for this process.  Part kernels times ops.linear_wgrad_split beside ops.linear_wgrad either way."""
import argparse
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from bench_chamfer import events_ms, peak_above_base, rand_rot  # noqa: E402
from bench_objective import launches  # noqa: E402
from bench_rotation_grad import MIN_BLOCK_S, compare  # noqa: E402

FORMS = ("kernels", "modules")
SHAPES = ((20, 1024), (32, 1024))
HEADS = "modules"                        # --heads
WGRAD = "fp32"                           # --wgrad


def line(what, res):
    (k, klo, khi), (m, mlo, mhi) = res["kernels"], res["modules"]
    verdict = "slower" if klo > mhi else "faster" if khi < mlo else "within the spread"
    print("  %-22s kernels %8.3f ms [%.3f .. %.3f]   modules %8.3f ms [%.3f .. %.3f]   kernels / modules %.3f  (%s)" %
          (what, k, klo, khi, m, mlo, mhi, k / m, verdict))


def make_refiner(dcl, form, rotation="device"):
    ref = dcl.refiner.Refiner(train_rotation=rotation, train_mlp=form, train_heads=HEADS,
                              train_wgrad=WGRAD if form == "kernels" else "fp32")
    ref.load_state_dict(dcl.synth.synth_state_dict(ref, 2))
    return ref.cuda().train()


def refiner_inputs(b, n, seed=4):
    g = torch.Generator().manual_seed(seed)
    x = torch.cat([torch.randn(b, 3, n, generator=g) * 0.05, torch.randn(b, 256, n, generator=g)], 1).cuda()
    conf = torch.rand(b, 2 * n, generator=g).cuda()
    labels = (torch.randn(b, 3, generator=g).cuda() * 0.01, rand_rot(g, b).cuda(), (torch.randn(b, 500, 3, generator=g) * 0.05).cuda(),
              (torch.arange(b) % 2).float().cuda(), {"rot_gt": rand_rot(g, b).cuda(), "trans_gt": (torch.randn(b, 3, generator=g) * 0.01).cuda()})
    return x, conf, labels


def part_accuracy(dcl, args):
    print("worst |grad - grad64| / max |grad64| over the 18 parameter tensors (float64: the module composition, host rotation)")
    cast = lambda v: v.double() if torch.is_tensor(v) else {k: w.double() for k, w in v.items()}     # noqa: E731
    for b, n in ((2, 1024), (3, 256)):
        x, conf, labels = refiner_inputs(b, n)
        conf = conf[:, :n] if n < 1024 else conf
        grads = {}
        for form in FORMS + ("float64",):
            ref = make_refiner(dcl, "modules" if form == "float64" else form, "host" if form == "float64" else "device")
            if form == "float64":
                out = ref.double()({"input_features": x.double(), "conf": conf.double(), "obj_idx": None})
                dcl.refiner.losses_refiner(None)(out, *[cast(v) for v in labels])["loss_all"].backward()
            else:
                out = ref({"input_features": x, "conf": conf, "obj_idx": None})
                dcl.refiner.losses_refiner(None)(out, *labels)["loss_all"].backward()
            grads[form] = {k: p.grad.double() for k, p in ref.named_parameters()}
        for form in FORMS:
            worst = max((float((g - grads["float64"][k]).abs().max()) / float(grads["float64"][k].abs().max()), k)
                        for k, g in grads[form].items())
            print("  %d x %-5d %-8s %.2e  (%s)" % (b, n, form, worst[0], worst[1]))


def part_kernels(dcl, args):
    b, n = 20, 1024
    M = b * n
    ops = dcl.ops
    print("library calls of one backward alone, %d rows (%d x %d), median of %d device-event timings; torch beside them" %
          (M, b, n, args.iters))
    print("  DCL_WGRAD_ROWS = %d -> %d splits" % (ops.WGRAD_ROWS, ops.linear_wgrad_splits(M)))
    g = torch.Generator().manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=g).cuda()                                               # noqa: E731
    for P, Q in ((1024, 512), (512, 512), (512, 256), (512, 3)):
        a, x = rnd(M, P), rnd(M, Q)
        t_own = events_ms(lambda: ops.linear_wgrad(a, x), args.iters, args.warmup)
        t_split = events_ms(lambda: ops.linear_wgrad_split(a, x), args.iters, args.warmup)
        t_lib = events_ms(lambda: torch.mm(a.t(), x), args.iters, args.warmup)
        print("  linear_wgrad  dW (%4d x %3d)   %7.1f us  %6.1f TFLOP/s     linear_wgrad_split %7.1f us  %6.1f TFLOP/s     "
              "torch.mm(a.t(), b) %7.1f us" % (P, Q, t_own * 1e3, 2.0 * M * P * Q / t_own / 1e9, t_split * 1e3,
                                               2.0 * M * P * Q / t_split / 1e9, t_lib * 1e3))
        del a, x
    for P in (1024, 512):
        h, gr = rnd(M, P), rnd(M, P)
        t_own = events_ms(lambda: ops.relu_bwd(h, gr, out=gr), args.iters, args.warmup)
        t_lib = events_ms(lambda: (torch.where(h > 0, gr, torch.zeros_like(gr)).sum(0)), args.iters, args.warmup)
        print("  relu_bwd      (%d x %4d) in place  %7.1f us  %6.2f TB/s       torch.where + sum  %7.1f us" %
              (M, P, t_own * 1e3, 12.0 * M * P / t_own / 1e9, t_lib * 1e3))
    h, w, gp = rnd(M, 1024), torch.rand(M, generator=g).cuda(), rnd(b, 1024)
    t_own = events_ms(lambda: ops.relu_bwd(h, roww=w, gpool=gp, rows_per_crop=n, out=h), args.iters, args.warmup)
    print("  relu_bwd      (%d x 1024) pooled form, in place  %7.1f us" % (M, t_own * 1e3))
    x, Wt, W = rnd(M, 512), rnd(512, 1024), rnd(1024, 512)
    dz, bias = rnd(M, 1024), rnd(1024)
    print("  linear_dma    h3 = relu(h2 Wt2 + b2) again        %7.1f us" %
          (events_ms(lambda: ops.linear_dma(x, Wt, bias, True), args.iters, args.warmup) * 1e3))
    print("  linear_dma    dH2 = dZ3 W2                         %7.1f us" %
          (events_ms(lambda: ops.linear_dma(dz, W), args.iters, args.warmup) * 1e3))


def op_step(ref, x, conf, G):
    inp = {"input_features": x, "conf": conf, "obj_idx": None}

    def step():
        for p in ref.parameters():
            p.grad = None
        out = ref(inp)
        (out["trans_pred"].sum() + (out["rot_pred"] * G).sum()).backward()
    return step


def part_op(dcl, args):
    print("forward + backward of refiner(inp) alone, train_rotation=\"device\" in both forms")
    for b, n in SHAPES:
        x, conf, _ = refiner_inputs(b, n)
        G = torch.randn(b, 3, 3, generator=torch.Generator().manual_seed(b)).cuda()
        steps = {form: op_step(make_refiner(dcl, form), x, conf, G) for form in FORMS}
        line("%d x %d" % (b, n), compare(steps, args.iters, args.warmup))


def stage2_step(dcl, net, data, form, iteration=2):
    ref = make_refiner(dcl, form)
    opt = dcl.optim.Adam(ref.parameters(), lr=1e-5)
    clip = dcl.optim.AutoClip(50, optimizer=opt)
    crit = dcl.refiner.losses_refiner(None, chamfer="fused", objective="fused")
    b = data["labels"]["rot_gt"].shape[0]
    sym = (torch.arange(b) % 2).float().cuda()
    gt = {k: data["labels"][k].cuda() for k in ("rot_gt", "trans_gt")}

    def step():
        # the body of the reference's Trainer.step (tools/train_YCBV_stage2.py:224-270) + clip + optimizer step
        with torch.no_grad():
            pred = net(data)
        rot_cur, trans_cur, conf, F = pred["rot_pred"], pred["trans_pred"], pred["conf"].detach(), pred["F_Xo_p"]
        pts, cld = data["labels"]["points_inp"], data["labels"]["points_tmp"]
        for p in ref.parameters():
            p.grad = None
        for _ in range(iteration):
            # (the loop's own pose arithmetic on ops.rigid_points and broadcast products: torch.bmm on (b, n, 3) x (b, 3, 3) and on
            #  3 x 3 matrices is three vendor GEMM launches per iteration, the only ones left once both switches are "kernels")
            cur = dcl.ops.rigid_points(pts.contiguous(), rot_cur.contiguous(), trans_cur.contiguous(), inverse=True)
            inp = torch.cat([cur.transpose(1, 2), F], dim=1).detach()
            out = ref({"input_features": inp, "conf": conf, "obj_idx": None})
            crit(out, trans_cur.detach(), rot_cur.detach(), cld, sym, gt)["loss_all"].backward()
            trans_cur = ((rot_cur * out["trans_pred"].unsqueeze(1)).sum(2) + trans_cur).detach()
            rot_cur = (rot_cur.unsqueeze(3) * out["rot_pred"].unsqueeze(1)).sum(2).detach()
        clip(ref)
        opt.step()
    return step


def part_step(dcl, args):
    print("stage-2 step: eval-mode Network forward, 2 x (refiner + losses_refiner fused + backward), AutoClip + dcl.optim.Adam")
    for b, n in SHAPES:
        net = dcl.DCL_Net.Network(dcl.synth.default_cfg(n, n), mode="test")
        net.load_state_dict(dcl.synth.synth_state_dict(net, 1))
        net = net.cuda().eval()
        data = dcl.synth.make_batch(b, n, n)
        steps = {form: stage2_step(dcl, net, data, form) for form in FORMS}
        line("%d x %d" % (b, n), compare(steps, args.step_iters, args.warmup))
        del net, steps


def part_launches(dcl, args):
    b, n = SHAPES[0]
    print("one forward + backward of refiner(inp) at %d x %d under torch's profiler (timings under it are not quoted)" % (b, n))
    x, conf, _ = refiner_inputs(b, n)
    G = torch.randn(b, 3, 3, generator=torch.Generator().manual_seed(b)).cuda()
    for form in FORMS:
        step = op_step(make_refiner(dcl, form), x, conf, G)
        step()
        peak = peak_above_base(step)
        rows = launches(step)
        total, vendor = sum(c for _, c in rows), sum(c for k, c in rows if k.startswith("Cijk_"))
        print("  %s: %d kernels, %d of them vendor GEMMs (Cijk_*); peak memory above the base %.0f MB" %
              (form, total, vendor, peak / 1e6))
        for k, c in rows:
            print("    %3d  %s" % (c, k[:150]))


def part_trace(dcl, args):
    b, n = SHAPES[1]
    net = dcl.DCL_Net.Network(dcl.synth.default_cfg(n, n), mode="test")
    net.load_state_dict(dcl.synth.synth_state_dict(net, 1))
    net = net.cuda().eval()
    step = stage2_step(dcl, net, dcl.synth.make_batch(b, n, n), "kernels")
    for _ in range(13):
        step()
    torch.cuda.synchronize()
    print("  13 stage-2 steps at %d x %d, train_mlp=\"kernels\", train_heads=\"%s\"" % (b, n, HEADS))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("accuracy", "kernels", "op", "step", "launches", "trace"), required=True)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--step-iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--heads", choices=("modules", "kernels"), default="modules")
    ap.add_argument("--wgrad", choices=("fp32", "split"), default="fp32")
    ap.add_argument("--wgrad-all", action="store_true")
    args = ap.parse_args()
    global HEADS, WGRAD
    HEADS, WGRAD = args.heads, args.wgrad
    if not torch.cuda.is_available():
        raise SystemExit("bench_refiner_grad: needs the GPU (no CPU timing is meaningful)")
    dcl = importlib.import_module("dcl-net_amd")
    if args.wgrad_all:
        class EveryShape(dict):
            def get(self, key, default=None):
                return 0
        dcl.ops.WGRAD_SPLIT_SHAPES = EveryShape()
    print("== refiner training, part %s: train_mlp=\"kernels\" (csrc/linear_bwd.hip + the own GEMM core) vs \"modules\" (torch); train_heads=\"%s\", train_wgrad=\"%s\"%s" % (args.part, args.heads, args.wgrad, " on every shape" if args.wgrad_all else ""))
    print("device: %s, torch %s; blocks of at least %d calls / %d steps and %.2f s, six alternating blocks after %d warm-up rounds" %
          (torch.cuda.get_device_name(0), torch.__version__, args.iters, args.step_iters, MIN_BLOCK_S, args.warmup))
    {"accuracy": part_accuracy, "kernels": part_kernels, "op": part_op, "step": part_step, "launches": part_launches, "trace": part_trace}[args.part](dcl, args)


if __name__ == "__main__":
    main()
