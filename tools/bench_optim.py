"""The tail of a training step -- what follows loss.backward() -- on Network's 156 parameter tensors (8 393 972 fp32 elements)
and on the refiner's 18, with synthetic gradients:

  item+default  the reference's form (tools/train_YCBV_stage1.py:119-125, 212-231): a norm kernel and a blocking .item() per
                parameter tensor, np.percentile over the history, clip_grad_norm_, torch.optim.Adam with its default
                implementation
  item+fused    the same with torch.optim.Adam(fused=True)
  dcl           dcl.optim.AutoClip(50, optimizer=opt) + dcl.optim.Adam.step(): one norm pass, one read-back, one update launch

  python tools/bench_optim.py [--iters 50] [--warmup 5]

Per model: median ms of one device-synchronised tail (host clock), in blocks that rotate the three forms inside one process,
every form on its own copy of the parameters with the same gradients.  Then the two library calls alone (device events)
against the bytes they must move (4 B per element the norm, 28 B the update) as a fraction of the 6.3 TB/s copy rate; the
update's 235 MB of Network fit the 256 MiB Infinity Cache, so that fraction is of a rate, not proof of HBM traffic.
profiles/optim.txt holds one run's output."""
import argparse
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

COPY_RATE = 6.3e12            # bytes/s: the measured device-to-device copy rate the byte counts are held against
SHIPPED = dict(lr=1e-3, betas=(0.5, 0.999), eps=1e-6)
REPS = 20                     # library calls per timed window


class ItemAutoClip(object):
    """AutoClip in the form the reference's training scripts run it: every gradient's norm read back on its own, the clip
    value a percentile of the history, then torch's clip_grad_norm_ (which measures everything once more)"""

    def __init__(self, percentile):
        self.percentile, self.history = percentile, []

    def __call__(self, model):
        total = 0.0
        for p in model.parameters():
            if p.grad is not None:
                total += p.grad.detach().norm(2).item() ** 2
        self.history.append(total ** 0.5)
        torch.nn.utils.clip_grad_norm_(model.parameters(), np.percentile(self.history, self.percentile))


class _Params(torch.nn.Module):
    """a model's parameter tensors, copied, with fixed synthetic gradients"""

    def __init__(self, model, seed=0):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(p.detach().clone()) for p in model.parameters()])
        self.grads = [(torch.randn(p.shape, generator=g) * 1e-3).to(p.device) for p in self.ps]

    def fill(self):
        for p, g in zip(self.ps, self.grads):
            p.grad = g.clone()           # clip_grad_norm_ rewrites gradients in place: every tail starts from the same ones


def median_ms(step, iters):
    ts = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        step()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


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


def bench(dcl, name, model, iters, warmup):
    forms, setups = {}, {}
    for tag in ("item+default", "item+fused", "dcl"):
        m = _Params(model)
        if tag == "dcl":
            opt = dcl.optim.Adam(m.parameters(), **SHIPPED)
            clip = dcl.optim.AutoClip(50, optimizer=opt)
        else:
            opt = torch.optim.Adam(m.parameters(), fused=(tag == "item+fused") or None, **SHIPPED)
            clip = ItemAutoClip(50)
        setups[tag] = (m, opt, clip)

        def tail(m=m, opt=opt, clip=clip):
            clip(m)
            opt.step()
        forms[tag] = tail
    n_el = sum(p.numel() for p in setups["dcl"][0].ps)
    print("\n%s: %d parameter tensors, %d elements" % (name, len(setups["dcl"][0].ps), n_el))

    def timed(tag):
        m = setups[tag][0]
        ts = []
        for _ in range(iters):
            m.fill()
            ts.append(median_ms(forms[tag], 1))
        ts.sort()
        return ts[len(ts) // 2]
    for tag in forms:
        for _ in range(warmup):
            setups[tag][0].fill()
            forms[tag]()
    tags = list(forms)
    blocks = []
    for r in range(3):
        for tag in tags[r:] + tags[:r]:
            blocks.append((tag, timed(tag)))
    print("  blocks in run order (median ms of one tail): " + ", ".join("%s %.3f" % bl for bl in blocks))
    mid = {}
    for tag in tags:
        v = sorted(t for k, t in blocks if k == tag)
        mid[tag] = v[len(v) // 2]
        print("  %-13s %.3f ms (blocks %s)" % (tag, mid[tag], " ".join("%.3f" % t for t in v)))
    best = min(mid["item+default"], mid["item+fused"])
    print("  dcl / faster reference form = %.3f  (%.1fx)" % (mid["dcl"] / best, best / mid["dcl"]))
    # the two library calls alone: REPS calls behind one another between two events, so that the GPU and not the host's
    # enqueue (an allocation or two and a ctypes call: ~25 us, longer than the norm pass itself) is what is timed
    m, opt, _ = setups["dcl"]
    m.fill()
    plan = opt._prepare()
    table, chunk_tensor, chunk_begin = plan.layout.views(plan.slot.dev)
    _, beta1, beta2, eps = plan.hyper[0]
    N, L = dcl._native, dcl._native.lib()
    nt, nc = plan.layout.n_tensors, plan.layout.n_chunks
    partials, sq, norm = (torch.empty(k, dtype=torch.float64, device=table.device) for k in (nc, nt, 1))
    f = N.C.c_float

    def norm_calls():
        for _ in range(REPS):
            N.check(L.dcl_grad_sqnorm(nt, N.ptr(table), nc, N.ptr(chunk_tensor), N.ptr(chunk_begin), N.ptr(partials), N.ptr(sq),
                                      N.ptr(norm), N.stream()))

    def adam_calls():
        for _ in range(REPS):
            N.check(L.dcl_adam_step(nt, N.ptr(table), nc, N.ptr(chunk_tensor), N.ptr(chunk_begin), f(1.0), f(beta1), f(beta2),
                                    f(eps), N.stream()))
    t_norm = events_ms(norm_calls, iters, warmup) / REPS
    t_adam = events_ms(adam_calls, iters, warmup) / REPS
    for what, t, nbytes in (("dcl_grad_sqnorm (both launches)", t_norm, 4 * n_el), ("dcl_adam_step", t_adam, 28 * n_el)):
        print("  %-32s %.4f ms for %.1f MB: %.2f TB/s, %.0f %% of the 6.3 TB/s copy rate"
              % (what, t, nbytes / 1e6, nbytes / (t * 1e-3) / 1e12, 100 * nbytes / (t * 1e-3) / COPY_RATE))
    print("  both                             %.4f ms for %.1f MB: %.0f %% of the 6.3 TB/s copy rate"
          % (t_norm + t_adam, 32 * n_el / 1e6, 100 * 32 * n_el / ((t_norm + t_adam) * 1e-3) / COPY_RATE))
    return mid


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim: needs the GPU (no CPU timing is meaningful)")
    dcl = importlib.import_module("dcl-net_amd")
    print("AutoClip + Adam after loss.backward(): the reference's form (per-tensor .item()) vs dcl.optim (csrc/optim.hip)")
    net = dcl.DCL_Net.Network(dcl.synth.default_cfg(1024, 1024), mode="train").cuda()
    mids = [bench(dcl, "Network", net, args.iters, args.warmup)]
    mids.append(bench(dcl, "Refiner", dcl.refiner.Refiner().cuda(), args.iters, args.warmup))
    for mid in mids:
        if mid["dcl"] > min(mid["item+default"], mid["item+fused"]):
            raise SystemExit("bench_optim: dcl.optim is SLOWER than the reference's form: a defect, not a result")


if __name__ == "__main__":
    main()
