"""The tail of a training step -- what follows loss.backward() -- on Network's 156 parameter tensors (8 393 972 fp32 elements)
and on the refiner's 18, with synthetic gradients:

  item+default  the reference's form (tools/train_YCBV_stage1.py:119-125, 212-231): a norm kernel and a blocking .item() per
                parameter tensor, np.percentile over the history, clip_grad_norm_, torch.optim.Adam with its default
                implementation
  item+fused    the same with torch.optim.Adam(fused=True)
  dcl           dcl.optim.AutoClip(50, optimizer=opt) + dcl.optim.Adam.step(): one norm pass, one read-back, one update launch

  python tools/bench_optim.py [--iters 50] [--warmup 5] [--part all|forms|history]

Per model: median ms of one device-synchronised tail (host clock), in blocks that rotate the three forms inside one process,
every form on its own copy of the parameters with the same gradients.  Then the two library calls alone (device events)
against the bytes they must move (4 B per element the norm, 28 B the update) as a fraction of the 6.3 TB/s copy rate; the
update's 235 MB of Network fit the 256 MiB Infinity Cache, so that fraction is of a rate, not proof of HBM traffic.
profiles/optim.txt holds one run's output.

--part history: the dcl tail again on Network's tensors with a norm history ALREADY HELD, as late in a run (the reference's
schedule ends at 631 050 steps): dcl.optim.AutoClip (np.percentile over a Python list, one read-back) against
dcl.optim.DeviceAutoClip (the sorted history and the percentile on the GPU, no read-back), histories of HISTORY_LENGTHS entries
preloaded through load_state_dict and loaded again in front of every block, the two forms alternating block by block, a
block at least BLOCK_SECONDS of single synchronised tails; then the two observe launches alone (device events) against
the 16 n bytes they move.  profiles/autoclip_device.txt holds one run's output."""
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
HISTORY_LENGTHS = (0, 10000, 100000, 631050)      # 631 050 = 210 epochs x 3005 iterations, the reference's schedule
BLOCK_SECONDS = 0.3


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


def bench_history(dcl, model, warmup, rounds=3):
    """the dcl tail with a history already held: AutoClip ("host") against DeviceAutoClip ("device"), see the module docstring"""
    setups = {}
    for tag in ("host", "device"):
        m = _Params(model)
        opt = dcl.optim.Adam(m.parameters(), **SHIPPED)
        clip = (dcl.optim.DeviceAutoClip if tag == "device" else dcl.optim.AutoClip)(50, optimizer=opt)
        setups[tag] = (m, opt, clip)
    print("\nNetwork with a held history: %d parameter tensors; dcl.optim.AutoClip (host) vs dcl.optim.DeviceAutoClip (device)"
          % len(setups["host"][0].ps))
    print("  per block: the history is loaded again, then single synchronised tails for >= %.1f s; median ms of one tail"
          % BLOCK_SECONDS)
    rng = np.random.default_rng(0)

    def block(tag, sd):
        m, opt, clip = setups[tag]
        clip.load_state_dict(sd)
        ts, t_end = [], time.perf_counter() + BLOCK_SECONDS
        while len(ts) < 20 or (time.perf_counter() < t_end and len(ts) < 2000):
            m.fill()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            clip(m)
            opt.step()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        ts.sort()
        return ts[len(ts) // 2], len(ts)
    table = []
    for n in HISTORY_LENGTHS:
        sd = {"percentile": 50, "history": rng.lognormal(0.0, 1.0, n).tolist()}
        for tag in setups:                                            # warm-up at this length: growth, the staging ring
            m, opt, clip = setups[tag]
            clip.load_state_dict(sd)
            for _ in range(warmup):
                m.fill()
                clip(m)
                opt.step()
        torch.cuda.synchronize()
        blocks = []
        for r in range(rounds):
            for tag in (("host", "device") if r % 2 == 0 else ("device", "host")):
                blocks.append((tag,) + block(tag, sd))
        print("  history %7d, blocks in run order: %s" % (n, ", ".join("%s %.3f (%d tails)" % bl for bl in blocks)))
        row = {}
        for tag in setups:
            v = sorted(t for k, t, _ in blocks if k == tag)
            row[tag] = (v[len(v) // 2], v[0], v[-1])
            print("    %-6s %8.3f ms  (blocks %.3f .. %.3f)" % ((tag,) + row[tag]))
        h, d = row["host"], row["device"]
        verdict = "device faster, block ranges disjoint" if d[2] < h[1] else \
                  "host faster, block ranges disjoint" if h[2] < d[1] else "block ranges overlap: a tie"
        print("    host / device = %.2f  (%s)" % (h[0] / d[0], verdict))
        table.append((n, row))
    # the two observe launches alone, at a fixed n (the same source and destination every call)
    dev = torch.device("cuda")
    ops = dcl.ops
    for n in HISTORY_LENGTHS:
        src = torch.from_numpy(np.sort(rng.lognormal(0.0, 1.0, n))).to(dev)
        dst, arrival = (torch.empty(n + 1, dtype=torch.float64, device=dev) for _ in range(2))
        norm = torch.ones(1, dtype=torch.float64, device=dev)
        out = torch.zeros(ops.AUTOCLIP_OUT_DOUBLES, dtype=torch.float64, device=dev)

        def calls():
            for _ in range(REPS):
                ops.autoclip_observe(n, src, dst, arrival, norm, 50, out)
        t = events_ms(calls, 30, warmup) / REPS
        nbytes = 16 * n
        print("  dcl_autoclip_observe (both launches), n = %7d: %.4f ms for %.3f MB: %.3f TB/s, %.1f %% of the 6.3 TB/s copy rate"
              % (n, t, nbytes / 1e6, nbytes / (t * 1e-3) / 1e12, 100 * nbytes / (t * 1e-3) / COPY_RATE))
    return table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--part", choices=("all", "forms", "history"), default="all")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim: needs the GPU (no CPU timing is meaningful)")
    dcl = importlib.import_module("dcl-net_amd")
    print("AutoClip + Adam after loss.backward(): the reference's form (per-tensor .item()) vs dcl.optim (csrc/optim.hip)")
    net = dcl.DCL_Net.Network(dcl.synth.default_cfg(1024, 1024), mode="train").cuda()
    mids = []
    if args.part in ("all", "forms"):
        mids.append(bench(dcl, "Network", net, args.iters, args.warmup))
        mids.append(bench(dcl, "Refiner", dcl.refiner.Refiner().cuda(), args.iters, args.warmup))
    if args.part in ("all", "history"):
        bench_history(dcl, net, args.warmup)
    for mid in mids:
        if mid["dcl"] > min(mid["item+default"], mid["item+fused"]):
            raise SystemExit("bench_optim: dcl.optim is SLOWER than the reference's form: a defect, not a result")


if __name__ == "__main__":
    main()
