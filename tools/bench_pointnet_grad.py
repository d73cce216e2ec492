"""pointnet_lib gradients at bench.py's primitive shape (B=32, C=64, N=12288, npoint=2048 FPS centres, nsample=64, ball
query r=0.03): time of the backward calls against their forwards measured in the same process, with the bytes each call
must move, the rate, the fraction of the 8 TB/s HBM peak and the backward / forward ratio.

  python tools/bench_pointnet_grad.py [--iters 20] [--warmup 5]

`bwd` is the C-ABI call (inverse index + ordered gather) adding into a preallocated grad_points; `bwd+zero` adds the
zero-fill that the autograd Functions do first.  Targets (issue estimate from byte counts): group_points backward <= 1.5x
its forward, three_interpolate backward <= its forward; gather_points is reported only."""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

PEAK = 8.0e12


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) for a, b in ev)
    return t[len(t) // 2]                                        # median, ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    dcl = importlib.import_module("dcl-net_amd")
    B, N, NP, NS, C, r = 32, 12288, 2048, 64, 64, 0.03
    data = dcl.synth.make_batch(B, N, 64)
    xyz = data["inp"]["feats"][:, 4:7].reshape(B, N, 3).contiguous().cuda()
    fps = dcl.ops.furthest_point_sampling(xyz, NP)
    new_xyz = torch.gather(xyz, 1, fps.long().unsqueeze(-1).expand(-1, -1, 3)).contiguous()
    idx = dcl.ops.ball_query(r, NS, xyz, new_xyz)
    d2, i3 = dcl.ops.three_nn(xyz, new_xyz)
    w = 1.0 / (torch.sqrt(d2) + 1e-8)
    w = (w / w.sum(2, keepdim=True)).contiguous()
    g = torch.Generator(device="cuda").manual_seed(0)
    feats = torch.randn(B, C, N, device="cuda", generator=g)
    go = torch.randn(B, C, NP, NS, device="cuda", generator=g)
    gp = torch.zeros(B, C, N, device="cuda")
    f_small = torch.randn(B, C, NP, device="cuda", generator=g)
    gi = torch.randn(B, C, N, device="cuda", generator=g)
    gp_small = torch.zeros(B, C, NP, device="cuda")
    gidx = fps
    gg = torch.randn(B, C, NP, device="cuda", generator=g)
    F = 4
    rows = []

    def row(name, ms, nbytes, fwd_ms=None):
        d = dict(op=name, ms=round(ms, 4), GB=round(nbytes / 1e9, 4), GBps=round(nbytes / (ms * 1e-3) / 1e9, 1),
                 frac_8TBps=round(nbytes / (ms * 1e-3) / PEAK, 3))
        if fwd_ms is not None:
            d["bwd_over_fwd"] = round(ms / fwd_ms, 3)
        rows.append(d)
        print("%-34s %9.4f ms %8.3f GB %8.1f GB/s %6.3f of 8 TB/s%s" % (
            name, ms, d["GB"], d["GBps"], d["frac_8TBps"], "  bwd/fwd %.3f" % d["bwd_over_fwd"] if fwd_ms else ""))

    # group_points
    t_gf = timed(lambda: dcl.ops.group_points(feats, idx), args.iters, args.warmup)
    row("group_points fwd", t_gf, F * (B * C * NP * NS + B * NP * NS + B * C * N))
    t_gb = timed(lambda: dcl.ops.group_points_grad(go, idx, N, grad_points=gp), args.iters, args.warmup)
    row("group_points bwd", t_gb, F * (B * C * NP * NS + B * NP * NS + 2 * B * C * N), t_gf)
    t_gz = timed(lambda: dcl.ops.group_points_grad(go, idx, N), args.iters, args.warmup)
    row("group_points bwd+zero", t_gz, F * (B * C * NP * NS + B * NP * NS + 3 * B * C * N), t_gf)
    # three_interpolate: (32,64,2048) -> (32,64,12288) forward, the reverse backward
    t_if = timed(lambda: dcl.ops.three_interpolate(f_small, i3, w), args.iters, args.warmup)
    row("three_interpolate fwd", t_if, F * (B * C * N + B * C * NP + 2 * B * N * 3))
    t_ib = timed(lambda: dcl.ops.three_interpolate_grad(gi, i3, w, NP, grad_points=gp_small), args.iters, args.warmup)
    row("three_interpolate bwd", t_ib, F * (B * C * N + 2 * B * N * 3 + 2 * B * C * NP), t_if)
    t_iz = timed(lambda: dcl.ops.three_interpolate_grad(gi, i3, w, NP), args.iters, args.warmup)
    row("three_interpolate bwd+zero", t_iz, F * (B * C * N + 2 * B * N * 3 + 3 * B * C * NP), t_if)
    # gather_points (report only)
    t_af = timed(lambda: dcl.ops.gather_points(feats, gidx), args.iters, args.warmup)
    row("gather_points fwd", t_af, F * (B * C * NP + B * NP + B * C * N))
    t_ab = timed(lambda: dcl.ops.gather_points_grad(gg, gidx, N, grad_points=gp), args.iters, args.warmup)
    row("gather_points bwd", t_ab, F * (B * C * NP + B * NP + 2 * B * C * N), t_af)
    print("targets: group_points bwd/fwd %.3f (<= 1.5), three_interpolate bwd/fwd %.3f (<= 1.0)" % (t_gb / t_gf, t_ib / t_if))
    print(json.dumps(dict(shape=dict(B=B, C=C, N=N, npoint=NP, nsample=NS, radius=r), rows=rows)))


if __name__ == "__main__":
    main()
