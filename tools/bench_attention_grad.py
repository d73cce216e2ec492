"""Forward + backward of ONE direction of the correspondence attention: autograd.CrossAttentionFn (dcl_cross_attention +
csrc/attention_bwd.hip, no attention map) against the materialised composition the module path trains with by default
(softmax(bmm) + two bmm, torch autograd, fp32), same inputs, at the reference training shape 32 x 1024 x 1024 and at
4 crops of the stress shape, 4 x 12288 x 2048.

  python tools/bench_attention_grad.py [--iters 20] [--warmup 3]

Per shape: median ms of a device-synchronised forward + backward over `iters` repetitions, in blocks that alternate the two
forms in both orders (fused / materialised / fused, then materialised / fused / materialised) inside one process; the
peak of torch.cuda.max_memory_allocated above what was allocated before the step, for each form; and the backward call
alone (ops.cross_attention_backward, device events) as fp32 TFLOP/s against the 157.3 TFLOP/s fp32 MFMA peak, counting
2 nq nk (2*64 + 2*320 + 320 + 64 + 64) flop per crop: S and dP twice (once per sweep), dV, dK, dQ once -- the stats pass's
own S is work the count leaves out, so the rate is what a user gets, not what the matrix pipe issues.
profiles/attention_grad.txt holds one run's output."""
import argparse
import importlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

PEAK_FP32_MFMA = 157.3e12
SHAPES = [(32, 1024, 1024), (4, 12288, 2048)]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    assert args.iters >= 20, "at least 20 timed repetitions per block"
    if not torch.cuda.is_available():
        raise SystemExit("bench_attention_grad: needs the GPU (no CPU timing is meaningful)")
    dcl = importlib.import_module("dcl-net_amd")
    Fn = dcl.autograd.CrossAttentionFn
    print("attention forward + backward, one direction: fused (CrossAttentionFn) vs materialised (softmax(bmm) + 2 bmm, autograd)")
    print("device: %s, torch %s, %d timed repetitions per block after %d warm-up steps" %
          (torch.cuda.get_device_name(0), torch.__version__, args.iters, args.warmup))
    for b, nq, nk in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(nq + nk)
        Q, K = torch.randn(b, nq, 64, device="cuda", generator=g), torch.randn(b, nk, 64, device="cuda", generator=g)
        V1, V2 = torch.randn(b, nk, 256, device="cuda", generator=g), torch.randn(b, nk, 64, device="cuda", generator=g)
        dO1, dO2 = torch.randn(b, nq, 256, device="cuda", generator=g), torch.randn(b, nq, 64, device="cuda", generator=g)
        dO1t, dO2t = dO1.transpose(1, 2).contiguous(), dO2.transpose(1, 2).contiguous()
        leaves = [t.requires_grad_(True) for t in (Q, K, V1, V2)]

        def clear():
            for t in leaves:
                t.grad = None

        def fused():
            clear()
            o1, o2 = Fn.apply(*leaves)
            torch.autograd.backward([o1, o2], [dO1, dO2])

        def materialised():
            clear()
            q, k, v1, v2 = leaves
            A = torch.softmax(torch.bmm(k, q.transpose(1, 2)), dim=1)
            torch.autograd.backward([torch.bmm(v1.transpose(1, 2), A), torch.bmm(v2.transpose(1, 2), A)], [dO1t, dO2t])

        for _ in range(args.warmup):
            fused()
            materialised()
        forms = {"fused": fused, "materialised": materialised}
        blocks = []
        for order in (("fused", "materialised", "fused"), ("materialised", "fused", "materialised")):
            for name in order:
                blocks.append((name, median_ms(forms[name], args.iters)))
        mem = {name: peak_above_base(fn) for name, fn in forms.items()}

        # the backward call alone, device events
        with torch.no_grad():
            O1, O2 = torch.empty(b * nq, 256, device="cuda"), torch.empty(b * nq, 64, device="cuda")
            flat = [t.detach().reshape(-1, t.shape[2]) for t in (Q, K, V1, V2)]
            dcl.ops.cross_attention(b, flat[0], flat[1], flat[2], O1, flat[3], O2)
            bwd = lambda: dcl.ops.cross_attention_backward(b, *flat, O1, O2, dO1.reshape(-1, 256), dO2.reshape(-1, 64))  # noqa: E731
            for _ in range(args.warmup):
                bwd()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.iters)]
            for a, z in ev:
                a.record()
                bwd()
                z.record()
            torch.cuda.synchronize()
            t_bwd = sorted(a.elapsed_time(z) for a, z in ev)[len(ev) // 2]
        flop = 2.0 * b * nq * nk * (2 * 64 + 2 * 320 + 320 + 64 + 64)

        one_map = b * nq * nk * 4
        print("\nshape b x nq x nk = %d x %d x %d   (one attention map: %.1f MiB)" % (b, nq, nk, one_map / 2 ** 20))
        print("  blocks in run order (median ms of forward + backward): " + ", ".join("%s %.3f" % bl for bl in blocks))
        med = {n: sorted(t for m, t in blocks if m == n) for n in forms}
        mid = {n: v[len(v) // 2] for n, v in med.items()}
        print("  fused        %.3f ms (blocks %s)" % (mid["fused"], " ".join("%.3f" % t for t in med["fused"])))
        print("  materialised %.3f ms (blocks %s)" % (mid["materialised"], " ".join("%.3f" % t for t in med["materialised"])))
        print("  fused / materialised time = %.3f" % (mid["fused"] / mid["materialised"]))
        print("  peak memory above the inputs: fused %.1f MiB (%.2f maps), materialised %.1f MiB (%.2f maps)" %
              (mem["fused"] / 2 ** 20, mem["fused"] / one_map, mem["materialised"] / 2 ** 20, mem["materialised"] / one_map))
        print("  backward call alone (3 launches): %.3f ms, %.1f GFLOP counted -> %.1f TFLOP/s = %.1f %% of the fp32 MFMA peak"
              % (t_bwd, flop / 1e9, flop / t_bwd / 1e9, 100.0 * flop / (t_bwd * 1e-3) / PEAK_FP32_MFMA))
        del leaves, Q, K, V1, V2, dO1, dO2, dO1t, dO2t, O1, O2, flat
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
