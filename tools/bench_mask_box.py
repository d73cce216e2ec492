"""The loaders' get_bbox(mask_to_bbox(mask)) for a mask that is already in HBM, in its two forms:

  device   ops.mask_box (csrc/mask_box.hip): six launches, the box row stays on the device
  host     the only alternative that exists: download the mask, run the host twin (dcl_mask_box_host), upload the box row

timed alone and inside CropBuilder.build_lmo (build_lm(obj_bb=None) with / without a given box, the box then made the host way),
on three masks of 480 x 640: an occluded scene mask (tests/lmo_scene.py), a Bernoulli 0.41 mask and the checkerboard (the most
runs a mask can have).  No speed-up is assumed: what comes out is recorded, also where the device form is slower.

  timeout -k 10 600 python tools/bench_mask_box.py

Timing: a host clock around a block of calls ended by a device synchronise, at least `iters` of them and at least a quarter
of a second's worth, in six blocks that alternate the two forms in both orders, in one process; reported are the median of a
form's three block means and their range.  profiles/mask_box.txt holds one run's output."""
import argparse
import importlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

MIN_BLOCK_S = 0.25          # a timed block lasts at least this long: shorter windows time the clock and the scheduler


def block_ms(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def compare(forms, iters, warmup):
    """{name: fn} for two forms -> {name: (median of its three block means, lowest, highest)}; both forms run the same
    number of calls per block, at least `iters` and enough for the slower one to fill MIN_BLOCK_S"""
    a, c = list(forms)
    for _ in range(warmup):
        for fn in forms.values():
            fn()
    slowest = max(block_ms(fn, iters) for fn in forms.values())
    iters = max(iters, int(MIN_BLOCK_S * 1e3 / slowest) + 1)
    blocks = [(name, block_ms(forms[name], iters)) for order in ((a, c, a), (c, a, c)) for name in order]
    out = {}
    for n in forms:
        v = sorted(t for k, t in blocks if k == n)
        out[n] = (v[len(v) // 2], v[0], v[-1])
    return out


def line(what, res):
    (d, dlo, dhi), (h, hlo, hhi) = res["device"], res["host"]
    verdict = "slower" if dlo > hhi else "faster" if dhi < hlo else "within the spread"
    print("  %-34s device %8.4f ms [%.4f .. %.4f]   host %8.4f ms [%.4f .. %.4f]   device / host %.2f  (%s)" %
          (what, d, dlo, dhi, h, hlo, hhi, d / h, verdict))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mask_box: needs the GPU (no CPU timing is meaningful)")
    dcl = importlib.import_module("dcl-net_amd")
    import mask_cases as MC
    from lmo_scene import CASES, CFG, make_lmo_scene
    print("== mask -> box: device (csrc/mask_box.hip) vs host (download the mask, host twin, upload the box row)")
    print("device: %s, torch %s; blocks of at least %d calls and %.2f s, six alternating blocks after %d warm-up rounds" %
          (torch.cuda.get_device_name(0), torch.__version__, args.iters, MIN_BLOCK_S, args.warmup))
    seed, kw = CASES[0]
    sc = make_lmo_scene(seed, tmp_size=CFG["tmp_size"], **kw)
    named = dict(MC.mask_cases(480, 640))
    masks = [("occluded scene mask", sc["mask_label"]), ("Bernoulli 0.41", named["bernoulli 0.41 seed 1"]),
             ("checkerboard", named["checkerboard"])]
    print("the call alone (mask resident as int32; the result is the (1, 4) box row on the device)")
    for name, m in masks:
        dev = torch.from_numpy(np.ascontiguousarray(m.astype(np.int32))).cuda()
        want = dcl.ops.mask_box_host(m, 1, 0)
        assert np.array_equal(dcl.ops.mask_box(dev, 1, 0).cpu().numpy(), want), name

        def device(dev=dev):
            return dcl.ops.mask_box(dev, 1, 0)[:, 4:8].contiguous()

        def host(dev=dev):
            box = dcl.ops.mask_box_host(dev.cpu().numpy(), 1, 0)[:, 4:8]
            return torch.from_numpy(np.ascontiguousarray(box)).cuda()
        line("%s (%d components)" % (name, int(want[0, 8])), compare({"device": device, "host": host}, args.iters, args.warmup))
    print("inside the sample builder (frame as numpy arrays, as the loader reads them; CropBuilder.build_lm in eval mode with")
    print("obj_bb=None = what build_lmo runs, against the same call with the box made the host way from the uploaded mask)")
    builder = dcl.crops.CropBuilder(CFG, sc["cad_pts"], sc["cad_col"], camera=dcl.crops.LM_CAMERA)
    for name, m in masks:
        def device(m=m):
            np.random.seed(1)
            return builder.build_lm(sc["img"], sc["depth"], m, None, sc["cls"], eval_mode=True)

        def host(m=m):
            np.random.seed(1)
            dev = torch.from_numpy(np.ascontiguousarray(m).astype(np.int32)).cuda()     # the mask is on the device: bring it back
            box = dcl.ops.mask_box_host(dev.cpu().numpy(), 1, 0)[0, :4].tolist()
            return builder.build_lm(sc["img"], sc["depth"], m, box, sc["cls"], eval_mode=True)
        a, b = device(), host()
        assert (a is None) == (b is None) and (a is None or all(torch.equal(x, y) for x, y in zip(a, b))), name
        line(name, compare({"device": device, "host": host}, max(args.iters // 5, 5), args.warmup))


if __name__ == "__main__":
    main()
