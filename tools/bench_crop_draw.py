#!/usr/bin/env python3
"""The crop builder with the loader's host draws (draws="host": one read-back of the point counts per frame) and with the draws on
the device (draws="device": none), both forms alternating in ONE process on the same frames, network and weights.

  tools/bench_crop_draw.py [--blocks 5] [--images 40]

Workloads: bench.py's eval-stream frames -- synth.make_frame(500 + i): 6 objects per 480 x 640 frame at 6 mm voxels (YCB-V) and one
object per frame at 5 mm (LineMOD) -- N = M = 1024, frames resident, capacity-form crops (capacity=True), default routing (graph
replay).  Per workload, `blocks` blocks; in each, first the host form, then the device form:
  builder    ms per frame of CropBuilder.build alone, timed from the first call to a device synchronisation behind the last
  serial     build -> forward -> ADD-S, one frame after the other on one stream
  pipelined  frame k+1 is built on a second stream while frame k's forward runs
  prefetch   crops.CropPrefetcher: a builder thread two frames ahead
The distances stay on the device until a stream ends; the tabulation reads `valid` and the distances in ONE read-back.  Reported:
the median block with the range over the blocks.  A difference is CLAIMED only where the two ranges are disjoint.
Also: the device time of k_crop_draw alone (HIP events) for 6 instances and for one instance of m = 2 000 / 30 000 / 300 000 points."""
import argparse
import importlib
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--images", type=int, default=40)
    args = ap.parse_args()
    if args.blocks < 3:
        ap.error("--blocks: at least 3 (a median with a range)")
    import numpy as np
    import torch
    dcl = importlib.import_module("dcl-net_amd")
    dev = torch.device("cuda:0")
    images = args.images
    bstream = torch.cuda.Stream(dev)
    main_s = torch.cuda.current_stream(dev)

    def fmt(v):
        return "%7.3f [%7.3f .. %7.3f]" % (statistics.median(v), min(v), max(v))

    print("ms per frame: median of %d blocks of %d frames [min .. max]; forms alternate block by block in one process" % (args.blocks, images))
    for tag, unit, n_o in (("ycbv", 0.006, 6), ("linemod", 0.005, 1)):
        cfg_b = dict(input_size=1024, tmp_size=1024, unit_voxel_extent=[unit] * 3, voxel_num_limit=[64] * 3, voxelization_mode=4)
        frames = [dcl.synth.make_frame(500 + i, n_obj=n_o, tmp_size=1024) for i in range(4)]
        res = [dcl.crops.CropBuilder.resident(f["img"], f["depth"], f["label"], dev) for f in frames]
        builders = {form: dcl.crops.CropBuilder(cfg_b, frames[0]["cad_pts"], frames[0]["cad_col"], device=dev, capacity=True, draws=form)
                    for form in ("host", "device")}
        net = dcl.DCL_Net.Network(dcl.synth.default_cfg(1024, 1024, unit=unit), mode="test")
        net.load_state_dict(dcl.synth.synth_state_dict(net, 1))
        net = net.to(dev).eval()
        sym = torch.tensor([0, 1] * 16, dtype=torch.int32, device=dev)

        def build(form, i):
            f, (im, de, la) = frames[i % 4], res[i % 4]
            return builders[form].build(im, de, la, f["rois"], f["gt_obj"], poses=f["poses"])

        def build_ahead(form, i):
            with torch.cuda.stream(bstream):
                d = build(form, i)

            def mark(v):
                if torch.is_tensor(v):
                    if v.is_cuda:
                        v.record_stream(main_s)
                elif isinstance(v, dict):
                    for x in v.values():
                        mark(x)
            mark(d)
            return d

        def metric(d, p):
            b = p["rot_pred"].shape[0]
            cld = d["tmp"]["feats"][:, 4:7].reshape(b, 1024, 3)
            if tag == "linemod":
                return dcl.sharding.add_lm(cld, p["rot_pred"], p["trans_pred"], d["labels"]["rot_gt"], d["labels"]["trans_gt"], sym[:b])
            return dcl.sharding.add_s(cld, p["rot_pred"], p["trans_pred"], d["labels"]["rot_gt"], d["labels"]["trans_gt"])

        def step(d, acc):
            p = net(d)
            b = p["rot_pred"].shape[0]
            valid = d["valid"].float() if "valid" in d else torch.ones(b, device=dev)
            acc.append(torch.stack([metric(d, p), valid, d["inp"]["vi_info"][2:3].float().expand(b)]))

        def stream(form, sched):
            acc = []
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if sched == "builder":
                for i in range(images):
                    d = build(form, i)
            elif sched == "serial":
                for i in range(images):
                    step(build(form, i), acc)
            elif sched == "pipelined":
                d = build_ahead(form, 0)
                for i in range(images):
                    main_s.wait_event(d["ready_event"])
                    step(d, acc)
                    if i + 1 < images:
                        d = build_ahead(form, i + 1)
            else:
                feed_args = ((res[i % 4][0], res[i % 4][1], res[i % 4][2], frames[i % 4]["rois"], frames[i % 4]["gt_obj"],
                              {"poses": frames[i % 4]["poses"]}) for i in range(images))
                with dcl.crops.CropPrefetcher(builders[form], feed_args, depth=2, stream=bstream) as feed:
                    for d in feed:
                        step(d, acc)
            torch.cuda.synchronize()
            good = None
            if acc:
                tab = torch.cat(acc, 1).cpu()                            # distances, valid, pitch flag: the one read-back
                assert int(tab[2].sum()) == 0, "a crop's voxel rows exceeded the builder's v2p_pitch"
                good = tab[0][tab[1] > 0]
                assert bool(torch.isfinite(good).all())
            return (time.perf_counter() - t0) / images * 1e3, good

        with torch.no_grad():
            np.random.seed(1)
            for form in ("host", "device"):                              # graph capture, builder caches, lazy initialisation
                for i in range(6):
                    step(build(form, i), [])
            torch.cuda.synchronize()
            scheds = ("builder", "serial", "pipelined", "prefetch")
            t = {(form, s): [] for form in ("host", "device") for s in scheds}
            crops = {}
            for _ in range(args.blocks):
                for form in ("host", "device"):
                    for s in scheds:
                        ms, good = stream(form, s)
                        t[(form, s)].append(ms)
                        if good is not None:
                            crops[form] = int(good.numel())
        print("%s: %d object(s) per 480x640 frame, N = M = 1024, %g mm voxels; real crops per %d frames: host form %d, device form %d"
              % (tag, n_o, unit * 1e3, images, crops["host"], crops["device"]))
        for s in scheds:
            h, d = t[("host", s)], t[("device", s)]
            disjoint = max(d) < min(h) or max(h) < min(d)
            print("  %-9s host %s   device %s   device/host %+6.1f %%  ranges %s"
                  % (s, fmt(h), fmt(d), 100 * (statistics.median(d) / statistics.median(h) - 1.0),
                     "disjoint" if disjoint else "OVERLAP: no claim"))
        del net, builders
        torch.cuda.empty_cache()

    print("k_crop_draw alone, npoint 1024 (HIP events over 50 launches; us per launch)")
    for n_inst in (6, 1):
        for m in (2000, 30000, 300000):
            counts = torch.full((n_inst, 3), m, dtype=torch.int32, device=dev)
            for _ in range(5):
                dcl.ops.crop_draw(counts, 1024, 1, 0)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            for f in range(50):
                dcl.ops.crop_draw(counts, 1024, 1, f)
            ev[1].record()
            torch.cuda.synchronize()
            print("  %d instance(s) of m = %6d: %7.1f us" % (n_inst, m, ev[0].elapsed_time(ev[1]) / 50 * 1e3))


if __name__ == "__main__":
    main()
