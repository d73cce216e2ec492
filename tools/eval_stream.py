"""bench.py's `eval_stream` leg alone (crop builder -> forward -> ADD-S -> table, serial / pipelined / builder thread).
--template-cache: the YCB-V regime of that stream (6 objects per frame, N = M = 1024, capacity-form crops, default routing) with
the per-class template cache -- CropBuilder(template_ids=True) names the template side, Network.cache_templates(builder.
templates()) holds it -- beside the plain form in the same process: serial schedule and builder thread, images per second, and
whether both forms give the same ADD-S distances to 1e-6 m.  The metric's template cloud is data["labels"]["points_tmp"], which
the cached forward fills from the cache."""
import importlib, json, os, sys, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench
dcl = importlib.import_module("dcl-net_amd")


def cached_eval_stream(dev, images=40, n_obj=6):
    cfg_b = dict(input_size=1024, tmp_size=1024, unit_voxel_extent=[0.006] * 3, voxel_num_limit=[64] * 3, voxelization_mode=4)
    frames = [dcl.synth.make_frame(500 + i, n_obj=n_obj, tmp_size=1024) for i in range(4)]
    res = [dcl.crops.CropBuilder.resident(f["img"], f["depth"], f["label"], dev) for f in frames]
    net = dcl.DCL_Net.Network(dcl.synth.default_cfg(1024, 1024), mode="test")
    net.load_state_dict(dcl.synth.synth_state_dict(net, 1))
    net = net.to(dev).eval()
    builders = {form: dcl.crops.CropBuilder(cfg_b, frames[0]["cad_pts"], frames[0]["cad_col"], device=dev, capacity=True,
                                            template_ids=(form == "cached")) for form in ("plain", "cached")}
    cache = net.cache_templates(builders["cached"].templates(), cfg_b["voxel_num_limit"])
    bstream = torch.cuda.Stream(dev)
    out = {"workload": "%d objects per 480x640 frame, N=M=1024, 6 mm voxels; %d classes cached (%.1f MB)"
                       % (n_obj, len(cache.class_ids), cache.nbytes() / 1e6)}
    dists = {}

    def frame_args(i):
        f, (im, de, la) = frames[i % 4], res[i % 4]
        return (im, de, la, f["rois"], f["gt_obj"], {"poses": f["poses"]})

    def step(d, sink):
        p = net(d)
        b = p["rot_pred"].shape[0]
        sink.append(dcl.sharding.add_s(d["labels"]["points_tmp"].reshape(b, 1024, 3), p["rot_pred"], p["trans_pred"],
                                       d["labels"]["rot_gt"], d["labels"]["trans_gt"]))

    with torch.no_grad():
        for form, builder in builders.items():
            np.random.seed(1)
            for i in range(6):                                   # warm-up: graph capture, builder caches
                a = frame_args(i)
                step(builder.build(*a[:-1], **a[-1]), [])
            torch.cuda.synchronize()
            out[form] = {}
            for sched in ("serial", "prefetch_thread"):
                np.random.seed(2)
                sink = []
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if sched == "serial":
                    for i in range(images):
                        a = frame_args(i)
                        step(builder.build(*a[:-1], **a[-1]), sink)
                else:
                    with dcl.crops.CropPrefetcher(builder, (frame_args(i) for i in range(images)), depth=2, stream=bstream) as feed:
                        for d in feed:
                            step(d, sink)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                out[form][sched] = {"images_per_s": round(images / dt, 1), "ms_per_image": round(dt / images * 1e3, 3)}
                dists[form, sched] = torch.cat(sink).cpu()
    out["template_miss"] = int(cache.miss.cpu()[0])
    out["max_distance_difference_m"] = max(float((dists["cached", s] - dists["plain", s]).abs().max()) for s in ("serial", "prefetch_thread"))
    return out


if "--template-cache" in sys.argv[1:]:
    print(json.dumps(cached_eval_stream(torch.device("cuda:0")), indent=1))
else:
    print(json.dumps(bench.eval_stream_bench(dcl, torch.device("cuda:0")), indent=1))
