#!/usr/bin/env python3
"""One-crop stream (LineMOD-style b=1 calls): ms per call and kernel nodes of the captured forward -- the lm_stream leg of
bench.py on its own.  usage: stream_b1.py [reps] [crops per call] [--template-cache]
--template-cache: the same stream with the per-class template cache (Network.cache_templates): every call carries
data["tmp_cls"] instead of data["tmp"]; launch by launch and as the whole-forward graph replay, like the leg itself."""
import importlib, json, os, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench
dcl = importlib.import_module("dcl-net_amd")
if os.environ.get("DCL_USE_DIAG"):                 # A/B through the diagnostic library's switches (tools/_diag.py reads DCL_CONV_* here)
    from _diag import use_diag
    use_diag(dcl)


def cached_stream(dev, reps=100, b=1):
    """bench.lm_stream_bench's workload and timing with the cached form of the call"""
    cfg = dcl.synth.default_cfg(1024, 1024, unit=0.005)
    net = dcl.DCL_Net.Network(cfg, mode="test", graph_max_batch=0)
    net.load_state_dict(dcl.synth.synth_state_dict(net, 1))
    net = net.to(dev).eval()
    data = bench.to_device(dcl.synth.make_batch(b, 1024, 1024, unit=0.005), dev)
    net.cache_templates({int(c): dcl.synth.class_template_side(int(c), 1024, 0.005) for c in set(data["obj_idx"].tolist())},
                        data["voxel_num_limit"])
    del data["tmp"]
    data["tmp_cls"] = data["obj_idx"].to(dev).int()
    out = {"workload": "LineMOD stream with the template cache: %d crop%s per call, N=M=1024, 64^3 x 5 mm voxels"
                       % (b, "" if b == 1 else "s")}
    for name, fn, warm, n in (("eager", lambda: net(data), 3, reps), ("hipgraph", lambda: net.forward_graphed(data), 10, 8 * reps)):
        with torch.no_grad():
            for _ in range(warm):
                fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                fn()
            torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / n * 1e3
        out[name] = {"ms_per_frame": round(ms, 3), "frames_per_s": round(1e3 / ms, 1), "calls_timed": n}
    ent = next(iter(getattr(net, "_graphs", {}).values()), None)
    out["hipgraph"]["kernel_nodes"] = None if ent is None else ent.get("nodes")
    out["template_miss"] = int(net.template_cache.miss.cpu()[0])
    return out


argv = [a for a in sys.argv[1:] if a != "--template-cache"]
reps, b = int(argv[0]) if len(argv) > 0 else 100, int(argv[1]) if len(argv) > 1 else 1
if "--template-cache" in sys.argv[1:]:
    print(json.dumps(cached_stream(torch.device("cuda:0"), reps=reps, b=b)))
else:
    print(json.dumps(bench.lm_stream_bench(dcl, torch.device("cuda:0"), reps=reps, b=b)))
