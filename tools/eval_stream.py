"""bench.py's `eval_stream` leg alone (crop builder -> forward -> ADD-S -> table, serial / pipelined / builder thread).
--template-cache: the YCB-V regime of that stream (6 objects per frame, N = M = 1024, capacity-form crops, default routing) with
the per-class template cache -- CropBuilder(template_ids=True) names the template side, Network.cache_templates(builder.
templates()) holds it -- beside the plain form in the same process: serial schedule and builder thread, images per second, and
whether both forms give the same ADD-S distances to 1e-6 m.  The metric's template cloud is data["labels"]["points_tmp"], which
the cached forward fills from the cache.
--device-table: that regime with draws="device" and stage2_chain(compose="device", trajectory=True), every refine iteration scored,
under three tabulation forms alternating block by block in one process -- (1) a read-back per frame into the host table, (2) the
distances kept and read back once at the end, (3) sharding.DeviceAddsTable -- ms per image as median and range over the blocks,
whether (2) and (3) give the same tables bit for bit, and the metric kernels' own times from device events.
--frames-per-call 1,2,4,6 [--pad 8]: the --device-table regime (form 3) fed SEVERAL frames per builder call (CropBuilder.
build_frames) against the per-frame loop through build(), block by block in one process; frames of 6, 4, 6 and 5
objects, so the crop count of a call changes from call to call unless it is padded.  --lm: the LineMOD regime -- one object per
frame, 5 mm voxels, build_lm_frames, DeviceLmTable -- at --frames-per-call 1,8,32.  ms per image as median [min .. max] over the
blocks per form, padded and unpadded forms apart; a gain is claimed only where a form's range lies wholly below the baseline's.
Also the largest |distance difference| between each form and the baseline and whether the tables' integer columns agree."""
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


def device_table_stream(dev, images=24, blocks=6, n_obj=6, iteration=2):
    n = 1024
    cfg_b = dict(input_size=n, tmp_size=n, unit_voxel_extent=[0.006] * 3, voxel_num_limit=[64] * 3, voxelization_mode=4)
    frames = [dcl.synth.make_frame(500 + i, n_obj=n_obj, tmp_size=n, empty=(i % n_obj if i % 2 else None)) for i in range(4)]
    res = [dcl.crops.CropBuilder.resident(f["img"], f["depth"], f["label"], dev) for f in frames]
    net = dcl.DCL_Net.Network(dcl.synth.default_cfg(n, n), mode="test")
    net.load_state_dict(dcl.synth.synth_state_dict(net, 1))
    net = net.to(dev).eval()
    ref = dcl.refiner.Refiner()
    ref.load_state_dict(dcl.synth.synth_state_dict(ref, 2))
    ref = ref.to(dev).eval()
    builder = dcl.crops.CropBuilder(cfg_b, frames[0]["cad_pts"], frames[0]["cad_col"], device=dev, capacity=True, template_ids=True,
                                    draws="device", draw_seed=1)
    net.cache_templates(builder.templates(), cfg_b["voxel_num_limit"])
    T, C = iteration + 1, 22                                             # (class ids 1 .. 21)
    S = dcl.sharding

    def frame(i):
        f, (im, de, la) = frames[i % 4], res[i % 4]
        d = builder.build(im, de, la, f["rois"], f["gt_obj"], poses=f["poses"])
        _, _, _, (rots, transs) = dcl.refiner.stage2_chain(net, ref, d, iteration, graph=True, compose="device", trajectory=True)
        b = rots.shape[1]
        return d["labels"]["points_tmp"].reshape(b, n, 3), d["tmp_cls"], rots, transs, d["labels"]["rot_gt"], d["labels"]["trans_gt"], d["valid"]

    def distances(cld, rots, transs, Rg, tg):
        return torch.stack([dcl.ops.add_s(cld, rots[t], transs[t], Rg, tg) for t in range(T)])

    def tabulate(hosts, rows):                                           # rows (T + 2, b) on the host: distances, valid, class
        b = rows.shape[1]
        for t in range(T):
            for k in range(b):
                hosts[t].add(int(rows[T + 1, k]), float(rows[t, k]) if rows[T, k] else float("inf"))

    def run(form, first):
        hosts = [S.AddsTable(C) for _ in range(T)]
        table, kept = S.DeviceAddsTable(C, steps=T, device=dev), []
        for i in range(first, first + images):
            cld, cls, rots, transs, Rg, tg, valid = frame(i)
            if form == "device_table":
                table.add_frame(cld, cls, rots, transs, Rg, tg, valid=valid, per_crop=True)
                continue
            rows = torch.cat([distances(cld, rots, transs, Rg, tg), valid.float().unsqueeze(0), cls.float().unsqueeze(0)])
            if form == "read_back_per_frame":
                tabulate(hosts, rows.cpu().numpy())
            else:
                kept.append(rows)
        if form == "device_table":
            return table.to_host_all()                                    # the one read-back
        if form == "read_back_at_the_end":
            tabulate(hosts, torch.cat(kept, dim=1).cpu().numpy())
        return hosts

    forms = ("read_back_per_frame", "read_back_at_the_end", "device_table")
    ms = {f: [] for f in forms}
    equal = True
    with torch.no_grad():
        for f in forms:                                                  # warm-up: graph captures, builder caches, scratch
            run(f, 0)
        for blk in range(blocks):
            tables = {}
            for f in (forms if blk % 2 == 0 else forms[::-1]):           # alternate the order inside the blocks
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                tables[f] = run(f, blk * images)
                torch.cuda.synchronize()
                ms[f].append((time.perf_counter() - t0) / images * 1e3)
            a, b = tables["read_back_at_the_end"], tables["device_table"]
            equal = equal and all(x.sums.tobytes() == y.sums.tobytes() and x.maxd.tobytes() == y.maxd.tobytes() for x, y in zip(a, b))
            last = b[-1].finalize()[:2]
        # the metric kernels alone, from device events
        cld, cls, rots, transs, Rg, tg, valid = frame(0)
        table = S.DeviceAddsTable(C, steps=T, device=dev)
        dis = dcl.ops.add_traj(cld, rots, transs, Rg, tg, valid=valid)
        ev = {}
        for name, call in (("add_frame_two_launches", lambda: table.add_frame(cld, cls, rots, transs, Rg, tg, valid=valid, per_crop=True)),
                           ("tabulate_one_launch", lambda: table.add_distances(cls, dis, valid)),
                           ("add_s_per_step_%d_calls" % T, lambda: distances(cld, rots, transs, Rg, tg))):
            for _ in range(10):
                call()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(200):
                call()
            e1.record()
            torch.cuda.synchronize()
            ev[name] = round(e0.elapsed_time(e1) / 200 * 1e3, 2)
    out = {"workload": "%d objects per 480x640 frame (every other frame: one empty mask), N=M=1024, template cache, draws on the "
                       "device, stage-2 chain with %d refine iterations, all %d poses scored; %d blocks of %d images"
                       % (n_obj, iteration, T, blocks, images),
           "ms_per_image": {f: {"median": round(float(np.median(v)), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
                            for f, v in ms.items()},
           "device_table_equals_read_back_at_the_end": bool(equal),
           "last_block_mean_auc_acc": list(last),
           "metric_kernels_us_per_call_back_to_back": ev}
    return out


def frame_batches_stream(dev, per_call, pad=None, lm=False, images=48, blocks=6, iteration=2):
    n = 1024
    unit = 0.005 if lm else 0.006
    cfg_b = dict(input_size=n, tmp_size=n, unit_voxel_extent=[unit] * 3, voxel_num_limit=[64] * 3, voxelization_mode=4)
    S = dcl.sharding
    T, C = iteration + 1, 22
    n_objs = (1, 1, 1, 1) if lm else (6, 4, 6, 5)
    frames = [dcl.synth.make_frame(500 + i, n_obj=k, tmp_size=n, empty=(1 if i == 2 and not lm else None)) for i, k in enumerate(n_objs)]
    for f in frames:
        if lm:                                                            # millimetres, as the LineMOD loaders read them
            f["depth"] = (f["depth"].astype(np.float64) / 10).astype(np.uint16)
    net = dcl.DCL_Net.Network(dcl.synth.default_cfg(n, n, unit), mode="test")
    net.load_state_dict(dcl.synth.synth_state_dict(net, 1))
    net = net.to(dev).eval()
    # every form keeps its captured graphs for the whole comparison (a run uses ONE form: the unpadded ones here need up to three
    # batch sizes each, the padded ones one or two); the default bound of 8 would make the forms evict each other block by block
    net.MAX_GRAPHS = 32
    ref = dcl.refiner.Refiner()
    ref.load_state_dict(dcl.synth.synth_state_dict(ref, 2))
    ref = ref.to(dev).eval()
    builder = dcl.crops.CropBuilder(cfg_b, frames[0]["cad_pts"], frames[0]["cad_col"], device=dev, capacity=True, template_ids=True,
                                    draws="device", draw_seed=1, camera=dcl.crops.LM_CAMERA if lm else dcl.crops.YCBV_CAMERA)
    cache = net.cache_templates(builder.templates(), cfg_b["voxel_num_limit"])
    if lm:
        masks = [f["label"] == int(f["gt_obj"][0]) for f in frames]
        gts = [(torch.from_numpy(f["poses"][:, :3, 0].astype(np.float32)).to(dev), torch.from_numpy(f["poses"][:, 3, 0]).to(dev)) for f in frames]
        diam = np.full(C, 0.1)
    else:
        res = [dcl.crops.CropBuilder.resident(f["img"], f["depth"], f["label"], dev) for f in frames]

    def new_table():
        return S.DeviceLmTable(diam, steps=T, device=dev) if lm else S.DeviceAddsTable(C, steps=T, device=dev)

    def build(first, k, padded):
        """the data dict of frames first .. first + k - 1: k == 1 unpadded is the per-frame path of the parent commit"""
        if lm:
            rows = [(frames[i % 4]["img"], frames[i % 4]["depth"], masks[i % 4], None, int(frames[i % 4]["gt_obj"][0]))
                    for i in range(first, first + k)]
            if k == 1 and not padded:
                fi, vi, cls, _, cen, valid = builder.build_lm(*rows[0][:3], None, rows[0][4], eval_mode=True)
                coords = torch.cat([torch.zeros((n, 1), dtype=torch.int64, device=dev), vi], 1)
                d = {"inp": builder._inp_side(fi, coords, 1), "tmp_cls": cls, "valid": valid, "all_centroids": cen.view(1, 3),
                     "batch_offsets": torch.arange(2).int() * n, "voxel_num_limit": torch.tensor(builder.limit),
                     "flags": torch.IntTensor([-1]), "labels": {}}
            else:
                d = builder.build_lm_frames(rows, eval_mode=True, pad_to=pad if padded else None)
            b = d["valid"].shape[0]
            live = [gts[i % 4] for i in range(first, first + k)]
            R = torch.eye(3, device=dev).repeat(b, 1, 1)
            t = torch.zeros((b, 3), dtype=torch.float64, device=dev)
            R[:k], t[:k] = torch.stack([g[0] for g in live]), torch.stack([g[1] for g in live])
            d["labels"] = {"rot_gt": R, "trans_gt": (t - d["all_centroids"].double()).float()}    # the loader's labels: the caller's
            return d
        if k == 1 and not padded:
            f, (im, de, la) = frames[first % 4], res[first % 4]
            return builder.build(im, de, la, f["rois"], f["gt_obj"], poses=f["poses"])
        group = [res[i % 4] + (frames[i % 4]["rois"], frames[i % 4]["gt_obj"], frames[i % 4]["poses"]) for i in range(first, first + k)]
        return builder.build_frames(group, pad_to=pad if padded else None)

    def run(form, first, sink=None):
        k, padded = form
        table = new_table()
        builder.draw_frame = first
        for i in range(first, first + images, k):
            d = build(i, k, padded)
            _, _, _, (rots, transs) = dcl.refiner.stage2_chain(net, ref, d, iteration, graph=True, compose="device", trajectory=True)
            b = rots.shape[1]
            args = (d["labels"]["points_tmp"].reshape(b, n, 3), d["tmp_cls"], rots, transs, d["labels"]["rot_gt"], d["labels"]["trans_gt"])
            table.add_frame(*args, valid=d["valid"], per_crop=True)
            if sink is not None:                                          # outside the timed runs: the distances of the live rows
                dis = dcl.ops.add_traj(args[0], rots, transs, args[4], args[5], valid=d["valid"], mode="add" if lm else "adds")
                sink.append(dis[:, d["valid"] >= 0])
        return table

    forms = [(1, False)] + [(k, False) for k in per_call if k != 1] + ([(k, True) for k in per_call] if pad else [])
    for k, _ in forms:
        if images % k:
            raise SystemExit("--frames-per-call %d does not divide the %d images of a block" % (k, images))
    name = lambda f: "%d frame%s per call%s" % (f[0], "" if f[0] == 1 else "s", ", padded to %d" % pad if f[1] else "")   # noqa: E731
    ms = {f: [] for f in forms}
    with torch.no_grad():
        dists, tabs = {}, {}
        for f in forms:                                                  # warm-up of every batch size used, and the distances
            sink = []
            tabs[f] = run(f, 0, sink)
            dists[f] = torch.cat(sink, 1).cpu()
        graphs = len(net.__dict__.get("_graphs", {}))
        for blk in range(blocks):
            for f in (forms if blk % 2 == 0 else forms[::-1]):          # alternate the order inside the blocks
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(f, blk * images)
                torch.cuda.synchronize()
                ms[f].append((time.perf_counter() - t0) / images * 1e3)
    base = forms[0]
    host = {f: tabs[f].to_host_all() for f in forms}
    ints = (lambda t: t.counts) if lm else (lambda t: t.sums[:, [0, 1, 3]])     # noqa: E731
    out = {"workload": ("LineMOD regime: one object per 480x640 frame, box from the mask, 5 mm voxels, DeviceLmTable" if lm else
                        "YCB-V regime: 480x640 frames of 6, 4, 6 and 5 objects (one empty mask in four frames), DeviceAddsTable") +
                       "; N=M=1024, template cache, draws on the device, stage-2 chain with %d refine iterations, all %d poses "
                       "scored; %d blocks of %d images per form after a warm-up of every form" % (iteration, T, blocks, images),
           "baseline": name(base) + " through build%s() -- the parent commit's path" % ("_lm" if lm else ""),
           "ms_per_image median [min .. max]": {}, "gain_claimed (ranges disjoint)": {}, "max_abs_distance_difference_to_baseline_m": {},
           "table_integer_columns_equal_to_baseline": {}, "captured_forward_graphs_after_warm_up": graphs,
           "template_miss": int(cache.miss.cpu()[0])}
    for f in forms:
        v = ms[f]
        out["ms_per_image median [min .. max]"][name(f)] = "%.3f [%.3f .. %.3f]" % (float(np.median(v)), min(v), max(v))
        if f != base:
            out["gain_claimed (ranges disjoint)"][name(f)] = ("%.2fx" % (float(np.median(ms[base])) / float(np.median(v)))
                                                              if max(v) < min(ms[base]) else "none")
            a, b = dists[f], dists[base]
            both = torch.isfinite(a) & torch.isfinite(b)
            same_inf = bool((torch.isfinite(a) == torch.isfinite(b)).all())
            out["max_abs_distance_difference_to_baseline_m"][name(f)] = (float((a[both] - b[both]).abs().max()) if same_inf else "inf pattern differs")
            out["table_integer_columns_equal_to_baseline"][name(f)] = bool(all(np.array_equal(ints(x), ints(y)) for x, y in zip(host[f], host[base])))
    return out


def _int_list(flag, default):
    a = sys.argv[1:]
    return [int(v) for v in a[a.index(flag) + 1].split(",")] if flag in a else default


if "--frames-per-call" in sys.argv[1:] or "--lm" in sys.argv[1:]:
    lm = "--lm" in sys.argv[1:]
    pad = _int_list("--pad", [None])[0]
    per_call = _int_list("--frames-per-call", [1, 8, 32] if lm else [1, 2, 4, 6])
    print(json.dumps(frame_batches_stream(torch.device("cuda:0"), per_call, pad, lm, images=256 if lm else 240), indent=1))
elif "--device-table" in sys.argv[1:]:
    print(json.dumps(device_table_stream(torch.device("cuda:0")), indent=1))
elif "--template-cache" in sys.argv[1:]:
    print(json.dumps(cached_eval_stream(torch.device("cuda:0")), indent=1))
else:
    print(json.dumps(bench.eval_stream_bench(dcl, torch.device("cuda:0")), indent=1))
