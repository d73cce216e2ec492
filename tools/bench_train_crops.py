"""One TRAINING batch of 32 frames, from decoded frames to the dict Network(mode='train') consumes in HBM, in its two forms:

  device   CropBuilder.build_train (csrc/crops_train.hip): the frames are uploaded, the class table, the masked back-projection,
           the centroid, the re-pose, the grid filter, the sampling gather and the voxelisation run on the device
  host     the only alternative that exists: the training loader's `__getitem__` + `collate`
           (YCBV/dataloader_train_YCBV.py:105-266) restated in numpy below, one sample after the other in this process, and the
           finished dict uploaded

Image decoding is excluded on both sides (the frames are numpy arrays in memory).  Both forms make the loader's draws on the
global generators from the same seeds; the order of the draws differs for a batch (crops.py: build_train), so the two dicts hold
different samples of the same frames -- the restatement is checked against build_train sample by sample with replayed draws
before anything is timed.  No speed-up is assumed: what comes out is recorded.

  timeout -k 10 600 python tools/bench_train_crops.py

Timing: a host clock around a block of calls ended by a device synchronise, in six blocks that alternate the two forms in both
orders, in one process; reported are the median of a form's three block means and their range.  profiles/train_crops.txt
holds one run's output."""
import argparse
import importlib
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

MIN_BLOCK_S = 0.25


def block_ms(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def compare(forms, iters, warmup):
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
    return out, iters


class NumpyLoader(object):
    """`Dataset.__getitem__` ('train') and `collate` restated in numpy; `draw` as CropBuilder.build_train takes it"""

    def __init__(self, dcl, cfg, cad_pts, cad_col):
        self.dcl, self.n_inp, self.n_tmp = dcl, cfg["input_size"], cfg["tmp_size"]
        self.unit = np.array(cfg["unit_voxel_extent"]).astype(float)
        self.limit = np.array(cfg["voxel_num_limit"]).astype(float)
        self.extent = self.limit * self.unit
        self.mode = cfg["voxelization_mode"]
        self.cad_pts, self.cad_col = cad_pts, cad_col
        self.radius = {c: np.linalg.norm(p / 1000.0, axis=1).max() for c, p in cad_pts.items()}
        self.xmap = np.array([[j for _ in range(640)] for j in range(480)])
        self.ymap = np.array([[i for i in range(640)] for _ in range(480)])

    def item(self, frame, meta, draw):
        img, depth, label = frame
        obj = np.asarray(meta["cls_indexes"]).flatten().astype(np.int32)
        cx, cy, fx, fy = meta["camera"]
        mask_depth = depth != 0
        while True:
            idx = draw.pick(len(obj))
            mask_label = label == obj[idx]
            mask = mask_label * mask_depth
            if len(mask.nonzero()[0]) > 50:
                break
        rows, cols = np.any(mask_label, axis=1), np.any(mask_label, axis=0)
        r0, r1 = np.where(rows)[0][[0, -1]]
        c0, c1 = np.where(cols)[0][[0, -1]]
        rmin, rmax, cmin, cmax = self.dcl.crops.extent_box(r0, r1, c0, c1)
        target_r = meta["poses"][:, :, idx][:, 0:3]
        target_t = meta["poses"][:, :, idx][:, 3]
        choose = mask[rmin:rmax, cmin:cmax].flatten().nonzero()[0]
        if len(choose) < 50:
            return None
        img_masked = img[:, :, :3][rmin:rmax, cmin:cmax, :].astype(np.float32).reshape((-1, 3))[choose, :]
        img_masked = img_masked / 255.0 - np.array([0.485, 0.456, 0.406])[np.newaxis, :]
        depth_masked = depth[rmin:rmax, cmin:cmax].flatten()[choose][:, np.newaxis].astype(np.float32)
        xmap_masked = self.xmap[rmin:rmax, cmin:cmax].flatten()[choose][:, np.newaxis].astype(np.float32)
        ymap_masked = self.ymap[rmin:rmax, cmin:cmax].flatten()[choose][:, np.newaxis].astype(np.float32)
        pt2 = depth_masked / np.asarray(meta["factor_depth"]).reshape(-1)[0]
        pt0 = (ymap_masked - cx) * pt2 / fx
        pt1 = (xmap_masked - cy) * pt2 / fy
        cloud = np.concatenate((pt0, pt1, pt2), axis=1)
        centroid = np.mean(cloud, axis=0)
        cloud = cloud - centroid[np.newaxis, :]
        target_t = target_t - centroid
        aug_r = self.dcl.crops.euler2mat(*draw.angles()).astype(np.float32)
        target_t, target_r = target_t.astype(np.float32), target_r.astype(np.float32)
        cloud = (cloud - target_t[np.newaxis, :]) @ target_r
        target_t = target_t + np.array(draw.jitter()).astype(np.float32)
        target_r = target_r @ aug_r
        cloud = cloud @ target_r.T + target_t[np.newaxis, :]
        cls = int(obj[idx])
        inside = (np.abs(cloud[:, 0]) < self.extent[0] * 0.5) & (np.abs(cloud[:, 1]) < self.extent[1] * 0.5) & \
                 (np.abs(cloud[:, 2]) < self.extent[2] * 0.5)
        if np.sum(inside) <= 50:
            return None
        cloud, img_masked = cloud[inside, :], img_masked[inside, :]
        pick = draw.choice(cloud.shape[0], self.n_inp)
        cloud, img_masked = cloud[pick, :], img_masked[pick, :].astype(np.float32)
        model_points = (self.cad_pts[cls] / 1000.0).astype(np.float32)
        feat_inp = np.concatenate([np.ones((self.n_inp, 1), np.float32), img_masked, cloud], 1)
        feat_tmp = np.concatenate([np.ones((self.n_tmp, 1), np.float32), self.cad_col[cls].astype(np.float32), model_points], 1)
        half, unit = np.float32(self.extent[0] * 0.5), self.unit.astype(np.float32)
        return (feat_inp, ((cloud + half) / unit).astype(np.int64), feat_tmp, ((model_points + half) / unit).astype(np.int64),
                np.float32(cls - 1 in (12, 15, 18, 19, 20)), target_r, target_t, np.int32(cls - 1), np.float32(self.radius[cls]))

    def batch(self, frames, metas, draw, device="cuda"):
        items = [self.item(f, m, draw) for f, m in zip(frames, metas)]
        kept = [it is not None for it in items]
        items = [it for it in items if it is not None]
        b = len(items)
        out = {"kept": np.array(kept), "batch_offsets": (torch.arange(b + 1) * self.n_inp).int(), "voxel_num_limit": torch.tensor(self.limit)}
        for side, fi, vi, n in (("inp", 0, 1, self.n_inp), ("tmp", 2, 3, self.n_tmp)):
            ids = np.repeat(np.arange(b, dtype=np.int64), n)[:, None]
            coords = torch.from_numpy(np.concatenate([ids, np.concatenate([it[vi] for it in items], 0)], 1))
            occ, p2v, v2p = self.dcl.ops.voxelize_idx(coords, b, self.mode)
            out[side] = {"feats": torch.from_numpy(np.concatenate([it[fi] for it in items], 0)).to(device),
                         "occupied_voxels": occ.to(device), "p2v_maps": p2v.to(device), "v2p_maps": v2p.to(device)}
        out["labels"] = {"rot_gt": torch.from_numpy(np.stack([it[5] for it in items])).to(device),
                         "trans_gt": torch.from_numpy(np.stack([it[6] for it in items])).to(device),
                         "obj_idx": torch.from_numpy(np.stack([it[7] for it in items])[:, None]).to(device)}
        out["flags"] = torch.from_numpy(np.stack([it[4] for it in items])).to(device)
        out["radius"] = torch.from_numpy(np.stack([it[8] for it in items])[:, None]).to(device)
        return out


class Recorded(object):
    """records the draws of one form so that the other can replay them (the agreement check only)"""

    def __init__(self, inner):
        self.inner, self.log = inner, []

    def __getattr__(self, name):
        fn = getattr(self.inner, name)

        def call(*a):
            v = fn(*a)
            self.log.append((name, v))
            return v
        return call


class Replayed(object):
    def __init__(self, log):
        self.q = {}
        for name, v in log:
            self.q.setdefault(name, []).append(v)

    def __getattr__(self, name):
        return lambda *a: self.q[name].pop(0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_train_crops: needs the GPU (no CPU timing is meaningful)")
    dcl = importlib.import_module("dcl-net_amd")
    import train_scene as TS
    cfg = dict(TS.CFG, input_size=1024, tmp_size=1024)
    scs = [TS.make_train_scene(200 + i, tmp_size=cfg["tmp_size"], camera=1 + i % 2) for i in range(args.frames)]
    frames, metas = [(s["img"], s["depth"], s["label"]) for s in scs], [s["meta"] for s in scs]
    print("== one training batch: device (CropBuilder.build_train) vs host (the loader restated in numpy, then uploaded)")
    print("device: %s, torch %s; %d frames of 480 x 640 with 4 objects each, %d / %d points; six alternating blocks of at least "
          "%d calls and %.2f s after %d warm-up rounds" % (torch.cuda.get_device_name(0), torch.__version__, args.frames,
                                                         cfg["input_size"], cfg["tmp_size"], args.iters, MIN_BLOCK_S, args.warmup))
    for name, capacity in (("exact form (3 read-backs)", False), ("capacity form (2 read-backs)", True)):
        builder = dcl.crops.CropBuilder(cfg, scs[0]["cad_pts"], scs[0]["cad_col"], capacity=capacity)
        loader = NumpyLoader(dcl, cfg, scs[0]["cad_pts"], scs[0]["cad_col"])
        # agreement: the same draws through both forms.  Frame by frame, so that one list of draws serves both orders
        for f, m in list(zip(frames, metas))[:4]:
            np.random.seed(3)
            random.seed(3)
            rec = Recorded(dcl.crops.LoaderDraw())
            a = dcl.crops.exact_form(builder.build_train([f], [m], draw=rec))
            b = loader.batch([f], [m], Replayed(rec.log))
            assert a["kept"].tolist() == b["kept"].tolist()
            assert torch.equal(a["inp"]["feats"][:, :4], b["inp"]["feats"][:, :4])
            assert float((a["inp"]["feats"] - b["inp"]["feats"]).abs().max()) < 1e-5
            assert torch.equal(a["labels"]["trans_gt"], b["labels"]["trans_gt"]) and torch.equal(a["tmp"]["feats"], b["tmp"]["feats"])

        def device():
            np.random.seed(1)
            random.seed(1)
            return builder.build_train(frames, metas)

        def host():
            np.random.seed(1)
            random.seed(1)
            return loader.batch(frames, metas, dcl.crops.LoaderDraw())
        kept = int(device()["kept"].sum())
        res, iters = compare({"device": device, "host": host}, args.iters, args.warmup)
        (d, dlo, dhi), (h, hlo, hhi) = res["device"], res["host"]
        verdict = "slower" if dlo > hhi else "faster" if dhi < hlo else "within the spread"
        print("  %-30s device %8.3f ms [%.3f .. %.3f]   host %8.3f ms [%.3f .. %.3f]   device / host %.3f  (%s; %d of %d frames "
              "kept, %d calls per block)" % (name, d, dlo, dhi, h, hlo, hhi, d / h, verdict, kept, args.frames, iters))
        print("  %-30s per sample: device %.3f ms, host %.3f ms" % ("", d / max(kept, 1), h / max(kept, 1)))
    res_frames = [dcl.crops.CropBuilder.resident(*f) for f in frames]
    builder = dcl.crops.CropBuilder(cfg, scs[0]["cad_pts"], scs[0]["cad_col"], capacity=True)

    def resident():
        np.random.seed(1)
        random.seed(1)
        return builder.build_train(res_frames, metas)
    resident()
    v = sorted(block_ms(resident, max(args.iters, 5)) for _ in range(3))
    print("  %-30s device %8.3f ms [%.3f .. %.3f]   (frames already in HBM, CropBuilder.resident; no host form exists)" %
          ("capacity form, resident frames", v[1], v[0], v[2]))


if __name__ == "__main__":
    main()
