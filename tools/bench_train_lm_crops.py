"""One LineMOD TRAINING batch of 32 frames, from decoded frames to the dict Network(mode='train') consumes in HBM:

  device   CropBuilder.build_train_lm (csrc/crops_train_lm.hip): the frames and their occluder frames are uploaded; mask
           extents, the occlusion paste with its commit / roll-back, the masked back-projection, the centroid, the float64
           re-pose, the grid filter, the sampling gather and the voxelisation run on the device
  host     the only alternative that exists: the training loader's `occlude_with_another_object`, `__getitem__` and `collate`
           (LM/dataloader_train_LM.py:125-348) restated in numpy (tests/train_lm_scene.py::numpy_occlude and below), one sample
           after the other in this process, and the finished dict uploaded

Three figures: numpy frames (both forms), frames already in HBM (CropBuilder.resident_lm; device only), and the paste alone
(ops.mask_extent + ops.occlude_paste on resident frames).  Image decoding is excluded on both sides.  The method is that of
tools/bench_train_crops.py: a host clock around a block of calls ended by a device synchronise, six blocks that alternate the
two forms in both orders in one process, the median of a form's three block means and their range.  The restatement is checked
against build_train_lm with replayed draws before anything is timed.  No speed-up is assumed: what comes out is recorded.

  timeout -k 10 600 python tools/bench_train_lm_crops.py        (profiles/train_lm_crops.txt holds one run's output)"""
import argparse
import importlib
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_train_crops import MIN_BLOCK_S, Recorded, Replayed, block_ms, compare  # noqa: E402


class NumpyLmLoader(object):
    """`occlude_with_another_object`, `Dataset.__getitem__` ('train') and `collate` restated in numpy; `draw` as
    CropBuilder.build_train_lm takes it"""

    def __init__(self, dcl, LS, cfg, cad_pts, cad_col):
        self.dcl, self.LS, self.n_inp, self.n_tmp = dcl, LS, cfg["input_size"], cfg["tmp_size"]
        self.unit = np.array(cfg["unit_voxel_extent"]).astype(float)
        self.limit = np.array(cfg["voxel_num_limit"]).astype(float)
        self.extent = self.limit * self.unit
        self.mode = cfg["voxelization_mode"]
        self.cad_pts, self.cad_col = cad_pts, cad_col
        self.xmap = np.array([[j for _ in range(640)] for j in range(480)])
        self.ymap = np.array([[i for i in range(640)] for _ in range(480)])

    def item(self, s, draw):
        img, depth, label = s["img"][:, :, :3], s["depth"], s["mask"]
        if s["other"] is not None:
            oys, oxs = np.nonzero(s["other"][2][:, :, 0])
            ys, xs = np.nonzero(label[:, :, 0])
            if oys.size and ys.size:
                oh, ow = oys.max() - oys.min() + 1, oxs.max() - oxs.min() + 1
                sy, sx = draw.paste(ys.min() - oh + 1, ys.max() + 1, xs.min() - ow + 1, xs.max() + 1)
                img, depth, label = self.LS.numpy_occlude(img, depth, label, s["other"][0], s["other"][1], s["other"][2], sy, sx)[:3]
        cx, cy, fx, fy = self.LS.LM_CAMERA
        mask = (label[:, :, 0] == 255) * (depth != 0)
        rmin, rmax, cmin, cmax = self.dcl.crops.lm_box(s["obj_bb"])
        target_r = np.resize(np.array(s["cam_R_m2c"]), (3, 3))
        target_t = np.array(s["cam_t_m2c"]) / 1000.0
        choose = mask[rmin:rmax, cmin:cmax].flatten().nonzero()[0]
        if len(choose) == 0:
            return None
        img_masked = img[rmin:rmax, cmin:cmax, :].astype(np.float32).reshape((-1, 3))[choose, :]
        img_masked = img_masked / 255.0 - np.array([0.485, 0.456, 0.406])[np.newaxis, :]
        depth_masked = depth[rmin:rmax, cmin:cmax].flatten()[choose][:, np.newaxis].astype(np.float32)
        xmap_masked = self.xmap[rmin:rmax, cmin:cmax].flatten()[choose][:, np.newaxis].astype(np.float32)
        ymap_masked = self.ymap[rmin:rmax, cmin:cmax].flatten()[choose][:, np.newaxis].astype(np.float32)
        pt2 = depth_masked / 1.0
        pt0 = (ymap_masked - cx) * pt2 / fx
        pt1 = (xmap_masked - cy) * pt2 / fy
        cloud = np.concatenate((pt0, pt1, pt2), axis=1) / 1000.0
        centroid = np.mean(cloud, axis=0)
        cloud = cloud - centroid[np.newaxis, :]
        target_t = target_t - centroid
        aug_r = self.dcl.crops.euler2mat(*draw.angles())
        cloud = (cloud - target_t[np.newaxis, :]) @ target_r                     # float64 from here on
        target_t = target_t + np.array(draw.jitter())
        target_r = target_r @ aug_r
        cloud = cloud @ target_r.T + target_t[np.newaxis, :]
        obj = int(s["obj"])
        inside = (np.abs(cloud[:, 0]) < self.extent[0] * 0.5) & (np.abs(cloud[:, 1]) < self.extent[1] * 0.5) & \
                 (np.abs(cloud[:, 2]) < self.extent[2] * 0.5)
        if np.sum(inside) <= 128:
            return None
        cloud, img_masked = cloud[inside, :], img_masked[inside, :]
        pick = draw.choice(cloud.shape[0], self.n_inp)
        cloud, img_masked = cloud[pick, :].astype(np.float32), img_masked[pick, :].astype(np.float32)
        model_points = (self.cad_pts[obj] / 1000.0).astype(np.float32)
        feat_inp = np.concatenate([np.ones((self.n_inp, 1), np.float32), img_masked, cloud], 1)
        feat_tmp = np.concatenate([np.ones((self.n_tmp, 1), np.float32), self.cad_col[obj].astype(np.float32), model_points], 1)
        half, unit = np.float32(self.extent[0] * 0.5), self.unit.astype(np.float32)
        idx = self.LS.OBJLIST.index(obj)
        return (feat_inp, ((cloud + half) / unit).astype(np.int64), feat_tmp, ((model_points + half) / unit).astype(np.int64),
                np.float32(idx in (7, 8)), target_r.astype(np.float32), target_t.astype(np.float32), np.int32(idx), centroid)

    def batch(self, samples, draw, device="cuda"):
        items = [self.item(s, draw) for s in samples]
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
                         "trans_gt": torch.from_numpy(np.stack([it[6] for it in items])).to(device)}
        out["flags"] = torch.from_numpy(np.stack([it[4] for it in items])).to(device)
        out["obj_idx"] = torch.from_numpy(np.stack([it[7] for it in items])).to(device)
        out["centriods"] = torch.from_numpy(np.stack([it[8] for it in items])).to(device)
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_train_lm_crops: needs the GPU (no CPU timing is meaningful)")
    dcl = importlib.import_module("dcl-net_amd")
    import train_lm_scene as LS
    cfg = dict(LS.CFG, input_size=1024, tmp_size=1024)
    objs = [o for o in LS.OBJLIST if o != 15]
    scs = [LS.make_lm_scene(300 + i, tmp_size=cfg["tmp_size"], own=(150 + 5 * (i % 9), 120 + 9 * (i % 11), 110, 120),
                            occ=(60 + i % 30, 70 + i % 20), obj=objs[i % len(objs)]) for i in range(args.frames)]
    samples = [LS.sample_of(s) for s in scs]
    print("== one LineMOD training batch: device (CropBuilder.build_train_lm) vs host (the loader restated in numpy, then uploaded)")
    print("device: %s, torch %s; %d frames of 480 x 640 with an occluder frame each, %d / %d points; six alternating blocks of at "
          "least %d calls and %.2f s after %d warm-up rounds" % (torch.cuda.get_device_name(0), torch.__version__, args.frames,
                                                                 cfg["input_size"], cfg["tmp_size"], args.iters, MIN_BLOCK_S, args.warmup))
    loader = NumpyLmLoader(dcl, LS, cfg, scs[0]["cad_pts"], scs[0]["cad_col"])
    for name, capacity in (("exact form (4 read-backs)", False), ("capacity form (3 read-backs)", True)):
        builder = dcl.crops.CropBuilder(cfg, scs[0]["cad_pts"], scs[0]["cad_col"], camera=dcl.crops.LM_CAMERA, capacity=capacity)
        # agreement: the same draws through both forms.  Frame by frame, so that one list of draws serves both orders
        for s in samples[:4]:
            np.random.seed(3)
            random.seed(3)
            rec = Recorded(dcl.crops.LoaderDraw())
            a = dcl.crops.exact_form(builder.build_train_lm([s], draw=rec))
            b = loader.batch([s], Replayed(rec.log))
            assert a["kept"].tolist() == b["kept"].tolist()
            assert torch.equal(a["inp"]["feats"][:, :4], b["inp"]["feats"][:, :4])
            assert float((a["inp"]["feats"] - b["inp"]["feats"]).abs().max()) < 1e-6
            assert float((a["inp"]["feats"] != b["inp"]["feats"]).float().mean()) < 1e-3     # float64 re-pose: BLAS order, rare ulps
            assert torch.equal(a["tmp"]["feats"], b["tmp"]["feats"]) and torch.equal(a["centriods"], b["centriods"])

        def device():
            np.random.seed(1)
            random.seed(1)
            return builder.build_train_lm(samples)

        def host():
            np.random.seed(1)
            random.seed(1)
            return loader.batch(samples, dcl.crops.LoaderDraw())
        first = device()
        kept, occluded = int(first["kept"].sum()), int(first["occluded"].sum())
        res, iters = compare({"device": device, "host": host}, args.iters, args.warmup)
        (d, dlo, dhi), (h, hlo, hhi) = res["device"], res["host"]
        verdict = "slower" if dlo > hhi else "faster" if dhi < hlo else "within the spread"
        print("  %-30s device %8.3f ms [%.3f .. %.3f]   host %8.3f ms [%.3f .. %.3f]   device / host %.3f  (%s; %d of %d frames "
              "kept, %d occluded, %d calls per block)" % (name, d, dlo, dhi, h, hlo, hhi, d / h, verdict, kept, args.frames, occluded, iters))
        print("  %-30s per sample: device %.3f ms, host %.3f ms" % ("", d / max(kept, 1), h / max(kept, 1)))
    res_samples = []
    for s in samples:
        r = dict(s)
        r["img"], r["depth"], r["mask"] = dcl.crops.CropBuilder.resident_lm(s["img"], s["depth"], s["mask"])
        r["other"] = dcl.crops.CropBuilder.resident_lm(*s["other"])
        res_samples.append(r)
    builder = dcl.crops.CropBuilder(cfg, scs[0]["cad_pts"], scs[0]["cad_col"], camera=dcl.crops.LM_CAMERA, capacity=True)

    def resident():
        np.random.seed(1)
        random.seed(1)
        return builder.build_train_lm(res_samples)
    resident()
    v = sorted(block_ms(resident, max(args.iters, 5)) for _ in range(3))
    print("  %-30s device %8.3f ms [%.3f .. %.3f]   (frames already in HBM, CropBuilder.resident_lm; no host form exists)" %
          ("capacity form, resident frames", v[1], v[0], v[2]))
    # the paste alone: extents, then the composite with its commit / roll-back, on stacked resident frames and fixed plans
    i_t = torch.stack([r["img"] for r in res_samples])
    d_t = torch.stack([r["depth"] for r in res_samples])
    m_t = torch.stack([r["mask"] for r in res_samples] + [r["other"][2] for r in res_samples])
    oi_t, od_t = torch.stack([r["other"][0] for r in res_samples]), torch.stack([r["other"][1] for r in res_samples])
    nf = len(res_samples)
    ext = dcl.ops.mask_extent(m_t).cpu().numpy()
    plans = np.zeros((nf, dcl.ops.PASTE_PLAN_INTS), np.int32)
    rng = np.random.default_rng(1)
    for f, s in enumerate(samples):
        own, oth = ext[f, :4], ext[nf + f, :4]
        oh, ow = int(oth[1] - oth[0]) + 1, int(oth[3] - oth[2]) + 1
        row = dcl.crops.lm_paste_plan(480, 640, own, oth, rng.integers(max(own[0] - oh + 1, 0), own[1] + 1 - oh // 2),
                                      rng.integers(max(own[2] - ow + 1, 0), own[3] + 1 - ow // 2))
        if row is not None:
            plans[f] = row
            plans[f, 1] = f
        r0, r1, c0, c1 = dcl.crops.lm_box(s["obj_bb"])
        plans[f, 12:16] = (max(r0, 0), min(r1, 480), max(c0, 0), min(c1, 640))
    plan_t = torch.from_numpy(plans).cuda()

    def paste():
        e = dcl.ops.mask_extent(m_t)
        return dcl.ops.occlude_paste(i_t, d_t, m_t[:nf], oi_t, od_t, m_t[nf:], plans, plan_t, e[:nf])
    info = paste()[3].cpu().numpy()
    v = sorted(block_ms(paste, 20) for _ in range(3))
    print("  %-30s device %8.3f ms [%.3f .. %.3f]   (mask_extent of %d masks + occlude_paste of %d frames, resident; %d pastes "
          "enabled, %d kept)" % ("the paste alone", v[1], v[0], v[2], 2 * nf, nf, int(plans[:, 0].sum()), int(info[:, 0].sum())))


if __name__ == "__main__":
    main()
