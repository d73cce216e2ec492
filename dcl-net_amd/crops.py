"""Device-side crop builder: what `YCBDataset.__getitem__` does per image (YCBV/dataloader_test_YCBV.py:99-258), with
the per-pixel work on the GPU (csrc/crops.hip) and the result already resident in HBM for `Network.forward`.

    builder = CropBuilder(cfg, cad_points_mm, cad_colors)            # cfg: input_size, tmp_size, unit_voxel_extent, ...
    data = builder.build(img_u8, depth_u16, label, rois, gt_obj, poses)     # the loader's dict, CUDA tensors

The sampling draws stay `np.random.choice` on the host, made in the reference's order with the reference's arguments, so
a seeded run consumes the global numpy RNG stream exactly like the original loader and produces the same crops.  That
needs the per-instance point counts on the host: the one read-back of the builder (plus the {V, maxActive} read-back of
each voxelize_idx).  No CPU fallback: the arrays are uploaded and everything else happens on the device.

CropBuilder(draws="device") is the opt-in form without that read-back: the draws are made on the GPU from a counter-based
generator (ops.crop_draw; include/dclnet_hip.h pins it) -- NOT the loader's MT19937 stream, a different sample of the same
distribution that repeats from (draw_seed, draw_frame).  With capacity=True a frame then goes from images to `data` without a
host synchronisation; nothing is dropped from the batch, and data["valid"] says which crops are real.

build_frames / build_lm_frames / build_lmo_frames build the crops of SEVERAL frames in one call (the same crops, bit for bit, as
the per-frame calls), and pad_to=k pads the batch to a multiple of k with rows of valid == -1 that the metric kernels skip, so
that one captured graph serves a run whose crop count changes from call to call.
"""
import math
import random
import time

import numpy as np
import torch

from . import ops

RGB_MEAN = (0.485, 0.456, 0.406)                                     # dataloader_test_YCBV.py:57,145
YCBV_CAMERA = (312.9869, 241.3109, 1066.778, 1067.487, 10000.0, 1.0)  # cx, cy, fx, fy, depth scale (:77-81), post-division
LM_CAMERA = (325.26110, 242.04899, 572.41140, 573.57043, 1.0, 1000.0)  # LM/dataloader_test_LM.py:104-107,153-160
MIN_VALID = 32                                                        # :163
LM_MIN_VALID = 128                                                    # LM/dataloader_test_LM.py:197
LMO_MIN_VALID = 0                                                     # LM/dataloader_test_LMO.py:262 (`np.sum(choose_idx)>0`)
# the training loader (YCBV/dataloader_train_YCBV.py): its two cameras (cx, cy, fx, fy; :83-91 -- the second one for the real
# sequences 0060 and later, :113-122), `minimum_num_pt` (:97) and the symmetric objects' indices obj - 1 (:98)
YCBV_TRAIN_CAMERA_1 = (312.9869, 241.3109, 1066.778, 1067.487)
YCBV_TRAIN_CAMERA_2 = (323.7872, 279.6921, 1077.836, 1078.189)
TRAIN_MIN_PT = 50
TRAIN_SYMMETRY_OBJ_IDX = (12, 15, 18, 19, 20)
# the LineMOD training loader (LM/dataloader_train_LM.py): its object list (:43), the symmetric objects' indices IN that list
# (:120,195: objects 10 and 11), the in-grid point threshold (:201) and the mask sum below which an occlusion is undone (:343)
LM_OBJLIST = (1, 2, 4, 5, 6, 8, 9, 10, 11, 12, 13, 14, 15)
LM_TRAIN_SYMMETRY_OBJ_IDX = (7, 8)
LM_TRAIN_MIN_PT = 128
LM_OCCLUDE_MIN_SUM = 20


def snap_box(rois, row, img_h=480, img_w=640):
    """`get_bbox` (dataloader_test_YCBV.py:266-303): the detection's box grown to sides that are multiples of 40 px
    (0 -> 40), kept centred and pushed back inside the image.  Returns (rmin, rmax, cmin, cmax)."""
    r0, r1 = max(int(rois[row][3]) + 1, 0), min(int(rois[row][5]) - 1, img_h)
    c0, c1 = max(int(rois[row][2]) + 1, 0), min(int(rois[row][4]) - 1, img_w)

    def grow(v):                       # open intervals between the borders -1, 40, 80, ... 680 round up to the next border
        return (v // 40 + 1) * 40 if -1 < v < 680 and (v % 40 != 0 or v == 0) else v
    hr, hc = int(grow(r1 - r0) / 2), int(grow(c1 - c0) / 2)
    mr, mc = int((r0 + r1) / 2), int((c0 + c1) / 2)
    r0, r1, c0, c1 = mr - hr, mr + hr, mc - hc, mc + hc
    if r0 < 0:
        r0, r1 = 0, r1 - r0
    if c0 < 0:
        c0, c1 = 0, c1 - c0
    if r1 > img_h:
        r0, r1 = r0 - (r1 - img_h), img_h
    if c1 > img_w:
        c0, c1 = c0 - (c1 - img_w), img_w
    return r0, r1, c0, c1


def lm_box(obj_bb, img_h=480, img_w=640):
    """`get_bbox` of the LineMOD loader (LM/dataloader_test_LM.py:287-333): [x, y, w, h] -> (rmin, rmax, cmin, cmax) with
    sides grown to multiples of 40 px like `snap_box`."""
    r0, r1, c0, c1 = obj_bb[1], obj_bb[1] + obj_bb[3], obj_bb[0], obj_bb[0] + obj_bb[2]
    r0, c0 = max(r0, 0), max(c0, 0)
    r1 = img_h - 1 if r1 >= img_h else r1
    c1 = img_w - 1 if c1 >= img_w else c1

    def grow(v):
        return (v // 40 + 1) * 40 if -1 < v < 680 and (v % 40 != 0 or v == 0) else v
    hr, hc = int(grow(r1 - r0) / 2), int(grow(c1 - c0) / 2)
    mr, mc = int((r0 + r1) / 2), int((c0 + c1) / 2)
    r0, r1, c0, c1 = mr - hr, mr + hr, mc - hc, mc + hc
    if r0 < 0:
        r0, r1 = 0, r1 - r0
    if c0 < 0:
        c0, c1 = 0, c1 - c0
    if r1 > img_h:
        r0, r1 = r0 - (r1 - img_h), img_h
    if c1 > img_w:
        c0, c1 = c0 - (c1 - img_w), img_w
    return r0, r1, c0, c1


def extent_box(rmin, rmax, cmin, cmax, img_h=480, img_w=640):
    """`get_bbox(mask_label)` of the training loader (dataloader_train_YCBV.py:280-318) from the mask's extent -- rmin, rmax, cmin,
    cmax are the first and last set row / column, INCLUSIVE (np.where(rows)[0][[0, -1]]): sides grown to the next entry of the
    border list (a side that equals an entry stays), the box centred on the extent and shifted back inside the loader's
    img_h x img_w image.  Returns (rmin, rmax, cmin, cmax), the slice bounds."""
    r0, r1, c0, c1 = int(rmin), int(rmax) + 1, int(cmin), int(cmax) + 1

    def grow(v):                       # `r_b > border_list[tt] and r_b < border_list[tt + 1]` over -1, 40, 80, ... 680
        return (v // 40 + 1) * 40 if -1 < v < 680 and (v % 40 != 0 or v == 0) else v
    hr, hc = int(grow(r1 - r0) / 2), int(grow(c1 - c0) / 2)
    mr, mc = int((r0 + r1) / 2), int((c0 + c1) / 2)
    r0, r1, c0, c1 = mr - hr, mr + hr, mc - hc, mc + hc
    if r0 < 0:
        r0, r1 = 0, r1 - r0
    if c0 < 0:
        c0, c1 = 0, c1 - c0
    if r1 > img_h:
        r0, r1 = r0 - (r1 - img_h), img_h
    if c1 > img_w:
        c0, c1 = c0 - (c1 - img_w), img_w
    return r0, r1, c0, c1


def euler2mat(a1, a2, a3):
    """`transforms3d.euler.euler2mat(a1, a2, a3)` with its default axes 'sxyz' (static x, y, z), taken as Rz(a3) Ry(a2) Rx(a1) in
    float64.  transforms3d is not installed where this project is built: the convention is an ASSUMPTION that is not pinned
    against the package.  The one place the augmentation rotation is written."""
    c1, s1, c2, s2, c3, s3 = math.cos(a1), math.sin(a1), math.cos(a2), math.sin(a2), math.cos(a3), math.sin(a3)
    rx = np.array([[1.0, 0.0, 0.0], [0.0, c1, -s1], [0.0, s1, c1]])
    ry = np.array([[c2, 0.0, s2], [0.0, 1.0, 0.0], [-s2, 0.0, c2]])
    rz = np.array([[c3, -s3, 0.0], [s3, c3, 0.0], [0.0, 0.0, 1.0]])
    return rz @ ry @ rx


def lm_paste_plan(H, W, own_extent, other_extent, start_y, start_x, other_channels=3):
    """The slicing of `occlude_with_another_object` (LM/dataloader_train_LM.py:307-334) on two mask extents and the two drawn
    starts, bug for bug -> the plan row ops.occlude_paste takes (ops.PASTE_PLAN; `other` 0 and the crop box empty: the caller's),
    or None where the loader ends in its `except:` and returns the originals.

    own_extent / other_extent: (min row, max row, min col, max col) of channel 0 of this frame's and the occluder's mask, as
    ops.mask_extent gives them; an empty mask (max < min) -> None (`np.min` of an empty array raises, before any draw).
    The patch is the occluder's extent rectangle.  What the loader then does: a patch that starts above row 0 loses its first
    rows, one that ends below row H its last ones (:315-324) -- and the same two trims are applied for x, but BOTH slice ROWS of
    the patch again (columns are never trimmed) and the x-limit is H (`image.shape[0]`), not W (:325-334).  Negative slice
    lengths mean what Python slicing means: the rows are tracked as a `range` sliced the way the loader slices its arrays.
    The target rectangle is image[start_y:end_y, start_x:end_x] as numpy clips it.  The paste happens iff the patch broadcasts
    to the target: per axis equal, or a patch axis of 1, which repeats (rep_y / rep_x).  Anything else raises in the loader
    (:336); so does an occluder colour image with other than 3 channels (:338, after the draws)."""
    ymin, ymax, xmin, xmax = (int(v) for v in own_extent)
    oy0, oy1, ox0, ox1 = (int(v) for v in other_extent)
    if ymax < ymin or xmax < xmin or oy1 < oy0 or ox1 < ox0:
        return None
    start_y, start_x = int(start_y), int(start_x)
    oh, ow = oy1 - oy0 + 1, ox1 - ox0 + 1
    rows = range(oh)                                   # the rows of the patch that are left
    end_y, end_x = start_y + oh, start_x + ow
    if start_y < 0:
        rows, start_y = rows[-start_y:], 0
    if end_y > H:
        end_y = H
        rows = rows[:end_y - start_y]
    if start_x < 0:
        rows, start_x = rows[-start_x:], 0             # :326-328 slice axis 0
    if end_x > H:                                      # :330 compares with image.shape[0]
        end_x = H
        rows = rows[:end_x - start_x]                  # :332-334 slice axis 0
    ty, tx = range(H)[start_y:end_y], range(W)[start_x:end_x]
    ph, pw, th, tw = len(rows), ow, len(ty), len(tx)
    if not ((ph == th or ph == 1) and (pw == tw or pw == 1)) or other_channels != 3:
        return None
    row = np.zeros(ops.PASTE_PLAN_INTS, np.int32)
    row[0] = 1
    row[2], row[3], row[4], row[5] = oy0 + (rows[0] if ph else 0), ox0, ph, pw
    row[6], row[7], row[8], row[9] = (ty[0] if th else 0), (tx[0] if tw else 0), th, tw
    row[10], row[11] = int(ph == 1 and th != 1), int(pw == 1 and tw != 1)
    return row


def lm_other_index(dict_index_objs, obj):
    """`get_other_idx` (LM/dataloader_train_LM.py:286-291): a frame index outside the block [start, stop) of `obj`, drawn
    with random.choice.  The loader builds the list of all other indices; indexing a `range` of the same length draws the same
    number from Python's generator, and the position maps to the same index."""
    start, stop = dict_index_objs[obj][0], dict_index_objs[obj][1]
    length_all = dict_index_objs[15][1]
    k = random.choice(range(start + max(length_all - stop, 0)))
    return k if k < start else stop + (k - start)


class LoaderDraw(object):
    """The random draws of the training loaders, made on the loaders' own generators with the loaders' own calls
    (dataloader_train_YCBV.py:127,162-164,172,195-198; LM/dataloader_train_LM.py:311,313,180-182,186,205-208).
    CropBuilder.build_train / build_train_lm take any object with these methods, so a test can replay recorded draws."""

    def paste(self, lo_y, hi_y, lo_x, hi_x):
        start_y = int(np.random.randint(lo_y, hi_y))
        return start_y, int(np.random.randint(lo_x, hi_x))

    def pick(self, k):
        return int(np.random.randint(0, k))

    def angles(self):
        return [np.random.uniform(-math.pi / 36.0, math.pi / 36.0) for _ in range(3)]

    def jitter(self):
        return [random.uniform(-0.03, 0.03) for _ in range(3)]

    def choice(self, m, n):
        # choice(m, n, replace=False) through the library's walk on the same generator state (ops.legacy_choice_heads)
        return ops.legacy_choice_heads([int(m)], n)[0] if m > n else np.random.choice(m, n)


def _upload(a, dev):
    """small host array -> device WITHOUT stalling the host: through pinned memory (torch's caching host allocator hands the
    block out again only after the copy has run) and a non-blocking copy.  A pageable .to(dev) is stream-ordered AND blocks
    the host: in the middle of build() it waited for the crop kernel, at its start for the previous frame's forward."""
    t = torch.from_numpy(np.ascontiguousarray(a)) if not torch.is_tensor(a) else a
    return t.pin_memory().to(dev, non_blocking=True)


MARKS = None          # tools/builder_trace.py sets a list: (label, perf_counter) host marks of build()


def _mark(label):
    if MARKS is not None:
        MARKS.append((label, time.perf_counter()))


class CropBuilder(object):
    def __init__(self, cfg, cad_points_mm, cad_colors, camera=YCBV_CAMERA, device="cuda", capacity=False, v2p_pitch=33,
                 template_ids=False, draws="host", draw_seed=0):
        """cfg: mapping with input_size, tmp_size, unit_voxel_extent, voxel_num_limit, voxelization_mode (the `test`
        block of configs/config_YCBV_bs32.yaml).  cad_points_mm / cad_colors: {class id: (tmp_size,3) float64}, the
        loader's list_pc_CAD / list_rgb_CAD (millimetres; colours already mean-subtracted, :57-58).
        capacity=True: the observed side's voxelisation stays in CAPACITY form -- occupied_voxels (b*n, 4) and v2p_maps
        (b*n, v2p_pitch) with the live row count on the device (data["inp"]["v0_dev"]) -- so build() makes ONE host
        read-back per frame (the per-instance point counts the loader's random draws need) instead of two; Network.forward
        takes that form on its graph path (exact_form(data) converts, with the read-back).  v2p_pitch: 1 + the most points of
        a crop one voxel may hold.  Exact mode repeats an image whose crops exceed it with the general op; in capacity mode
        the device-side flag data["inp"]["vi_info"][2] says so (the caller reads it with its results; exact_form raises).
        template_ids=True: the eval builders name the template side instead of building it -- build() emits data["tmp_cls"], a
        device tensor of the crops' class ids, and no data["tmp"]; build_lm / build_lmo return that one-element tensor and None
        in place of (feat_tmp, voxel_tmp).  For a Network with a per-class template cache: net.cache_templates(builder.templates(),
        voxel_num_limit) once, then every such call runs no template-side work (models/DCL_Net.py).  The training builders
        (build_train, build_train_lm) do not read it.
        draws="host" (default): the loader's np.random.choice draws on the host, bit for bit, behind the read-back of the point
        counts.  draws="device": the eval builders (build, build_lm, build_lmo) draw on the GPU with ops.crop_draw from
        (draw_seed, self.draw_frame, instance row) and never read the counts back.  draw_frame starts at 0, goes up by one per
        built frame / sample and may be read and set: the same (draw_seed, draw_frame) gives the same crops bit for bit, and a
        CropPrefetcher (one thread, in order) makes the serial loop's draws.  These are NOT the loader's draws and consume
        nothing of np.random.  The batch of build() is then EVERY candidate (an instance with an empty mask stays, as a lattice
        dummy crop: ops.crop_sample_valid) and data["valid"] (b,) i32 on the device marks the real ones; build_lm / build_lmo
        never return None and return `valid` (1,) as a sixth element.  Labels and centroid of a crop that is not valid are
        unspecified: consumers mask by `valid`, read together with their results.  Zero host synchronisations per frame needs
        capacity=True (the exact form keeps its {V, maxActive} read-back).  The training builders do not read the switch."""
        if draws not in ("host", "device"):
            raise ValueError("CropBuilder: draws must be 'host' or 'device', got %r" % (draws,))
        self.draws, self.draw_seed, self.draw_frame = draws, int(draw_seed), 0
        if draws == "device" and not 1 <= int(cfg["input_size"]) <= min(ops.CROP_DRAW_MAX_POINTS, int(cfg["voxel_num_limit"][0]) ** 3):
            raise ValueError("CropBuilder(draws='device'): input_size must be 1 .. %d and at most voxel_num_limit^3"
                             % ops.CROP_DRAW_MAX_POINTS)
        self.capacity, self.v2p_pitch = bool(capacity), int(v2p_pitch)
        self.template_ids = bool(template_ids)
        self.n_inp, self.n_tmp = int(cfg["input_size"]), int(cfg["tmp_size"])
        self.unit = np.array(cfg["unit_voxel_extent"]).astype(float)
        self.limit = np.array(cfg["voxel_num_limit"]).astype(float)
        self.extent = self.limit * self.unit
        self.mode = int(cfg["voxelization_mode"])
        self.camera = tuple(camera)
        self.dev = torch.device(device)
        if self.dev.type != "cuda":
            raise RuntimeError("dcl-net_amd.CropBuilder runs on the GPU only")
        # template side (:179-183): constant per class -> feats rows and voxel coordinates once, on the device
        self.cls_ids = sorted(cad_points_mm.keys())
        self.cls_row = {c: i for i, c in enumerate(self.cls_ids)}
        pts = torch.stack([torch.FloatTensor(np.asarray(cad_points_mm[c]) / 1000.0) for c in self.cls_ids]).to(self.dev)
        col = torch.stack([torch.FloatTensor(np.asarray(cad_colors[c])) for c in self.cls_ids]).to(self.dev)
        assert pts.shape[1] == self.n_tmp
        feats, coords = ops.crop_sample(pts.contiguous(), col.contiguous(), None, None, self.extent[0] * 0.5, self.unit,
                                        int(self.limit[0]))
        self.tmp_feats = feats.view(len(self.cls_ids), self.n_tmp, 7)
        self.tmp_vox = coords.view(len(self.cls_ids), self.n_tmp, 4)[:, :, 1:].contiguous()
        self._cad_mm, self._radius_tab = cad_points_mm, None      # build_train's per-class radius table, made on first use
        self.draw_seconds = 0.0                  # host time spent in the loader's np.random.choice draws (accumulated)
        # The template side of a batch is a function of the crops' CLASSES alone (:179-183,223): voxelise every class once
        # (device voxelize_idx, crop id 0) and keep the three maps on the host; a frame's maps are those tables put side by
        # side with the crop ids / row offsets applied (_template_side) -- no kernel and no read-back per frame.
        S = int(self.limit[0])
        self._tmp_tab, self._tmp_side_cache = [], {}
        zero = torch.zeros((self.n_tmp, 1), dtype=torch.int64, device=self.dev)
        for r in range(len(self.cls_ids)):
            occ, p2v, v2p = ops.voxelize_idx_gpu(torch.cat([zero, self.tmp_vox[r]], 1).contiguous(), 1, S, self.mode)
            v2p = v2p.cpu().numpy()
            ids = (np.arange(v2p.shape[1])[None, :] >= 1) & (np.arange(v2p.shape[1])[None, :] <= v2p[:, :1])
            self._tmp_tab.append((occ.cpu().numpy(), p2v.cpu().numpy(), v2p, ids))

    def templates(self):
        """{class id: one-crop data["tmp"]} of every class the builder holds -- feats (n_tmp, 7) on the device, occupied_voxels
        (v, 4) and v2p_maps (v, ma + 1) of crop index 0 from the per-class tables: the dict Network.cache_templates takes"""
        out = {}
        for c, r in self.cls_row.items():
            occ, _, v2p, _ = self._tmp_tab[r]
            out[int(c)] = {"feats": self.tmp_feats[r], "occupied_voxels": torch.from_numpy(occ), "v2p_maps": torch.from_numpy(v2p)}
        return out

    def _template_side(self, rows):
        """occupied_voxels / p2v_maps / v2p_maps of the template clouds of the classes `rows` (one per crop), exactly what
        voxelize_idx returns for the batch's (b * n_tmp, 4) coordinate rows (first-encounter voxel ids crop by crop, point
        ids offset by the crop's first point, maxActive = the batch's maximum).  Assembled on the host from the per-class
        tables and cached per class tuple (the objects of a video sequence repeat frame after frame)."""
        key = tuple(int(r) for r in rows)
        hit = self._tmp_side_cache.get(key)
        if hit is not None:
            # the entry was made on whatever stream built it first (pageable uploads + a cat kernel); a hit from another
            # stream or thread orders itself behind that work.  The tensors are shared by every frame with this class tuple:
            # READ-ONLY for consumers.
            torch.cuda.current_stream(self.dev).wait_event(hit[1])
            return hit[0]
        tabs = [self._tmp_tab[r] for r in key]
        ma = max(t[2].shape[1] for t in tabs) - 1
        occ, p2v, v2p, voff = [], [], [], 0
        for j, (o, p, v, ids) in enumerate(tabs):
            oj = o.copy()
            oj[:, 0] = j
            occ.append(oj)
            p2v.append(p + voff)
            vj = np.zeros((v.shape[0], ma + 1), np.int32)
            vj[:, :v.shape[1]] = v + (j * self.n_tmp) * ids
            v2p.append(vj)
            voff += o.shape[0]
        out = tuple(torch.from_numpy(np.ascontiguousarray(np.concatenate(a, 0))).to(self.dev) for a in (occ, p2v, v2p))
        b = len(key)
        ids = torch.arange(b, device=self.dev).view(b, 1, 1).expand(b, self.n_tmp, 1)
        rows_t = torch.tensor(key, device=self.dev)
        out = out + (torch.cat([ids, self.tmp_vox[rows_t]], 2).reshape(b * self.n_tmp, 4).contiguous(),)   # voxelize_idx's input rows
        if len(self._tmp_side_cache) >= 64:
            self._tmp_side_cache.pop(next(iter(self._tmp_side_cache)))
        ready = torch.cuda.Event()
        ready.record(torch.cuda.current_stream(self.dev))
        self._tmp_side_cache[key] = (out, ready)
        return out

    @staticmethod
    def resident(img, depth, label, device="cuda"):
        """upload one frame's arrays in the layout build() wants (u8 colour, depth as 16-bit storage, i32 labels): a caller
        that decodes frames ahead of the network keeps them in HBM and passes these tensors instead of numpy arrays"""
        dev = torch.device(device)
        return (torch.from_numpy(np.ascontiguousarray(img)).to(dev),
                torch.from_numpy(np.ascontiguousarray(depth).astype(np.uint16).view(np.int16)).to(dev),
                torch.from_numpy(np.ascontiguousarray(label).astype(np.int32)).to(dev))

    def build(self, img, depth, label, rois, gt_obj, poses=None):
        """img (H,W,3|4) u8, depth (H,W) u16, label (H,W) integer, rois (k,>=6), gt_obj (n) class ids, poses (3,4,n) or
        None -- numpy arrays as the loader reads them, or the CUDA tensors of CropBuilder.resident().  Returns the loader's
        dict with CUDA tensors (instances without a detection or with an empty mask are dropped and flagged 0 in
        `all_flags`, :116,134).  Host synchronisations per frame: the per-instance point counts (the sampling draws are the
        loader's own np.random.choice calls) and {V, maxActive} of the observed side's voxelisation; nothing else.
        draws="device" (see __init__): no read-back of the counts -- crop_points, crop_draw, crop_sample_valid, the voxelisation.
        The batch is every candidate (b = the instances with a detection; `all_flags` marks them), data["valid"] (b,) i32,
        data["counts"] (b,3) i32 and data["picks"] (b, input_size) i64 stay on the device.  "every object mask of this image is
        empty" cannot be raised in this form (it would need the counts): such a frame is a batch of dummy crops with valid = 0."""
        _mark("start")
        H, W = depth.shape
        gt_obj = np.asarray(gt_obj).astype(np.int32)
        rois = np.asarray(rois)
        cand, boxes = [], []
        for i, cls in enumerate(gt_obj):
            hit = np.where(rois[:, 1] == cls)[0]
            if hit.size:
                r0, r1, c0, c1 = snap_box(rois, hit[0], H, W)
                cand.append(i)
                boxes.append((max(r0, 0), min(r1, H), max(c0, 0), min(c1, W)))      # numpy slice clipping (:132)
        dev = self.dev
        flags = np.zeros(len(gt_obj), np.int8)
        if not cand:
            raise ValueError("no object instance of this image has a detection")
        if torch.is_tensor(depth):
            i_t, d_t, l_t = img, depth, label                                       # resident frame (CropBuilder.resident)
        else:
            i_t, d_t, l_t = self.resident(img, depth, label, dev)
        bo = np.concatenate([np.asarray(boxes, np.int32), gt_obj[cand][:, None]], 1)   # boxes + class ids: one upload
        bo_t = _upload(bo, dev)
        b_t, o_t = bo_t[:, :4].contiguous(), bo_t[:, 4].contiguous()
        cap = max(1, max(max(r1 - r0, 0) * max(c1 - c0, 0) for r0, r1, c0, c1 in boxes))
        xyz, col, centroid, counts = ops.crop_points(d_t, l_t, i_t, b_t, o_t, self.camera, RGB_MEAN, self.extent * 0.5,
                                                     MIN_VALID, cap=cap)
        _mark("crop_points issued")
        # What does not depend on the instances' point counts is issued NOW, while the GPU runs k_crop_points (~0.17 ms) and
        # before the host waits for the counts: the template side (class rows, feats, voxel tables), the gt labels (the
        # centroids are read on the device, in stream order) and the dict's host tensors -- for ALL candidates; the rare image
        # that then drops an instance (an empty mask) redoes this part for the kept ones.
        def count_free_part(keep):
            rows = [self.cls_row[int(gt_obj[cand[k]])] for k in keep]
            if self.template_ids:                   # the template side by name: the candidates' class ids are on the device already
                part = {"rows": rows, "labels": {},
                        "tmp_cls": o_t if len(keep) == len(cand) else o_t[_upload(np.asarray(keep, np.int64), dev)].contiguous()}
            else:
                cls_rows = _upload(np.asarray(rows, np.int64), dev)
                part = {"rows": rows, "feats_tmp": self.tmp_feats[cls_rows].reshape(len(keep) * self.n_tmp, 7),
                        "tmp_side": self._template_side(rows), "labels": {}}
            cen = centroid if len(keep) == len(cand) else centroid[_upload(np.asarray(keep, np.int64), dev)]
            if poses is not None:
                # rot_gt = poses[:, 0:3], trans_gt = poses[:, 3] - centroid (:226-240: float64 difference, rounded to float32
                # once) -- formed on the device from one small upload, so the centroids never come back to the host
                P = _upload(np.asarray(poses, np.float64)[:, :, [cand[k] for k in keep]], dev)
                part["labels"] = {"rot_gt": P[:, 0:3, :].permute(2, 0, 1).float().contiguous(),
                                  "trans_gt": (P[:, 3, :].t() - cen.double()).float().contiguous()}
            part["centroid"] = cen
            part["host"] = {"batch_offsets": (torch.arange(len(keep) + 1) * 1024).int(), "voxel_num_limit": torch.tensor(self.limit),
                            "obj_idx": torch.IntTensor(gt_obj - 1), "flags": torch.IntTensor([-1])}
            return part
        part = count_free_part(list(range(len(cand))))
        _mark("count-free part issued")
        if self.draws == "device":
            frame, self.draw_frame = self.draw_frame, self.draw_frame + 1
            picks, valid = ops.crop_draw(counts, self.n_inp, self.draw_seed, frame, MIN_VALID, keep_sparse=True)   # :134,163
            feats_inp, coords_inp = ops.crop_sample_valid(xyz, col, picks, counts, valid, self.extent[0] * 0.5, self.unit,
                                                          int(self.limit[0]), min_valid=MIN_VALID)
            flags[cand] = 1
            b = len(cand)
            data = dict(part["host"], all_flags=torch.IntTensor(flags), all_centroids=part["centroid"], labels=part["labels"],
                        counts=counts, valid=valid, picks=picks)
            _mark("draw + sample + labels issued")
            data["inp"] = self._inp_side(feats_inp, coords_inp, b)
            _mark("voxelisation issued")
            if self.template_ids:
                data["tmp_cls"] = part["tmp_cls"]
            else:
                occ, p2v, v2p, coords_tmp = part["tmp_side"]
                data["tmp"] = {"feats": part["feats_tmp"], "coords": coords_tmp, "occupied_voxels": occ, "p2v_maps": p2v,
                               "v2p_maps": v2p}
            data["ready_event"] = torch.cuda.Event()
            data["ready_event"].record(torch.cuda.current_stream(dev))
            _mark("end")
            return data
        cnt = counts.cpu().numpy()                                                  # the builder's host read-back
        _mark("counts read back")
        keep = [k for k in range(len(cand)) if cnt[k, 0] > 0]
        if not keep:
            raise ValueError("every object mask of this image is empty")
        picks = []
        t_draw = time.perf_counter()
        # :166-169, the loader's RNG calls, in the loader's order on the global legacy generator: choice(m, n, replace=False) --
        # numpy shuffles all m masked points for it, 14.5 ns each -- runs of such objects go through ops.legacy_choice_heads (the
        # same walk on the same generator state, bit for bit, ~3x faster: 0.44 -> 0.14 ms per 6-object frame); the rare
        # choice(m, n) WITH replacement (m <= n points) stays numpy's.  A seeded run consumes the stream like the original.
        run = []
        def flush():
            if run:
                picks.extend(ops.legacy_choice_heads([int(cnt[k, 2]) for k in run], self.n_inp))
                del run[:]
        for k in keep:
            m = int(cnt[k, 2])
            if m > self.n_inp:
                run.append(k)
            else:
                flush()
                picks.append(np.random.choice(m, self.n_inp))
            flags[cand[k]] = 1
        flush()
        self.draw_seconds += time.perf_counter() - t_draw
        _mark("draws done")
        if len(keep) != len(cand):
            kt = _upload(np.asarray(keep, np.int64), dev)
            xyz, col, counts = xyz[kt].contiguous(), col[kt].contiguous(), counts[kt].contiguous()
            part = count_free_part(keep)
        pick_t = _upload(np.stack(picks).astype(np.int64), dev)
        feats_inp, coords_inp = ops.crop_sample(xyz, col, pick_t, counts, self.extent[0] * 0.5, self.unit,
                                                int(self.limit[0]), min_valid=MIN_VALID)
        b = len(keep)
        data = dict(part["host"], all_flags=torch.IntTensor(flags), all_centroids=part["centroid"], labels=part["labels"],
                    counts=cnt[keep])
        _mark("sample + labels issued")
        data["inp"] = self._inp_side(feats_inp, coords_inp, b)
        _mark("voxelisation issued")
        if self.template_ids:
            data["tmp_cls"] = part["tmp_cls"]
        else:
            occ, p2v, v2p, coords_tmp = part["tmp_side"]                            # tables: no kernel, no read-back
            data["tmp"] = {"feats": part["feats_tmp"], "coords": coords_tmp, "occupied_voxels": occ, "p2v_maps": p2v,
                           "v2p_maps": v2p}
        # a Network(async_inputs=True) lets its side streams wait for exactly this point instead of the whole stream
        data["ready_event"] = torch.cuda.Event()
        data["ready_event"].record(torch.cuda.current_stream(dev))
        _mark("end")
        return data

    # ------------------------------------------------------------------------------ several frames per call
    def _pad_rows(self, n_live, pad_to):
        """rows of a batch of n_live crops padded to the next multiple of pad_to (None: no padding)"""
        if pad_to is None:
            return n_live
        if self.draws != "device":
            raise ValueError("pad_to needs CropBuilder(draws='device'): the host form has no `valid` to mark padding rows with")
        k = int(pad_to)
        if k < 1:
            raise ValueError("pad_to must be a positive integer, got %r" % (pad_to,))
        return -(-n_live // k) * k

    def _check_capacity_rows(self, rows, what):
        if self.capacity and rows > ops.VI_CROPS_MAX_BATCH:
            raise ValueError("%s: %d crops in one call, the capacity form holds at most %d (ops.VI_CROPS_MAX_BATCH): pass fewer "
                             "frames per call" % (what, rows, ops.VI_CROPS_MAX_BATCH))

    def _device_rows(self, stack, src_t, fidx, cap, keys, rows, min_valid, always_filter, keep_sparse, clamp_sparse):
        """crop_points_frames -> crop_draw_keyed -> crop_sample_valid for the n live crops of src_t, in groups of instances whose
        four (n, cap, 3) float buffers stay under FRAMES_SCRATCH_BYTES; the last group carries the rows - n padding rows (valid -1,
        lattice rows, counts / picks / centroid zero).  Nothing is read back.  -> feats, coords, centroid, counts, picks, valid"""
        i_t, d_t, l_t = stack                                                      # _stack_frames' order
        n = src_t.shape[0]
        per = max(1, int(self.FRAMES_SCRATCH_BYTES // (48 * cap)))
        out = []
        for g0 in range(0, n, per):
            g1 = min(n, g0 + per)
            g_rows = g1 - g0 + (rows - n if g1 == n else 0)
            xyz, col, cen, cnt = ops.crop_points_frames(d_t, l_t, i_t, fidx[g0:g1], src_t[g0:g1], self.camera, RGB_MEAN,
                                                        self.extent * 0.5, min_valid, always_filter=always_filter, cap=cap, rows=g_rows)
            picks, valid = ops.crop_draw_keyed(cnt, self.n_inp, self.draw_seed, keys[g0:g1], min_valid, keep_sparse=keep_sparse,
                                               rows=g_rows)
            feats, coords = ops.crop_sample_valid(xyz, col, picks, cnt if clamp_sparse else None, valid, self.extent[0] * 0.5,
                                                  self.unit, int(self.limit[0]), min_valid=min_valid)
            if g0:
                coords[:, 0] += g0                                                 # the crop column: the group's first row
            out.append((feats, coords, cen, cnt, picks, valid))
        if len(out) == 1:
            return out[0]
        return tuple(torch.cat([o[k] for o in out]) for k in range(6))

    FRAMES_SCRATCH_BYTES = 512 << 20      # budget of crop_points_frames' four (n, cap, 3) float buffers per group of instances

    def build_frames(self, frames, pad_to=None):
        """build() for SEVERAL frames in one call: frames = [(img, depth, label, rois, gt_obj[, poses]), ...] -- numpy arrays or
        resident() tensors, one channel count, poses for every frame or for none.  Returns the dict build() would return for the
        crops of all frames, in frame order and then instance order: every per-crop tensor (inp feats / coords with the crop
        column counting through the batch, labels, all_centroids, tmp / tmp_cls; counts, picks, valid in the device form) is bit
        for bit the concatenation of the per-frame build() results, obj_idx and all_flags are the per-frame tensors
        concatenated, and the observed side is voxelised in ONE call over all crops.  New keys: frame_offsets (F+1) i32 host,
        the crop rows of each frame; frame_objects (F+1) i32 host, each frame's range of obj_idx / all_flags; n_live, the
        number of rows that are not padding.  Frames of different sizes are stacked as _stack_frames stacks them (depth 0,
        label -1 outside a frame); every frame's boxes are clipped to its own size.
        draws="device": frame f draws with the key (draw_frame + f, instance row inside its frame) -- the crops of F serial
        build() calls -- and draw_frame advances by F; with capacity=True nothing is read back.
        draws="host": ONE read-back of all counts; the loader's np.random calls are made frame by frame in the order of serial
        build() calls and leave the generator in the same state; instances with an empty mask are dropped.
        pad_to=k (device draws only): the batch is extended to the next multiple of k with PADDING rows -- valid == -1 ("not a
        crop": the metric kernels skip such a row, include/dclnet_hip.h), the lattice dummy crop of the row's own crop index,
        counts and picks zero, rot_gt = I, trans_gt = 0, centroid 0, the class of the first live crop (so that a template cache
        is not missed and template_ids=False has a real template side).  The live rows are those of the unpadded call, so one
        captured graph per multiple of k serves a run whose crop count changes from call to call.
        ValueError: an empty list, a frame without a detected instance (before any device work, with its index), mixed channel
        counts, more than ops.VI_CROPS_MAX_BATCH crops with capacity=True (never a silent fall-back); host form: a frame whose
        masks are all empty (with its index)."""
        _mark("start")
        F = len(frames)
        if F == 0:
            raise ValueError("build_frames: at least one frame")
        dev = self.dev
        chans = set(int(fr[0].shape[2]) for fr in frames)
        if len(chans) != 1:
            raise ValueError("build_frames: every frame has the same number of colour channels, got %s" % sorted(chans))
        with_poses = [len(fr) > 5 and fr[5] is not None for fr in frames]
        if any(with_poses) != all(with_poses):
            raise ValueError("build_frames: poses for every frame or for none")
        src, cls_of, pose_cols, flags, objs, cand_of = [], [], [], [], [], []
        frame_offsets, frame_objects = [0], [0]
        for f, fr in enumerate(frames):
            H, W = fr[1].shape
            rois, gt_obj = np.asarray(fr[3]), np.asarray(fr[4]).astype(np.int32)
            cand = []
            for i, cls in enumerate(gt_obj):
                hit = np.where(rois[:, 1] == cls)[0]
                if hit.size:
                    r0, r1, c0, c1 = snap_box(rois, hit[0], H, W)
                    cand.append(i)
                    src.append((max(r0, 0), min(r1, H), max(c0, 0), min(c1, W), int(cls), f))   # numpy slice clipping (:132)
            if not cand:
                raise ValueError("build_frames: no object instance of frame %d has a detection" % f)
            if with_poses[f]:
                pose_cols.append(np.asarray(fr[5], np.float64)[:, :, cand])
            cand_of.append(cand)
            flags.append(np.zeros(len(gt_obj), np.int8))
            objs.append(gt_obj)
            frame_offsets.append(len(src))
            frame_objects.append(frame_objects[-1] + len(gt_obj))
        n_live = len(src)
        rows_total = self._pad_rows(n_live, pad_to)
        self._check_capacity_rows(rows_total, "build_frames")
        src_a = np.asarray(src, np.int32)
        stack = self._stack_frames([fr[:3] for fr in frames])
        cap = max(1, int(((src_a[:, 1] - src_a[:, 0]).clip(0) * (src_a[:, 3] - src_a[:, 2]).clip(0)).max()))
        host = {"voxel_num_limit": torch.tensor(self.limit), "obj_idx": torch.IntTensor(np.concatenate(objs) - 1),
                "flags": torch.IntTensor([-1]), "frame_objects": torch.IntTensor(frame_objects)}

        def count_free_part(keep, rows, centroid):
            """what does not depend on the point counts, for the live crops `keep` (indices into src) and rows - len(keep)
            padding rows behind them (as in build(): issued while the crop kernels run)"""
            pad = rows - len(keep)
            cls = [int(src_a[k, 4]) for k in keep] + [int(src_a[keep[0], 4])] * pad
            trows = [self.cls_row[c] for c in cls]
            part = {"labels": {}}
            if self.template_ids:
                part["tmp_cls"] = _upload(np.asarray(cls, np.int32), dev)
            else:
                cls_rows = _upload(np.asarray(trows, np.int64), dev)
                part["feats_tmp"] = self.tmp_feats[cls_rows].reshape(rows * self.n_tmp, 7)
                part["tmp_side"] = self._template_side(trows)
            if pose_cols:
                P = np.concatenate(pose_cols, 2)[:, :, keep]
                if pad:
                    P = np.concatenate([P, np.tile(np.eye(3, 4)[:, :, None], (1, 1, pad))], 2)
                P = _upload(P, dev)
                # build()'s arithmetic row by row: the float64 difference, rounded to float32 once
                part["labels"] = {"rot_gt": P[:, 0:3, :].permute(2, 0, 1).float().contiguous(),
                                  "trans_gt": (P[:, 3, :].t() - centroid.double()).float().contiguous()}
            part["batch_offsets"] = (torch.arange(rows + 1) * 1024).int()
            return part

        def finish(part, data, feats_inp, coords_inp, rows):
            data["inp"] = self._inp_side(feats_inp, coords_inp, rows)
            _mark("voxelisation issued")
            if self.template_ids:
                data["tmp_cls"] = part["tmp_cls"]
            else:
                occ, p2v, v2p, coords_tmp = part["tmp_side"]
                data["tmp"] = {"feats": part["feats_tmp"], "coords": coords_tmp, "occupied_voxels": occ, "p2v_maps": p2v,
                               "v2p_maps": v2p}
            data["ready_event"] = torch.cuda.Event()
            data["ready_event"].record(torch.cuda.current_stream(dev))
            _mark("end")
            return data

        if self.draws == "device":
            frame0, self.draw_frame = self.draw_frame, self.draw_frame + F
            keys = np.stack([frame0 + src_a[:, 5].astype(np.int64),
                             np.concatenate([np.arange(frame_offsets[f + 1] - frame_offsets[f]) for f in range(F)])], 1)
            src_t, keys_t = _upload(src_a, dev), _upload(keys.astype(np.int64), dev)
            feats_inp, coords_inp, centroid, counts, picks, valid = self._device_rows(
                stack, src_t, src_a[:, 5], cap, keys_t, rows_total, MIN_VALID, False, True, True)
            _mark("crop_points + draw + sample issued")
            part = count_free_part(list(range(n_live)), rows_total, centroid)
            for f in range(F):
                flags[f][cand_of[f]] = 1
            data = dict(host, batch_offsets=part["batch_offsets"], all_flags=torch.IntTensor(np.concatenate(flags)),
                        all_centroids=centroid, labels=part["labels"], counts=counts, valid=valid, picks=picks,
                        frame_offsets=torch.IntTensor(frame_offsets), n_live=n_live)
            return finish(part, data, feats_inp, coords_inp, rows_total)

        src_t = _upload(src_a, dev)
        xyz, col, centroid, counts = ops.crop_points_frames(stack[1], stack[2], stack[0], src_a[:, 5], src_t, self.camera, RGB_MEAN,
                                                            self.extent * 0.5, MIN_VALID, cap=cap)
        _mark("crop_points issued")
        cnt = counts.cpu().numpy()                                                  # the call's ONE host read-back
        _mark("counts read back")
        keep, kept_offsets = [], [0]
        for f in range(F):
            mine = [k for k in range(frame_offsets[f], frame_offsets[f + 1]) if cnt[k, 0] > 0]
            if not mine:
                raise ValueError("build_frames: every object mask of frame %d is empty" % f)
            keep.extend(mine)
            kept_offsets.append(len(keep))
        picks = []
        t_draw = time.perf_counter()
        for f in range(F):                        # the loader's draws, frame by frame as serial build() calls make them
            run = []

            def flush():
                if run:
                    picks.extend(ops.legacy_choice_heads([int(cnt[k, 2]) for k in run], self.n_inp))
                    del run[:]
            for k in keep[kept_offsets[f]:kept_offsets[f + 1]]:
                m = int(cnt[k, 2])
                if m > self.n_inp:
                    run.append(k)
                else:
                    flush()
                    picks.append(np.random.choice(m, self.n_inp))
                flags[f][cand_of[f][k - frame_offsets[f]]] = 1
            flush()
        self.draw_seconds += time.perf_counter() - t_draw
        _mark("draws done")
        if len(keep) != n_live:
            kt = _upload(np.asarray(keep, np.int64), dev)
            xyz, col, counts, centroid = xyz[kt].contiguous(), col[kt].contiguous(), counts[kt].contiguous(), centroid[kt]
        part = count_free_part(keep, len(keep), centroid)
        pick_t = _upload(np.stack(picks).astype(np.int64), dev)
        feats_inp, coords_inp = ops.crop_sample(xyz, col, pick_t, counts, self.extent[0] * 0.5, self.unit, int(self.limit[0]),
                                                min_valid=MIN_VALID)
        data = dict(host, batch_offsets=part["batch_offsets"], all_flags=torch.IntTensor(np.concatenate(flags)),
                    all_centroids=centroid, labels=part["labels"], counts=cnt[keep], frame_offsets=torch.IntTensor(kept_offsets),
                    n_live=len(keep))
        _mark("sample + labels issued")
        return finish(part, data, feats_inp, coords_inp, len(keep))

    def _stack_frames(self, frames):
        """frames -> (rgb (f,H,W,C) u8, depth (f,H,W) 16-bit storage, label (f,H,W) i32) on the device.  Frames of different
        sizes are padded at the bottom and the right to the largest one with depth 0 and label -1 (a label outside every
        class range takes no part anywhere; pixel coordinates do not move)."""
        dev = self.dev
        if torch.is_tensor(frames[0][1]):
            Hm, Wm = max(f[1].shape[0] for f in frames), max(f[1].shape[1] for f in frames)

            def pad(t, value, tail=0):
                h, w = t.shape[0], t.shape[1]
                if (h, w) == (Hm, Wm):
                    return t
                return torch.nn.functional.pad(t, (0, 0) * tail + (0, Wm - w, 0, Hm - h), value=value)
            return (torch.stack([pad(f[0], 0, 1) for f in frames]), torch.stack([pad(f[1], 0) for f in frames]),
                    torch.stack([pad(f[2], -1) for f in frames]))
        Hm, Wm = max(f[1].shape[0] for f in frames), max(f[1].shape[1] for f in frames)
        ch = frames[0][0].shape[2]
        img = np.zeros((len(frames), Hm, Wm, ch), np.uint8)
        dep = np.zeros((len(frames), Hm, Wm), np.uint16)
        lab = np.full((len(frames), Hm, Wm), -1, np.int32)
        for k, (i, d, l) in enumerate(frames):
            h, w = d.shape
            img[k, :h, :w], dep[k, :h, :w], lab[k, :h, :w] = i, d, l
        return (torch.from_numpy(img).to(dev), torch.from_numpy(dep.view(np.int16)).to(dev), torch.from_numpy(lab).to(dev))

    def _radius(self, cls):
        """`radius_obj` (dataloader_train_YCBV.py:77-80): np.linalg.norm(cad / 1000, axis=1).max() per class, made on first use"""
        if self._radius_tab is None:
            self._radius_tab = {c: np.linalg.norm(np.asarray(p) / 1000.0, axis=1).max() for c, p in self._cad_mm.items()}
        return self._radius_tab[cls]

    def build_train(self, frames, metas, draw=None):
        """One TRAINING batch (`Dataset.__getitem__` in 'train' mode + `collate`, YCBV/dataloader_train_YCBV.py:105-266): one
        object per frame, the box from the mask's own extent, the cloud re-posed with the jittered ground-truth pose before the
        unconditional grid filter, the jittered pose as the labels.

        frames: a list of (img (H,W,3|4) u8, depth (H,W) u16, label (H,W) integer) numpy triples, or of resident() tensors.
        metas:  per frame a mapping with `cls_indexes` (k class ids), `poses` (3,4,k), `factor_depth` and `camera`
                (cx, cy, fx, fy: YCBV_TRAIN_CAMERA_1 / _2) -- the frame's meta.mat plus the loader's camera choice.
        draw:   the source of every random number: pick(k), angles(), jitter(), choice(m, n).  Default LoaderDraw(): the loader's
                calls on np.random and random.

        ORDER OF THE DRAWS.  Frame by frame: pick() until the picked object has more than 50 valid pixels (:126-132), then --
        unless the crop is the dummy of :139 -- angles() and jitter().  When every frame has had these, frame by frame again:
        choice(m, input_size) for every frame that survived.  For one frame this is exactly `__getitem__`'s order on both
        generators; for b > 1 the choice draws of all frames come after the pick / angle draws of all frames (np.random is shared
        by pick, angles and choice, so a seeded batch differs from b seeded `__getitem__` calls in the choice draws; a test
        that wants sample-for-sample equality replays recorded draws).  This order is what keeps a batch at two read-backs: the
        picks need the label table, the choices need the point counts, nothing else comes back.

        Host synchronisations per batch: (1) the label table, which feeds the pick loop and the boxes, (2) `counts`, which
        feeds the choice draws; the exact-form builder adds build()'s {V, maxActive} read-back, the capacity-form one nothing.

        A frame is dropped, as `collate` drops the dummy sample, when the box holds fewer than 50 masked pixels (:139) or at
        most 50 points lie inside the grid after the re-pose (:191).  The box arithmetic is the loader's, with its 480 x 640
        constants whatever the frame's size.

        Returns collate's dict: inp / tmp {feats, occupied_voxels, p2v_maps, v2p_maps} (and coords) as build() returns them,
        labels {rot_gt (b,3,3), trans_gt (b,3), obj_idx (b,1) i32}, flags (b) and radius (b,1) float32 -- CUDA tensors --
        batch_offsets and voxel_num_limit (host, as build()), and beside collate's keys: kept (f) bool numpy, obj (f) the
        picked class ids, boxes (f,4), counts and centroids of the kept crops."""
        draw = LoaderDraw() if draw is None else draw
        dev = self.dev
        nf = len(frames)
        if nf == 0 or len(metas) != nf:
            raise ValueError("build_train: one meta per frame, at least one frame")
        n_cls = max(self.cls_ids) + 1
        i_t, d_t, l_t = self._stack_frames(frames)
        Hm, Wm = d_t.shape[1], d_t.shape[2]
        tab_t = ops.label_table(l_t, d_t, n_cls)
        if Hm > 480 or Wm > 640:
            # a frame larger than the loader's image: get_bbox pushes the box back inside 480 x 640, where it still covers the
            # part of the mask that lies there -- so the masked pixels of the BOX (:138) are the mask's pixels in that window
            win_t = ops.label_table(l_t[:, :480, :640].contiguous(), d_t[:, :480, :640].contiguous(), n_cls)
            both = torch.stack([tab_t, win_t]).cpu().numpy()                         # host read-back 1 of 2
            tab, win = both[0], both[1]
        else:
            tab = win = tab_t.cpu().numpy()                                           # host read-back 1 of 2
        kept = np.zeros(nf, bool)
        obj_of, boxes = np.zeros(nf, np.int32), np.zeros((nf, 4), np.int32)
        src, cams, R0s, ts, jits, augs = [], [], [], [], [], []
        for f, meta in enumerate(metas):
            obj = np.asarray(meta["cls_indexes"]).flatten().astype(np.int32)
            valid = [int(tab[f, c, 0]) if 0 <= c < n_cls else 0 for c in obj]
            if not valid or max(valid) <= TRAIN_MIN_PT:
                raise ValueError("build_train: no object of frame %d has more than %d valid pixels (the loader would draw "
                                 "for ever)" % (f, TRAIN_MIN_PT))
            while True:                                                               # :126-132
                idx = draw.pick(len(obj))
                if valid[idx] > TRAIN_MIN_PT:
                    break
            c = int(obj[idx])
            obj_of[f] = c
            r0, r1, c0, c1 = extent_box(*tab[f, c, 1:5])
            boxes[f] = (r0, r1, c0, c1)
            if win[f, c, 0] < TRAIN_MIN_PT:                                           # :139, before any further draw
                continue
            self.cls_row[c]                                                           # a class without a CAD cloud: KeyError, as :179
            a1, a2, a3 = draw.angles()                                                # :162-164
            jit = draw.jitter()                                                       # :172
            P = np.asarray(meta["poses"], np.float64)[:, :, idx]
            kept[f] = True
            src.append((max(r0, 0), min(r1, Hm), max(c0, 0), min(c1, Wm), c, f))      # numpy slice clipping (:138)
            cams.append(tuple(meta["camera"])[:4] + (float(np.asarray(meta["factor_depth"]).reshape(-1)[0]),))
            R0s.append(P[:, 0:3])
            ts.append(P[:, 3])
            jits.append(jit)
            augs.append(euler2mat(a1, a2, a3))
        cand = np.nonzero(kept)[0]
        out = {"batch_offsets": None, "voxel_num_limit": torch.tensor(self.limit), "kept": kept, "obj": obj_of, "boxes": boxes}
        if cand.size == 0:
            return dict(out, flags=torch.zeros(0, device=dev), batch_offsets=torch.zeros(1).int())
        src_a = np.asarray(src, np.int32)
        src_t, cam_t = _upload(src_a, dev), _upload(np.asarray(cams, np.float32), dev)
        pose_t = _upload(ops.pose_rows(R0s, ts, jits, augs), dev)
        cap = max(1, int(((src_a[:, 1] - src_a[:, 0]).clip(0) * (src_a[:, 3] - src_a[:, 2]).clip(0)).max()))
        xyz, col, centroid, counts, rot_gt, trans_gt = ops.crop_points_posed(
            d_t, l_t, i_t, src_a[:, 5], src_t, cam_t, pose_t, RGB_MEAN, self.extent * 0.5, TRAIN_MIN_PT, cap=cap)

        def count_free_part(keep):
            # what does not depend on the point counts, issued while the crop kernels run (as in build())
            cls = [int(obj_of[cand[k]]) for k in keep]
            rows = [self.cls_row[c] for c in cls]
            cls_rows = _upload(np.asarray(rows, np.int64), dev)
            small = np.array([[float(c - 1 in TRAIN_SYMMETRY_OBJ_IDX), self._radius(c), c - 1] for c in cls], np.float32)
            small_t = _upload(small, dev)
            return {"feats_tmp": self.tmp_feats[cls_rows].reshape(len(keep) * self.n_tmp, 7),
                    "tmp_side": self._template_side(rows), "flags": small_t[:, 0].contiguous(),
                    "radius": small_t[:, 1:2].contiguous(), "obj_idx": small_t[:, 2:3].int()}
        part = count_free_part(list(range(cand.size)))
        cnt = counts.cpu().numpy()                                                    # host read-back 2 of 2
        keep = [k for k in range(cand.size) if cnt[k, 2] > 0]                         # :191: more than 50 points inside the grid
        for k in range(cand.size):
            kept[cand[k]] = cnt[k, 2] > 0
        if not keep:
            return dict(out, flags=torch.zeros(0, device=dev), batch_offsets=torch.zeros(1).int())
        t_draw = time.perf_counter()
        picks = [np.asarray(draw.choice(int(cnt[k, 2]), self.n_inp)) for k in keep]  # :195-198
        self.draw_seconds += time.perf_counter() - t_draw
        if len(keep) != cand.size:
            kt = _upload(np.asarray(keep, np.int64), dev)
            xyz, col, centroid = xyz[kt].contiguous(), col[kt].contiguous(), centroid[kt]
            rot_gt, trans_gt = rot_gt[kt].contiguous(), trans_gt[kt].contiguous()
            part = count_free_part(keep)
        pick_t = _upload(np.stack(picks).astype(np.int64), dev)
        # no clamp: the filter was applied, every point lies inside the grid (:203)
        feats_inp, coords_inp = ops.crop_sample(xyz, col, pick_t, None, self.extent[0] * 0.5, self.unit, int(self.limit[0]))
        b = len(keep)
        out["inp"] = self._inp_side(feats_inp, coords_inp, b)
        occ, p2v, v2p, coords_tmp = part["tmp_side"]
        out["tmp"] = {"feats": part["feats_tmp"], "coords": coords_tmp, "occupied_voxels": occ, "p2v_maps": p2v, "v2p_maps": v2p}
        out["labels"] = {"rot_gt": rot_gt, "trans_gt": trans_gt, "obj_idx": part["obj_idx"]}
        out["batch_offsets"] = (torch.arange(b + 1) * self.n_inp).int()
        out["flags"], out["radius"] = part["flags"], part["radius"]
        out["counts"], out["centroids"] = cnt[keep], centroid
        out["ready_event"] = torch.cuda.Event()
        out["ready_event"].record(torch.cuda.current_stream(dev))
        return out

    @staticmethod
    def resident_lm(img, depth, mask, device="cuda"):
        """upload one LineMOD training frame (or occluder frame) in the layout build_train_lm wants: u8 colour, depth as
        16-bit storage, the (H,W,3) u8 mask"""
        dev = torch.device(device)
        return (torch.from_numpy(np.ascontiguousarray(img)).to(dev),
                torch.from_numpy(np.ascontiguousarray(depth).astype(np.uint16).view(np.int16)).to(dev),
                torch.from_numpy(np.ascontiguousarray(mask).astype(np.uint8)).to(dev))

    def build_train_lm(self, samples, draw=None):
        """One LineMOD TRAINING batch (`Dataset.__getitem__` in 'train' mode, `occlude_with_another_object` and `collate`,
        LM/dataloader_train_LM.py:125-348): the object of another frame pasted over this frame's colour, depth and mask, the
        box from `obj_bb`, the cloud re-posed in FLOAT64 with the jittered ground-truth pose before the unconditional grid
        filter, the jittered pose as the labels.  The builder must have been made with camera=LM_CAMERA.

        samples: per frame a mapping with `img` (H,W,3+) u8, `depth` (H,W) u16 millimetres, `mask` (H,W,3) u8 (numpy arrays, or
                 the CUDA tensors of resident_lm), `obj` (class id), `obj_bb` [x, y, w, h], `cam_R_m2c` (9), `cam_t_m2c` (3,
                 millimetres) and `other`: None or the occluder frame's (img, depth, mask).  Which meta entry and which other
                 frame (lm_other_index) is dataset I/O: the caller's.  All frames have one size.
        draw:    paste(lo_y, hi_y, lo_x, hi_x), angles(), jitter(), choice(m, n).  Default LoaderDraw().

        ORDER OF THE DRAWS.  Frame by frame paste() -- where an occluder was given and neither mask is empty (:301-313) --;
        then, frame by frame, angles() and jitter() for every frame whose box holds a valid pixel after the paste (:157-159);
        then, frame by frame, choice(m, input_size) for every frame with more than 128 points inside the grid (:201-208).  For
        one frame this is `__getitem__`'s own order on both generators (the caller draws the other index first); for b > 1
        the three groups are batched per group: np.random is shared by all three, so a seeded batch differs from b seeded
        `__getitem__` calls (a test that wants sample-for-sample equality replays recorded draws).

        Host synchronisations per batch, and why three: (1) the mask extents and sums -- the paste draws' ranges are the
        extents; (2) the pasted frames' valid-pixel counts -- the loader draws its pose jitter only for a non-empty crop, and
        the count depends on the commit / roll-back the device decided; (3) `counts`, which feeds the choice draws.  The
        exact-form builder adds build()'s {V, maxActive} read-back.

        Returns collate's dict under its key names: inp / tmp {feats, occupied_voxels, p2v_maps, v2p_maps} (and coords), labels
        {rot_gt (b,3,3), trans_gt (b,3)}, flags (b) the symmetry flags, obj_idx (b) i32 index in LM_OBJLIST, centriods (b,3)
        (sic) -- CUDA tensors --, batch_offsets and voxel_num_limit (host); beside them kept (f) bool, occluded (f) bool (the
        composite was kept), boxes (f,4), counts of the kept crops, ready_event.  An all-dummy batch: as build_train."""
        draw = LoaderDraw() if draw is None else draw
        dev = self.dev
        nf = len(samples)
        if nf == 0:
            raise ValueError("build_train_lm: at least one frame")
        if self.camera != tuple(LM_CAMERA):
            raise ValueError("build_train_lm: the builder must be made with camera=LM_CAMERA")
        # ---- 1. stack and upload; the extents of own and occluder masks in one call
        with_other = [f for f, s in enumerate(samples) if s.get("other") is not None]
        other_of = {f: k for k, f in enumerate(with_other)}
        shape = tuple(samples[0]["depth"].shape)
        H, W = shape
        others = [samples[f]["other"] for f in with_other]
        other_ch = [int(o[0].shape[2]) for o in others]
        for s in samples:
            if tuple(s["depth"].shape) != shape or tuple(s["mask"].shape) != shape + (3,):
                raise ValueError("build_train_lm: every frame has the same size and an (H,W,3) mask")
        if torch.is_tensor(samples[0]["depth"]):
            i_t = torch.stack([s["img"] for s in samples])
            d_t = torch.stack([s["depth"] for s in samples])
            m_t = torch.stack([s["mask"] for s in samples] + [o[2] for o in others])
            zero = torch.zeros((H, W, 3), dtype=torch.uint8, device=dev)
            oi_t = torch.stack([o[0] if c == 3 else zero for o, c in zip(others, other_ch)]) if others else torch.zeros((0, H, W, 3), dtype=torch.uint8, device=dev)
            od_t = torch.stack([o[1] for o in others]) if others else torch.zeros((0, H, W), dtype=d_t.dtype, device=dev)
        else:
            i_t = torch.from_numpy(np.stack([np.asarray(s["img"], np.uint8) for s in samples])).to(dev)
            d_t = torch.from_numpy(np.stack([np.asarray(s["depth"]).astype(np.uint16) for s in samples]).view(np.int16)).to(dev)
            m_t = torch.from_numpy(np.stack([np.asarray(s["mask"], np.uint8) for s in samples] +
                                            [np.asarray(o[2], np.uint8) for o in others])).to(dev)
            oi = np.zeros((len(others), H, W, 3), np.uint8)
            od = np.zeros((len(others), H, W), np.uint16)
            for k, (o, c) in enumerate(zip(others, other_ch)):
                if c == 3:
                    oi[k] = o[0]
                od[k] = o[1]
            oi_t, od_t = torch.from_numpy(oi).to(dev), torch.from_numpy(od.view(np.int16)).to(dev)
        ext_t = ops.mask_extent(m_t)
        ext = ext_t.cpu().numpy()                                                     # host read-back 1 of 3
        # ---- 2. the paste draws and plans, the boxes
        plans = np.zeros((nf, ops.PASTE_PLAN_INTS), np.int32)
        boxes = np.zeros((nf, 4), np.int32)
        for f, s in enumerate(samples):
            r0, r1, c0, c1 = lm_box([int(v) for v in s["obj_bb"]])
            boxes[f] = (r0, r1, c0, c1)
            k = other_of.get(f)
            if k is not None:
                own, oth = ext[f, :4], ext[nf + k, :4]
                if own[1] >= own[0] and oth[1] >= oth[0]:                             # both masks non-empty (:301-306)
                    oh, ow = int(oth[1] - oth[0]) + 1, int(oth[3] - oth[2]) + 1
                    sy, sx = draw.paste(int(own[0]) - oh + 1, int(own[1]) + 1, int(own[2]) - ow + 1, int(own[3]) + 1)   # :311,313
                    row = lm_paste_plan(H, W, own, oth, sy, sx, other_ch[k])
                    if row is not None:
                        plans[f] = row
                        plans[f, 1] = k
            plans[f, 12:16] = (min(max(r0, 0), H), min(max(r1, 0), H), min(max(c0, 0), W), min(max(c1, 0), W))   # numpy slice clipping (:157)
        plan_t = _upload(plans, dev)
        w_rgb, w_dep, w_lab, info_t = ops.occlude_paste(i_t, d_t, m_t[:nf], oi_t, od_t, m_t[nf:], plans, plan_t, ext_t[:nf])
        info = info_t.cpu().numpy()                                                   # host read-back 2 of 3
        occluded = info[:, 0] != 0
        # ---- 3. the pose draws of every frame with a valid pixel in its box (:157-159,180-187)
        kept = np.zeros(nf, bool)
        src, R0s, ts, jits, augs = [], [], [], [], []
        for f, s in enumerate(samples):
            if info[f, 2] == 0:
                continue
            self.cls_row[int(s["obj"])]                                               # a class without a CAD cloud: KeyError, as :191
            a1, a2, a3 = draw.angles()                                                # :180-182
            jit = draw.jitter()                                                       # :186
            kept[f] = True
            src.append(tuple(int(v) for v in plans[f, 12:16]) + (255, f))
            R0s.append(np.resize(np.array(s["cam_R_m2c"]), (3, 3)))                   # :153
            ts.append(np.array(s["cam_t_m2c"]) / 1000.0)                              # :154
            jits.append(jit)
            augs.append(euler2mat(a1, a2, a3))
        cand = np.nonzero(kept)[0]
        out = {"batch_offsets": None, "voxel_num_limit": torch.tensor(self.limit), "kept": kept, "occluded": occluded, "boxes": boxes}
        if cand.size == 0:
            return dict(out, flags=torch.zeros(0, device=dev), batch_offsets=torch.zeros(1).int())
        src_a = np.asarray(src, np.int32)
        src_t = _upload(src_a, dev)
        cam_t = _upload(np.tile(np.asarray(self.camera, np.float32), (cand.size, 1)), dev)
        pose_t = _upload(ops.pose_rows64(R0s, ts, jits, augs), dev)
        cap = max(1, int(((src_a[:, 1] - src_a[:, 0]).clip(0) * (src_a[:, 3] - src_a[:, 2]).clip(0)).max()))
        xyz, col, centroid, counts, rot_gt, trans_gt = ops.crop_points_posed64(
            w_dep, w_lab, w_rgb, src_a[:, 5], src_t, cam_t, pose_t, RGB_MEAN, self.extent * 0.5, LM_TRAIN_MIN_PT, cap=cap)

        def count_free_part(keep):
            objs = [int(samples[cand[k]]["obj"]) for k in keep]
            rows = [self.cls_row[c] for c in objs]
            cls_rows = _upload(np.asarray(rows, np.int64), dev)
            small = np.array([[float(LM_OBJLIST.index(c) in LM_TRAIN_SYMMETRY_OBJ_IDX), LM_OBJLIST.index(c)] for c in objs], np.float32)
            small_t = _upload(small, dev)
            return {"feats_tmp": self.tmp_feats[cls_rows].reshape(len(keep) * self.n_tmp, 7),
                    "tmp_side": self._template_side(rows), "flags": small_t[:, 0].contiguous(), "obj_idx": small_t[:, 1].int()}
        part = count_free_part(list(range(cand.size)))
        cnt = counts.cpu().numpy()                                                    # host read-back 3 of 3
        keep = [k for k in range(cand.size) if cnt[k, 2] > 0]                         # :201: more than 128 points inside the grid
        for k in range(cand.size):
            kept[cand[k]] = cnt[k, 2] > 0
        if not keep:
            return dict(out, flags=torch.zeros(0, device=dev), batch_offsets=torch.zeros(1).int())
        t_draw = time.perf_counter()
        picks = [np.asarray(draw.choice(int(cnt[k, 2]), self.n_inp)) for k in keep]  # :205-208
        self.draw_seconds += time.perf_counter() - t_draw
        if len(keep) != cand.size:
            kt = _upload(np.asarray(keep, np.int64), dev)
            xyz, col, centroid = xyz[kt].contiguous(), col[kt].contiguous(), centroid[kt]
            rot_gt, trans_gt = rot_gt[kt].contiguous(), trans_gt[kt].contiguous()
            part = count_free_part(keep)
        pick_t = _upload(np.stack(picks).astype(np.int64), dev)
        # no clamp: the filter was applied, every point lies inside the grid (:202)
        feats_inp, coords_inp = ops.crop_sample(xyz, col, pick_t, None, self.extent[0] * 0.5, self.unit, int(self.limit[0]))
        b = len(keep)
        out["inp"] = self._inp_side(feats_inp, coords_inp, b)
        occ, p2v, v2p, coords_tmp = part["tmp_side"]
        out["tmp"] = {"feats": part["feats_tmp"], "coords": coords_tmp, "occupied_voxels": occ, "p2v_maps": p2v, "v2p_maps": v2p}
        out["labels"] = {"rot_gt": rot_gt, "trans_gt": trans_gt}
        out["batch_offsets"] = (torch.arange(b + 1) * self.n_inp).int()
        out["flags"], out["obj_idx"] = part["flags"], part["obj_idx"]
        out["counts"], out["centriods"] = cnt[keep], centroid
        out["ready_event"] = torch.cuda.Event()
        out["ready_event"].record(torch.cuda.current_stream(dev))
        return out

    def _inp_side(self, feats_inp, coords_inp, b):
        """the observed side of a batch of b crops from its sampled feats rows and voxelize_idx input rows: capacity form
        (no read-back) or exact form (the {V, maxActive} read-back), see __init__"""
        S = int(self.limit[0])
        if (b <= ops.VI_CROPS_MAX_BATCH and self.n_inp <= ops.VI_CROPS_MAX_POINTS and S == ops.VI_CROPS_S and
                self.mode in (3, 4)):
            # the image's crops are voxelised in ONE launch (one workgroup per crop) into capacity-shaped tensors
            occ, p2v, v2p, info = ops.voxelize_idx_crops(coords_inp, b, self.n_inp, S, self.mode, pitch=self.v2p_pitch)
            if self.capacity:
                # capacity form: nothing comes back to the host -- occupied_voxels / v2p_maps keep their b*n rows and `pitch`
                # columns, the live row count stays on the device (v0_dev; Network.forward's graph path takes it as it is)
                return {"feats": feats_inp, "coords": coords_inp, "occupied_voxels": occ, "p2v_maps": p2v, "v2p_maps": v2p,
                        "v0_dev": info[0:1], "vi_info": info}
            else:
                V, ma, err = info.cpu().tolist()                                    # the builder's second host read-back
                if err:      # a voxel with more points than the pitch holds (a tiny object sampled with replacement): general op
                    occ, p2v, v2p = ops.voxelize_idx_gpu(coords_inp, b, S, self.mode)
                    return {"feats": feats_inp, "coords": coords_inp, "occupied_voxels": occ, "p2v_maps": p2v, "v2p_maps": v2p}
                else:
                    return {"feats": feats_inp, "coords": coords_inp, "occupied_voxels": occ[:V], "p2v_maps": p2v,
                            "v2p_maps": v2p[:V, :max(ma, 1) + 1].contiguous()}
        else:
            occ, p2v, v2p = ops.voxelize_idx_gpu(coords_inp, b, S, self.mode)
            return {"feats": feats_inp, "coords": coords_inp, "occupied_voxels": occ, "p2v_maps": p2v, "v2p_maps": v2p}

    def build_lm(self, img, depth, mask_label, obj_bb=None, obj=None, eval_mode=False):
        """One LineMOD sample (`PoseDataset.__getitem__`, LM/dataloader_test_LM.py:116-214, test / eval modes): img (H,W,3+) u8,
        depth (H,W) u16 in millimetres, mask_label (H,W) bool object mask (the loader's `mask_label`), obj_bb [x,y,w,h],
        obj = class id.  obj_bb=None: the box is the loader's `mask_to_bbox(mask_label)` (:16-32,144, eval mode), computed
        on the device from the uploaded mask (ops.mask_box) -- the box row never visits the host.  The builder must have
        been made with camera=LM_CAMERA.  Returns (feat_inp (N,7), voxel_inp (N,3) i64, feat_tmp (M,7), voxel_tmp (M,3) i64,
        centroid (3,)) as CUDA tensors, or None where the loader returns its all-zero dummy sample (empty mask; in test mode
        also when at most 128 points fall inside the voxel grid).  draws="device" (see __init__): never None -- a sixth element
        `valid` (1,) i32 on the device says, by the same rule, whether the sample is real (0: a lattice dummy crop)."""
        if obj is None:
            raise TypeError("build_lm: obj (the class id) is required")
        return self._lm_sample(img, depth, mask_label, obj_bb, obj, LM_MIN_VALID, eval_mode, eval_mode)

    def build_lmo(self, img, depth, mask_label, obj):
        """One Occlusion-LineMOD sample (`Dataset.__getitem__`, LM/dataloader_test_LMO.py:197-284, eval / test modes): as
        build_lm, but the box ALWAYS comes from the mask (`get_bbox(mask_to_bbox(mask_label, padding=0))`, :215 -- the mask
        of an occluded object comes in pieces and the loader keeps the piece with the largest bounding rectangle), the
        voxel-grid filter is always applied (:261-264) and the dummy sample is returned when no masked pixel with depth lies
        inside the crop (:220-222) or no point lies inside the grid (:262,282-284) -> None.  camera=LM_CAMERA.  The pose
        labels (the LineMOD -> Occlusion alignment included) are the caller's.  draws="device": as build_lm, never None, with
        `valid` as the sixth element."""
        return self._lm_sample(img, depth, mask_label, None, obj, LMO_MIN_VALID, True, False)

    def _lm_sample(self, img, depth, mask_label, obj_bb, obj, min_valid, always_filter, keep_sparse):
        """the common body of build_lm / build_lmo.  min_valid: the sample is the dummy unless more than min_valid points lie
        inside the grid (keep_sparse: LineMOD's eval mode keeps it whatever the count)."""
        H, W = depth.shape
        dev = self.dev
        d_t = torch.from_numpy(np.ascontiguousarray(depth).astype(np.uint16).view(np.int16)).to(dev)
        l_t = torch.from_numpy(np.ascontiguousarray(mask_label).astype(np.int32)).to(dev)
        i_t = torch.from_numpy(np.ascontiguousarray(img)).to(dev)
        if obj_bb is None:
            b_t = ops.mask_box(l_t, 1, 0)[:, 4:8].contiguous()               # device tensor: no host round trip
            cap = H * W
        else:
            r0, r1, c0, c1 = lm_box(obj_bb, H, W)
            box = [max(r0, 0), min(r1, H), max(c0, 0), min(c1, W)]
            b_t = torch.tensor([box], dtype=torch.int32, device=dev)
            # (the device form knows the box on the host: crop_points need not read it back for its capacity)
            cap = max(1, max(box[1] - box[0], 0) * max(box[3] - box[2], 0)) if self.draws == "device" else None
        o_t = torch.ones(1, dtype=torch.int32, device=dev)
        xyz, col, centroid, counts = ops.crop_points(d_t, l_t, i_t, b_t, o_t, self.camera, RGB_MEAN, self.extent * 0.5,
                                                     min_valid, always_filter=always_filter, cap=cap)
        if self.draws == "device":
            frame, self.draw_frame = self.draw_frame, self.draw_frame + 1
            picks, valid = ops.crop_draw(counts, self.n_inp, self.draw_seed, frame, min_valid, keep_sparse=keep_sparse)
            feats, coords = ops.crop_sample_valid(xyz, col, picks, None, valid, self.extent[0] * 0.5, self.unit, int(self.limit[0]))
            if self.template_ids:
                return (feats, coords[:, 1:].contiguous(), torch.tensor([int(obj)], dtype=torch.int32, device=dev), None,
                        centroid[0], valid)
            row = self.cls_row[int(obj)]
            return feats, coords[:, 1:].contiguous(), self.tmp_feats[row], self.tmp_vox[row], centroid[0], valid
        n_mask, n_valid, m = counts.cpu().numpy()[0]
        if n_mask == 0 or not (n_valid > min_valid or keep_sparse):
            return None
        pick = ops.legacy_choice_heads([int(m)], self.n_inp)[0] if m > self.n_inp else np.random.choice(m, self.n_inp)
        pick_t = torch.from_numpy(pick.astype(np.int64)).view(1, -1).to(dev)
        feats, coords = ops.crop_sample(xyz, col, pick_t, None, self.extent[0] * 0.5, self.unit, int(self.limit[0]))
        row = self.cls_row[int(obj)]
        if self.template_ids:
            return feats, coords[:, 1:].contiguous(), torch.tensor([int(obj)], dtype=torch.int32, device=dev), None, centroid[0]
        return feats, coords[:, 1:].contiguous(), self.tmp_feats[row], self.tmp_vox[row], centroid[0]

    def build_lm_frames(self, samples, eval_mode=False, pad_to=None):
        """build_lm for SEVERAL samples in one call: samples = [(img, depth, mask_label, obj_bb or None, obj), ...] of one size
        and channel count, obj_bb given for every sample or for none (None: the boxes come from ONE ops.mask_box call over the
        stacked masks).  One crop per sample.  Returns a dict of build_frames' kind, not tuples: inp (feats, coords and the
        voxelisation of all crops in one call), tmp or tmp_cls, all_centroids (b,3), obj (host, the class ids), all_flags,
        frame_offsets / frame_objects (one crop, one object per sample), n_live, batch_offsets, voxel_num_limit, labels = {}
        (the pose labels are the caller's) -- and counts, picks, valid on the device in the device form, counts on the host
        in the host form.  Row i of every per-crop tensor is bit for bit what build_lm returns for sample i (feat_inp =
        inp.feats rows, voxel_inp = inp.coords[:, 1:], feat_tmp / voxel_tmp likewise, centroid).
        draws="device": every sample stays (valid == 0 where build_lm's device form says so), sample i draws with the key
        (draw_frame + i, 0), draw_frame advances by len(samples); pad_to as in build_frames.  draws="host": the samples for
        which build_lm returns None are dropped and flagged 0 in all_flags; one read-back of the counts per group.
        Mask-derived boxes are device tensors, so crop_points_frames' capacity is H * W per instance: the instances are issued in
        groups whose four (n, cap, 3) float buffers stay under FRAMES_SCRATCH_BYTES (512 MB: 34 instances of 480 x 640)."""
        return self._lm_frames(samples, LM_MIN_VALID, eval_mode, eval_mode, pad_to, "build_lm_frames", True)

    def build_lmo_frames(self, samples, pad_to=None):
        """build_lmo for several samples in one call; samples as build_lm_frames takes them (obj_bb is not read: the box always
        comes from the mask).  The dict of build_lm_frames."""
        return self._lm_frames(samples, LMO_MIN_VALID, True, False, pad_to, "build_lmo_frames", False)

    def _lm_frames(self, samples, min_valid, always_filter, keep_sparse, pad_to, what, read_boxes):
        n = len(samples)
        if n == 0:
            raise ValueError("%s: at least one sample" % what)
        dev = self.dev
        if len(set(tuple(s[1].shape) for s in samples)) != 1 or len(set(int(s[0].shape[2]) for s in samples)) != 1:
            raise ValueError("%s: every sample has the same size and channel count" % what)
        given = [read_boxes and s[3] is not None for s in samples]
        if any(given) != all(given):
            raise ValueError("%s: obj_bb for every sample or for none" % what)
        if any(s[4] is None for s in samples):
            raise TypeError("%s: obj (the class id) is required" % what)
        objs = [int(s[4]) for s in samples]
        rows_total = self._pad_rows(n, pad_to)
        self._check_capacity_rows(rows_total, what)
        H, W = samples[0][1].shape
        i_t = torch.from_numpy(np.stack([np.ascontiguousarray(s[0]) for s in samples])).to(dev)
        d_t = torch.from_numpy(np.stack([np.ascontiguousarray(s[1]).astype(np.uint16) for s in samples]).view(np.int16)).to(dev)
        l_t = torch.from_numpy(np.stack([np.ascontiguousarray(s[2]).astype(np.int32) for s in samples])).to(dev)
        fidx = np.arange(n, dtype=np.int32)
        if all(given):
            src = []
            for k, s in enumerate(samples):
                r0, r1, c0, c1 = lm_box(s[3], H, W)
                src.append((max(r0, 0), min(r1, H), max(c0, 0), min(c1, W), 1, k))
            src_a = np.asarray(src, np.int32)
            src_t = _upload(src_a, dev)
            cap = max(1, int(((src_a[:, 1] - src_a[:, 0]).clip(0) * (src_a[:, 3] - src_a[:, 2]).clip(0)).max()))
        else:
            tail = _upload(np.stack([np.ones(n, np.int32), fidx], 1), dev)
            src_t = torch.cat([ops.mask_box(l_t, 1, 0)[:, 4:8], tail], 1).contiguous()      # device rows: no host round trip
            cap = H * W
        stack = (i_t, d_t, l_t)
        host = {"voxel_num_limit": torch.tensor(self.limit), "obj": torch.IntTensor(objs), "flags": torch.IntTensor([-1]),
                "frame_objects": torch.arange(n + 1).int(), "labels": {}}

        def finish(data, keep, rows, feats_inp, coords_inp):
            cls = [objs[k] for k in keep] + [objs[keep[0]]] * (rows - len(keep))
            data["batch_offsets"] = (torch.arange(rows + 1) * 1024).int()
            data["inp"] = self._inp_side(feats_inp, coords_inp, rows)
            if self.template_ids:
                data["tmp_cls"] = _upload(np.asarray(cls, np.int32), dev)
            else:
                trows = [self.cls_row[c] for c in cls]
                occ, p2v, v2p, coords_tmp = self._template_side(trows)
                feats_tmp = self.tmp_feats[_upload(np.asarray(trows, np.int64), dev)].reshape(rows * self.n_tmp, 7)
                data["tmp"] = {"feats": feats_tmp, "coords": coords_tmp, "occupied_voxels": occ, "p2v_maps": p2v, "v2p_maps": v2p}
            data["ready_event"] = torch.cuda.Event()
            data["ready_event"].record(torch.cuda.current_stream(dev))
            return data

        if self.draws == "device":
            frame0, self.draw_frame = self.draw_frame, self.draw_frame + n
            keys_t = _upload(np.stack([frame0 + np.arange(n, dtype=np.int64), np.zeros(n, np.int64)], 1), dev)
            feats_inp, coords_inp, centroid, counts, picks, valid = self._device_rows(
                stack, src_t, fidx, cap, keys_t, rows_total, min_valid, always_filter, keep_sparse, False)
            data = dict(host, all_flags=torch.ones(n, dtype=torch.int32), all_centroids=centroid, counts=counts, valid=valid,
                        picks=picks, frame_offsets=torch.arange(n + 1).int(), n_live=n)
            return finish(data, list(range(n)), rows_total, feats_inp, coords_inp)

        per = max(1, int(self.FRAMES_SCRATCH_BYTES // (48 * cap)))
        keep, feats_g, coords_g, cen_g, cnt_g = [], [], [], [], []
        for g0 in range(0, n, per):
            g1 = min(n, g0 + per)
            xyz, col, cen, counts = ops.crop_points_frames(d_t, l_t, i_t, fidx[g0:g1], src_t[g0:g1], self.camera, RGB_MEAN,
                                                           self.extent * 0.5, min_valid, always_filter=always_filter, cap=cap)
            cnt = counts.cpu().numpy()                                              # the group's host read-back
            mine = [k for k in range(g1 - g0) if cnt[k, 0] != 0 and (cnt[k, 1] > min_valid or keep_sparse)]
            if not mine:
                continue
            picks = [ops.legacy_choice_heads([int(cnt[k, 2])], self.n_inp)[0] if cnt[k, 2] > self.n_inp
                     else np.random.choice(int(cnt[k, 2]), self.n_inp) for k in mine]     # build_lm's draw, sample by sample
            if len(mine) != g1 - g0:
                kt = _upload(np.asarray(mine, np.int64), dev)
                xyz, col, cen = xyz[kt].contiguous(), col[kt].contiguous(), cen[kt]
            pick_t = _upload(np.stack(picks).astype(np.int64), dev)
            feats, coords = ops.crop_sample(xyz, col, pick_t, None, self.extent[0] * 0.5, self.unit, int(self.limit[0]))
            if keep:
                coords[:, 0] += len(keep)
            keep.extend(g0 + k for k in mine)
            feats_g.append(feats), coords_g.append(coords), cen_g.append(cen), cnt_g.append(cnt[mine])
        if not keep:
            raise ValueError("%s: every sample of this call is the loader's dummy sample" % what)
        cat = lambda ts: ts[0] if len(ts) == 1 else torch.cat(ts)  # noqa: E731
        flags = np.zeros(n, np.int32)
        flags[keep] = 1
        data = dict(host, all_flags=torch.IntTensor(flags), all_centroids=cat(cen_g), counts=np.concatenate(cnt_g),
                    frame_offsets=torch.IntTensor(np.concatenate([[0], np.cumsum(flags)])), n_live=len(keep))
        return finish(data, keep, len(keep), cat(feats_g), cat(coords_g))


class CropPrefetcher(object):
    """The role of the reference's loader workers (torch.utils.data.DataLoader(num_workers=...), tools/test_YCBV_stage1.py:133-
    137, tools/test_LM.py:88-92: frames are prepared ahead of the network): ONE host thread builds the crops of up to `depth`
    frames ahead on its own stream while the caller's thread runs the network.  `frames` yields the argument tuples of
    CropBuilder.build (a trailing dict = keyword arguments).  The frames are built strictly in order by that one thread, so
    a seeded run consumes the global np.random stream exactly like a serial loop; the caller must not draw from np.random
    while iterating.  Iterating yields build()'s dicts: the caller's current stream already waits for the builder's
    ready_event, and every tensor is marked as used on that stream (allocator hand-over between streams).  frames_per_call=k
    (or pad_to): the frame iterator is taken k frames at a time (the last call: what is left) and iterating yields
    build_frames(group, pad_to=pad_to)'s dicts; frames_per_call=1 with pad_to=None keeps calling build().  priority: of the
    builder's stream (0 = default; a high-priority builder stream (-1) was measured slower on 6-object frames: its kernels then
    cut into the network's); stream: an existing stream to build on (a long-lived process that has made many streams may
    want to reuse one it knows not to share a hardware queue with the network's)."""
    _END = object()

    def __init__(self, builder, frames, depth=2, priority=0, stream=None, frames_per_call=1, pad_to=None):
        import queue
        import threading
        self.builder, self.dev = builder, builder.dev
        self._per_call, self._pad_to = int(frames_per_call), pad_to
        if self._per_call < 1:
            raise ValueError("CropPrefetcher: frames_per_call must be at least 1")
        self._q = queue.Queue(maxsize=max(1, int(depth)))
        self._stop = threading.Event()
        self._priority = int(priority)
        self._stream = stream                         # the builder's stream (None: a new one of the given priority)
        self._thread = threading.Thread(target=self._work, args=(iter(frames),), name="dcl-crop-prefetch", daemon=True)
        self._thread.start()

    def _put(self, item):
        import queue
        while not self._stop.is_set():
            try:
                self._q.put(item, timeout=0.05)
                return True
            except queue.Full:
                continue
        return False

    def _work(self, frames):
        try:
            with torch.cuda.device(self.dev):
                stream = self._stream if self._stream is not None else torch.cuda.Stream(self.dev, priority=self._priority)
                with torch.cuda.stream(stream):
                    group = []
                    for args in frames:
                        if self._stop.is_set():
                            return
                        args = tuple(args)
                        kw = args[-1] if args and isinstance(args[-1], dict) else {}
                        if kw:
                            args = args[:-1]
                        if self._per_call == 1 and self._pad_to is None:
                            if not self._put(self.builder.build(*args, **kw)):
                                return
                            continue
                        extra = set(kw) - {"poses"}
                        if extra or len(args) > 6:
                            raise TypeError("CropPrefetcher: build_frames takes (img, depth, label, rois, gt_obj[, poses]) per frame")
                        group.append(args[:5] + ((kw["poses"],) if "poses" in kw else args[5:]))
                        if len(group) == self._per_call:
                            if not self._put(self.builder.build_frames(group, pad_to=self._pad_to)):
                                return
                            group = []
                    if group and not self._put(self.builder.build_frames(group, pad_to=self._pad_to)):   # the last, shorter call
                        return
            self._put(self._END)
        except BaseException as e:                      # handed to the consumer, raised from its next()
            self._put(e)

    def __iter__(self):
        return self

    def __next__(self):
        item = self._q.get()
        if item is self._END:
            self._q.put(item)                           # a second next() ends as well
            raise StopIteration
        if isinstance(item, BaseException):
            self._q.put(self._END)
            raise item
        cur = torch.cuda.current_stream(self.dev)
        cur.wait_event(item["ready_event"])

        def mark(v):
            if torch.is_tensor(v):
                if v.is_cuda:
                    v.record_stream(cur)
            elif isinstance(v, dict):
                for x in v.values():
                    mark(x)
        mark(item)
        return item

    def close(self):
        """stop the builder thread (frames already built are dropped)"""
        import queue
        self._stop.set()
        try:
            while True:
                self._q.get_nowait()
        except queue.Empty:
            pass
        self._thread.join(timeout=5.0)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def exact_form(data):
    """a capacity-form data dict of CropBuilder(capacity=True) -> the loader's exact form (occupied_voxels (V,4), v2p_maps
    (V, 1+maxActive)): ONE host read-back of {V, maxActive, error}.  A dict that is exact already is returned as it is."""
    side = data["inp"]
    if "v0_dev" not in side:
        return data
    V, ma, err = side["vi_info"].cpu().tolist()
    if err:
        raise RuntimeError("CropBuilder: a voxel holds more points than v2p_pitch - 1, or a point lies outside its grid")
    out = dict(data)
    out["inp"] = {k: v for k, v in side.items() if k not in ("v0_dev", "vi_info")}
    out["inp"]["occupied_voxels"] = side["occupied_voxels"][:V]
    out["inp"]["v2p_maps"] = side["v2p_maps"][:V, :max(ma, 1) + 1].contiguous()
    return out
