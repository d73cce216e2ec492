"""Frame sharding across the GPUs of a node + exact reduction of the ADD-S metric.

Crops/images are independent: rank r owns items r, r+W, r+2W, ... and runs the whole forward on its own
GPU with no traffic.  The only collective is the metric reduction at the end, made exact by the closed form
of the reference's VOCap AUC (tools/test_YCBV_stage1.py:83-125):
    AUC_c = 100 * (10/n_c) * (0.1*m_c - (sum_valid D - max_valid D)),   valid: D <= 0.1
so per class only [n, m, sum D, #(D<0.02)] (SUM) and max D (MAX) cross the wire: 21x4 + 21 fp64 values
over RCCL (backend "nccl" on ROCm) or gloo in the CPU tests.
"""
import numpy as np
import torch
import torch.distributed as dist

N_CLASSES = 21
MAX_DIS = 0.1


def shard_indices(n_items, rank, world):
    return list(range(rank, n_items, world))


def add_s(cld, R_pred, t_pred, R_gt, t_gt, chunk=512):
    """ADD-S per object (tools/test_YCBV_stage1.py:186-189): cld (b,P,3); mean_i min_j |pred_i - gt_j|.
    CUDA tensors go to the fused HIP kernel (ops.add_s); the torch form below is the CPU-side helper of the gloo tests."""
    if cld.is_cuda:
        from . import ops
        return ops.add_s(cld, R_pred, t_pred, R_gt, t_gt)
    pred = torch.bmm(cld, R_pred.transpose(1, 2)) + t_pred.unsqueeze(1)
    gt = torch.bmm(cld, R_gt.transpose(1, 2)) + t_gt.unsqueeze(1)
    mins = []
    for s in range(0, pred.shape[1], chunk):
        mins.append(torch.cdist(pred[:, s:s + chunk], gt, compute_mode="donot_use_mm_for_euclid_dist").min(dim=2)[0])
    return torch.cat(mins, dim=1).mean(dim=1)


def add_lm(cld, R_pred, t_pred, R_gt, t_gt, sym_flag):
    """LineMOD distance per object (tools/test_LM.py:123-135): ADD (`l2_dis`) where sym_flag == 0, ADD-S (`cd_dis`) where it
    is 1.  CUDA tensors go to the fused HIP kernel; the torch form is the CPU-side helper of the gloo tests."""
    if cld.is_cuda:
        from . import ops
        return ops.add_s(cld, R_pred, t_pred, R_gt, t_gt, sym_flag=sym_flag)
    pred = torch.bmm(cld, R_pred.transpose(1, 2)) + t_pred.unsqueeze(1)
    gt = torch.bmm(cld, R_gt.transpose(1, 2)) + t_gt.unsqueeze(1)
    l2 = torch.norm(pred - gt, dim=2).mean(dim=1)
    cd = torch.cdist(pred, gt, compute_mode="donot_use_mm_for_euclid_dist").min(dim=2)[0].mean(dim=1)
    return torch.where(sym_flag.to(l2.device) != 0, cd, l2)


class LmTable(object):
    """LineMOD ADD(S) < 0.1 d success table (tools/test_LM.py:99-100,126-141,148-153): per object `num_count` and
    `success_count` with the threshold `dis < diameter[idx]` (diameter[] already holds 0.1 * object diameter in metres,
    tools/test_LM.py:68-75); lost detections (flag -1) are not counted at all.  Integer counts: the SUM all-reduce over
    RCCL / gloo is exact."""
    OBJLIST = (1, 2, 4, 5, 6, 8, 9, 10, 11, 12, 13, 14, 15)          # tools/test_LM.py:71

    def __init__(self, diameter):
        self.diameter = np.asarray(diameter, np.float64)
        self.counts = np.zeros((len(self.diameter), 2), np.int64)        # num_count, success_count

    def add(self, idx, dis, flag=0):
        if flag == -1:
            return
        self.counts[idx, 0] += 1
        if dis < self.diameter[idx]:
            self.counts[idx, 1] += 1

    def add_batch(self, obj_idx, dis, flags=None):
        """the per-frame loop of tools/test_LM.py:126-141: `flags` covers every object of the frame (incl. -1 = lost),
        obj_idx / dis only the detected ones, in order"""
        flags = [0] * len(dis) if flags is None else [int(f) for f in flags]
        k = 0
        for f in flags:
            if f == -1:
                continue
            self.add(int(obj_idx[k]), float(dis[k]))
            k += 1
        assert k == len(dis)

    def reduce(self, device=None, group=None):
        if not (dist.is_available() and dist.is_initialized()):
            return self
        c = torch.from_numpy(self.counts).to(device or "cpu")
        dist.all_reduce(c, op=dist.ReduceOp.SUM, group=group)
        self.counts = c.cpu().numpy()
        return self

    def finalize(self):
        """-> (ALL success rate, per-object success rates) as tools/test_LM.py:148-153 logs them"""
        num, suc = self.counts[:, 0], self.counts[:, 1]
        with np.errstate(divide="ignore", invalid="ignore"):
            per = np.where(num > 0, suc / np.maximum(num, 1), np.nan)
        return (float(suc.sum()) / float(num.sum()) if num.sum() else float("nan")), per


class LmoTable(LmTable):
    """Occlusion-LineMOD success table (tools/test_LMO.py:98-99,104-118,136-154,163-167): LmTable's counts and threshold,
    except that a LOST detection counts as a failure instead of being dropped -- `num_count[idx] += 1` without a distance
    ("Following HybridPose, count it on", :107-116).  The reference takes that branch for a frame whose only object is
    lost; its collate then still carries the object's index (LM/dataloader_test_LMO.py:341-352).  Integer counts: the SUM
    all-reduce stays exact."""
    OBJLIST = (1, 5, 6, 8, 9, 10, 11, 12)                              # tools/test_LMO.py:68
    SYM_IDX = (5, 6)                                                   # LM/dataloader_test_LMO.py:104: eggbox, glue

    def add_lost(self, idx):
        self.counts[idx, 0] += 1

    def add_batch(self, obj_idx, dis, flags=None):
        """one frame of the eval loop.  `flags` covers every object of the frame (-1 = lost).  A lost object is counted
        (add_lost) when obj_idx names it too -- len(obj_idx) == len(flags), the lost-frame collate of the Occlusion-LineMOD
        loader -- and skipped as in LmTable when obj_idx covers the detected objects only; `dis` always covers only the
        detected ones, in order."""
        flags = [0] * len(dis) if flags is None else [int(f) for f in flags]
        with_lost = len(obj_idx) == len(flags)
        k = 0
        for j, f in enumerate(flags):
            if f == -1:
                if with_lost:
                    self.add_lost(int(obj_idx[j]))
                continue
            self.add(int(obj_idx[j if with_lost else k]), float(dis[k]))
            k += 1
        assert k == len(dis)


class AddsTable(object):
    """per-class sufficient statistics of the YCB-V ADD-S AUC / <2cm metric."""

    def __init__(self, n_classes=N_CLASSES):
        self.sums = np.zeros((n_classes, 4), np.float64)      # n, m, sum D valid, count D < 0.02
        self.maxd = np.zeros(n_classes, np.float64)

    def add(self, cls, d):
        """d = ADD-S distance, np.inf for a missed detection (tools/test_YCBV_stage1.py:192-194)."""
        self.sums[cls, 0] += 1
        if d <= MAX_DIS:
            self.sums[cls, 1] += 1
            self.sums[cls, 2] += d
            self.maxd[cls] = max(self.maxd[cls], d)
        if d < 0.02:
            self.sums[cls, 3] += 1

    def reduce(self, device=None, group=None):
        """all_reduce over the process group (no-op when torch.distributed is not initialised; a one-rank group still
        goes through the collective, so a single-GPU smoke run exercises the RCCL path)."""
        if not (dist.is_available() and dist.is_initialized()):
            return self
        s = torch.from_numpy(self.sums).to(device or "cpu")
        m = torch.from_numpy(self.maxd).to(device or "cpu")
        dist.all_reduce(s, op=dist.ReduceOp.SUM, group=group)
        dist.all_reduce(m, op=dist.ReduceOp.MAX, group=group)
        self.sums, self.maxd = s.cpu().numpy(), m.cpu().numpy()
        return self

    def finalize(self):
        """-> (mean AUC, mean <2cm, per-class AUC, per-class <2cm) as cal_metric_auc_acc reports them."""
        n, m, sd, c2 = self.sums.T
        with np.errstate(divide="ignore", invalid="ignore"):
            auc = np.where(n > 0, 100.0 * (10.0 / np.maximum(n, 1)) * (MAX_DIS * m - (sd - self.maxd)), 0.0)
            acc = np.where(n > 0, 100.0 * c2 / np.maximum(n, 1), 0.0)
        return round(float(np.mean(auc)), 2), round(float(np.mean(acc)), 2), auc, acc


# ------------------------------------------------------------------------------------------ device-resident tables
class _DeviceTable(object):
    """The sufficient statistics of a host table above as tensors on `device`, one set per step (pose of a trajectory), updated
    by ONE call per frame from device-side poses / distances, class ids and the crop builder's `valid` -- nothing is read
    back until to_host() / finalize() (csrc/metric_table.hip; the rules: include/dclnet_hip.h, "device-resident eval tables").
    The update is the host class's, crop by crop in ascending order with its comparisons in double, so to_host() returns the
    table the host class would hold had it been fed `float(d)` of every fp32 distance in the same order.

    OWNERSHIP: one table belongs to ONE stream.  Every call enqueues on the current stream and the update is not atomic across
    launches: calls on a table are ordered by that stream (or by events the caller places), never issued from two streams at
    once.  With device="cpu" the tensors are CPU tensors and the update is the library's host twin (no GPU call)."""
    MODE = None
    HOST = None

    def __init__(self, n_classes, steps=1, device=None, diameter=None):
        from . import ops
        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        self.device = torch.device(device)
        self.steps, self.n_classes = int(steps), int(n_classes)
        self.arrays = ops.metric_table_arrays(self.MODE, self.steps, self.n_classes, self.device)
        self.diameter_host = None if diameter is None else np.asarray(diameter, np.float64).copy()
        self.diameter = None if diameter is None else torch.from_numpy(self.diameter_host).to(self.device)
        self._buffers = {}

    # the arrays by name, as the host classes name them
    sums = property(lambda self: self.arrays["sums"])
    maxd = property(lambda self: self.arrays["maxd"])
    counts = property(lambda self: self.arrays["counts"])
    bad = property(lambda self: self.arrays["bad"])

    def _poses(self, rots, transs):
        if rots.dim() == 3:
            rots, transs = rots.unsqueeze(0), transs.unsqueeze(0)
        if rots.shape[0] != self.steps:
            raise ValueError("the table holds %d step(s), the poses %d" % (self.steps, rots.shape[0]))
        return rots, transs

    def add_frame(self, cld, cls, rots, transs, R_gt, t_gt, valid=None, sym_flag=None, per_crop=False):
        """one frame from poses: rots (b,3,3) / (steps,b,3,3), transs (b,3) / (steps,b,3), one ground truth (b,3,3), (b,3);
        cls (b,) int32 the class ids; cld (n_clouds,P,3) with crop i's cloud cld[cls[i]], or, per_crop=True, (b,P,3) with
        crop i's cloud cld[i]; valid (b,) int32 or None (the crop builder's data["valid"]: > 0 a crop, 0 a candidate that gave
        none, < 0 a PADDING row of build_frames(pad_to=...) -- not a crop: its poses are not read and no entry of any table, nor
        `bad`, is touched for it); sym_flag (b,) as add_lm's.
        The distance is ADD-S for the YCB-V table; for the LineMOD tables ADD where sym_flag == 0 (or None), ADD-S elsewhere.
        On the GPU: two launches, no read-back, and no allocation after the first call of a (b, P) when the tensors are
        float32 / int32 and contiguous."""
        from . import ops
        rots, transs = self._poses(rots, transs)
        T, b, P = self.steps, int(rots.shape[1]), int(cld.shape[1])
        metric = "adds" if self.MODE == "adds" else "add"
        if not self.device.type == "cuda":
            pick = cld if per_crop else cld[cls.long()]
            rows = []
            for t in range(T):
                d = add_s(pick, rots[t], transs[t], R_gt, t_gt) if (metric == "adds" and sym_flag is None) else \
                    add_lm(pick, rots[t], transs[t], R_gt, t_gt, torch.zeros(b, dtype=torch.int32) if sym_flag is None else sym_flag)
                rows.append(d.float())
            return self.add_distances(cls, torch.stack(rows) if b else torch.zeros((T, 0)), valid)
        key = (b, P)
        if key not in self._buffers:
            self._buffers[key] = torch.empty((T, b, (P + 255) // 256), dtype=torch.float32, device=self.device)
        ops.add_tabulate(self.arrays, cld, cls, rots, transs, R_gt, t_gt, valid=valid, cloud=None if per_crop else cls,
                         sym_flag=sym_flag, metric=metric, mode=self.MODE, diameter=self.diameter, scratch=self._buffers[key])
        return self

    def add_distances(self, cls, dis, valid=None):
        """distances computed elsewhere: dis (b,) / (steps,b) float32, cls (b,) int32, valid (b,) int32 or None.  One launch."""
        from . import ops
        if dis.dim() == 1:
            dis = dis.unsqueeze(0)
        if dis.shape[0] != self.steps:
            raise ValueError("the table holds %d step(s), the distances %d" % (self.steps, dis.shape[0]))
        fn = ops.metric_tabulate if self.device.type == "cuda" else ops.metric_tabulate_host
        fn(self.arrays, dis, cls, valid, mode=self.MODE, diameter=self.diameter)
        return self

    def add_lost(self, cls_ids):
        """lost detections a loader reports on the HOST (the reference loaders' all_flags == 0 / flag -1): the same update
        with an all-invalid batch, at every step -- AddsTable.add(c, inf), dropped by the LineMOD table, counted by the
        Occlusion-LineMOD one.  Uploads the ids; reads nothing back."""
        ids = torch.as_tensor(np.asarray(cls_ids, np.int32).reshape(-1)).to(self.device)
        n = int(ids.numel())
        return self.add_distances(ids, torch.zeros((self.steps, n), dtype=torch.float32, device=self.device),
                                  torch.zeros(n, dtype=torch.int32, device=self.device))

    def reduce(self, group=None):
        """all_reduce of the tensors where they live (SUM for sums / counts, MAX for maxd and bad); a no-op when
        torch.distributed is not initialised."""
        if not (dist.is_available() and dist.is_initialized()):
            return self
        for name, op in (("sums", dist.ReduceOp.SUM), ("counts", dist.ReduceOp.SUM), ("maxd", dist.ReduceOp.MAX),
                         ("bad", dist.ReduceOp.MAX)):
            if self.arrays[name] is not None:
                dist.all_reduce(self.arrays[name], op=op, group=group)
        return self

    def _read_back(self):
        live = [(k, v) for k, v in self.arrays.items() if v is not None]
        packed = torch.cat([v.reshape(-1).to(live[0][1].dtype) for _, v in live]).cpu().numpy()      # ONE read-back
        host, at = {}, 0
        for k, v in live:
            host[k] = packed[at:at + v.numel()].reshape(tuple(v.shape)).astype(np.int32 if k == "bad" else packed.dtype)
            at += v.numel()
        if int(host["bad"][0]) != 0:
            raise ValueError("a class id outside [0, %d) was fed to this table (it updated nothing)" % self.n_classes)
        return host

    def to_host(self, step=-1):
        """the host table of one step (one read-back).  ValueError if a class id outside [0, n_classes) was ever fed."""
        return self._host_table(self._read_back(), step)

    def to_host_all(self):
        """the host tables of every step, from one read-back"""
        host = self._read_back()
        return [self._host_table(host, t) for t in range(self.steps)]

    def finalize(self, step=-1):
        """to_host(step).finalize(): the reported numbers come from the host class's own code"""
        return self.to_host(step).finalize()


class DeviceAddsTable(_DeviceTable):
    """AddsTable on the device (see _DeviceTable): sums (steps,C,4) / maxd (steps,C) float64, bad (1) int32."""
    MODE = "adds"

    def __init__(self, n_classes=N_CLASSES, steps=1, device=None):
        _DeviceTable.__init__(self, n_classes, steps, device)

    def _host_table(self, host, step):
        t = AddsTable(self.n_classes)
        t.sums, t.maxd = host["sums"][step].copy(), host["maxd"][step].copy()
        return t


class DeviceLmTable(_DeviceTable):
    """LmTable on the device (see _DeviceTable): counts (steps,C,2) int64; a crop with valid == 0 is dropped."""
    MODE = "lm"
    HOST = LmTable

    def __init__(self, diameter, steps=1, device=None):
        _DeviceTable.__init__(self, len(diameter), steps, device, diameter)

    def _host_table(self, host, step):
        t = self.HOST(self.diameter_host)
        t.counts = host["counts"][step].copy()
        return t


class DeviceLmoTable(DeviceLmTable):
    """LmoTable on the device: DeviceLmTable, except that a crop with valid == 0 (and add_lost) counts as an attempt."""
    MODE = "lmo"
    HOST = LmoTable


for _cls in (DeviceAddsTable, DeviceLmTable, DeviceLmoTable):
    _cls.__doc__ += "\n\n" + _DeviceTable.__doc__
del _cls


# ------------------------------------------------------------------------------------------ rank placement on the host
def _parse_cpulist(text):
    cpus = set()
    for part in text.strip().split(","):
        if not part:
            continue
        lo, _, hi = part.partition("-")
        cpus.update(range(int(lo), int(hi or lo) + 1))
    return cpus


def gpu_numa_nodes(sysfs_root="/sys"):
    """NUMA node of every GPU in KFD enumeration order (= HIP device order unless *_VISIBLE_DEVICES reorders), read from the
    KFD topology in sysfs -- no HIP call, so it can run before the process touches a GPU.  A GPU node is a topology node
    with simd_count > 0; its NUMA node is the CPU node at the other end of its cheapest io_link.  [] if there is no KFD."""
    import os
    base = os.path.join(sysfs_root, "class", "kfd", "kfd", "topology", "nodes")
    if not os.path.isdir(base):
        return []

    def props(path):
        out = {}
        try:
            for line in open(path):
                k, _, v = line.strip().partition(" ")
                out[k] = v
        except OSError:
            pass
        return out
    nodes = sorted((int(d) for d in os.listdir(base) if d.isdigit()))
    info = {n: props(os.path.join(base, str(n), "properties")) for n in nodes}
    cpu_nodes = [n for n in nodes if int(info[n].get("cpu_cores_count", "0") or 0) > 0]
    numa = []
    for n in nodes:
        if int(info[n].get("simd_count", "0") or 0) <= 0:
            continue
        best, best_w = (cpu_nodes[0] if cpu_nodes else 0), None
        links = os.path.join(base, str(n), "io_links")
        if os.path.isdir(links):
            for l in sorted(os.listdir(links)):
                p = props(os.path.join(links, l, "properties"))
                to, w = int(p.get("node_to", "-1") or -1), int(p.get("weight", "0") or 0)
                if to in cpu_nodes and (best_w is None or w < best_w):
                    best, best_w = to, w
        numa.append(cpu_nodes.index(best) if best in cpu_nodes else 0)
    return numa


def visible_device_map(env, n_gpus):
    """KFD GPU index of every HIP ordinal under ROCR_VISIBLE_DEVICES / HIP_VISIBLE_DEVICES / CUDA_VISIBLE_DEVICES (ROCR first:
    it filters what HIP then numbers): list of ints, all of 0..n_gpus-1 when nothing is set; None when a variable cannot be
    resolved to plain ordinals (then the topology is not used)."""
    ids = list(range(n_gpus))
    for var in ("ROCR_VISIBLE_DEVICES", "HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        val = env.get(var)
        if val is None or val.strip() == "":
            continue
        picked = []
        for tok in val.split(","):
            tok = tok.strip()
            if not tok.isdigit() or int(tok) >= len(ids):
                return None
            picked.append(ids[int(tok)])
        ids = picked
        if var == "HIP_VISIBLE_DEVICES":
            break                                              # (CUDA_VISIBLE_DEVICES is an alias of it: not applied twice)
    return ids


def rank_cpu_set(local_rank, local_world, allowed=None, sysfs_root="/sys", env=None):
    """the host cores rank `local_rank` of `local_world` ranks on this node should run on: the cores of its GPU's NUMA node
    (inside the process's allowed set), divided evenly among the ranks whose GPUs share that node -- with one process per GPU
    and a per-call host read-back on the launch-by-launch path, eight ranks hopping over 2 sockets become launch-bound
    otherwise.  Falls back to an even split of the allowed cores when the topology cannot be read.  Pure function."""
    import os
    if allowed is None:
        allowed = os.sched_getaffinity(0)
    allowed = sorted(allowed)
    numa = gpu_numa_nodes(sysfs_root)
    peers, mine = list(range(local_world)), allowed
    # HIP ordinal i is KFD GPU i only while no *_VISIBLE_DEVICES selects or reorders a subset (a leased N-of-8 box): an
    # explicit plain list "a,b,c" of ordinals is followed; anything else (uuids, ...) takes the even split below
    vis = visible_device_map(env if env is not None else os.environ, len(numa))
    if vis is None:
        numa = []
    else:
        numa = [numa[g] for g in vis]
    if len(numa) >= local_world and local_world > 0:
        node = numa[local_rank]
        try:
            cpus = _parse_cpulist(open(os.path.join(sysfs_root, "devices", "system", "node", "node%d" % node, "cpulist")).read())
        except OSError:
            cpus = set()
        on_node = [c for c in allowed if c in cpus]
        if on_node:
            mine = on_node
            peers = [r for r in range(local_world) if numa[r] == node]
    k, i = len(peers), peers.index(local_rank) if local_rank in peers else 0
    per = max(1, len(mine) // max(k, 1))
    chunk = mine[i * per:(i + 1) * per] if i * per < len(mine) else mine
    return set(chunk or mine)


def pin_rank_to_gpu_numa(local_rank, local_world, sysfs_root="/sys"):
    """call BEFORE the first GPU call of a rank (bench.py does): sets the process's CPU affinity to rank_cpu_set(...).
    Returns the sorted core list in effect (what the bench line reports per rank)."""
    import os
    try:
        cpus = rank_cpu_set(local_rank, local_world, sysfs_root=sysfs_root)
        if local_world > 1:
            os.sched_setaffinity(0, cpus)
    except OSError:
        pass
    return sorted(os.sched_getaffinity(0))
