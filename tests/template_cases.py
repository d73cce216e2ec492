"""Cases of the template-row scatter (csrc/template_rows.hip) shared by the CPU test of its host twin and the GPU test of the
kernel: a cache of four classes, batches that repeat a class, and block sets that take the 16-byte path, the float-by-float
path, or both in one launch.  The reference is plain numpy indexing, computed once per case and never modified."""
import functools

import numpy as np
import torch

CLASS_IDS = (2, 5, 7, 21)
LUT_LEN = 22
COLS = 643                                  # the network's row: [p1 256 | m1 64 | p2 256 | m2 64 | xyz 3]
SENTINEL = -7.5                             # destinations are pre-filled with it: a write outside a block shows

# a block: (src_col, width, buffer, dst_col); a buffer: name -> (pitch, base offset in floats -- 1 = off 16-byte alignment)
BLOCK_SETS = {
    # Yop1 (256 dense), Yom1 (64 dense), Yop2 = fuse2[:, 256:], Yom2 = conf_in2[:, 64:], points_tmp (3 dense)
    "network": ([(0, 256, "p1", 0), (256, 64, "m1", 0), (320, 256, "fuse2", 256), (576, 64, "conf2", 64), (640, 3, "xyz", 0)],
                {"p1": (256, 0), "m1": (64, 0), "fuse2": (512, 0), "conf2": (128, 0), "xyz": (3, 0)}),
    "aligned_4_12": ([(8, 4, "a", 4), (100, 12, "b", 0)], {"a": (12, 0), "b": (16, 0)}),
    "narrow_1_3_7": ([(0, 1, "a", 2), (5, 3, "b", 1), (636, 7, "c", 0)], {"a": (4, 0), "b": (5, 0), "c": (7, 0)}),
    # the same aligned blocks on a buffer whose base is one float off: the float-by-float path
    "base_off": ([(8, 4, "a", 4), (100, 12, "b", 0)], {"a": (12, 1), "b": (16, 1)}),
}
BATCHES = {1: (7,), 3: (5, 21, 5)}          # class ids per crop; the three-crop batch repeats a class
N_TMP = (1, 5, 64, 517)
PITCHES = (644, 643)                        # cache row pitch: 644 = 16-byte aligned rows (what the network keeps), 643 = dense
CASES = [(b, n, name, pitch) for b in sorted(BATCHES) for n in N_TMP for name in BLOCK_SETS for pitch in PITCHES]


def case_id(case):
    return "b%d-n%d-%s-p%d" % case


@functools.lru_cache(maxsize=None)
def cache_rows(n_tmp):
    """(C, n_tmp, COLS) float32: distinct, exactly representable values, so one wrong element shows"""
    rng = np.random.default_rng(100 + n_tmp)
    a = rng.integers(-(1 << 20), 1 << 20, (len(CLASS_IDS), n_tmp, COLS)).astype(np.float32) / np.float32(64)
    a.setflags(write=False)
    return a


def lut():
    t = np.full(LUT_LEN, -1, np.int32)
    for slot, c in enumerate(CLASS_IDS):
        t[c] = slot
    return t


def reference(n_tmp, ids, name):
    """{buffer: (rows, pitch) float32} by plain indexing; a missed crop's blocks are zeros; -> (buffers, miss)"""
    blocks, bufs = BLOCK_SETS[name]
    rows, table = cache_rows(n_tmp), lut()
    out = {k: np.full((len(ids) * n_tmp, pitch), SENTINEL, np.float32) for k, (pitch, _) in bufs.items()}
    miss = 0
    for i, c in enumerate(ids):
        slot = table[c] if 0 <= c < LUT_LEN else -1
        miss |= int(slot < 0)
        for src_col, width, buf, dst_col in blocks:
            blk = rows[slot, :, src_col:src_col + width] if slot >= 0 else np.zeros((n_tmp, width), np.float32)
            out[buf][i * n_tmp:(i + 1) * n_tmp, dst_col:dst_col + width] = blk
    return out, miss


def cache_tensor(n_tmp, pitch, device):
    """the cache as a (C, n_tmp, COLS) tensor whose rows are `pitch` floats apart"""
    store = torch.full((len(CLASS_IDS), n_tmp, pitch), float("nan"), dtype=torch.float32)
    store[:, :, :COLS] = torch.from_numpy(cache_rows(n_tmp).copy())
    return store.to(device)[:, :, :COLS]


def buffers(n_tmp, b, name, device):
    """sentinel-filled destination buffers and the op's block list; -> ({buffer: (rows, pitch) tensor}, [(src_col, dst view)])"""
    blocks, bufs = BLOCK_SETS[name]
    flat, views = {}, {}
    for k, (pitch, base) in bufs.items():
        flat[k] = torch.full((base + b * n_tmp * pitch,), SENTINEL, dtype=torch.float32, device=device)
        views[k] = flat[k][base:].view(b * n_tmp, pitch)
        assert (views[k].data_ptr() % 16 == 0) == (base == 0)
    return views, [(src_col, views[buf][:, dst_col:dst_col + width]) for src_col, width, buf, dst_col in blocks]


def run(op, n_tmp, ids, name, pitch, device, cls=None, miss=None):
    """one call of `op` (ops.template_rows or its host twin) on fresh buffers -> ({buffer: numpy}, miss value)"""
    views, blocks = buffers(n_tmp, len(ids), name, device)
    if cls is None:
        cls = torch.tensor(ids, dtype=torch.int32, device=device)
    miss = op(cache_tensor(n_tmp, pitch, device), torch.from_numpy(lut()).to(device), cls, blocks, miss)
    return {k: v.cpu().numpy() for k, v in views.items()}, int(miss.cpu()[0])
