"""Cases and helpers of the capacity-mode sparse-half tests (test_backbone_cap_cases.py on the CPU, test_gpu_backbone_cap.py on
the GPU): voxel families of 1 .. 300 voxels per crop on the 64^3 grid, the staged inputs of an ops.BackboneRunCap for a given
capacity -- live rows in front, the rows behind them filled by a named padding mode --, read-out points, the call sequences a
reused runner is fed, and the oracle's eight active sets of a case.  Everything is built on the CPU, once per case
(functools.lru_cache), and handed out read-only."""
import collections
import functools
import os
import re

import numpy as np

from test_gpu_ops import _edge_voxels

S = 64
UNIT = 0.006
OFFSET = float(np.float32(-0.5 * UNIT * S))
EXTENTS = tuple(float(np.float32(UNIT * sc)) for sc in (2, 4, 6, 8))      # the production quirk of models/DCL_Net.py:54
N_PER = 40                                    # read-out points per crop
MAX_ACTIVE = 4                                # points per voxel of the voxelisation rider's rules
BIG = 300                                     # voxels of a "big" crop
SMALL = 60                                    # ... of a "small" one (the batches of 31 / 32 crops)
PADDINGS = ("zero", "stale", "wild")
INT32_MAX = 2 ** 31 - 1
# ---- switches the product does not export: literals of the csrc files, restated here.  source_thresholds() reads them back from
#      the source text, so a retuned literal fails tests/test_backbone_cap_cases.py; the GPU census confirms where each one acts
GEO_SMALL_ROWS = 32768                        # csrc/rulebook.hip kGeoSmallRows: most rows of a one-launch geometry of 9 .. 16 crops
GEO_SMALL_ANY_ROWS = 8                        # csrc/rulebook.hip dcl_internal_geometry_small_ok: up to here whatever the rows
GEO_SMALL_BATCH = 16                          # csrc/rulebook.hip kGeoSmallBatch: most crops of the one-launch geometry
ORDER_MIN_BATCH = 14                          # csrc/backbone.hip kOrderMinBatch: row orders of the deep levels from here on
FEW_ROWS = 24576                              # csrc/sparse_conv.hip kConvFewRowsHint: few-row forms up to this many expected rows
STEM_LANE_PER_ROW_ABOVE = 49152               # csrc/sparse_conv.hip conv_dispatch: the stem's lane-per-row instance above this
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def source_thresholds():
    """{name: value} of the switches above as the csrc files spell them"""
    def find(name, pattern):
        m = re.search(pattern, open(os.path.join(ROOT, "dcl-net_amd", "csrc", name)).read())
        assert m, "csrc/%s no longer spells %r" % (name, pattern)
        return int(m.group(1))
    return {"GEO_SMALL_ROWS": find("rulebook.hip", r"constexpr int kGeoSmallRows = (\d+);"),
            "GEO_SMALL_ANY_ROWS": find("rulebook.hip", r"\(batch <= (\d+) \|\| rows <= kGeoSmallRows\)"),
            "GEO_SMALL_BATCH": find("rulebook.hip", r"DCL_HOOK_INT\(kGeoSmallBatch, (\d+)\)"),
            "ORDER_MIN_BATCH": find("backbone.hip", r"DCL_HOOK_INT\(kOrderMinBatch, (\d+)\)"),
            "FEW_ROWS": find("sparse_conv.hip", r"DCL_HOOK_INT\(kConvFewRowsHint, (\d+)\)"),
            "STEM_LANE_PER_ROW_ABOVE": find("sparse_conv.hip",
                                            r"if \(expect > (\d+)\)\s+hipLaunchKernelGGL\(\(k_sparse_conv_stem<7, 16, 1>")}


Case = collections.namedtuple("Case", "key family b occ vox feats v2p pts")


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _blob(rng, n, centre=None, sigma=4.0):
    """exactly n distinct voxels of a gaussian blob (dense enough that the convs find neighbours), shuffled"""
    c = rng.integers(16, 48, 3) if centre is None else np.asarray(centre)
    have = np.zeros((0, 3), np.int64)
    while len(have) < n:
        v = np.clip(np.floor(rng.normal(c, sigma, (3 * n, 3))), 0, S - 1).astype(np.int64)
        have = np.unique(np.concatenate([have, v]), axis=0)
    return have[rng.permutation(len(have))[:n]]


def _rows(per_crop):
    return np.concatenate([np.concatenate([np.full((len(v), 1), c), v], 1) for c, v in enumerate(per_crop)]).astype(np.int32)


def _voxels(family, b, seed):
    rng = np.random.default_rng([{"big": 1, "tiny": 2, "edge": 3, "lopsided": 4, "small": 5}[family], b, seed])
    if family == "big":
        return _rows([_blob(rng, BIG) for _ in range(b)]), b
    if family == "small":
        return _rows([_blob(rng, SMALL, sigma=2.5) for _ in range(b)]), b
    if family == "tiny":
        return _rows([rng.integers(0, S, (1, 3)) for _ in range(b)]), b
    if family == "edge":
        occ, nb = _edge_voxels(rng, S)
        assert b == nb
        return occ, b
    if family == "lopsided":
        # crop 0 holds almost all voxels, the others 1 .. 3; the LAST crop holds none.  (A crop that has a voxel keeps a row at
        # every level -- the dilating conv and the k3 s2 p1 pool never drop a crop's last voxel --, so a crop is empty at the
        # deepest level only if it is empty: tests/test_backbone_cap_cases.py asserts both from the oracle.)
        assert b >= 2
        per = [_blob(rng, BIG - 20)] + [_blob(rng, int(rng.integers(1, 4)), sigma=1.0) for _ in range(b - 2)]
        return _rows(per + [np.zeros((0, 3), np.int64)]), b
    raise KeyError(family)


@functools.lru_cache(maxsize=None)
def case(family, b, seed=1):
    """a batch of b crops of `family` with everything a pass needs: occ (V0, 4) int32 batch-sorted, vox (V0, 7) the voxelised
    features the feature stage is fed, feats (b * N_PER, 7) + v2p (V0, 1 + MAX_ACTIVE) the rider's inputs (every voxel averages
    1 .. MAX_ACTIVE of the points), pts (b * N_PER, 4) [crop, x, y, z] read-out points"""
    occ, b = _voxels(family, b, seed)
    rng = np.random.default_rng([77, b, seed, len(occ)])
    V0 = occ.shape[0]
    vox = rng.normal(size=(V0, 7)).astype(np.float32)
    feats = rng.normal(size=(b * N_PER, 7)).astype(np.float32)
    v2p = np.zeros((V0, 1 + MAX_ACTIVE), np.int32)
    v2p[:, 0] = rng.integers(1, MAX_ACTIVE + 1, V0)
    pick = rng.integers(0, b * N_PER, (V0, MAX_ACTIVE))
    v2p[:, 1:] = np.where(np.arange(MAX_ACTIVE)[None, :] < v2p[:, :1], pick, 0)
    pts = []
    for c in range(b):
        own = occ[occ[:, 0] == c][:, 1:4].astype(np.float64)
        p = rng.uniform(-0.19, 0.19, (N_PER, 3))                                   # anywhere in the grid (and a little outside)
        if len(own):
            k = N_PER // 2                                                         # half of them inside / beside occupied voxels
            near = own[rng.integers(0, len(own), k)]
            p[:k] = (near + rng.uniform(-0.5, 1.5, near.shape)) * UNIT + OFFSET
            p[0] = near[0] * UNIT + OFFSET                                         # a voxel corner: lattice ties
        pts.append(np.concatenate([np.full((N_PER, 1), c), p], 1))
    pts = np.concatenate(pts).astype(np.float32)
    return Case((family, b, seed), family, b, *_freeze(occ, vox, feats, v2p, pts))


def crops_without_voxels(c):
    return [i for i in range(c.b) if not bool((c.occ[:, 0] == i).any())]


def excluded_points(c):
    """bool (b * N_PER): points of a crop that has no voxel at all -- the only read-out rows the oracle comparison leaves out (the
    reference interpolates garbage there)"""
    return np.isin(c.pts[:, 0].astype(np.int64), crops_without_voxels(c))


def default_cap(b):
    return b * 512


def stage(c, V0_cap, padding, donor=None):
    """the static buffers of a BackboneRunCap holding case c: dict of occ (V0_cap, 4) i32, vox (V0_cap, 7) f32, v2p (V0_cap, 1 +
    MAX_ACTIVE) i32, all with c's rows in front, and v0.  The rows behind them:
      "zero"   zeros
      "stale"  the donor's staged rows (what the host staging of a replay leaves behind the live count: the previous call's);
               the donor is a dict this function or full_donor() returned for the same capacity.  It must hold more live rows
               than c, or nothing stale is left: stale_rows() counts what is
      "wild"   occ rows with crop ids >= b and < 0 and coordinates -1 / 64 / INT32_MAX, vox rows of NaN.  (The rider's rules
               stay zero there: dcl_backbone_geometry_cap_vox is handed V0_cap rules and voxelises every one of them, so a
               rule row is never padding to it.)"""
    V0 = c.occ.shape[0]
    assert V0_cap >= V0 and padding in PADDINGS
    if padding == "stale":
        assert donor is not None and donor["occ"].shape[0] == V0_cap and donor["feats_rows"] == c.feats.shape[0]
        occ, vox, v2p = donor["occ"].copy(), donor["vox"].copy(), donor["v2p"].copy()
    else:
        occ, vox = np.zeros((V0_cap, 4), np.int32), np.zeros((V0_cap, 7), np.float32)
        v2p = np.zeros((V0_cap, 1 + MAX_ACTIVE), np.int32)
    if padding == "wild":
        n = V0_cap - V0
        i = np.arange(n)
        pad = np.empty((n, 4), np.int64)
        pad[:, 0] = np.choose(i % 4, [c.b, -1, c.b + 7, INT32_MAX])
        for ax in range(3):
            pad[:, 1 + ax] = np.choose((i // 4 + ax) % 4, [-1, S, INT32_MAX, S // 2])
        pad[i % 8 == 5, 0] = 0                                                   # a VALID crop id with coordinates off the grid
        pad[i % 8 == 5, 1:] = np.array([S, -1, INT32_MAX])
        occ[V0:] = pad.astype(np.int32)
        vox[V0:] = np.nan
    occ[:V0], vox[:V0], v2p[:V0] = c.occ, c.vox, c.v2p
    return {"occ": occ, "vox": vox, "v2p": v2p, "v0": V0, "feats_rows": c.feats.shape[0]}


def full_donor(b, V0_cap, seed=9):
    """staged buffers whose EVERY row looks live: V0_cap distinct in-grid voxels with crop ids 0 .. b - 1 (batch-sorted), finite
    features, valid rules -- the most a previous call can have left behind"""
    rng = np.random.default_rng([99, b, V0_cap, seed])
    per = [V0_cap // b + (1 if i < V0_cap % b else 0) for i in range(b)]
    rows = []
    for i, n in enumerate(per):
        lin = rng.choice(S ** 3, size=n, replace=False)
        rows.append(np.stack([np.full(n, i), lin // (S * S), (lin // S) % S, lin % S], 1))
    v2p = np.zeros((V0_cap, 1 + MAX_ACTIVE), np.int32)
    v2p[:, 0] = MAX_ACTIVE
    v2p[:, 1:] = rng.integers(0, b * N_PER, (V0_cap, MAX_ACTIVE))
    return {"occ": np.concatenate(rows).astype(np.int32), "vox": rng.normal(size=(V0_cap, 7)).astype(np.float32), "v2p": v2p,
            "v0": V0_cap, "feats_rows": b * N_PER}


def stale_rows(staged, b):
    """how many rows behind the live count are in-grid voxels of a valid crop: rows a kernel that ran past *v0_dev would take for
    live ones"""
    pad = staged["occ"][staged["v0"]:]
    return int(((pad[:, 0] >= 0) & (pad[:, 0] < b) & (pad[:, 1:] >= 0).all(1) & (pad[:, 1:] < S).all(1) & pad.any(1)).sum())


# ---- the batches of the one-pass tests and of the census (family, crops[, capacity per crop])
ONE_PASS_CASES = (("big", 2), ("edge", 5))
CENSUS_CASES = (("big", 2, 512), ("big", 8, 512), ("big", 13, 512), ("big", 14, 512), ("tiny", 14, 512), ("big", 16, 512),
                ("big", 16, 2304), ("big", 17, 512), ("tiny", 17, 512), ("small", 31, 512), ("small", 32, 512))
PAIR_PADDINGS = ("stale", "wild", "stale", "zero")     # per element of PAIR_SEQUENCE, from full_donor() (the repeat: another mode)
PAIR_BATCH = 3
PAIR_CAPS = (512, 128)                                  # capacity per crop of side a / side b


def pair_case(side, family, b, seed):
    """side b's capacity holds b * 128 rows: where the sequence names a big batch there it gets the 60-voxel family"""
    return case("small" if side == 1 and family == "big" else family, b, seed)


# ---- the call sequences of a reused runner (family, seed), and the elements whose results must repeat bit for bit
SEQUENCE = (("big", 1), ("tiny", 1), ("lopsided", 1), ("big", 2), ("tiny", 1), ("big", 1))
SEQUENCE_REPEATS = ((5, 0), (4, 1))      # (later element, the earlier one it equals): big after tiny, tiny after big'
EDGE_SEQUENCE = (("edge", 1), ("big", 1), ("edge", 1))
EDGE_REPEATS = ((2, 0),)
# both sides in one launch sequence: (side a, side b) per element
PAIR_SEQUENCE = ((("big", 1), ("lopsided", 1)), (("big", 1), ("big", 2)), (("big", 1), ("tiny", 1)), (("big", 1), ("lopsided", 1)))


def sequence_paddings(n):
    return [PADDINGS[i % len(PADDINGS)] for i in range(n)]


def stage_sequence(cases, V0_cap):
    """the staged buffers of every element of a sequence, paddings cycling; "stale" takes the element before it as its donor (what a
    replay's host staging leaves)"""
    out, prev = [], full_donor(cases[0].b, V0_cap)
    for c, padding in zip(cases, sequence_paddings(len(cases))):
        prev = stage(c, V0_cap, padding, donor=prev)
        out.append(prev)
    return out


# ---- the oracle's eight active sets
@functools.lru_cache(maxsize=None)
def oracle_sets(family, b, seed=1):
    """[(rows (n, 4) int32)] * 8 of the case -- conv set and pooled set of the four levels, as oracle.graph.backbone walks them"""
    from oracle import native as K
    c = case(family, b, seed)
    idx, shape, out = c.occ, [S] * 3, []
    for _ in range(4):
        idx, _, _, shape = K.get_indice_pairs(idx, b, shape, 3, 1, 1, 1)
        out.append(idx)
        idx, _, _, shape = K.get_indice_pairs(idx, b, shape, 3, 2, 1, 1)
        out.append(idx)
    return _freeze(*out)


def oracle_counts(family, b, seed=1):
    return [int(r.shape[0]) for r in oracle_sets(family, b, seed)]


# ---- the crop-count switches of the capacity-mode forms
def split_layers(ops, b):
    """{(cin, cout, subm)} of the conv layers ops.CONV_SPLIT_WIDTHS sends to the split-bf16 form at b crops"""
    chan = ops.BACKBONE_CHANNELS
    out = set()
    for i in range(8):
        cin, cout, subm = chan[i], chan[i + 1], bool(i % 2)
        need = ops.CONV_SPLIT_WIDTHS.get((cin, cout, subm))
        if ops.CONV_SPLIT and need is not None and b * ops.CONV_SPLIT_ROWS_PER_CROP[i // 2] >= need:
            out.add((cin, cout, subm))
    return out


def split_switch_batch(ops):
    """the smallest crop count at which a layer takes the split-bf16 form (every threshold of ops.CONV_SPLIT_WIDTHS is the
    layer's expected rows at 32 crops, so this is 32 -- not 16: the census batches are the two on either side of it)"""
    return next(b for b in range(1, 1025) if split_layers(ops, b))
