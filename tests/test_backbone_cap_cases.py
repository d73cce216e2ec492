"""What the cases of tests/backbone_cap_cases.py claim, checked on the CPU: voxel counts per family, the live counts per level and
the crops that are empty at each level from the oracle's own geometry, the properties of the three padding modes, the share of
read-out rows the oracle comparison leaves out, and the crop counts at which the capacity-mode form switches sit, computed from
the tables the product exports (ops.CONV_SPLIT_WIDTHS, ops.CONV_SPLIT_ROWS_PER_CROP)."""
import numpy as np
import pytest

import backbone_cap_cases as BC

CASES = [("small", 32), ("big", 2), ("big", 3), ("big", 5), ("big", 16), ("tiny", 3), ("tiny", 14), ("tiny", 17), ("edge", 5),
         ("lopsided", 2), ("lopsided", 3), ("lopsided", 16)]


@pytest.fixture(scope="module")
def ops(dcl):
    return dcl.ops


@pytest.mark.parametrize("family,b", CASES)
def test_case_is_what_its_family_says(oracle, family, b):
    c = BC.case(family, b)
    occ = c.occ
    assert occ.dtype == np.int32 and occ.shape[1] == 4 and occ.shape[0] <= BC.default_cap(b)
    assert bool((np.diff(occ[:, 0]) >= 0).all()) and occ[:, 0].min() >= 0 and occ[:, 0].max() < b   # batch-sorted
    assert occ[:, 1:].min() >= 0 and occ[:, 1:].max() < BC.S
    assert len(np.unique(occ, axis=0)) == len(occ)
    per = np.bincount(occ[:, 0], minlength=b)
    empty = BC.crops_without_voxels(c)
    if family == "big":
        assert per.tolist() == [BC.BIG] * b and not empty
    elif family == "small":
        assert per.tolist() == [BC.SMALL] * b and not empty
    elif family == "tiny":
        assert per.tolist() == [1] * b and not empty
    elif family == "edge":
        assert b == 5 and empty == [1] and per[2] == 1 and per[4] == 30 * 40
        assert occ[occ[:, 0] == 0][:, 1:].min() == 0 and occ[occ[:, 0] == 0][:, 1:].max() == BC.S - 1    # touches the faces
    else:
        assert per[0] >= 0.9 * per.sum() and empty == [b - 1] and all(1 <= n <= 3 for n in per[1:-1])
    assert len(empty) <= 1                                  # at most one crop without any voxel per batch
    # the live counts per level and who is empty where, from the oracle's geometry
    sets = BC.oracle_sets(*c.key)
    counts = BC.oracle_counts(*c.key)
    assert len(counts) == 8 and counts[0] >= len(occ)
    for i, rows in enumerate(sets):
        Sl = BC.S >> ((i + 1) // 2)
        assert rows[:, 1:].max() < Sl
        have = np.bincount(rows[:, 0], minlength=b) > 0
        # a crop is empty at a level exactly when it has no voxel at all (lopsided's last crop: empty at level 4 because empty)
        assert [j for j in range(b) if not have[j]] == empty, i
        lin = ((rows[:, 0].astype(np.int64) * Sl + rows[:, 1]) * Sl + rows[:, 2]) * Sl + rows[:, 3]
        assert bool((np.diff(lin) > 0).all())               # ascending linear index: the numbering the runner must reproduce
    if family == "tiny":
        # one voxel per crop: at most 27 rows per crop on the first conv set and on the first pooled set.  A crop does not keep
        # ONE row per level: each dilating conv grows its set again, to about a hundred rows at the deep levels -- still less
        # than one 128-row conv tile per crop, in launches whose grids are sized by capacity.
        assert counts[0] <= 27 * b and counts[1] <= 27 * b and all(b <= n < 128 * b for n in counts)
    if family == "lopsided":
        big = BC.oracle_counts("big", b)
        assert all(n < m for n, m in zip(counts, big))      # every level of this side is smaller than a big side's
        deep = np.bincount(sets[7][:, 0], minlength=b)
        assert deep[0] == deep.max() and deep[-1] == 0
    # capacities of the runner (csrc/backbone.hip make_geo_layout: 27 x, then 8 x, bounded by the grid) hold every live count
    cap = BC.default_cap(b)
    for m in range(4):
        cap = min(cap * 27, b * (BC.S >> m) ** 3)
        assert counts[2 * m] <= cap
        cap = min(cap * 8, b * (BC.S >> (m + 1)) ** 3)
        assert counts[2 * m + 1] <= cap


@pytest.mark.parametrize("family,b", CASES)
def test_excluded_read_out_rows_are_the_points_of_voxelless_crops(family, b):
    c = BC.case(family, b)
    ex = BC.excluded_points(c)
    assert c.pts.shape == (b * BC.N_PER, 4) and c.pts.dtype == np.float32
    assert np.array_equal(c.pts[:, 0], np.repeat(np.arange(b), BC.N_PER).astype(np.float32))
    want = {"big": 0.0, "small": 0.0, "tiny": 0.0, "edge": 1.0 / 5, "lopsided": 1.0 / b}[family]
    assert float(ex.mean()) == pytest.approx(want) and float(ex.mean()) <= 0.5
    assert sorted(set(c.pts[ex, 0].astype(int).tolist())) == BC.crops_without_voxels(c)
    # the rider's rules: 1 .. MAX_ACTIVE valid point rows per voxel, unused columns zero
    n = c.v2p[:, 0]
    assert n.min() >= 1 and n.max() <= BC.MAX_ACTIVE and c.v2p[:, 1:].min() >= 0 and c.v2p[:, 1:].max() < c.feats.shape[0]
    assert bool((c.v2p[:, 1:][np.arange(BC.MAX_ACTIVE)[None, :] >= n[:, None]] == 0).all())


def test_padding_modes(oracle):
    c, d = BC.case("tiny", 3), BC.case("big", 3)
    cap = BC.default_cap(3)
    V0 = c.occ.shape[0]
    donor = BC.stage(d, cap, "zero")
    got = {p: BC.stage(c, cap, p, donor=donor) for p in BC.PADDINGS}
    for p, st in got.items():
        assert st["occ"].shape == (cap, 4) and st["vox"].shape == (cap, 7) and st["v2p"].shape == (cap, 1 + BC.MAX_ACTIVE)
        assert st["occ"].dtype == np.int32 and st["vox"].dtype == np.float32 and st["v2p"].dtype == np.int32 and st["v0"] == V0
        assert np.array_equal(st["occ"][:V0], c.occ) and np.array_equal(st["vox"][:V0], c.vox)
        assert np.array_equal(st["v2p"][:V0], c.v2p)
        # the rider voxelises every rule row of the buffer: they stay valid in every mode
        assert st["v2p"].min() >= 0 and st["v2p"][:, 0].max() <= BC.MAX_ACTIVE and st["v2p"][:, 1:].max() < c.feats.shape[0]
    z, s, w = got["zero"], got["stale"], got["wild"]
    assert not z["occ"][V0:].any() and not z["vox"][V0:].any() and not z["v2p"][V0:].any()
    Vd = d.occ.shape[0]
    assert Vd > V0 and np.array_equal(s["occ"][V0:Vd], d.occ[V0:]) and np.array_equal(s["vox"][V0:Vd], d.vox[V0:])
    assert bool((s["occ"][V0:Vd, 0] < 3).all())              # stale rows look exactly like live ones
    pad = w["occ"][V0:]
    assert bool(np.isnan(w["vox"][V0:]).all())
    assert bool((pad[:, 0] >= 3).any()) and bool((pad[:, 0] < 0).any()) and bool((pad[:, 0] == 0).any())
    for v in (-1, BC.S, BC.INT32_MAX):
        assert bool((pad[:, 1:] == v).any()), v
    inside = (pad[:, 0] >= 0) & (pad[:, 0] < 3) & (pad[:, 1:] >= 0).all(1) & (pad[:, 1:] < BC.S).all(1)
    assert not inside.any()                                  # no wild row is a voxel of the batch
    assert BC.stale_rows(z, 3) == 0 and BC.stale_rows(w, 3) == 0 and BC.stale_rows(s, 3) == Vd - V0
    # sequences: paddings cycle, "stale" inherits the element before it
    cases = [BC.case(f, 3, s_) for f, s_ in BC.SEQUENCE]
    seq = BC.stage_sequence(cases, cap)
    assert BC.sequence_paddings(6) == ["zero", "stale", "wild", "zero", "stale", "wild"]
    assert np.array_equal(seq[1]["occ"][cases[1].occ.shape[0]:cases[0].occ.shape[0]], cases[0].occ[cases[1].occ.shape[0]:])
    assert np.array_equal(seq[4]["occ"][cases[4].occ.shape[0]:cases[3].occ.shape[0]], cases[3].occ[cases[4].occ.shape[0]:])
    for (late, early), s_ in zip(BC.SEQUENCE_REPEATS, (BC.SEQUENCE,) * 2):
        assert s_[late] == s_[early] and late > early
    assert BC.EDGE_SEQUENCE[2] == BC.EDGE_SEQUENCE[0]


def test_crop_count_switches_follow_the_exported_tables(ops):
    """the batches of the census tests sit on either side of every switch the product exports; the split-bf16 layers are computed
    from the table, never spelled out"""
    rows = ops.CONV_SPLIT_ROWS_PER_CROP
    assert rows == (3600, 1800, 900, 450) and ops.BACKBONE_CHANNELS == (7, 16, 32, 32, 64, 64, 128, 128, 256)
    # FINDING: no layer of the table is listed for 16 crops -- every threshold is the layer's expected rows at 32 crops (the only
    # batch size profiles/conv_split.txt measured), so the switch sits between 31 and 32 crops, for all five layers at once
    sw = BC.split_switch_batch(ops)
    assert BC.split_layers(ops, 14) == set() and BC.split_layers(ops, 16) == set() and BC.split_layers(ops, sw - 1) == set()
    at = BC.split_layers(ops, sw)
    assert sw == 32 and at == set(ops.CONV_SPLIT_WIDTHS)
    for (cin, cout, subm), need in ops.CONV_SPLIT_WIDTHS.items():
        level = {32: 1, 64: 2, 128: 3}[cin] if subm else {64: 2, 128: 3}[cin]
        assert ((cin, cout, subm) in at) == (sw * rows[level] >= need)
        assert ops.conv_split_ok(27, cin, cout)
    assert BC.case("small", sw).occ.shape[0] == sw * BC.SMALL <= BC.GEO_SMALL_ROWS
    # capacities of the geometry routes at 16 crops: b * 512 stays on the one-launch stage, b * 2304 leaves it
    assert 16 * 512 <= BC.GEO_SMALL_ROWS < 16 * 2304 and BC.case("big", 16).occ.shape[0] <= 16 * 512
    # the switches the product does not export: the restated literals are what the csrc files spell, and the census batches
    # lie on either side of each
    assert BC.source_thresholds() == {k: getattr(BC, k) for k in BC.source_thresholds()}
    batches = sorted({b for _, b, _ in BC.CENSUS_CASES})
    assert BC.ORDER_MIN_BATCH - 1 in batches and BC.ORDER_MIN_BATCH in batches
    assert BC.GEO_SMALL_ANY_ROWS in batches and BC.GEO_SMALL_BATCH in batches and BC.GEO_SMALL_BATCH + 1 in batches
    assert {per for _, b, per in BC.CENSUS_CASES if b == BC.GEO_SMALL_BATCH} == {512, 2304}
    assert 13 * rows[0] <= BC.STEM_LANE_PER_ROW_ABOVE < 14 * rows[0] and 13 in batches and 14 in batches
    assert 2 * rows[0] <= BC.FEW_ROWS < 8 * rows[0] and 8 * rows[1] <= BC.FEW_ROWS < 14 * rows[1] and 2 in batches
    assert sw - 1 in batches and sw in batches


def _stale_stagings():
    """(what, crops, staged buffers) of every "stale" staging the GPU file makes"""
    out = []
    for family, b in BC.ONE_PASS_CASES:
        cap = BC.default_cap(b)
        out.append((("one pass", family, b), b, BC.stage(BC.case(family, b), cap, "stale", donor=BC.full_donor(b, cap))))
    for b, seq in ((3, BC.SEQUENCE), (16, BC.SEQUENCE), (5, BC.EDGE_SEQUENCE)):
        cases = [BC.case(f, b, s) for f, s in seq]
        staged = BC.stage_sequence(cases, BC.default_cap(b))
        paddings = BC.sequence_paddings(len(cases))
        out += [(("sequence", b, i), b, st) for i, (st, p) in enumerate(zip(staged, paddings)) if p == "stale"]
    b = BC.PAIR_BATCH
    for i, (elem, padding) in enumerate(zip(BC.PAIR_SEQUENCE, BC.PAIR_PADDINGS)):
        for side, (family, seed) in enumerate(elem):
            cap = b * BC.PAIR_CAPS[side]
            if padding == "stale":
                c = BC.pair_case(side, family, b, seed)
                out.append((("pair", i, side), b, BC.stage(c, cap, "stale", donor=BC.full_donor(b, cap))))
    return out


def test_every_stale_staging_leaves_rows_that_look_live(oracle):
    """behind the live count of every "stale" staging lie in-grid voxel rows with a valid crop id, finite features and valid
    rules -- rows a kernel that read past *v0_dev would take for live ones: a full-capacity donor for the one-pass and pair
    tests, the element before it in a reused runner's sequence"""
    got = _stale_stagings()
    assert len(got) == 2 + 2 + 2 + 1 + 4
    for what, b, st in got:
        V0, cap = st["v0"], st["occ"].shape[0]
        n = BC.stale_rows(st, b)
        assert n >= 100 and V0 + n <= cap, (what, n)
        if what[0] != "sequence":
            assert n == cap - V0, what                      # the donor fills the capacity
        pad = st["occ"][V0:V0 + n]
        assert pad[:, 0].min() >= 0 and pad[:, 0].max() < b and bool(np.isfinite(st["vox"][V0:V0 + n]).all()), what
        assert bool(st["vox"][V0:V0 + n].any()) and st["v2p"][V0:V0 + n, 0].min() >= 1, what
    # no side of the pair sequence runs out of rows at any level
    for elem in BC.PAIR_SEQUENCE:
        for side, (family, seed) in enumerate(elem):
            assert min(BC.oracle_counts(*BC.pair_case(side, family, BC.PAIR_BATCH, seed).key)) > 0
    d = BC.full_donor(3, 384)
    assert len(np.unique(d["occ"], axis=0)) == 384 and bool((np.diff(d["occ"][:, 0]) >= 0).all())
    assert d["occ"][:, 1:].min() >= 0 and d["occ"][:, 1:].max() < BC.S and set(d["occ"][:, 0]) == {0, 1, 2}
