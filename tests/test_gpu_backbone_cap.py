"""The capacity-mode sparse half (ops.BackboneRunCap: what forward_graphed replays for every one-image call) op by op, on
reused runners.  Cases, paddings and sequences: tests/backbone_cap_cases.py (asserted on the CPU by test_backbone_cap_cases.py).

Nothing compared here is taken from the code under test in the same mode: values come from oracle.graph.backbone /
oracle.graph.point_feats within the project's bound 5e-5 * max(1, max|ref|); exact bits -- the eight counts, the level voxel
rows, the 3-NN results -- come from the exact-mode ops.BackboneRun (and the level rows from the oracle's geometry too), the
rider's from ops.voxelize_fp, and the history-independence bits from an earlier call of the same sequence.

Entry points driven, per part:
  2  one pass, stage by stage (b = 2 "big", b = 5 "edge"; paddings zero / stale / wild, each on a fresh runner whose ws, ws2 and
     levels were filled with a byte pattern first): geometry() -> dcl_backbone_geometry_cap, geometry(voxelize=) ->
     dcl_backbone_geometry_cap_vox, features() -> dcl_backbone_features_cap_split, point_neighbours() ->
     dcl_point_neighbours_cap, point_interpolate() -> dcl_point_interpolate (with the capacities), point_features() ->
     dcl_point_features_cap; dcl_backbone_level_info(batch, S, V0_cap, m) for the level rows
  3  one runner per side, many calls (b = 3, b = 16: big, tiny, lopsided, big', tiny, big; b = 5: edge, big, edge), launch by
     launch and as ONE torch.cuda.graph captured from the first element and replayed for every element: the same five entry points
  4  ops.backbone_features_pair on two BackboneRunCap of capacities b * 512 and b * 128 -> dcl_backbone_features_pair_split with
     counts_dev, four elements on one pair of runners
  5  the switches that go by crop count, by the diagnostic library's launch census (one single-side pass per batch):
       stem          13 crops k_sparse_conv_stem<7, 16, 4> (four lanes per row), 14 crops k_sparse_conv_stem<7, 16, 1>
       row order     14 crops k_order_masks + k_order_windows, 13 crops neither
       geometry      8 crops and 16 crops of capacity 16 * 512: k_geometry_small; 17 crops and 16 crops of capacity 16 * 2304:
                     k_mark_rows, k_fill_perm, k_mask_chain64, k_enumerate_sets; the two routes of 16 crops: the same bits
       few / many    2 crops: k_sparse_conv_dma<16, 4, 1, 1, false> and the 64-row tiles <.., 2, 2, ..> on every wider layer, no
                     k_sparse_conv_wlds; 8 crops: k_sparse_conv_wlds<16, 32, true> on level 0 (8 x 3600 > 24576), level 1 still on
                     k_sparse_conv_dma<32, 2, 2, 1, false> (8 x 1800); 14 crops: level 1 on k_sparse_conv_wlds<32, 32, false> and
                     k_sparse_conv_dma<32, 4, 2, 1, false> (14 x 1800 > 24576)
       split-bf16    FINDING: ops.CONV_SPLIT_WIDTHS lists no layer for 16 crops.  Every threshold is the layer's expected rows at
                     32 crops, so the switch sits between 31 and 32 crops for all five layers at once: 32 crops run
                     k_sparse_conv_dma_split<32 | 64 | 128, 4, 1, 2, ..> on exactly the layers computed from the table, 31, 16
                     and 14 crops run none.  The batches of 31 / 32 crops are "small" (60 voxels a crop).
Two facts about the cases: a one-voxel crop does not keep one row per level (each dilating conv grows its set again, to about a
hundred rows at the deep levels), and a crop that has a voxel keeps a row at every level, so "lopsided"'s last crop is empty
at every level and no side of a pair launch ever runs out of rows.  And one about the pair launch: a side's last bits DO depend
on how many live rows the other side holds (see part 4's test).

Measured on an MI355X (each test prints its figures before it asserts; pytest -s shows them).  The whole file, its oracle
passes included: 27 tests in 17.0 s, the slowest (the launch-by-launch sequence of 16 crops, four oracle passes) 2.6 s, every
census batch about 1 s or less.  Largest error over the bound 5e-5 * max(1, max|ref|), level features / read-out, per batch size:
    part 2   b = 2: 0.008 / 0.005     b = 5: 0.009 / 0.004
    part 3   b = 3: 0.008 / 0.006     b = 5: 0.009 / 0.005     b = 16: 0.011 / 0.005   (both sides; graph replays: same bits)
    part 4   b = 3: 0.007 (features only)
    part 5   b = 2: 0.008 / 0.005   8: 0.007 / 0.005   13: 0.008 / 0.004   14: 0.009 / 0.006   16: 0.010 / 0.005   17: 0.011 / 0.005
             31: 0.007 / 0.005   32 (split-bf16 layers): 0.012 / 0.009
-- the existing bound leaves two orders of magnitude of room at these sizes; what is sharp here are the bit-for-bit comparisons."""
import ctypes

import numpy as np
import pytest
import torch

import backbone_cap_cases as BC
from test_gpu_ops import enter_diag
from test_kernel_census import census

pytestmark = pytest.mark.gpu

S = BC.S
BYTE_PATTERNS = {"zero": 0xFF, "stale": 0x7F, "wild": 0xA5}       # first content of ws / ws2 / levels (torch.empty: anything goes)
KEYS = ("counts", "rows", "rider", "levels", "d2", "idx", "pf", "pf2")


def dev(a, dtype=None):
    t = torch.from_numpy(np.array(a))
    return (t if dtype is None else t.to(dtype)).cuda()


class Ctx(object):
    """the network's folded weights and the references, each computed once per case and handed out unchanged"""

    def __init__(self, dcl):
        self.dcl, self.ops = dcl, dcl.ops
        net = dcl.DCL_Net.Network(dcl.synth.default_cfg(64, 64), mode="test")
        self.sd = dcl.synth.synth_state_dict(net, 7)
        net.load_state_dict(self.sd)
        self.net = net.cuda().eval()
        self.f = self.net._fold()
        self.worst = {}                                   # (part, b) -> [feature error / bound, read-out error / bound]
        self._oracle, self._exact = {}, {}

    def oracle(self, key, side="inp"):
        """-> ([(features, rows)] * 4, read-out (n, 480)) of the case through the oracle graph"""
        if (key, side) not in self._oracle:
            from oracle import graph as G
            c = BC.case(*key)
            levels = G.backbone(self.sd, "backbone_" + side, c.vox.copy(), c.occ.copy(), [S] * 3, c.b)
            pf = G.point_feats(torch.from_numpy(c.pts.copy()), levels, [BC.UNIT] * 3, [S] * 3).numpy()
            self._oracle[(key, side)] = (levels, pf)
        return self._oracle[(key, side)]

    def exact(self, key):
        """-> (counts, level rows, dist2, idx) of the case from the EXACT-mode runner (fresh buffers sized by the data)"""
        if key not in self._exact:
            c = BC.case(*key)
            run = self.ops.BackboneRun(dev(c.occ), c.b, S)
            counts = run.counts_dev.cpu().tolist()
            run.set_counts(counts)
            rows = [run.level_indices(m).clone() for m in range(4)]
            d2, idx = run.point_neighbours(dev(c.pts), BC.EXTENTS, BC.OFFSET)
            self._exact[key] = (counts, rows, d2, idx)
        return self._exact[key]

    def note(self, part, b, feat, read):
        w = self.worst.setdefault((part, b), [0.0, 0.0])
        w[0], w[1] = max(w[0], feat), max(w[1], read)


@pytest.fixture(scope="module")
def ctx(dcl, oracle):
    c = Ctx(dcl)
    yield c
    for (part, b), (feat, read) in sorted(c.worst.items()):
        print("\n[backbone cap] part %s b=%d: worst feature error %.3f of the bound, worst read-out error %.3f of the bound"
              % (part, b, feat, read))


class Runner(object):
    """one BackboneRunCap with its static buffers (what Network._capture keeps per side)"""

    def __init__(self, ctx, b, V0_cap, side="inp", pattern=None):
        ops, n = ctx.ops, b * BC.N_PER
        self.ctx, self.b, self.cap, self.side = ctx, b, V0_cap, side
        self.occ = torch.zeros((V0_cap, 4), dtype=torch.int32, device="cuda")
        self.vox = torch.zeros((V0_cap, 7), device="cuda")
        self.v2p = torch.zeros((V0_cap, 1 + BC.MAX_ACTIVE), dtype=torch.int32, device="cuda")
        self.v0 = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.feats = torch.zeros((n, 7), device="cuda")
        self.pts = torch.zeros((n, 4), device="cuda")
        self.d2 = torch.zeros((4, n, 3), device="cuda")
        self.idx = torch.zeros((4, n, 3), dtype=torch.int32, device="cuda")
        self.pf, self.pf2 = torch.zeros((n, 480), device="cuda"), torch.zeros((n, 480), device="cuda")
        self.run = ops.BackboneRunCap(self.occ, self.v0, b, S)
        self.tmp = torch.empty(self.run.tmp_bytes(n), dtype=torch.uint8, device="cuda")
        self.ptrs = ctx.f["backbone_%s_ptrs" % side]
        self.rider = None
        if pattern is not None:                          # before the first call only: tickets and exchange words are the library's
            self.run.ws.fill_(pattern)
            self.run.ws2.fill_(pattern)
            for t in self.run.levels:
                t.view(torch.uint8).fill_(pattern)

    def load(self, c, staged):
        """overwrite the static inputs (the host staging of a replay)"""
        self.case = c
        self.occ.copy_(dev(staged["occ"]))
        self.vox.copy_(dev(staged["vox"]))
        self.v2p.copy_(dev(staged["v2p"]))
        self.v0.fill_(staged["v0"])
        self.feats.copy_(dev(c.feats))
        self.pts.copy_(dev(c.pts))

    def body(self):
        """a whole pass; only enqueues work (capturable)"""
        r = self.run
        self.rider = r.geometry(voxelize=(self.feats, self.v2p, 4))
        r.features(self.vox, *self.ptrs)
        r.point_neighbours(self.pts, BC.EXTENTS, BC.OFFSET, self.d2, self.idx)
        r.point_interpolate(self.d2, self.idx, self.pf2)
        r.point_features(self.pts, BC.EXTENTS, BC.OFFSET, self.pf, self.tmp)

    def level_rows(self, m, n):
        off, _, _ = self.ctx.dcl._native.query("dcl_backbone_level_info", self.b, S, self.cap, m,
                                               ctype=(ctypes.c_int64, ctypes.c_int64, ctypes.c_int32))
        return self.run.ws[off:off + 16 * n].view(torch.int32).view(n, 4)

    def snapshot(self):
        """the live results of the pass just run, cloned"""
        torch.cuda.synchronize()
        counts = self.run.counts_dev.cpu().tolist()
        V0 = self.case.occ.shape[0]
        out = {"counts": counts, "rows": [self.level_rows(m, counts[2 * m + 1]).clone() for m in range(4)],
               "levels": [self.run.levels[m][:counts[2 * m + 1]].clone() for m in range(4)],
               "rider": None if self.rider is None else self.rider[:V0].clone(),
               "d2": self.d2.clone(), "idx": self.idx.clone(), "pf": self.pf.clone(), "pf2": self.pf2.clone()}
        return out


def equal_bits(x, y):
    """bit for bit (the read-out rows of a crop without voxels are NaN: the reference interpolates garbage there, and so do we)"""
    if x.is_floating_point():
        x, y = x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)
    return torch.equal(x, y)


def same_bits(a, b, keys=KEYS, what=""):
    for k in keys:
        x, y = a[k], b[k]
        if isinstance(x, list):
            assert len(x) == len(y), (what, k)
            for m, (p, q) in enumerate(zip(x, y)):
                assert (p == q) if isinstance(p, int) else equal_bits(p, q), (what, k, m)
        else:
            assert equal_bits(x, y), (what, k)


def check(ctx, snap, c, part, side="inp", readout=True):
    """one pass against the exact-mode runner and the oracle"""
    counts, rows, d2, idx = ctx.exact(c.key)
    (want, want_pf), osets = ctx.oracle(c.key, side), BC.oracle_sets(*c.key)
    tag = (part, c.key)
    assert snap["counts"] == counts == BC.oracle_counts(*c.key), tag
    feat_ratio = 0.0
    for m in range(4):
        n = counts[2 * m + 1]
        assert torch.equal(snap["rows"][m], rows[m]), tag + (m,)
        assert np.array_equal(snap["rows"][m].cpu().numpy(), osets[2 * m + 1]), tag + (m,)
        assert np.array_equal(want[m][1], osets[2 * m + 1])
        got = snap["levels"][m].cpu().numpy()
        assert got.shape == want[m][0].shape == (n, ctx.ops.BACKBONE_CHANNELS[2 * m + 2]), tag + (m,)
        assert bool(np.isfinite(got).all()), tag + (m,)
        bound = 5e-5 * max(1.0, float(np.abs(want[m][0]).max()))
        err = float(np.abs(got - want[m][0]).max())
        feat_ratio = max(feat_ratio, err / bound)
        print("[backbone cap] %s level %d: feature error %.3g, bound %.3g" % (tag, m, err, bound))
        assert err <= bound, tag + (m, err, bound)
    if snap["rider"] is not None:
        V0 = c.occ.shape[0]
        assert torch.equal(snap["rider"], ctx.ops.voxelize_fp(dev(c.feats), dev(c.v2p), 4)[:V0]), tag
        assert V0 == 0 or float(snap["rider"].abs().sum()) > 0
    if not readout:
        ctx.note(part, c.b, feat_ratio, 0.0)
        return
    live = torch.from_numpy(~BC.excluded_points(c)).cuda()
    assert torch.equal(snap["d2"][:, live], d2[:, live]) and torch.equal(snap["idx"][:, live], idx[:, live]), tag
    for m in range(4):                                    # every point, those of a crop without voxels included
        i = snap["idx"][m]
        assert int(i.min()) >= 0 and int(i.max()) < max(counts[2 * m + 1], 1), tag + (m,)
    assert equal_bits(snap["pf"], snap["pf2"]) and bool(torch.isfinite(snap["pf"][live]).all()), tag
    got, lv = snap["pf"].cpu().numpy(), live.cpu().numpy()
    bound = 5e-5 * max(1.0, float(np.abs(want_pf[lv]).max()))
    err = float(np.abs(got[lv] - want_pf[lv]).max())
    print("[backbone cap] %s read-out error %.3g, bound %.3g" % (tag, err, bound))
    ctx.note(part, c.b, feat_ratio, err / bound)
    assert err <= bound, tag + (err, bound)


# --------------------------------------------------------------------------------- 2. one pass, stage by stage
@pytest.mark.parametrize("family,b", BC.ONE_PASS_CASES)
def test_one_capacity_pass_stage_by_stage(ctx, family, b):
    """every stage of one capacity pass on a pattern-filled fresh runner, under the three paddings: counts, level rows, rider,
    level features, 3-NN, both read-out forms; the rows of `levels` past the live counts never reach the read-out; the three
    paddings give the same bits"""
    c = BC.case(family, b)
    cap = BC.default_cap(b)
    donor = BC.full_donor(b, cap)                         # every row behind the live count looks like a live voxel
    snaps = {}
    for padding in BC.PADDINGS:
        R = Runner(ctx, b, cap, pattern=BYTE_PATTERNS[padding])
        staged = BC.stage(c, cap, padding, donor=donor)
        assert (BC.stale_rows(staged, b) == cap - c.occ.shape[0]) == (padding == "stale")
        R.load(c, staged)
        # geometry without the rider, then with it: same counts, same rows
        R.run.geometry()
        plain = R.snapshot()
        R.body()
        snap = R.snapshot()
        same_bits(plain, snap, keys=("counts", "rows"), what=(padding, "rider or not"))
        check(ctx, snap, c, "2")
        # rows of `levels` past the live counts: NaN, then 1e30 -- the interpolation reads neither
        for fill in (float("nan"), 1e30):
            for m in range(4):
                R.run.levels[m][snap["counts"][2 * m + 1]:] = fill
            R.pf2.fill_(7.0)
            R.run.point_interpolate(R.d2, R.idx, R.pf2)
            live = torch.from_numpy(~BC.excluded_points(c)).cuda()
            assert equal_bits(R.pf2, snap["pf"]) and bool(torch.isfinite(R.pf2[live]).all()), (padding, fill)
            R.pf.fill_(7.0)
            R.run.point_features(R.pts, BC.EXTENTS, BC.OFFSET, R.pf, R.tmp)
            assert equal_bits(R.pf, snap["pf"]), (padding, fill)
        snaps[padding] = snap
    for padding in BC.PADDINGS[1:]:
        same_bits(snaps["zero"], snaps[padding], what=padding)


# --------------------------------------------------------------------------------- 3. one runner, many calls
_LAUNCHED = {}


def _sequence(b):
    seq, repeats = (BC.EDGE_SEQUENCE, BC.EDGE_REPEATS) if b == 5 else (BC.SEQUENCE, BC.SEQUENCE_REPEATS)
    cases = [BC.case(f, b, s) for f, s in seq]
    return cases, BC.stage_sequence(cases, BC.default_cap(b)), repeats


def _launch_by_launch(ctx, b, side):
    if (b, side) not in _LAUNCHED:
        cases, staged, _ = _sequence(b)
        R = Runner(ctx, b, BC.default_cap(b), side=side, pattern=0xC3)
        snaps = []
        for c, st in zip(cases, staged):
            R.load(c, st)
            R.body()
            snaps.append(R.snapshot())
        _LAUNCHED[(b, side)] = snaps
    return _LAUNCHED[(b, side)]


@pytest.mark.parametrize("side", ["inp", "tmp"])
@pytest.mark.parametrize("b", [3, 5, 16])
def test_reused_runner_launch_by_launch(ctx, b, side):
    """ONE runner of a side (its backbone's weights) and one set of static buffers through big, tiny, lopsided, big', tiny, big
    (b = 5: edge, big, edge), paddings cycling: every element as a fresh pass would give it, and a case that comes back gives the
    bits it gave before -- whatever ran in between (occupancy masks, prefixes, split-K slots and tickets, exchange words,
    row-order tables all outlive a call)"""
    cases, _, repeats = _sequence(b)
    snaps = _launch_by_launch(ctx, b, side)
    for c, snap in zip(cases, snaps):
        check(ctx, snap, c, "3", side=side)
    for late, early in repeats:
        same_bits(snaps[late], snaps[early], what=("element", late, "against", early))


@pytest.mark.parametrize("side", ["inp", "tmp"])
@pytest.mark.parametrize("b", [3, 5, 16])
def test_reused_runner_as_one_captured_graph(ctx, b, side):
    """the same sequence as replays of ONE torch.cuda.graph captured from the first element (two warm-up passes on a side
    stream, then the capture, as Network._capture does), the static inputs overwritten before each replay: bit for bit the
    launch-by-launch results, element by element"""
    cases, staged, repeats = _sequence(b)
    want = _launch_by_launch(ctx, b, side)
    R = Runner(ctx, b, BC.default_cap(b), side=side, pattern=0x3C)
    R.load(cases[0], staged[0])
    with torch.no_grad():
        warm = torch.cuda.Stream()
        warm.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(warm):
            for _ in range(2):
                R.body()
        torch.cuda.current_stream().wait_stream(warm)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            R.body()
    snaps = []
    for c, st in zip(cases, staged):
        R.load(c, st)
        g.replay()
        snaps.append(R.snapshot())
    for i, (snap, w) in enumerate(zip(snaps, want)):
        same_bits(snap, w, what=("replay", i))
    for late, early in repeats:
        same_bits(snaps[late], snaps[early], what=("replay", late, "against", early))
    check(ctx, snaps[0], cases[0], "3g", side=side)


# --------------------------------------------------------------------------------- 4. both sides in one launch sequence
@pytest.mark.parametrize("b", [BC.PAIR_BATCH])
def test_pair_launch_in_capacity_mode_on_reused_runners(ctx, b):
    """ops.backbone_features_pair on two BackboneRunCap of different capacities (b * 512 and b * 128), four elements on the same
    two runners: each side's counts and rows bit for bit, its levels within the bound of the oracle and of its own single-side
    capacity pass; an element that comes back (the last is the first again, under another padding) gives both sides the bits it
    gave before.

    What does NOT hold, and is therefore not asserted: that a side's bits are independent of the other side.  The stream-K unit
    range of a pair launch runs over both sides' live tiles (csrc/conv_body.h: total = units0 + units1, U = ceil(total / G)), so
    where a side's chunk segments are cut -- the order of its partial sums -- follows the other side's live rows.  The result is
    deterministic for a given pair (the repeat above) and stays within the bound of the oracle; how far side a's levels move
    with what side b holds is printed (MI355X: 0.0044 of the 5e-5 bound).  A side that runs out of rows at a level does not
    occur: a crop that holds a voxel keeps a row at every level (tests/test_backbone_cap_cases.py)."""
    sides = ("inp", "tmp")
    caps = {s: b * per for s, per in zip(sides, BC.PAIR_CAPS)}
    runs = {s: Runner(ctx, b, caps[s], side=s, pattern=0x5A) for s in sides}
    solo = {s: Runner(ctx, b, caps[s], side=s, pattern=0xE1) for s in sides}
    donors = {s: BC.full_donor(b, caps[s]) for s in sides}
    gots = []
    for i, (elem, padding) in enumerate(zip(BC.PAIR_SEQUENCE, BC.PAIR_PADDINGS)):
        cs = {}
        for j, (s, (fam, seed)) in enumerate(zip(sides, elem)):
            c = cs[s] = BC.pair_case(j, fam, b, seed)
            staged = BC.stage(c, caps[s], padding, donor=donors[s])
            assert (BC.stale_rows(staged, b) == caps[s] - c.occ.shape[0]) == (padding == "stale")
            for R in (runs[s], solo[s]):
                R.load(c, staged)
                R.rider = None
                R.run.geometry()
        a, t = runs["inp"], runs["tmp"]
        ctx.ops.backbone_features_pair(a.run, a.vox, a.ptrs, t.run, t.vox, t.ptrs)
        got = {s: runs[s].snapshot() for s in sides}
        for s in sides:
            solo[s].run.features(solo[s].vox, *solo[s].ptrs)
            alone = solo[s].snapshot()
            same_bits(got[s], alone, keys=("counts", "rows"), what=(i, s))
            check(ctx, got[s], cs[s], "4", side=s, readout=False)
            check(ctx, alone, cs[s], "4", side=s, readout=False)
            for m in range(4):
                w = alone["levels"][m]
                assert float((got[s]["levels"][m] - w).abs().max()) <= 5e-5 * max(1.0, float(w.abs().max())), (i, s, m)
        gots.append(got)
    shift = 0.0
    for i, got in enumerate(gots):                        # side a holds the same batch throughout
        same_bits(got["inp"], gots[0]["inp"], keys=("counts", "rows"), what=("side a, element", i))
        for m in range(4):
            w = gots[0]["inp"]["levels"][m]
            shift = max(shift, float((got["inp"]["levels"][m] - w).abs().max()) / (5e-5 * max(1.0, float(w.abs().max()))))
    print("[backbone cap] part 4: side a's levels move by at most %.4f of the bound with what side b holds" % shift)
    last = len(BC.PAIR_SEQUENCE) - 1
    assert BC.PAIR_SEQUENCE[last] == BC.PAIR_SEQUENCE[0] and BC.PAIR_PADDINGS[last] != BC.PAIR_PADDINGS[0]
    for s in sides:                                       # the first element again, after two others: its bits again
        same_bits(gots[last][s], gots[0][s], keys=("counts", "rows", "levels"), what=("element", last, s))


# --------------------------------------------------------------------------------- 5. the switches that go by crop count
def _dma(seen, split=False):
    """{(CIN, WR, WCW, NT): launches} of the LDS-DMA conv kernel's instances (natural and ordered rows together)"""
    out = {}
    name = "k_sparse_conv_dma_split<" if split else "k_sparse_conv_dma<"
    for k, n in seen.items():
        if k.startswith(name):
            a = tuple(int(v) for v in k[len(name):-1].split(",")[:4])
            out[a] = out.get(a, 0) + n
    return out


_CENSUS = {}


def _census_pass(request, ctx, family, b, per_crop):
    """one capacity pass (wild padding, pattern-filled fresh runner) on the diagnostic library -> (census of the pass, results)"""
    key = (family, b, per_crop)
    if key not in _CENSUS:
        lib = enter_diag(ctx.dcl, request)
        c = BC.case(family, b)
        R = Runner(ctx, b, b * per_crop, pattern=0x96)
        R.load(c, BC.stage(c, b * per_crop, "wild"))
        torch.cuda.synchronize()
        lib.dcl_debug_launch_census_reset()
        R.body()
        snap = R.snapshot()
        seen = {k: n for k, n in census(lib).items() if n > 0}
        print("[backbone cap] census %s b=%d cap=%d: %s" % (family, b, b * per_crop, sorted(seen.items())))
        _CENSUS[key] = (seen, snap)
    return _CENSUS[key]


@pytest.mark.parametrize("family,b,per_crop", BC.CENSUS_CASES)
def test_forms_by_crop_count(request, ctx, family, b, per_crop):
    """one capacity pass per batch on the diagnostic library, checked like part 2, with the launch census of the pass: which
    kernel instances ran (see the module docstring for the table)"""
    ops, cap = ctx.ops, b * per_crop
    seen, snap = _census_pass(request, ctx, family, b, per_crop)
    check(ctx, snap, BC.case(family, b), "5")
    dma, split = _dma(seen), _dma(seen, split=True)
    rows = ops.CONV_SPLIT_ROWS_PER_CROP
    # the stem: a lane per row above 49152 expected rows (crops x 3600: from 14 crops on)
    lane_per_row = b * rows[0] > BC.STEM_LANE_PER_ROW_ABOVE
    assert ("k_sparse_conv_stem<7, 16, 1>" in seen) == lane_per_row
    assert ("k_sparse_conv_stem<7, 16, 4>" in seen) == (not lane_per_row)
    # row orders of the deep levels from 14 crops on
    ordered = b >= BC.ORDER_MIN_BATCH
    assert ("k_order_masks" in seen and "k_order_windows" in seen) == ordered
    assert any(k.startswith("k_order_") for k in seen) == ordered
    # the geometry stage: one launch up to 8 crops, and up to 16 while the capacity stays within 32768 rows
    small = b <= BC.GEO_SMALL_ANY_ROWS or (b <= BC.GEO_SMALL_BATCH and cap <= BC.GEO_SMALL_ROWS)
    assert ("k_geometry_small" in seen) == small
    for k in ("k_mark_rows", "k_fill_perm", "k_mask_chain64", "k_enumerate_sets"):
        assert (k in seen) == (not small), k
    # split-bf16: exactly the layers the table lists for this many crops (one launch per layer, instances by Cin)
    want = {}
    for cin, cout, subm in BC.split_layers(ops, b):
        want[(cin, 4, 1, 2)] = want.get((cin, 4, 1, 2), 0) + 1
    assert split == want and (bool(want) == (b >= BC.split_switch_batch(ops)))
    # few-row and many-row forms (24576 expected rows; ordered launches: 6144)
    few = [b * r <= BC.FEW_ROWS for r in rows]
    assert any(k.startswith("k_sparse_conv_wlds<16, 32, true>") for k in seen) == (not few[0])
    assert ((16, 4, 1, 1) in dma) == few[0]
    assert any(k.startswith("k_sparse_conv_wlds<32, 32, false>") for k in seen) == (not few[1])
    assert ((32, 4, 1, 1) in dma) == few[1]
    if (32, 64, True) not in BC.split_layers(ops, b):
        assert ((32, 2, 2, 1) in dma) == few[1] and ((32, 4, 2, 1) in dma) == (not few[1])
    if b == 2:
        assert set(dma) == {(16, 4, 1, 1), (32, 4, 1, 1), (32, 2, 2, 1), (64, 2, 2, 1), (64, 2, 2, 2), (128, 2, 2, 2)}
        assert not any(k.startswith("k_sparse_conv_wlds") for k in seen)


def test_the_two_geometry_routes_of_16_crops_give_the_same_bits(request, ctx):
    """k_geometry_small (capacity 16 * 512) against the separate launches (capacity 16 * 2304) on the same batch"""
    a, b = _census_pass(request, ctx, "big", 16, 512), _census_pass(request, ctx, "big", 16, 2304)
    assert "k_geometry_small" in a[0] and "k_geometry_small" not in b[0]
    same_bits(a[1], b[1], keys=("counts", "rows", "rider", "d2", "idx"))
