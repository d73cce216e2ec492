"""The folded read-out on the GPU: dcl_linear_split_gather_fwd (csrc/linear_split.hip, EPI 4) and dcl_point_features_fold
(csrc/interp.hip, csrc/backbone.hip) against float64 twins, against today's route, on exact operands, inside guard bands, with
a NaN in one gathered row, and through a whole forward.  Operands, twins and the bound: tests/readout_fold_cases.py; the CPU side
of the same cases: tests/test_readout_fold_model.py.  Every test prints its figures (pytest -s) before it asserts; the figures are
kept in profiles/readout_fold.txt."""
import numpy as np
import pytest
import torch

import guard_arena as GA
import readout_fold_cases as RF
import test_gpu_network as TN
import test_gpu_ops as TO

pytestmark = pytest.mark.gpu


def report(case, **figures):
    print("readout-fold\t%s\t%s" % (case, "\t".join("%s=%s" % (k, ("%.4g" % v) if isinstance(v, float) else v) for k, v in figures.items())))


def pitched(t, extra, lead=0):
    """t on the GPU as a column block of a wider buffer: row pitch = width + extra, first column `lead`"""
    wide = torch.full((t.shape[0], t.shape[1] + extra), 7.0, dtype=t.dtype).cuda()
    view = wide[:, lead:lead + t.shape[1]]
    view.copy_(t)
    return view


def gather_tables(dcl, F, Wl, pitch_extra=16):
    """G_l = F_l @ W_l on the fp32-MFMA core (c_l accumulations per output), written into buffers of a larger row pitch"""
    out = []
    for f, w in zip(F, Wl):
        buf = torch.full((f.shape[0], w.shape[1] + pitch_extra), 7.0).cuda()
        out.append(dcl.ops.linear_dma(f.cuda(), w.cuda(), out=buf[:, :w.shape[1]]))
    return out


# ------------------------------------------------------------------------------------------- the gather GEMM against float64
@pytest.mark.parametrize("K,nfold,R", RF.GATHER_KFR)
@pytest.mark.parametrize("M,N", RF.GATHER_MN)
def test_gather_gemm_against_its_float64_twin(dcl, M, N, K, nfold, R):
    """One, ragged and three row tiles; one whole and a ragged column tile; one chunk of K and fourteen; one and two folded
    levels; tables of 7 rows (every row shared by many points) and of 300; every operand with a row pitch larger than its
    width.  Per output |err| <= gather_bound units of 2^-24 (sum |x||w| + sum_l,i fw sum |F||W| + |bias|): the count of roundings
    written out in readout_fold_cases.gather_bound.  ReLU on every second case (it widens no error)."""
    x, W0, bias, F, Wl, fw, fi = RF.gather_case(M, N, K, nfold, R)
    relu = bool((M + N + K + nfold + R) & 1)
    G = gather_tables(dcl, F, Wl)
    y = pitched(torch.zeros(M, N), 24, 8)
    got = dcl.ops.linear_split_gather(pitched(x, 8, 4), dcl.ops.SplitWeight(W0.cuda()), bias.cuda(), fw.cuda(), fi.cuda(), G, relu, out=y)
    assert got.data_ptr() == y.data_ptr()
    want, mag = RF.gather_reference(x, W0, bias, F, Wl, fw, fi)
    units, bound = RF.gather_units(got.cpu(), want, mag, relu), RF.gather_bound(K, RF.GATHER_C[nfold])
    report("gather M=%d N=%d K=%d nfold=%d R=%d relu=%d" % (M, N, K, nfold, R, relu), units=units, bound=bound)
    assert units <= bound
    wide = y._base if y._base is not None else y
    assert bool((wide[:, :8] == 7.0).all()) and bool((wide[:, 8 + N:] == 7.0).all())          # the neighbours of the column block


# ------------------------------------------------------------------------------------------- both routes of the first layer
@pytest.fixture(scope="module")
def routes(dcl):
    """today's route on the Gaussian case -- the read-out's interpolation kernels, then dcl_linear_split_fwd at K = 480 -- and its
    operands on the GPU; computed once"""
    F, W, bias, w, idx = RF.route_case()
    Fd, Wd, bd = [f.cuda() for f in F], W.cuda(), bias.cuda()
    pf = torch.empty(RF.ROUTE_M, 480).cuda()
    for m in range(4):
        dcl.ops.three_interpolate_sp(Fd[m], idx[m].cuda().contiguous(), w[m].cuda().contiguous(), out=pf[:, RF.COL[m]:RF.COL[m + 1]])
    today = dcl.ops.linear_split(pf, dcl.ops.SplitWeight(Wd), bd)
    return dict(F=Fd, W=Wd, bias=bd, pf=pf, today=today.cpu(), want=RF.unfolded_reference(F, W, bias, w, idx))


def folded_route(dcl, F, W, bias, pf, w, idx, nfold, relu=False):
    """the folded route as models/DCL_Net.py runs it: G_m = ops.linear(F_m, row block of W), the GEMM over the first columns of the
    read-out with the gather epilogue"""
    k0 = RF.K0[nfold]
    G = [dcl.ops.linear(F[m], W[RF.COL[m]:RF.COL[m + 1]]) for m in range(4 - nfold, 4)]
    return dcl.ops.linear_split_gather(pf[:, :k0], dcl.ops.SplitWeight(W[:k0]), bias, w[4 - nfold:].cuda().contiguous(),
                                       idx[4 - nfold:].cuda().contiguous(), G, relu)


@pytest.mark.parametrize("nfold", (1, 2))
def test_folded_route_is_as_accurate_as_todays(dcl, routes, nfold):
    """Gaussian operands, 768 points, 192 columns, tables of 300 rows: max |folded - float64| <= 1.5 max |today's - float64| (the
    margin DESIGN 5c grants a re-associated form).  Measured on an MI355X (profiles/readout_fold.txt)."""
    F, W, bias, w, idx = RF.route_case()
    got = folded_route(dcl, routes["F"], routes["W"], routes["bias"], routes["pf"], w, idx, nfold).cpu()
    e_today = float((routes["today"].double() - routes["want"]).abs().max())
    e_folded = float((got.double() - routes["want"]).abs().max())
    report("route nfold=%d" % nfold, today=e_today, folded=e_folded, ratio=e_folded / e_today, allowed=RF.ROUTE_OVER_TODAY)
    assert e_folded <= RF.ROUTE_OVER_TODAY * e_today


@pytest.mark.parametrize("relu", (False, True))
@pytest.mark.parametrize("nfold", (1, 2))
def test_exact_operands_fold_bit_for_bit(dcl, nfold, relu):
    """small integers, weights 0.5 / 0.25 / 0.25: nothing rounds on either route, so the folded kernel, today's kernels and float64
    agree in every bit (a kernel that drops a neighbour or a level does not: tests/test_readout_fold_model.py)"""
    F, W, bias, w, idx = RF.exact_case()
    Fd, Wd, bd = [f.cuda() for f in F], W.cuda(), bias.cuda()
    pf = torch.empty(RF.EXACT_M, 480).cuda()
    for m in range(4):
        dcl.ops.three_interpolate_sp(Fd[m], idx[m].cuda().contiguous(), w[m].cuda().contiguous(), out=pf[:, RF.COL[m]:RF.COL[m + 1]])
    want = RF.unfolded_reference(F, W, bias, w, idx)
    want = torch.relu(want) if relu else want
    today = dcl.ops.linear_split(pf, dcl.ops.SplitWeight(Wd), bd, relu).cpu()
    got = folded_route(dcl, Fd, Wd, bd, pf, w, idx, nfold, relu).cpu()
    assert torch.equal(today.double(), want)
    assert torch.equal(got.double(), want)


# ------------------------------------------------------------------------------------------- the read-out variant
@pytest.fixture(scope="module")
def readout(dcl):
    """a backbone pass over crops with voxels on the grid's edges (tests/test_gpu_ops.py: _edge_voxels) and a few thousand points:
    the full read-out, its two halves, and what the fold needs; computed once"""
    rng = np.random.default_rng(41)
    occ, b = TO._edge_voxels(rng)
    unit = 0.006
    off = float(np.float32(-0.5 * unit * 64))
    extents = [float(np.float32(unit * sc)) for sc in (2, 4, 6, 8)]
    q = []
    for bi in range(b):
        own = occ[occ[:, 0] == bi][:, 1:4].astype(np.float32)
        if len(own):
            pick = own[rng.integers(0, len(own), 700)]
            q.append(np.c_[np.full(700, bi), (pick + rng.uniform(0, 1, pick.shape)) * unit + off])
            q.append(np.c_[np.full(40, bi), rng.uniform(-0.3, 0.3, (40, 3))])                  # isolated and out-of-grid queries
    pb4 = TO.cuda(np.concatenate(q).astype(np.float32))
    net = dcl.DCL_Net.Network(dcl.synth.default_cfg(64, 64), mode="test")
    net.load_state_dict(dcl.synth.synth_state_dict(net, 5))
    f = net.cuda().eval()._fold()
    run = dcl.ops.BackboneRun(TO.cuda(occ), b, 64)
    run.set_counts(run.counts_dev.cpu().tolist())
    run.features(TO.cuda(rng.normal(size=(occ.shape[0], 7)).astype(np.float32)), *f["backbone_inp_ptrs"])
    d2, idx = run.point_neighbours(pb4, extents, off)
    return dict(run=run, pb4=pb4, extents=extents, off=off, full=run.point_features(pb4, extents, off), d2=d2.cpu(), idx=idx.cpu(), f=f)


@pytest.mark.parametrize("nfold", (1, 2))
def test_read_out_variant_has_the_bits_of_the_full_read_out(dcl, readout, nfold):
    """its columns are columns 0 .. K0 - 1 of dcl_point_features bit for bit (written into a buffer of a larger pitch, whose other
    columns stay); fi is what dcl_point_neighbours finds; fw has the bits the interpolation's own expressions give: the existing
    interpolation kernel (dcl_three_interpolate_dist2_sp: the same source expressions) run on a one-hot table returns its three
    weights unchanged, w_i at column idx_i.  Beside that, the formula on the CPU -- 1 / (sqrt(d) + 1e-8) over (r0 + r1) + r2 in
    fp32 -- within 6 ulp (five operations between d and a weight, each of which the two machines may round differently by one
    ulp; measured on an MI355X: 17-19 % of the weights differ, by at most 2.5 ulp, profiles/readout_fold.txt)"""
    r = readout
    n, k0 = r["pb4"].shape[0], RF.K0[nfold]
    assert n > 1000 and bool(torch.isfinite(r["full"]).all(1).sum() > 1000)
    wide = torch.full((n, k0 + 12), 7.0).cuda()
    out, fw, fi = r["run"].point_features_fold(r["pb4"], r["extents"], r["off"], nfold, out=wide[:, 4:4 + k0])
    assert bool((wide[:, :4] == 7.0).all()) and bool((wide[:, 4 + k0:] == 7.0).all())
    same = lambda a, b: torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))      # noqa: E731
    assert same(out.cpu(), r["full"][:, :k0].cpu())
    assert torch.equal(fi.cpu(), r["idx"][4 - nfold:])
    for l in range(nfold):
        m = 4 - nfold + l
        idx_m, d2_m = r["idx"][m].cuda().contiguous(), r["d2"][m].cuda().contiguous()
        rows = r["run"].levels[m].shape[0]
        onehot = dcl.ops.three_interpolate_sp(torch.eye(rows, device="cuda"), idx_m, d2_m, from_dist2=True)
        want = torch.gather(onehot, 1, idx_m.long()).cpu()
        found = torch.isfinite(r["d2"][m]).all(1)                        # three distinct rows were found
        assert int(found.sum()) > 1000
        assert same(fw[l].cpu()[found], want[found])
        assert bool(torch.isnan(fw[l].cpu()[~torch.isfinite(r["d2"][m]).any(1)]).all())        # no voxel at all: 0 / 0, as today
        rec = 1.0 / (torch.sqrt(r["d2"][m][found]) + np.float32(1e-8))
        cpu = rec / ((rec[:, 0] + rec[:, 1]) + rec[:, 2]).unsqueeze(1)
        ulp = float(((fw[l].cpu()[found] - cpu).abs() / cpu).max()) * 2.0 ** 23
        report("readout nfold=%d level=%d" % (nfold, m), rows=rows, points=int(found.sum()), cpu_formula_ulp=ulp,
               differing=int((fw[l].cpu()[found] != cpu).sum()))
        assert ulp <= 6.0


def test_read_out_variant_and_gather_gemm_compose_to_the_full_first_layer(dcl, readout):
    """1 and 2 levels of a real read-out folded through a first layer of 192 columns, beside the read-out + K = 480 GEMM.  Both are
    inside their hard bounds of the exact value -- today's 3 (the interpolation's roundings of every x) + 6 * 480 + 2 units, the
    folded route's gather_bound -- so they differ by at most the sum of the two, in units of 2^-24 (sum |pf||w| + |bias|) (the
    features are ReLU outputs and the weights positive: the folded part's magnitude is the unfolded one's)"""
    r = readout
    rows = torch.isfinite(r["full"]).all(1)
    g = torch.Generator().manual_seed(5)
    W, bias = (torch.randn(480, 192, generator=g) * 0.05).cuda(), torch.randn(192, generator=g).cuda()
    today = dcl.ops.linear_split(torch.nan_to_num(r["full"]), dcl.ops.SplitWeight(W), bias, True)[rows].cpu()
    mag = RF.SC.magnitude(r["full"][rows].cpu(), W.cpu(), bias.cpu())
    for nfold in (1, 2):
        out, fw, fi = r["run"].point_features_fold(r["pb4"], r["extents"], r["off"], nfold)
        G = [dcl.ops.linear_dma(r["run"].levels[m], W[RF.COL[m]:RF.COL[m + 1]]) for m in range(4 - nfold, 4)]
        got = dcl.ops.linear_split_gather(out, dcl.ops.SplitWeight(W[:RF.K0[nfold]]), bias, fw, fi, G, True)[rows].cpu()
        units = float(((got.double() - today.double()).abs() / (RF.SC.U * mag)).max())
        bound = (3 + 6 * 480 + 2) + RF.gather_bound(RF.K0[nfold], RF.LEVEL_C[4 - nfold:])
        report("compose nfold=%d" % nfold, units=units, bound=bound)
        assert units <= bound


# ------------------------------------------------------------------------------------------- guard bands, non-finite input
def test_new_entry_points_inside_guard_bands(dcl, readout):
    """both entry points between poisoned bands (tests/guard_arena.py): no stray write around y, out, fw, fi; no read outside G, fw,
    fi, x; ragged tiles (M = 300, N = 192), two folded levels, tables of 7 rows"""
    x, W0, bias, F, Wl, fw, fi = RF.gather_case(300, 192, 16, 2, 7)
    G = [t.contiguous() for t in gather_tables(dcl, F, Wl, 0)]
    mods = GA.allocating_modules(dcl)

    def gemm(x, W0, bias, fw, fi, G0, G1):
        return dcl.ops.linear_split_gather(x, dcl.ops.SplitWeight(W0), bias, fw, fi, [G0, G1], True)
    GA.guarded(gemm, [x.cuda(), W0.cuda(), bias.cuda(), fw.cuda(), fi.cuda(), G[0], G[1]], modules=mods)
    r = readout

    def read(pb4):
        return r["run"].point_features_fold(pb4, r["extents"], r["off"], 2)
    finite = torch.isfinite(r["full"]).all(1)
    GA.guarded(read, [r["pb4"][finite].contiguous()], modules=mods)


def test_a_nan_in_one_gathered_row_reaches_exactly_the_rows_that_name_it(dcl):
    """a NaN in row 3 of G_1: exactly the output rows with a 3 among their level-1 neighbours are NaN (whatever the weight), in every
    column; every other row keeps the bits of the clean launch"""
    M, N, K, nfold, R = 300, 192, 16, 2, 7
    x, W0, bias, F, Wl, fw, fi = RF.gather_case(M, N, K, nfold, R)
    G = gather_tables(dcl, F, Wl)
    args = (x.cuda(), dcl.ops.SplitWeight(W0.cuda()), bias.cuda(), fw.cuda(), fi.cuda())
    clean = dcl.ops.linear_split_gather(*args, G).cpu()
    G[1][3, 5] = float("nan")
    G[1][3, 191] = float("nan")
    got = dcl.ops.linear_split_gather(*args, G).cpu()
    named = (fi[1] == 3).any(1)
    assert 0 < int(named.sum()) < M
    assert bool(torch.isnan(got[named][:, [5, 191]]).all())
    keep = torch.ones(M, N, dtype=torch.bool)
    keep[named.nonzero().flatten()[:, None], torch.tensor([5, 191])] = False
    assert torch.equal(got[keep].view(torch.int32), clean[keep].view(torch.int32))


# ------------------------------------------------------------------------------------------- the whole forward
@pytest.fixture(scope="module")
def forwards(dcl):
    """b = 6 crops of N = M = 1024 points launch by launch (6144 rows: the smallest size the split core takes), the fold's minimum
    point count lowered to that, READOUT_FOLD = 0, 1, 2 and each folded value twice"""
    ops = dcl.ops
    net, _, _ = TN._net(dcl, 1024, 1024, 1, graph_max_batch=0)
    data = dcl.synth.make_batch(6, 1024, 1024)
    keep = (ops.READOUT_FOLD, ops.READOUT_FOLD_MIN_POINTS)
    out, seen = {}, {}
    real = ops.linear_split_gather

    def counting(*a, **k):
        seen[ops.READOUT_FOLD] = seen.get(ops.READOUT_FOLD, 0) + 1
        return real(*a, **k)
    try:
        ops.READOUT_FOLD_MIN_POINTS, ops.linear_split_gather = 6144, counting
        for fold, tag in ((0, "0"), (1, "1"), (1, "1 again"), (2, "2"), (2, "2 again")):
            ops.READOUT_FOLD = fold
            clone = {k: ({kk: vv.clone() for kk, vv in v.items()} if isinstance(v, dict) else v) for k, v in data.items()}
            with torch.no_grad():
                pred = net(clone)
            torch.cuda.synchronize()
            out[tag] = {k: pred[k].cpu() for k in ("rot_pred", "trans_pred", "conf", "F_Xo_p")}
    finally:
        ops.READOUT_FOLD, ops.READOUT_FOLD_MIN_POINTS = keep
        ops.linear_split_gather = real
    out["launches"] = seen
    return out


@pytest.mark.parametrize("fold", (1, 2))
def test_whole_forward_with_folded_read_out(forwards, fold):
    """the pose, the confidence and the per-point features of the folded forward within the tolerances tests/test_gpu_network.py
    uses between graph and eager; the folded route really ran (two gather GEMMs per forward, none with READOUT_FOLD = 0); two
    folded runs give identical bits"""
    base, got, again = forwards["0"], forwards[str(fold)], forwards["%d again" % fold]
    assert forwards["launches"] == {1: 4, 2: 4}
    dR = float((got["rot_pred"] - base["rot_pred"]).abs().max())
    dt = float((got["trans_pred"] - base["trans_pred"]).abs().max())
    dc = float((got["conf"] - base["conf"]).abs().max())
    dF = float((got["F_Xo_p"] - base["F_Xo_p"]).abs().max())
    report("forward fold=%d" % fold, dR=dR, dt=dt, dconf=dc, dF=dF)
    assert dR <= TN.R_TOL and dt <= TN.T_TOL
    assert dc <= 1e-4 * max(1.0, float(base["conf"].abs().max())) and dF <= 1e-4 * max(1.0, float(base["F_Xo_p"].abs().max()))
    for k in got:
        assert torch.equal(got[k].view(torch.int32), again[k].view(torch.int32)), k
