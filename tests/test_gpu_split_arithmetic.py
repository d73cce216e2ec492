"""The split-bf16 kernels (csrc/linear_split.hip: k_linear_split<EPI>; csrc/dense.hip: k_cross_attn_split) on operands chosen
to expose a lost piece product, a leaking ragged row or column, a wrong crop boundary or an un-isolated non-finite value -- each
case beside the fp32 form of the same operation on the same bits, both against float64.  Operands, references and bounds come
from tests/split_cases.py; tests/test_split_model.py shows on the CPU that every bound asserted here holds in a model of the
arithmetic and is violated by a kernel that lost a term.  Bounds are either derived by counting roundings (docstrings) or
relative to a CPU fp32 FMA chain / the fp32 kernel; the figures are kept in profiles/split_arithmetic.txt.  Every test prints
its figures (pytest -s) before it asserts."""
import math

import pytest
import torch

import split_cases as SC
import test_gpu_ops as TO

pytestmark = pytest.mark.gpu
enter_diag, _attn_ref, cuda = TO.enter_diag, TO._attn_ref, TO.cuda


def report(case, **figures):
    print("split-arithmetic\t%s\t%s" % (case, "\t".join("%s=%s" % (k, ("%.3f" % v) if isinstance(v, float) else v)
                                                         for k, v in figures.items())))


def fp32_linear(dcl, x, Wt, bias=None, relu=False):
    """the fp32-MFMA core on the same operands; it takes K in whole 32-chunks only, so a K = 16 layer gets 16 zero columns of x
    and 16 zero rows of Wt (exact zeros add nothing and round nothing)"""
    K = x.shape[1]
    if K % 32:
        x = torch.cat([x, torch.zeros(x.shape[0], 32 - K % 32, device=x.device)], 1)
        Wt = torch.cat([Wt, torch.zeros(32 - K % 32, Wt.shape[1], device=Wt.device)], 0)
    return dcl.ops.linear_dma(x, dcl.ops.pad_linear_weight(Wt), bias, relu)


# ------------------------------------------------------------------------------------------- a. sparse rows
@pytest.mark.parametrize("shape", SC.SPARSE_SHAPES)
@pytest.mark.parametrize("with_bias,relu", [(False, False), (True, True)])
def test_sparse_rows_every_piece_product_is_there(dcl, shape, with_bias, relu):
    """Rows with s = 1, 2, 3 non-zeros (values and weights randn * 2^randint(-20, 20): all three pieces non-zero), a non-zero at
    every k of every 16-chunk, in every wave, 32-row block, 32-column block, a second and a ragged column tile.  Per output
    |err| <= (6 s + 1 + [bias]) 2^-24 (sum |x||w| + |bias|):
      * a zero of x is three zero pieces: its products are exact zeros and an accumulator that adds zero does not round;
      * each of the s non-zero products enters as six piece products, each exact (8 x 8 bits), each added into the fp32
        accumulator with ONE rounding of a partial sum whose magnitude is at most sum |x||w|: 6 s units;
      * the three products left out: |m| <= 2^-8 |v| and |l| <= 2^-17 |v| (l is the rounding error of an 8-bit m), so
        |xm wl + xl wm + xl wl| <= (2^-25 + 2^-25 + 2^-34) |x w|: half a unit in the typical case, one in the worst: 1 unit;
      * the bias add rounds once: 1 unit of sum |x||w| + |bias|.
    The fp32 core (one FMA per non-zero, zeros exact) must hold s + 1 + [bias].  A kernel without one of the six products is off
    by >= 97 units on the one-hot rows (tests/test_split_model.py)."""
    x, Wt, bias, s = SC.sparse_case(*shape)
    bias = bias if with_bias else None
    xd, wd, bd = x.cuda(), Wt.cuda(), None if bias is None else bias.cuda()
    got = dcl.ops.linear_split(xd, dcl.ops.SplitWeight(wd), bd, relu).cpu()
    ref = fp32_linear(dcl, xd, wd, bd, relu).cpu()
    um, um32 = SC.unit_map(got, x, Wt, bias, relu), SC.unit_map(ref, x, Wt, bias, relu)
    for k in (1, 2, 3):
        report("sparse M=%d K=%d N=%d bias=%d s=%d" % (shape + (with_bias, k)), split=float(um[s == k].max()),
               fp32=float(um32[s == k].max()), allowed_split=SC.sparse_bound_split(k, with_bias), allowed_fp32=SC.sparse_bound_fp32(k, with_bias))
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(ref).all())
    worst = um / SC.sparse_bound_split(s, with_bias).double().view(-1, 1)
    assert float(worst.max()) <= 1.0, "split kernel: row %d, column %d at %.2f of its bound" % (
        int(worst.max(1).values.argmax()), int(worst.max(0).values.argmax()), float(worst.max()))
    worst32 = um32 / SC.sparse_bound_fp32(s, with_bias).double().view(-1, 1)
    assert float(worst32.max()) <= 1.0, "fp32 core at %.2f of its bound" % float(worst32.max())


# ------------------------------------------------------------------------------------------- b. dense adversarial rows
@pytest.mark.parametrize("K,N", SC.DENSE_KN)
@pytest.mark.parametrize("name", SC.DENSE_SETS)
def test_dense_rows_against_the_fp32_chain(dcl, name, K, N):
    """units(split kernel) <= 1.5 units(CPU fp32 FMA chain) and units(fp32 core) <= 1.05 units(chain), units = max over outputs
    of |err| / (2^-24 sum |x||w|) against float64: Gaussian rows, elements spread over 2^+-30 inside a row, rows that cancel to
    2^-12 of their magnitude, and all-positive operands whose second and third pieces all have the same sign (a lost small term
    then adds up instead of averaging out).  M = 517: two whole row tiles and a ragged one."""
    x, Wt, _ = SC.dense_case(name, K, N)
    xd, wd = x.cuda(), Wt.cuda()
    chain = SC.chain_units(name, K, N)
    split = SC.units(dcl.ops.linear_split(xd, dcl.ops.SplitWeight(wd)).cpu(), x, Wt)
    fp32 = SC.units(fp32_linear(dcl, xd, wd).cpu(), x, Wt)
    report("dense %s K=%d N=%d" % (name, K, N), split=split, fp32=fp32, chain=chain, split_over_chain=split / chain, fp32_over_chain=fp32 / chain)
    assert split <= SC.SPLIT_OVER_CHAIN * chain, (name, K, N, split, chain)
    assert fp32 <= SC.FP32_OVER_CHAIN * chain, (name, K, N, fp32, chain)


# ------------------------------------------------------------------------------------------- c. range and non-finite operands
@pytest.mark.parametrize("name", SC.RANGE_SETS)
def test_operands_at_the_ends_of_the_exponent_range(dcl, name):
    """'huge': |x| up to 2^127 with weights near 2^-98, products finite -- the bounds of (b).  'tiny': |x| < 2^-110, where the
    third piece is a bf16 subnormal and h + m + l may fall short of x by a bf16 subnormal step -- the bound of (b) plus
    sum_k 2^-126 |w_k|, one fp32 minimum normal per term, which covers a piece that is flushed as well as one that is inexact.
    The test prints which of the two the hardware does: the worst error in units of the (b) bound alone.  Measured on an MI355X
    (profiles/split_arithmetic.txt): 33.437 units, the digits of the CPU model that keeps bf16-subnormal pieces (flushed: 3842) --
    the conversion and the matrix pipe keep them."""
    x, Wt = SC.range_case(name)
    M, K, N = SC.RANGE_SHAPE
    xd, wd = x.cuda(), Wt.cuda()
    chain = SC.chain_units(name, K, N)
    mag, want = SC.magnitude(x, Wt), SC.reference(x, Wt)
    extra = SC.tiny_allowance(Wt) if name == "tiny" else 0.0
    got = dcl.ops.linear_split(xd, dcl.ops.SplitWeight(wd)).cpu()
    ref = fp32_linear(dcl, xd, wd).cpu()
    e, e32 = (got.double() - want).abs(), (ref.double() - want).abs()
    report("range %s" % name, split=float((e / (SC.U * mag)).max()), fp32=float((e32 / (SC.U * mag)).max()), chain=chain,
           split_in_allowance=float((e / (SC.SPLIT_OVER_CHAIN * chain * SC.U * mag + extra)).max()))
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(ref).all())
    assert bool((e <= SC.SPLIT_OVER_CHAIN * chain * SC.U * mag + extra).all())
    assert bool((e32 <= SC.FP32_OVER_CHAIN * chain * SC.U * mag + extra).all())


def test_an_operand_whose_first_piece_overflows_gives_nan_for_its_row_only(dcl):
    """|v| >= 3.3962e38 (bits 0x7F7F8000) is finite in fp32 but rounds to inf in bf16: h = inf, m = -inf, l = NaN, so every
    output of that row is NaN on the split core (the fp32 core still computes it) -- unsupported range, pinned here.  The value
    just below is fine, and every other row has the bits of the same launch with the overflowing rows zeroed."""
    x, Wt = SC.range_case("huge")
    M, K, N = SC.RANGE_SHAPE
    edge = torch.tensor([SC.H_OVERFLOWS, SC.H_OVERFLOWS - 1, 0x7F7FFFFF], dtype=torch.int32).view(torch.float32)
    x = x.clone()
    x[10, 3], x[75, 20], x[299, 63] = edge[0], -edge[1], -edge[2]
    zeroed = x.clone()
    zeroed[[10, 299]] = 0.0
    wd = Wt.cuda()
    sw = dcl.ops.SplitWeight(wd)
    got, clean = dcl.ops.linear_split(x.cuda(), sw).cpu(), dcl.ops.linear_split(zeroed.cuda(), sw).cpu()
    ref = fp32_linear(dcl, x.cuda(), wd).cpu()
    assert bool(torch.isnan(got[[10, 299]]).all())
    assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(got[75]).all())
    others = [i for i in range(M) if i not in (10, 299)]
    assert torch.equal(got[others], clean[others])
    assert SC.units(got[75:76], x[75:76], Wt) <= SC.SPLIT_OVER_CHAIN * SC.chain_units("huge", K, N)


@pytest.mark.parametrize("poison", [math.inf, -math.inf, math.nan])
def test_a_non_finite_row_or_weight_column_stays_alone(dcl, poison):
    """A row of x holding +inf, -inf or NaN: every output of that row is NaN on the split core (h = +-inf, v - h = NaN; the
    fp32 core gives +-inf by the sign of the weight for an inf) -- and EVERY OTHER ROW of the launch has, bit for bit, the values
    of the same launch with that row zeroed, although rows share LDS tiles and MFMA operands: poisoned rows at the first, a middle
    and the last row of a 64-row wave block and in the ragged last row tile (whose last row also stands in for the rows past M).
    Likewise a non-finite weight: its column is NaN in every row, the other columns keep their bits.  Behind the ReLU epilogue a
    poisoned row is 0 in every column: the epilogue is fmaxf(v, 0), and fmaxf returns its other operand for a NaN."""
    K, N = 256, 260
    x, Wt, bias = SC.dense_case("gaussian", K, N)
    M = x.shape[0]
    rows, cols = list(SC.POISON_ROWS), list(SC.POISON_COLS)
    assert rows[-1] == M - 1 and cols[-1] == N - 1
    xp, xz = x.clone(), x.clone()
    for r in rows:
        xp[r, (7 * r) % K] = poison
    xz[rows] = 0.0
    wd = Wt.cuda()
    sw = dcl.ops.SplitWeight(wd)
    keep = [i for i in range(M) if i not in rows]
    got, clean = dcl.ops.linear_split(xp.cuda(), sw, bias.cuda()).cpu(), dcl.ops.linear_split(xz.cuda(), sw, bias.cuda()).cpu()
    assert bool(torch.isnan(got[rows]).all()), "a poisoned row must be NaN in every column"
    assert torch.equal(got[keep], clean[keep]), "rows beside a poisoned row changed"
    relu_out = dcl.ops.linear_split(xp.cuda(), sw, bias.cuda(), True).cpu()
    report("nonfinite %s relu" % poison, nan=int(torch.isnan(relu_out[rows]).sum()), zero=int((relu_out[rows] == 0).sum()))
    assert bool((relu_out[rows] == 0).all()), "a poisoned row behind the ReLU epilogue must be 0 in every column"
    assert torch.equal(relu_out[keep], torch.relu(clean[keep]))
    ref, ref_clean = fp32_linear(dcl, xp.cuda(), wd, bias.cuda()).cpu(), fp32_linear(dcl, xz.cuda(), wd, bias.cuda()).cpu()
    assert torch.equal(ref[keep], ref_clean[keep])
    if math.isnan(poison):
        assert bool(torch.isnan(ref[rows]).all())
    else:                                                   # the documented difference: inf, not NaN, signed like poison * weight
        wk = torch.stack([Wt[(7 * r) % K] for r in rows])
        assert torch.equal(ref[rows], torch.sign(wk) * poison)
    # a non-finite weight
    wp, wz = Wt.clone(), Wt.clone()
    for c in cols:
        wp[(11 * c) % K, c] = poison
    wz[:, cols] = 0.0
    keepc = [c for c in range(N) if c not in cols]
    xd = x.cuda()
    got, clean = dcl.ops.linear_split(xd, dcl.ops.SplitWeight(wp.cuda())).cpu(), dcl.ops.linear_split(xd, dcl.ops.SplitWeight(wz.cuda())).cpu()
    assert bool(torch.isnan(got[:, cols]).all()), "a poisoned column must be NaN in every row"
    assert torch.equal(got[:, keepc], clean[:, keepc]), "columns beside a poisoned column changed"


# ------------------------------------------------------------------------------------------- d. the epilogues
@pytest.mark.parametrize("M,K,N,rpc", SC.POOL_CASES)
def test_pooling_epilogue_of_the_split_core(dcl, M, K, N, rpc):
    """dcl_linear_split_pool_fwd (EPI 1) called directly: part[t] = sum over the rows j of 128-row tile t of w_j relu(x_j Wt +
    bias), against float64 and beside the fp32 core's linear_pool.  M = 1000 is ragged (rows past M weigh nothing, the last
    workgroup tile has one pooling tile only), N = 200 is one whole and one ragged column tile; 3 crops x 384 rows with the
    weights at a stride of 500: 384 is a whole number of pooling tiles but not of 256-row workgroup tiles, so one workgroup tile
    holds rows of two crops.  Zero and negative weights.  `part` is a column block of a NaN-filled buffer: every entry is
    written, no neighbour is.  Two launches give the same bits.
    Bound, per entry, in units of 2^-24 sum_j |w_j| (sum_k |x||w| + |bias|): every activation is off by at most the GEMM's bound
    of (b), 1.5 x the fp32 chain's units on these operands (ReLU does not widen an error); the weighted sum is 64 FMAs in a lane,
    an add across the lane halves and an add across the two waves, each rounding a partial sum of at most that magnitude: 66."""
    x, Wt, bias, roww = SC.pool_case(M, K, N, rpc)
    w = SC.pool_row_weights(roww, M, rpc)
    want, mag = SC.pool_reference(x, Wt, bias, w)
    tiles = want.shape[0]
    xd, wd, bd, rd = x.cuda(), Wt.cuda(), bias.cuda(), roww.cuda()
    sw = dcl.ops.SplitWeight(wd)
    kw = {} if rpc is None else dict(rows_per_crop=rpc, w_stride=SC.POOL_W_STRIDE)
    wide = torch.full((tiles, N + 24), float("nan"), device="cuda")
    dcl.ops.linear_split_pool(xd, sw, bd, rd, True, part=wide[:, 8:8 + N], **kw)
    got = wide[:, 8:8 + N].clone()
    assert bool(torch.isnan(wide[:, :8]).all()) and bool(torch.isnan(wide[:, 8 + N:]).all()) and not bool(torch.isnan(got).any())
    assert torch.equal(got, dcl.ops.linear_split_pool(xd, sw, bd, rd, True, **kw))
    ref = dcl.ops.linear_pool(xd, wd, bd, rd, True, **kw)                               # Wt was never prepared: the fp32 core
    chain = SC.pool_chain_units(M, K, N, rpc)
    e, e32 = (got.cpu().double() - want).abs() / (SC.U * mag), (ref.cpu().double() - want).abs() / (SC.U * mag)
    allowed = SC.epilogue_bound(SC.SPLIT_OVER_CHAIN * chain, SC.POOL_FMAS)
    report("pool M=%d K=%d N=%d crops=%s" % (M, K, N, rpc), split=float(e.max()), fp32=float(e32.max()), chain=chain, allowed=allowed)
    assert float(e.max()) <= allowed and float(e32.max()) <= allowed


@pytest.mark.parametrize("M,N", SC.ROWDOT_CASES)
def test_row_dot_epilogue_of_the_split_core(dcl, M, N):
    """dcl_linear_split_rowdot_fwd (EPI 2) called directly: out[m] = w3 . relu(x[m] Wt + bias) + b3 against float64 and beside
    the fp32 core's linear_rowdot; w3 a column of a padded buffer (stride 4); N = 96: the 32 columns past N contribute EXACTLY
    nothing -- the bits equal those of the same layer padded to 128 columns with zeros; M = 1000, 37, 1 and 0 rows.
    Bound in units of 2^-24 (sum_c |w3_c| (sum_k |x||w| + |bias_c|) + |b3|): the GEMM's bound of (b) per hidden activation, plus
    4 FMAs in a lane, 5 butterfly adds and the add of b3: 10."""
    x, Wt, bias, w3, b3 = SC.rowdot_case(M, N)
    want, mag = SC.rowdot_reference(x, Wt, bias, w3, b3)
    xd, wd, bd, b3d = x.cuda(), Wt.cuda(), bias.cuda(), b3.cuda()
    w3d = dcl.ops.pad_linear_weight(w3.cuda())
    assert w3d.stride(0) == 4
    sw = dcl.ops.SplitWeight(wd)
    got = dcl.ops.linear_split_rowdot(xd, sw, bd, w3d, b3d)
    assert got.shape == (M, 1) and torch.equal(got, dcl.ops.linear_split_rowdot(xd, sw, bd, w3d, b3d))
    ref = dcl.ops.linear_rowdot(xd, wd, bd, w3d, b3d)
    assert ref.shape == (M, 1)
    if M == 0:
        return
    if N < 128:
        z = 128 - N                                         # the same layer with z zero columns, zero biases and zero w3 rows
        wfull = torch.cat([wd, torch.zeros(SC.ROWDOT_K, z, device="cuda")], 1)
        w3full = dcl.ops.pad_linear_weight(torch.cat([w3.cuda(), torch.zeros(z, 1, device="cuda")], 0))
        full = dcl.ops.linear_split_rowdot(xd, dcl.ops.SplitWeight(wfull), torch.cat([bd, torch.zeros(z, device="cuda")]), w3full, b3d)
        assert torch.equal(got, full)
    chain = SC.rowdot_chain_units(M, N)
    e, e32 = (got.cpu().double() - want).abs() / (SC.U * mag), (ref.cpu().double() - want).abs() / (SC.U * mag)
    allowed = SC.epilogue_bound(SC.SPLIT_OVER_CHAIN * chain, SC.ROWDOT_FMAS)
    report("rowdot M=%d N=%d" % (M, N), split=float(e.max()), fp32=float(e32.max()), chain=chain, allowed=allowed)
    assert float(e.max()) <= allowed and float(e32.max()) <= allowed


def test_v_pieces_epilogue_without_relu_keeps_both_signs(request, dcl):
    """dcl_linear_split_vpieces_fwd (EPI 3) with relu = False and pre-activations of both signs: the pieces it writes are, bit
    for bit, those the attention's piece pass makes from the fp32 output of the same GEMM, and h + m + l read back from the
    scratch is that fp32 output exactly, which holds the bound of (b) against float64"""
    lib = enter_diag(dcl, request)
    lib.dcl_debug_attention_variant(3)
    try:
        g = torch.Generator().manual_seed(78)
        b, nq, nk, Kd = 2, 200, 512, 64
        H, Wt, bias = torch.randn(b * nk, Kd, generator=g), torch.randn(Kd, 256, generator=g) * 0.1, torch.randn(256, generator=g) * 0.1
        sw = dcl.ops.SplitWeight(Wt.cuda())
        V1 = dcl.ops.linear_split(H.cuda(), sw, bias.cuda(), False)
        assert float(V1.min()) < -0.1 and float(V1.max()) > 0.1
        Q, Km = torch.randn(b * nq, 64, generator=g).cuda(), torch.randn(b * nk, 64, generator=g).cuda()
        planes_a, whole = dcl.ops.attention_planes(b, nq, nk, 1)
        assert planes_a is not None and whole
        planes_b = torch.zeros_like(planes_a)
        O1, O2 = torch.empty(b * nq, 256, device="cuda"), torch.empty(b * nq, 64, device="cuda")
        dcl.ops.cross_attention(b, Q, Km, V1, O1, Km, O2, planes=planes_a)                 # the piece pass over all 320 channels
        dcl.ops.linear_split_vpieces(H.cuda(), sw, bias.cuda(), planes_b, nk, relu=False)
        nht = nk // 16
        va = planes_a[:b * nht * 30720].view(b * nht, 3, 320, 32)[:, :, :256]
        vb = planes_b[:b * nht * 30720].view(b * nht, 3, 320, 32)[:, :, :256]
        assert torch.equal(va, vb)
        pieces = vb.cpu().contiguous().view(torch.bfloat16).view(b, nht, 3, 256, 2, 8).double().sum(2)       # h + m + l
        c, hs, e = torch.arange(256).view(-1, 1, 1), torch.arange(2).view(1, -1, 1), torch.arange(8).view(1, 1, -1)
        key = (e & 3) + 8 * (e >> 2) + 4 * (hs ^ ((c >> 3) & 1))                                             # (256, 2, 8)
        back = torch.zeros(b, nht, 16, 256, dtype=torch.float64)
        back[:, :, key, c.expand(256, 2, 8)] = pieces
        assert torch.equal(back.view(b * nk, 256), V1.cpu().double())
        chain = SC.units(SC.model_fma_chain(H, Wt, bias), H, Wt, bias)
        split = SC.units(V1.cpu(), H, Wt, bias)
        report("vpieces K=%d" % Kd, split=split, chain=chain)
        assert split <= SC.SPLIT_OVER_CHAIN * chain
    finally:
        lib.dcl_debug_attention_variant(0)


# ------------------------------------------------------------------------------------------- e. dispatch
def _split_launches(lib):
    import test_kernel_census as TC
    return sum(v for k, v in TC.census(lib).items() if k.startswith("k_linear_split"))


@pytest.mark.parametrize("K", [16, 32])
def test_prepared_layers_switch_cores_at_192_tiles(request, dcl, K):
    """A prepared (K, 128) weight: at M = 48896 (191 tiles of 256 x 128) linear, linear_pool and linear_rowdot launch no
    k_linear_split kernel, at M = 48897 (192 tiles) each launches one; with GEMM_SPLIT off neither size does.  K = 16 is the
    smallest layer the split core takes, and one the fp32 core does not (K in whole 32-chunks): below the threshold linear runs
    on the vendor library and linear_pool / linear_rowdot, which have no other kernel, fail loudly -- pinned; K = 32 compares the
    values across the switch for all three.  The first 48896 rows (382 pooling tiles) agree across the switch within the sum of
    the two cores' bounds of (b) / (d); the vendor library is allowed the a-priori K + 2 units of any fp32 summation order."""
    lib = enter_diag(dcl, request)
    M0, M1, n = SC.DISPATCH_BELOW, SC.DISPATCH_FROM, SC.DISPATCH_N
    assert (M0 + 255) // 256 == dcl.ops.SPLIT_MIN_TILES - 1 and (M1 + 255) // 256 == dcl.ops.SPLIT_MIN_TILES
    g = torch.Generator().manual_seed(160 + K)
    x, Wt, bias = torch.randn(M1, K, generator=g), torch.randn(K, n, generator=g) * 0.2, torch.randn(n, generator=g) * 0.2
    roww, w3, b3 = torch.randn(M1, generator=g), torch.randn(n, 1, generator=g), torch.randn(1, generator=g)
    xd, wd, bd, rd, w3d, b3d = x.cuda(), Wt.cuda(), bias.cuda(), roww.cuda(), w3.cuda(), b3.cuda()
    assert dcl.ops.prepare_linear(wd) is not None
    calls = {"linear": lambda M: dcl.ops.linear(xd[:M], wd, bd, True),
             "linear_pool": lambda M: dcl.ops.linear_pool(xd[:M], wd, bd, rd[:M].contiguous(), True),
             "linear_rowdot": lambda M: dcl.ops.linear_rowdot(xd[:M], wd, bd, w3d, b3d)}
    own_fp32 = K % 32 == 0
    out = {}
    try:
        for split_on in (True, False):
            dcl.ops.GEMM_SPLIT = split_on
            for M in (M0, M1):
                for name, call in calls.items():
                    lib.dcl_debug_launch_census_reset()
                    expect_split = split_on and M == M1
                    if not expect_split and not own_fp32 and name != "linear":
                        with pytest.raises(RuntimeError):
                            call(M)
                    else:
                        got = call(M)
                        if split_on:
                            out[name, M] = got.cpu()
                    assert _split_launches(lib) == (1 if expect_split else 0), (name, M, split_on)
    finally:
        dcl.ops.GEMM_SPLIT = True
    x0, r0 = x[:M0], roww[:M0]
    chain = SC.units(SC.model_fma_chain(x0, Wt, bias), x0, Wt, bias)
    other = SC.FP32_OVER_CHAIN * chain if own_fp32 else K + 2
    mag = SC.magnitude(x0, Wt, bias)
    d = (out["linear", M1][:M0].double() - out["linear", M0].double()).abs() / (SC.U * mag)
    report("dispatch linear K=%d" % K, across=float(d.max()), chain=chain, allowed=SC.SPLIT_OVER_CHAIN * chain + other)
    assert float(d.max()) <= SC.SPLIT_OVER_CHAIN * chain + other
    assert SC.units(out["linear", M1][:M0], x0, Wt, bias, True) <= SC.SPLIT_OVER_CHAIN * chain
    if own_fp32:
        _, pmag = SC.pool_reference(x0, Wt, bias, r0)
        d = (out["linear_pool", M1][:M0 // 128].double() - out["linear_pool", M0].double()).abs() / (SC.U * pmag)
        allowed = SC.epilogue_bound(SC.SPLIT_OVER_CHAIN * chain, SC.POOL_FMAS) + SC.epilogue_bound(other, SC.POOL_FMAS)
        report("dispatch linear_pool K=%d" % K, across=float(d.max()), allowed=allowed)
        assert float(d.max()) <= allowed
        _, rmag = SC.rowdot_reference(x0, Wt, bias, w3, b3)
        d = (out["linear_rowdot", M1][:M0].double() - out["linear_rowdot", M0].double()).abs() / (SC.U * rmag)
        allowed = SC.epilogue_bound(SC.SPLIT_OVER_CHAIN * chain, SC.ROWDOT_FMAS) + SC.epilogue_bound(other, SC.ROWDOT_FMAS)
        report("dispatch linear_rowdot K=%d" % K, across=float(d.max()), allowed=allowed)
        assert float(d.max()) <= allowed


# ------------------------------------------------------------------------------------------- f. attention
ATTN_KERNELS = {(3, 1): "k_cross_attn_split", (3, 0): "k_cross_attn_dma<8>", (1, 0): "k_cross_attn_shared<8", (2, 0): "k_cross_attn<"}


@pytest.fixture
def attn(request, dcl):
    """run(Q, K, V, bf16, split, variant=3) -> O (b, nq, 320) on the CPU.  Variant 3 is the 8-wave attention whatever the size, as
    the split-bf16 form (bf16 = 1: k_cross_attn_split) or the fp32 form (bf16 = 0: k_cross_attn_dma<8>), with the key split the
    launch plan picks on its own (split = 0), none (1) or a forced one; variants 1 and 2 are the general-shape fp32 kernels of the
    diagnostic library (k_cross_attn_shared<8>, k_cross_attn), which never split.  The launch census shows that the kernel meant
    ran, once, and no other attention kernel; and the combine pass exactly when the keys were split."""
    import test_kernel_census as TC
    lib = enter_diag(dcl, request)

    def reset():
        lib.dcl_debug_attention_variant(0)
        lib.dcl_debug_attention_bf16(1)
        lib.dcl_debug_attention_split(0)
    request.addfinalizer(reset)

    def run(Q, K, V, bf16, split, variant=3):
        b, nq, nk = Q.shape[0], Q.shape[1], K.shape[1]
        lib.dcl_debug_attention_variant(variant)
        lib.dcl_debug_attention_bf16(bf16)
        lib.dcl_debug_attention_split(split)
        O1, O2 = torch.empty(b * nq, 256, device="cuda"), torch.empty(b * nq, 64, device="cuda")
        Qd, Kd, Vd = Q.cuda().reshape(-1, 64), K.cuda().reshape(-1, 64), V.cuda()
        V1, V2 = Vd[..., :256].reshape(-1, 256), Vd[..., 256:].reshape(-1, 64).contiguous()
        lib.dcl_debug_launch_census_reset()
        dcl.ops.cross_attention(b, Qd, Kd, V1, O1, V2, O2)
        seen = {k: v for k, v in TC.census(lib).items() if k.startswith("k_cross_attn")}
        nsplit = SC.effective_split(nk, split, b, nq) if variant == 3 else 1
        main = [k for k in seen if k.startswith(ATTN_KERNELS[variant, bf16])]
        assert len(main) == 1 and seen[main[0]] == 1, (variant, bf16, split, seen)
        assert seen.get("k_cross_attn_combine", 0) == (1 if nsplit > 1 else 0), (variant, bf16, split, seen)
        assert len(seen) == (2 if nsplit > 1 else 1), (variant, bf16, split, seen)
        return torch.cat([O1.view(b, nq, 256), O2.view(b, nq, 64)], 2).cpu()
    return run


ATTN_GRID = [(nk, split) for nk in SC.ATTN_NKS for split in SC.ATTN_SPLITS]


@pytest.mark.parametrize("nk,split", ATTN_GRID)
def test_attention_one_hot_softmax_returns_the_selected_row(attn, nk, split):
    """Query i's logit for key j*(i) leads every other by >= 47 (all others together weigh < e^-40); the j* cover every slot of
    two 32-key tiles, both half tiles, the ragged last tile and both sides of every key-split boundary; V is randn *
    2^randint(-20, 20) per element.  |O_i - V[j*]| <= c 2^-24 |V[j*]| + e^-40 max |V| per channel, c by counting roundings:
    the weight of j* is exp(0) = 1 whatever the lazy maximum did before (a lead of 47 > the rescale threshold of 20 forces the
    rescale to j*'s logit), so it and the sum of the weights carry the same value; the six piece products enter the accumulator
    with one rounding each (6), the three left out are at most one unit (1), a later rescale multiplies once (1), the sum of the
    weights rounds at most once where the others are below half a step of 1 (1), the division (1): c = 10.  With a key split
    the partial is not divided; the combine multiplies numerator and denominator by a factor each and divides (3 for 1): c = 12.
    A kernel without one of the three products of P's first piece is off by >= 2^-17 |V| = 128 units (tests/test_split_model.py);
    the fp32 form holds the same bound."""
    Q, K, V = SC.attn_case("onehot", nk)
    jstar = SC.onehot_keys(nk)
    vs = torch.stack([V[i, jstar] for i in range(V.shape[0])]).double()
    bound = SC.onehot_bound(V, jstar, SC.effective_split(nk, split))
    worst = {}
    for bf16 in (1, 0):
        O = attn(Q, K, V, bf16, split)
        assert bool(torch.isfinite(O).all())
        worst[bf16] = float(((O.double() - vs).abs() / bound).max())
    report("attention onehot nk=%d split=%d" % (nk, split), split_of_bound=worst[1], fp32_of_bound=worst[0], c=SC.onehot_c(SC.effective_split(nk, split)))
    assert worst[1] <= 1.0 and worst[0] <= 1.0, worst


@pytest.mark.parametrize("name", ["cancel_v", "v_spread"])
@pytest.mark.parametrize("nk,split", ATTN_GRID)
def test_attention_adversarial_v_beside_the_fp32_form(attn, name, nk, split):
    """cancel_v: near-uniform weights over key pairs (v, -v (1 + 2^-12)), outputs 2^-12 of their magnitude.  v_spread: V rows
    scaled by 2^e_j, e_j in [-30, 30], the large weights on the small rows.  In units of 2^-24 sum_j p_j |v_j| (p from the
    float64 softmax): split form <= 1.5 x the fp32 form measured on the same operands, both <= the a-priori nk + 64 of an fp32
    form (one rounding per key in the P.V chain; 64 for exp, the sum of the weights, the division and the rescales)."""
    Q, K, V = SC.attn_case(name, nk)
    u = {bf16: SC.units_attn(attn(Q, K, V, bf16, split), name, nk) for bf16 in (1, 0)}
    report("attention %s nk=%d split=%d" % (name, nk, split), split=u[1], fp32=u[0], split_over_fp32=u[1] / u[0], apriori=SC.attn_apriori_units(nk))
    assert u[1] <= SC.ATTN_SPLIT_OVER_FP32 * u[0], u
    assert u[1] <= SC.attn_apriori_units(nk) and u[0] <= SC.attn_apriori_units(nk), u


@pytest.mark.parametrize("nk,split", ATTN_GRID)
def test_attention_logits_that_cancel(attn, nk, split):
    """|q_c k_c| ~ 2^6 per channel, channel pairs of opposite sign, the logit of order one: a logit is off by at most dS = 25 2^-24
    max sum |q||k| (4 k steps x 6 products + 1 roundings of a partial sum of at most sum |q||k|), a weight by a factor e^+-dS and,
    normalised, by at most 2 dS; so |dO| <= (2 dS + (nk + 64) 2^-24) sum_j p_j |v_j|.  Split form <= 1.5 x the fp32 form."""
    Q, K, V = SC.attn_case("cancel_s", nk)
    O, D, _, qk = SC.attn_reference("cancel_s", nk)
    allowed = (2 * SC.cancel_s_delta(qk) + SC.attn_apriori_units(nk) * SC.U) * D
    got = {bf16: attn(Q, K, V, bf16, split) for bf16 in (1, 0)}
    u = {bf16: SC.units_attn(got[bf16], "cancel_s", nk) for bf16 in (1, 0)}
    report("attention cancel_s nk=%d split=%d" % (nk, split), split=u[1], fp32=u[0], split_over_fp32=u[1] / u[0],
           allowed=float((allowed / (SC.U * D)).min()))
    for bf16 in (1, 0):
        assert bool(((got[bf16].double() - O).abs() <= allowed).all()), bf16
    assert u[1] <= SC.ATTN_SPLIT_OVER_FP32 * u[0], u


@pytest.mark.parametrize("nk,split", ATTN_GRID)
def test_attention_non_finite_operands_stay_alone(attn, nk, split):
    """NaN in one Q row: that query's outputs are NaN and every other query -- its wave mates included -- keeps the bits of the
    clean launch (in all four attention kernels: the lazy rescale of the reference maximum is applied per query).  NaN in a K row or inf in a V1 entry of crop 0: crop 1 keeps its bits (and an inf in V1 only touches its own
    channel of crop 0).  Split form and fp32 form."""
    Q, K, V = SC.attn_case("gaussian", nk)
    b, nq = Q.shape[0], Q.shape[1]
    for bf16 in (1, 0):
        clean = attn(Q, K, V, bf16, split)
        assert bool(torch.isfinite(clean).all())
        Qp = Q.clone()
        Qp[0, 37, 5], Qp[1, nq - 1, 63] = math.nan, math.nan
        got = attn(Qp, K, V, bf16, split)
        assert bool(torch.isnan(got[0, 37]).all()) and bool(torch.isnan(got[1, nq - 1]).all())
        keep0, keep1 = [i for i in range(nq) if i != 37], list(range(nq - 1))
        assert torch.equal(got[0, keep0], clean[0, keep0]) and torch.equal(got[1, keep1], clean[1, keep1]), \
            "bf16=%d: queries beside a NaN query changed" % bf16
        if bf16 == 0 and split == 0:                        # the other two fp32 kernels rescale per query too
            for variant in (1, 2):
                c, g = attn(Q, K, V, 0, 0, variant), attn(Qp, K, V, 0, 0, variant)
                assert bool(torch.isfinite(c).all()) and bool(torch.isnan(g[0, 37]).all()) and bool(torch.isnan(g[1, nq - 1]).all())
                assert torch.equal(g[0, keep0], c[0, keep0]) and torch.equal(g[1, keep1], c[1, keep1]), \
                    "variant %d: queries beside a NaN query changed" % variant
        Kp = K.clone()
        Kp[0, 5, 9] = math.nan
        got = attn(Q, Kp, V, bf16, split)
        assert bool(torch.isnan(got[0]).all()) and torch.equal(got[1], clean[1]), bf16
        Vp = V.clone()
        Vp[0, 40, 7] = math.inf
        got = attn(Q, K, Vp, bf16, split)
        others = [c for c in range(320) if c != 7]
        assert not bool(torch.isfinite(got[0, :, 7]).any()) and torch.equal(got[1], clean[1]), bf16
        assert torch.equal(got[0][:, others], clean[0][:, others]), bf16
        if bf16:
            assert bool(torch.isnan(got[0, :, 7]).all())
