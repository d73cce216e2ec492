"""The dense tail of the eval forward (Network._dense_tail: correspondence attention, confidence softmax, confidence-weighted
pooling, trailing BatchNorm finish, pose heads) op by op against float64, at the shapes on either side of every switch of
csrc/dense.hip's launchers and of the route choice in models/DCL_Net.py.  Cases, references and bounds: tests/tail_cases.py
(checked on the CPU by tests/test_tail_cases.py).  Which kernel ran is read from the diagnostic library's launch census.

Bounds: softmax / pooling / finish err <= max(2 err_module, 1e-6 max|ref64|) (conf_pool_cases.compare), err_module = the fp32
torch composition of the module's lines on the same operands against the same float64 reference; attention 2e-5 max(1, max|want|)
(test_cross_attention_matches_fp64); exact operand sets bit for bit.  Every comparison prints one `tail` line."""
import re

import pytest
import torch

import tail_cases as TC
import test_gpu_ops as TO
import test_kernel_census as CENSUS

pytestmark = pytest.mark.gpu

R_TOL, T_TOL, CONF_TOL = 1e-4, 1e-5, 1e-4         # the parity bounds of tests/test_gpu_network.py


def _census(lib, fn):
    """fn() and the set of kernels it launched"""
    lib.dcl_debug_launch_census_reset()
    out = fn()
    torch.cuda.synchronize()
    return out, {k for k, n in CENSUS.census(lib).items() if n > 0}


def _starts(ran, prefix):
    return sorted(k for k in ran if k.startswith(prefix))


def _pool_gemms(ran):
    """the GEMM cores' instances with the pooling epilogue (EPI = 1: k_linear_dma<BM, BN, WGR, EPI, KS>, k_linear_split<EPI>)"""
    out = []
    for k in ran:
        m = re.match(r"k_linear_(dma|split)<(.*)>$", k)
        if m:
            args = [a.strip() for a in m.group(2).split(",")]
            if (args[3] if m.group(1) == "dma" else args[0]) == "1":
                out.append(k)
    return sorted(out)


def _flat(t):
    return t.cuda().reshape(-1)


# ================================================================================================ 1. conf_softmax
@pytest.mark.parametrize("kind", TC.LOGIT_SETS)
@pytest.mark.parametrize("i", range(len(TC.SOFTMAX_SHAPES)), ids=TC.SOFTMAX_IDS)
def test_conf_softmax_matches_float64(request, dcl, i, kind):
    """dcl_conf_softmax alone against the float64 sigmoid, softmax and direction sums, in the 256-thread form up to 4096 logits
    per crop and the 1024-thread form beyond.  Fails if: the 1024-thread kernel combines its wave sums with the 256-thread tree
    (4 of 16 waves: the weights sum to ~4), a strided pass skips the ragged tail of L, n1 is rounded to a wave when the
    direction sums are split, or expf(-x) = inf for x = -100 poisons the row."""
    lib = TO.enter_diag(dcl, request)
    b, n1, n2 = TC.SOFTMAX_SHAPES[i]
    L = n1 + n2
    l1, l2, ref, module = TC.softmax_case(i, kind)
    a1, a2 = _flat(l1), _flat(l2)
    (conf, w, ws), ran = _census(lib, lambda: dcl.ops.conf_softmax(b, a1, a2))
    assert _starts(ran, "k_conf_") == ["k_conf_softmax<1024>" if L > TC.SOFTMAX_WIDE_ABOVE else "k_conf_softmax<256>"], sorted(ran)
    tag = "softmax %s %s" % (TC.SOFTMAX_IDS[i], kind)
    for name, got in (("conf", conf), ("w", w), ("wsum", ws)):
        TC.check(tag, name, got, ref[name], module[name])
    assert bool(torch.isfinite(w).all()) and bool((w > 0).all())
    assert float((w.double().sum(1) - 1).abs().max()) <= 1e-6
    assert float((ws.double().sum(1) - 1).abs().max()) <= 1e-6
    again = dcl.ops.conf_softmax(b, a1, a2)
    assert all(TC.same_bits(x, y) for x, y in zip((conf, w, ws), again))
    if L > TC.SOFTMAX_WIDE_ABOVE:
        return
    # conf and wsum of conf_pool on the same logits, in both of its forms, bit for bit: the two-launch form runs this very kernel,
    # the one-launch form (up to 8 crops of up to 2048 logits) promises its operations in its order
    # (two launches: the crops repeated until they are more than 8; one launch: the first 8 crops at most)
    forms = [("k_weighted_colsum", b, -(-(TC.POOL_SMALL_MAX_CROPS + 1) // b))]
    if L <= TC.POOL_SMALL_MAX_LOGITS:
        forms.append(("k_conf_pool_small", min(b, TC.POOL_SMALL_MAX_CROPS), 1))
    for kernel, k, rep in forms:
        r1, r2 = _flat(l1[:k].repeat(rep, 1)), _flat(l2[:k].repeat(rep, 1))
        F1, F2 = torch.zeros((rep * k * n1, 4), device="cuda"), torch.zeros((rep * k * n2, 4), device="cuda")
        (pc, _, _, pws), ran = _census(lib, lambda: dcl.ops.conf_pool(rep * k, r1, r2, F1, F2))
        assert any(x.startswith(kernel) for x in ran) and (kernel == "k_weighted_colsum") == ("k_conf_softmax<256>" in ran), sorted(ran)
        assert TC.same_bits(pc[:k], conf[:k]) and TC.same_bits(pws[:k], ws[:k]), kernel


# ================================================================================================ 2. conf_pool
def _conf_pool_raw(dcl, b, l1, l2, F1, F2):
    """ops.conf_pool's own call of dcl_conf_pool with every output pre-filled with NaN: (conf, w, nslices, part1, part2, wsum)"""
    ops, N = dcl.ops, dcl.ops.N
    n1, n2, c = F1.shape[0] // b, F2.shape[0] // b, F1.shape[1]
    nslices = TC.pool_slices(b, c)
    nan = lambda *s: torch.full(s, float("nan"), device="cuda")                                  # noqa: E731
    conf, w, part1, part2, ws = nan(b, n1 + n2), nan(b, n1 + n2), nan(b, nslices, c), nan(b, nslices, c), nan(b, 2)
    N.check(N.lib().dcl_conf_pool(b, c, n1, n2, N.ptr(l1), N.ptr(l2), N.ptr(F1), ops._ld(F1), N.ptr(F2), ops._ld(F2), N.ptr(conf),
                                  N.ptr(w), nslices, N.ptr(part1), N.ptr(part2), N.ptr(ws), N.stream()), "conf_pool")
    return conf, w, nslices, part1, part2, ws


def _column_block(F):
    """F as a column block of a wider buffer (pitch c + 24, offset 8 floats), NaN around it"""
    rows, c = F.shape
    buf = torch.full((rows, c + TC.POOL_PAD), float("nan"), device="cuda")
    buf[:, TC.POOL_OFF:TC.POOL_OFF + c] = F
    return buf[:, TC.POOL_OFF:TC.POOL_OFF + c]


def _pool_form(b, n1, n2):
    return "k_conf_pool_small" if b <= TC.POOL_SMALL_MAX_CROPS and n1 + n2 <= TC.POOL_SMALL_MAX_LOGITS else "k_weighted_colsum"


@pytest.mark.parametrize("layout", ["contiguous", "column block"])
@pytest.mark.parametrize("i", range(len(TC.POOL_SHAPES)), ids=TC.POOL_IDS)
def test_conf_pool_matches_float64_on_both_sides_of_its_switch(request, dcl, i, layout):
    """dcl_conf_pool (+ dcl_pool_finish) against float64 in its one-launch form (up to 8 crops of up to 2048 logits) and its
    two-launch form, F contiguous and as a column block.  Fails if: the last (ragged) slice of a direction is dropped or a
    slice that owns no point is left unwritten, the channels behind the last whole 256-channel block are skipped, the row pitch
    is taken for the width, or direction 2 reads its weights from offset 0 instead of n1."""
    lib = TO.enter_diag(dcl, request)
    b, n1, n2, c = TC.POOL_SHAPES[i]
    k = TC.pool_case(i)
    ref, module = k["ref"], k["module"]
    l1, l2 = _flat(k["l1"]), _flat(k["l2"])
    F1, F2 = k["F1"].cuda().reshape(-1, c), k["F2"].cuda().reshape(-1, c)
    if layout == "column block":
        F1, F2 = _column_block(F1), _column_block(F2)
    aff = tuple(t.cuda() for t in k["affine"])
    (conf, w, ns, part1, part2, ws), ran = _census(lib, lambda: _conf_pool_raw(dcl, b, l1, l2, F1, F2))
    form = _pool_form(b, n1, n2)
    assert any(x.startswith(form) for x in ran) and (form == "k_weighted_colsum") == ("k_conf_softmax<256>" in ran), sorted(ran)
    assert bool(torch.isfinite(part1).all()) and bool(torch.isfinite(part2).all()), "a partial was left unwritten"
    for n, part in ((n1, part1), (n2, part2)):
        for s, (j0, j1) in enumerate(TC.slice_ranges(n, ns)):
            if j1 <= j0:
                assert bool((part[:, s] == 0).all()), ("a slice that owns no point is not 0", s)
    tag = "pool %s %s %s" % (TC.POOL_IDS[i], layout, form)
    TC.check(tag, "conf", conf, ref["conf"], module["conf"])
    TC.check(tag, "wsum", ws, ref["wsum"], module["wsum"])
    TC.check(tag, "pooled", part1.sum(1) + part2.sum(1), ref["pooled"], module["pooled"])
    conf2, finished = dcl.ops.conf_pool(b, l1, l2, F1, F2, affine=aff)
    TC.check(tag, "finished", finished, ref["finished"], module["finished"])
    conf3, (ns3, p1, p2, ws3) = dcl.ops.conf_pool(b, l1, l2, F1, F2, affine=aff, finish=False)
    assert ns3 == ns and TC.same_bits(conf2, conf) and TC.same_bits(conf3, conf) and TC.same_bits(ws3, ws)
    assert TC.same_bits(p1, part1) and TC.same_bits(p2, part2)


@pytest.mark.parametrize("i", range(len(TC.EXACT_POOL_SHAPES)), ids=TC.EXACT_POOL_IDS)
def test_conf_pool_exact_set_bit_for_bit(request, dcl, i):
    """logits 0 (every weight exactly 1 / L, L a power of two), integer F, dyadic affine: every fp32 sum is exact, so conf, wsum,
    pooled and the finish must be the float64 values bit for bit in both forms.  Fails if one row is weighted twice or dropped."""
    lib = TO.enter_diag(dcl, request)
    b, n1, n2, c = TC.EXACT_POOL_SHAPES[i]
    k = TC.exact_pool_case(i)
    ref = k["ref"]
    l1, l2 = _flat(k["l1"]), _flat(k["l2"])
    F1, F2 = k["F1"].cuda().reshape(-1, c), k["F2"].cuda().reshape(-1, c)
    aff = tuple(t.cuda() for t in k["affine"])
    (conf, p1, p2, ws), ran = _census(lib, lambda: dcl.ops.conf_pool(b, l1, l2, F1, F2))
    assert any(x.startswith(_pool_form(b, n1, n2)) for x in ran), sorted(ran)
    assert TC.same_bits(conf, ref["conf"].float()) and TC.same_bits(ws, ref["wsum"].float())
    assert TC.same_bits(p1, ref["P1"].float()) and TC.same_bits(p2, ref["P2"].float())
    assert TC.same_bits(dcl.ops.conf_pool(b, l1, l2, _column_block(F1), _column_block(F2), affine=aff)[1], ref["finished"].float())
    sconf, sw, sws = dcl.ops.conf_softmax(b, l1, l2)
    assert TC.same_bits(sconf, conf) and TC.same_bits(sws, ws) and bool((sw == 1.0 / (n1 + n2)).all())
    print("tail\tpool exact %s %s\tbit-equal" % (TC.EXACT_POOL_IDS[i], _pool_form(b, n1, n2)))


# ================================================================================================ 3. pool_finish2
def _pool_finish(dcl, part1, part2, ws, affine, ns):
    """dcl_pool_finish as ops.conf_pool calls it"""
    N = dcl.ops.N
    b, c = ws.shape[0], part1.shape[-1]
    out = torch.full((b, c), float("nan"), device="cuda")
    N.check(N.lib().dcl_pool_finish(b, c, ns, N.ptr(part1), N.ptr(part2), N.ptr(ws), *(N.ptr(t) for t in affine), N.ptr(out),
                                    N.stream()), "pool_finish")
    return out


@pytest.mark.parametrize("ns1,ns2", TC.FINISH_COUNTS, ids=["%dx%d" % p for p in TC.FINISH_COUNTS])
def test_pool_finish2_matches_float64(dcl, ns1, ns2):
    """dcl_pool_finish2 with unequal partial counts per direction and counts that are no multiple of 4, 1024 and 260 channels, 1 and
    9 crops: Gaussian operands under the rule, the exact set bit for bit.  Fails if ns1 / ns2 are swapped, the ns % 4 partials behind
    the last group of four are dropped, the two weight sums are swapped, or channel 256.. of a 260-channel row is not written."""
    for b in TC.FINISH_CROPS:
        for c in TC.FINISH_CHANNELS:
            for kind in ("gauss", "exact"):
                k = TC.finish_case(b, c, ns1, ns2, kind)
                p1, p2, ws = k["part1"].cuda(), k["part2"].cuda(), k["ws"].cuda()
                aff = tuple(t.cuda() for t in k["affine"])
                got = dcl.ops.pool_finish2(p1, p2, ws, aff)
                tag = "finish %dx%d b%d c%d %s" % (ns1, ns2, b, c, kind)
                if kind == "exact":
                    assert TC.same_bits(got, k["ref"].float()), tag
                    print("tail\t%s\tbit-equal" % tag)
                else:
                    TC.check(tag, "out", got, k["ref"], k["module"])
                assert TC.same_bits(got, dcl.ops.pool_finish2(p1, p2, ws, aff))
                if ns1 == ns2:
                    assert TC.same_bits(_pool_finish(dcl, p1, p2, ws, aff, ns1), got), tag


@pytest.fixture(scope="module")
def heads(dcl):
    """the synth network of tail_cases.heads64 on the GPU and its folded weights"""
    net = TC.heads_network().cuda().eval()
    return net, net._fold()


@pytest.mark.parametrize("ns", TC.PARTS_SLICES)
def test_pose_heads_parts_equal_finish_plus_heads_at_every_slice_count(dcl, heads, ns):
    """dcl_pose_heads_parts on given partials == dcl_pool_finish + dcl_pose_heads bit for bit at 1, 3, 4 and 64 slices (the code
    promises the same operations in the same order; the wrapper alone only ever picks one count).  Fails if the folded finish
    walks the rest slices in another order or reads part2 at part1's count."""
    _, f = heads
    b = 3
    k = TC.finish_case(b, 1024, ns, ns, "gauss")
    p1, p2, ws = k["part1"].cuda().view(b, ns, 1024), k["part2"].cuda().view(b, ns, 1024), k["ws"].cuda()
    aff = tuple(t.cuda() for t in k["affine"])
    pooled = _pool_finish(dcl, p1, p2, ws, aff, ns)
    TC.check("parts ns%d" % ns, "pooled", pooled, k["ref"], k["module"])
    want = dcl.ops.pose_heads(pooled, f["regressor_rot"], f["regressor_trans"], with_rotation=True)
    got = dcl.ops.pose_heads_parts((ns, p1, p2, ws), aff, f["regressor_rot"], f["regressor_trans"], with_rotation=True)
    for a, w in zip(got, want):
        assert TC.same_bits(a, w)


# ================================================================================================ 4. the pooling routes
def _check_heads(tag, o9, t3, ref, crops):
    r64, t64 = ref["o9"], ref["t3"]
    sel = torch.tensor(crops)
    e9 = float((o9.cpu().double()[sel] - r64).abs().max())
    e3 = float((t3.cpu().double()[sel] - t64).abs().max())
    lim9, lim3 = 2e-5 * max(1.0, float(r64.abs().max())), 2e-6 * max(1.0, float(t64.abs().max()) / 0.02)
    print("tail\t%s\to9 err=%.3g bound=%.3g\tt3 err=%.3g bound=%.3g" % (tag, e9, lim9, e3, lim3))
    assert e9 <= lim9 and e3 <= lim3, (tag, e9, lim9, e3, lim3)


@pytest.mark.parametrize("i", range(len(TC.ROUTE_SHAPES)), ids=TC.ROUTE_IDS)
def test_pooling_routes_against_one_float64_reference(dcl, heads, i):
    """The routes Network._dense_tail picks among by batch size, on the same operands against one float64 reference:
    (a) linear + conf_pool(finish=False) + pose_heads_parts, (b) linear + conf_pool(affine) + pose_heads, (c) conf_softmax +
    linear_pool per direction (direction 2's weights passed as w.view(-1)[n1:]) + pool_finish2 + pose_heads, (d) route b's pooled
    feature through the padded _mlp heads + ortho9d_to_matrix.  (a) == (b) bit for bit.  Fails if a route drops a tile, weighs
    direction 2 with direction 1's weights, or finishes with the directions' tile counts swapped."""
    net, f = heads
    ops = dcl.ops
    b, n1, n2, crops = TC.ROUTE_SHAPES[i]
    stress = i == len(TC.ROUTE_SHAPES) - 1
    k = TC.route_case(i)
    ref, module = k["ref"], k["module"]
    sel = torch.tensor(crops)
    H1, H2, W1, b1, W2, b2 = (k[n].cuda() for n in ("H1", "H2", "W1", "b1", "W2", "b2"))
    ops.prepare_linear(W1); ops.prepare_linear(W2)          # as the Network's folded fuser weights are
    l1, l2 = _flat(k["l1"]), _flat(k["l2"])
    aff = tuple(t.cuda() for t in k["affine"])
    rot, tr = f["regressor_rot"], f["regressor_trans"]
    tag = "route %s" % TC.ROUTE_IDS[i]
    F1, F2 = ops.linear(H1, W1, b1, True), ops.linear(H2, W2, b2, True)
    # (a)
    conf_a, parts = ops.conf_pool(b, l1, l2, F1, F2, affine=aff, finish=False)
    o9a, t3a, Ra = ops.pose_heads_parts(parts, aff, rot, tr, with_rotation=True)
    _check_heads(tag + " a", o9a, t3a, ref, crops)
    # (b)
    conf_b, pooled_b = ops.conf_pool(b, l1, l2, F1, F2, affine=aff)
    del F1, F2
    TC.check(tag + " b", "pooled", pooled_b[sel.cuda()], ref["finished"], module["finished"])
    TC.check(tag + " b", "conf", conf_b[sel.cuda()], ref["conf"], module["conf"])
    o9b, t3b, Rb = ops.pose_heads(pooled_b, rot, tr, with_rotation=True)
    assert TC.same_bits(conf_a, conf_b) and TC.same_bits(o9a, o9b) and TC.same_bits(t3a, t3b) and TC.same_bits(Ra, Rb)
    # (c)
    L = n1 + n2
    conf_c, w, ws = ops.conf_softmax(b, l1, l2)
    part1 = ops.linear_pool(H1, W1, b1, w.view(-1), relu=True, rows_per_crop=n1, w_stride=L)
    part2 = ops.linear_pool(H2, W2, b2, w.view(-1)[n1:], relu=True, rows_per_crop=n2, w_stride=L)
    T = ops.LINEAR_POOL_TILE
    assert part1.shape == (b * n1 // T, 1024) and part2.shape == (b * n2 // T, 1024)
    pooled_c = ops.pool_finish2(part1, part2, ws, aff)
    TC.check(tag + " c", "pooled", pooled_c[sel.cuda()], ref["finished"], module["finished"])
    TC.check(tag + " c", "conf", conf_c[sel.cuda()], ref["conf"], module["conf"])
    o9c, t3c, Rc = ops.pose_heads(pooled_c, rot, tr, with_rotation=True)
    _check_heads(tag + " c", o9c, t3c, ref, crops)
    assert float((Rc - Rb).abs().max()) <= R_TOL
    if stress:
        return
    # (d)
    t3d = net._mlp(pooled_b, f["regressor_trans_padded"])
    o9d = net._mlp(pooled_b, f["regressor_rot_padded"])
    Rd = ops.ortho9d_to_matrix(o9d)
    _check_heads(tag + " d", o9d, t3d, ref, crops)
    assert float((Rd - Rb).abs().max()) <= R_TOL
    eye = torch.eye(3, dtype=torch.float64, device="cuda")
    assert float((Rd.double() @ Rd.double().transpose(1, 2) - eye).abs().max()) <= 1e-5


# ================================================================================================ 5. the network's route
@pytest.mark.parametrize("b,n_inp,n_tmp", [(8, 128, 128), (9, 128, 128), (9, 128, 100), (129, 128, 128)])
def test_network_takes_the_route_its_size_calls_for(request, dcl, b, n_inp, n_tmp):
    """which tail kernels one launch-by-launch forward runs (launch census) on either side of POSE_PARTS_MAX, of the point counts
    that tile the pooling GEMM, and of POSE_HEADS_MAX; crops 0 and b - 1 must agree with the same crops run alone.  Fails if a
    threshold moves without its route being tested, or if a route's result depends on a crop's batch mates."""
    lib = TO.enter_diag(dcl, request)
    N = dcl.DCL_Net.Network
    net = N(dcl.synth.default_cfg(n_inp, n_tmp), mode="test", graph_max_batch=0)
    net.load_state_dict(dcl.synth.synth_state_dict(net, 1))
    net = net.cuda().eval()
    data = dcl.synth.make_batch(b, n_inp, n_tmp)
    with torch.no_grad():
        full, ran = _census(lib, lambda: net(data))
    tail = [k for k in sorted(ran) if k.startswith(("k_conf_", "k_weighted_", "k_pool_", "k_heads_", "k_ortho9d"))] + _pool_gemms(ran)
    print("tail\tnetwork b%d %dx%d\t%s" % (b, n_inp, n_tmp, " ".join(tail)))
    has = lambda p: bool(_starts(ran, p))                                                        # noqa: E731
    tiles = n_inp % dcl.ops.LINEAR_POOL_TILE == 0 and n_tmp % dcl.ops.LINEAR_POOL_TILE == 0
    if b <= N.POSE_PARTS_MAX:
        assert has("k_conf_pool_small") and "k_heads_l1<true>" in ran
        assert not (has("k_conf_softmax") or has("k_weighted_colsum") or has("k_pool_finish") or _pool_gemms(ran)), tail
    elif tiles:
        assert "k_conf_softmax<256>" in ran and _pool_gemms(ran) and has("k_pool_finish")
        assert not (has("k_weighted_colsum") or has("k_conf_pool_small")), tail
    else:
        assert "k_conf_softmax<256>" in ran and has("k_weighted_colsum") and has("k_pool_finish") and not _pool_gemms(ran), tail
        assert not has("k_conf_pool_small"), tail
    if N.POSE_PARTS_MAX < b <= N.POSE_HEADS_MAX:
        assert "k_heads_l1<false>" in ran and has("k_heads_l23") and not has("k_ortho9d"), tail
    if b > N.POSE_HEADS_MAX:
        assert not has("k_heads_") and has("k_ortho9d"), tail
    assert tuple(full["rot_pred"].shape) == (b, 3, 3) and tuple(full["conf"].shape) == (b, n_inp + n_tmp)
    for i in (0, b - 1):
        with torch.no_grad():
            one = net(dcl.synth.make_batch(1, n_inp, n_tmp, first=i))
        dR = float((one["rot_pred"][0] - full["rot_pred"][i]).abs().max())
        dt = float((one["trans_pred"][0] - full["trans_pred"][i]).abs().max())
        dc = float((one["conf"][0] - full["conf"][i]).abs().max())
        print("tail\tnetwork b%d %dx%d crop %d\tdR=%.3g dt=%.3g dconf=%.3g" % (b, n_inp, n_tmp, i, dR, dt, dc))
        assert dR <= R_TOL and dt <= T_TOL and dc <= CONF_TOL, (i, dR, dt, dc)


# ================================================================================================ 6. attention
SENT = 12345.0


def _attn_call(dcl, lib, b, Q, K, V1, O1, O2, conc, planes, forced=0):
    """one ops.cross_attention call with V2 the very tensor passed as K; returns the attention kernels that ran"""
    keep = dcl.ops.ATTENTION_SPLIT
    dcl.ops.ATTENTION_SPLIT = planes
    lib.dcl_debug_attention_split(forced)
    try:
        _, ran = _census(lib, lambda: dcl.ops.cross_attention(b, Q, K, V1, O1, K, O2, concurrent=conc))
    finally:
        lib.dcl_debug_attention_split(0)
        dcl.ops.ATTENTION_SPLIT = keep
    return {k for k in ran if k.startswith(("k_cross_attn", "k_attn_split"))}


def _attn_err(tag, O, k, b, nq):
    worst = 0.0
    for i, want in k["want"].items():
        e = float((O[i * nq:(i + 1) * nq].cpu().double() - want).abs().max())
        lim = TC.ATTN_TOL * max(1.0, float(want.abs().max()))
        print("tail\t%s crop %d\tmax|want|=%.3g\terr=%.3g\tbound=%.3g" % (tag, i, float(want.abs().max()), e, lim))
        assert e <= lim, (tag, i, e, lim)
        worst = max(worst, e)
    return worst


@pytest.mark.parametrize("case", list(TC.ATTN_CASES))
def test_cross_attention_in_the_network_calling_form(request, dcl, case):
    """every product attention kernel the way Network._dense_tail calls it: O1 / O2 the right, then the left halves of (rows + 3,
    512) / (rows + 3, 128) buffers, V2 the very tensor passed as K, Q and K column blocks (pitch 136, offset 8), both axes ragged.
    Fails if: ldo2 is ignored (O2's rows land at pitch 64), a pitch is taken for the width, a row past b * nq is written (guard
    rows), the 3 padded keys of the last tile are counted, or the result depends on the operands' layout."""
    lib = TO.enter_diag(dcl, request)
    b, nq, nk, conc, planes, kernels, combine = TC.ATTN_CASES[case]
    k = TC.attn_case(b, nq, nk)
    rows = b * nq
    wide = lambda t: torch.full((t.shape[0], TC.ATTN_PITCH), SENT, device="cuda")                # noqa: E731
    QB, KB = wide(k["Q"]), wide(k["K"])
    Q, K = QB[:, TC.ATTN_OFF:TC.ATTN_OFF + 64], KB[:, TC.ATTN_OFF:TC.ATTN_OFF + 64]
    Q.copy_(k["Q"]); K.copy_(k["K"])
    V1 = k["V1"].cuda()
    Oc1, Oc2 = torch.full((rows, 256), SENT, device="cuda"), torch.full((rows, 64), SENT, device="cuda")
    ran = _attn_call(dcl, lib, b, Q.contiguous(), K.contiguous(), V1, Oc1, Oc2, conc, planes)
    assert ran - {"k_cross_attn_combine"} == set(kernels) and ("k_cross_attn_combine" in ran) == combine, sorted(ran)
    _attn_err("attention %s contiguous" % case, torch.cat([Oc1, Oc2], 1), k, b, nq)
    for right in (True, False):
        B1 = torch.full((rows + TC.ATTN_GUARD, 512), SENT, device="cuda")
        B2 = torch.full((rows + TC.ATTN_GUARD, 128), SENT, device="cuda")
        c1, c2 = (slice(256, 512), slice(64, 128)) if right else (slice(0, 256), slice(0, 64))
        O1, O2 = B1[:rows, c1], B2[:rows, c2]
        ran = _attn_call(dcl, lib, b, Q, K, V1, O1, O2, conc, planes)
        assert ran - {"k_cross_attn_combine"} == set(kernels) and ("k_cross_attn_combine" in ran) == combine, sorted(ran)
        assert TC.same_bits(O1, Oc1) and TC.same_bits(O2, Oc2), "the result depends on the operands' layout"
        for buf, cols in ((B1, c1), (B2, c2)):
            keep = torch.ones_like(buf, dtype=torch.bool)
            keep[:rows, cols] = False
            assert bool((buf[keep] == SENT).all()), "written outside the output block"
    assert bool((QB[:, :TC.ATTN_OFF] == SENT).all()) and bool((KB[:, TC.ATTN_OFF + 64:] == SENT).all())


# (b, nq, concurrent, planes) -> the kernels of the call, whatever the key count below
_ATTN_KERNELS = {
    "dma4": ((128, 200, 1, True), {"k_cross_attn_dma<4>"}),
    "dma4 few": ((2, 200, 1, True), {"k_cross_attn_dma<4>"}),          # few workgroups: the launch that splits its keys when it can
    "dma4 short": ((3, 33, 1, True), {"k_cross_attn_dma<4>"}),         # fewer than 64 queries per crop
    "dma8": ((128, 500, 1, False), {"k_cross_attn_dma<8>"}),
    "split": ((128, 200, 2, True), {"k_attn_split_v", "k_attn_split_k", "k_cross_attn_split"}),
}


def _attn_plain(dcl, lib, name, nk, kind, forced=0):
    (b, nq, conc, planes), kernels = _ATTN_KERNELS[name]
    k = TC.attn_case(b, nq, nk, kind)
    Q, K, V1 = k["Q"].cuda(), k["K"].cuda(), k["V1"].cuda()
    O1, O2 = torch.full((b * nq, 256), SENT, device="cuda"), torch.full((b * nq, 64), SENT, device="cuda")
    ran = _attn_call(dcl, lib, b, Q, K, V1, O1, O2, conc, planes, forced)
    assert ran - {"k_cross_attn_combine"} == kernels, (name, nk, sorted(ran))
    return k, torch.cat([O1, O2], 1), "k_cross_attn_combine" in ran


@pytest.mark.parametrize("name", ["dma4", "dma4 short", "dma8", "split"])
def test_cross_attention_of_one_key_returns_its_value_row(request, dcl, name):
    """nk = 1: P = exp(0) = 1, l = 1, and the three bf16 pieces of a value sum to it exactly -- every output row is the key's
    [V1 | V2] row bit for bit.  Fails if one of the 31 padded keys of the tile weighs anything.  (A key split needs at least
    two 32-key tiles per split: with 1, 31 or 33 keys the plan cannot produce k_cross_attn_combine, asserted here.)"""
    lib = TO.enter_diag(dcl, request)
    (b, nq, _, _), _ = _ATTN_KERNELS[name]
    k, O, combined = _attn_plain(dcl, lib, name, 1, "gauss")
    assert not combined
    V = torch.cat([k["V1"], k["K"]], 1).view(b, 1, 320).expand(b, nq, 320).reshape(b * nq, 320)
    assert TC.same_bits(O, V)
    print("tail\tattention %s nk=1\tbit-equal" % name)


@pytest.mark.parametrize("nk", [31, 33])
@pytest.mark.parametrize("name", ["dma4", "dma4 short", "dma8", "split"])
def test_cross_attention_just_below_and_above_one_key_tile(request, dcl, name, nk):
    """31 and 33 keys (one ragged tile; one whole tile and one key) with Gaussian operands against float64.  Fails if the ragged
    tile's padded keys are counted or the lone key of the second tile is dropped."""
    lib = TO.enter_diag(dcl, request)
    (b, nq, _, _), _ = _ATTN_KERNELS[name]
    k, O, combined = _attn_plain(dcl, lib, name, nk, "gauss")
    assert not combined
    _attn_err("attention %s nk=%d" % (name, nk), O, k, b, nq)


@pytest.mark.parametrize("forced", [0, 2])
@pytest.mark.parametrize("nk", [64, 128])
@pytest.mark.parametrize("name", ["dma4", "dma4 few", "dma8", "split"])
def test_cross_attention_of_zero_queries_is_the_exact_mean(request, dcl, name, nk, forced):
    """Q = 0 with integer values: every score is 0, every weight 1, the output sum(V) / nk exactly (nk a power of two) -- bit for
    bit against float64 on every crop, also with the key split forced to 2 (dcl_debug_attention_split; it takes effect from four
    key tiles on, i.e. at nk = 128).  Fails if a padded key is counted, a tile is visited twice, or the combine weighs a split twice."""
    lib = TO.enter_diag(dcl, request)
    (b, nq, _, _), _ = _ATTN_KERNELS[name]
    k, O, combined = _attn_plain(dcl, lib, name, nk, "zeroq", forced)
    if name.startswith("dma4"):
        assert combined == (forced == 2 and nk == 128), (name, nk, forced, combined)
    V = torch.cat([k["V1"], k["K"]], 1).view(b, nk, 320).double()
    want = (V.sum(1) / nk).float().view(b, 1, 320).expand(b, nq, 320).reshape(b * nq, 320)
    assert TC.same_bits(O, want)
    print("tail\tattention %s nk=%d forced=%d combine=%s\tbit-equal" % (name, nk, forced, combined))


@pytest.mark.parametrize("name", ["dma4", "dma8", "split"])
def test_cross_attention_with_strongly_negative_scores(request, dcl, name):
    """every real score about -60 at nk = 61: the 3 padded keys of the last tile (score -inf, not 0) must weigh nothing -- with a
    padded key scored 0 it would outweigh all real keys by e^60.  Gaussian bound against float64."""
    lib = TO.enter_diag(dcl, request)
    (b, nq, _, _), _ = _ATTN_KERNELS[name]
    k, O, _ = _attn_plain(dcl, lib, name, 61, "neg60")
    s = k["K"][:61].double() @ k["Q"][:nq].double().t()
    assert -75 < float(s.min()) and float(s.max()) < -45
    _attn_err("attention %s neg60" % name, O, k, b, nq)


def test_cross_attention_refuses_unaligned_operands(dcl):
    """a pitch that is no multiple of 4 floats and an operand 4 bytes off 16-byte alignment are refused (RuntimeError) before
    anything is launched: the outputs keep their sentinel"""
    b, nq, nk = 2, 200, 61
    k = TC.attn_case(b, nq, nk)
    Q, K, V1 = k["Q"].cuda(), k["K"].cuda(), k["V1"].cuda()
    O1, O2 = torch.full((b * nq, 256), SENT, device="cuda"), torch.full((b * nq, 64), SENT, device="cuda")
    odd = torch.full((b * nq, 258), SENT, device="cuda")
    with pytest.raises(RuntimeError):
        dcl.ops.cross_attention(b, Q, K, V1, odd[:, :256], K, O2)
    flat = torch.zeros(b * nq * 64 + 4, device="cuda")
    off = flat[1:1 + b * nq * 64].view(b * nq, 64)
    off.copy_(Q)
    assert off.data_ptr() % 16 == 4
    with pytest.raises(RuntimeError):
        dcl.ops.cross_attention(b, off, K, V1, O1, K, O2)
    torch.cuda.synchronize()
    assert bool((odd == SENT).all()) and bool((O1 == SENT).all()) and bool((O2 == SENT).all())
