"""CPU checks of tests/tail_cases.py, the cases tests/test_gpu_eval_tail.py holds the dense tail's kernels against: the float64
references agree with the literal module lines run in double, the exact sets are exact, every threshold-named shape sits on the
side of its threshold its name says, and the deliberately wrong references show beyond the bounds the GPU tests assert."""
import importlib

import pytest
import torch

import conf_pool_cases as CP
import tail_cases as TC


def _close(a, b, tol=1e-12):
    return float((a.double() - b.double()).abs().max()) <= tol * max(1.0, float(b.abs().max()))


# ------------------------------------------------------------------------------------------------ references
@pytest.mark.parametrize("kind", TC.LOGIT_SETS)
@pytest.mark.parametrize("i", range(len(TC.SOFTMAX_SHAPES)), ids=TC.SOFTMAX_IDS)
def test_softmax_reference_is_the_module_lines_in_double(i, kind):
    l1, l2, ref, _ = TC.softmax_case(i, kind)
    m = TC.module_lines(l1[:, None].double(), l2[:, None].double())
    for name in ("conf", "w", "wsum"):
        assert _close(ref[name], m[name]), (name, kind)
    assert float((ref["w"].sum(1) - 1).abs().max()) <= 1e-12 and bool((ref["w"] > 0).all())


def test_module_lines_are_the_lines_of_conf_pool_cases():
    """tail_cases.module_lines (no autograd, plus the affine finish) restates conf_pool_cases.module_form: same values in double"""
    k = CP.random_case(2)
    names = ("logit1", "logit2", "F1", "F2", "g_conf", "g_pooled")
    want = CP.module_form(*(k[n].double() for n in names))
    got = TC.module_lines(k["logit1"].double(), k["logit2"].double(), k["F1"].double(), k["F2"].double())
    assert _close(got["conf"], want["conf"], 1e-15) and _close(got["pooled"], want["pooled"], 1e-15)


@pytest.mark.parametrize("i", range(len(TC.POOL_SHAPES)), ids=TC.POOL_IDS)
def test_pool_reference_is_the_module_lines_in_double(i):
    """sA sum w F1 + tA sum w1 + ... (BatchNorm after the pooling, as the kernels finish it) == the module's BatchNorm before it"""
    k = TC.pool_case(i)
    m = TC.pool_module(k["l1"], k["l2"], k["F1"], k["F2"], k["affine"], torch.float64)
    for name in ("conf", "wsum", "pooled", "finished"):
        assert _close(k["ref"][name], m[name]), name


@pytest.mark.parametrize("i", range(len(TC.ROUTE_SHAPES) - 1), ids=TC.ROUTE_IDS[:-1])
def test_route_reference_is_the_module_lines_in_double(i):
    """(the stress shape's reference is the same function on more rows: built by the GPU test only)"""
    k = TC.route_case(i)
    b, n1, n2, crops = TC.ROUTE_SHAPES[i]
    sel = torch.tensor(crops)
    F = lambda H, W, bias: torch.relu(H.double() @ W.double() + bias.double())               # noqa: E731
    m = TC.pool_module(k["l1"][sel], k["l2"][sel], F(k["H1"].view(b, n1, 512)[sel], k["W1"], k["b1"]),
                       F(k["H2"].view(b, n2, 512)[sel], k["W2"], k["b2"]), k["affine"], torch.float64)
    assert _close(k["ref"]["finished"], m["finished"])
    net = TC.heads_network().double()
    with torch.no_grad():
        o9 = net.regressor_rot(m["finished"].unsqueeze(2)).squeeze(2)
        t3 = net.regressor_trans(m["finished"].unsqueeze(2)).squeeze(2)
    assert _close(k["ref"]["o9"], o9) and _close(k["ref"]["t3"], t3) and tuple(t3.shape) == (len(crops), 3)


def test_finish_reference_and_its_module_form():
    for b in TC.FINISH_CROPS:
        for ns1, ns2 in TC.FINISH_COUNTS:
            k = TC.finish_case(b, 260, ns1, ns2, "gauss")
            m = TC.finish_module(k["part1"].double(), k["part2"].double(), k["ws"].double(), tuple(t.double() for t in k["affine"]),
                                 ns1, ns2)
            assert _close(k["ref"], m)


# ------------------------------------------------------------------------------------------------ exact sets
@pytest.mark.parametrize("i", range(len(TC.EXACT_POOL_SHAPES)), ids=TC.EXACT_POOL_IDS)
def test_exact_pool_sets_are_exact(i):
    """L a power of two, every weight 1 / L, sum |F| an integer below 2^24 per (crop, channel): every partial sum of the pooling
    in any order is k / L with |k| < 2^24, and so is the finish -- fp32 holds them all, the fp32 evaluation IS the float64 one"""
    b, n1, n2, c = TC.EXACT_POOL_SHAPES[i]
    k = TC.exact_pool_case(i)
    L = n1 + n2
    assert L & (L - 1) == 0
    r = k["ref"]
    assert bool((r["conf"] == 0.5).all()) and bool((r["w"] == 1.0 / L).all())
    sA, tA, sB, tB = k["affine"]
    worst = 2 * (k["F1"].abs().sum(1) + n1 * tA.abs()).max() + 2 * (k["F2"].abs().sum(1) + n2 * tB.abs()).max()
    assert float(worst) < 2 ** 24
    assert bool((k["F1"] == k["F1"].round()).all()) and set(sA.tolist()) | set(sB.tolist()) <= {0.5, 1.0, 2.0}
    for name in ("pooled", "finished", "wsum", "P1", "P2"):
        assert bool((r[name].float().double() == r[name]).all()), name
    w32 = torch.full((b, L), 1.0 / L)
    got = torch.einsum("bjc,bj->bc", k["F1"], w32[:, :n1]) + torch.einsum("bjc,bj->bc", k["F2"], w32[:, n1:])
    assert TC.same_bits(got, r["pooled"].float())


def test_exact_finish_sets_are_exact():
    for b in TC.FINISH_CROPS:
        for c in TC.FINISH_CHANNELS:
            for ns1, ns2 in TC.FINISH_COUNTS:
                k = TC.finish_case(b, c, ns1, ns2, "exact")
                assert float(2 * 9 * max(ns1, ns2) * 2 + 2 * 3) < 2 ** 24
                assert bool((k["ref"].float().double() == k["ref"]).all())
                assert TC.same_bits(k["module"], k["ref"].float())


def test_exact_attention_mean_is_exact():
    """zero queries: the output is sum(V) / nk with integer V and nk a power of two"""
    for nk in (64, 128):
        k = TC.attn_case(2, 200, nk, "zeroq")
        for i, want in k["want"].items():
            V = torch.cat([k["V1"], k["K"]], 1)[i * nk:(i + 1) * nk]
            assert bool((want == (V.double().sum(0) / nk)[None]).all()) and bool((want.float().double() == want).all())
            # count a padded key (the clamped last row once more): every channel whose last value is not the mean moves
            wrong = (V.double().sum(0) + V[-1].double()) / (nk + 1)
            assert float((wrong - want[0]).abs().max()) > 1e-3


# ------------------------------------------------------------------------------------------------ thresholds
def test_shapes_cross_the_switches_they_are_named_for():
    dcl = importlib.import_module("dcl-net_amd")
    wide, small_crops, small_logits = TC.source_thresholds()
    assert (wide, small_crops, small_logits) == (TC.SOFTMAX_WIDE_ABOVE, TC.POOL_SMALL_MAX_CROPS, TC.POOL_SMALL_MAX_LOGITS)
    L = lambda s: s[1] + s[2]                                                                # noqa: E731
    S = TC.SOFTMAX_SHAPES
    assert L(S[5]) == wide and L(S[6]) == wide + 1 and L(S[7]) > wide and L(S[8]) > wide and L(S[8]) % 1024 and S[8][1] % 64
    assert all(L(s) <= wide for s in S[:5])
    P = TC.POOL_SHAPES
    small = lambda s: s[0] <= small_crops and L(s) <= small_logits                           # noqa: E731
    assert P[0][0] == small_crops and small(P[0]) and P[1][0] == small_crops + 1 and P[1][1:] == P[0][1:] and not small(P[1])
    assert P[2][0] <= small_crops and L(P[2]) == small_logits + 1
    for s, d in ((P[3], 1), (P[4], 2)):                                    # a direction with fewer points than slices
        ns = TC.pool_slices(s[0], s[3])
        assert s[d] < ns and [j1 <= j0 for j0, j1 in TC.slice_ranges(s[d], ns)].count(True) == ns - s[d] and small(s)
    assert P[5][3] % TC.POOL_CHANNEL_BLOCK == 4 and P[5][3] > TC.POOL_CHANNEL_BLOCK
    assert any(j1 <= j0 for j0, j1 in TC.slice_ranges(P[5][2], TC.pool_slices(P[5][0], P[5][3])))
    assert P[6][0] > small_crops
    E = TC.EXACT_POOL_SHAPES
    assert small(E[0]) and E[1][0] > small_crops and L(E[1]) <= small_logits and E[2][0] <= small_crops < L(E[2]) > small_logits
    # the routes of Network._dense_tail: parts up to POSE_PARTS_MAX crops, the pooling epilogue beyond where both point counts tile
    N = dcl.DCL_Net.Network
    T = dcl.ops.LINEAR_POOL_TILE
    R = TC.ROUTE_SHAPES
    assert R[0][0] <= N.POSE_PARTS_MAX < R[1][0] <= N.POSE_HEADS_MAX and all(s[1] % T == 0 and s[2] % T == 0 for s in R)
    assert R[1][1] != R[1][2] and R[2][1] // T != R[2][2] // T and R[2][1] // T % 4 != 0     # unequal tile counts, no multiple of 4
    assert (R[3][1] // T, R[3][2] // T) == (96, 16) and (96, 16) in TC.FINISH_COUNTS
    assert max(TC.PARTS_SLICES) == TC.pool_slices(1, 1024) and 3 in TC.PARTS_SLICES and 4 in TC.PARTS_SLICES
    # attention: the ragged sizes stay inside their plan entries (same 256-query and 32-key tile counts as the aligned ones)
    for (b, nq, nk, *_), (nq0, nk0) in zip(TC.ATTN_CASES.values(), ((256, 64), (256, 256), (512, 64), (256, 64))):
        assert -(-nq // 256) == nq0 // 256 and -(-nk // 32) == nk0 // 32 and nq % 32 and nk % 32
    assert TC.ATTN_PITCH % 4 == 0 and TC.ATTN_OFF % 4 == 0 and TC.ATTN_PITCH >= TC.ATTN_OFF + 64


# ------------------------------------------------------------------------------------------------ the wrong twins show
def test_a_wrong_reduction_tree_shows_in_the_softmax_reference():
    """the 256-thread tree in the 1024-thread kernel = only 4 of 16 wave sums in the normaliser: the weights no longer sum to 1
    (the GPU test asserts |sum - 1| <= 1e-6) and leave the rule's bound by orders of magnitude"""
    i = TC.SOFTMAX_SHAPES.index((2, 2048, 2049))
    l1, l2, ref, module = TC.softmax_case(i, "gauss")
    wrong = TC.softmax64(l1, l2, wave_tree=4)
    assert float((wrong["w"].sum(1) - 1).abs().min()) > 1.0
    for name in ("w", "wsum"):
        assert float((wrong[name] - ref[name]).abs().max()) > 1e3 * TC.bound(ref[name], module[name])[0]


def test_one_dropped_slice_shows_in_the_pool_reference():
    """the last non-empty slice of a direction left out moves pooled / finished past the bound the GPU test asserts, at every shape"""
    for i, (b, n1, n2, c) in enumerate(TC.POOL_SHAPES):
        k = TC.pool_case(i)
        for d, n in ((0, n1), (1, n2)):
            j0, j1 = [r for r in TC.slice_ranges(n, TC.pool_slices(b, c)) if r[1] > r[0]][-1]
            wrong = TC.pool64(k["l1"], k["l2"], k["F1"], k["F2"], k["affine"], skip=(d, j0, j1))
            for name in ("pooled", "finished"):
                assert float((wrong[name] - k["ref"][name]).abs().max()) > 10 * TC.bound(k["ref"][name], k["module"][name])[0], (i, d, name)


def test_dropped_rest_partials_and_swapped_weight_sums_show_in_the_finish_reference():
    for ns1, ns2 in TC.FINISH_COUNTS:
        k = TC.finish_case(9, 260, ns1, ns2, "gauss")
        lim = TC.bound(k["ref"], k["module"])[0]
        args = (k["part1"], k["part2"], k["ws"], k["affine"], ns1, ns2)
        assert float((TC.finish64(*args, swap_ws=True) - k["ref"]).abs().max()) > 1e3 * lim
        if ns1 % 4 or ns2 % 4:
            assert float((TC.finish64(*args, drop_rest=True) - k["ref"]).abs().max()) > 1e3 * lim
        if ns1 != ns2:                                                     # ns1 / ns2 swapped: another crop's rows are read
            sw = TC.finish64(k["part1"][:9 * min(ns1, ns2)], k["part2"][:9 * min(ns1, ns2)], k["ws"], k["affine"], min(ns1, ns2), min(ns1, ns2))
            assert float((sw - k["ref"]).abs().max()) > 1e3 * lim
