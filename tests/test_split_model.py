"""The CPU side of tests/test_gpu_split_arithmetic.py: every bound a GPU test asserts is held, on exactly the operands the GPU test
uses (tests/split_cases.py), by the model of the split-bf16 arithmetic -- and is violated by the mutants a GPU test must not
pass: a kernel that lost one of its six piece products, or whose split chops instead of rounding.  No GPU needed."""
import math

import pytest
import torch

import split_cases as SC


def _violates(got, x, Wt, bias, relu, allowed):
    """does any output exceed its allowance (units, per row)?"""
    return bool((SC.unit_map(got, x, Wt, bias, relu) > allowed.view(-1, 1)).any())


def test_three_pieces_sum_to_the_operand():
    """h + m + l == v in float64 for every operand of the range and sparse builders of magnitude >= 2^-110; below that the third
    piece is a bf16 subnormal and what is left over is at most 2^-133 (half a bf16 subnormal step of 2^-133, rounded up)"""
    vals = torch.cat([t.reshape(-1) for name in SC.RANGE_SETS for t in SC.range_case(name)] +
                     [t.reshape(-1) for shape in SC.SPARSE_SHAPES for t in SC.sparse_case(*shape)[:2]])
    h, m, l = SC.split3(vals)
    left = (vals.double() - (h.double() + m.double() + l.double())).abs()
    big = vals.abs() >= 2.0 ** -110
    assert int(big.sum()) > 10000 and int((~big & (vals != 0)).sum()) > 10000
    assert float(left[big].max()) == 0.0
    assert float(left[~big].max()) <= 2.0 ** -133
    for piece in (h, m, l):
        assert torch.equal(piece, SC.rn_bf16(piece))


@pytest.mark.parametrize("shape", SC.SPARSE_SHAPES)
@pytest.mark.parametrize("with_bias,relu", [(False, False), (True, True)])
def test_sparse_row_bounds_hold_in_the_model_and_catch_every_mutant(shape, with_bias, relu):
    x, Wt, bias, s = SC.sparse_case(*shape)
    bias = bias if with_bias else None
    assert set(s.tolist()) == {1, 2, 3}
    nz = (x != 0)
    M, K, _ = shape
    assert bool(nz.view(M, K // 16, 16).any(0).all()), "a non-zero at every k position of every chunk"
    assert bool(nz[s == 1][:, torch.arange(K)].any(0).all()), "... and from one-hot rows alone"
    allowed = SC.sparse_bound_split(s, with_bias).double()
    assert not _violates(SC.model_split_gemm(x, Wt, None, bias, relu), x, Wt, bias, relu, allowed)
    assert not _violates(SC.model_fma_chain(x, Wt, bias, relu), x, Wt, bias, relu, SC.sparse_bound_fp32(s, with_bias).double())
    for drop in range(6):
        assert _violates(SC.model_split_gemm(x, Wt, drop, bias, relu), x, Wt, bias, relu, allowed), drop
    if not with_bias:       # (a chopping split is off by at most 7.8 units on a one-hot row: above the 7 allowed without a bias only)
        assert _violates(SC.model_split_gemm(x, Wt, None, bias, relu, rnd=SC.trunc_bf16), x, Wt, bias, relu, allowed)


@pytest.mark.parametrize("K,N", SC.DENSE_KN)
@pytest.mark.parametrize("name", SC.DENSE_SETS)
def test_dense_rows_the_model_stays_within_the_fp32_chain(name, K, N):
    x, Wt, _ = SC.dense_case(name, K, N)
    chain = SC.chain_units(name, K, N)
    got = SC.units(SC.model_split_gemm(x, Wt), x, Wt)
    assert 0.0 < chain <= K and got <= SC.SPLIT_OVER_CHAIN * chain, (name, K, N, got, chain)
    if name == "same_sign_l":
        for t in (x, Wt):
            h, m, l = SC.split3(t)
            assert bool((l > 0).all()) and bool((m > 0).all())
    if name == "cancelling":
        y = SC.reference(x, Wt).abs() / SC.magnitude(x, Wt)
        assert float(y.median()) < 3e-4


@pytest.mark.parametrize("name", SC.RANGE_SETS)
def test_range_operands_the_model_stays_within_the_fp32_chain(name):
    x, Wt = SC.range_case(name)
    M, K, N = SC.RANGE_SHAPE
    chain = SC.chain_units(name, K, N)
    err = (SC.model_split_gemm(x, Wt).double() - SC.reference(x, Wt)).abs()
    allowed = SC.SPLIT_OVER_CHAIN * chain * SC.U * SC.magnitude(x, Wt)
    if name == "tiny":
        allowed = allowed + SC.tiny_allowance(Wt)
    assert bool((err <= allowed).all()), (name, float((err / allowed).max()))


def test_an_operand_whose_first_piece_overflows_is_not_a_number_in_the_model():
    """RN_bf16 of |v| >= 0x7F7F8000 is inf: m = -inf, l = NaN, and a NaN piece poisons every product of the row"""
    v = torch.tensor([SC.H_OVERFLOWS, SC.H_OVERFLOWS - 1, 0x7F7FFFFF], dtype=torch.int32).view(torch.float32)
    h, m, l = SC.split3(v)
    assert math.isinf(float(h[0])) and math.isnan(float(l[0])) and math.isnan(float(l[2]))
    assert bool(torch.isfinite(torch.stack([h[1], m[1], l[1]])).all())
    assert float(v[0]) == pytest.approx(3.3962e38, rel=1e-4)


@pytest.mark.parametrize("M,K,N,rpc", SC.POOL_CASES)
def test_pooling_epilogue_bound_holds_in_the_model(M, K, N, rpc):
    x, Wt, bias, roww = SC.pool_case(M, K, N, rpc)
    w = SC.pool_row_weights(roww, M, rpc)
    assert int((w == 0).sum()) > 0 and int((w < 0).sum()) > 0
    want, mag = SC.pool_reference(x, Wt, bias, w)
    allowed = SC.epilogue_bound(SC.SPLIT_OVER_CHAIN * SC.pool_chain_units(M, K, N, rpc), SC.POOL_FMAS) * SC.U * mag
    for drop, ok in ((None, True), (5, False)):
        got = SC.model_pool(SC.model_split_gemm(x, Wt, drop, bias, True), w)
        assert bool(((got.double() - want).abs() <= allowed).all()) == ok, drop


@pytest.mark.parametrize("M,N", SC.ROWDOT_CASES)
def test_row_dot_epilogue_bound_holds_in_the_model(M, N):
    x, Wt, bias, w3, b3 = SC.rowdot_case(M, N)
    want, mag = SC.rowdot_reference(x, Wt, bias, w3, b3)
    allowed = SC.epilogue_bound(SC.SPLIT_OVER_CHAIN * SC.rowdot_chain_units(M, N), SC.ROWDOT_FMAS) * SC.U * mag
    got = SC.model_rowdot(SC.model_split_gemm(x, Wt, None, bias, True), w3, b3)
    assert got.shape == (M, 1) and bool(((got.double() - want).abs() <= allowed).all())


@pytest.mark.parametrize("nk", SC.ATTN_NKS)
def test_one_hot_attention_bound_holds_in_the_model_and_catches_a_lost_term(nk):
    """the selected key's weight is exactly 1 = (1, 0, 0) in pieces, so the one-hot probe sees the three products with the first
    piece of P (V's l, m and h pieces): those mutants must violate it.  The products with P's second and third piece are probed
    by the dense weights of the cancelling-V case below."""
    Q, K, V = SC.attn_case("onehot", nk)
    jstar = SC.onehot_keys(nk)
    _, _, S, _ = SC.attn_reference("onehot", nk)
    top = S.gather(1, jstar.view(1, 1, -1).expand(S.shape[0], 1, -1))[:, 0]                # (b, nq)
    rest = S.clone()
    rest.scatter_(1, jstar.view(1, 1, -1).expand(S.shape[0], 1, -1), -1e30)
    assert float((top - rest.max(1).values).min()) >= SC.ONEHOT_LEAD
    seen = set(jstar.tolist())
    tiles = (nk + 31) // 32
    assert set(range(min(64, nk))) <= seen and set(range(32 * (tiles - 1), nk)) <= seen
    for z in range(1, 4):
        cut = 32 * (z * tiles // 4)
        assert {j for j in (cut - 1, cut) if 0 <= j < nk} <= seen
    vs = torch.stack([V[i, jstar] for i in range(V.shape[0])]).double()
    for nsplit in (1, 4):
        bound = SC.onehot_bound(V, jstar, nsplit)
        assert bool(((SC.model_split_attention(Q, K, V).double() - vs).abs() <= bound).all())
        for drop in (0, 3, 5):
            assert bool(((SC.model_split_attention(Q, K, V, drop_pv=drop).double() - vs).abs() > bound).any()), drop


@pytest.mark.parametrize("nk", SC.ATTN_NKS)
def test_cancelling_v_attention_the_model_stays_within_the_fp32_form_and_catches_a_lost_term(nk):
    Q, K, V = SC.attn_case("cancel_v", nk)
    fp32 = SC.units_attn(SC.model_fp32_attention(Q, K, V), "cancel_v", nk)
    got = SC.units_attn(SC.model_split_attention(Q, K, V), "cancel_v", nk)
    assert got <= SC.ATTN_SPLIT_OVER_FP32 * fp32 and fp32 <= SC.attn_apriori_units(nk), (got, fp32)
    for drop in range(6):
        bad = SC.units_attn(SC.model_split_attention(Q, K, V, drop_pv=drop), "cancel_v", nk)
        assert bad > SC.ATTN_SPLIT_OVER_FP32 * fp32, (drop, bad, fp32)


@pytest.mark.parametrize("nk", SC.ATTN_NKS)
def test_cancelling_s_attention_bound_holds_in_the_model_and_catches_a_lost_term(nk):
    Q, K, V = SC.attn_case("cancel_s", nk)
    O, D, S, qk = SC.attn_reference("cancel_s", nk)
    assert 2.0 ** 11 <= qk <= 2.0 ** 13 and float(S.abs().max()) < 8.0
    allowed = (2 * SC.cancel_s_delta(qk) + SC.attn_apriori_units(nk) * SC.U) * D
    assert bool(((SC.model_split_attention(Q, K, V).double() - O).abs() <= allowed).all())
    # (the 2^-16 terms of S are inside 25 units of sum |q||k|, and a lost K_h Q_m cancels like the logit itself, Q being equal
    #  within a channel pair: the GEMM's sparse rows probe those orders)
    for drop in (3, 5):
        assert bool(((SC.model_split_attention(Q, K, V, drop_s=drop).double() - O).abs() > allowed).any()), drop


@pytest.mark.parametrize("nk", SC.ATTN_NKS)
def test_spread_v_attention_the_model_stays_within_the_fp32_form(nk):
    Q, K, V = SC.attn_case("v_spread", nk)
    fp32 = SC.units_attn(SC.model_fp32_attention(Q, K, V), "v_spread", nk)
    got = SC.units_attn(SC.model_split_attention(Q, K, V), "v_spread", nk)
    assert got <= SC.ATTN_SPLIT_OVER_FP32 * fp32 and fp32 <= SC.attn_apriori_units(nk), (got, fp32)
