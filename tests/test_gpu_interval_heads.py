"""The hand-offs of the split-bf16 kernels' barrier intervals (csrc/linear_split.hip: k_linear_split<EPI>; csrc/dense.hip:
k_cross_attn_split) at the smallest shapes at which they can go wrong.

GEMM: with the store, pooling and row-dot epilogues a wave reads and splits its own x rows of chunk c + 1 under the MFMAs of
chunk c, behind its own counted wait and in front of the barrier, and the next chunk's DMA pieces are issued behind MFMA blocks;
the V-piece epilogue reads, fetches and splits behind the barrier.  K = 16 is one chunk (no prefetch), 32 two, 48 an odd count
(stage parity), 64 four; M = 1, 255, 256, 257, 513 are clamped source rows and a partial second / third row tile; N = 96, 128,
160 a ragged, a whole and a second column tile.  Attention: tile t + 1 of the K / V pieces is fetched into the other buffers
under the second interval of tile t, the two wave groups half a tile apart; nk = 32 is one tile (prologue only), 40 two tiles
with a ragged one, 96 and 160 odd tile counts, 160 with the keys split in two (tile ranges of 2 and 3); nq = 32 is one live
wave, 256 a whole workgroup, 300 a ragged second one.

Operands, float64 references and bounds are those of tests/split_cases.py; every bound is the one tests/test_gpu_split_arithmetic.py
holds the same kernel to.  Every test prints its figures (pytest -s) before it asserts."""
import pytest
import torch

import split_cases as SC
import test_gpu_split_arithmetic as TS

pytestmark = pytest.mark.gpu
attn = TS.attn                                    # the fixture that forces the 8-wave split kernel on a call of any size
report = TS.report

KS = (16, 32, 48, 64)
MS = (1, 255, 256, 257, 513)
NS = (96, 128, 160)
M_FULL = max(MS)


@pytest.mark.parametrize("with_bias,relu", [(False, False), (True, True)])
@pytest.mark.parametrize("K", KS)
def test_store_epilogue_over_chunk_counts_and_ragged_tiles(dcl, K, with_bias, relu):
    """EPI 0.  Per (K, N) one Gaussian operand set of 513 rows (SC.dense_case); the launches with fewer rows take its first M rows.
    A row's accumulators depend on that row of x and on the weights alone, so the M-row launch must return the bits of the first
    M rows of the 513-row launch, and the 513-row launch must hold the bound of test_dense_rows_against_the_fp32_chain: units
    <= 1.5 x the units of the CPU fp32 FMA chain on the same operands (with the bias and the ReLU where the launch has them)."""
    for N in NS:
        x, Wt, bias = SC.dense_case("gaussian", K, N, M_FULL)
        bias = bias if with_bias else None
        xd, sw, bd = x.cuda(), dcl.ops.SplitWeight(Wt.cuda()), None if bias is None else bias.cuda()
        full = dcl.ops.linear_split(xd, sw, bd, relu).cpu()
        chain = SC.units(SC.model_fma_chain(x, Wt, bias, relu), x, Wt, bias, relu)
        split = SC.units(full, x, Wt, bias, relu)
        report("interval-heads store K=%d N=%d bias=%d" % (K, N, with_bias), split=split, chain=chain)
        assert bool(torch.isfinite(full).all())
        assert split <= SC.SPLIT_OVER_CHAIN * chain, (K, N, split, chain)
        for M in MS[:-1]:
            got = dcl.ops.linear_split(xd[:M], sw, bd, relu).cpu()
            assert got.shape == (M, N) and torch.equal(got, full[:M]), (K, M, N)


@pytest.mark.parametrize("rpc", [128, 256])
@pytest.mark.parametrize("K", KS)
def test_pooling_epilogue_over_chunk_counts(dcl, K, rpc):
    """EPI 1 (row weights staged behind the ring): 768 rows = three workgroup tiles, crops of 128 and of 256 rows with the weights
    at a stride of 500, N = 200.  The bound of test_pooling_epilogue_of_the_split_core."""
    M, N = 768, 200
    x, Wt, bias, roww = SC.pool_case(M, K, N, rpc)
    want, mag = SC.pool_reference(x, Wt, bias, SC.pool_row_weights(roww, M, rpc))
    sw = dcl.ops.SplitWeight(Wt.cuda())
    got = dcl.ops.linear_split_pool(x.cuda(), sw, bias.cuda(), roww.cuda(), True, rows_per_crop=rpc, w_stride=SC.POOL_W_STRIDE).cpu()
    e = (got.double() - want).abs() / (SC.U * mag)
    allowed = SC.epilogue_bound(SC.SPLIT_OVER_CHAIN * SC.pool_chain_units(M, K, N, rpc), SC.POOL_FMAS)
    report("interval-heads pool K=%d crops=%d" % (K, rpc), split=float(e.max()), allowed=allowed)
    assert got.shape == want.shape and bool(torch.isfinite(got).all())
    assert float(e.max()) <= allowed


@pytest.mark.parametrize("K", KS)
def test_row_dot_epilogue_over_chunk_counts(dcl, K):
    """EPI 2 with N = 128, 513 rows (and the first 257, 1 of them: the same bits).  The bound of
    test_row_dot_epilogue_of_the_split_core."""
    M, N = M_FULL, 128
    g = SC._gen("interval-heads rowdot", K)
    x, Wt, bias = torch.randn(M, K, generator=g), torch.randn(K, N, generator=g) * 0.1, torch.randn(N, generator=g)
    w3, b3 = torch.randn(N, 1, generator=g), torch.randn(1, generator=g)
    want, mag = SC.rowdot_reference(x, Wt, bias, w3, b3)
    xd, bd, b3d = x.cuda(), bias.cuda(), b3.cuda()
    sw, w3d = dcl.ops.SplitWeight(Wt.cuda()), dcl.ops.pad_linear_weight(w3.cuda())
    got = dcl.ops.linear_split_rowdot(xd, sw, bd, w3d, b3d).cpu()
    chain = SC.units(SC.model_fma_chain(x, Wt, bias), x, Wt, bias)
    e = (got.double() - want).abs() / (SC.U * mag)
    allowed = SC.epilogue_bound(SC.SPLIT_OVER_CHAIN * chain, SC.ROWDOT_FMAS)
    report("interval-heads rowdot K=%d" % K, split=float(e.max()), allowed=allowed)
    assert got.shape == (M, 1) and bool(torch.isfinite(got).all())
    assert float(e.max()) <= allowed
    for m in (257, 1):
        assert torch.equal(dcl.ops.linear_split_rowdot(xd[:m], sw, bd, w3d, b3d).cpu(), got[:m]), (K, m)


@pytest.mark.parametrize("N", [64, 320])
@pytest.mark.parametrize("K", KS)
def test_v_pieces_epilogue_over_chunk_counts(dcl, K, N):
    """EPI 3 at M = 512, two crops of 256 keys: h + m + l read back from the pieces is, bit for bit, the fp32 output of the store
    epilogue on the same operands (as in test_v_pieces_epilogue_without_relu_keeps_both_signs), which holds the GEMM's bound."""
    M, rpc = 512, 256
    x, Wt, bias = SC.dense_case("gaussian", K, N, M)
    xd, sw, bd = x.cuda(), dcl.ops.SplitWeight(Wt.cuda()), bias.cuda()
    V = dcl.ops.linear_split(xd, sw, bd, False).cpu()
    nht = M // 16
    planes = torch.zeros(nht * 30720, dtype=torch.uint8, device="cuda")
    dcl.ops.linear_split_vpieces(xd, sw, bd, planes, rpc, relu=False)
    pieces = planes.view(nht, 3, 320, 32)[:, :, :N].cpu().contiguous().view(torch.bfloat16).view(nht, 3, N, 2, 8).double().sum(1)
    c, hs, e = torch.arange(N).view(-1, 1, 1), torch.arange(2).view(1, -1, 1), torch.arange(8).view(1, 1, -1)
    key = (e & 3) + 8 * (e >> 2) + 4 * (hs ^ ((c >> 3) & 1))
    back = torch.zeros(nht, 16, N, dtype=torch.float64)
    back[:, key, c.expand(N, 2, 8)] = pieces
    chain = SC.units(SC.model_fma_chain(x, Wt, bias), x, Wt, bias)
    split = SC.units(V, x, Wt, bias)
    report("interval-heads vpieces K=%d N=%d" % (K, N), split=split, chain=chain)
    assert bool(torch.isfinite(V).all())
    assert torch.equal(back.view(M, N), V.double())
    assert split <= SC.SPLIT_OVER_CHAIN * chain


@pytest.mark.parametrize("split", [1, 2])
@pytest.mark.parametrize("nk", [32, 40, 96, 160])
def test_attention_over_tile_counts(attn, nk, split):
    """b = 2; the operands are SC.attn_case("cancel_v", nk) (300 queries) and its first 256 and 32 queries -- a query's output
    depends on that query, K and V alone, so the float64 reference of the 300 serves all three.  Bounds of
    test_attention_adversarial_v_beside_the_fp32_form: in units of 2^-24 sum_j p_j |v_j|, the split form <= 1.5 x the fp32 form
    on the same operands, both <= the a-priori nk + 64."""
    name = "cancel_v"
    Q, K, V = SC.attn_case(name, nk)
    O, D, _, _ = SC.attn_reference(name, nk)
    for nq in (32, 256, 300):
        u = {}
        for bf16 in (1, 0):
            got = attn(Q[:, :nq].contiguous(), K, V, bf16, split)
            assert got.shape == (SC.ATTN_B, nq, 320) and bool(torch.isfinite(got).all()), (nq, bf16)
            u[bf16] = float(((got.double() - O[:, :nq]).abs() / (D[:, :nq] * SC.U)).max())
        report("interval-heads attention nq=%d nk=%d split=%d" % (nq, nk, split), split=u[1], fp32=u[0], apriori=SC.attn_apriori_units(nk))
        assert u[1] <= SC.ATTN_SPLIT_OVER_FP32 * u[0], (nq, u)
        assert u[1] <= SC.attn_apriori_units(nk) and u[0] <= SC.attn_apriori_units(nk), (nq, u)
