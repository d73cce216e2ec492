"""ops.linear_wgrad_split (csrc/linear_wgrad_split.hip) on the GPU: the contract of ops.linear_wgrad (any shape, pitch and
alignment, the same bits call after call, nothing written beside the output block, inside guard bands), the split-bf16
arithmetic on the operands of tests/split_cases.py in the orientation a = x.t().contiguous(), b = Wt (so dW = x Wt and that
file's references, magnitudes and yardsticks apply unchanged), its range semantics, and the switches that lead to it
(PointLinearFn / RefinerShareFn wgrad="split", Network(train_wgrad="split")).  Every test prints its figures (pytest -s) before
it asserts; ops.linear_wgrad runs beside the new kernel wherever a yardstick is involved, so the yardstick itself is checked."""
import importlib
import math

import pytest
import torch

import guard_arena as GA
import split_cases as SC
import step_replay as SR
import test_gpu_linear_wgrad as TW

pytestmark = pytest.mark.gpu

R, U, POISON = TW.R, TW.U, TW.POISON
CASES = list(TW.WGRAD_CASES) + [(M, 33, 65) for M in (0, 1, 15, 16, 17, 511, 512, 513)]


def report(case, **figures):
    print("wgrad-split\t%s\t%s" % (case, "\t".join("%s=%s" % (k, ("%.3f" % v) if isinstance(v, float) else v)
                                                    for k, v in figures.items())))


def bits(t):
    return t.contiguous().view(torch.int32)


def split_wgrad(dcl, x, Wt):
    """dW = x Wt through the new kernel: the reduction index on the rows of both operands"""
    return dcl.ops.linear_wgrad_split(x.t().contiguous().cuda(), Wt.cuda()).cpu()


def fp32_wgrad(dcl, x, Wt):
    return dcl.ops.linear_wgrad(x.t().contiguous().cuda(), Wt.cuda()).cpu()


def apriori(dcl, M, mag):
    """the header's a-priori bound: (6 DCL_WGRAD_ROWS + splits + 32) 2^-24 sum_j |a_jp| |b_jq|"""
    units = dcl.ops.linear_wgrad_split_units(M)
    assert units == 6 * R + max(1, -(-M // R)) + 32
    return units * U * mag


# ------------------------------------------------------------------------------------------- 1, 3: shapes, pitches, integers
@pytest.fixture(scope="module")
def runs():
    """every case and operand kind once: (dense result, a second dense launch, the strided / unaligned run, its poisoned frame,
    float64 result, float64 magnitude sum, the fp32 kernel's result)"""
    dcl = importlib.import_module("dcl-net_amd")
    out = {}
    for i, (M, P, Q) in enumerate(CASES):
        for kind in ("random", "integers"):
            a, b = TW._operands(M, P, Q, kind, 300 + i)
            dense = dcl.ops.linear_wgrad_split(a, b)
            again = dcl.ops.linear_wgrad_split(a, b)
            _, ab = TW._block(a, 2, 3)
            _, bb = TW._block(b, 1, 2)
            assert M == 0 or ab.data_ptr() % 16 != 0 or bb.data_ptr() % 16 != 0
            frame, ob = TW._block(torch.full((P, Q), POISON, device="cuda"), 3, 4)
            got = dcl.ops.linear_wgrad_split(ab, bb, out=ob)
            assert got.data_ptr() == ob.data_ptr()
            fp32 = dcl.ops.linear_wgrad(a, b)
            want = a.double().t() @ b.double()
            mag = a.double().abs().t() @ b.double().abs()
            out[(M, P, Q, kind)] = tuple(t.cpu() for t in (dense, again, ob, frame, want, mag, fp32))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("case", CASES)
def test_within_the_a_priori_bound_of_float64(dcl, runs, case):
    M, P, Q = case
    dense, _, _, _, want, mag, _ = runs[case + ("random",)]
    bound = apriori(dcl, M, mag)
    err = (dense.double() - want).abs()
    report("apriori %s" % (case,), worst_over_bound=float((err / bound.clamp_min(1e-300)).max()),
           units=float((err / (U * mag).clamp_min(1e-300)).max()))
    assert bool(torch.isfinite(dense).all())
    assert bool((err <= bound).all())
    if M == 0:
        assert bool((dense == 0).all())


@pytest.mark.parametrize("kind", ["random", "integers"])
@pytest.mark.parametrize("case", CASES)
def test_same_bits_again_and_for_any_pitch_and_alignment(runs, case, kind):
    M, P, Q = case
    dense, again, block, frame, _, _, _ = runs[case + (kind,)]
    assert torch.equal(bits(dense), bits(again))
    assert torch.equal(bits(dense), bits(block))
    outside = torch.ones_like(frame, dtype=torch.bool)
    outside[:, 3:3 + Q] = False
    assert bool((frame[outside] == POISON).all())                  # nothing beside the column block was written


@pytest.mark.parametrize("case", CASES)
def test_exact_on_small_integers_and_the_fp32_kernels_bits(runs, case):
    """operands in [-4, 4]: one bf16 piece each, every product and every partial sum representable"""
    dense, _, block, _, want, _, fp32 = runs[case + ("integers",)]
    assert float(want.abs().max()) < 2 ** 24
    assert torch.equal(dense.double(), want)
    assert torch.equal(block.double(), want)
    assert torch.equal(bits(dense), bits(fp32))


# ------------------------------------------------------------------------------------------- 2: guard bands
def test_inside_poisoned_guard_bands(dcl):
    """(M, P, Q) = (257, 48, 72), dense and as a column block of a wider gradient: no band damaged, no input written, the same
    bits plain and under both poisons; then the NaN pass alone"""
    g = torch.Generator().manual_seed(11)
    a, b = torch.randn(257, 48, generator=g).cuda(), torch.randn(257, 72, generator=g).cuda()
    wide = torch.randn(48, 72 + 5, generator=g).cuda()
    mods = GA.allocating_modules(dcl)

    def fn(a, b, wide):
        dcl.ops.linear_wgrad_split(a, b, out=wide[:, 3:75])
        return dcl.ops.linear_wgrad_split(a, b)
    GA.guarded(fn, [a, b, wide], inplace=(2,), modules=mods)
    GA.poison_pass(fn, [a, b, wide], "nan", modules=mods)


# ------------------------------------------------------------------------------------------- 4: all three pieces arrive
def test_all_three_pieces_of_an_operand_arrive(dcl):
    """a has ONE non-zero per column, with a full 24-bit significand (three non-zero pieces); b holds signed powers of two (one
    piece).  Every dW[p][q] is then one fp32 product that is exact, and every partial sum on the way (l.h, then + m.h, then
    + h.h; the other products are zero) is a prefix of its bits: the result equals the fp32 product bit for bit.  A kernel that
    loses m or l of a, or misplaces a row in the transposed read, cannot."""
    M, P, Q = 530, 140, 45
    g = torch.Generator().manual_seed(5)
    sig = (torch.randint(0, 2 ** 22, (P,), generator=g) * 2 + 1 + 2 ** 23).double()          # odd, 24 bits
    val = sig * torch.exp2(torch.randint(-30, 10, (P,), generator=g).double()) * (torch.randint(0, 2, (P,), generator=g) * 2 - 1)
    a = torch.zeros(M, P)
    rows = (torch.arange(P) * 37) % M
    a[rows, torch.arange(P)] = val.float()
    assert bool((a[rows, torch.arange(P)].double() == val).all())
    b = torch.exp2(torch.randint(-10, 11, (M, Q), generator=g).float()) * (torch.randint(0, 2, (M, Q), generator=g) * 2 - 1)
    for swap in (False, True):                                     # the three pieces of b as well
        x, y = (b, a) if swap else (a, b)
        want = (x.double().t() @ y.double())
        assert torch.equal(want.float().double(), want)
        got = dcl.ops.linear_wgrad_split(x.cuda(), y.cuda()).cpu()
        report("three pieces swap=%d" % swap, differing=int((bits(got) != bits(want.float())).sum()))
        assert torch.equal(bits(got), bits(want.float()))


# ------------------------------------------------------------------------------------------- 5: sparse columns
@pytest.mark.parametrize("shape", SC.SPARSE_SHAPES)
def test_sparse_columns_every_piece_product_is_there(dcl, shape):
    """column i of a (row i of SC.sparse_case's x) has s = 1, 2, 3 non-zeros: |err| <= (6 s + 1) units per output, as
    SC.sparse_bound_split derives; the fp32 kernel holds s + 1"""
    x, Wt, _, s = SC.sparse_case(*shape)
    got, ref = split_wgrad(dcl, x, Wt), fp32_wgrad(dcl, x, Wt)
    um, um32 = SC.unit_map(got, x, Wt), SC.unit_map(ref, x, Wt)
    for k in (1, 2, 3):
        report("sparse %s s=%d" % (shape, k), split=float(um[s == k].max()), fp32=float(um32[s == k].max()),
               allowed_split=SC.sparse_bound_split(k, False), allowed_fp32=SC.sparse_bound_fp32(k, False))
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(ref).all())
    worst = um / SC.sparse_bound_split(s, False).double().view(-1, 1)
    assert float(worst.max()) <= 1.0, "split kernel at %.2f of its bound" % float(worst.max())
    worst32 = um32 / SC.sparse_bound_fp32(s, False).double().view(-1, 1)
    assert float(worst32.max()) <= 1.0, "fp32 kernel at %.2f of its bound" % float(worst32.max())


# ------------------------------------------------------------------------------------------- 6: dense adversarial, one split
@pytest.mark.parametrize("K,N", SC.DENSE_KN)
@pytest.mark.parametrize("name", SC.DENSE_SETS)
def test_dense_one_split_against_the_fp32_chain(dcl, name, K, N):
    """units(split kernel) <= 1.5 units(CPU fp32 FMA chain), units(ops.linear_wgrad) <= 1.05 units(chain); P = 517 columns,
    K <= 512 rows: one split"""
    x, Wt, _ = SC.dense_case(name, K, N)
    assert x.shape[0] == 517 and K <= R
    chain = SC.chain_units(name, K, N)
    split, fp32 = SC.units(split_wgrad(dcl, x, Wt), x, Wt), SC.units(fp32_wgrad(dcl, x, Wt), x, Wt)
    report("dense %s K=%d N=%d" % (name, K, N), split=split, fp32=fp32, chain=chain, split_over_chain=split / chain,
           fp32_over_chain=fp32 / chain)
    assert split <= SC.SPLIT_OVER_CHAIN * chain, (name, K, N, split, chain)
    assert fp32 <= SC.FP32_OVER_CHAIN * chain, (name, K, N, fp32, chain)


# ------------------------------------------------------------------------------------------- 7: dense adversarial, several splits
SEVERAL = [(1030, 70, 96), (1536, 33, 40)]          # (reduction length, M, N): three splits each, the first with a ragged last chunk


def chain_of_splits_units(name, K, M, N):
    """the yardstick over several splits: the CPU fp32 FMA chain per split of DCL_WGRAD_ROWS rows, then one rounded fp32 add per
    split, ascending"""
    x, Wt, _ = SC.dense_case(name, K, N, M)
    acc = None
    for lo in range(0, K, R):
        part = SC.model_fma_chain(x[:, lo:lo + R].contiguous(), Wt[lo:lo + R].contiguous())
        acc = part if acc is None else acc + part
    return SC.units(acc, x, Wt)


@pytest.mark.parametrize("K,M,N", SEVERAL)
@pytest.mark.parametrize("name", SC.DENSE_SETS)
def test_dense_several_splits_against_the_chain_of_splits(dcl, name, K, M, N):
    x, Wt, _ = SC.dense_case(name, K, N, M)
    assert dcl.ops.linear_wgrad_splits(K) == -(-K // R) >= 3
    chain = chain_of_splits_units(name, K, M, N)
    split, fp32 = SC.units(split_wgrad(dcl, x, Wt), x, Wt), SC.units(fp32_wgrad(dcl, x, Wt), x, Wt)
    report("splits %s K=%d M=%d N=%d" % (name, K, M, N), split=split, fp32=fp32, chain=chain, split_over_chain=split / chain,
           fp32_over_chain=fp32 / chain)
    assert split <= SC.SPLIT_OVER_CHAIN * chain, (name, K, M, N, split, chain)
    assert fp32 <= SC.FP32_OVER_CHAIN * chain, (name, K, M, N, fp32, chain)


# ------------------------------------------------------------------------------------------- 8 - 10: range and non-finite
@pytest.mark.parametrize("name", SC.RANGE_SETS)
def test_operands_at_the_ends_of_the_exponent_range(dcl, name):
    """'huge' and 'tiny' of SC.range_case with the bounds of tests/test_gpu_split_arithmetic.py: 1.5 x the chain, plus
    SC.tiny_allowance for 'tiny' (third pieces that are bf16 subnormals)"""
    x, Wt = SC.range_case(name)
    M, K, N = SC.RANGE_SHAPE
    chain = SC.chain_units(name, K, N)
    mag, want = SC.magnitude(x, Wt), SC.reference(x, Wt)
    extra = SC.tiny_allowance(Wt) if name == "tiny" else 0.0
    got, ref = split_wgrad(dcl, x, Wt), fp32_wgrad(dcl, x, Wt)
    e, e32 = (got.double() - want).abs(), (ref.double() - want).abs()
    report("range %s" % name, split=float((e / (SC.U * mag)).max()), fp32=float((e32 / (SC.U * mag)).max()), chain=chain,
           split_in_allowance=float((e / (SC.SPLIT_OVER_CHAIN * chain * SC.U * mag + extra)).max()))
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(ref).all())
    assert bool((e <= SC.SPLIT_OVER_CHAIN * chain * SC.U * mag + extra).all())
    assert bool((e32 <= SC.FP32_OVER_CHAIN * chain * SC.U * mag + extra).all())


def test_a_value_whose_first_piece_overflows_gives_nan_for_its_row_only(dcl):
    """bits 0x7F7F8000 in column p of a: dW[p][:] is NaN (the fp32 kernel still computes it); the value one below is fine, and
    every other row has the bits of the launch with the overflowing columns zeroed"""
    x, Wt = SC.range_case("huge")
    M, K, N = SC.RANGE_SHAPE
    edge = torch.tensor([SC.H_OVERFLOWS, SC.H_OVERFLOWS - 1, 0x7F7FFFFF], dtype=torch.int32).view(torch.float32)
    x = x.clone()
    x[10, 3], x[75, 20], x[299, 63] = edge[0], -edge[1], -edge[2]
    zeroed = x.clone()
    zeroed[[10, 299]] = 0.0
    got, clean, ref = split_wgrad(dcl, x, Wt), split_wgrad(dcl, zeroed, Wt), fp32_wgrad(dcl, x, Wt)
    assert bool(torch.isnan(got[[10, 299]]).all())
    assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(got[75]).all())
    others = [i for i in range(M) if i not in (10, 299)]
    assert torch.equal(bits(got[others]), bits(clean[others]))
    assert SC.units(got[75:76], x[75:76], Wt) <= SC.SPLIT_OVER_CHAIN * SC.chain_units("huge", K, N)


# first / middle / last column of a 32-column wave block of the fp32 kernel's 128 x 128 tile, and the ragged last tile
NF_P, NF_Q, NF_M = 300, 200, 70
NF_COLS_A, NF_COLS_B = (64, 80, 95, 299), (64, 80, 95, 199)


@pytest.mark.parametrize("poison", [math.inf, -math.inf, math.nan])
def test_a_non_finite_value_stays_in_its_row_or_column(dcl, poison):
    """one non-finite element in column p of a: dW[p][:] is all NaN, and every other row is bit-equal to the launch with that
    column zeroed, although columns share LDS images and MFMA operands; likewise an element of b and the columns of dW"""
    g = torch.Generator().manual_seed(9)
    a, b = torch.randn(NF_M, NF_P, generator=g), torch.randn(NF_M, NF_Q, generator=g)
    assert NF_COLS_A[-1] == NF_P - 1 and NF_COLS_B[-1] == NF_Q - 1
    ap, az = a.clone(), a.clone()
    for p in NF_COLS_A:
        ap[(7 * p) % NF_M, p] = poison
    az[:, list(NF_COLS_A)] = 0.0
    op = dcl.ops.linear_wgrad_split
    got, clean = op(ap.cuda(), b.cuda()).cpu(), op(az.cuda(), b.cuda()).cpu()
    keep = [i for i in range(NF_P) if i not in NF_COLS_A]
    assert bool(torch.isnan(got[list(NF_COLS_A)]).all()), "a poisoned column of a must make its row of dW NaN throughout"
    assert torch.equal(bits(got[keep]), bits(clean[keep])), "rows beside a poisoned row changed"
    bp, bz = b.clone(), b.clone()
    for q in NF_COLS_B:
        bp[(5 * q) % NF_M, q] = poison
    bz[:, list(NF_COLS_B)] = 0.0
    got, clean = op(a.cuda(), bp.cuda()).cpu(), op(a.cuda(), bz.cuda()).cpu()
    keep = [i for i in range(NF_Q) if i not in NF_COLS_B]
    assert bool(torch.isnan(got[:, list(NF_COLS_B)]).all()), "a poisoned column of b must make its column of dW NaN throughout"
    assert torch.equal(bits(got[:, keep]), bits(clean[:, keep])), "columns beside a poisoned column changed"


# ------------------------------------------------------------------------------------------- 11: autograd
def _within_apriori(dcl, dW, dz, x, what):
    dz, x = dz.double().cpu(), x.double().cpu()
    want, mag = dz.t() @ x, dz.abs().t() @ x.abs()
    err = (dW.double().cpu().reshape(want.shape) - want).abs()
    bound = apriori(dcl, dz.shape[0], mag)
    report(what, rows=dz.shape[0], worst_over_bound=float((err / bound.clamp_min(1e-300)).max()),
           units=float((err / (U * mag).clamp_min(1e-300)).max()))
    assert bool(torch.isfinite(dW).all())
    assert bool((err <= bound).all()), what


@pytest.mark.parametrize("relu", [False, True])
def test_point_linear_fn_split_against_fp32(dcl, relu):
    """outputs, dx and db bit-identical between the forms (and the four-argument call); dW inside the a-priori bound of
    float64 formed from the same dz and x"""
    M, K, Nw = 600, 96, 64
    g = torch.Generator().manual_seed(21)
    x0 = torch.randn(M, K, generator=g).cuda()
    W0 = (torch.randn(Nw, K, 1, generator=g) * 0.1).cuda()
    b0 = torch.randn(Nw, generator=g).cuda() if relu else None
    go = torch.randn(M, Nw, generator=g).cuda()
    res = {}
    for form in ("four", "fp32", "split"):
        x, W = x0.clone().requires_grad_(True), W0.clone().requires_grad_(True)
        b = None if b0 is None else b0.clone().requires_grad_(True)
        extra = () if form == "four" else (form,)
        y = dcl.autograd.PointLinearFn.apply(x, W, b, relu, *extra)
        y.backward(go)
        res[form] = (y.detach(), x.grad, W.grad, None if b is None else b.grad)
    for form in ("fp32", "split"):
        for i in (0, 1, 3):
            if res["four"][i] is not None:
                assert torch.equal(bits(res[form][i]), bits(res["four"][i])), (form, i)
    assert torch.equal(bits(res["fp32"][2]), bits(res["four"][2]))
    assert tuple(res["split"][2].shape) == tuple(W0.shape)
    y = res["split"][0]
    dz = torch.where(y > 0, go, torch.zeros_like(go)) if relu else go
    _within_apriori(dcl, res["split"][2], dz, x0, "PointLinearFn relu=%d" % relu)
    with pytest.raises(ValueError):
        dcl.autograd.PointLinearFn.apply(x0, W0, b0, relu, "bf16")


def test_refiner_share_fn_split_against_fp32(dcl, monkeypatch):
    """RefinerShareFn: the pooled output, the bias gradients and (through them) every dz are bit-identical between the forms;
    each of the four dW of the split form is inside the a-priori bound of float64 formed from the dz and x the kernel was
    given; with only the feature block of W0 on the split kernel (out=dW0[:, 3:]) the xyz block keeps the fp32 form's bits"""
    b, n = 2, 384
    g = torch.Generator().manual_seed(23)
    xyz, F = (torch.randn(b * n, 3, generator=g) * 0.05).cuda(), torch.randn(b * n, 256, generator=g).cuda()
    conf_w = torch.softmax(torch.rand(b, n, generator=g), dim=1).cuda()
    dims = [259, 512, 512, 1024]
    params0 = []
    for i in range(3):
        params0 += [(torch.randn(dims[i + 1], dims[i], 1, generator=g) * dims[i] ** -0.5).cuda(), (torch.randn(dims[i + 1], generator=g) * 0.1).cuda()]
    go = torch.randn(b, 1024, generator=g).cuda()
    seen = []
    real = dcl.ops.linear_wgrad_split

    def recording(a, bb, out=None):
        res = real(a, bb, out=out)
        seen.append((a.detach().clone(), bb.detach().clone(), res.detach().clone()))
        return res
    monkeypatch.setattr(dcl.ops, "linear_wgrad_split", recording)

    def run(*extra):
        params = [p.clone().requires_grad_(True) for p in params0]
        out = dcl.autograd.RefinerShareFn.apply(xyz, F, conf_w, *params, *extra)
        out.backward(go)
        return out.detach(), [p.grad for p in params]
    out9, g9 = run()
    assert not seen
    out_f, g_f = run("fp32")
    assert not seen
    out_s, g_s = run("split")
    assert len(seen) == 4
    for a, bb, res in seen:
        _within_apriori(dcl, res, a, bb, "RefinerShareFn dW (%d x %d)" % (a.shape[1], bb.shape[1]))
    del seen[:]
    out_m, g_m = run(("fp32", "split", "fp32", "fp32"))
    assert len(seen) == 1 and tuple(seen[0][2].shape) == (512, 256)
    for o in (out_f, out_s, out_m):
        assert torch.equal(bits(o), bits(out9))
    for i in range(6):
        assert torch.equal(bits(g_f[i]), bits(g9[i])), i
    for grads in (g_s, g_m):
        for i in (1, 3, 5):                                        # the bias gradients: every dz is the fp32 form's
            assert torch.equal(bits(grads[i]), bits(g9[i])), i
    assert torch.equal(bits(g_m[0][:, :3]), bits(g9[0][:, :3])), "the xyz block beside out=dW0[:, 3:] changed"
    assert torch.equal(bits(g_m[0][:, 3:]), bits(g_s[0][:, 3:]))
    assert torch.equal(bits(g_m[2]), bits(g9[2])) and torch.equal(bits(g_m[4]), bits(g9[4]))
    with pytest.raises(ValueError):
        dcl.autograd.RefinerShareFn.apply(xyz, F, conf_w, *params0, ("split", "fp32"))


# ------------------------------------------------------------------------------------------- 12: one whole step
class _EveryShape(dict):
    """ops.WGRAD_SPLIT_SHAPES as 'every shape, from no rows on'"""

    def get(self, key, default=None):
        return 0


def _leaves(t):
    """the parameters a tensor was formed from (itself, or the leaves of its graph: torch.cat of four weights)"""
    if t.grad_fn is None:
        return [t]
    out, seen, stack = [], set(), [t.grad_fn]
    while stack:
        fn = stack.pop()
        if fn is None or id(fn) in seen:
            continue
        seen.add(id(fn))
        if hasattr(fn, "variable"):
            out.append(fn.variable)
        stack.extend(f for f, _ in fn.next_functions)
    return out


def test_one_whole_step_with_every_wide_layer_on_the_split_kernel(dcl, monkeypatch):
    K = dcl.DCL_Net.TRAIN_KERNELS
    _, (base,) = SR.run_steps(dcl, 2, 256, steps=1, switches=dict(K))
    monkeypatch.setattr(dcl.ops, "WGRAD_SPLIT_SHAPES", _EveryShape())
    rec = SR.StepRecorder(SR.function_classes(dcl.autograd), monkeypatch, SR.MUTATED)
    net, (step,) = SR.run_steps(dcl, 2, 256, steps=1, switches=dict(K, train_wgrad="split"), rec=rec)
    rec.active = False
    assert SR.same_bits(step["loss"], base["loss"])
    assert set(step["pred"]) == set(base["pred"])
    for k in base["pred"]:
        assert SR.same_bits(step["pred"][k], base["pred"][k]), k
    calls = [c for c in rec.calls if c.name == "PointLinearFn"]
    assert calls and all(len(c.inputs) == 5 and c.inputs[4] == "split" for c in calls)
    touched = set()
    for c in calls:
        assert c.grads_in is not None and len(c.grads_out) == 5 and c.grads_out[4] is None
        x, relu = c.inputs[0], c.inputs[3]
        dz = c.grads_in[0]
        if relu:
            dz = torch.where(c.outputs[0] > 0, dz, torch.zeros_like(dz))
        _within_apriori(dcl, c.grads_out[1], dz, x, "step call %d %s" % (c.index, tuple(c.inputs[1].shape)))
        touched |= {id(p) for p in _leaves(c.args[1])}
    names = {id(p): k for k, p in net.named_parameters()}
    assert touched and touched <= set(names)
    differing = 0
    for k, p in net.named_parameters():
        got, want = step["grads"][k], base["grads"][k]
        assert (got is None) == (want is None), k
        if got is None:
            continue
        if id(p) in touched:
            differing += int(not SR.same_bits(got, want))
            assert bool(torch.isfinite(got).all()), k
        else:
            assert SR.same_bits(got, want), "gradient of %s changed although no split weight gradient feeds it" % k
    report("step", point_linear_calls=len(calls), weights_on_the_split_kernel=len(touched), with_other_bits=differing)
    assert differing > 0                                           # the switch did reach the kernel


def test_refiner_switch_goes_by_the_shape_table(dcl, monkeypatch):
    """Refiner(train_mlp="kernels", train_wgrad="split"): with a table that names only W1's shape, RefinerShareFn gets the
    forms (fp32, fp32, split, fp32); the outputs and every gradient but W1's keep the fp32 form's bits, W1's is close to them.  With
    no shape in the table the call keeps today's nine arguments."""
    import test_gpu_refiner_train as TR
    b, n = 2, 128
    x, conf, labels = TR._inputs(b, n, n)
    seen = []
    real = dcl.autograd.RefinerShareFn.apply
    monkeypatch.setattr(dcl.autograd.RefinerShareFn, "apply", staticmethod(lambda *a: seen.append(a[9:]) or real(*a)))
    res = {}
    for name, table in (("fp32", None), ("empty", {}), ("w1", {(512, 512): b * n})):
        if table is not None:
            monkeypatch.setattr(dcl.ops, "WGRAD_SPLIT_SHAPES", table)
        ref = dcl.refiner.Refiner(train_rotation="device", train_mlp="kernels", train_wgrad="fp32" if table is None else "split")
        ref.load_state_dict(dcl.synth.synth_state_dict(ref, 2))
        res[name] = TR._step(dcl, ref.cuda().train(), x, conf, labels)
    assert seen == [(), (), (("fp32", "fp32", "split", "fp32"),)]
    w1 = "MLP_share.layers.2.weight"
    assert w1 in res["fp32"][1]
    for name in ("empty", "w1"):
        for k, v in res["fp32"][0].items():
            assert torch.equal(bits(res[name][0][k]), bits(v)), (name, k)
        for k, g in res["fp32"][1].items():
            if name == "w1" and k == w1:
                d = float((res[name][1][k] - g).abs().max()) / float(g.abs().max())
                report("refiner switch", w1_rel_diff=d)
                assert 0 < d < 1e-5
            else:
                assert torch.equal(bits(res[name][1][k]), bits(g)), (name, k)
