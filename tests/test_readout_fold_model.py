"""The folded read-out on the CPU (tests/readout_fold_cases.py): the identity the fold rests on, in exact arithmetic and in a model
of the kernels' fp32 arithmetic; mutants that lose a neighbour or a level; the bound the GPU test asserts; the new entry points'
argument checks.  No GPU."""
import ctypes as C

import pytest
import torch

import readout_fold_cases as RF
import split_cases as SC


@pytest.mark.parametrize("nfold", (1, 2))
def test_exact_operands_fold_bit_for_bit(nfold):
    """small integers, weights 0.5 / 0.25 / 0.25: the folded model, the unfolded model and float64 agree in every bit"""
    F, W, bias, w, idx = RF.exact_case()
    want = RF.unfolded_reference(F, W, bias, w, idx)
    unfolded = SC.model_fma_chain(RF.model_read_out(F, w, idx), W) + bias
    folded = RF.model_folded(F, W, bias, w, idx, nfold)
    assert torch.equal(unfolded.double(), want)
    assert torch.equal(folded.double(), want)
    assert torch.equal(folded, unfolded)
    assert float(want.abs().max()) < 2.0 ** 22 and bool((want * 4 == (want * 4).round()).all())      # quarter integers, far inside fp32


@pytest.mark.parametrize("nfold", (1, 2))
def test_a_lost_neighbour_or_level_is_seen(nfold):
    """the mutants the exact case must catch: one neighbour of the folded levels left out, one folded level left out"""
    F, W, bias, w, idx = RF.exact_case()
    want = RF.unfolded_reference(F, W, bias, w, idx)
    for i in range(3):
        got = RF.model_folded(F, W, bias, w, idx, nfold, drop_neighbour=i)
        assert float((got.double() != want).double().mean()) > 0.9, i
    for m in range(4 - nfold, 4):
        got = RF.model_folded(F, W, bias, w, idx, nfold, drop_level=m)
        assert float((got.double() != want).double().mean()) > 0.9, m


@pytest.mark.parametrize("nfold", (1, 2))
def test_the_model_holds_the_bound_and_the_route_margin(nfold):
    """Gaussian operands: the fp32 model of the folded route stays inside gather_bound (in units of the extended magnitude) and
    within ROUTE_OVER_TODAY of the fp32 model of today's route -- the two assertions of tests/test_gpu_readout_fold.py"""
    F, W, bias, w, idx = RF.route_case()
    want = RF.unfolded_reference(F, W, bias, w, idx)
    today = SC.model_fma_chain(RF.model_read_out(F, w, idx), W) + bias
    folded = RF.model_folded(F, W, bias, w, idx, nfold)
    e_today, e_folded = float((today.double() - want).abs().max()), float((folded.double() - want).abs().max())
    print("readout-fold model\tnfold=%d\ttoday=%.3e\tfolded=%.3e\tratio=%.3f" % (nfold, e_today, e_folded, e_folded / e_today))
    assert e_folded <= RF.ROUTE_OVER_TODAY * e_today
    k0 = RF.K0[nfold]
    x = RF.model_read_out(F, w, idx, 4 - nfold)
    ref, mag = RF.gather_reference(x, W[:k0], bias, F[4 - nfold:], [W[RF.COL[m]:RF.COL[m + 1]] for m in range(4 - nfold, 4)],
                                   w[4 - nfold:], idx[4 - nfold:])
    units = RF.gather_units(folded, ref, mag, False)
    print("readout-fold model\tnfold=%d\tunits=%.3f\tbound=%d" % (nfold, units, RF.gather_bound(k0, RF.LEVEL_C[4 - nfold:])))
    assert units <= RF.gather_bound(k0, RF.LEVEL_C[4 - nfold:])


def test_the_bound_counts_operations():
    assert RF.gather_bound(16, (64,)) == max(6 * 16 + 2, 64) + 3 + 1
    assert RF.gather_bound(224, (32, 64)) == 6 * 224 + 2 + 6 + 1
    assert RF.gather_bound(16, (128, 256)) == 256 + 6 + 1
    assert RF.gather_bound(96, (128, 256), g_units=(6 * 128 + 1, 6 * 256 + 1)) == 6 * 256 + 1 + 6 + 1


def test_new_entry_points_check_their_arguments_without_touching_the_gpu(dcl):
    """a bad argument is DCL_EINVAL before any device call (pointers here are never dereferenced)"""
    lib = dcl._native.lib()
    p = C.c_void_p(4096)
    G, ldg = (C.c_void_p * 2)(4096, 4096), (C.c_int64 * 2)(128, 128)
    good = dict(x=p, ldx=16, planes=p, bias=None, nfold=1, fw=p, fi=p, level_stride=3 * 256, G=G, ldg=ldg, y=p, ldy=128, M=256, N=128,
                K=16, relu=0)
    for change in (dict(nfold=0), dict(nfold=3), dict(fw=None), dict(fi=None), dict(G=None), dict(ldg=None), dict(level_stride=3 * 256 - 1),
                   dict(ldg=(C.c_int64 * 2)(127, 128)), dict(G=(C.c_void_p * 2)(None, 4096)), dict(K=8), dict(ldx=15), dict(ldy=127)):
        a = dict(good, **change)
        rc = lib.dcl_linear_split_gather_fwd(a["x"], a["ldx"], a["planes"], a["bias"], a["nfold"], a["fw"], a["fi"], a["level_stride"],
                                             a["G"], a["ldg"], a["y"], a["ldy"], a["M"], a["N"], a["K"], a["relu"], None)
        assert rc == -1 and b"invalid argument" in lib.dcl_last_error(), change
    chan, counts, ve = (C.c_int32 * 9)(*dcl.ops.BACKBONE_CHANNELS), (C.c_int32 * 8)(), (C.c_float * 4)(1, 2, 3, 4)
    feats = (C.c_void_p * 4)(4096, 4096, 4096, 4096)
    for nfold, ld, tmp_bytes in ((0, 224, 1 << 20), (3, 224, 1 << 20), (1, 224, 16), (1, 100, 1 << 20), (2, 92, 1 << 20), (1, 226, 1 << 20)):
        rc = lib.dcl_point_features_fold(100, p, 2, 64, 1000, p, counts, chan, feats, ve, -0.192, nfold, p, ld, p, p, p, tmp_bytes, None)
        assert rc == -1 and b"invalid argument" in lib.dcl_last_error(), (nfold, ld, tmp_bytes)
