"""Gradients of the correspondence attention without the attention map (csrc/attention_bwd.hip, ops.cross_attention_backward,
autograd.CrossAttentionFn, Network(train_attention="fused")).

Precision is judged against torch autograd in float64 of test_gpu_ops._attn_ref's expression, next to the materialised
fp32 composition the module path trains with (softmax(bmm) + bmm, torch autograd on the GPU) on the same inputs:
err(g) <= max(2 * err_mat(g), 2e-5 * max(1, |want|max)) per gradient tensor -- twice the materialised path's own error
(two fp32 evaluations in different summation orders can sit on opposite sides of the exact value) or this project's
standing fp32 GEMM tolerance (test_gpu_ops.py), whichever is larger."""
import os

import numpy as np
import pytest
import torch

from conftest import load_golden_data

pytestmark = pytest.mark.gpu

NAMES = ("dQ", "dK", "dV1", "dV2")


def _inputs(b, nq, nk, scale, seed=None):
    g = torch.Generator().manual_seed(nq + nk if seed is None else seed)
    Q = (torch.randn(b, nq, 64, generator=g) * scale).cuda()
    K = torch.randn(b, nk, 64, generator=g).cuda()
    V1 = torch.randn(b, nk, 256, generator=g).cuda()
    V2 = torch.randn(b, nk, 64, generator=g).cuda()
    dO1 = torch.randn(b, nq, 256, generator=g).cuda()
    dO2 = torch.randn(b, nq, 64, generator=g).cuda()
    return Q, K, V1, V2, dO1, dO2


def _spiked():
    """test_gpu_ops.test_cross_attention_forced_rescale's construction: single keys that dominate one query's row"""
    b, nq, nk = 1, 96, 320
    g = torch.Generator().manual_seed(0)
    Q = torch.randn(b, nq, 64, generator=g)
    K = torch.randn(b, nk, 64, generator=g) * 0.1
    K[0, 200] = Q[0, 5] * 3.0
    K[0, 300] = Q[0, 40] * 5.0
    V1, V2 = torch.randn(b, nk, 256, generator=g), torch.randn(b, nk, 64, generator=g)
    dO1, dO2 = torch.randn(b, nq, 256, generator=g), torch.randn(b, nq, 64, generator=g)
    return tuple(t.cuda() for t in (Q, K, V1, V2, dO1, dO2))


def _grads_fp64(Q, K, V1, V2, dO1, dO2):
    import test_gpu_ops as TO
    leaves = [t.double().requires_grad_(True) for t in (Q, K, V1, V2)]
    O = TO._attn_ref(leaves[0], leaves[1], torch.cat([leaves[2], leaves[3]], 2))
    O.backward(torch.cat([dO1, dO2], 2).double())
    return [t.grad for t in leaves]


def _grads_materialised(Q, K, V1, V2, dO1, dO2):
    """what Network._forward_compat runs by default: Aligner's softmax(bmm) map and two bmm with it, fp32, torch autograd"""
    leaves = [t.clone().requires_grad_(True) for t in (Q, K, V1, V2)]
    q, k, v1, v2 = leaves
    A = torch.softmax(torch.bmm(k, q.transpose(1, 2)), dim=1)                   # (b, nk, nq)
    O1 = torch.bmm(v1.transpose(1, 2), A)                                          # (b, 256, nq)
    O2 = torch.bmm(v2.transpose(1, 2), A)
    torch.autograd.backward([O1, O2], [dO1.transpose(1, 2), dO2.transpose(1, 2)])
    return [t.grad for t in leaves]


def _forward(dcl, Q, K, V1, V2):
    b, nq = Q.shape[0], Q.shape[1]
    O1 = torch.empty(b * nq, 256, device="cuda")
    O2 = torch.empty(b * nq, 64, device="cuda")
    dcl.ops.cross_attention(b, Q.reshape(-1, 64), K.reshape(-1, 64), V1.reshape(-1, 256), O1, V2.reshape(-1, 64), O2)
    return O1, O2


def _grads_fused(dcl, Q, K, V1, V2, dO1, dO2):
    b = Q.shape[0]
    O1, O2 = _forward(dcl, Q, K, V1, V2)
    got = dcl.ops.cross_attention_backward(b, Q.reshape(-1, 64), K.reshape(-1, 64), V1.reshape(-1, 256), V2.reshape(-1, 64),
                                           O1, O2, dO1.reshape(-1, 256), None if dO2 is None else dO2.reshape(-1, 64))
    return [g.view(t.shape) for g, t in zip(got, (Q, K, V1, V2))]


SHAPES = [(2, 256, 256, 1.0), (1, 200, 500, 1.0), (3, 64, 96, 6.0), (1, 1000, 132, 0.3), (2, 1024, 1024, 1.0), (1, 1, 1, 1.0),
          (2, 33, 31, 1.0), (1, 12288, 2048, 1.0), "spiked"]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: s if isinstance(s, str) else "%dx%dx%d_s%g" % s)
def test_gradients_match_fp64(dcl, shape):
    ins = _spiked() if shape == "spiked" else _inputs(*shape)
    want = _grads_fp64(*ins)
    mat = _grads_materialised(*ins)
    got = _grads_fused(dcl, *ins)
    failures = []
    for name, w, m, g in zip(NAMES, want, mat, got):
        assert g.shape == w.shape and bool(torch.isfinite(g).all()), name
        err, err_mat = float((g.double() - w).abs().max()), float((m.double() - w).abs().max())
        bound = max(2.0 * err_mat, 2e-5 * max(1.0, float(w.abs().max())))
        print("attention_grad %s %s: err %.3e  err_mat %.3e  err/err_mat %.3f  |want|max %.3e  bound %.3e"
              % (shape, name, err, err_mat, err / err_mat if err_mat > 0 else float("inf"), float(w.abs().max()), bound))
        if not err <= bound:
            failures.append((name, err, bound))
    assert not failures, failures


def test_missing_dO2_is_a_zero_gradient(dcl):
    Q, K, V1, V2, dO1, dO2 = _inputs(2, 100, 70, 1.0, seed=11)
    a = _grads_fused(dcl, Q, K, V1, V2, dO1, None)
    z = _grads_fused(dcl, Q, K, V1, V2, dO1, torch.zeros_like(dO2))
    for name, x, y in zip(NAMES, a, z):
        assert torch.equal(x, y), name
    assert float(a[3].abs().max()) == 0.0                          # dV2 = P dO2


# ---------------------------------------------------------------------------------------------------- row strides
def _block(t2d, left, right, fill):
    """t2d as a column block of a wider buffer: (wide buffer, view of the block)"""
    rows, c = t2d.shape
    wide = torch.full((rows, left + c + right), fill, device="cuda", dtype=torch.float32)
    wide[:, left:left + c] = t2d
    return wide, wide[:, left:left + c]


@pytest.mark.parametrize("b,nq,nk", [(2, 130, 75), (1, 64, 64)])
def test_row_strides(dcl, b, nq, nk):
    Q, K, V1, V2, dO1, dO2 = _inputs(b, nq, nk, 1.0, seed=3)
    O1, O2 = _forward(dcl, Q, K, V1, V2)
    flat = [Q.reshape(-1, 64), K.reshape(-1, 64), V1.reshape(-1, 256), V2.reshape(-1, 64), O1, O2, dO1.reshape(-1, 256),
            dO2.reshape(-1, 64)]
    want = dcl.ops.cross_attention_backward(b, *flat)
    SENT = 12345.0
    pads = [(4, 8), (0, 4), (64, 0), (8, 64), (256, 4), (4, 4), (12, 0), (0, 16)]
    wide_in = [_block(t, l, r, 7.0) for t, (l, r) in zip(flat, pads)]
    outs = [_block(torch.full_like(w, SENT), l, r, SENT) for w, (l, r) in zip(want, [(4, 4), (64, 8), (0, 64), (256, 0)])]
    got = dcl.ops.cross_attention_backward_into(b, *[v for _, v in wide_in], *[v for _, v in outs])
    torch.cuda.synchronize()
    for name, w, g, (wide, view), (l, r) in zip(NAMES, want, got, outs, [(4, 4), (64, 8), (0, 64), (256, 0)]):
        assert torch.equal(g, w), name
        c = w.shape[1]
        assert bool((wide[:, :l] == SENT).all()) and bool((wide[:, l + c:] == SENT).all()), name
    for (wide, view), t, (l, r) in zip(wide_in, flat, pads):           # inputs are read only
        assert torch.equal(view, t)
        assert bool((wide[:, :l] == 7.0).all()) and bool((wide[:, l + t.shape[1]:] == 7.0).all())


# ---------------------------------------------------------------------------------------------------- determinism
@pytest.mark.parametrize("b,nq,nk", [(2, 1024, 1024), (3, 200, 500)])
def test_bit_identical_call_after_call(dcl, b, nq, nk):
    ins = _inputs(b, nq, nk, 1.0, seed=5)
    first = [g.clone() for g in _grads_fused(dcl, *ins)]
    second = [g.clone() for g in _grads_fused(dcl, *ins)]
    junk = [torch.empty(n, device="cuda").normal_() for n in (1000003, 17, 5 * 1024 * 1024 + 1, 4099)]   # move the allocator on
    del junk[1], junk[2]
    keep = torch.full((3 * 1024 * 1024 + 5,), float("nan"), device="cuda")
    third = _grads_fused(dcl, *ins)
    torch.cuda.synchronize()
    for name, x, y, z in zip(NAMES, first, second, third):
        assert torch.equal(x, y), name
        assert torch.equal(x, z), name
    del keep, junk


# ---------------------------------------------------------------------------------------------------- autograd
def test_autograd_function(dcl):
    Fn = dcl.autograd.CrossAttentionFn
    Q, K, V1, V2, dO1, dO2 = _inputs(2, 150, 90, 1.0, seed=7)
    O1, O2 = _forward(dcl, Q, K, V1, V2)
    leaves = [t.clone().requires_grad_(True) for t in (Q, K, V1, V2)]
    o1, o2 = Fn.apply(*leaves)
    assert o1.shape == (2, 150, 256) and o2.shape == (2, 150, 64)
    assert torch.equal(o1.reshape(-1, 256), O1) and torch.equal(o2.reshape(-1, 64), O2)          # the op's own bits
    # non-contiguous incoming gradients
    g1 = dO1.transpose(1, 2).contiguous().transpose(1, 2)
    g2 = dO2.transpose(1, 2).contiguous().transpose(1, 2)
    assert not g1.is_contiguous()
    torch.autograd.backward([o1, o2], [g1, g2])
    want = _grads_fused(dcl, Q, K, V1, V2, dO1, dO2)
    for name, t, w in zip(NAMES, leaves, want):
        assert torch.equal(t.grad, w), name

    # the keys as the second value tensor (DCL-Net's O2 = bmm(F_m, A)): K.grad = dK + dV2
    q, k, v1 = [t.clone().requires_grad_(True) for t in (Q, K, V1)]
    o1, o2 = Fn.apply(q, k, v1, k)
    torch.autograd.backward([o1, o2], [dO1, dO2])
    wk = _grads_fused(dcl, Q, K, V1, K, dO1, dO2)
    assert torch.equal(q.grad, wk[0]) and torch.equal(v1.grad, wk[2])
    assert torch.equal(k.grad, wk[1] + wk[3])

    # only O1 used = a zero gradient for O2
    leaves = [t.clone().requires_grad_(True) for t in (Q, K, V1, V2)]
    o1, o2 = Fn.apply(*leaves)
    (o1 * dO1).sum().backward()
    want0 = _grads_fused(dcl, Q, K, V1, V2, dO1, torch.zeros_like(dO2))
    for name, t, w in zip(NAMES, leaves, want0):
        assert torch.equal(t.grad, w), name

    # inputs that need no gradient get none
    q = Q.clone().requires_grad_(True)
    o1, o2 = Fn.apply(q, K, V1, V2)
    torch.autograd.backward([o1, o2], [dO1, dO2])
    assert torch.equal(q.grad, want[0]) and K.grad is None and V1.grad is None and V2.grad is None
    o1, o2 = Fn.apply(Q, K, V1, V2)
    assert not o1.requires_grad and not o2.requires_grad


# ---------------------------------------------------------------------------------------------------- no map
def test_no_map_sized_allocation(dcl):
    """b = 2, nq = nk = 4096: one attention map is 128 MiB; every per-point tensor of the call together is about 45 MiB"""
    b, n = 2, 4096
    one_map = b * n * n * 4
    Q, K, V1, V2, dO1, dO2 = _inputs(b, n, n, 1.0, seed=9)

    def peak_of(step):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        step()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    def fused():
        leaves = [t.clone().requires_grad_(True) for t in (Q, K, V1, V2)]
        o1, o2 = dcl.autograd.CrossAttentionFn.apply(*leaves)
        torch.autograd.backward([o1, o2], [dO1, dO2])
        assert all(bool(torch.isfinite(t.grad).all()) for t in leaves)

    fused()                                                    # (first-use allocations of the libraries are not the op's)
    rise = peak_of(fused)
    rise_mat = peak_of(lambda: _grads_materialised(Q, K, V1, V2, dO1, dO2))
    print("attention_grad peak memory above the inputs at 2 x 4096 x 4096: fused %.1f MiB, materialised %.1f MiB, one map %.1f MiB"
          % (rise / 2 ** 20, rise_mat / 2 ** 20, one_map / 2 ** 20))
    assert rise < one_map, (rise, one_map)
    assert rise_mat >= 2 * one_map, (rise_mat, one_map)       # scores and softmax at the least


# ---------------------------------------------------------------------------------------------------- launch census
def _bwd_kernels(seen):
    return {k: v for k, v in seen.items() if k.startswith("k_attn_bwd")}


def test_launch_census(request, dcl):
    import test_gpu_ops as TO
    import test_kernel_census as TC
    lib = TO.enter_diag(dcl, request)
    counts = []
    for nk in (40, 700, 5000):
        Q, K, V1, V2, dO1, dO2 = _inputs(2, 300, nk, 1.0, seed=13)
        O1, O2 = _forward(dcl, Q, K, V1, V2)
        torch.cuda.synchronize()
        lib.dcl_debug_launch_census_reset()
        dcl.ops.cross_attention_backward(2, Q.reshape(-1, 64), K.reshape(-1, 64), V1.reshape(-1, 256), V2.reshape(-1, 64), O1, O2,
                                         dO1.reshape(-1, 256), dO2.reshape(-1, 64))
        torch.cuda.synchronize()
        seen = {k: v for k, v in TC.census(lib).items() if v}
        assert seen and seen == _bwd_kernels(seen), seen                   # kernels of attention_bwd.hip only
        counts.append(sum(seen.values()))
    assert counts[0] == counts[1] == counts[2], counts                      # a number of launches independent of nk
    src = open(os.path.join(TC.ROOT, "dcl-net_amd", "csrc", "attention_bwd.hip")).read()
    for k in seen:
        assert k.split("<")[0] in src, k


# ---------------------------------------------------------------------------------------------------- Network
FIXTURE = "dclnet_nm384_train.npz"


def _net(dcl, golden_dir, **kw):
    data, exp, (b, n_inp, n_tmp, wseed) = load_golden_data(os.path.join(golden_dir, FIXTURE))
    cfg = dcl.synth.default_cfg(n_inp, n_tmp, unit=0.005)
    net = dcl.DCL_Net.Network(cfg, mode="train", **kw)
    net.load_state_dict(dcl.synth.synth_state_dict(net, wseed))
    return net.cuda(), data, exp


def test_network_fused_attention_outputs_match_reference_golden(dcl, golden_dir):
    """the compat path with eval-mode BatchNorm, as test_gpu_network.test_train_mode_outputs_match_reference_golden pins it"""
    import test_gpu_network as TN
    net, data, exp = _net(dcl, golden_dir, fused=False, train_attention="fused")
    net = net.eval()
    with torch.no_grad():
        pred = net(data)
    TN._check(pred, exp["rot_pred"], exp["trans_pred"], exp["conf"])
    for k in ("Xo_pred", "Yc_pred"):
        assert tuple(pred[k].shape) == exp[k].shape
        assert np.abs(pred[k].cpu().numpy() - exp[k]).max() <= 1e-4 * max(1.0, np.abs(exp[k]).max()), k
    lo = dcl.DCL_Net.losses(None)(pred, data["labels"])
    got = np.array([float(lo[k]) for k in ("loss_pose", "loss_Xo", "loss_Yc", "loss_conf", "loss_all")])
    assert np.abs(got - exp["losses"]).max() <= 2e-4 * max(1.0, np.abs(exp["losses"]).max())


def _train_step(dcl, golden_dir, **kw):
    net, data, _ = _net(dcl, golden_dir, **kw)
    net = net.train()
    pred = net(data)
    dcl.DCL_Net.losses(None)(pred, data["labels"])["loss_all"].backward()
    torch.cuda.synchronize()
    return net, pred


def test_network_parameter_gradients_agree(dcl, golden_dir):
    """a wiring check (a dropped dV2 term or a transposed operand is an error of order 1): the precision claim rests on
    test_gradients_match_fp64.  No bit-equality between training steps is asserted: the sparse half's gradients keep the
    reference's atomic scatter.  Measured on an MI355X: the largest difference is 1.84e-3 x max|grad| (neck_fuser_bi.layers.6.bias,
    the bias in front of a ReLU + train-mode BatchNorm; the same figure run after run), the next ones 9.2e-4 and 8.0e-4."""
    net_m, _ = _train_step(dcl, golden_dir, train_attention="materialised")
    net_f, _ = _train_step(dcl, golden_dir, train_attention="fused")
    ratios = []
    pm = dict(net_m.named_parameters())
    for name, p in net_f.named_parameters():
        gm, gf = pm[name].grad, p.grad
        assert gm is not None and gf is not None, name
        assert bool(torch.isfinite(gf).all()) and bool(torch.isfinite(gm).all()), name
        scale = float(gm.abs().max())
        d = float((gf - gm).abs().max())
        ratios.append((d / scale if scale > 0 else (0.0 if d == 0 else float("inf")), name))
    ratios.sort(reverse=True)
    print("attention_grad network: largest parameter-gradient differences fused vs materialised, in units of max|grad|: "
          + ", ".join("%.3e (%s)" % r for r in ratios[:4]))
    assert ratios[0][0] <= 2e-3, ratios[:4]


def test_network_default_is_the_materialised_path(request, dcl, golden_dir):
    import test_gpu_ops as TO
    import test_kernel_census as TC
    lib = TO.enter_diag(dcl, request)
    lib.dcl_debug_launch_census_reset()
    _, pred_d = _train_step(dcl, golden_dir)
    seen_d = TC.census(lib)
    _, pred_m = _train_step(dcl, golden_dir, train_attention="materialised")
    for k in ("rot_pred", "trans_pred", "conf", "F_Xo_p", "Xo_pred", "Yc_pred"):
        assert torch.equal(pred_d[k], pred_m[k]), k
    assert not _bwd_kernels({k: v for k, v in TC.census(lib).items() if v})
    assert any(k.startswith("k_") for k, v in seen_d.items() if v), seen_d           # the census did count the step
    lib.dcl_debug_launch_census_reset()
    _train_step(dcl, golden_dir, train_attention="fused")
    seen_f = _bwd_kernels({k: v for k, v in TC.census(lib).items() if v})
    assert seen_f.get("k_attn_bwd_stats", 0) == 2, seen_f                              # one backward per direction
    assert sum(v for k, v in seen_f.items() if k.startswith("k_attn_bwd_sweep")) == 4, seen_f
