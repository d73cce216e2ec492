"""Whole-step checks of the all-kernels training configuration, Network(cfg, mode="train", **DCL_Net.TRAIN_KERNELS) with the
fused Chamfer, the fused objective and dcl.optim.Adam + AutoClip: what a lone Function's test cannot see.

1. tests/step_replay.py records every call of every Function class of dcl.autograd during two consecutive steps at (b, n) =
   (2, 256) and (3, 192) -- 576 rows, no power of two, an odd crop count -- and checks on the way that no backward writes over
   its incoming gradient (a), that nothing a Function may have saved changed before its backward (b) and that no custom node
   of the loss's graph went unrecorded (c).
2. Every recorded call is replayed alone on contiguous clones: outputs, updated running statistics and every returned gradient
   must have the recorded bits, which ties the layouts the network passes (column blocks, views, strided gradients, the same
   tensor as K and V2) to what the Functions' own float64 tests verify.  A Function that does not promise pinned order would be
   named in NOT_PINNED with the bound of its own test; the all-kernels step has none: every Function it reaches promises the
   same bits for the same inputs (include/dclnet_hip.h, the classes' docstrings), so NOT_PINNED is empty and every comparison
   is bit for bit.  A second run from the same initial state repeats the loss and every parameter gradient of both steps.
3. train_conv_wgrad and train_conv_dgrad change no forward kernel; the gradients that cannot depend on them are asserted bit
   for bit against a default network (see the two tests' docstrings for the derivation).  train_rotation: the "host" form
   composes U diag(1, 1, det) V^T from a LAPACK SVD on the host, which is not the eval kernel's arithmetic, so "device" does
   not keep the default network's forward bits and no such assertion exists for it.
4. For each Function class the step runs, the recorded call with the most rows (step 1 of (2, 256)) is checked against the
   float64 form and the fp32 module form the case modules hold, under the project's rule err <= max(2 err_module, 1e-6
   max|ref64|), each form against the float64 twin with its own ReLU masks / nearest-neighbour indices.  No class is left out;
   VoxelizationFn is forward only (the voxel features are data and take no gradient), and SparseAvgPoolFn's divisor, which is
   no recorded operand, is counted from the recorded neighbour table.
   Finding: PointLinearFn's bias gradient (ops.relu_bwd) missed the rule on the (512, 512) fuser layer -- max|ref| 1.2e-4, err
   1.92e-10, err_module 7.41e-11, bound 1.48e-10 -- because csrc/linear_bwd.hip added a split's 512 masked gradients of mixed
   sign in ONE fp32 chain; the chain's accumulator is float64 now (same order, one rounding per split), and the case stays.
5. The torch-native backward nodes of the step that do arithmetic on activations (convolution, matrix products, batch norm,
   softmax) are pinned as found: a later switch that quietly falls back to the module path adds one and fails here."""
import numpy as np
import pytest
import torch

import bn_relu_cases as B
import conf_pool_cases as CP
import conv_grad_cases as CG
import heads_cases as H
import objective_cases as OC
import step_replay as SR
import train_dense_cases as TD

pytestmark = pytest.mark.gpu

SHAPES = [(2, 256), (3, 192)]
IDS = ["b%dn%d" % s for s in SHAPES]
NOT_PINNED = {}                     # class name -> absolute bound of its own stand-alone test; empty: everything is bit for bit
# the Function classes the all-kernels step must reach (VoxelizationFn forward only: the voxel features take no gradient)
REACHED = ("VoxelizationFn", "SparseConvFn", "BnReluFn", "SparseAvgPoolFn", "ThreeInterpolateFn", "PointLinearFn",
           "CrossAttentionFn", "NarrowLinearFn", "ConfPoolPmFn", "PoseHeadsFn", "Ortho9dFn", "RigidPointsFn", "ChamferFn",
           "PoseObjectiveFn")
# part 5, as found on an MI355X: no torch-native convolution, matrix-product, batch-norm or softmax node is left
CENSUS = set()


@pytest.fixture(scope="module")
def runs(dcl):
    """get(b, n) -> the recorded two-step run of that shape (made once): dict(rec, calls, steps, census, nodes, error)"""
    mp = pytest.MonkeyPatch()
    rec = SR.StepRecorder(SR.function_classes(dcl.autograd), mp, SR.MUTATED)
    rec.active = False
    done = {}

    def get(b, n):
        if (b, n) not in done:
            rec.calls, rec.step, rec.active = [], 0, True
            census, nodes, out = [], [], dict(rec=rec, error=None, steps=None)

            def on_loss(s, loss, net):
                census.append((SR.arithmetic_nodes(loss), SR.torch_nodes(loss)))
                nodes.append(rec.count_custom_nodes(loss))
            try:
                _, out["steps"] = SR.run_steps(dcl, b, n, rec=rec, on_loss=on_loss)
            except SR.ReplayError as e:
                out["error"] = e
            finally:
                rec.active = False
            out.update(calls=rec.calls, census=census, nodes=nodes)
            done[(b, n)] = out
        if done[(b, n)]["error"] is not None:
            raise done[(b, n)]["error"]
        return done[(b, n)]
    yield get
    mp.undo()


# ---------------------------------------------------------------------------------------------------- parts 1 and 2
@pytest.mark.parametrize("b,n", SHAPES, ids=IDS)
def test_no_gradient_or_saved_tensor_is_overwritten_and_every_custom_node_is_recorded(runs, b, n):
    """checks (a), (b), (c) of the recorder over two consecutive steps (a failure is raised where it is found and names the
    call), every expected class is reached, and both steps have the same calls in the same order"""
    r = runs(b, n)
    rec = r["rec"]
    for step in (1, 2):
        calls = [c for c in r["calls"] if c.step == step]
        counts = {}
        for c in calls:
            counts[c.name] = counts.get(c.name, 0) + 1
        ran = sum(c.grads_in is not None for c in calls)
        print("b=%d n=%d step %d: %d calls, %d custom nodes: %s" % (b, n, step, len(calls), r["nodes"][step - 1], counts))
        assert set(counts) == set(REACHED), sorted(set(counts) ^ set(REACHED))
        assert r["nodes"][step - 1] == ran > 0
        assert len(calls) - ran == counts["VoxelizationFn"]          # the only calls outside the graph
    assert [c.name for c in r["calls"] if c.step == 1] == [c.name for c in r["calls"] if c.step == 2]
    assert rec.active is False


@pytest.mark.parametrize("b,n", SHAPES, ids=IDS)
def test_every_recorded_call_replays_bit_for_bit_on_contiguous_clones(runs, b, n):
    r = runs(b, n)
    rec = r["rec"]
    rec.active = True
    try:
        failures, strided = [], 0
        for c in r["calls"]:
            strided += any(isinstance(a, torch.Tensor) and not a.is_contiguous() for a in c.args)
            report = []
            bad = rec.replay(c, report)
            if bad and c.name in NOT_PINNED:
                bad = ["%s: %.3g > %.3g" % (w, e, NOT_PINNED[c.name]) for w, e, _ in report if not e <= NOT_PINNED[c.name]]
            if bad:
                failures.append((repr(c), bad))
    finally:
        rec.active = False
    print("b=%d n=%d: %d calls replayed, %d of them took a non-contiguous input in the network" % (b, n, len(r["calls"]), strided))
    assert not failures, "first of %d: %s" % (len(failures), failures[0])
    assert strided > 0                                               # the network does pass views: the replay compares layouts


@pytest.mark.parametrize("b,n", SHAPES, ids=IDS)
def test_a_second_run_repeats_the_loss_and_every_parameter_gradient_of_both_steps(dcl, runs, b, n):
    """a new network, the same seed, initial state and batch, the recorder switched off: step 2 covers everything derived from
    the weights after an optimiser step"""
    r = runs(b, n)
    assert r["rec"].active is False
    _, again = SR.run_steps(dcl, b, n)
    for s, (one, two) in enumerate(zip(r["steps"], again)):
        assert bool(torch.isfinite(one["loss"])) and SR.same_bits(one["loss"], two["loss"]), (s, float(one["loss"]), float(two["loss"]))
        assert set(one["grads"]) == set(two["grads"])
        bad = [k for k, g in one["grads"].items() if g is None or two["grads"][k] is None or not SR.same_bits(g, two["grads"][k])]
        assert bad == [], (s, bad[:5], len(bad))
        for k, v in one["pred"].items():
            assert SR.same_bits(v, two["pred"][k]), (s, k)
    assert not SR.same_bits(r["steps"][0]["loss"], r["steps"][1]["loss"])        # the optimiser did step in between


# ---------------------------------------------------------------------------------------------------- part 5
@pytest.mark.parametrize("b,n", SHAPES, ids=IDS)
def test_census_of_the_arithmetic_left_on_torch(runs, b, n):
    r = runs(b, n)
    for s, (arith, every) in enumerate(r["census"]):
        print("b=%d n=%d step %d torch-native nodes: %s" % (b, n, s + 1, dict(sorted(every.items()))))
        assert arith == CENSUS, sorted(arith ^ CENSUS)


# ---------------------------------------------------------------------------------------------------- part 3
def _one_step(dcl, **switches):
    _, (out,) = SR.run_steps(dcl, 2, 256, steps=1, switches=switches)
    return out


@pytest.fixture(scope="module")
def default_step(dcl):
    return _one_step(dcl)


def _conv_names(dcl, net_switches=None):
    net = dcl.DCL_Net.Network(dcl.synth.default_cfg(256, 256), mode="train")
    conv = {id(m.weight) for m in net.modules() if isinstance(m, dcl.spconv.SparseConvolution)}
    names = [k for k, p in net.named_parameters() if id(p) in conv]
    assert len(names) == 16
    return names, [k for k, _ in net.named_parameters()]


def _same_everywhere(one, two, names):
    return [k for k in names if not SR.same_bits(one["grads"][k], two["grads"][k])]


def test_wgrad_pairs_changes_nothing_but_the_sparse_convolutions_weight_gradients(dcl, default_step):
    """Derived as independent of train_conv_wgrad: the loss, every prediction, and the gradient of every parameter except the 16
    `backbone_{inp,tmp}.module{1..4}.{0,1}.layers.0.weight`.  From: Network.__init__ sets only SparseConvolution.wgrad
    (models/DCL_Net.py, the loop over both backbones' modules); spconv/conv.py hands it to SparseConvFn.apply, whose forward
    does not read it (autograd.py: SparseConvFn.forward passes `fwd` alone to ops.sparse_conv); ops.sparse_conv_backward
    (ops.py:3063-3072) branches on wgrad only where dW is formed, and dx (ops.py:3073-3081) reads dout, nbr and W, never dW."""
    conv, every = _conv_names(dcl)
    got = _one_step(dcl, train_conv_wgrad="pairs")
    assert SR.same_bits(got["loss"], default_step["loss"])
    assert [k for k, v in default_step["pred"].items() if not SR.same_bits(v, got["pred"][k])] == []
    assert _same_everywhere(got, default_step, [k for k in every if k not in conv]) == []
    assert len(_same_everywhere(got, default_step, conv)) > 0          # the switch is wired: another summation order


def test_dgrad_direct_changes_nothing_downstream_of_the_two_layers_it_runs_on(dcl, default_step):
    """Derived as independent of train_conv_dgrad: the loss, every prediction, the gradient of every parameter outside the two
    backbones (the dense half and the heads; the losses have none), and in each backbone the last block's
    `module4.1.layers.0.weight` (the 128 -> 256 convolution nearest the output) with its BatchNorm's `module4.1.layers.1.weight`
    and `.bias`.  From: ops.conv_dgrad_form selects "direct" on (cin, cout) in ops.CONV_DGRAD_DIRECT_WIDTHS = {(16, 32),
    (128, 256)} (ops.py:2995-3007), module1.1 and module4.1; SparseConvFn.forward does not read dgrad; ops.sparse_conv_backward
    forms dW before and without dx (ops.py:3063-3072) and branches on dgrad for dx alone (ops.py:3076-3081); a block's BatchNorm
    gradient reads the block's own input and incoming gradient (BnReluFn.backward); the backward reaches the backbones after
    the dense half, the read-out and the pools, so nothing there reads a convolution's dx.  Everything upstream of module4.1
    in a backbone takes its dx and may differ."""
    conv, every = _conv_names(dcl)
    got = _one_step(dcl, train_conv_dgrad="direct")
    assert SR.same_bits(got["loss"], default_step["loss"])
    assert [k for k, v in default_step["pred"].items() if not SR.same_bits(v, got["pred"][k])] == []
    last = ["%s.module4.1.layers.%s" % (bb, p) for bb in ("backbone_inp", "backbone_tmp") for p in ("0.weight", "1.weight", "1.bias")]
    assert all(k in every for k in last)
    independent = [k for k in every if not k.startswith("backbone_")] + last
    assert len(independent) == len(every) - 2 * (8 + 16) + len(last)           # a backbone: 8 conv weights + 8 BatchNorm pairs
    assert _same_everywhere(got, default_step, independent) == []
    upstream = [k for k in every if k.startswith("backbone_") and k not in last]
    assert len(_same_everywhere(got, default_step, upstream)) > 0              # the switch is wired


# ---------------------------------------------------------------------------------------------------- part 4
def _cpu(t):
    return None if t is None else t.detach().cpu()


def _biggest(calls, name):
    """the step-1 call of a class with the most rows (ties: the most input elements), among those whose backward ran and whose
    first input takes a gradient where there are any"""
    c = [x for x in calls if x.name == name and x.step == 1]
    c = [x for x in c if x.grads_in is not None] or c
    c = [x for x in c if x.requires_grad[0]] or c
    return max(c, key=lambda x: (x.rows, sum(a.numel() for a in x.inputs if isinstance(a, torch.Tensor))))


def _rule(tag, got, ref64, module, module_ref64, names):
    names = [k for k in names if got.get(k) is not None]
    TD.compare(tag, got, ref64, module, module_ref64, names)
    return names


def _leaf(t, dtype):
    return t.detach().to(dtype).clone().requires_grad_(True)


def _check_point_linear(dcl, c):
    x, W, bias, relu = c.inputs
    N, K = W.shape[0], W.shape[1]
    k = dict(x=_cpu(x), W=_cpu(W).reshape(N, K, 1), bias=torch.zeros(N) if bias is None else _cpu(bias), g=_cpu(c.grads_in[0]))
    got = dict(y=c.outputs[0], dx=c.grads_out[0], dW=c.grads_out[1].reshape(N, K, 1), db=c.grads_out[2])
    mask = (_cpu(c.outputs[0]) > 0) if relu else None
    module = TD.linear_form(k, relu, torch.float32)
    return _rule("PointLinearFn %s" % (tuple(x.shape),), got, TD.linear_form(k, relu, torch.float64, mask), module,
                 TD.linear_form(k, relu, torch.float64, module["mask"]), ("y", "dx", "dW", "db"))


def _check_bn_relu(dcl, c):
    x, gamma, beta, rm, rv, momentum, eps = c.inputs[:7]
    relu = bool(c.inputs[7]) if len(c.inputs) > 7 else True
    k = dict(x=_cpu(x), gamma=_cpu(gamma), beta=_cpu(beta), g=_cpu(c.grads_in[0]), running_mean=_cpu(rm), running_var=_cpu(rv))
    got = dict(z=c.outputs[0], running_mean=c.expect[3], running_var=c.expect[4], dx=c.grads_out[0], dgamma=c.grads_out[1],
               dbeta=c.grads_out[2])
    f64 = lambda mask: B.formulas64(k["x"], k["gamma"], k["beta"], k["g"], eps, momentum, k["running_mean"],      # noqa: E731
                                    k["running_var"], mask, relu)
    module = B.module_form(k, torch.float32, relu, eps, momentum)
    names = [n for n in ("z", "running_mean", "running_var", "dx", "dgamma", "dbeta") if got[n] is not None]
    B.compare("BnReluFn %s relu=%s" % (tuple(x.shape), relu), got, f64(_cpu(c.outputs[0]) > 0 if relu else None), module,
              f64(module["z"] > 0 if relu else None), names)
    return names


def _check_narrow(dcl, c):
    x, W, bias = c.inputs
    N, K = W.shape[0], W.shape[1]
    k = dict(x=_cpu(x), W=_cpu(W).reshape(N, K, 1), bias=_cpu(bias), g=_cpu(c.grads_in[0]))
    got = dict(y=c.outputs[0], dx=c.grads_out[0], dW=c.grads_out[1].reshape(N, K, 1), db=c.grads_out[2])
    ref = H.narrow_form(k, torch.float64)
    return _rule("NarrowLinearFn %s" % (tuple(x.shape),), got, ref, H.narrow_form(k, torch.float32), ref, H.NARROW_OUT)


def _check_conf_pool_pm(dcl, c):
    l1, l2, F1, F2 = (_cpu(t) for t in c.inputs)
    b = l1.shape[0]
    cm = lambda F: F.view(b, F.shape[0] // b, -1).transpose(1, 2).contiguous()               # noqa: E731
    ops = (l1.reshape(b, 1, -1), l2.reshape(b, 1, -1), cm(F1), cm(F2), _cpu(c.grads_in[0]), _cpu(c.grads_in[1]))
    pm = lambda F: None if F is None else F.transpose(1, 2).reshape(-1, F.shape[1])          # noqa: E731
    form = lambda dt: {k: (pm(v) if k in ("dF1", "dF2") else v)                              # noqa: E731
                       for k, v in CP.module_form(*(t.to(dt) for t in ops)).items()}
    got = dict(conf=c.outputs[0], pooled=c.outputs[1], dlogit1=c.grads_out[0].reshape(b, -1), dlogit2=c.grads_out[1].reshape(b, -1),
               dF1=c.grads_out[2], dF2=c.grads_out[3])
    names = ("conf",) + CP.OUTPUTS
    CP.compare("ConfPoolPmFn %s" % (tuple(F1.shape),), got, form(torch.float64), form(torch.float32), names)
    return names


def _check_pose_heads(dcl, c):
    k = dict(zip(("x",) + H.PARAMS, (_cpu(t) for t in c.inputs)))
    k.update(g_o9=_cpu(c.grads_in[0]), g_t3=_cpu(c.grads_in[1]))
    _, _, h1, h2 = dcl.ops.pose_heads_train(c.inputs[0].contiguous(), [t.contiguous() for t in c.inputs[1:]])
    got = dict(o9=c.outputs[0], t3=c.outputs[1], dx=c.grads_out[0])
    got.update({"d_" + n: g.reshape(k[n].shape) for n, g in zip(H.PARAMS, c.grads_out[1:])})
    module = H.pose_form(k, torch.float32)
    return _rule("PoseHeadsFn %s" % (tuple(k["x"].shape),), got, H.pose_form(k, torch.float64, H.pose_masks(h1, h2)), module,
                 H.pose_form(k, torch.float64, module["masks"]), H.POSE_OUT)


def _check_sparse_conv(dcl, c):
    feat, W, nbr, n_out = c.inputs[:4]
    X, Wn, G = _cpu(feat).numpy(), _cpu(W).numpy(), _cpu(c.grads_in[0]).numpy()
    pairs, num = CG.pairs_of_table(_cpu(nbr).numpy(), n_out, X.shape[0])
    assert int(num.sum()) > 0
    form = lambda dt: dict(zip(("out", "dx", "dW"), (torch.from_numpy(a) for a in                        # noqa: E731
                                                      CG.conv_form(X, Wn, G, pairs, num, n_out, dt))))
    got = dict(out=c.outputs[0], dx=c.grads_out[0], dW=c.grads_out[1].reshape(-1, Wn.shape[-2], Wn.shape[-1]))
    ref = form(np.float64)
    return _rule("SparseConvFn %s -> %d rows, %s" % (tuple(feat.shape), n_out, c.inputs[5:]), got, ref, form(np.float32), ref,
                 ("out", "dx", "dW"))


def _check_attention(dcl, c):
    Q, K, V1, V2 = (_cpu(t) for t in c.inputs)
    shared = c.args[3] is c.args[1]
    dO1, dO2 = (_cpu(g) for g in c.grads_in)

    def form(dt):
        q, k, v1 = _leaf(Q, dt), _leaf(K, dt), _leaf(V1, dt)
        v2 = k if shared else _leaf(V2, dt)
        A = torch.softmax(torch.bmm(q, k.transpose(1, 2)), dim=2)
        O1, O2 = torch.bmm(A, v1), torch.bmm(A, v2)
        pairs = [(o, g.to(dt)) for o, g in ((O1, dO1), (O2, dO2)) if g is not None]
        torch.autograd.backward([o for o, _ in pairs], [g for _, g in pairs])
        return dict(O1=O1.detach(), O2=O2.detach(), dQ=q.grad, dK=k.grad, dV1=v1.grad, dV2=None if shared else v2.grad)
    gq, gk, gv1, gv2 = c.grads_out
    got = dict(O1=c.outputs[0], O2=c.outputs[1], dQ=gq, dK=gk if not shared else gk + gv2, dV1=gv1, dV2=None if shared else gv2)
    ref = form(torch.float64)
    return _rule("CrossAttentionFn %s keys %d" % (tuple(Q.shape), K.shape[1]), got, ref, form(torch.float32), ref,
                 ("O1", "O2", "dQ", "dK", "dV1", "dV2"))


def _check_chamfer(dcl, c):
    pred, target, active = c.inputs
    _, ipt, _, itp = dcl.ops.chamfer(pred.contiguous(), target.contiguous(), active)
    P, T = _cpu(pred), _cpu(target)
    live = torch.ones(P.shape[0], 1) if active is None else (_cpu(active) != 0).float().unsqueeze(1)
    g_pt, g_tp = (_cpu(g) for g in c.grads_in)
    take = lambda cloud, idx: torch.gather(cloud, 1, idx.clamp_min(0).long().unsqueeze(2).expand(-1, -1, 3))    # noqa: E731

    def form(dt, idx=None):
        """idx None: the module composition, both minima of the pairwise matrix (models/losses.py: cd_dis); given: the float64
        twin through those nearest-neighbour indices (tests/test_gpu_objective.py: _cd64)"""
        p, t = _leaf(P, dt), _leaf(T, dt)
        d = torch.norm(p.unsqueeze(2) - t.unsqueeze(1), dim=3)
        own = (d.argmin(dim=2), d.argmin(dim=1))
        if idx is None:
            pt, tp = d.min(dim=2)[0], d.min(dim=1)[0]
        else:
            pt, tp = torch.norm(p - take(t, idx[0]), dim=2), torch.norm(take(p, idx[1]) - t, dim=2)
        pt, tp = pt * live.to(dt), tp * live.to(dt)
        torch.autograd.backward([pt, tp], [g_pt.to(dt), g_tp.to(dt)])
        return dict(dist_pt=pt.detach(), dist_tp=tp.detach(), d_pred=p.grad, d_target=t.grad, idx=own)
    got = dict(dist_pt=c.outputs[0], dist_tp=c.outputs[1], d_pred=c.grads_out[0], d_target=c.grads_out[1])
    module = form(torch.float32)
    return _rule("ChamferFn %s" % (tuple(P.shape),), got, form(torch.float64, (_cpu(ipt), _cpu(itp))), module,
                 form(torch.float64, module["idx"]), ("dist_pt", "dist_tp", "d_pred", "d_target"))


def _check_rigid(dcl, c):
    pts, R, t, inverse = c.inputs
    g = _cpu(c.grads_in[0])

    def form(dt):
        p, r, tt = _leaf(_cpu(pts), dt), _leaf(_cpu(R), dt), _leaf(_cpu(t), dt)
        out = torch.bmm(p - tt.unsqueeze(1), r) if inverse else torch.bmm(p, r.transpose(1, 2)) + tt.unsqueeze(1)
        out.backward(g.to(dt))
        return dict(out=out.detach(), d_pts=p.grad, d_R=r.grad, d_t=tt.grad)
    got = dict(out=c.outputs[0], d_pts=c.grads_out[0], d_R=c.grads_out[1], d_t=c.grads_out[2])
    ref = form(torch.float64)
    return _rule("RigidPointsFn %s" % (tuple(pts.shape),), got, ref, form(torch.float32), ref, ("out", "d_pts", "d_R", "d_t"))


def _check_ortho9d(dcl, c):
    o9, g = _cpu(c.inputs[0]), _cpu(c.grads_in[0])

    def form(dt):
        x = _leaf(o9, dt)
        R = dcl.DCL_Net.ortho9d2matrix(x[:, :3], x[:, 3:6], x[:, 6:], "host")
        R.backward(g.to(dt))
        return dict(R=R.detach(), d_o9=x.grad)
    ref = form(torch.float64)
    return _rule("Ortho9dFn %s" % (tuple(o9.shape),), dict(R=c.outputs[0], d_o9=c.grads_out[0]), ref, form(torch.float32), ref,
                 ("R", "d_o9"))


def _check_three_interpolate(dcl, c):
    feat, idx, w = (_cpu(t) for t in c.inputs)
    g = _cpu(c.grads_in[0])

    def form(dt):
        f, ww = _leaf(feat, dt), w.to(dt)
        out = (f[idx.long()] * ww.unsqueeze(2)).sum(dim=1)
        out.backward(g.to(dt))
        return dict(out=out.detach(), d_feat=f.grad)
    ref = form(torch.float64)
    return _rule("ThreeInterpolateFn %s -> %d points" % (tuple(feat.shape), idx.shape[0]), dict(out=c.outputs[0], d_feat=c.grads_out[0]),
                 ref, form(torch.float32), ref, ("out", "d_feat"))


def _check_objective(dcl, c):
    a = [_cpu(t) for t in c.inputs]
    case = dict(posed=a[0], posed_gt=a[1], sym=a[2], cd_pose=(a[3], a[4]), Yc=a[5], cano_pred=a[6], cano_gt=a[7], Xo=a[8],
                conf=a[9], cd_Xo=(a[10], a[11]), cd_Yc=(a[12], a[13]))
    g = c.grads_out
    flat = lambda r: dict(packed=r["packed"], d_posed=r["posed"], d_Xo=r["Xo"], d_Yc=r["Yc"], d_conf=r["conf"],      # noqa: E731
                          d_cd_pose_pt=r["cd_pose"][0], d_cd_pose_tp=r["cd_pose"][1], d_cd_Xo_pt=r["cd_Xo"][0],
                          d_cd_Xo_tp=r["cd_Xo"][1], d_cd_Yc_pt=r["cd_Yc"][0], d_cd_Yc_tp=r["cd_Yc"][1])
    got = dict(packed=c.outputs[0], d_posed=g[0], d_cd_pose_pt=g[3], d_cd_pose_tp=g[4], d_Yc=g[5], d_Xo=g[8], d_conf=g[9],
               d_cd_Xo_pt=g[10], d_cd_Xo_tp=g[11], d_cd_Yc_pt=g[12], d_cd_Yc_tp=g[13])
    gp = _cpu(c.grads_in[0])
    ref = flat(OC.objective_form(case, gp, torch.float64))
    return _rule("PoseObjectiveFn %s" % (tuple(a[0].shape),), got, ref, flat(OC.objective_form(case, gp, torch.float32)), ref,
                 tuple(ref))


def _check_avgpool(dcl, c):
    feat, nbr, n_out = c.inputs
    X, G = _cpu(feat).numpy(), _cpu(c.grads_in[0]).numpy()
    pairs, num = CG.pairs_of_table(_cpu(nbr).numpy(), n_out, X.shape[0])
    form = lambda dt: dict(zip(("out", "d_feat"), (torch.from_numpy(a) for a in                          # noqa: E731
                                                    CG.avgpool_form(X, G, pairs, num, n_out, dt)[:2])))
    assert int(CG.avgpool_form(X, G, pairs, num, n_out, np.float64)[2].min()) >= 1           # every output row has an input row
    ref = form(np.float64)
    return _rule("SparseAvgPoolFn %s -> %d rows" % (tuple(feat.shape), n_out), dict(out=c.outputs[0], d_feat=c.grads_out[0]), ref,
                 form(np.float32), ref, ("out", "d_feat"))


def _check_voxelization(dcl, c):
    """forward only: the voxel features are data and take no gradient"""
    feats, rule = _cpu(c.inputs[0]), _cpu(c.inputs[1]).long()
    mode = c.inputs[2] if len(c.inputs) > 2 else 4
    cnt, ids = rule[:, 0], rule[:, 1:]
    live = (torch.arange(ids.shape[1]).unsqueeze(0) < cnt.unsqueeze(1)).unsqueeze(2)

    def form(dt):
        s = torch.where(live, feats.to(dt)[ids.clamp(0, feats.shape[0] - 1)], torch.zeros((), dtype=dt)).sum(dim=1)
        return dict(out=s / cnt.clamp_min(1).to(dt).unsqueeze(1) if mode == 4 else s)
    ref = form(torch.float64)
    return _rule("VoxelizationFn %s -> %d voxels" % (tuple(feats.shape), rule.shape[0]), dict(out=c.outputs[0]), ref,
                 form(torch.float32), ref, ("out",))


CHECKS = dict(VoxelizationFn=_check_voxelization, SparseAvgPoolFn=_check_avgpool, SparseConvFn=_check_sparse_conv, BnReluFn=_check_bn_relu, PointLinearFn=_check_point_linear,
              CrossAttentionFn=_check_attention, ConfPoolPmFn=_check_conf_pool_pm, NarrowLinearFn=_check_narrow,
              PoseHeadsFn=_check_pose_heads, ChamferFn=_check_chamfer, RigidPointsFn=_check_rigid, Ortho9dFn=_check_ortho9d,
              ThreeInterpolateFn=_check_three_interpolate, PoseObjectiveFn=_check_objective)
LEFT_OUT = ()                                                        # at most three may be; none is


def test_part_4_covers_every_class_but_the_named_ones():
    assert set(CHECKS) | set(LEFT_OUT) == set(REACHED) and not set(CHECKS) & set(LEFT_OUT) and len(LEFT_OUT) <= 3
    assert {"SparseConvFn", "BnReluFn", "PointLinearFn", "CrossAttentionFn", "ConfPoolPmFn"} <= set(CHECKS)


@pytest.mark.parametrize("name", sorted(CHECKS))
def test_float64_at_the_network_s_own_operands(dcl, runs, name):
    """the project's rule on the operands the network really passes: post-ReLU sparse rows, BatchNorm-scaled rows, a peaked
    confidence softmax, near-orthogonal 9-D heads, Chamfer on nearly aligned clouds"""
    c = _biggest(runs(2, 256)["calls"], name)
    print()
    forward_only = name == "VoxelizationFn"                          # its input is data: no node, no gradient
    assert forward_only or (c.grads_in is not None and c.grads_out is not None), c
    names = CHECKS[name](dcl, c)
    assert len(names) >= (1 if forward_only else 2), (name, names)   # an output and at least one gradient were compared
