"""Stage-2 pose refiner: drop-in for the reference's models/refiner.py:57-95 (same 18-key state_dict),
plus the iterative refinement loop of tools/test_YCBV_stage2.py:204-225 as a reusable function.

fused path: point-major GEMMs with bias+ReLU epilogues for MLP_share (259->512->512->1024), the
un-renormalised softmax slice (refiner.py:81) and the weighted sum as one GEMV-shaped reduction,
on-device 3x3 SVD.  Shapes are static, so `refine_loop(..., graph=True)` captures the loop body in a
hipGraph (torch.cuda.CUDAGraph) and replays it.
"""
import torch
import torch.nn as nn

from .. import ops
from .Modules import Head_MultiLayerPerceptron
from .losses import losses_refiner  # noqa: F401  (reference: models/refiner.py::losses_refiner)


def ortho9d2matrix(x_raw, y_raw, z_raw, train_rotation="host"):
    """models/refiner.py:34-56 == models/DCL_Net.py:15-36; differentiable when a gradient is needed (DCL_Net.ortho9d2matrix)"""
    from .DCL_Net import ortho9d2matrix as _o
    return _o(x_raw, y_raw, z_raw, train_rotation)


_VERSION_OF = __import__("operator").attrgetter("_version")


def _param_version(mod):
    """sum of the in-place version counters of every parameter and buffer: changes whenever a weight is rewritten in
    place (optimizer.step(), EMA swaps via p.data.copy_, manual surgery), so caches keyed on it cannot go stale"""
    ts = mod.__dict__.get("_vlist")
    if ts is None:
        ts = mod.__dict__["_vlist"] = list(mod.parameters()) + list(mod.buffers())
    return sum(map(_VERSION_OF, ts))


class Refiner(nn.Module):
    POSE_HEADS_MAX = 128      # crops up to which the two heads run as dcl_pose_heads (two launches; Network.POSE_HEADS_MAX)

    TRAIN_MLP_MODES = ("modules", "kernels")

    TRAIN_HEADS_MODES = ops.TRAIN_HEADS_MODES

    def __init__(self, cfg=None, train_rotation="host", train_mlp="modules", train_heads="modules", train_wgrad="fp32"):
        """train_rotation: "host" (default) or "device" -- how a call that needs a gradient differentiates the rotation
        head's projection; see DCL_Net.Network.
        train_mlp: how train() mode runs MLP_share and the pooling.  "modules" (default): the registered nn.Conv1d / nn.ReLU
        modules (vendor GEMMs in both passes).  "kernels": autograd.RefinerShareFn -- the library's own GEMM core forward, its
        own weight-gradient GEMM and ReLU / bias kernels backward, every reduction in a pinned order;
        needs n % 128 == 0 and inputs that do not require grad (ValueError otherwise).  eval() mode is the same either way.
        train_heads: how train() mode runs regressor_rot2 / regressor_trans2, in either train_mlp form.  "modules" (default): the
        registered modules (vendor GEMMs and element-wise launches on b rows).  "kernels": ONE autograd.PoseHeadsFn on the pooled
        feature (csrc/pose_heads_grad.hip: three launches forward, at most six backward, the weights read as registered, pinned
        summation orders).  Same parameters and state_dict keys, no cached weights; eval() mode never reads it.
        train_wgrad: the form of RefinerShareFn's weight gradients.  "fp32" (default): ops.linear_wgrad.  "split":
        ops.linear_wgrad_split (the bf16 matrix pipe, fp32-sized errors, its own pinned order) on the layers whose shape is in
        ops.WGRAD_SPLIT_SHAPES, ops.linear_wgrad on the others.  Read only by train_mlp="kernels" (ValueError otherwise)."""
        super().__init__()
        from .DCL_Net import check_train_rotation
        self.train_rotation = check_train_rotation(train_rotation)
        if train_mlp not in self.TRAIN_MLP_MODES:
            raise ValueError('train_mlp must be "modules" or "kernels", got %r' % (train_mlp,))
        self.train_mlp = train_mlp
        self.train_heads = ops.check_train_heads(train_heads)
        if ops.check_linear_wgrad(train_wgrad, "train_wgrad") == "split" and train_mlp != "kernels":
            raise ValueError('train_wgrad="split" requires train_mlp="kernels" (the modules form their weight gradients '
                             'themselves), got train_mlp=%r' % (train_mlp,))
        self.train_wgrad = train_wgrad
        self.MLP_share = Head_MultiLayerPerceptron([256 + 3, 512, 512, 1024], ["relu"] * 3, [False] * 3, [0.0] * 3)
        self.regressor_rot2 = Head_MultiLayerPerceptron([1024, 512, 128, 9], ["relu", "relu", "none"], [False] * 3,
                                                        [0.0] * 3)
        self.regressor_trans2 = Head_MultiLayerPerceptron([1024, 512, 128, 3], ["relu", "relu", "none"], [False] * 3,
                                                          [0.0] * 3)
        self._folded = None

    def _invalidate(self):
        """folded weights and captured refine-loop graphs (folded tensors' addresses baked in) follow the parameters"""
        self._folded = None
        self.__dict__.pop("_graphs", None)
        self.__dict__.pop("_vlist", None)

    def train(self, mode=True):
        self._invalidate()
        return super().train(mode)

    def _apply(self, fn, *a, **k):
        self._invalidate()
        return super()._apply(fn, *a, **k)

    def load_state_dict(self, *a, **k):
        self._invalidate()
        return super().load_state_dict(*a, **k)

    def __getstate__(self):
        state = dict(self.__dict__)
        state.pop("_graphs", None)
        state.pop("_vlist", None)
        state["_folded"] = None
        return state

    def _fold(self):
        ver = _param_version(self)
        if self._folded is not None and self.__dict__.get("_fold_version") != ver:
            self._invalidate()                       # weights were rewritten in place since the fold / the graph capture
        if self._folded is None:
            self.__dict__["_fold_version"] = ver
            with torch.no_grad():
                f = {}
                for name in ("MLP_share", "regressor_rot2", "regressor_trans2"):
                    L = getattr(self, name).layers
                    f[name] = [(L[i].weight[:, :, 0].t().contiguous(), L[i].bias.contiguous()) for i in (0, 2, 4)]
                # split the 259-row first weight: rows 0..2 act on xyz, rows 3.. on F_Xo_p
                Wt, bias = f["MLP_share"][0]
                f["share0_xyz"], f["share0_feat"] = Wt[:3].contiguous(), Wt[3:].contiguous()
                # the big layers prepared for the split-bf16 GEMM core (ops.prepare_linear; models/DCL_Net.py: _fold)
                for Wt in (f["share0_feat"], f["MLP_share"][1][0], f["MLP_share"][2][0]):
                    ops.prepare_linear(Wt)
            self._folded = f
        return self._folded

    def forward_pm(self, xyz_pm, feat_term, conf_w):
        """Point-major core: xyz_pm (b*n,3) canonicalised points, feat_term (b*n,512) = F_Xo_p @ W0[3:] + b0
        (constant over refinement iterations), conf_w (b,n) softmax slice.  -> (delta_t (b,3), delta_R (b,3,3))."""
        f = self._fold()
        b, n = conf_w.shape
        # first shared layer: the K = 3 product + the constant term + ReLU in one pass (ops.affine3_relu; a library GEMM and a
        # ReLU sweep before: 49 -> ~27 us per iteration at 32 768 rows)
        h = ops.affine3_relu(xyz_pm.contiguous(), f["share0_xyz"], feat_term)
        # (the own GEMM core, ops.linear -> csrc/linear_dma.hip: no vendor kernel that a caller overlapping the refiner with
        #  another forward's GEMMs could hang the GPU with; see models/DCL_Net.py: _lin_relu)
        h = ops.linear(h, f["MLP_share"][1][0], f["MLP_share"][1][1], True)
        if n % ops.LINEAR_POOL_TILE == 0:
            # the last shared layer with the confidence-weighted sum over the points as its epilogue: the (b*n, 1024) activation
            # is never stored; a crop's n / 128 tile partials are added in tile order
            part = ops.linear_pool(h, f["MLP_share"][2][0], f["MLP_share"][2][1], conf_w.reshape(-1), relu=True)
            shared = part.view(b, n // ops.LINEAR_POOL_TILE, -1).sum(dim=1)                  # (b, 1024)
        else:
            h = ops.linear(h, f["MLP_share"][2][0], f["MLP_share"][2][1], True)              # (b*n, 1024)
            shared = torch.bmm(conf_w.unsqueeze(1), h.view(b, n, -1)).squeeze(1)             # (b, 1024)
        # both pose heads (1024 -> 512 -> 128 -> 9 | 3) and the rotation in two launches (ops.pose_heads, as in stage 1) instead of
        # six library GEMMs of 5-14 us each on 32 rows + the ortho kernel; larger batches keep the library
        if b <= self.POSE_HEADS_MAX:
            _, dt, dR = ops.pose_heads(shared, f["regressor_rot2"], f["regressor_trans2"], with_rotation=True)
            return dt, dR

        def head(x, layers):
            x = ops.linear(x, layers[0][0], layers[0][1], True)
            x = ops.linear(x, layers[1][0], layers[1][1], True)
            return ops.linear(x, layers[2][0], layers[2][1], False)
        o9 = head(shared, f["regressor_rot2"])
        return head(shared, f["regressor_trans2"]), ops.ortho9d_to_matrix(o9)

    def _train_heads(self, shared):
        """the two heads of a train-mode forward on shared (b, 1024, 1) -> the prediction dict"""
        if self.train_heads == "kernels":
            from ..autograd import PoseHeadsFn
            from .DCL_Net import pose_head_params
            o9, delta_t = PoseHeadsFn.apply(shared.squeeze(2), *pose_head_params(self.regressor_rot2, self.regressor_trans2))
        else:
            o9 = self.regressor_rot2(shared).squeeze(-1)
            delta_t = self.regressor_trans2(shared).squeeze(-1)
        return {"trans_pred": delta_t, "rot_pred": ortho9d2matrix(o9[:, :3], o9[:, 3:6], o9[:, 6:], self.train_rotation)}

    def _forward_modules(self, x, conf):
        """training path (tools/train_YCBV_stage2.py:169,243-262 calls refiner.train(); outputs = refiner(inp);
        loss.backward()): the registered modules composed as the reference composes them (models/refiner.py:78-95), every
        step differentiable, no cached weights."""
        conf_softmax = torch.softmax(conf.unsqueeze(1), dim=2)[:, :, :1024]
        shared = (self.MLP_share(x) * conf_softmax).sum(dim=2, keepdim=True)
        return self._train_heads(shared)

    def _forward_kernels(self, x, conf):
        """training path with train_mlp="kernels": the shared MLP and the pooling as autograd.RefinerShareFn on point-major
        copies of the input (made once; the training script detaches input_features and conf, so no gradient leaves through
        them), then the two heads as the registered modules on the (b, 1024) pooled feature.  No cached weights: the function
        reads the registered parameters, so an optimizer step is seen whoever takes it."""
        from ..autograd import RefinerShareFn
        b, _, n = x.shape
        if n % ops.LINEAR_POOL_TILE:
            raise ValueError('train_mlp="kernels" needs n %% %d == 0 (the pooling tile), got n = %d'
                             % (ops.LINEAR_POOL_TILE, n))
        if x.requires_grad or conf.requires_grad:
            raise ValueError('train_mlp="kernels" takes input_features and conf that do not require grad (the training '
                             'script detaches them); train_mlp="modules" differentiates through them')
        conf_w = torch.softmax(conf.unsqueeze(1), dim=2)[:, 0, :1024].contiguous()           # refiner.py:81
        if tuple(conf_w.shape) != (b, n):
            raise ValueError('train_mlp="kernels" needs one confidence per point: conf[:, :1024] is %s for n = %d'
                             % (tuple(conf_w.shape), n))
        pm = x.float().transpose(1, 2)
        xyz_pm = pm[:, :, :3].reshape(b * n, 3)
        F_pm = pm[:, :, 3:].reshape(b * n, -1)
        L = self.MLP_share.layers
        args = (xyz_pm, F_pm, conf_w, L[0].weight, L[0].bias, L[2].weight, L[2].bias, L[4].weight, L[4].bias)
        # per weight-gradient block (W0's xyz columns, W0's feature columns, W1, W2): by the shape alone
        forms = tuple(ops.linear_wgrad_form(b * n, P, Q, self.train_wgrad)
                      for P, Q in ((L[0].out_channels, 3), (L[0].out_channels, F_pm.shape[1]),
                                   (L[2].out_channels, L[2].in_channels), (L[4].out_channels, L[4].in_channels)))
        if "split" in forms:
            args += (forms,)
        shared = RefinerShareFn.apply(*args).unsqueeze(2)
        return self._train_heads(shared)

    def forward(self, input_dict):
        """reference contract: {"input_features" (b,259,n), "conf" (b,n+m), "obj_idx"} ->
        {"trans_pred" (b,3), "rot_pred" (b,3,3)}.  train() mode: differentiable module path (train_mlp="kernels": its shared
        MLP on the library's own kernels); eval(): fused inference path (folded weights, no autograd graph)."""
        x = input_dict["input_features"]
        conf = input_dict["conf"]
        if not x.is_cuda:
            raise RuntimeError("dcl-net_amd.Refiner runs on the GPU only (no CPU fallback)")
        if self.training:
            if self.train_mlp == "kernels":
                return self._forward_kernels(x, conf)
            return self._forward_modules(x, conf)
        with torch.no_grad():
            f = self._fold()
            b, _, n = x.shape
            conf_w = torch.softmax(conf.unsqueeze(1), dim=2)[:, 0, :1024].contiguous()       # refiner.py:81
            pm = x.transpose(1, 2).reshape(b * n, -1)
            feat_term = ops.linear(pm[:, 3:], f["share0_feat"], f["MLP_share"][0][1], False)
            dt, dR = self.forward_pm(pm[:, :3].contiguous(), feat_term, conf_w)
        return {"trans_pred": dt, "rot_pred": dR}


COMPOSE_MODES = ("host", "device")


def refine_loop(refiner, pred, points_inp, iteration=2, graph=False, compose="host", trajectory=False):
    """Iterative refinement of tools/test_YCBV_stage2.py:204-225 on the outputs of Network.forward:
    pred {"rot_pred","trans_pred","F_Xo_p" (b,256,n),"conf"}, points_inp (b,n,3) -> (rot (b,3,3), trans (b,3)).
    With graph=True the whole loop is captured once per shape into a hipGraph and replayed.
    compose: where the pose lives between the iterations.  "host" (default): torch expressions compose it (pts - t, bmm, R @ dR:
    about a dozen launches per iteration, five of them vendor GEMMs on b x 3 x 3 operands).  "device": the current and the next
    pose live in device arrays rots (iteration + 1, b, 3, 3) / transs (iteration + 1, b, 3), index 0 the incoming pose, and one
    iteration is five launches of the library's own kernels -- ops.refine_first (canonicalisation + first shared layer),
    ops.linear, ops.linear_pool, ops.refine_heads (the tile partials added in a pinned order, both heads, R <- R dR and
    t <- R dt + t as the epilogue) -- no torch kernel, no vendor GEMM.  Needs n % ops.LINEAR_POOL_TILE == 0 and b <= 65535
    (ValueError otherwise; never a silent fall-back).  Not the "host" form's bits: the same formulas in other association orders.
    trajectory=True ("device" only): also returns (rots, transs), the pose after every iteration -- what the reference's script
    can only get by running the loop again."""
    if compose not in COMPOSE_MODES:
        raise ValueError('compose must be "host" or "device", got %r' % (compose,))
    if trajectory and compose != "device":
        raise ValueError('trajectory=True needs compose="device" (the "host" form keeps no pose but the last)')
    if compose == "device":
        return _refine_loop_device(refiner, pred, points_inp, int(iteration), graph, trajectory)
    f = refiner._fold()
    rot0, trans0, conf = pred["rot_pred"], pred["trans_pred"], pred["conf"]
    F_pm = pred["F_Xo_p"].transpose(1, 2)                                 # (b,n,256) (a view when fused)
    b, n, _ = F_pm.shape

    def feature_term(F_pm, out=None):
        # the feature half of the first shared layer: the same in every iteration, computed once per call
        bias, W = f["MLP_share"][0][1], f["share0_feat"]
        # point-major rows (what Network.forward hands over: dense from a graph replay, a 256-column block of the 512-wide fuser
        # input -- row pitch 512 -- launch by launch): one GEMM of the own core on the (b*n, 256) rows as they lie
        if F_pm.stride(2) == 1 and F_pm.stride(0) == n * F_pm.stride(1):
            rows = F_pm.as_strided((b * n, F_pm.shape[2]), (F_pm.stride(1), 1))
            return ops.linear(rows, W, bias, False, out=out)
        # channel-first features (the reference's own layout, (b, 256, n) storage): one transposing copy (33 MB at 32 crops, ~15 us)
        # and the same GEMM -- not torch.baddbmm on the transposed view: torch takes the vendor library's first-choice algorithm,
        # for some row counts a workspace-exchanging stream-K kernel that must never meet a second one on the GPU (csrc/linear.cpp)
        return ops.linear(F_pm.contiguous().view(b * n, -1), W, bias, False, out=out)

    def body(rot, trans, feat_term, conf, pts):
        conf_w = torch.softmax(conf.unsqueeze(1), dim=2)[:, 0, :1024].contiguous()
        for _ in range(iteration):
            cur = torch.bmm(pts - trans.unsqueeze(1), rot).reshape(b * n, 3)
            dt, dR = refiner.forward_pm(cur, feat_term, conf_w)
            trans = (rot @ dt.unsqueeze(2)).squeeze(2) + trans
            rot = rot @ dR
        return rot, trans

    with torch.no_grad():
        if not graph:
            return body(rot0, trans0, feature_term(F_pm), conf, points_inp)
        key = (b, n, iteration, conf.shape[1])
        cache = refiner.__dict__.setdefault("_graphs", {})
        if key not in cache:
            cc = lambda t: t.clone(memory_format=torch.contiguous_format)                     # noqa: E731
            static = [cc(rot0), cc(trans0), feature_term(F_pm), cc(conf), cc(points_inp)]
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                for _ in range(2):                                        # warm-up (allocator, lazy inits)
                    body(*static)
            torch.cuda.current_stream().wait_stream(s)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                out = body(*static)
            cache[key] = (g, static, out)
        g, static, out = cache[key]
        # the 256-channel features are not copied into the graph (33 MB at 32 crops): their GEMM runs in front of the replay and
        # writes the graph's static feature term; the small inputs are copied
        feature_term(F_pm, out=static[2])
        ops.pad_copy_many([(static[0].view(b, 9), rot0.reshape(b, 9)), (static[1], trans0.reshape(b, 3)),
                           (static[3], conf.reshape(b, -1)), (static[4].view(b * n, 3), points_inp.reshape(b * n, 3))])
        g.replay()
        rot, trans = torch.empty_like(out[0]), torch.empty_like(out[1])     # (the graph's own outputs are overwritten by the next replay)
        ops.pad_copy_many([(rot.view(b, 9), out[0].reshape(b, 9)), (trans, out[1].reshape(b, 3))])
        return rot, trans


def _refine_loop_device(refiner, pred, points_inp, iteration, graph, trajectory):
    """refine_loop(compose="device"): see there"""
    rot0, trans0, conf = pred["rot_pred"], pred["trans_pred"], pred["conf"]
    F_pm = pred["F_Xo_p"].transpose(1, 2)                                 # (b,n,256) (a view when fused)
    b, n, _ = F_pm.shape
    if n % ops.LINEAR_POOL_TILE:
        raise ValueError('compose="device" needs n %% %d == 0 (the pooling tile: a crop is a whole number of tile partials), '
                         'got n = %d' % (ops.LINEAR_POOL_TILE, n))
    if b > 65535:
        raise ValueError('compose="device" needs b <= 65535 crops (one grid row per crop), got b = %d' % b)
    if iteration < 0:
        raise ValueError("iteration must be >= 0, got %d" % iteration)
    if min(conf.shape[1], 1024) != n:
        raise ValueError('compose="device" needs one confidence per point: conf[:, :1024] has %d columns for n = %d'
                         % (min(conf.shape[1], 1024), n))
    f = refiner._fold()
    T = n // ops.LINEAR_POOL_TILE
    dev = F_pm.device

    def feature_term(out=None):
        # the feature half of the first shared layer, once per call (refine_loop: feature_term)
        bias, W = f["MLP_share"][0][1], f["share0_feat"]
        if F_pm.stride(2) == 1 and F_pm.stride(0) == n * F_pm.stride(1):
            rows = F_pm.as_strided((b * n, F_pm.shape[2]), (F_pm.stride(1), 1))
            return ops.linear(rows, W, bias, False, out=out)
        return ops.linear(F_pm.contiguous().view(b * n, -1), W, bias, False, out=out)

    def set_pose(rots, transs):
        ops.pad_copy_many([(rots[0].view(b, 9), rot0.reshape(b, 9)), (transs[0], trans0.reshape(b, 3))])

    def body(rots, transs, feat_term, conf, pts):
        conf_w = torch.softmax(conf.unsqueeze(1), dim=2)[:, 0, :1024].contiguous()
        for i in range(iteration):
            h = ops.refine_first(pts, rots[i], transs[i], f["share0_xyz"], feat_term)
            h = ops.linear(h, f["MLP_share"][1][0], f["MLP_share"][1][1], True)
            part = ops.linear_pool(h, f["MLP_share"][2][0], f["MLP_share"][2][1], conf_w.reshape(-1), relu=True)
            ops.refine_heads(part, T, f["regressor_rot2"], f["regressor_trans2"], rots[i], transs[i], rots[i + 1], transs[i + 1])

    def pose_arrays():
        return (torch.empty((iteration + 1, b, 3, 3), dtype=torch.float32, device=dev),
                torch.empty((iteration + 1, b, 3), dtype=torch.float32, device=dev))

    with torch.no_grad():
        if not graph:
            rots, transs = pose_arrays()
            set_pose(rots, transs)
            body(rots, transs, feature_term(), conf, ops.N.f32c(points_inp))
        else:
            key = (b, n, iteration, conf.shape[1], "device")
            cache = refiner.__dict__.setdefault("_graphs", {})
            if key not in cache:
                static = list(pose_arrays()) + [feature_term(), conf.clone(memory_format=torch.contiguous_format),
                                                ops.N.f32c(points_inp).clone()]
                set_pose(static[0], static[1])
                s = torch.cuda.Stream()
                s.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(s):
                    for _ in range(2):                                    # warm-up (allocator, lazy inits)
                        body(*static)
                torch.cuda.current_stream().wait_stream(s)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    body(*static)
                cache[key] = (g, static)
            g, static = cache[key]
            # as in the "host" form: the feature term's GEMM runs in front of the replay, the small inputs are copied in
            feature_term(out=static[2])
            ops.pad_copy_many([(static[0][0].view(b, 9), rot0.reshape(b, 9)), (static[1][0], trans0.reshape(b, 3)),
                               (static[3], conf.reshape(b, -1)), (static[4].view(b * n, 3), points_inp.reshape(b * n, 3))])
            g.replay()
            rots, transs = torch.empty_like(static[0]), torch.empty_like(static[1])  # (the graph's own arrays are overwritten by the next replay)
            rows = (iteration + 1) * b
            ops.pad_copy_many([(rots.view(rows, 9), static[0].view(rows, 9)), (transs.view(rows, 3), static[1].view(rows, 3))])
        if trajectory:
            return rots[-1], transs[-1], (rots, transs)
        return rots[-1], transs[-1]


def stage2_chain(model, refiner, data, iteration=2, graph=True, compose="host", trajectory=False):
    """BASELINE configs[4] as one call: the body of the reference's stage-2 eval loop (tools/test_YCBV_stage2.py:204-225):
    `model(data)` -> canonicalised points (P - t) R -> cat[points, F_Xo_p] -> `iteration` x refiner with pose composition
    t <- R dt + t, R <- R dR.  -> (rot (b,3,3), trans (b,3), stage-1 prediction dict).  With graph=True the refine loop
    replays its hipGraph (static shapes); the stage-1 forward keeps its own schedule (eager or forward_graphed).
    compose / trajectory: handed to refine_loop; with trajectory=True (compose="device") the pose after every iteration,
    (rots, transs), is returned as a fourth value."""
    with torch.no_grad():
        pred = model(data)
        points_inp = data["labels"]["points_inp"]
        out = refine_loop(refiner, pred, points_inp, iteration, graph=graph, compose=compose, trajectory=trajectory)
    return (out[0], out[1], pred) + tuple(out[2:])
