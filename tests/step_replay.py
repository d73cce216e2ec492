"""Helpers of the whole-step tests (tests/test_gpu_step_replay.py; no test functions here, and nothing that needs a GPU to
import): a recorder of every call of a set of torch.autograd.Function classes during one training step, the stand-alone replay
of a recorded call, the walk over a loss's autograd graph, and the all-kernels training step itself.

StepRecorder(classes, monkeypatch) replaces `apply` and `backward` on each class -- the engine looks `backward` up on the class
when the node runs, so setting the attribute is enough, and no product code changes.  Per call it keeps clones of the tensor
inputs as they were BEFORE the call (for BnReluFn these include the running statistics before their update), their
requires_grad, the other arguments, clones of the outputs, and, once the node has run, clones of the incoming gradients taken
before the backward and of the gradients it returned.  Three checks are the recorder's own:
  (a) right after a backward call its incoming gradients have the bits they had before it: nothing was written over them
      (autograd hands the same tensor to both sides of an add and through views);
  (b) when a backward call starts, every tensor input and every output of its forward call still has its forward-time bits:
      nothing a Function may have saved was changed behind the graph.  Inputs a call updates on purpose (`mutated`: the running
      statistics of BnReluFn) are compared with their value right after the call;
  (c) check_all_nodes_recorded(loss): the nodes of `classes` in loss's graph are exactly the recorded backward calls of the step.
      A condition, not a measurement: no custom node goes unrecorded.
A failed check raises ReplayError where it is found (inside loss.backward() for (a) and (b)).

replay(call) runs the call again, alone: fresh CONTIGUOUS clones of the recorded inputs with the recorded requires_grad (the
same tensor given twice stays the same tensor), Cls.apply, then torch.autograd.grad with contiguous clones of the recorded
incoming gradients; it returns the list of differences in bits between the recorded and the replayed outputs, updated
statistics and returned gradients (empty: the layout the network passed is the one the Function's own float64 tests verified)."""
import torch


class ReplayError(AssertionError):
    pass


def _is_t(v):
    return isinstance(v, torch.Tensor)


_INT_OF = {4: torch.int32, 8: torch.int64, 2: torch.int16, 1: torch.uint8}


def same_bits(a, b):
    """shape and bit pattern (NaNs and signed zeros included), compared where the tensors live; one read-back"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.numel() == 0:
        return True
    a, b = a.detach().contiguous(), b.detach().to(a.device).contiguous()
    if a.dtype.is_floating_point:
        a, b = a.view(_INT_OF[a.element_size()]), b.view(_INT_OF[b.element_size()])
    return bool(torch.equal(a, b))


def max_abs_diff(a, b):
    if a.shape != b.shape:
        return float("inf")
    return float((a.detach().double().cpu() - b.detach().double().cpu()).abs().max()) if a.numel() else 0.0


def _clone(v, contiguous=False):
    if not _is_t(v):
        return v
    return v.detach().clone(memory_format=torch.contiguous_format if contiguous else torch.preserve_format)


class Call(object):
    """one recorded Function call (see the module docstring)"""

    def __init__(self, cls, index, step, args):
        self.cls, self.index, self.step = cls, index, step
        self.args = args                                      # the live objects: identity (aliasing) and check (b)
        self.inputs = [_clone(a) for a in args]
        self.requires_grad = [_is_t(a) and a.requires_grad for a in args]
        self.expect = list(self.inputs)                       # what check (b) wants of the live inputs
        self.live_outputs = self.outputs = self.node = None
        self.single = False
        self.grads_in = self.grads_out = None

    @property
    def name(self):
        return self.cls.__name__

    @property
    def rows(self):
        """the rows of the call's first tensor input (the call 'with the most rows' of a class)"""
        for a in self.inputs:
            if _is_t(a):
                return int(a.shape[0]) if a.dim() < 3 else int(a.shape[0] * a.shape[1])
        return 0

    def __repr__(self):
        shapes = [tuple(a.shape) if _is_t(a) else a for a in self.inputs]
        return "<step %d call %d %s %s>" % (self.step, self.index, self.name, shapes)


class StepRecorder(object):
    def __init__(self, classes, monkeypatch, mutated=None):
        self.classes = tuple(classes)
        self.mutated = dict(mutated or {})                    # class name -> argument positions the call updates on purpose
        self.calls, self.by_node = [], {}
        self.step, self.active, self._sink = 0, True, None
        self._apply = {}
        for cls in self.classes:
            self._apply[cls] = cls.apply
            monkeypatch.setattr(cls, "apply", staticmethod(self._wrap_apply(cls, cls.apply)))
            monkeypatch.setattr(cls, "backward", staticmethod(self._wrap_backward(cls, cls.backward)))

    # ------------------------------------------------------------------ recording
    def begin_step(self):
        self.step += 1

    def _wrap_apply(self, cls, apply):
        def recorded_apply(*args):
            if not self.active:
                return apply(*args)
            sink = self.calls if self._sink is None else self._sink
            call = Call(cls, len(sink), self.step, args)
            out = apply(*args)
            outs = (out,) if _is_t(out) else tuple(out)
            call.single = _is_t(out)
            call.live_outputs = outs
            call.outputs = [_clone(o) for o in outs]
            for i in self.mutated.get(cls.__name__, ()):
                call.expect[i] = _clone(args[i])
            nodes = [o.grad_fn for o in outs if _is_t(o) and o.grad_fn is not None]
            if nodes:
                call.node = nodes[0]
                self.by_node[id(call.node)] = call
            sink.append(call)
            return out
        return recorded_apply

    def _wrap_backward(self, cls, backward):
        def recorded_backward(ctx, *grads):
            call = self.by_node.get(id(ctx)) if self.active else None
            if call is None or call.node is not ctx:
                return backward(ctx, *grads)
            before = [_clone(g) for g in grads]
            for what, live, want in (("input", call.args, call.expect), ("output", call.live_outputs, call.outputs)):
                for i, (t, w) in enumerate(zip(live, want)):
                    if _is_t(t) and not same_bits(t, w):
                        raise ReplayError("(b) %s %d of %r no longer has its forward-time bits when its backward starts "
                                          "(max |diff| %.3g)" % (what, i, call, max_abs_diff(t, w)))
            res = backward(ctx, *grads)
            for i, (g, w) in enumerate(zip(grads, before)):
                if _is_t(g) and not same_bits(g, w):
                    raise ReplayError("(a) the backward of %r wrote over its incoming gradient %d (max |diff| %.3g)"
                                      % (call, i, max_abs_diff(g, w)))
            if call.grads_in is not None:
                raise ReplayError("the backward of %r ran twice" % (call,))
            call.grads_in = before
            call.grads_out = [_clone(g) for g in (res if isinstance(res, tuple) else (res,))]
            return res
        return recorded_backward

    # ------------------------------------------------------------------ the graph
    def custom_nodes(self, root):
        """the nodes of the recorder's classes in the autograd graph of `root` (a tensor)"""
        seen, stack, found = {}, [root.grad_fn], []          # seen holds the nodes: a freed wrapper's id would be reused
        while stack:
            node = stack.pop()
            if node is None or id(node) in seen:
                continue
            seen[id(node)] = node
            if getattr(type(node), "_forward_cls", None) in self.classes:
                found.append(node)
            stack.extend(fn for fn, _ in node.next_functions)
        return found

    def count_custom_nodes(self, root):
        return len(self.custom_nodes(root))

    def check_all_nodes_recorded(self, root, step=None):
        """condition (c), after root's backward has run"""
        step = self.step if step is None else step
        nodes = self.custom_nodes(root)
        ran = [c for c in self.calls if c.step == step and c.grads_in is not None]
        missing = [type(n).__name__ for n in nodes if id(n) not in self.by_node or self.by_node[id(n)].node is not n
                   or self.by_node[id(n)].grads_in is None]
        if missing or len(nodes) != len(ran):
            raise ReplayError("(c) the graph holds %d custom nodes, %d backward calls were recorded in step %d; unrecorded: %s"
                              % (len(nodes), len(ran), step, missing))
        return len(nodes)

    def counts(self, step=None):
        out = {}
        for c in self.calls:
            if step is None or c.step == step:
                out[c.name] = out.get(c.name, 0) + 1
        return out

    # ------------------------------------------------------------------ the replay
    def replay(self, call, report=None):
        """-> the differences in bits as a list of strings; report (a list) receives (what, max |diff|, max |recorded|) of
        every compared tensor"""
        fresh, args = {}, []
        for i, a in enumerate(call.args):
            if not _is_t(a):
                args.append(a)
                continue
            if id(a) not in fresh:
                fresh[id(a)] = _clone(call.inputs[i], contiguous=True).requires_grad_(call.requires_grad[i])
            args.append(fresh[id(a)])
        bad = []

        def cmp(what, got, want):
            if (got is None) != (want is None):
                bad.append("%s: %s against recorded %s" % (what, "None" if got is None else "a tensor", "None" if want is None
                                                            else "a tensor"))
            elif got is not None:
                if report is not None:
                    report.append((what, max_abs_diff(got, want), float(want.abs().max()) if want.numel() else 0.0))
                if not same_bits(got, want):
                    bad.append("%s: max |diff| %.3g" % (what, max_abs_diff(got, want)))
        sink, old = [], self._sink
        self._sink = sink
        try:
            out = call.cls.apply(*args)
            outs = (out,) if _is_t(out) else tuple(out)
            again = sink[0]
            for i, (o, w) in enumerate(zip(outs, call.outputs)):
                cmp("output %d" % i, o, w)
            for i in self.mutated.get(call.name, ()):
                cmp("updated input %d" % i, args[i], call.expect[i])
            if call.grads_in is not None:
                pairs = [(o, _clone(g, contiguous=True)) for o, g in zip(outs, call.grads_in) if g is not None]
                leaves = [t for t in fresh.values() if t.requires_grad]
                torch.autograd.grad([o for o, _ in pairs], leaves, [g for _, g in pairs], allow_unused=True)
                if again.grads_out is None:
                    bad.append("the replayed backward did not run")
                else:
                    for i, (g, w) in enumerate(zip(again.grads_out, call.grads_out)):
                        cmp("gradient %d" % i, g, w)
        finally:
            self._sink = old
            for c in sink:
                if c.node is not None:
                    self.by_node.pop(id(c.node), None)
        return bad


# ---------------------------------------------------------------------------------------------------- the step under test
SHIPPED_ADAM = dict(lr=1e-3, betas=(0.5, 0.999), eps=1e-6)     # the stage-1 training script's optimizer (tests/test_gpu_optim.py)
MUTATED = {"BnReluFn": (3, 4)}                                 # running_mean, running_var: updated by the forward launches


def function_classes(autograd_module):
    """every torch.autograd.Function class a module defines, in definition order"""
    out = [v for v in vars(autograd_module).values() if isinstance(v, type) and issubclass(v, torch.autograd.Function)
           and v is not torch.autograd.Function and v.__module__ == autograd_module.__name__]
    return out


def make_net(dcl, n, **switches):
    net = dcl.DCL_Net.Network(dcl.synth.default_cfg(n, n), mode="train", graph_max_batch=0, **switches)
    net.load_state_dict(dcl.synth.synth_state_dict(net, 1))
    return net.cuda().train()


def make_data(dcl, b, n):
    data = dcl.synth.make_batch(b, n, n)
    data["flags"] = torch.tensor([float(i % 2) for i in range(b)])
    return data


def run_steps(dcl, b, n, steps=2, rec=None, switches=None, fused_losses=True, on_loss=None):
    """`steps` consecutive training steps of a fresh network from the same initial state, seed and batch: AutoClip + Adam with
    the shipped settings step in between.  -> (net, per step: dict(loss, pred {name: tensor}, grads {name: tensor}), all
    detached clones).  rec: a StepRecorder that records each step and has conditions (c) checked; on_loss(step, loss, net) runs
    between the forward and the backward."""
    torch.manual_seed(0)
    net = make_net(dcl, n, **(dcl.DCL_Net.TRAIN_KERNELS if switches is None else switches))
    crit = dcl.DCL_Net.losses(None, chamfer="fused", objective="fused") if fused_losses else dcl.DCL_Net.losses(None)
    opt = dcl.optim.Adam(net.parameters(), **SHIPPED_ADAM)
    clip = dcl.optim.AutoClip(50, optimizer=opt)
    data = make_data(dcl, b, n)
    out = []
    for s in range(steps):
        if rec is not None:
            rec.begin_step()
        opt.zero_grad()
        pred = net(data)
        loss = crit(pred, data["labels"])["loss_all"]
        if on_loss is not None:
            on_loss(s, loss, net)
        loss.backward()
        if rec is not None:
            rec.check_all_nodes_recorded(loss)
        out.append(dict(loss=loss.detach().clone(),
                        pred={k: v.detach().clone() for k, v in pred.items() if _is_t(v)},
                        grads={k: (None if p.grad is None else p.grad.detach().clone()) for k, p in net.named_parameters()}))
        clip(net)
        opt.step()
    torch.cuda.synchronize()
    return net, out


# ---------------------------------------------------------------------------------------------------- the census
ARITHMETIC_FAMILIES = ("Convolution", "Addmm", "Mm", "Bmm", "Mv", "Baddbmm", "Linear", "NativeBatchNorm", "CudnnBatchNorm",
                       "MiopenBatchNorm", "Softmax", "LogSoftmax", "NativeLayerNorm", "Einsum")


def torch_nodes(root):
    """{node type name: count} over the torch-native (not custom Function) nodes of root's autograd graph"""
    seen, stack, found = {}, [root.grad_fn], {}              # seen holds the nodes: a freed wrapper's id would be reused
    while stack:
        node = stack.pop()
        if node is None or id(node) in seen:
            continue
        seen[id(node)] = node
        if getattr(type(node), "_forward_cls", None) is None:
            name = type(node).__name__
            found[name] = found.get(name, 0) + 1
        stack.extend(fn for fn, _ in node.next_functions)
    return found


def arithmetic_nodes(root):
    """the torch-native node types of root's graph that do arithmetic on activations in a vendor or torch kernel of the
    convolution, matrix-product, batch-norm or softmax families (name = family + 'Backward' + a digit)"""
    out = set()
    for name in torch_nodes(root):
        base = name.split("Backward")[0]
        if base in ARITHMETIC_FAMILIES:
            out.add(name)
    return out
