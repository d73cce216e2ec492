"""The tail of a training step on the library's own kernels (csrc/optim.hip): AutoClip's gradient norm and the Adam update.

The reference (tools/train_YCBV_stage1.py:119-125, 212-231, the same in train_YCBV_stage2.py) runs, after loss.backward(),

    AutoClip(50)(model)          one norm kernel and one blocking .item() PER PARAMETER TENSOR (156 in Network), np.percentile
                                 over the history of norms, then clip_grad_norm_: every norm again and a multiply per gradient
    Adam(betas=(0.5, 0.999), eps=1e-6).step()

Here the same three lines of a training script,

    clipper = dcl.optim.AutoClip(50, optimizer=opt)          # opt = dcl.optim.Adam(model.parameters(), ...)
    clipper(model)
    opt.step()

are one norm pass over all gradients (two launches), ONE 8-byte read-back (the clip value is a percentile over a host-side
history that includes this step) and one update launch per parameter group, the clip factor multiplied in on the way
(p.grad itself is not rewritten: DESIGN.md section 9).  dcl.optim.DeviceAutoClip(50, optimizer=opt) in AutoClip's place
keeps that history sorted on the GPU and takes the percentile there: no read-back at all, and a cost that does not grow
with the length of the run.  The kernels are driven by two small device tables
(include/dclnet_hip.h at dclOptimTensor) that are packed on the host every step and uploaded with one asynchronous copy
from pinned memory; there is no CPU fallback."""
import numpy as np
import torch

from . import ops

CHUNK = ops.OPTIM_CHUNK
# dclOptimTensor, field for field
TENSOR_DTYPE = np.dtype([("param", "<u8"), ("grad", "<u8"), ("exp_avg", "<u8"), ("exp_avg_sq", "<u8"), ("numel", "<i8"),
                         ("step_size", "<f4"), ("bc2_sqrt", "<f4")])
assert TENSOR_DTYPE.itemsize == ops.OPTIM_TENSOR_BYTES


def chunk_table(numels):
    """numels of the listed tensors -> (chunk_tensor i32, chunk_begin i64): every tensor cut into runs of CHUNK elements,
    the chunks of a tensor consecutive and ascending"""
    numels = np.asarray(numels, dtype=np.int64)
    counts = (numels + CHUNK - 1) // CHUNK
    first = np.cumsum(counts) - counts
    chunk_tensor = np.repeat(np.arange(len(numels), dtype=np.int32), counts)
    chunk_begin = (np.arange(int(counts.sum()), dtype=np.int64) - np.repeat(first, counts)) * CHUNK
    return chunk_tensor, chunk_begin


def bias_corrections(lr, beta1, beta2, t):
    """(step_size, bc2_sqrt) of a tensor at its t-th update (t = 1, 2, ..; array or scalar): evaluated in double, rounded
    once to fp32"""
    t = np.asarray(t, dtype=np.float64)
    step_size = np.float64(lr) / (1.0 - np.float64(beta1) ** t)
    bc2_sqrt = np.sqrt(1.0 - np.float64(beta2) ** t)
    return step_size.astype(np.float32), bc2_sqrt.astype(np.float32)


def _pad16(n):
    return (n + 15) & ~15


class _Layout(object):
    """Byte layout of one packed upload: [tensor table | chunk_tensor | chunk_begin | chunk_tensor relative to its group],
    every section 16-byte aligned.  groups = [(first tensor, tensors, first chunk, chunks)] of the parameter groups that list
    a tensor; the last section exists only where there is more than one (a group's launch indexes its own slice of the
    tensor table)."""

    def __init__(self, numels, group_sizes):
        self.n_tensors = len(numels)
        chunk_tensor, chunk_begin = chunk_table(numels)
        self.n_chunks = len(chunk_tensor)
        self.groups = []
        t0 = 0
        for n in group_sizes:
            if n:
                c0, c1 = np.searchsorted(chunk_tensor, [t0, t0 + n])
                self.groups.append((t0, n, int(c0), int(c1 - c0)))
            t0 += n
        self.off_ct = _pad16(self.n_tensors * TENSOR_DTYPE.itemsize)
        self.off_cb = self.off_ct + _pad16(4 * self.n_chunks)
        self.off_rel = self.off_cb + _pad16(8 * self.n_chunks)
        self.nbytes = self.off_rel + (_pad16(4 * self.n_chunks) if len(self.groups) > 1 else 0)
        self.template = np.zeros(self.nbytes, dtype=np.uint8)
        self.template[self.off_ct:self.off_ct + 4 * self.n_chunks] = chunk_tensor.view(np.uint8)
        self.template[self.off_cb:self.off_cb + 8 * self.n_chunks] = chunk_begin.view(np.uint8)
        if len(self.groups) > 1:
            rel = chunk_tensor.copy()
            for t0, _, c0, nc in self.groups:
                rel[c0:c0 + nc] -= t0
            self.template[self.off_rel:self.off_rel + 4 * self.n_chunks] = rel.view(np.uint8)

    def views(self, dev, first_tensor=0, tensors=None, first_chunk=0, chunks=None):
        """(table, chunk_tensor, chunk_begin) views of an uploaded buffer: all tensors, or one group's slice"""
        whole = tensors is None
        tensors = self.n_tensors if whole else tensors
        chunks = self.n_chunks if whole else chunks
        b = TENSOR_DTYPE.itemsize
        table = dev[first_tensor * b:(first_tensor + tensors) * b]
        ct0 = (self.off_ct if whole or len(self.groups) == 1 else self.off_rel) + 4 * first_chunk
        chunk_tensor = dev[ct0:ct0 + 4 * chunks].view(torch.int32)
        cb0 = self.off_cb + 8 * first_chunk
        chunk_begin = dev[cb0:cb0 + 8 * chunks].view(torch.int64)
        return table, chunk_tensor, chunk_begin


class _TableRing(object):
    """Pinned staging buffers and their device copies, used in turn.  A slot is rewritten only after the event recorded
    behind the last launch that read it has completed, so neither the pinned bytes an asynchronous copy may still be reading
    nor the device table a queued kernel may still be reading are ever overwritten -- and with several slots that wait is
    over long before it is asked for."""
    SLOTS = 4

    class Slot(object):
        def __init__(self):
            self.pinned = self.dev = self.event = None

    def __init__(self, device):
        self.device = device
        self.slots = [self.Slot() for _ in range(self.SLOTS)]
        self.turn = 0

    def upload(self, host):
        slot = self.slots[self.turn]
        self.turn = (self.turn + 1) % self.SLOTS
        if slot.event is not None:
            slot.event.synchronize()
        n = host.size
        if slot.pinned is None or slot.pinned.numel() < n:
            cap = max(4096, 2 * n)
            slot.pinned = torch.empty(cap, dtype=torch.uint8).pin_memory()
            slot.dev = torch.empty(cap, dtype=torch.uint8, device=self.device)
            slot.event = torch.cuda.Event()
        slot.pinned.numpy()[:n] = host
        with torch.cuda.device(self.device):
            slot.dev[:n].copy_(slot.pinned[:n], non_blocking=True)
        return slot

    @staticmethod
    def used(slot):
        """call behind every launch that reads the slot's device table"""
        slot.event.record(torch.cuda.current_stream(slot.dev.device))


def _check_grad(p):
    g = p.grad
    if g.is_sparse:
        raise RuntimeError("dcl.optim: sparse gradients are not supported (a parameter of shape %s has one)" % (tuple(p.shape),))
    if g.dtype != torch.float32 or not g.is_contiguous() or g.device != p.device or g.shape != p.shape:
        raise RuntimeError("dcl.optim: a gradient must be a contiguous fp32 tensor on its parameter's GPU (got %s, %s, "
                           "contiguous=%s for a parameter of shape %s)" % (g.dtype, g.device, g.is_contiguous(), tuple(p.shape)))
    return g


class _Plan(object):
    """one packed and uploaded set of tables, and what it was packed from"""

    def __init__(self, layout, signature, slot, params, hyper):
        self.layout, self.signature, self.slot, self.params, self.hyper = layout, signature, slot, params, hyper


class Adam(torch.optim.Optimizer):
    """torch.optim.Adam (no weight decay, no amsgrad, no maximize) for fp32 GPU parameters, every parameter tensor of a group
    updated by ONE launch of dcl_adam_step.  A drop-in: lr schedulers (CyclicLR(..., cycle_momentum=False)), zero_grad,
    parameter groups and checkpoint savers work unchanged, state_dict() loads into torch.optim.Adam and torch's loads here.
    state[p] = {"step" (CPU fp32 scalar tensor, as torch's default implementation keeps it), "exp_avg", "exp_avg_sq"}, made
    at a parameter's first step; the two moments are views into one flat device buffer each, the step counts views into one
    flat host tensor.

    Per element the update runs the five fp32 lines documented at dcl_adam_step in include/dclnet_hip.h, with the bias
    corrections evaluated in double on the host from every tensor's own step count.  The kernel writes through raw pointers,
    so step() moves the version counters of what it updated (torch.autograd.graph.increment_version): caches keyed on them
    -- Network._fold, Refiner._fold and the captured graphs behind them -- follow the new weights."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, maximize=False):
        if not 0.0 <= lr:
            raise ValueError("invalid learning rate: %r" % (lr,))
        if not 0.0 < eps:
            raise ValueError("invalid eps: %r (must be > 0)" % (eps,))
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError("invalid betas: %r" % (betas,))
        # every key torch.optim.Adam's groups carry, so that a state dict moves between the two classes either way
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize,
                        foreach=None, capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False)
        self._flat = None
        super().__init__(params, defaults)
        ps = [p for g in self.param_groups for p in g["params"]]
        dev = ps[0].device
        if any(p.device != dev for p in ps):
            raise RuntimeError("dcl.optim.Adam: all parameters must live on one GPU")
        # the moments of all parameters in one flat buffer each; every tensor starts on a 16-byte boundary
        self._slot_of, total = {}, 0
        for i, p in enumerate(ps):
            self._slot_of[p] = (i, total)
            total += (p.numel() + 3) & ~3
        self._flat = self._new_flat(total, dev)
        self._steps = torch.zeros(len(ps), dtype=torch.float32)
        self._ring = _TableRing(dev)
        self._layouts = {}
        self._pending = None          # tables a clipper has already uploaded for the coming step
        self._grad_scale = 1.0        # handed over by AutoClip for the next step() only (DeviceAutoClip: a device fp32)

    @staticmethod
    def _new_flat(total, dev):
        return (torch.zeros(total, dtype=torch.float32, device=dev), torch.zeros(total, dtype=torch.float32, device=dev))

    @staticmethod
    def _check_group(group):
        if group["weight_decay"] != 0 or group["amsgrad"] or group["maximize"]:
            raise ValueError("dcl.optim.Adam implements plain Adam: weight_decay != 0, amsgrad and maximize are not supported "
                             "(got weight_decay=%r, amsgrad=%r, maximize=%r)"
                             % (group["weight_decay"], group["amsgrad"], group["maximize"]))

    def add_param_group(self, param_group):
        if self._flat is not None:
            raise RuntimeError("dcl.optim.Adam: parameter groups are fixed at construction (the moments live in one flat buffer)")
        super().add_param_group(param_group)
        group = self.param_groups[-1]
        self._check_group(group)
        for p in group["params"]:
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise TypeError("dcl.optim.Adam: parameters must be contiguous float32 tensors (got %s, contiguous=%s, shape %s)"
                                % (p.dtype, p.is_contiguous(), tuple(p.shape)))
            if not p.is_cuda:
                raise RuntimeError("dcl.optim.Adam runs on the GPU only (got a parameter on %s); no CPU fallback" % p.device)

    def _state_views(self, p, flat=None):
        """(step, exp_avg, exp_avg_sq) of p: views into the flat step tensor and the two flat moment buffers"""
        flat = self._flat if flat is None else flat
        (i, o), n = self._slot_of[p], p.numel()
        return self._steps[i], flat[0][o:o + n].view_as(p), flat[1][o:o + n].view_as(p)

    def _layout_for(self, params, group_sizes):
        """the layout of this set of tensors, with everything that does not change from step to step filled in; makes the
        state of a parameter that steps for the first time"""
        key = tuple(map(id, params))
        layout = self._layouts.get(key)
        if layout is None:
            self._layouts.clear()
            layout = self._layouts[key] = _Layout([p.numel() for p in params], group_sizes)
            tab = layout.template[:layout.n_tensors * TENSOR_DTYPE.itemsize].view(TENSOR_DTYPE)
            for j, p in enumerate(params):
                st = self.state[p]
                if len(st) == 0:
                    st["step"], st["exp_avg"], st["exp_avg_sq"] = self._state_views(p)     # zero since construction / the last load
                tab["exp_avg"][j], tab["exp_avg_sq"][j] = st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()
                tab["numel"][j] = p.numel()
            layout.step_index = np.array([self._slot_of[p][0] for p in params], dtype=np.int64)
        return layout

    def _prepare(self):
        """pack the tables of the coming step and upload them -- or keep the upload a clipper made a moment ago, when
        nothing it was packed from has changed since"""
        params, grads, group_sizes, hyper = [], [], [], []
        for group in self.param_groups:
            self._check_group(group)
            before = len(params)
            for p in group["params"]:
                g = p.grad
                if g is not None and p.numel() > 0:
                    params.append(p)
                    grads.append(g)
            group_sizes.append(len(params) - before)
            if group_sizes[-1]:
                beta1, beta2 = group["betas"]
                hyper.append((float(group["lr"]), float(beta1), float(beta2), float(group["eps"])))
        if not params:
            return None
        grad_ptrs, param_ptrs = [g.data_ptr() for g in grads], [p.data_ptr() for p in params]
        signature = (tuple(map(id, params)), grad_ptrs, param_ptrs, hyper)
        pend = self._pending
        if pend is not None and pend.signature == signature:       # (the step counts move only in step(), which drops it)
            return pend
        for p in params:
            _check_grad(p)
        layout = self._layout_for(params, group_sizes)
        host = layout.template.copy()
        tab = host[:layout.n_tensors * TENSOR_DTYPE.itemsize].view(TENSOR_DTYPE)
        tab["param"], tab["grad"] = param_ptrs, grad_ptrs
        t = self._steps.numpy()[layout.step_index].astype(np.float64) + 1.0
        for (t0, n, _, _), (lr, beta1, beta2, _) in zip(layout.groups, hyper):
            tab["step_size"][t0:t0 + n], tab["bc2_sqrt"][t0:t0 + n] = bias_corrections(lr, beta1, beta2, t[t0:t0 + n])
        self._pending = _Plan(layout, signature, self._ring.upload(host), params, hyper)
        return self._pending

    def grad_norm(self):
        """(sq_per_tensor, norm): float64 device tensors -- the squared 2-norm of every gradient this step, in the order the
        parameter groups list them (parameters without a gradient left out), and the 2-norm of all of them together.  No host
        read-back.  The tables stay uploaded for the step() that follows."""
        plan = self._prepare()
        if plan is None:
            dev = self._flat[0].device
            return torch.zeros(0, dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.float64, device=dev)
        out = ops.grad_sqnorm(*plan.layout.views(plan.slot.dev))
        _TableRing.used(plan.slot)
        return out

    def set_grad_scale(self, scale):
        """multiply the gradients by `scale` inside the NEXT step() only (what AutoClip hands over).  A float goes to the
        kernel as an argument; a one-element fp32 CUDA tensor (what DeviceAutoClip hands over) is read by the kernel when it
        runs (dcl_adam_step_dev), so the host never sees the value."""
        if isinstance(scale, torch.Tensor):
            if not scale.is_cuda or scale.dtype != torch.float32 or scale.numel() != 1 or scale.device != self._flat[0].device:
                raise TypeError("dcl.optim.Adam.set_grad_scale: a tensor factor must be one fp32 element on the parameters' GPU "
                                "(got %s, %s, %d elements)" % (scale.dtype, scale.device, scale.numel()))
            self._grad_scale = scale
        else:
            self._grad_scale = float(scale)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        plan = self._prepare()
        scale, self._grad_scale = self._grad_scale, 1.0
        self._pending = None
        if plan is None:
            return loss
        update = ops.adam_step_dev if isinstance(scale, torch.Tensor) else ops.adam_step
        for (t0, n, c0, nc), (_, beta1, beta2, eps) in zip(plan.layout.groups, plan.hyper):
            update(*plan.layout.views(plan.slot.dev, t0, n, c0, nc), scale, beta1, beta2, eps)
        _TableRing.used(plan.slot)
        self._steps.numpy()[plan.layout.step_index] += 1.0           # state[p]["step"] are views of it
        # the kernel wrote through raw pointers: tell autograd (and every cache keyed on _version) that these tensors changed
        torch.autograd.graph.increment_version(plan.params)
        return loss

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        ours = self.defaults
        for group in self.param_groups:
            self._check_group(group)
            # a dict saved by torch.optim.Adam(fused=True / capturable=True) carries its implementation switches: not ours
            for k in ("foreach", "capturable", "differentiable", "fused", "decoupled_weight_decay"):
                group[k] = ours[k]
        # what was loaded goes into fresh flat buffers (it may be views of the present ones) and the state points at them
        flat = self._new_flat(self._flat[0].numel(), self._flat[0].device)
        steps = torch.zeros_like(self._steps)
        loaded = [(p, st) for p, st in self.state.items() if len(st)]
        for p, st in loaded:
            if "max_exp_avg_sq" in st:
                raise ValueError("dcl.optim.Adam: the loaded state was saved with amsgrad=True, which is not supported")
            steps[self._slot_of[p][0]] = float(st["step"])
        self._steps = steps
        for p, st in loaded:
            step, m, v = self._state_views(p, flat)
            m.copy_(st["exp_avg"])
            v.copy_(st["exp_avg_sq"])
            st["step"], st["exp_avg"], st["exp_avg_sq"] = step, m, v
        self._flat = flat
        self._layouts.clear()
        self._pending = None
        self._grad_scale = 1.0


class AutoClip(object):
    """The reference's AutoClip (tools/train_YCBV_stage1.py:212-231; Seetharaman et al., 2020): clip the global gradient norm
    to the `percentile`-th percentile of the norms seen so far, this step's included.  Called as the reference calls it,
    `clipper(model)` in front of `optimizer.step()`.

    optimizer=a dcl.optim.Adam: one norm pass over the optimizer's tables, one 8-byte read-back, and the factor is handed to
      the optimizer's next step(), which multiplies it in on the way (p.grad is NOT rewritten; `model` is not looked at: the
      optimizer's parameters are what is clipped).
    optimizer=None: the same measurement over model.parameters(), and the gradients are scaled in place.

    The norm is the float64 2-norm of all gradients (the reference adds squares of per-tensor fp32 norms, ~1e-5 relative
    away).  `history` is the public list of norms; state_dict() / load_state_dict() carry it.  A non-finite norm is not
    special-cased, as in the reference."""

    def __init__(self, percentile=50, optimizer=None):
        if optimizer is not None and not isinstance(optimizer, Adam):
            raise TypeError("AutoClip(optimizer=...) takes a dcl.optim.Adam (got %s)" % type(optimizer).__name__)
        self.percentile = percentile
        self.optimizer = optimizer
        self.history = []
        self.clip_value = None        # of the latest call
        self._ring = None

    def observe(self, norm):
        """the host arithmetic of one call: append `norm`, take the percentile, return the factor for this step's gradients"""
        norm = float(norm)
        self.history.append(norm)
        self.clip_value = float(np.percentile(self.history, self.percentile))
        return min(1.0, self.clip_value / (norm + 1e-6))

    def _norm_of(self, grads):
        """device (1,) float64 norm of a list of gradients, measured as the optimizer form measures"""
        dev = grads[0].device
        if self._ring is None or self._ring.device != dev:
            self._ring = _TableRing(dev)
        layout = _Layout([g.numel() for g in grads], [len(grads)])
        host = layout.template.copy()
        tab = host[:layout.n_tensors * TENSOR_DTYPE.itemsize].view(TENSOR_DTYPE)
        tab["grad"] = [g.data_ptr() for g in grads]
        tab["numel"] = [g.numel() for g in grads]
        slot = self._ring.upload(host)
        _, norm = ops.grad_sqnorm(*layout.views(slot.dev))
        _TableRing.used(slot)
        return norm

    def __call__(self, model=None):
        if self.optimizer is not None:
            _, norm = self.optimizer.grad_norm()
            scale = self.observe(norm.item())                      # the one read-back of the step
            self.optimizer.set_grad_scale(scale)
            return
        ps = [p for p in model.parameters() if p.grad is not None and p.numel() > 0]
        if not ps:
            return
        grads = [_check_grad(p) for p in ps]
        if not grads[0].is_cuda:
            raise RuntimeError("dcl.optim.AutoClip measures on the GPU only (got gradients on %s); no CPU fallback" % grads[0].device)
        scale = self.observe(self._norm_of(grads).item())
        torch._foreach_mul_(grads, scale)

    def state_dict(self):
        return {"percentile": self.percentile, "history": list(self.history)}

    def load_state_dict(self, sd):
        self.percentile = sd["percentile"]
        self.history = [float(x) for x in sd["history"]]


class DeviceAutoClip(object):
    """AutoClip(percentile, optimizer=a dcl.optim.Adam) with the history on the GPU (csrc/optim.hip: dcl_autoclip_observe), as
    sharding.DeviceAddsTable is of AddsTable: the norms seen so far are kept SORTED in device memory, `clipper(model)` inserts
    this step's norm there, evaluates np.percentile and the factor on the device (the arithmetic is pinned line by line in
    include/dclnet_hip.h) and hands the optimizer a POINTER to the factor, which the next step()'s kernels read.  No
    read-back, so the host goes on issuing the next step; and the cost does not grow with the run as np.percentile over a
    Python list does.  Same norm kernel, same fp32 factor: the parameters have AutoClip's bits.

    A call is the optimizer's norm pass and two launches on the current stream -- the one the optimizer launches on; nothing
    is allocated after construction except at growth: when the `capacity` entries are used up the buffers double by device
    copies (the host counts its own calls, so it knows when without asking the device).  `model` is not looked at: the
    optimizer's parameters are what is clipped.  The model-only form is AutoClip's.

    history (arrival order), clip_value and scale (of the latest call; None before it) each READ BACK: for logging and
    checkpoints, not for the loop.  state_dict() / load_state_dict() carry AutoClip's keys, and a dict moves between the
    two classes either way; loading sorts once on the host.  A norm with the sign bit set (-0.0 included) is refused there:
    the order of the device history is defined for norms (>= +0, +inf, NaN; NaN last)."""

    def __init__(self, percentile=50, optimizer=None, capacity=4096):
        if not isinstance(optimizer, Adam):
            raise TypeError("DeviceAutoClip(optimizer=...) takes a dcl.optim.Adam (got %s); the model-only form is AutoClip's"
                            % type(optimizer).__name__)
        if not 0 <= percentile <= 100:
            raise ValueError("DeviceAutoClip: percentile must be in [0, 100] (got %r)" % (percentile,))
        if int(capacity) < 1:
            raise ValueError("DeviceAutoClip: capacity must be >= 1 (got %r)" % (capacity,))
        self.percentile = percentile
        self.optimizer = optimizer
        self.device = optimizer._flat[0].device
        self._n = 0
        self._observed = False        # whether _out holds a call's results
        self._out = torch.zeros(ops.AUTOCLIP_OUT_DOUBLES, dtype=torch.float64, device=self.device)
        self._scale32 = self._out.view(torch.float32)[ops.AUTOCLIP_SCALE_F32_INDEX:ops.AUTOCLIP_SCALE_F32_INDEX + 1]
        self._allocate(int(capacity))

    def _allocate(self, capacity):
        """fresh buffers of `capacity` entries: the sorted history ([0] holds it, [1] takes the next insertion) and the arrivals"""
        self.capacity = capacity
        self._sorted = [torch.empty(capacity, dtype=torch.float64, device=self.device) for _ in range(2)]
        self._arrival = torch.empty(capacity, dtype=torch.float64, device=self.device)

    def _grow(self):
        n, src, arrival = self._n, self._sorted[0], self._arrival
        self._allocate(2 * self.capacity)
        self._sorted[0][:n].copy_(src[:n])                # device to device, on the stream of the launches around them
        self._arrival[:n].copy_(arrival[:n])              # (the third buffer is the next insertion's destination: all written)

    def __len__(self):
        return self._n

    def __call__(self, model=None):
        _, norm = self.optimizer.grad_norm()
        if self._n == self.capacity:
            self._grow()
        src, dst = self._sorted
        ops.autoclip_observe(self._n, src, dst, self._arrival, norm, self.percentile, self._out)
        self._sorted = [dst, src]
        self._n += 1
        self._observed = True
        self.optimizer.set_grad_scale(self._scale32)

    @property
    def history(self):
        """the norms in arrival order, as AutoClip.history (a read-back of the whole history)"""
        return self._arrival[:self._n].cpu().tolist()

    @property
    def clip_value(self):
        """of the latest call (a read-back); None before it"""
        return float(self._out[1].cpu()) if self._observed else None

    @property
    def scale(self):
        """the factor of the latest call, in double (a read-back); None before it"""
        return float(self._out[2].cpu()) if self._observed else None

    def state_dict(self):
        return {"percentile": self.percentile, "history": self.history}

    def load_state_dict(self, sd):
        history = np.array([float(x) for x in sd["history"]], dtype=np.float64)
        if np.signbit(history).any():
            raise ValueError("DeviceAutoClip.load_state_dict: entry %d of the history has its sign bit set (%r): not a norm"
                             % (int(np.flatnonzero(np.signbit(history))[0]), float(history[np.signbit(history)][0])))
        if not 0 <= sd["percentile"] <= 100:
            raise ValueError("DeviceAutoClip: percentile must be in [0, 100] (got %r)" % (sd["percentile"],))
        self.percentile = sd["percentile"]
        n = history.size
        capacity = self.capacity
        while capacity < n:
            capacity *= 2
        self._allocate(capacity)
        self._sorted[0][:n].copy_(torch.from_numpy(np.sort(history)))     # np.sort: ascending, NaN last -- the device's key
        self._arrival[:n].copy_(torch.from_numpy(history))
        self._n = n
        self._observed = False
