"""Guard-band runs (helper; no test functions here, and nothing that needs a GPU to import).

The product library allocates nothing on the device itself: every byte a kernel touches is handed over from Python, as an
input or as one of the torch.empty / zeros / full buffers of the allocating modules.  Arena puts each of them between two
poisoned bands of one uint8 tensor, so that a kernel that writes outside what it was given damages a band, and one that reads
outside it, or reads scratch before writing it, computes different bits under the two poisons.

  Arena(device, poison, band, capacity)   bump allocator; a slot is  band | payload | band.  The trailing band starts at the
                                          payload's last byte + 1 and runs to the next 512-byte boundary plus `band`.  A fresh
                                          payload is 512-byte aligned like the caching allocator's blocks; a placed view keeps
                                          its source's address modulo 512, so the launchers take the paths the plain run takes.
  poison "nan"                            all-ones bytes: a NaN for floating types, -1 for integer types and bool
  poison "huge"                           1e30 for floating types, 0 for integer types and bool
                                          (an integer poison is only ever -1 or 0: a stray index read never becomes a far access)
  arena.place(t)                          copies the smallest storage extent t spans and returns t's shape, strides and dtype on
                                          it; the same extent placed twice is the same memory (aliased arguments stay aliased)
  arena.installed(monkeypatch, modules)   context: the module-global `torch` of each module forwards to torch but allocates
                                          empty / empty_like / zeros / zeros_like / full / ones of the arena's device from the arena;
                                          arena.entered collects the functions of those modules that were entered (a profile
                                          function, and the stack of every allocation: the autograd engine's threads have none)
  arena.check()                           one comparison of every band byte with its pattern
  guarded(fn, inputs, ...)                plain run, then one run per poison; bands, inputs and bit-identical outputs

What it does not see: a stray read that reaches no result, memory the C side allocates itself (the vendor and diagnostic
path of csrc/linear.cpp), anything under graph capture (the arena's addresses would be baked into the graph), a stray
access further than `band` bytes away from its buffer, and a buffer an op caches at module level once a plain run has made
it (ops._VI_COMM: zero-initialised words that persist between calls)."""
import ast
import bisect
import contextlib
import os
import sys

import torch

from step_replay import same_bits

POISONS = ("nan", "huge")
ALIGN = 512
HUGE = 1e30
_OVERRIDDEN = ("empty", "empty_like", "zeros", "zeros_like", "full", "ones")
_UNINITIALISED = ("empty", "empty_like")
_INT_OF = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


class GuardError(AssertionError):
    pass


def poison_value(dtype, poison):
    """the one-element tensor a band of `dtype` is filled with"""
    size = torch.empty((), dtype=dtype).element_size()
    if poison == "nan" or not dtype.is_floating_point:
        byte = 255 if poison == "nan" else 0
        return torch.full((size,), byte, dtype=torch.uint8).view(dtype)
    return torch.full((1,), HUGE, dtype=dtype)


def span_elements(shape, stride):
    """elements between the first and one past the last element of a view (0 for an empty one)"""
    n = 1
    for s, st in zip(shape, stride):
        if s == 0:
            return 0
        n += (s - 1) * st
    return n


class Slot(object):
    def __init__(self, label, dtype, shape, begin, payload, nbytes, end):
        self.label, self.dtype, self.shape = label, dtype, tuple(shape)
        self.begin, self.payload, self.nbytes, self.end = begin, payload, nbytes, end      # byte offsets in the arena

    def describe(self):
        return "%s %s %s" % (self.label, str(self.dtype).replace("torch.", ""), self.shape)


class Arena(object):
    def __init__(self, device, poison, band=65536, capacity=None):
        assert poison in POISONS, poison
        assert band > 0 and band % ALIGN == 0, "band is a multiple of %d" % ALIGN
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.poison, self.band = poison, band
        if capacity is None:
            capacity = (1 << 28) if self.device.type == "cuda" else (1 << 24)
        self.capacity = capacity
        raw = torch.empty(capacity + ALIGN, dtype=torch.uint8, device=self.device)
        self._shift = (-raw.data_ptr()) % ALIGN                # byte 0 of the arena is 512-byte aligned
        self.buf = raw[self._shift:self._shift + capacity]
        self.expect = torch.empty(capacity, dtype=torch.uint8, device=self.device)        # the bands' pattern
        self.isband = torch.empty(capacity, dtype=torch.bool, device=self.device)
        self.top = 0
        self.slots, self._starts = [], []
        self._placed, self._keep = {}, []
        self.entered = set()                                   # (file name, first line) of every code object entered
        self._files = set()

    # ------------------------------------------------------------------------------------------------ allocation
    def _paint(self, target, lo, hi, dtype):
        if hi > lo:
            pat = poison_value(dtype, self.poison)
            octets = pat.view(torch.uint8)
            if bool((octets == octets[0]).all()):
                target[lo:hi].fill_(int(octets[0]))
            else:
                target[lo:hi].view(dtype).fill_(pat[0])

    def _fill(self, lo, hi, dtype):
        self._paint(self.buf, lo, hi, dtype)
        self._paint(self.expect, lo, hi, dtype)

    def carve(self, nbytes, dtype, shape, label, misalign=0, poison_payload=True):
        """-> (slot, the payload as a uint8 tensor of nbytes)"""
        size = torch.empty((), dtype=dtype).element_size()
        assert nbytes > 0 and nbytes % size == 0 and misalign % size == 0 and 0 <= misalign < ALIGN
        begin = self.top                                        # always 512-byte aligned
        payload = begin + self.band + misalign
        tail = payload + nbytes
        end = (tail + ALIGN - 1) // ALIGN * ALIGN + self.band
        if end > self.capacity:
            raise GuardError("the arena of %d bytes is full at slot %d (%s): give the run a larger capacity"
                             % (self.capacity, len(self.slots), label))
        self.top = end
        self._fill(begin, payload, dtype)
        self._fill(tail, end, dtype)
        self.isband[begin:payload] = True
        self.isband[payload:tail] = False
        self.isband[tail:end] = True
        if poison_payload:
            self._paint(self.buf, payload, tail, dtype)
        slot = Slot(label, dtype, shape, begin, payload, nbytes, end)
        self.slots.append(slot)
        self._starts.append(begin)
        return slot, self._own(payload, nbytes, torch.uint8)

    def _own(self, at, nbytes, dtype, shape=None, stride=None):
        """bytes at .. at + nbytes of the arena as a tensor of dtype (1-D, or of the given shape and strides) that is NOT a view
        of the arena tensor: every slot has its own version counter, as separately allocated tensors have (autograd forbids
        a custom Function's output whose base was modified in place, and every write to another slot would count as one)"""
        size = torch.empty((), dtype=dtype).element_size()
        at += self.buf.storage_offset()
        assert at % size == 0 and nbytes % size == 0
        if shape is None:
            shape, stride = (nbytes // size,), (1,)
        return torch.empty(0, dtype=dtype, device=self.device).set_(self.buf.untyped_storage(), at // size, tuple(shape), tuple(stride))

    def new(self, shape, stride, dtype, label, poison_payload=True):
        """a tensor of the given shape and (dense or overlapping, non-negative) strides in a slot of its own"""
        size = torch.empty((), dtype=dtype).element_size()
        span = span_elements(shape, stride)
        slot, _ = self.carve(span * size, dtype, shape, label, poison_payload=poison_payload)
        return self._own(slot.payload, slot.nbytes, dtype, shape, stride)

    def place(self, t, label=None):
        if not isinstance(t, torch.Tensor):
            return t
        if t.numel() == 0:
            return t.detach().to(self.device).requires_grad_(t.requires_grad)
        assert all(st >= 0 for st in t.stride()), "negative strides are not placed"
        span = span_elements(t.shape, t.stride())
        key = (t.untyped_storage().data_ptr(), t.device, t.dtype, t.storage_offset(), span)
        hit = self._placed.get(key)
        if hit is None:
            flat = t.detach().as_strided((span,), (1,), t.storage_offset())
            label = "place(%s)" % (label if label is not None else "input %d" % len(self._placed))
            slot, payload = self.carve(span * t.element_size(), t.dtype, t.shape, label,
                                       misalign=t.data_ptr() % ALIGN if t.device.type == self.device.type else 0,
                                       poison_payload=False)
            mine = self._own(slot.payload, slot.nbytes, t.dtype)
            mine.copy_(flat)
            hit = self._placed[key] = (slot, mine, flat.clone())
            self._keep.append(t)                               # the key holds an address: the source stays alive
        out = self._own(hit[0].payload, hit[0].nbytes, t.dtype, t.shape, t.stride())
        return out.requires_grad_(True) if t.requires_grad else out

    def placed_changes(self, written=None):
        """labels of the placed inputs whose payload no longer has the bits that were copied in.  written: {label: [(shape,
        stride), ...]}, the views through which an argument may be written in place -- of such a payload only the elements
        OUTSIDE those views are held to their bits (the neighbour columns of an `out=` column block)"""
        written = written or {}
        out = []
        for slot, now, was in self._placed.values():
            was = was.to(self.device)
            if slot.label in written:
                keep = torch.ones(now.numel(), dtype=torch.bool, device=self.device)
                for shape, stride in written[slot.label]:
                    keep.as_strided(tuple(shape), tuple(stride)).fill_(False)
                if not same_bits(now[keep], was[keep]):
                    out.append(slot.label + " outside the view it may be written through")
            elif not same_bits(now, was):
                out.append(slot.label)
        return out

    def forget_cached(self, modules):
        """drops the entries of the modules' global dicts that hold a tensor of this arena (a buffer an op caches at module
        level, such as ops._VI_COMM, must not outlive the run that allocated it from the arena)"""
        mine = self.buf.untyped_storage().data_ptr()
        for mod in modules:
            for value in vars(mod).values():
                if isinstance(value, dict):
                    for k in [k for k, v in value.items() if any(t.untyped_storage().data_ptr() == mine for t in tensors_of(v))]:
                        del value[k]

    # ------------------------------------------------------------------------------------------------ the proxy
    @contextlib.contextmanager
    def installed(self, monkeypatch, modules):
        proxy = _TorchProxy(self)
        files = self._files = set(os.path.abspath(m.__file__) for m in modules)
        entered = self.entered

        def profile(frame, event, arg):
            if event == "call" and os.path.abspath(frame.f_code.co_filename) in files:
                entered.add((os.path.abspath(frame.f_code.co_filename), frame.f_code.co_firstlineno))

        with monkeypatch.context() as m:
            for mod in modules:
                assert getattr(mod, "torch", None) is torch, "%s has no module-global torch" % mod.__name__
                m.setattr(mod, "torch", proxy)
            old = sys.getprofile()
            sys.setprofile(profile)
            try:
                yield self
            finally:
                sys.setprofile(old)

    def entered_functions(self, module):
        """qualified names of the functions of `module` entered while the proxy was installed (a lambda or a comprehension
        counts for the function that holds it)"""
        return entered_names(self.entered, module)

    # ------------------------------------------------------------------------------------------------ the check
    def damage(self):
        """-> list of (slot, 'leading' | 'trailing', first, last damaged byte offset relative to the payload)"""
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        top = self.top
        bad = (self.buf[:top] != self.expect[:top]) & self.isband[:top]
        if not bool(bad.any()):
            return []
        found = {}
        for pos in bad.nonzero().flatten().tolist():
            slot = self.slots[bisect.bisect_right(self._starts, pos) - 1]
            side = "leading" if pos < slot.payload else "trailing"
            rel = pos - slot.payload
            lo, hi = found.get((id(slot), side), (rel, rel))
            found[(id(slot), side)] = (min(lo, rel), max(hi, rel))
        by_id = dict((id(s), s) for s in self.slots)
        return [(by_id[i], side, lo, hi) for (i, side), (lo, hi) in sorted(found.items(), key=lambda kv: by_id[kv[0][0]].begin)]

    def check(self):
        dmg = self.damage()
        if dmg:
            raise GuardError("damaged guard bands (%s poison):\n" % self.poison + "\n".join(
                "  %s: %s band, bytes %+d .. %+d relative to the payload of %d bytes" % (s.describe(), side, lo, hi, s.nbytes)
                for s, side, lo, hi in dmg))


def _site(depth=2):
    f = sys._getframe(depth)
    return "%s:%s:%d" % (os.path.basename(f.f_code.co_filename), f.f_code.co_name, f.f_lineno)


class _TorchProxy(object):
    """forwards every attribute to torch; the six allocating functions go through the arena where they would allocate on its
    device"""

    def __init__(self, arena):
        object.__setattr__(self, "_arena", arena)
        for name in _OVERRIDDEN:
            object.__setattr__(self, name, self._make(name))

    def __getattr__(self, name):
        return getattr(torch, name)

    def __setattr__(self, name, value):
        setattr(torch, name, value)

    def _mine(self, device):
        arena = self._arena.device
        dev = torch.device(device) if device is not None else torch.empty(0).device
        if dev.type != arena.type:
            return False
        return dev.index is None or arena.index is None or dev.index == arena.index

    def _make(self, name):
        real = getattr(torch, name)
        like = name.endswith("_like")

        def alloc(*args, **kw):
            device = kw.get("device")
            if like and device is None:
                device = args[0].device
            if kw.get("out") is not None or kw.get("pin_memory") or not self._mine(device):
                return real(*args, **kw)
            meta_kw = dict((k, v) for k, v in kw.items() if k not in ("pin_memory", "requires_grad"))
            meta_kw["device"] = "meta"
            meta = real(*args, **meta_kw)                       # torch's own shape, dtype and strides
            if meta.numel() == 0:
                return real(*args, **kw)
            arena = self._arena
            f = sys._getframe(1)
            while f is not None:                                # the autograd engine's threads run no profile function
                if os.path.abspath(f.f_code.co_filename) in arena._files:
                    arena.entered.add((os.path.abspath(f.f_code.co_filename), f.f_code.co_firstlineno))
                f = f.f_back
            t = arena.new(meta.shape, meta.stride(), meta.dtype, _site(), poison_payload=name in _UNINITIALISED)
            if name.startswith("zeros"):
                t.zero_()
            elif name == "ones":
                t.fill_(1)
            elif name == "full":
                t.fill_(args[1] if len(args) > 1 else kw["fill_value"])
            return t.requires_grad_(True) if kw.get("requires_grad") else t
        alloc.__name__ = name
        return alloc


# ---------------------------------------------------------------------------------------------------- source census
class function_table(object):
    """the named functions of a source file by line: name_at(first line of a code object) -> qualified name of the innermost
    def that holds it; allocating(names) -> {qualified name: lines of the calls torch.<name>(...) it holds}"""

    def __init__(self, path):
        with open(path) as f:
            self.tree = ast.parse(f.read(), path)
        self.spans = []                                         # (first line, last line, qualified name)
        self._walk(self.tree, "")

    def _walk(self, node, prefix):
        for child in ast.iter_child_nodes(node):
            if isinstance(child, (ast.FunctionDef, ast.AsyncFunctionDef, ast.ClassDef)):
                name = prefix + child.name
                if not isinstance(child, ast.ClassDef):
                    first = min([child.lineno] + [d.lineno for d in child.decorator_list])
                    self.spans.append((first, child.end_lineno, name, child))
                self._walk(child, name + ".")
            else:
                self._walk(child, prefix)

    def name_at(self, line):
        best = None
        for first, last, name, _ in self.spans:
            if first <= line <= last and (best is None or first >= best[0]):
                best = (first, name)
        return best[1] if best else None

    def allocating(self, names=_UNINITIALISED):
        out = {}
        for _, _, name, node in self.spans:
            lines = [c.lineno for c in ast.walk(node) if _is_torch_call(c, names) and self.name_at(c.lineno) == name]
            if lines:
                out[name] = lines
        return out


def _is_torch_call(node, names):
    return (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr in names
            and isinstance(node.func.value, ast.Name) and node.func.value.id == "torch")


def modules_allocating(package_dir, names=_UNINITIALISED):
    """the .py files under package_dir in which torch.empty or torch.empty_like is called, relative paths"""
    out = []
    for root, _, files in os.walk(package_dir):
        for fn in sorted(files):
            if fn.endswith(".py"):
                path = os.path.join(root, fn)
                with open(path) as f:
                    tree = ast.parse(f.read(), path)
                if any(_is_torch_call(c, names) for c in ast.walk(tree)):
                    out.append(os.path.relpath(path, package_dir))
    return sorted(out)


ALLOCATING_MODULES = ("ops", "autograd", "optim", "sharding", "models.refiner", "models.DCL_Net",
                      "libs.pointnet_lib.pointnet2_utils")


def allocating_modules(dcl):
    """the modules of the product package given to Arena.installed (tests/test_guard_arena.py keeps the list complete)"""
    import importlib
    return [importlib.import_module(dcl.__name__ + "." + name) for name in ALLOCATING_MODULES]


# ---------------------------------------------------------------------------------------------------- the guarded run
def clone_extent(t):
    """a copy of the storage extent t spans with t's shape and strides on it, at t's address modulo 512 where the allocator
    aligns its blocks (a column block keeps its pitch, its neighbours and the alignment the launchers look at)"""
    if t.numel() == 0 or any(st < 0 for st in t.stride()):
        return t.detach().clone().requires_grad_(t.requires_grad)
    span = span_elements(t.shape, t.stride())
    lead = (t.data_ptr() % ALIGN) // t.element_size()
    flat = torch.empty(lead + span, dtype=t.dtype, device=t.device)
    flat[lead:].copy_(t.detach().as_strided((span,), (1,), t.storage_offset()))
    return flat.as_strided(tuple(t.shape), tuple(t.stride()), lead).requires_grad_(t.requires_grad)


def tensors_of(value, out=None):
    """the tensors of a nested result (tensors, lists, tuples, dict values in key order, objects are skipped), in order"""
    out = [] if out is None else out
    if isinstance(value, torch.Tensor):
        out.append(value)
    elif isinstance(value, (list, tuple)):
        for v in value:
            tensors_of(v, out)
    elif isinstance(value, dict):
        for k in sorted(value, key=str):
            tensors_of(value[k], out)
    return out


def map_tensors(value, fn):
    if isinstance(value, torch.Tensor):
        return fn(value)
    if isinstance(value, tuple):
        return tuple(map_tensors(v, fn) for v in value)
    if isinstance(value, list):
        return [map_tensors(v, fn) for v in value]
    if isinstance(value, dict):
        return dict((k, map_tensors(v, fn)) for k, v in value.items())
    return value


def _bits(t):
    t = t.detach().contiguous()
    if t.dtype == torch.bool:
        return t.view(torch.uint8)
    return t.view(_INT_OF[t.element_size()]) if t.dtype.is_floating_point else t


def _first_difference(a, b):
    """index (flat, in a contiguous copy) of the first element whose bits differ, and how many differ"""
    ne = (_bits(a) != _bits(b.to(a.device))).flatten()
    return int(ne.nonzero()[0]), int(ne.sum())


def _is_poison(t, flat_index, poison):
    v = t.detach().contiguous().flatten()[flat_index:flat_index + 1].cpu()
    return bool(torch.equal(_bits(v), _bits(poison_value(t.dtype, poison))))


def compare_runs(plain, runs, what="output"):
    """plain: list of tensors; runs: {poison: list of tensors}.  -> list of messages, empty when all three agree in bits"""
    bad = []
    for poison, outs in runs.items():
        if len(outs) != len(plain):
            bad.append("%s run returned %d tensors, the plain run %d" % (poison, len(outs), len(plain)))
    if bad:
        return bad
    for i, want in enumerate(plain):
        for poison, outs in runs.items():
            got = outs[i]
            if same_bits(got, want):
                continue
            if got.shape != want.shape or got.dtype != want.dtype:
                bad.append("%s %d: %s %s under %s poison, %s %s plain" % (what, i, got.dtype, tuple(got.shape), poison, want.dtype,
                                                                          tuple(want.shape)))
                continue
            at, count = _first_difference(got, want)
            never = all(r[i].shape == want.shape and _is_poison(r[i], at, p) for p, r in runs.items())
            bad.append("%s %d %s: %d of %d elements differ from the plain run under %s poison, the first at flat index %d %s: %s"
                       % (what, i, tuple(want.shape), count, want.numel(), poison, at,
                          tuple(int(v) for v in torch.unravel_index(torch.tensor(at), want.shape)) if want.dim() else (),
                          "it holds the poison pattern in every guarded run (never written)" if never else
                          "it does not hold the poison pattern (computed from memory the op does not own)"))
    return bad


def guarded(fn, inputs, valid=None, inplace=(), modules=(), device=None, band=65536, capacity=None, entered=None):
    """Runs fn(*inputs) plain, then once per poison inside a fresh arena with placed inputs and the proxy installed in
    `modules`, and raises GuardError unless (a) every band is intact, (b) every placed input has the bits that were copied
    in, except the arguments whose positions `inplace` names, and (c) the outputs, followed by the in-place arguments, are
    bit-identical in all three runs over valid(outputs) (a function from the list of output tensors to the list of tensors
    to compare; default: all of them, whole).  Every run gets clones of `inputs`.  entered: a set that receives
    Arena.entered of the guarded runs.  -> the plain run's result"""
    import pytest

    def fresh():
        done = {}

        def copy(t):
            if id(t) not in done:
                done[id(t)] = clone_extent(t)
            return done[id(t)]
        return map_tensors(list(inputs), copy)
    select = (lambda outs: outs) if valid is None else valid

    def collect(result, args):
        return list(select(tensors_of(result))) + [t for i in inplace for t in tensors_of(args[i])]

    args = fresh()
    result = fn(*args)
    plain = [t.detach().clone() for t in collect(result, args)]
    if device is None:
        first = tensors_of(list(inputs)) + tensors_of(result)
        device = first[0].device if first else torch.device("cpu")
    runs, problems = {}, []
    for poison in POISONS:
        arena = Arena(device, poison, band=band, capacity=capacity)
        src = fresh()
        labels = {}

        def put(t):
            labels.setdefault(id(t), len(labels))
            return arena.place(t, "tensor %d of the inputs" % labels[id(t)])
        args = map_tensors(src, put)
        written = {}
        for i in inplace:
            for t in tensors_of(src[i]):
                written.setdefault("place(tensor %d of the inputs)" % labels[id(t)], []).append((t.shape, t.stride()))
        try:
            with arena.installed(pytest.MonkeyPatch(), list(modules)):
                res = fn(*args)
        finally:
            arena.forget_cached(modules)
        if entered is not None:
            entered |= arena.entered
        runs[poison] = [t.detach().clone() for t in collect(res, args)]
        for s, side, lo, hi in arena.damage():
            problems.append("(a) %s poison: %s band of %s damaged, bytes %+d .. %+d relative to the payload of %d bytes"
                            % (poison, side, s.describe(), lo, hi, s.nbytes))
        for label in arena.placed_changes(written):
            problems.append("(b) %s poison: %s was written to" % (poison, label))
    problems += ["(c) " + m for m in compare_runs(plain, runs)]
    if problems:
        raise GuardError("\n".join(problems))
    return result


def poison_pass(fn, inputs, poison, modules=(), device=None, band=65536, capacity=None, entered=None):
    """one guarded run alone, without the comparisons: fn(*placed inputs) under `poison` with the proxy installed, then the
    band check.  -> the run's result"""
    import pytest
    if device is None:
        first = tensors_of(list(inputs))
        device = first[0].device if first else torch.device("cpu")
    arena = Arena(device, poison, band=band, capacity=capacity)
    done = {}

    def put(t):
        if id(t) not in done:
            done[id(t)] = arena.place(clone_extent(t))
        return done[id(t)]
    args = map_tensors(list(inputs), put)
    try:
        with arena.installed(pytest.MonkeyPatch(), list(modules)):
            res = fn(*args)
    finally:
        arena.forget_cached(modules)
    if entered is not None:
        entered |= arena.entered
    arena.check()
    return res


def entered_names(codes, module):
    """qualified names of the functions of `module` among (file, first line) pairs as Arena.entered holds them"""
    path = os.path.abspath(module.__file__)
    table = function_table(path)
    return set(table.name_at(line) for f, line in codes if f == path) - {None}
