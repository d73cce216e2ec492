"""The guard-band harness (tests/guard_arena.py) catches what it is for: toy ops written in torch run on a CPU arena through the
same proxy the GPU cases use, each with one planted error, and the report has to name the slot and the offset.  CPU only."""
import os
import re
import sys

import pytest
import torch

import guard_arena as GA
from guard_arena import Arena, GuardError, guarded

HERE = sys.modules[__name__]
N = 5
X = torch.arange(1.0, N + 1)


# ---------------------------------------------------------------------------------------------------- the toy ops
def _stray(t, k):
    """the element k places from t's first one, where t's storage holds it: the plain run's CPU blocks have no slack for a
    stray store to land in, the caching allocator's rounded blocks and the arena do"""
    at = t.storage_offset() + k
    if 0 <= at and (at + 1) * t.element_size() <= t.untyped_storage().nbytes():
        return t.as_strided((1,), (1,), at)
    return torch.empty(1)


def op_clean(x):
    out = torch.empty_like(x)
    acc = torch.zeros(x.shape[0])
    acc += x
    out.copy_(acc * 2)
    return out


def op_write_past(x):
    out = torch.empty(x.shape[0])
    out.copy_(x * 2)
    _stray(out, x.shape[0]).fill_(7.0)
    return out


def op_write_before(x):
    out = torch.empty(x.shape[0])
    out.copy_(x * 2)
    _stray(out, -1).fill_(7.0)
    return out


def op_leaves_one(x):
    out = torch.empty(x.shape[0])
    out[:-1].copy_(x[:-1] * 2)
    return out


def op_reads_scratch(x):
    scratch = torch.empty(x.shape[0])
    out = torch.empty(x.shape[0])
    out.copy_(x + 0.5 * scratch)
    return out


def op_reads_past(x):
    out = torch.empty(x.shape[0])
    out.copy_(x.as_strided((x.shape[0],), (1,), x.storage_offset() + 1) * 2)
    return out


def op_inplace(x):
    x.mul_(2)
    return x.sum().reshape(1)


def _line(fn, text):
    """the line of fn's source that holds `text`"""
    import inspect
    lines, first = inspect.getsourcelines(fn)
    return first + [i for i, l in enumerate(lines) if text in l][0]


def _fails(fn, *patterns, **kw):
    with pytest.raises(GuardError) as err:
        guarded(fn, [X], modules=[HERE], **kw)
    msg = str(err.value)
    for p in patterns:
        assert re.search(p, msg), (p, msg)
    return msg


# ---------------------------------------------------------------------------------------------------- planted errors
def test_clean_op_passes():
    entered = set()
    out = guarded(op_clean, [X], modules=[HERE], entered=entered)
    assert torch.equal(out, X * 2)
    assert (os.path.abspath(__file__), op_clean.__code__.co_firstlineno) in entered


def test_write_one_past_an_output_is_reported():
    site = r"test_guard_arena\.py:op_write_past:%d float32 \(5,\)" % _line(op_write_past, "torch.empty")
    msg = _fails(op_write_past, r"\(a\) nan poison: trailing band of %s damaged, bytes \+20 \.\. \+23 relative" % site,
                 r"\(a\) huge poison: trailing band of %s damaged, bytes \+20 \.\. \+23" % site)
    assert "leading" not in msg and "(c)" not in msg


def test_write_one_before_an_output_is_reported():
    site = r"test_guard_arena\.py:op_write_before:%d float32 \(5,\)" % _line(op_write_before, "torch.empty")
    msg = _fails(op_write_before, r"\(a\) nan poison: leading band of %s damaged, bytes -4 \.\. -1 relative" % site)
    assert "trailing" not in msg


def test_unwritten_output_element_is_reported():
    msg = _fails(op_leaves_one, r"\(c\) output 0 \(5,\): 1 of 5 elements differ .* first at flat index 4 \(4,\): it holds the "
                                r"poison pattern in every guarded run \(never written\)")
    assert "(a)" not in msg and "(b)" not in msg


def test_scratch_read_before_written_is_reported():
    msg = _fails(op_reads_scratch, r"\(c\) output 0 \(5,\): 5 of 5 elements differ .* first at flat index 0 \(0,\): it does not "
                                   r"hold the poison pattern \(computed from memory the op does not own\)")
    assert "(a)" not in msg


def test_read_one_past_a_placed_input_is_reported():
    """the plain run reads friendly memory, as a prefix view of a larger operand gives it; the placed copy ends where the view
    ends, so the element past it is poison"""
    big = torch.arange(1.0, N + 2)
    plain = [op_reads_past(big[:N])]
    assert torch.equal(plain[0], big[1:] * 2)
    runs = {}
    for poison in GA.POISONS:
        arena = Arena("cpu", poison)
        x = arena.place(big[:N], "x")
        assert x.shape == (N,) and arena.slots[0].nbytes == 4 * N
        with arena.installed(pytest.MonkeyPatch(), [HERE]):
            runs[poison] = [op_reads_past(x)]
        arena.check()                                           # a read damages nothing
        assert arena.placed_changes() == []
    msgs = GA.compare_runs(plain, runs)
    assert len(msgs) == 2, msgs
    for m in msgs:
        assert re.search(r"output 0 \(5,\): 1 of 5 elements differ .* first at flat index 4 \(4,\): it does not hold the poison "
                         r"pattern \(computed from memory", m), m


def test_written_input_is_reported_unless_declared():
    _fails(op_inplace, r"\(b\) nan poison: place\(tensor 0 of the inputs\) was written to")
    out = guarded(op_inplace, [X], inplace=(0,), modules=[HERE])
    assert float(out) == float(X.sum() * 2) and torch.equal(X, torch.arange(1.0, N + 1))


def op_block(x, out):
    out.copy_(x * 2)
    return out


def op_block_spills(x, out):
    out.copy_(x * 2)
    _stray(out, out.shape[1]).fill_(3.0)                        # the neighbour column behind row 0 of the block
    return out


def test_neighbours_of_an_in_place_column_block_are_held_to_their_bits():
    x, buf = torch.arange(6.0).reshape(3, 2), torch.full((3, 5), 7.0)
    guarded(op_block, [x, buf[:, 1:3]], inplace=(1,), modules=[HERE])
    with pytest.raises(GuardError) as err:
        guarded(op_block_spills, [x, buf[:, 1:3]], inplace=(1,), modules=[HERE])
    assert "(b) nan poison: place(tensor 1 of the inputs) outside the view it may be written through was written to" in str(err.value)
    assert "(a)" not in str(err.value)


CACHE = {}


def op_caches(x):
    if "words" not in CACHE:
        CACHE["words"] = [torch.zeros(4), 0]
    return op_clean(x)


def test_a_module_level_cache_made_in_the_arena_is_dropped_with_it():
    CACHE.clear()
    GA.poison_pass(op_caches, [X], "nan", modules=[HERE])
    assert CACHE == {}
    keep = CACHE["words"] = [torch.zeros(4), 0]                 # one made outside stays
    guarded(op_caches, [X], modules=[HERE])
    assert CACHE["words"] is keep
    CACHE.clear()


def test_check_names_slot_and_offsets():
    arena = Arena("cpu", "huge", band=1024)
    a = arena.new((3,), (1,), torch.int32, "first")
    b = arena.new((2, 2), (2, 1), torch.float32, "second")
    arena.check()
    b.as_strided((3,), (1,), b.storage_offset() + 4).fill_(1.0)
    a.as_strided((1,), (1,), a.storage_offset() - 2).fill_(5)
    with pytest.raises(GuardError) as err:
        arena.check()
    msg = str(err.value)
    assert "first int32 (3,): leading band, bytes -8 .. -8 relative to the payload of 12 bytes" in msg, msg      # the low byte of 5
    assert "second float32 (2, 2): trailing band, bytes +16 .. +27 relative to the payload of 16 bytes" in msg, msg


# ---------------------------------------------------------------------------------------------------- layout
@pytest.mark.parametrize("poison", GA.POISONS)
@pytest.mark.parametrize("n,dtype", [(5, torch.float32), (3, torch.int32), (1, torch.uint8)])
def test_payload_alignment_and_trailing_band(n, dtype, poison):
    arena = Arena("cpu", poison, band=512)
    arena.new((7,), (1,), torch.float32, "before")              # an odd slot in front
    t = arena.new((n,), (1,), dtype, "t")
    slot = arena.slots[-1]
    nbytes = n * t.element_size()
    assert t.data_ptr() % 512 == 0 and slot.nbytes == nbytes
    assert t.data_ptr() - arena.buf.data_ptr() == slot.payload
    tail = slot.payload + nbytes
    assert not bool(arena.isband[slot.payload:tail].any())
    assert bool(arena.isband[slot.begin:slot.payload].all()) and bool(arena.isband[tail:slot.end].all())
    assert slot.payload - slot.begin == 512 and slot.end - tail >= 512 and slot.end % 512 == 0
    arena.check()
    arena.buf[tail] ^= 1                                        # the very first byte after the payload
    dmg = arena.damage()
    assert [(s.label, side, lo, hi) for s, side, lo, hi in dmg] == [("t", "trailing", nbytes, nbytes)]


def test_a_placed_view_keeps_pitch_neighbours_and_alignment():
    base = torch.arange(24.0).reshape(4, 6)
    col = base[:, 2:5]
    arena = Arena("cpu", "nan")
    p = arena.place(col)
    assert p.shape == col.shape and p.stride() == col.stride() and torch.equal(p, col)
    assert arena.slots[0].nbytes == 4 * (3 * 6 + 3)             # from the first to the last element of the block
    assert float(p.as_strided((1,), (1,), p.storage_offset() + 3)) == 5.0        # the neighbour column came along
    assert p.data_ptr() % 512 == col.data_ptr() % 512


def test_same_tensor_placed_twice_is_the_same_memory():
    arena = Arena("cpu", "nan")
    x = torch.randn(6, 4)
    a, b = arena.place(x), arena.place(x)
    assert a.data_ptr() == b.data_ptr() and len(arena.slots) == 1
    c = arena.place(x.t())                                      # another view of the same extent: still the same memory
    assert c.data_ptr() == a.data_ptr() and c.stride() == (1, 4)
    assert arena.place(torch.randn(6, 4)).data_ptr() != a.data_ptr()


@pytest.mark.parametrize("view", ["column_block", "transposed", "dense"])
def test_empty_like_has_torchs_strides(view):
    base = torch.arange(24.0).reshape(4, 6)
    t = {"column_block": base[:, 2:5], "transposed": base.t(), "dense": base}[view]
    arena = Arena("cpu", "nan")
    proxy = GA._TorchProxy(arena)
    for fn in ("empty_like", "zeros_like"):
        got, want = getattr(proxy, fn)(t), getattr(torch, fn)(t)
        assert got.stride() == want.stride() and got.shape == want.shape and got.dtype == want.dtype
    assert len(arena.slots) == 2
    assert proxy.empty_like(t, dtype=torch.int32).dtype == torch.int32


@pytest.mark.parametrize("poison", GA.POISONS)
def test_integer_poison_is_minus_one_or_zero(poison):
    for dtype in (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64, torch.bool):
        octets = GA.poison_value(dtype, poison).view(torch.uint8)
        assert bool((octets == (255 if poison == "nan" else 0)).all())
        arena = Arena("cpu", poison, band=512, capacity=1 << 16)
        t = GA._TorchProxy(arena).empty(3, dtype=dtype)
        assert t.to(torch.int64).abs().max() <= (1 if dtype != torch.uint8 else 255)
        s = arena.slots[0]
        assert set(arena.buf[s.begin:s.end].tolist()) == {255 if poison == "nan" else 0}
    for dtype in (torch.float32, torch.float64, torch.bfloat16):
        v = GA.poison_value(dtype, poison)
        assert bool(torch.isnan(v).all()) if poison == "nan" else 0.99e30 < float(v) < 1.01e30


def test_initialised_allocations_keep_their_content():
    arena = Arena("cpu", "nan")
    proxy = GA._TorchProxy(arena)
    assert torch.equal(proxy.zeros(3, 2), torch.zeros(3, 2))
    assert torch.equal(proxy.ones((4,), dtype=torch.int32), torch.ones(4, dtype=torch.int32))
    assert torch.equal(proxy.full((2, 2), 1e10), torch.full((2, 2), 1e10))
    assert torch.equal(proxy.zeros_like(X), torch.zeros_like(X))
    assert bool(torch.isnan(proxy.empty(3)).all()) and bool(torch.isnan(proxy.empty_like(X)).all())
    assert len(arena.slots) == 6
    arena.check()


def test_pinned_foreign_empty_and_out_requests_pass_through(monkeypatch):
    seen = []
    real = torch.empty

    def recorder(*args, **kw):
        seen.append((args, dict(kw)))
        kw.pop("pin_memory", None)                              # a machine without a GPU cannot pin
        return real(*args, **kw)
    arena = Arena("cpu", "nan")
    monkeypatch.setattr(torch, "empty", recorder)
    proxy = GA._TorchProxy(arena)
    proxy.empty(4, dtype=torch.int32, pin_memory=True)
    assert seen == [((4,), {"dtype": torch.int32, "pin_memory": True})]
    monkeypatch.setattr(torch, "empty", real)
    proxy = GA._TorchProxy(arena)
    assert proxy.empty(0).numel() == 0 and proxy.empty((3, 0), dtype=torch.int64).shape == (3, 0)
    assert proxy.empty(3, device="meta").device.type == "meta"
    buf = torch.empty(3)
    assert proxy.zeros(3, out=buf) is buf
    assert arena.slots == []
    assert proxy.float32 is torch.float32 and proxy.nn is torch.nn


# ---------------------------------------------------------------------------------------------------- the module list
def test_every_allocating_module_is_in_the_harness_list(dcl):
    package = os.path.dirname(os.path.abspath(dcl.__file__))
    want = GA.modules_allocating(package)
    listed = sorted(name.replace(".", os.sep) + ".py" for name in GA.ALLOCATING_MODULES)
    assert want == listed
    mods = GA.allocating_modules(dcl)
    assert all(m.torch is torch for m in mods)
    assert sorted(os.path.relpath(m.__file__, package) for m in mods) == listed


def test_function_table_names_functions_methods_and_lambdas(dcl):
    ops = GA.allocating_modules(dcl)[0]
    table = GA.function_table(ops.__file__)
    alloc = table.allocating()
    assert "sparse_conv" in alloc and "BackboneRun.__init__" in alloc and "_conf_pool_layout_backward" in alloc
    assert "linear_split_ok" not in alloc
    assert sum(len(v) for v in alloc.values()) == sum(len(v) for v in GA.function_table(ops.__file__).allocating().values())
    for name, lines in alloc.items():
        assert all(table.name_at(l) == name for l in lines)
