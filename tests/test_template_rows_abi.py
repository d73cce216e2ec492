"""The template-row scatter without a GPU (csrc/template_rows.hip): dcl_template_rows and its host twin are declared with the
documented argument lists and exported by both libraries, refuse bad arguments before any GPU work, and the host twin --
the same contract in plain C++ -- equals plain indexing on the shared cases, the miss semantics included."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import template_cases as tc
from test_conv_pairs_abi import declarations

_ARGS = ["const float *cache", "int64_t class_floats", "int row_floats", "int n_tmp", "const int32_t *lut", "int lut_len",
         "const int32_t *cls", "int b", "const DclTemplateBlock *blocks", "int nblocks", "int32_t *miss"]
WANT = {"dcl_template_rows": _ARGS + ["dclStream_t stream"], "dcl_template_rows_host": _ARGS}


def _libs(dcl):
    import os
    assert os.path.exists(dcl._native.DIAG_SO_PATH), "diagnostic library missing: build() makes it"
    return [("product", dcl._native.lib()), ("diag", dcl._native._open(dcl._native.DIAG_SO_PATH))]


def test_header_declares_both_entries_and_both_libraries_export_them(dcl):
    decl = declarations()
    for name, args in WANT.items():
        assert name in decl, name
        assert decl[name] == args, (name, decl[name])
    for tag, lib in _libs(dcl):
        for name in WANT:
            assert hasattr(lib, name), (tag, name)
        assert int(lib.dcl_abi_version()) == 2, tag                      # the entry joins the ABI, the version stays
    for op in ("template_rows", "template_rows_host"):
        assert list(inspect.signature(getattr(dcl.ops, op)).parameters) == ["cache", "lut", "cls", "blocks", "miss"]
    assert inspect.signature(dcl.ops.template_rows).parameters["miss"].default is None
    assert C.sizeof(dcl.ops._TemplateBlock) == 24 and dcl.ops.TEMPLATE_MAX_BLOCKS == 8


_HOST = (C.c_int32 * 4096)()            # host memory stands in for device buffers: a refused call never dereferences them
_P = C.cast(_HOST, C.c_void_p)
_ODD = C.c_void_p(C.addressof(_HOST) + 2)


def _call(dcl, L, host, cache=_P, class_floats=8 * 16, row_floats=16, n_tmp=8, lut=_P, lut_len=4, cls=_P, b=2, blocks="one",
          nblocks=None, miss=_P, **blk):
    q = dict(src_col=0, width=4, dst=_P.value, dst_pitch=4)
    q.update(blk)
    arr = (dcl.ops._TemplateBlock * 8)()
    for j in range(8):
        arr[j].src_col, arr[j].width, arr[j].dst, arr[j].dst_pitch = q["src_col"], q["width"], q["dst"], q["dst_pitch"]
    nb = 1 if nblocks is None else nblocks
    a = (cache, class_floats, row_floats, n_tmp, lut, lut_len, cls, b, None if blocks is None else arr, nb, miss)
    return L.dcl_template_rows_host(*a) if host else L.dcl_template_rows(*(a + (None,)))


_BAD = [dict(cache=None), dict(lut=None), dict(cls=None), dict(blocks=None), dict(miss=None), dict(dst=None),
        dict(b=0), dict(n_tmp=0), dict(nblocks=0), dict(nblocks=9), dict(width=0), dict(width=-4), dict(dst_pitch=3),
        dict(src_col=13), dict(src_col=-1), dict(width=17, dst_pitch=17), dict(lut_len=-1), dict(row_floats=0),
        dict(class_floats=8 * 16 - 1), dict(cache=_ODD), dict(cls=_ODD), dict(dst=_ODD.value)]


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
@pytest.mark.parametrize("kw", _BAD, ids=lambda kw: ",".join("%s=%s" % (k, "odd" if k in ("cache", "cls", "dst") and v else v)
                                                                for k, v in sorted(kw.items())))
def test_bad_arguments_return_einval_without_a_gpu(dcl, host, kw):
    for tag, lib in _libs(dcl):
        assert _call(dcl, lib, host, **kw) == -1, tag
        assert b"invalid argument" in lib.dcl_last_error(), tag


def test_the_refused_call_is_the_only_thing_wrong_with_it(dcl):
    """the same argument list with nothing bad in it runs (host twin) -- so each refusal above is the named argument's"""
    rows = np.arange(2 * 8 * 16, dtype=np.float32).reshape(2, 8, 16)
    lut = np.array([1, -1, 0, -1], np.int32)
    cls = np.array([2, 0], np.int32)
    dst = np.full((16, 4), -1, np.float32)
    miss = np.zeros(1, np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)                                  # noqa: E731
    L = dcl._native.lib()
    assert _call(dcl, L, True, cache=vp(rows), lut=vp(lut), cls=vp(cls), miss=vp(miss), dst=dst.ctypes.data, src_col=12) == 0
    assert np.array_equal(dst.reshape(2, 8, 4), rows[[0, 1], :, 12:16]) and miss[0] == 0


@pytest.mark.parametrize("case", tc.CASES, ids=tc.case_id)
def test_host_twin_equals_plain_indexing(dcl, case):
    b, n_tmp, name, pitch = case
    want, miss_want = tc.reference(n_tmp, tc.BATCHES[b], name)
    got, miss = tc.run(dcl.ops.template_rows_host, n_tmp, tc.BATCHES[b], name, pitch, "cpu")
    assert miss == miss_want == 0
    for k in want:
        assert np.array_equal(got[k], want[k]), k                                # whole buffers: the sentinel outside the blocks too


@pytest.mark.parametrize("name", sorted(tc.BLOCK_SETS))
def test_host_twin_miss_semantics(dcl, name):
    """ids {5, 3, -1}: class 3 is inside the table but not cached, -1 is outside it -- both crops are zeros, crop 5 is exact"""
    ids = (5, 3, -1)
    want, miss_want = tc.reference(5, ids, name)
    got, miss = tc.run(dcl.ops.template_rows_host, 5, ids, name, 644, "cpu")
    assert miss == miss_want == 1
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    # an id past the table's end, as int64 on the host through the wrapper; a clean call leaves a caller's flag alone
    got, miss = tc.run(dcl.ops.template_rows_host, 5, (22, 7), name, 643, "cpu", cls=torch.tensor([22, 7], dtype=torch.int64))
    want, _ = tc.reference(5, (22, 7), name)
    assert miss == 1 and all(np.array_equal(got[k], want[k]) for k in want)
    flag = torch.zeros(1, dtype=torch.int32)
    _, miss = tc.run(dcl.ops.template_rows_host, 5, (7, 2), name, 644, "cpu", cls=[7, 2], miss=flag)
    assert miss == 0 and int(flag[0]) == 0


def test_wrapper_refuses_what_it_can_see(dcl):
    rows = tc.cache_tensor(5, 644, "cpu")
    lut = torch.from_numpy(tc.lut())
    dst = torch.zeros((10, 4))
    with pytest.raises(ValueError):
        dcl.ops.template_rows_host(rows, lut, [5, 7], [(640, dst)])              # columns 640 .. 644 of 643
    with pytest.raises(ValueError):
        dcl.ops.template_rows_host(rows, lut, [5, 7, 2], [(0, dst)])             # three crops, rows for two
    with pytest.raises(ValueError):
        dcl.ops.template_rows_host(rows, lut.long(), [5, 7], [(0, dst)])
    with pytest.raises(ValueError):
        dcl.ops.template_rows_host(rows, lut, [5, 7], [])
    with pytest.raises(RuntimeError):
        dcl.ops.template_rows(rows, lut, [5, 7], [(0, dst)])                     # the device op has no CPU fallback


def test_cache_object_and_switches_exist(dcl):
    T = dcl.DCL_Net.TemplateCache
    assert T.COLS == 643 and T.PITCH % 4 == 0 and T.PITCH >= T.COLS
    assert [(c, w) for _, c, w in T.BLOCKS] == [(0, 256), (256, 64), (320, 256), (576, 64), (640, 3)]
    net = dcl.DCL_Net.Network(dcl.synth.default_cfg(64, 64), mode="test")
    assert net.template_cache is None
    with pytest.raises(ValueError):                                              # not in training mode (a new module is in it)
        net.cache_templates({2: dcl.synth.class_template_side(2, 64)}, [64, 64, 64])
    with pytest.raises(ValueError):
        net.eval()({"tmp_cls": [2], "batch_offsets": torch.zeros(2)})            # no cache
    assert inspect.signature(dcl.crops.CropBuilder.__init__).parameters["template_ids"].default is False
    side = dcl.synth.class_template_side(5, 64)
    want = dcl.synth.make_batch(1, 64, 64, first=5)["tmp"]                       # crop 5 is of class 5
    assert sorted(side) == sorted(want) and all(torch.equal(side[k], want[k]) for k in want)
