"""The optimizer-step entry points (dcl_grad_sqnorm, dcl_adam_step) are declared with the documented argument lists, exported
by both libraries and answer bad arguments and an empty table without a GPU; dcl.optim.Adam refuses what it does not
implement with a clear error; AutoClip's host arithmetic is the reference's."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WANT = {
    "dcl_grad_sqnorm": ["int n_tensors", "const dclOptimTensor *table", "int n_chunks", "const int32_t *chunk_tensor",
                        "const int64_t *chunk_begin", "double *partials", "double *sq_per_tensor", "double *norm",
                        "dclStream_t stream"],
    "dcl_adam_step": ["int n_tensors", "const dclOptimTensor *table", "int n_chunks", "const int32_t *chunk_tensor",
                      "const int64_t *chunk_begin", "float grad_scale", "float beta1", "float beta2", "float eps",
                      "dclStream_t stream"],
}
FIELDS = ["float *param", "const float *grad", "float *exp_avg", "float *exp_avg_sq", "int64_t numel", "float step_size",
          "float bc2_sqrt"]


def _header():
    return open(os.path.join(ROOT, "include", "dclnet_hip.h")).read()


def test_header_declares_the_entry_points_and_the_table_row(dcl):
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    decl = {}
    for m in re.finditer(r"\bint\s+(dcl_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        decl[m.group(1)] = [re.sub(r"\s+", " ", a).strip() for a in m.group(2).split(",")]
    for name, args in WANT.items():
        assert name in decl, name
        assert decl[name] == args, (name, decl[name])
    m = re.search(r"typedef struct dclOptimTensor \{(.*?)\} dclOptimTensor;", text, flags=re.S)
    assert m, "dclOptimTensor is not declared"
    assert [re.sub(r"\s+", " ", f).strip() for f in m.group(1).split(";") if f.strip()] == FIELDS
    assert re.search(r"#define DCL_ABI_VERSION 2\b", text)
    assert re.search(r"#define DCL_OPTIM_CHUNK 4096\b", text) and dcl.ops.OPTIM_CHUNK == 4096
    # the Python side packs the same row
    dt = dcl.optim.TENSOR_DTYPE
    assert list(dt.names) == [f.split()[-1].lstrip("*") for f in FIELDS]
    assert dt.itemsize == dcl.ops.OPTIM_TENSOR_BYTES == 48
    assert [dt.fields[n][1] for n in dt.names] == [0, 8, 16, 24, 32, 40, 44]


def test_the_header_states_the_order_of_operations():
    text = re.sub(r"[ \t]+", " ", _header())
    for line in ("g' = g * grad_scale", "m = m*beta1 + g'*omb1", "v = v*beta2 + (g'*g')*omb2", "d = sqrtf(v)/bc2_sqrt + eps",
                 "p = p - step_size*(m/d)"):
        assert line in text, line


def _libs(dcl):
    assert os.path.exists(dcl._native.DIAG_SO_PATH), "diagnostic library missing: build() makes it"
    return [("product", dcl._native.lib()), ("diag", C.CDLL(dcl._native.DIAG_SO_PATH))]


def test_both_libraries_export_them_and_the_python_layers_exist(dcl):
    for tag, lib in _libs(dcl):
        for name in WANT:
            assert hasattr(lib, name), (tag, name)
    assert callable(dcl.ops.grad_sqnorm) and callable(dcl.ops.adam_step)
    assert issubclass(dcl.optim.Adam, torch.optim.Optimizer) and callable(dcl.optim.AutoClip)


_BUF = (C.c_char * 64)()                 # host bytes standing in for device buffers: a rejected call never dereferences them
_P = C.cast(_BUF, C.c_void_p)
f32 = C.c_float


def _norm(L, n_tensors=2, n_chunks=3, table=_P, chunk_tensor=_P, chunk_begin=_P, partials=_P, sq=_P, norm=_P):
    return L.dcl_grad_sqnorm(n_tensors, table, n_chunks, chunk_tensor, chunk_begin, partials, sq, norm, None)


def _adam(L, n_tensors=2, n_chunks=3, table=_P, chunk_tensor=_P, chunk_begin=_P, grad_scale=1.0, beta1=0.5, beta2=0.999,
          eps=1e-6):
    return L.dcl_adam_step(n_tensors, table, n_chunks, chunk_tensor, chunk_begin, f32(grad_scale), f32(beta1), f32(beta2),
                           f32(eps), None)


@pytest.mark.parametrize("call", [
    lambda L: _norm(L, n_tensors=-1),
    lambda L: _norm(L, n_chunks=-1),
    lambda L: _norm(L, n_tensors=4, n_chunks=3),
    lambda L: _norm(L, table=None),
    lambda L: _norm(L, chunk_tensor=None),
    lambda L: _norm(L, chunk_begin=None),
    lambda L: _norm(L, partials=None),
    lambda L: _norm(L, sq=None),
    lambda L: _norm(L, norm=None),
    lambda L: _adam(L, n_tensors=-1),
    lambda L: _adam(L, n_chunks=-1),
    lambda L: _adam(L, n_tensors=4, n_chunks=3),
    lambda L: _adam(L, table=None),
    lambda L: _adam(L, chunk_tensor=None),
    lambda L: _adam(L, chunk_begin=None),
    lambda L: _adam(L, grad_scale=float("inf")),
    lambda L: _adam(L, grad_scale=float("-inf")),
    lambda L: _adam(L, grad_scale=float("nan")),
    lambda L: _adam(L, beta1=1.0),
    lambda L: _adam(L, beta1=-0.1),
    lambda L: _adam(L, beta1=float("nan")),
    lambda L: _adam(L, beta2=1.0),
    lambda L: _adam(L, beta2=-1e-3),
    lambda L: _adam(L, beta2=1.5),
    lambda L: _adam(L, eps=0.0),
    lambda L: _adam(L, eps=-1e-8),
    lambda L: _adam(L, eps=float("nan")),
])
def test_bad_arguments_return_einval_without_a_gpu(dcl, call):
    for tag, lib in _libs(dcl):
        lib.dcl_last_error.restype = C.c_char_p
        assert call(lib) == -1, tag
        assert b"invalid argument" in lib.dcl_last_error(), tag


def test_an_empty_table_is_not_an_error(dcl):
    for tag, lib in _libs(dcl):
        assert _norm(lib, n_tensors=0, n_chunks=0) == 0, tag
        assert _norm(lib, n_tensors=0, n_chunks=0, table=None, chunk_tensor=None, chunk_begin=None, partials=None, sq=None,
                     norm=None) == 0, tag
        assert _adam(lib, n_tensors=0, n_chunks=0) == 0, tag
        assert _adam(lib, n_tensors=0, n_chunks=0, table=None, chunk_tensor=None, chunk_begin=None) == 0, tag


def test_the_chunk_table_covers_every_element_once(dcl):
    numels = [1, 3, 5, 4095, 4096, 4097, 3 * 4096 + 7, 884736]
    ct, cb = dcl.optim.chunk_table(numels)
    assert ct.dtype == np.int32 and cb.dtype == np.int64 and len(ct) == len(cb) == sum((n + 4095) // 4096 for n in numels)
    assert (np.diff(ct) >= 0).all()
    for t, n in enumerate(numels):
        assert cb[ct == t].tolist() == list(range(0, n, 4096))
    # two groups: each group's launch indexes its own slice of the tensor table
    lay = dcl.optim._Layout(numels, [3, 0, 5])
    assert lay.groups == [(0, 3, 0, 3), (3, 5, 3, len(ct) - 3)]
    rel = lay.template[lay.off_rel:lay.off_rel + 4 * len(ct)].view(np.int32)
    assert rel[:3].tolist() == [0, 1, 2] and rel[3] == 0 and rel[-1] == 4
    assert lay.off_ct % 16 == 0 and lay.off_cb % 16 == 0 and lay.off_rel % 16 == 0


def test_bias_corrections_are_evaluated_in_double_and_rounded_once(dcl):
    t = np.array([1, 2, 7, 1000])
    step_size, bc2 = dcl.optim.bias_corrections(1e-3, 0.5, 0.999, t)
    assert step_size.dtype == np.float32 and bc2.dtype == np.float32
    for i, ti in enumerate(t.tolist()):
        assert step_size[i] == np.float32(1e-3 / (1.0 - 0.5 ** ti))
        assert bc2[i] == np.float32(np.sqrt(1.0 - 0.999 ** ti))


def test_adam_refuses_what_it_does_not_implement(dcl):
    w = lambda: torch.nn.Parameter(torch.zeros(4, 3))                    # noqa: E731
    with pytest.raises(RuntimeError, match="GPU"):
        dcl.optim.Adam([w()], lr=1e-3)
    with pytest.raises(ValueError, match="weight_decay"):
        dcl.optim.Adam([w()], weight_decay=1e-4)
    with pytest.raises(ValueError, match="amsgrad"):
        dcl.optim.Adam([w()], amsgrad=True)
    with pytest.raises(ValueError, match="maximize"):
        dcl.optim.Adam([w()], maximize=True)
    with pytest.raises(ValueError, match="weight_decay"):
        dcl.optim.Adam([{"params": [w()], "weight_decay": 1e-2}])
    with pytest.raises(TypeError, match="float32"):
        dcl.optim.Adam([torch.nn.Parameter(torch.zeros(4, 3).half())])
    with pytest.raises(TypeError, match="contiguous"):
        dcl.optim.Adam([torch.nn.Parameter(torch.zeros(4, 3).t())])
    with pytest.raises(ValueError):
        dcl.optim.Adam([w()], eps=0.0)
    with pytest.raises(ValueError):
        dcl.optim.Adam([w()], betas=(1.0, 0.999))
    with pytest.raises(TypeError, match="dcl.optim.Adam"):
        dcl.optim.AutoClip(50, optimizer=torch.optim.Adam([w()]))


def test_autoclip_host_arithmetic_is_the_references(dcl):
    norms = [3.0, 1.5, 8.0, 0.25, 2.0, 2.0, 40.0, 1e-9]
    for pct in (50, 10, 90):
        clip = dcl.optim.AutoClip(pct)
        for i, n in enumerate(norms):
            scale = clip.observe(n)
            want_clip = float(np.percentile(norms[:i + 1], pct))
            assert clip.clip_value == want_clip
            assert scale == min(1.0, want_clip / (n + 1e-6))
            assert clip.history == norms[:i + 1]
    first = dcl.optim.AutoClip(50)
    assert first.observe(3.0) == 3.0 / (3.0 + 1e-6) < 1.0
    # the history travels with a checkpoint
    sd = clip.state_dict()
    again = dcl.optim.AutoClip(1)
    again.load_state_dict(sd)
    assert again.history == norms and again.percentile == 90
    assert again.observe(5.0) == min(1.0, float(np.percentile(norms + [5.0], 90)) / (5.0 + 1e-6))
