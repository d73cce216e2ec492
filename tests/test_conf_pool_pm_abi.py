"""The point-major confidence pooling entry points (dcl_conf_pool_pm_fwd / _bwd / _bwd_ws_bytes and the two host twins) are
declared with the channel-major set's argument lists, exported by both libraries and answer bad arguments and an empty batch
without a GPU; the host twins -- the kernels' routines in the kernels' summation order -- are exact on exact operands, agree
with float64 under the project's rule, and give a crop the same bits alone as inside a batch; Network takes the `train_dense=`
switch."""
import ctypes as C
import os
import re

import pytest
import torch

import conf_pool_pm_cases as PM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_DIMS = ["int b", "int c", "int n1", "int n2"]
_FWD = ["const float *w", "const float *F1", "const float *F2", "float *pooled"]
_BWD = ["const float *conf", "const float *w", "const float *F1", "const float *F2", "const float *g_pooled",
        "const float *g_conf", "float *dlogit1", "float *dlogit2", "float *dF1", "float *dF2"]
_S = ["dclStream_t stream"]

WANT = {
    "dcl_conf_pool_pm_fwd": _DIMS + _FWD + _S,
    "dcl_conf_pool_pm_bwd_ws_bytes": _DIMS + ["int64_t *bytes_host"],
    "dcl_conf_pool_pm_bwd": _DIMS + _BWD + ["void *ws", "int64_t ws_bytes"] + _S,
    "dcl_conf_pool_pm_fwd_host": _DIMS + _FWD,
    "dcl_conf_pool_pm_bwd_host": _DIMS + _BWD,
}
_IN = ("conf", "w", "F1", "F2", "g_pooled", "g_conf")


def declarations():
    text = open(os.path.join(ROOT, "include", "dclnet_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for m in re.finditer(r"\bint\s+(dcl_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        out[m.group(1)] = [re.sub(r"\s+", " ", a).strip() for a in m.group(2).split(",")]
    return out


def test_header_declares_the_five_entry_points_with_the_channel_major_argument_lists():
    decl = declarations()
    for name, args in WANT.items():
        assert name in decl, name
        assert decl[name] == args, (name, decl[name])
        assert decl[name] == decl[name.replace("_pm_", "_cm_")], name
    text = open(os.path.join(ROOT, "include", "dclnet_hip.h")).read()
    assert re.search(r"#define DCL_ABI_VERSION 2\b", text)
    m = re.search(r"#define DCL_POOL_PM_ROWS (\d+)\b", text)
    assert m and int(m.group(1)) == PM.POOL_PM_ROWS
    section = text[text.index("confidence pooling, point-major"):]
    assert "PINNED ORDER" in section and "DCL_POOL_PM_ROWS" in section and "strides 32" in section


def _libs(dcl):
    assert os.path.exists(dcl._native.DIAG_SO_PATH), "diagnostic library missing: build() makes it"
    return [("product", dcl._native.lib()), ("diag", dcl._native._open(dcl._native.DIAG_SO_PATH))]


def test_both_libraries_export_them_and_the_python_layers_exist(dcl):
    for tag, lib in _libs(dcl):
        for name in WANT:
            assert hasattr(lib, name), (tag, name)
    for fn in ("conf_pool_pm", "conf_pool_pm_backward"):
        assert callable(getattr(dcl.ops, fn)) and callable(getattr(dcl.ops, fn + "_host")), fn
    assert hasattr(dcl.autograd.ConfPoolPmFn, "apply") and hasattr(dcl.autograd.PointLinearFn, "apply")
    assert dcl.ops.POOL_PM_ROWS == PM.POOL_PM_ROWS
    assert dcl.DCL_Net.TRAIN_DENSE_MODES == ("modules", "point_major")


_BUF = (C.c_char * 64)()                 # host bytes standing in for buffers: a rejected call never dereferences them
_P = C.cast(_BUF, C.c_void_p)


def _call(lib, name, **over):
    """one call with every pointer set, an ample ws_bytes, and `over` applied on top"""
    vals = {"b": 2, "c": 3, "n1": 5, "n2": 7, "ws_bytes": 1 << 20, "bytes_host": C.pointer(C.c_int64(0))}
    vals.update(over)
    args = []
    for a in WANT[name]:
        key = a.split("*")[-1].split()[-1]
        args.append(vals[key] if key in vals else (None if key == "stream" else _P))
    return getattr(lib, name)(*args)


BAD = []
for _n in WANT:
    BAD += [(_n, dict(b=-1)), (_n, dict(c=0)), (_n, dict(n1=0)), (_n, dict(n2=0)), (_n, dict(n1=-3))]
for _n in ("dcl_conf_pool_pm_fwd", "dcl_conf_pool_pm_fwd_host"):
    BAD += [(_n, {k: None}) for k in ("w", "F1", "F2", "pooled")]
for _n in ("dcl_conf_pool_pm_bwd", "dcl_conf_pool_pm_bwd_host"):
    BAD += [(_n, {k: None}) for k in ("conf", "w", "F1", "F2", "g_pooled")]
    # a half pair of outputs, and no output at all
    BAD += [(_n, {k: None}) for k in ("dlogit1", "dlogit2", "dF1", "dF2")]
    BAD += [(_n, dict(dlogit1=None, dlogit2=None, dF1=None, dF2=None))]
BAD += [("dcl_conf_pool_pm_bwd_ws_bytes", dict(bytes_host=None)),
        ("dcl_conf_pool_pm_bwd", dict(ws=None)), ("dcl_conf_pool_pm_bwd", dict(ws_bytes=0)),
        # one byte short of what the query asks for: 2 crops x 12 values of d
        ("dcl_conf_pool_pm_bwd", dict(ws_bytes=2 * 12 * 4 - 1))]


@pytest.mark.parametrize("name,over", BAD, ids=["%s-%s" % (n[17:], "-".join(sorted(o))) for n, o in BAD])
def test_bad_arguments_return_einval_without_a_gpu(dcl, name, over):
    for tag, lib in _libs(dcl):
        assert _call(lib, name, **dict(over)) == -1, tag
        assert b"invalid argument" in lib.dcl_last_error(), tag


def test_an_empty_batch_is_not_an_error_and_the_scratch_query_is_consistent(dcl):
    for tag, lib in _libs(dcl):
        for name in WANT:
            assert _call(lib, name, b=0) == 0, (tag, name)
        q = C.c_int64(-1)
        assert _call(lib, "dcl_conf_pool_pm_bwd_ws_bytes", bytes_host=C.pointer(q)) == 0 and q.value == 2 * 12 * 4, tag
        # d alone: one float per logit, whatever C is
        for c in (1, 130, 600):
            assert _call(lib, "dcl_conf_pool_pm_bwd_ws_bytes", b=3, c=c, n1=257, n2=64, bytes_host=C.pointer(q)) == 0
            assert q.value == 3 * 321 * 4, (tag, c)
        assert _call(lib, "dcl_conf_pool_pm_bwd_ws_bytes", b=0, bytes_host=C.pointer(q)) == 0 and q.value == 0, tag
        # beyond 32 bits
        assert _call(lib, "dcl_conf_pool_pm_bwd_ws_bytes", b=1 << 20, c=4, n1=1 << 10, n2=1 << 10, bytes_host=C.pointer(q)) == 0
        assert q.value == (1 << 20) * (1 << 11) * 4, tag


def test_network_takes_the_train_dense_switch(dcl):
    cfg = dcl.synth.default_cfg(64, 64)
    assert dcl.DCL_Net.Network(cfg).train_dense == "modules"
    net = dcl.DCL_Net.Network(cfg, train_dense="point_major", train_attention="fused")
    assert net.train_dense == "point_major"
    assert list(net.state_dict().keys()) == list(dcl.DCL_Net.Network(cfg).state_dict().keys())
    with pytest.raises(ValueError, match="train_attention"):
        dcl.DCL_Net.Network(cfg, train_dense="point_major")
    with pytest.raises(ValueError, match="train_attention"):
        dcl.DCL_Net.Network(cfg, train_dense="point_major", train_attention="materialised")
    with pytest.raises(ValueError, match="train_dense"):
        dcl.DCL_Net.Network(cfg, train_dense="x", train_attention="fused")
    text = open(os.path.join(ROOT, "tools", "train_step.py")).read()
    assert "--dense" in text and "train_dense=args.dense" in text and "--attention" in text


def test_the_functions_refuse_cpu_tensors_with_a_clear_error(dcl):
    k = PM.random_case(1)
    with pytest.raises(RuntimeError, match=r"GPU only.*'modules'"):
        dcl.autograd.ConfPoolPmFn.apply(k["logit1"], k["logit2"], k["F1"], k["F2"])
    with pytest.raises(RuntimeError, match="GPU"):
        dcl.ops.conf_pool_pm(k["w"], k["F1"], k["F2"])
    with pytest.raises(RuntimeError, match="GPU"):
        dcl.ops.conf_pool_pm_backward(k["conf"], k["w"], k["F1"], k["F2"], k["g_pooled"])
    with pytest.raises(RuntimeError, match="CUDA"):
        dcl.autograd.PointLinearFn.apply(torch.zeros(4, 32), torch.zeros(32, 32, 1), None, False)


def _host(dcl, k, g_conf):
    out = {"pooled": dcl.ops.conf_pool_pm_host(k["w"], k["F1"], k["F2"])}
    got = dcl.ops.conf_pool_pm_backward_host(k["conf"], k["w"], k["F1"], k["F2"], k["g_pooled"], g_conf)
    out.update(zip(("dlogit1", "dlogit2", "dF1", "dF2"), got))
    return out


@pytest.mark.parametrize("i", [0, 1, 2, 3, 5], ids=PM.IDS[:4] + PM.IDS[5:6])
def test_host_twins_against_float64(dcl, i):
    """conf and w from torch's fp32 sigmoid / softmax; err_module = the error of the four torch lines in fp32"""
    k = PM.random_case(i)
    PM.compare(PM.IDS[i], _host(dcl, k, k["g_conf"]), PM.formulas64(k, k["g_conf"]), PM.module_refs(i)[1], PM.OUTPUTS)


@pytest.mark.parametrize("with_g_conf", [True, False], ids=["g_conf", "no_g_conf"])
@pytest.mark.parametrize("i", range(len(PM.SHAPES)), ids=PM.IDS)
def test_host_twins_are_exact_on_exact_operands(dcl, i, with_g_conf):
    """every sum is exact, so fp32 in any order equals float64: a dropped or doubled element shows"""
    k = PM.exact_case(i)
    g_conf = k["g_conf"] if with_g_conf else None
    ref = PM.formulas64(k, g_conf)
    got = _host(dcl, k, g_conf)
    for name in PM.OUTPUTS:
        assert bool((got[name].double() == ref[name]).all()), (PM.IDS[i], name, float((got[name].double() - ref[name]).abs().max()))


@pytest.mark.parametrize("i", [2, 3], ids=PM.IDS[2:4])
def test_a_crop_gives_the_same_bits_alone_as_inside_a_batch_on_the_host_twins(dcl, i):
    k = PM.random_case(i)
    full = _host(dcl, k, k["g_conf"])
    b, _, n1, n2 = PM.SHAPES[i]
    for c in range(b):
        one = PM.crop(k, c, _IN)
        alone = _host(dcl, one, one["g_conf"])
        for name in PM.OUTPUTS:
            per = {"dF1": n1, "dF2": n2}.get(name, 1)
            assert PM.same_bits(alone[name], full[name][c * per:(c + 1) * per]), (c, name)


def test_selective_outputs_on_the_host_twin(dcl):
    k = PM.random_case(2)
    full = _host(dcl, k, k["g_conf"])
    dl1, dl2, dF1, dF2 = dcl.ops.conf_pool_pm_backward_host(k["conf"], k["w"], k["F1"], k["F2"], k["g_pooled"], k["g_conf"],
                                                            need_F=False)
    assert dF1 is None and dF2 is None and PM.same_bits(dl1, full["dlogit1"]) and PM.same_bits(dl2, full["dlogit2"])
    dl1, dl2, dF1, dF2 = dcl.ops.conf_pool_pm_backward_host(k["conf"], k["w"], k["F1"], k["F2"], k["g_pooled"], k["g_conf"],
                                                            need_logits=False)
    assert dl1 is None and dl2 is None and PM.same_bits(dF1, full["dF1"]) and PM.same_bits(dF2, full["dF2"])
