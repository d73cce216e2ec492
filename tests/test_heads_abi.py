"""The entry points behind train_heads="kernels" -- the narrow per-point layer (dcl_linear_narrow_*) and the two pose heads in
training (dcl_pose_heads_train_*) -- are declared with the stated argument lists, exported by both libraries and answer bad
arguments and an empty batch without a GPU; the host twins -- the kernels' routines in the kernels' summation orders -- are
exact on exact operands, agree with float64 under the project's rule and give a crop the same bits alone as inside a batch;
Network and Refiner take the `train_heads=` switch."""
import ctypes as C
import os
import re

import pytest
import torch

import heads_cases as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_LN = ["int64_t M", "int K", "int N", "const float *x", "int64_t x_pitch", "const float *W"]
_LN_BWD = _LN + ["const float *g", "float *dx", "float *dW", "float *db"]
_S = ["dclStream_t stream"]
_WS = ["void *ws", "int64_t ws_bytes"]
_PH = ["int b", "int d0", "int d1", "int d2", "int n_rot", "int n_trans"]
_PH_FWD = ["const float *x"] + ["const float *%s%s%d" % (h, t, l) for h in "rt" for l in range(3) for t in "Wb"] + \
    ["float *h1", "float *h2", "float *o9", "float *t3"]
_PH_BWD = ["const float *x"] + ["const float *%sW%d" % (h, l) for h in "rt" for l in range(3)] + \
    ["const float *h1", "const float *h2", "const float *g_o9", "const float *g_t3", "float *dx"] + \
    ["float *d_%s%s%d" % (h, t, l) for h in "rt" for l in range(3) for t in "Wb"]

WANT = {
    "dcl_linear_narrow_fwd": _LN + ["const float *bias", "float *y"] + _S,
    "dcl_linear_narrow_fwd_host": _LN + ["const float *bias", "float *y"],
    "dcl_linear_narrow_bwd_ws_bytes": ["int64_t M", "int K", "int N", "int64_t *bytes_host"],
    "dcl_linear_narrow_bwd": _LN_BWD + _WS + _S,
    "dcl_linear_narrow_bwd_host": _LN_BWD,
    "dcl_pose_heads_train_fwd": _PH + _PH_FWD + _S,
    "dcl_pose_heads_train_fwd_host": _PH + _PH_FWD,
    "dcl_pose_heads_train_bwd_ws_bytes": _PH + ["int64_t *bytes_host"],
    "dcl_pose_heads_train_bwd": _PH + _PH_BWD + _WS + _S,
    "dcl_pose_heads_train_bwd_host": _PH + _PH_BWD,
}
NARROW = [n for n in WANT if "narrow" in n]
POSE = [n for n in WANT if "pose" in n]


def declarations():
    text = open(os.path.join(ROOT, "include", "dclnet_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for m in re.finditer(r"\bint\s+(dcl_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        out[m.group(1)] = [re.sub(r"\s+", " ", a).strip() for a in m.group(2).split(",")]
    return out


def test_header_declares_the_entry_points_and_documents_the_pinned_orders():
    decl = declarations()
    for name, args in WANT.items():
        assert name in decl, name
        assert decl[name] == args, (name, decl[name])
    text = open(os.path.join(ROOT, "include", "dclnet_hip.h")).read()
    assert re.search(r"#define DCL_ABI_VERSION 2\b", text)
    m = re.search(r"#define DCL_NARROW_MAX_N (\d+)\b", text)
    assert m and int(m.group(1)) == H.NARROW_MAX_N and H.NARROW_MAX_N >= 9
    m = re.search(r"#define DCL_NARROW_ROWS (\d+)\b", text)
    assert m and int(m.group(1)) == H.NARROW_ROWS
    for title, words in (("narrow per-point layer", ("DCL_NARROW_ROWS", "strides 8", "DCL_EINVAL")),
                         ("two pose heads in training", ("DCL_POSE_TRAIN_CHUNK", "strides 32", "DCL_EINVAL", "eval kernels"))):
        section = text[text.index(title):]
        section = section[:section.index("*/")]
        assert "PINNED ORDER" in section, title
        for w in words:
            assert w in section, (title, w)


def _libs(dcl):
    assert os.path.exists(dcl._native.DIAG_SO_PATH), "diagnostic library missing: build() makes it"
    return [("product", dcl._native.lib()), ("diag", dcl._native._open(dcl._native.DIAG_SO_PATH))]


def test_both_libraries_export_them_and_the_python_layers_exist(dcl):
    for tag, lib in _libs(dcl):
        for name in WANT:
            assert hasattr(lib, name), (tag, name)
    for fn in ("linear_narrow", "linear_narrow_backward", "pose_heads_train", "pose_heads_train_backward"):
        assert callable(getattr(dcl.ops, fn)) and callable(getattr(dcl.ops, fn + "_host")), fn
    assert hasattr(dcl.autograd.NarrowLinearFn, "apply") and hasattr(dcl.autograd.PoseHeadsFn, "apply")
    assert (dcl.ops.NARROW_MAX_N, dcl.ops.NARROW_ROWS) == (H.NARROW_MAX_N, H.NARROW_ROWS)
    assert dcl.DCL_Net.TRAIN_HEADS_MODES == ("modules", "kernels") and callable(dcl.DCL_Net.check_train_heads)


_BUF = (C.c_char * 4160)()               # host bytes standing in for buffers: a rejected call never dereferences them
_P = C.c_void_p((C.addressof(_BUF) + 63) // 64 * 64)

_DEFAULT = {"M": 5, "K": 7, "N": 3, "x_pitch": 7, "b": 2, "d0": 16, "d1": 8, "d2": 4, "n_rot": 9, "n_trans": 3,
            "ws_bytes": 1 << 30}


def _call(lib, name, **over):
    """one call with every pointer set (64-byte aligned), an ample ws_bytes, and `over` applied on top"""
    vals = dict(_DEFAULT, bytes_host=C.pointer(C.c_int64(0)))
    vals.update(over)
    args = []
    for a in WANT[name]:
        key = a.split("*")[-1].split()[-1]
        args.append(vals[key] if key in vals else (None if key == "stream" else _P))
    return getattr(lib, name)(*args)


_PH_OUTS = ["dx"] + ["d_%s%s%d" % (h, t, l) for h in "rt" for l in range(3) for t in "Wb"]
BAD = []
for _n in NARROW:
    BAD += [(_n, dict(M=-1)), (_n, dict(K=0)), (_n, dict(K=-4)), (_n, dict(N=0)), (_n, dict(N=H.NARROW_MAX_N + 1))]
for _n in NARROW[:2] + NARROW[3:]:
    BAD += [(_n, {k: None}) for k in ("x", "W")] + [(_n, dict(x_pitch=6))]
for _n in NARROW[:2]:
    BAD += [(_n, dict(y=None))]
for _n in NARROW[3:]:
    BAD += [(_n, dict(g=None)), (_n, dict(dx=None, dW=None, db=None))]
# the scratch holds the chunks' partials: one chunk of 3 x 7 + 3 floats, padded to whole vectors
BAD += [("dcl_linear_narrow_bwd_ws_bytes", dict(bytes_host=None)), ("dcl_linear_narrow_bwd", dict(ws=None)),
        ("dcl_linear_narrow_bwd", dict(ws_bytes=24 * 4 - 1))]
for _n in POSE:
    BAD += [(_n, dict(b=-1)), (_n, dict(d0=0)), (_n, dict(d1=-8)), (_n, dict(d2=6)), (_n, dict(d0=2048)), (_n, dict(n_rot=0)),
            (_n, dict(n_trans=17))]
for _n in POSE[:2]:
    BAD += [(_n, {k: None}) for k in ("x", "rW0", "rb1", "tW2", "tb0", "h1", "h2", "o9", "t3")]
for _n in POSE[3:]:
    BAD += [(_n, {k: None}) for k in ("x", "rW0", "tW1", "h1", "h2")]
    BAD += [(_n, dict(g_o9=None, g_t3=None)), (_n, {k: None for k in _PH_OUTS})]
# dz2, dz1 of both heads and the largest layer's chunk partials: 2 (2 x 4 + 2 x 8 + 2 x 1 x 16) floats
BAD += [("dcl_pose_heads_train_bwd_ws_bytes", dict(bytes_host=None)), ("dcl_pose_heads_train_bwd", dict(ws=None)),
        ("dcl_pose_heads_train_bwd", dict(ws_bytes=2 * (8 + 16 + 32) * 4 - 1))]


@pytest.mark.parametrize("name,over", BAD, ids=["%s-%s" % (n[4:], "-".join("%s=%s" % kv for kv in sorted(o.items()))[:60])
                                                for n, o in BAD])
def test_bad_arguments_return_einval_without_a_gpu(dcl, name, over):
    for tag, lib in _libs(dcl):
        assert _call(lib, name, **dict(over)) == -1, tag
        assert b"invalid argument" in lib.dcl_last_error(), tag


def test_an_empty_batch_is_not_an_error_and_the_scratch_queries_are_consistent(dcl):
    for tag, lib in _libs(dcl):
        for name in WANT:
            assert _call(lib, name, M=0, b=0) == 0, (tag, name)
        q = C.c_int64(-1)
        ask = lambda name, **kw: _call(lib, name, bytes_host=C.pointer(q), **kw)               # noqa: E731
        assert ask("dcl_linear_narrow_bwd_ws_bytes") == 0 and q.value == 24 * 4, tag
        assert ask("dcl_linear_narrow_bwd_ws_bytes", M=0) == 0 and q.value == 0, tag
        # a chunk's partials are dW and db, padded to whole 16-byte vectors; one chunk per NARROW_ROWS rows
        for M, K, N in ((H.NARROW_ROWS, 128, 3), (H.NARROW_ROWS + 1, 128, 3), (513, 130, 9)):
            chunks, floats = -(-M // H.NARROW_ROWS), -(-(N * K + N) // 4) * 4
            assert ask("dcl_linear_narrow_bwd_ws_bytes", M=M, K=K, N=N) == 0 and q.value == chunks * floats * 4, (tag, M, K, N)
        # beyond 32 bits
        assert ask("dcl_linear_narrow_bwd_ws_bytes", M=1 << 31, K=128, N=3) == 0
        assert q.value == ((1 << 31) // H.NARROW_ROWS) * 388 * 4 and q.value > 1 << 32, tag
        assert ask("dcl_pose_heads_train_bwd_ws_bytes") == 0 and q.value == 2 * (8 + 16 + 32) * 4, tag
        assert ask("dcl_pose_heads_train_bwd_ws_bytes", b=0) == 0 and q.value == 0, tag
        d0, d1, d2, nr, nt = H.WIDTHS
        for b in (1, 33, 1 << 20):
            assert ask("dcl_pose_heads_train_bwd_ws_bytes", b=b, d0=d0, d1=d1, d2=d2, n_rot=nr, n_trans=nt) == 0
            # layer 1 is the largest: 512 / 32 chunks of (b, 1024) per head
            assert q.value == 2 * b * (d2 + d1 + (d1 // 32) * d0) * 4, (tag, b)
        assert q.value > 1 << 32


def test_the_switch_on_network_refiner_and_the_training_tool(dcl):
    cfg = dcl.synth.default_cfg(64, 64)
    Network, Refiner = dcl.DCL_Net.Network, dcl.refiner.Refiner
    assert Network(cfg).train_heads == "modules" and Refiner().train_heads == "modules"
    net = Network(cfg, train_heads="kernels", train_dense="point_major", train_attention="fused")
    assert net.train_heads == "kernels"
    assert list(net.state_dict().keys()) == list(Network(cfg).state_dict().keys())
    assert [n for n, _ in net.named_buffers()] == [n for n, _ in Network(cfg).named_buffers()]
    with pytest.raises(ValueError, match="train_dense"):
        Network(cfg, train_heads="kernels")
    with pytest.raises(ValueError, match="train_dense"):
        Network(cfg, train_heads="kernels", train_dense="modules", train_attention="fused")
    with pytest.raises(ValueError, match="train_heads"):
        Network(cfg, train_heads="x", train_dense="point_major", train_attention="fused")
    for mlp in Refiner.TRAIN_MLP_MODES:
        ref = Refiner(train_mlp=mlp, train_heads="kernels")
        assert ref.train_heads == "kernels" and list(ref.state_dict().keys()) == list(Refiner().state_dict().keys())
    with pytest.raises(ValueError, match="train_heads"):
        Refiner(train_heads="fused")
    text = open(os.path.join(ROOT, "tools", "train_step.py")).read()
    assert "--heads" in text and "train_heads=args.heads" in text and "--dense" in text and "train_dense=args.dense" in text
    assert "--heads" in open(os.path.join(ROOT, "tools", "bench_refiner_grad.py")).read()
    assert os.path.exists(os.path.join(ROOT, "tools", "bench_heads.py"))


def test_the_functions_refuse_cpu_tensors_with_a_clear_error(dcl):
    k = H.narrow_case(2)
    with pytest.raises(RuntimeError, match=r"CUDA.*'modules'"):
        dcl.autograd.NarrowLinearFn.apply(k["x"], k["W"], k["bias"])
    with pytest.raises(RuntimeError, match="GPU"):
        dcl.ops.linear_narrow(k["x"], k["W"], k["bias"])
    with pytest.raises(RuntimeError, match="GPU"):
        dcl.ops.linear_narrow_backward(k["x"], k["W"], k["g"])
    p = H.pose_case(1)
    with pytest.raises(RuntimeError, match=r"CUDA.*'modules'"):
        dcl.autograd.PoseHeadsFn.apply(p["x"], *H.pose_params(p))
    with pytest.raises(RuntimeError, match="GPU"):
        dcl.ops.pose_heads_train(p["x"], H.pose_params(p))
    with pytest.raises(ValueError, match="N = 17"):
        dcl.ops.linear_narrow_host(torch.zeros(4, 8), torch.zeros(17, 8))


# ---------------------------------------------------------------------------------------------------- host twins
def narrow_host(dcl, k, form="dense"):
    x = H.narrow_x(k["x"], form)
    out = {"y": dcl.ops.linear_narrow_host(x, k["W"], k["bias"])}
    dx, dW, db = dcl.ops.linear_narrow_backward_host(x, k["W"], k["g"])
    out.update(dx=dx, dW=dW.view_as(k["W"]), db=db)
    return out


def pose_host(dcl, k):
    o9, t3, h1, h2 = dcl.ops.pose_heads_train_host(k["x"], H.pose_params(k))
    dx, grads = dcl.ops.pose_heads_train_backward_host(k["x"], H.pose_params(k), h1, h2, k["g_o9"], k["g_t3"])
    out = {"o9": o9, "t3": t3, "dx": dx, "h1": h1, "h2": h2}
    out.update({"d_" + n: g for n, g in zip(H.PARAMS, grads)})
    return out


@pytest.mark.parametrize("i", range(len(H.NARROW_SHAPES)), ids=H.NARROW_IDS)
def test_narrow_host_twin_against_float64(dcl, i):
    k = H.narrow_case(i)
    ref = H.narrow_form(k, torch.float64)
    H.compare(H.NARROW_IDS[i], narrow_host(dcl, k), ref, H.narrow_form(k, torch.float32), ref, H.NARROW_OUT)


@pytest.mark.parametrize("form", H.NARROW_FORMS)
@pytest.mark.parametrize("i", range(len(H.NARROW_SHAPES)), ids=H.NARROW_IDS)
def test_narrow_host_twin_is_exact_on_exact_operands_in_every_form(dcl, i, form):
    """every sum is exact, so fp32 in any order equals float64: a dropped or doubled element shows"""
    k = H.narrow_case(i, exact=True)
    ref, got = H.narrow_form(k, torch.float64), narrow_host(dcl, k, form)
    for name in H.NARROW_OUT:
        assert bool((got[name].double() == ref[name]).all()), (name, float((got[name].double() - ref[name]).abs().max()))


@pytest.mark.parametrize("i", [3, 4], ids=H.NARROW_IDS[3:5])
def test_narrow_host_twin_gives_the_same_bits_for_any_pitch_and_alignment_and_for_each_subset(dcl, i):
    k = H.narrow_case(i)
    full = narrow_host(dcl, k)
    for form in H.NARROW_FORMS[1:]:
        got = narrow_host(dcl, k, form)
        for name in H.NARROW_OUT:
            assert H.same_bits(got[name], full[name]), (form, name)
    for need in ((True, False, False), (False, True, False), (False, False, True), (True, False, True)):
        got = dcl.ops.linear_narrow_backward_host(k["x"], k["W"], k["g"], *need)
        for name, g, want in zip(("dx", "dW", "db"), got, need):
            assert (g is not None) == want and (g is None or H.same_bits(g.reshape(full[name].shape), full[name])), (need, name)
    assert H.same_bits(dcl.ops.linear_narrow_host(k["x"], k["W"], None) + k["bias"], full["y"])      # the bias is added last


@pytest.mark.parametrize("b", H.POSE_B[:3], ids=H.POSE_IDS[:3])
def test_pose_host_twin_against_float64(dcl, b):
    """the float64 twin takes the ReLU masks of the forward under test; the fp32 module form is measured with its own"""
    k = H.pose_case(b)
    got = pose_host(dcl, k)
    mod32 = H.pose_form(k, torch.float32)
    H.compare("b%d" % b, got, H.pose_form(k, torch.float64, H.pose_masks(got["h1"], got["h2"])), mod32,
              H.pose_form(k, torch.float64, mod32["masks"]), H.POSE_OUT)


@pytest.mark.parametrize("b", H.POSE_B, ids=H.POSE_IDS)
def test_pose_host_twin_is_exact_on_exact_operands(dcl, b):
    k = H.pose_case(b, exact=True)
    got, ref = pose_host(dcl, k), H.pose_form(k, torch.float64)
    assert float(ref["dx"].abs().max()) > 0 and float(ref["d_rW0"].abs().max()) > 0
    for name in H.POSE_OUT:
        assert bool((got[name].double() == ref[name]).all()), (name, float((got[name].double() - ref[name]).abs().max()))


def test_a_crop_gives_the_same_bits_alone_as_inside_a_batch_on_the_pose_host_twin(dcl):
    k = H.pose_case(3)
    full = pose_host(dcl, k)
    for c in range(3):
        alone = pose_host(dcl, H.pose_crop(k, c))
        for name in ("o9", "t3", "dx"):
            assert H.same_bits(alone[name], full[name][c:c + 1]), (c, name)


def test_selective_outputs_equal_the_full_call_on_the_pose_host_twin(dcl):
    k = H.pose_case(3)
    full = pose_host(dcl, k)
    P = H.pose_params(k)
    back = dcl.ops.pose_heads_train_backward_host
    dx, grads = back(k["x"], P, full["h1"], full["h2"], k["g_o9"], k["g_t3"], need_params=False)
    assert grads == [None] * 12 and H.same_bits(dx, full["dx"])
    need = tuple(n in ("rW2", "tb1", "tW0") for n in H.PARAMS)
    dx, grads = back(k["x"], P, full["h1"], full["h2"], k["g_o9"], k["g_t3"], need_x=False, need_params=need)
    assert dx is None
    for n, g, want in zip(H.PARAMS, grads, need):
        assert (g is not None) == want and (g is None or H.same_bits(g, full["d_" + n])), n
    # one head's gradient alone: a missing one is a zero gradient
    zero = torch.zeros_like(k["g_t3"])
    a = back(k["x"], P, full["h1"], full["h2"], k["g_o9"], None)
    z = back(k["x"], P, full["h1"], full["h2"], k["g_o9"], zero)
    assert H.same_bits(a[0], z[0]) and all(H.same_bits(u, v) for u, v in zip(a[1], z[1]))
    assert float(a[1][6].abs().max()) == 0 and float(a[1][0].abs().max()) > 0
