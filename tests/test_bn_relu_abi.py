"""The sparse-conv BatchNorm + ReLU entry points (dcl_bn_relu_ws_bytes / _fwd / _bwd and the two host twins) are declared with
the documented argument lists, exported by both libraries and answer bad arguments and an empty matrix without a GPU; Network
takes the `train_norm=` switch, defaults to the module composition and keeps its state_dict keys; the host twins -- the kernels'
routines in the kernels' summation order -- agree with float64 under the project's rule (the backward with the twin's own
mask) and are exact on exact operands."""
import ctypes as C
import os
import re

import pytest
import torch

import bn_relu_cases as BN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_DIMS = ["int64_t rows", "int c"]
_IN = ["const float *x", "const float *gamma", "const float *beta"]
_FWD = _IN + ["float eps", "float momentum", "float *running_mean", "float *running_var", "float *mean", "float *invstd",
              "float *z", "int relu"]
_BWD = _IN + ["const float *mean", "const float *invstd", "const float *g", "int relu", "float *dx", "float *dgamma",
              "float *dbeta"]
_WS = ["void *ws", "int64_t ws_bytes", "dclStream_t stream"]

WANT = {
    "dcl_bn_relu_ws_bytes": _DIMS + ["int64_t *bytes_host"],
    "dcl_bn_relu_fwd": _DIMS + _FWD + _WS,
    "dcl_bn_relu_bwd": _DIMS + _BWD + _WS,
    "dcl_bn_relu_fwd_host": _DIMS + _FWD,
    "dcl_bn_relu_bwd_host": _DIMS + _BWD,
}


def declarations():
    text = open(os.path.join(ROOT, "include", "dclnet_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for m in re.finditer(r"\bint\s+(dcl_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        out[m.group(1)] = [re.sub(r"\s+", " ", a).strip() for a in m.group(2).split(",")]
    return out


def test_header_declares_the_five_entry_points_and_keeps_the_abi_version():
    decl = declarations()
    for name, args in WANT.items():
        assert name in decl, name
        assert decl[name] == args, (name, decl[name])
    text = open(os.path.join(ROOT, "include", "dclnet_hip.h")).read()
    assert re.search(r"#define DCL_ABI_VERSION 2\b", text)
    section = text[text.index("sparse-conv BatchNorm + ReLU"):text.index("optimizer step ---")]
    assert "PINNED ORDER" in section and "DCL_BN_ROWS" in section and "float64" in section and "ascending" in section
    assert re.search(r"#define DCL_BN_ROWS \d+", section)


def _libs(dcl):
    assert os.path.exists(dcl._native.DIAG_SO_PATH), "diagnostic library missing: build() makes it"
    return [("product", dcl._native.lib()), ("diag", dcl._native._open(dcl._native.DIAG_SO_PATH))]


def test_both_libraries_export_them_and_the_python_layers_exist(dcl):
    for tag, lib in _libs(dcl):
        for name in WANT:
            assert hasattr(lib, name), (tag, name)
        assert int(lib.dcl_abi_version()) == 2 == dcl._native.ABI_VERSION, tag
    for fn in ("bn_relu", "bn_relu_backward"):
        assert callable(getattr(dcl.ops, fn)) and callable(getattr(dcl.ops, fn + "_host")), fn
    assert callable(dcl.ops.check_train_norm) and dcl.ops.BN_ROWS == BN.R
    assert hasattr(dcl.autograd.BnReluFn, "apply")
    assert dcl.DCL_Net.TRAIN_NORM_MODES == ("modules", "fused")
    assert dcl.Modules.BasicBlock_SPCONV.norm_form == "modules"


_BUF = (C.c_char * 64)()                 # host bytes standing in for buffers: a rejected call never dereferences them
_P = C.cast(_BUF, C.c_void_p)


def _call(lib, name, **over):
    """one call with every pointer set, an ample ws_bytes, and `over` applied on top"""
    vals = {"rows": 300, "c": 5, "eps": 1e-5, "momentum": 0.1, "relu": 1, "ws_bytes": 1 << 20,
            "bytes_host": C.pointer(C.c_int64(0))}
    vals.update(over)
    args = []
    for a in WANT[name]:
        key = a.split("*")[-1].split()[-1]
        args.append(vals[key] if key in vals else (None if key == "stream" else _P))
    return getattr(lib, name)(*args)


_NEED = 2 * 2 * 5 * 8 + 2 * 5 * 4        # 300 rows are two chunks: 2 x (2 x 5) float64 partials, then mb and mg
BAD = []
for _n in WANT:
    BAD += [(_n, dict(rows=-1)), (_n, dict(rows=1)), (_n, dict(c=0)), (_n, dict(c=-4))]
for _n in ("dcl_bn_relu_fwd", "dcl_bn_relu_fwd_host"):
    BAD += [(_n, {k: None}) for k in ("x", "gamma", "beta", "mean", "invstd", "z")]
    BAD += [(_n, dict(running_mean=None)), (_n, dict(running_var=None))]                 # half a pair
    BAD += [(_n, dict(eps=-1e-5)), (_n, dict(eps=float("nan"))), (_n, dict(momentum=-0.1)), (_n, dict(momentum=1.5)),
            (_n, dict(relu=2))]
for _n in ("dcl_bn_relu_bwd", "dcl_bn_relu_bwd_host"):
    BAD += [(_n, {k: None}) for k in ("x", "gamma", "beta", "mean", "invstd", "g")]
    BAD += [(_n, dict(dgamma=None)), (_n, dict(dbeta=None)), (_n, dict(dx=None, dgamma=None, dbeta=None)), (_n, dict(relu=-1))]
BAD += [("dcl_bn_relu_ws_bytes", dict(bytes_host=None))]
for _n in ("dcl_bn_relu_fwd", "dcl_bn_relu_bwd"):
    BAD += [(_n, dict(ws=None)), (_n, dict(ws_bytes=0)), (_n, dict(ws_bytes=_NEED - 1))]


def _bad_id(n, o):
    return "%s-%s" % (n[12:], "-".join("%s=%s" % (k, o[k]) for k in sorted(o)))


@pytest.mark.parametrize("name,over", BAD, ids=[_bad_id(n, o) for n, o in BAD])
def test_bad_arguments_return_einval_without_a_gpu(dcl, name, over):
    for tag, lib in _libs(dcl):
        assert _call(lib, name, **dict(over)) == -1, tag
        assert b"invalid argument" in lib.dcl_last_error(), tag


def test_an_empty_matrix_is_not_an_error_and_the_scratch_query_answers(dcl):
    for tag, lib in _libs(dcl):
        for name in WANT:
            assert _call(lib, name, rows=0) == 0, (tag, name)
        q = C.c_int64(-1)
        assert _call(lib, "dcl_bn_relu_ws_bytes", bytes_host=C.pointer(q)) == 0 and q.value == _NEED, tag
        assert _call(lib, "dcl_bn_relu_ws_bytes", rows=BN.R, c=64, bytes_host=C.pointer(q)) == 0
        assert q.value == 1 * 2 * 64 * 8 + 2 * 64 * 4, tag
        assert _call(lib, "dcl_bn_relu_ws_bytes", rows=171887, c=32, bytes_host=C.pointer(q)) == 0
        assert q.value == -(-171887 // BN.R) * 2 * 32 * 8 + 2 * 32 * 4, tag
        assert _call(lib, "dcl_bn_relu_ws_bytes", rows=0, bytes_host=C.pointer(q)) == 0 and q.value == 0, tag
        # both optional pairs left out are fine for the argument checks: the calls below end at the empty matrix
        assert _call(lib, "dcl_bn_relu_fwd_host", rows=0, running_mean=None, running_var=None) == 0, tag


def test_network_takes_the_train_norm_switch_and_keeps_its_state_dict(dcl):
    cfg = dcl.synth.default_cfg(64, 64)
    plain = dcl.DCL_Net.Network(cfg)
    assert plain.train_norm == "modules"
    fused = dcl.DCL_Net.Network(cfg, train_norm="fused")
    assert fused.train_norm == "fused"
    with pytest.raises(ValueError, match="train_norm"):
        dcl.DCL_Net.Network(cfg, train_norm="x")
    with pytest.raises(ValueError, match="train_norm"):
        dcl.ops.check_train_norm(None)
    blocks = lambda net: [m for bb in (net.backbone_inp, net.backbone_tmp) for m in bb.modules()           # noqa: E731
                          if isinstance(m, dcl.Modules.BasicBlock_SPCONV)]
    assert len(blocks(fused)) == 16 and all(m.norm_form == "fused" for m in blocks(fused))
    assert all(m.norm_form == "modules" for m in blocks(plain))
    assert all(m._fused_norm() is m.layers[1] for m in blocks(fused))
    assert list(fused.state_dict().keys()) == list(plain.state_dict().keys())
    text = open(os.path.join(ROOT, "tools", "train_step.py")).read()
    assert "--norm" in text and "train_norm=args.norm" in text


def test_bn_relu_fn_and_the_ops_refuse_cpu_tensors_with_a_clear_error(dcl):
    k = BN.random_case(0, "conv")
    with pytest.raises(RuntimeError, match=r"GPU only.*'modules'"):
        dcl.autograd.BnReluFn.apply(k["x"], k["gamma"], k["beta"], None, None, 0.1, 1e-5)
    with pytest.raises(RuntimeError, match="GPU"):
        dcl.ops.bn_relu(k["x"], k["gamma"], k["beta"])
    with pytest.raises(RuntimeError, match="GPU"):
        dcl.ops.bn_relu_backward(k["x"], k["gamma"], k["beta"], k["gamma"], k["gamma"], k["g"])


def test_one_row_raises_as_torch_does_and_no_row_is_a_no_op(dcl):
    with pytest.raises(ValueError, match="more than 1"):
        dcl.ops.bn_relu_host(torch.ones(1, 4), torch.ones(4), torch.zeros(4))
    rm, rv = torch.full((4,), 0.5), torch.full((4,), 2.0)
    z, mean, invstd = dcl.ops.bn_relu_host(torch.ones(0, 4), torch.ones(4), torch.zeros(4), rm, rv)
    assert tuple(z.shape) == (0, 4) and bool((rm == 0.5).all()) and bool((rv == 2.0).all())


def test_the_formulas_agree_with_torchs_float64_module():
    """the reference itself: formulas64 is nn.BatchNorm1d -> nn.ReLU in float64, forward and backward, to rounding"""
    for kind in BN.KINDS:
        k = BN.random_case(4, kind)
        ref, mod = BN.case_formulas64(k), BN.module_refs(4, kind)[0]
        for name in BN.FWD[:1] + BN.FWD[3:] + BN.BWD:
            scale = float(ref[name].abs().max())
            assert float((ref[name] - mod[name]).abs().max()) <= 1e-9 * scale, (kind, name)


def host_run(dcl, k, relu=True, eps=BN.EPS, momentum=BN.MOMENTUM, **need):
    """one forward + backward of the host twins -> every output, the running statistics updated on clones"""
    rm, rv = k["running_mean"].clone(), k["running_var"].clone()
    z, mean, invstd = dcl.ops.bn_relu_host(k["x"], k["gamma"], k["beta"], rm, rv, momentum, eps, relu)
    dx, dgamma, dbeta = dcl.ops.bn_relu_backward_host(k["x"], k["gamma"], k["beta"], mean, invstd, k["g"], relu, **need)
    return dict(z=z, mean=mean, invstd=invstd, running_mean=rm, running_var=rv, dx=dx, dgamma=dgamma, dbeta=dbeta)


@pytest.mark.parametrize("kind", BN.KINDS)
@pytest.mark.parametrize("i", BN.SMALL + [10], ids=[BN.IDS[i] for i in BN.SMALL + [10]])
def test_host_twins_against_float64(dcl, i, kind):
    k = BN.random_case(i, kind)
    got = host_run(dcl, k)
    _, m32, m32_ref = BN.module_refs(i, kind)
    ref = BN.case_formulas64(k, mask=got["z"] > 0)                # the backward's reference takes the twin's own mask
    BN.compare("%s %s" % (BN.IDS[i], kind), got, ref, m32, m32_ref, BN.FWD + BN.BWD)
    n = BN.mask_differences(got["z"], ref)
    print("mask differences %d of %d (module: %d)" % (n, got["z"].numel(), BN.mask_differences(m32["z"], ref)))
    assert n <= BN.MASK_CAP * got["z"].numel()


@pytest.mark.parametrize("i", range(len(BN.EXACT_SHAPES)), ids=BN.EXACT_IDS)
def test_the_exact_cases_are_exact_and_the_host_twins_equal_float64_on_them(dcl, i):
    """every sum and quotient is exact, so fp32 in any order equals float64: a dropped or doubled element shows.  First the
    cases themselves: the formulas in fp32 reproduce the float64 ones bit for bit."""
    k = BN.exact_case(i)
    V = k["x"].shape[0]
    args = (k["x"], k["gamma"], k["beta"], k["g"], 0.0, BN.EXACT_MOMENTUM, k["running_mean"], k["running_var"])
    ref, f32 = BN.formulas64(*args), BN.formulas(*args, dtype=torch.float32)
    names = ["z", "mean", "invstd", "running_mean", "dgamma", "dbeta"] + (["dx"] if V == 2048 else [])
    for name in names:
        assert bool((f32[name].double() == ref[name]).all()), ("the case is not exact", name)
    hit = (ref["z"][:, 0] == 0) & (k["g"][:, 0] != 0)
    assert int(hit.sum()) == V // 2 and not bool(ref["dx"][hit, 0].isnan().any())        # y == 0 under a non-zero g
    got = host_run(dcl, k, eps=0.0, momentum=BN.EXACT_MOMENTUM)
    for name in names:
        assert bool((got[name].double() == ref[name]).all()), (BN.EXACT_IDS[i], name, float((got[name].double() - ref[name]).abs().max()))


def test_the_host_twins_honour_need_x_need_affine_and_relu_false(dcl):
    k = BN.random_case(5, "conv")
    full = host_run(dcl, k)
    only_x = host_run(dcl, k, need_affine=False)
    assert only_x["dgamma"] is None and only_x["dbeta"] is None and BN.same_bits(only_x["dx"], full["dx"])
    only_affine = host_run(dcl, k, need_x=False)
    assert only_affine["dx"] is None
    assert BN.same_bits(only_affine["dgamma"], full["dgamma"]) and BN.same_bits(only_affine["dbeta"], full["dbeta"])
    # dx written over g gives the bits of the out-of-place call
    g = k["g"].clone()
    dx, _, _ = dcl.ops.bn_relu_backward_host(k["x"], k["gamma"], k["beta"], full["mean"], full["invstd"], g, out=g)
    assert dx is g and BN.same_bits(g, full["dx"])
    # without the ReLU: z = y, nothing masked; same statistics
    lin = host_run(dcl, k, relu=False)
    ref = BN.case_formulas64(k, relu=False)
    assert BN.same_bits(lin["mean"], full["mean"]) and BN.same_bits(lin["invstd"], full["invstd"])
    assert bool((lin["z"] < 0).any()) and BN.same_bits(torch.where(lin["z"] > 0, lin["z"], torch.zeros(())), full["z"])
    m32 = BN.module_form(k, torch.float32, relu=False)
    BN.compare("no relu", lin, ref, m32, ref, ("z",) + BN.BWD)
