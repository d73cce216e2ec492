"""The point-major confidence pooling and its gradient on the GPU (csrc/conf_pool_pm.hip): the kernels against their host
twins bit for bit, exact operands against float64, autograd.ConfPoolPmFn against the module composition and a float64 twin
under the project's rule, determinism, a crop alone, selective gradients and non-contiguous inputs.
tests/conf_pool_pm_cases.py holds the shapes, the operands and the CPU references, built once."""
import pytest
import torch

import conf_pool_pm_cases as PM

pytestmark = pytest.mark.gpu

_IN = ("conf", "w", "F1", "F2", "g_pooled", "g_conf")


def _dev(k, names=_IN):
    return {n: k[n].cuda() for n in names}


def _kernels(dcl, d, g_conf, **need):
    out = {"pooled": dcl.ops.conf_pool_pm(d["w"], d["F1"], d["F2"])}
    got = dcl.ops.conf_pool_pm_backward(d["conf"], d["w"], d["F1"], d["F2"], d["g_pooled"], g_conf, **need)
    out.update(zip(("dlogit1", "dlogit2", "dF1", "dF2"), got))
    return out


def _host(dcl, k, g_conf):
    out = {"pooled": dcl.ops.conf_pool_pm_host(k["w"], k["F1"], k["F2"])}
    got = dcl.ops.conf_pool_pm_backward_host(k["conf"], k["w"], k["F1"], k["F2"], k["g_pooled"], g_conf)
    out.update(zip(("dlogit1", "dlogit2", "dF1", "dF2"), got))
    return out


@pytest.mark.parametrize("with_g_conf", [True, False], ids=["g_conf", "no_g_conf"])
@pytest.mark.parametrize("i", range(len(PM.SHAPES)), ids=PM.IDS)
def test_kernels_equal_their_host_twins_bit_for_bit(dcl, i, with_g_conf):
    k = PM.random_case(i)
    d = _dev(k)
    got = _kernels(dcl, d, d["g_conf"] if with_g_conf else None)
    want = _host(dcl, k, k["g_conf"] if with_g_conf else None)
    for name in PM.OUTPUTS:
        assert PM.same_bits(got[name], want[name]), (PM.IDS[i], name, float((got[name].cpu() - want[name]).abs().max()))


def test_float_by_float_accesses_give_the_bits_of_16_byte_ones(dcl):
    """the same operands one float off a 16-byte boundary take the scalar paths: the pinned orders do not notice"""
    k = PM.random_case(2)
    d = _dev(k)
    want = _kernels(dcl, d, d["g_conf"])
    off = {}
    for n in _IN:
        buf = torch.empty(d[n].numel() + 1, dtype=torch.float32, device="cuda")
        off[n] = buf[1:].view(d[n].shape).copy_(d[n])
        assert off[n].data_ptr() % 16 == 4 and off[n].is_contiguous()
    got = _kernels(dcl, off, off["g_conf"])
    for name in PM.OUTPUTS:
        assert PM.same_bits(got[name], want[name]), name


@pytest.mark.parametrize("i", [1, 2, 3, 4, 5, 6], ids=PM.IDS[1:])
def test_exact_operands_equal_float64_on_the_device(dcl, i):
    k = PM.exact_case(i)
    d = _dev(k)
    ref = PM.formulas64(k, k["g_conf"])
    got = _kernels(dcl, d, d["g_conf"])
    for name in PM.OUTPUTS:
        assert bool((got[name].cpu().double() == ref[name]).all()), (PM.IDS[i], name)


def _fn(dcl, k, logits=True, F=True, g_conf=True, g_pooled=True):
    """one ConfPoolPmFn forward + backward on the device -> outputs and the gradients that were asked for"""
    l1, l2 = (k[n].cuda().requires_grad_(logits) for n in ("logit1", "logit2"))
    F1, F2 = (k[n].cuda().requires_grad_(F) for n in ("F1", "F2"))
    conf, pooled = dcl.autograd.ConfPoolPmFn.apply(l1, l2, F1, F2)
    outs, grads = [], []
    if g_conf:
        outs.append(conf), grads.append(k["g_conf"].cuda())
    if g_pooled:
        outs.append(pooled), grads.append(k["g_pooled"].cuda())
    torch.autograd.backward(outs, grads)
    return dict(conf=conf.detach(), pooled=pooled.detach(), dlogit1=l1.grad, dlogit2=l2.grad, dF1=F1.grad, dF2=F2.grad)


@pytest.mark.parametrize("i", [1, 2, 3, 4], ids=PM.IDS[1:5])
def test_conf_pool_pm_fn_against_the_module_composition_and_float64(dcl, i):
    k = PM.random_case(i)
    ref64, mod32 = PM.module_refs(i)
    got = _fn(dcl, k)
    PM.compare(PM.IDS[i], got, ref64, mod32, ("conf",) + PM.OUTPUTS)
    b = k["w"].shape[0]
    conf, _, _ = dcl.ops.conf_softmax(b, k["logit1"].cuda().reshape(-1), k["logit2"].cuda().reshape(-1))
    assert PM.same_bits(got["conf"], conf)                                    # the train-mode conf is the eval kernel's


def test_the_same_call_twice_gives_the_same_bits(dcl):
    k = PM.random_case(4)
    a, b = _fn(dcl, k), _fn(dcl, k)
    for name in ("conf",) + PM.OUTPUTS:
        assert PM.same_bits(a[name], b[name]), name


@pytest.mark.parametrize("i", [2, 3], ids=PM.IDS[2:4])
def test_a_crop_gives_the_same_bits_alone_as_inside_a_batch(dcl, i):
    k = PM.random_case(i)
    full = _kernels(dcl, _dev(k), k["g_conf"].cuda())
    b, _, n1, n2 = PM.SHAPES[i]
    for c in range(b):
        one = _dev(PM.crop(k, c, _IN))
        alone = _kernels(dcl, one, one["g_conf"])
        for name in PM.OUTPUTS:
            per = {"dF1": n1, "dF2": n2}.get(name, 1)
            assert PM.same_bits(alone[name], full[name][c * per:(c + 1) * per]), (c, name)


def test_selective_gradients(dcl):
    k = PM.random_case(2)
    full = _fn(dcl, k)
    no_F = _fn(dcl, k, F=False)
    assert no_F["dF1"] is None and no_F["dF2"] is None
    assert PM.same_bits(no_F["dlogit1"], full["dlogit1"]) and PM.same_bits(no_F["dlogit2"], full["dlogit2"])
    no_l = _fn(dcl, k, logits=False)
    assert no_l["dlogit1"] is None and no_l["dlogit2"] is None
    assert PM.same_bits(no_l["dF1"], full["dF1"]) and PM.same_bits(no_l["dF2"], full["dF2"])
    # pooled unused: d = dot = 0, so ds = g_conf exactly and dlogit = (g_conf * s) * (1 - s) as the header writes it
    unused = _fn(dcl, k, g_pooled=False)
    assert not bool(unused["dF1"].any()) and not bool(unused["dF2"].any())
    s, g, n1 = unused["conf"], k["g_conf"].cuda(), PM.SHAPES[2][2]
    want = (g * s) * (1.0 - s)
    assert PM.same_bits(unused["dlogit1"], want[:, :n1]) and PM.same_bits(unused["dlogit2"], want[:, n1:])


def test_non_contiguous_inputs_are_copied_not_misread(dcl):
    k = PM.random_case(2)
    want = _fn(dcl, k)
    t = dict(k)
    t["F1"] = k["F1"].t().contiguous().t()                                    # the same values behind other strides
    t["F2"] = torch.cat([k["F2"], k["F2"]], dim=1)[:, :k["F2"].shape[1]]      # a column block of a wider matrix
    assert not t["F1"].is_contiguous() and not t["F2"].is_contiguous()
    got = _fn(dcl, t)
    for name in ("conf",) + PM.OUTPUTS:
        assert PM.same_bits(got[name], want[name]), name
    d = _dev(t)
    d["F2"] = torch.cat([d["F2"], d["F2"]], dim=1)[:, :k["F2"].shape[1]]
    assert not d["F1"].is_contiguous() and not d["F2"].is_contiguous()
    assert PM.same_bits(dcl.ops.conf_pool_pm(d["w"], d["F1"], d["F2"]), dcl.ops.conf_pool_pm(*(k[n].cuda() for n in ("w", "F1", "F2"))))
