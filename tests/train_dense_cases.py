"""Shapes, operands and float64 twins of the point-major dense half's tests (tests/test_gpu_train_dense.py): autograd's
PointLinearFn, the BatchNorm without ReLU, one side's disengage stacks and one fuser.  Operands are built on the CPU, once.

The twins are the torch module compositions (linear, train-mode batch_norm, ReLU) written as functions of a dtype, so that the
same lines serve as the float64 reference and, in fp32 on the CPU, as the module form whose error the project's rule measures
against.  ReLU masks: a twin takes every mask from the forward under test (tests/bn_relu_cases.py explains why); the fp32
module form is measured against the float64 twin that has ITS masks.  `Recorder` stands in for an autograd Function in the
model's namespace and keeps each call's arguments and output: the masks of the forward under test are its outputs > 0."""
import functools

import torch
import torch.nn.functional as Fn

EPS, MOMENTUM = 1e-5, 0.1

# PointLinearFn: (M, K, N)
LINEAR_SHAPES = [(300, 480, 1024), (257, 256, 64), (130, 512, 512), (256, 128, 128)]
LINEAR_IDS = ["x".join(str(v) for v in s) for s in LINEAR_SHAPES]


class Recorder:
    def __init__(self, fn):
        self.fn, self.calls = fn, []

    def apply(self, *args):
        out = self.fn.apply(*args)
        self.calls.append((args, out))
        return out


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())


def compare(tag, got, ref64, module, module_ref64, names):
    """the project's rule (tests/conf_pool_cases.py::compare): err <= max(2 err_module, 1e-6 max|ref64|) per output, each
    form against the float64 twin that has its own masks"""
    for name in names:
        r = ref64[name]
        e = float((got[name].detach().cpu().double() - r).abs().max())
        em = float((module[name].detach().cpu().double() - module_ref64[name]).abs().max())
        print("%s %-22s max|ref| %.3g  err %.3g  module %.3g" % (tag, name, float(r.abs().max()), e, em))
        assert e <= max(2 * em, 1e-6 * float(r.abs().max())), (tag, name, e, em)


def _relu(y, masks, own):
    """ReLU with the mask taken from `masks` (an iterator; None: y > 0); own collects y > 0"""
    own.append((y > 0).detach())
    m = own[-1] if masks is None else next(masks).to(y.device)
    return torch.where(m, y, torch.zeros_like(y))


def _bn(x, gamma, beta, rm, rv, stats):
    """train-mode BatchNorm1d on (rows, C); stats collects the updated running statistics"""
    rm, rv = rm.clone(), rv.clone()
    y = Fn.batch_norm(x, rm, rv, gamma, beta, True, MOMENTUM, EPS)
    stats.append((rm, rv))
    return y


def _leaf(t, dtype):
    return t.detach().to(dtype).clone().requires_grad_(True)


# ---------------------------------------------------------------------------------------------------- PointLinearFn
@functools.lru_cache(maxsize=None)
def linear_case(i):
    M, K, N = LINEAR_SHAPES[i]
    g = torch.Generator().manual_seed(500 + i)
    r = lambda *s: torch.randn(*s, generator=g)                                              # noqa: E731
    return dict(x=r(M, K), W=r(N, K, 1) / K ** 0.5, bias=r(N) * 0.1, g=r(M, N) * 0.1)


def linear_form(k, relu, dtype, mask=None):
    """Conv1d(kernel 1) [+ bias -> ReLU] with autograd in `dtype`: y, dx, dW, db (None without the bias) and its own mask"""
    x, W, b = _leaf(k["x"], dtype), _leaf(k["W"], dtype), _leaf(k["bias"], dtype)
    own = []
    y = Fn.linear(x, W[:, :, 0], b if relu else None)
    if relu:
        y = _relu(y, None if mask is None else iter([mask]), own)
    y.backward(k["g"].to(dtype))
    return dict(y=y.detach(), dx=x.grad, dW=W.grad, db=b.grad if relu else None, mask=own[0] if relu else None)


# ---------------------------------------------------------------------------------------------------- disengage stacks
STACKS = ("p1", "m1", "p2", "m2")


def disengage_params(net, side):
    """the four stacks' tensors of one side, detached CPU copies: name -> tensor, names "<stack>.<layer>.<what>" """
    P = {}
    for t in STACKS:
        st = getattr(net, "disengage_%s_%s" % (side, t))
        for l in (0, 1):
            conv, bn = st[l].layers[0], st[l].layers[1]
            P["%s.%d.W" % (t, l)] = conv.weight.detach().cpu().clone()
            for what, v in (("gamma", bn.weight), ("beta", bn.bias), ("rm", bn.running_mean), ("rv", bn.running_var)):
                P["%s.%d.%s" % (t, l, what)] = v.detach().cpu().clone()
    return P


def disengage_form(P, x, g, dtype, masks=None):
    """the four module stacks (Conv -> BatchNorm -> ReLU, twice) on x (M, 480) with autograd in `dtype`; g: stack -> upstream
    gradient; masks: {"first": (M, 1024) in the stacks' order, stack: (M, d)} or None.  -> a flat dict of outputs ("out.p1"),
    "dx", parameter gradients ("p1.0.W"), updated running statistics ("p1.0.rm") and "masks" in the same form"""
    L = {n: _leaf(v, dtype) for n, v in P.items() if n.split(".")[2] in ("W", "gamma", "beta")}
    x = _leaf(x, dtype)
    res, own_first, own = {}, [], {}
    outs = []
    for k, t in enumerate(STACKS):
        stats, o = [], []
        h = _bn(Fn.linear(x, L[t + ".0.W"].flatten(1)), L[t + ".0.gamma"], L[t + ".0.beta"], P[t + ".0.rm"].to(dtype),
                P[t + ".0.rv"].to(dtype), stats)
        h = _relu(h, None if masks is None else iter([masks["first"][:, 256 * k:256 * (k + 1)]]), o)
        y = _bn(Fn.linear(h, L[t + ".1.W"].flatten(1)), L[t + ".1.gamma"], L[t + ".1.beta"], P[t + ".1.rm"].to(dtype),
                P[t + ".1.rv"].to(dtype), stats)
        y = _relu(y, None if masks is None else iter([masks[t]]), o)
        own_first.append(o[0]), own.__setitem__(t, o[1])
        for l in (0, 1):
            res["%s.%d.rm" % (t, l)], res["%s.%d.rv" % (t, l)] = stats[l]
        res["out." + t] = y.detach()
        outs.append(y)
    torch.autograd.backward(outs, [g[t].to(dtype) for t in STACKS])
    res["dx"] = x.grad
    res.update({n: v.grad.reshape(P[n].shape) for n, v in L.items()})
    own["first"] = torch.cat(own_first, dim=1)
    res["masks"] = own
    return res


# ---------------------------------------------------------------------------------------------------- a fuser
def fuser_params(fuser):
    P = {}
    for l in range(3):
        conv, bn = fuser.layers[3 * l], fuser.layers[3 * l + 2]
        for what, v in (("W", conv.weight), ("b", conv.bias), ("gamma", bn.weight), ("beta", bn.bias), ("rm", bn.running_mean),
                        ("rv", bn.running_var)):
            P["%d.%s" % (l, what)] = v.detach().cpu().clone()
    return P


def fuser_form(P, x, g, dtype, masks=None):
    """three times Conv1d -> ReLU -> BatchNorm1d on x (M, 512) with autograd in `dtype`; masks: the three ReLUs' or None"""
    L = {n: _leaf(v, dtype) for n, v in P.items() if n.split(".")[1] in ("W", "b", "gamma", "beta")}
    x = _leaf(x, dtype)
    own, stats = [], []
    it = None if masks is None else iter(masks)
    y = x
    for l in range(3):
        y = _relu(Fn.linear(y, L["%d.W" % l].flatten(1), L["%d.b" % l]), it, own)
        y = _bn(y, L["%d.gamma" % l], L["%d.beta" % l], P["%d.rm" % l].to(dtype), P["%d.rv" % l].to(dtype), stats)
    y.backward(g.to(dtype))
    res = {"out": y.detach(), "dx": x.grad, "masks": own}
    res.update({n: v.grad.reshape(P[n].shape) for n, v in L.items()})
    for l in range(3):
        res["%d.rm" % l], res["%d.rv" % l] = stats[l]
    return res
