"""Shapes, operands and references of the sparse-conv BatchNorm + ReLU tests (csrc/bn_relu.hip), shared by
tests/test_bn_relu_abi.py (CPU: the host twins) and tests/test_gpu_bn_relu.py (the kernels).  Everything here is built on the
CPU, once per (shape, kind), and handed out unchanged.

The ReLU mask.  Two fp32 forms of y that differ in the last bit disagree about y > 0 for the few elements that land on zero,
and such an element moves dbeta, dgamma and a whole column of dx by a full |g|.  So the float64 reference of a backward takes
the mask of the forward under test (formulas64(..., mask=z_got > 0); the module form is measured against its own mask), and
the mask itself is held to a separate condition: at most MASK_CAP of a case's elements may differ from the float64 mask.
The data keep |mean| / sigma of a channel below ~100: beyond that the fp32 rounding of `mean` dominates every fp32 form."""
import functools
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_rows():
    text = open(os.path.join(ROOT, "include", "dclnet_hip.h")).read()
    return int(re.search(r"#define DCL_BN_ROWS (\d+)", text).group(1))


R = header_rows()                         # DCL_BN_ROWS: the rows per chunk of the sums
# (rows, C)
SHAPES = [
    (2, 16),                              # the fewest rows there are
    (R - 1, 32),                          # one short chunk
    (R, 64),                              # exactly one chunk
    (R + 1, 128),                         # a second chunk of one row
    (3 * R + 7, 256),                     # four chunks, four channel tiles of 16 slots
    (2 * R + 5, 5),                       # rows of 20 bytes: float by float, a short last group, 128 slots
    (R + 3, 24),                          # 16-byte rows whose 6 groups leave lanes idle (42 slots)
    (2048, 16),                           # the exact cases' power of two
    (R + 2, 1028),                        # 17 channel tiles, the last with a single group
    (171887, 32),                         # the training step's largest layers: 672 chunks, finished in batches of 256
    (12930, 256),                         # and its widest
]
IDS = ["x".join(str(v) for v in s) for s in SHAPES]
SMALL = list(range(9))                    # all but the two training-size shapes
KINDS = ("conv", "offset", "const")
EPS, MOMENTUM = 1e-5, 0.1
MASK_CAP = 1e-4
FWD = ("z", "mean", "invstd", "running_mean", "running_var")
BWD = ("dx", "dgamma", "dbeta")


@functools.lru_cache(maxsize=None)
def random_case(i, kind):
    """x, gamma, beta, the upstream gradient g and the running statistics before the step; CPU fp32 tensors.
    conv: per-channel scale 0.05 .. 3, offset within +-2.  offset: mean 5 .. 10, sigma 0.1.  const: conv with an all-zero
    column and a constant one."""
    V, C = SHAPES[i]
    gen = torch.Generator().manual_seed(1000 + 10 * i + KINDS.index(kind))
    rn = lambda *s: torch.randn(*s, generator=gen)                                           # noqa: E731
    ru = lambda *s: torch.rand(*s, generator=gen)                                            # noqa: E731
    if kind == "offset":
        x = rn(V, C) * 0.1 + (5.0 + 5.0 * ru(C))
    else:
        x = rn(V, C) * (0.05 + 2.95 * ru(C)) + (4.0 * ru(C) - 2.0)
    if kind == "const":
        x[:, 0] = 0.0
        x[:, C // 2] = 1.375
    sign = (torch.randint(0, 2, (C,), generator=gen) * 2 - 1).float()
    return dict(x=x.contiguous(), gamma=0.5 + ru(C), beta=sign * (0.05 + 0.5 * ru(C)), g=rn(V, C) * 0.1,
                running_mean=rn(C) * 0.1, running_var=0.5 + ru(C))


EXACT_SHAPES = [(2, 16), (R, 64), (R + 2, 128), (3 * R + 8, 256), (2 * R + 6, 5), (R + 4, 24), (2048, 16), (R + 2, 1028)]
EXACT_IDS = ["x".join(str(v) for v in s) for s in EXACT_SHAPES]
EXACT_MOMENTUM = 0.25


@functools.lru_cache(maxsize=None)
def exact_case(i):
    """operands on which every sum and quotient of the formulas is exact in fp32 (eps = 0): a column holds m + s and m - s
    equally often, s a power of two, m, gamma, beta small dyadics, g small integers.  Then mean = m, var = s^2, xhat = +-1,
    y = beta +- gamma, and the backward's sums are integers; dx is exact when rows is a power of two (2048).  Channel 0 has
    beta = gamma, so half of its y are exactly 0 under a non-zero g: the gradient there is 0."""
    V, C = EXACT_SHAPES[i]
    assert V % 2 == 0
    gen = torch.Generator().manual_seed(2000 + i)
    pick = lambda vals, *s: torch.tensor(vals)[torch.randint(0, len(vals), s, generator=gen)]  # noqa: E731
    m, s = pick([-2.0, -1.0, -0.5, 0.0, 0.5, 1.0, 1.5, 3.0], C), pick([0.25, 0.5, 1.0, 2.0], C)
    up = torch.stack([torch.randperm(V, generator=gen) < V // 2 for _ in range(C)], dim=1)
    x = m + torch.where(up, s, -s)
    gamma, beta = pick([0.5, 0.75, 1.0, 1.5], C), pick([-0.5, -0.25, 0.25, 0.5, 1.0], C)
    beta[0] = gamma[0]
    g = torch.randint(-4, 5, (V, C), generator=gen).float()
    g[:, 0] = g[:, 0].abs() + 1.0
    return dict(x=x.contiguous(), gamma=gamma, beta=beta, g=g, running_mean=pick([-1.0, 0.0, 0.5, 2.0], C),
                running_var=pick([0.5, 1.0, 2.0], C))


def formulas(x, gamma, beta, g, eps, momentum, running_mean, running_var, mask=None, relu=True, dtype=torch.float64):
    """the feature's formulas in `dtype`, nothing rounded in between; mask: the y > 0 the backward is to take (None: its own)"""
    x, gamma, beta, g, rm, rv = (t.to(dtype) for t in (x, gamma, beta, g, running_mean, running_var))
    V = x.shape[0]
    mean = x.sum(0) / V
    var = ((x * x).sum(0) / V - mean * mean).clamp_min(0.0)
    invstd = 1.0 / torch.sqrt(var + eps)
    xhat = (x - mean) * invstd
    y = xhat * gamma + beta
    own = y > 0
    z = torch.where(own, y, torch.zeros_like(y)) if relu else y
    out = dict(z=z, mean=mean, invstd=invstd, mask=own, running_mean=(1 - momentum) * rm + momentum * mean,
               running_var=(1 - momentum) * rv + momentum * (var * V / (V - 1)))
    if relu:
        dy = torch.where(own if mask is None else mask, g, torch.zeros_like(g))
    else:
        dy = g
    s1, s2 = dy.sum(0), (dy * xhat).sum(0)
    out.update(dbeta=s1, dgamma=s2, dx=(gamma * invstd) * ((dy - s1 / V) - xhat * (s2 / V)))
    return out


def formulas64(x, gamma, beta, g, eps, momentum, running_mean, running_var, mask=None, relu=True):
    return formulas(x, gamma, beta, g, eps, momentum, running_mean, running_var, mask, relu, torch.float64)


def case_formulas64(k, mask=None, relu=True, eps=EPS, momentum=MOMENTUM):
    return formulas64(k["x"], k["gamma"], k["beta"], k["g"], eps, momentum, k["running_mean"], k["running_var"], mask, relu)


def module_form(k, dtype, relu=True, eps=EPS, momentum=MOMENTUM):
    """nn.BatchNorm1d -> nn.ReLU in train mode with autograd, in `dtype` on the device of the operands"""
    C = k["x"].shape[1]
    bn = torch.nn.BatchNorm1d(C, eps=eps, momentum=momentum).to(device=k["x"].device, dtype=dtype).train()
    with torch.no_grad():
        bn.weight.copy_(k["gamma"]), bn.bias.copy_(k["beta"])
        bn.running_mean.copy_(k["running_mean"]), bn.running_var.copy_(k["running_var"])
    x = k["x"].detach().to(dtype).clone().requires_grad_(True)
    y = bn(x)
    z = torch.relu(y) if relu else y
    z.backward(k["g"].to(dtype))
    return dict(z=z.detach(), running_mean=bn.running_mean.detach().clone(), running_var=bn.running_var.detach().clone(),
                dx=x.grad, dgamma=bn.weight.grad, dbeta=bn.bias.grad, num_batches_tracked=int(bn.num_batches_tracked))


@functools.lru_cache(maxsize=None)
def module_refs(i, kind):
    """(float64, fp32) module compositions of random_case(i, kind) on the CPU, and the fp32 one's own float64 reference: the
    formulas with the fp32 module's mask"""
    k = random_case(i, kind)
    m64, m32 = module_form(k, torch.float64), module_form(k, torch.float32)
    return m64, m32, case_formulas64(k, mask=m32["z"] > 0)


def mask_differences(z_got, ref64):
    """how many elements of the forward under test have another y > 0 than float64"""
    return int(((z_got.detach().cpu() > 0) != ref64["mask"]).sum())


def compare(tag, got, ref64, module, module_ref64, names):
    """the project's rule (tests/conf_pool_cases.py::compare): err <= max(2 err_module, 1e-6 max|ref64|) per output, each
    form against the float64 reference that has its own mask; an output the module does not have (mean, invstd) has
    err_module = 0"""
    for name in names:
        r = ref64[name]
        e = float((got[name].detach().cpu().double() - r).abs().max())
        em = float((module[name].detach().cpu().double() - module_ref64[name]).abs().max()) if name in module else 0.0
        print("%s %-12s max|ref| %.3g  err %.3g  module %.3g" % (tag, name, float(r.abs().max()), e, em))
        assert e <= max(2 * em, 1e-6 * float(r.abs().max())), (tag, name, e, em)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())
