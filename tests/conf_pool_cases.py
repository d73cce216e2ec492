"""Shapes, operands and references of the channel-major confidence pooling tests (csrc/conf_pool_grad.hip), shared by
tests/test_conf_pool_grad_abi.py (CPU: the host twins) and tests/test_gpu_conf_pool_grad.py (the kernels).  Everything here is
built on the CPU, once per shape, and handed out unchanged."""
import functools

import torch

# (b, C, n1, n2)
SHAPES = [
    (1, 1, 1, 1),
    (2, 3, 5, 7),                 # everything odd: unaligned rows, tails only
    (3, 130, 257, 64),            # one past a 256-wide block, two past a 128-channel boundary, one aligned direction
    (2, 1024, 1024, 1024),        # the network's own shape on two crops
    (1, 1024, 12288, 2048),       # the stress crop: > 4096 logits (the 1024-thread softmax), many tiles
    (1, 300, 9, 6),               # beyond the five the feature was specified with: a short last chunk of channels (256 + 44)
]
IDS = ["x".join(str(v) for v in s) for s in SHAPES]
OUTPUTS = ("pooled", "dlogit1", "dlogit2", "dF1", "dF2")


@functools.lru_cache(maxsize=None)
def random_case(i):
    """logits (b,1,n), F, the upstream gradients, and conf / w from torch's fp32 sigmoid / softmax; CPU tensors"""
    b, c, n1, n2 = SHAPES[i]
    g = torch.Generator().manual_seed(100 + i)
    r = lambda *s: torch.randn(*s, generator=g)                                              # noqa: E731
    k = dict(logit1=r(b, 1, n1) * 2, logit2=r(b, 1, n2) * 2, F1=r(b, c, n1).relu_() * 1.5, F2=r(b, c, n2).relu_() * 1.5,
             g_pooled=r(b, c) * 0.1, g_conf=r(b, n1 + n2) * 0.01)
    k["conf"] = torch.sigmoid(torch.cat([k["logit1"], k["logit2"]], dim=2)).squeeze(1).contiguous()
    k["w"] = torch.softmax(k["conf"], dim=1)
    return k


@functools.lru_cache(maxsize=None)
def exact_case(i):
    """operands on which every sum of the formulas is exact in fp32: w and the gradients are powers of two (signed for the
    gradients), F holds small integers, s = 0.5.  w is not normalised: the routines take it as given."""
    b, c, n1, n2 = SHAPES[i]
    L = n1 + n2
    g = torch.Generator().manual_seed(200 + i)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g)                        # noqa: E731
    sign = lambda *s: (ri(0, 1, *s) * 2 - 1).float()                                         # noqa: E731
    return dict(conf=torch.full((b, L), 0.5), w=torch.pow(2.0, -ri(8, 9, b, L).float()),
                F1=ri(-4, 4, b, c, n1).float(), F2=ri(-4, 4, b, c, n2).float(),
                g_pooled=sign(b, c) * torch.pow(2.0, -ri(3, 4, b, c).float()),
                g_conf=sign(b, L) * torch.pow(2.0, -ri(0, 4, b, L).float()))


def formulas64(conf, w, F1, F2, g_pooled, g_conf=None):
    """the issue's formulas in float64, conf and w taken as given"""
    s, w, g = conf.double(), w.double(), g_pooled.double()
    F = torch.cat([F1.double(), F2.double()], dim=2)
    n1 = F1.shape[2]
    pooled = (F * w[:, None, :]).sum(dim=2)
    d = (g[:, :, None] * F).sum(dim=1)
    dot = (w * d).sum(dim=1, keepdim=True)
    ds = w * (d - dot) + (0.0 if g_conf is None else g_conf.double())
    dl = ds * s * (1.0 - s)
    dF = g[:, :, None] * w[:, None, :]
    return dict(pooled=pooled, dlogit1=dl[:, :n1], dlogit2=dl[:, n1:], dF1=dF[:, :, :n1], dF2=dF[:, :, n1:])


def module_form(logit1, logit2, F1, F2, g_conf, g_pooled):
    """the four lines of Network._forward_compat with autograd, in the dtype and on the device of the operands"""
    l1, l2, F1, F2 = (t.detach().clone().requires_grad_(True) for t in (logit1, logit2, F1, F2))
    conf = torch.sigmoid(torch.cat([l1, l2], dim=2))
    conf_softmax = torch.softmax(conf, dim=2)
    F_p = torch.cat([F1, F2], dim=2)
    F_p_wei = torch.sum(F_p * conf_softmax, dim=2, keepdim=True)
    torch.autograd.backward([conf, F_p_wei], [g_conf.unsqueeze(1), g_pooled.unsqueeze(2)])
    return dict(conf=conf.detach().squeeze(1), pooled=F_p_wei.detach().squeeze(2), dlogit1=l1.grad.squeeze(1),
                dlogit2=l2.grad.squeeze(1), dF1=F1.grad, dF2=F2.grad)


@functools.lru_cache(maxsize=None)
def module_refs(i):
    """(float64, fp32) module compositions of random_case(i) on the CPU"""
    k = random_case(i)
    names = ("logit1", "logit2", "F1", "F2", "g_conf", "g_pooled")
    return module_form(*(k[n].double() for n in names)), module_form(*(k[n] for n in names))


def compare(tag, got, ref64, module, names):
    """the project's rule (tests/test_gpu_objective.py::_compare): err <= max(2 err_module, 1e-6 max|ref64|) per output"""
    for name in names:
        r = ref64[name]
        e = float((got[name].detach().cpu().double() - r).abs().max())
        em = float((module[name].detach().cpu().double() - r).abs().max())
        print("%s %-8s max|ref| %.3g  err %.3g  module %.3g" % (tag, name, float(r.abs().max()), e, em))
        assert e <= max(2 * em, 1e-6 * float(r.abs().max())), (tag, name, e, em)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())
