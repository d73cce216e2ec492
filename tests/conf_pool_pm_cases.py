"""Shapes, operands and references of the point-major confidence pooling tests (csrc/conf_pool_pm.hip), shared by
tests/test_conf_pool_pm_abi.py (CPU: the host twins) and tests/test_gpu_conf_pool_pm.py (the kernels).  Everything here is
built on the CPU, once per shape, and handed out unchanged.  The operands are drawn channel-major, as tests/conf_pool_cases.py
draws them, so that its float64 formulas and its module composition serve as the references; F1 / F2 and the references' dF1 /
dF2 are then laid out point-major: (b n, C), crop i owning rows i n .. i n + n - 1."""
import functools

import torch

import conf_pool_cases as CP

POOL_PM_ROWS = 64                 # include/dclnet_hip.h: DCL_POOL_PM_ROWS

# (b, C, n1, n2)
SHAPES = [
    (1, 1, 1, 1),
    (2, 3, 5, 7),                 # everything odd: unaligned rows, tails only
    (3, 64, 130, 33),             # one channel tile; 2 chunks + 2 rows, one short chunk
    (2, 260, 513, 1),             # C and the rows straddle vector, tile and chunk tails: 4 x 64 + 4 channels, 8 chunks + 1 row
    (2, 1024, 256, 384),          # the network's width; 4 + 6 whole chunks
    (2, 8, POOL_PM_ROWS + 1, POOL_PM_ROWS - 1),      # one row past a chunk, one row short of one
    (1, 100, 70 * POOL_PM_ROWS + 3, 5),              # beyond the six asked for: more chunks (71 + 1) than one round of 64
]
IDS = ["x".join(str(v) for v in s) for s in SHAPES]
OUTPUTS = CP.OUTPUTS
compare, bits, same_bits = CP.compare, CP.bits, CP.same_bits


def to_pm(F):
    """(b, C, n) channel-major -> (b n, C) point-major, contiguous"""
    return F.transpose(1, 2).reshape(-1, F.shape[1]).contiguous()


def refs_to_pm(ref):
    out = dict(ref)
    out["dF1"], out["dF2"] = to_pm(ref["dF1"]), to_pm(ref["dF2"])
    return out


@functools.lru_cache(maxsize=None)
def random_case(i):
    """logits (b,n), F point-major, the upstream gradients, and conf / w from torch's fp32 sigmoid / softmax; CPU tensors.
    F1cm / F2cm / logit1cm / logit2cm: the same operands as the channel-major references want them."""
    b, c, n1, n2 = SHAPES[i]
    g = torch.Generator().manual_seed(300 + i)
    r = lambda *s: torch.randn(*s, generator=g)                                              # noqa: E731
    k = dict(logit1cm=r(b, 1, n1) * 2, logit2cm=r(b, 1, n2) * 2, F1cm=r(b, c, n1).relu_() * 1.5, F2cm=r(b, c, n2).relu_() * 1.5,
             g_pooled=r(b, c) * 0.1, g_conf=r(b, n1 + n2) * 0.01)
    k["conf"] = torch.sigmoid(torch.cat([k["logit1cm"], k["logit2cm"]], dim=2)).squeeze(1).contiguous()
    k["w"] = torch.softmax(k["conf"], dim=1)
    k["logit1"], k["logit2"] = k["logit1cm"].squeeze(1).contiguous(), k["logit2cm"].squeeze(1).contiguous()
    k["F1"], k["F2"] = to_pm(k["F1cm"]), to_pm(k["F2cm"])
    return k


@functools.lru_cache(maxsize=None)
def exact_case(i):
    """operands on which every sum of the formulas is exact in fp32 (tests/conf_pool_cases.py::exact_case): w and the gradients
    are powers of two, F holds small integers, s = 0.5"""
    b, c, n1, n2 = SHAPES[i]
    L = n1 + n2
    g = torch.Generator().manual_seed(400 + i)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g)                        # noqa: E731
    sign = lambda *s: (ri(0, 1, *s) * 2 - 1).float()                                         # noqa: E731
    k = dict(conf=torch.full((b, L), 0.5), w=torch.pow(2.0, -ri(8, 9, b, L).float()),
             F1cm=ri(-4, 4, b, c, n1).float(), F2cm=ri(-4, 4, b, c, n2).float(),
             g_pooled=sign(b, c) * torch.pow(2.0, -ri(3, 4, b, c).float()),
             g_conf=sign(b, L) * torch.pow(2.0, -ri(0, 4, b, L).float()))
    k["F1"], k["F2"] = to_pm(k["F1cm"]), to_pm(k["F2cm"])
    return k


def formulas64(k, g_conf):
    """the header's formulas in float64, conf and w taken as given; dF point-major"""
    return refs_to_pm(CP.formulas64(k["conf"], k["w"], k["F1cm"], k["F2cm"], k["g_pooled"], g_conf))


@functools.lru_cache(maxsize=None)
def module_refs(i):
    """(float64, fp32) module compositions of random_case(i) on the CPU, dF point-major"""
    k = random_case(i)
    names = ("logit1cm", "logit2cm", "F1cm", "F2cm", "g_conf", "g_pooled")
    return (refs_to_pm(CP.module_form(*(k[n].double() for n in names))), refs_to_pm(CP.module_form(*(k[n] for n in names))))


def crop(k, c, names):
    """crop c of a case alone: rows of the (b, .) operands, row blocks of the point-major ones"""
    b = k["w"].shape[0]
    out = {}
    for n in names:
        t = k[n]
        if n in ("F1", "F2"):
            per = t.shape[0] // b
            out[n] = t[c * per:(c + 1) * per].contiguous()
        else:
            out[n] = t[c:c + 1].contiguous()
    return out
