"""Inputs and float64 references for the rotation head's gradient (tests/test_rotation_grad_abi.py on the host twin,
tests/test_gpu_rotation_grad.py on the kernel).  Everything is made on the CPU from generators with fixed seeds and cached:
a reference is computed once per (class, batch) and shared by the tests that need it."""
import functools
import itertools

import torch

# class -> (seed, bound).  The bound is per crop, relative to that crop's max |reference gradient|.  A closed form evaluated
# in fp64 on the kernel's fp32 normalisation and rounded to fp32 measured <= 7.8e-8 on the noisy-orthonormal classes and
# <= 2.3e-6 on the others against the float64 reference, which normalises in float64: about a tenth of the bounds.
AUTOGRAD_CLASSES = {
    "gaussian": (11, 2e-5),
    "gaussian_scaled": (12, 2e-5),
    "ortho_noise_1e-2": (13, 1e-6),
    "ortho_noise_1e-4": (14, 1e-6),
    "ortho_noise_1e-6": (15, 1e-6),
    "left_handed": (16, 2e-5),
    "third_near_first": (17, 2e-5),
}
EXACT_CLASS = "ortho_exact"          # float64 autograd is NaN there: central differences, bound 1e-5 (their own error ~1e-9)
EXACT_BOUND = 1e-5
ALL_CLASSES = tuple(AUTOGRAD_CLASSES) + (EXACT_CLASS,)


def _rotations(b, g):
    q = torch.linalg.qr(torch.randn(b, 3, 3, generator=g, dtype=torch.float64))[0]
    return q * torch.det(q).view(b, 1, 1)                                  # columns = right-handed orthonormal axes


def _to_o9(axes):
    """(b, 3, 3) with the axes as COLUMNS -> o9 (b, 9) fp32: axis c at [3c, 3c + 3)"""
    return axes.transpose(1, 2).reshape(-1, 9).float().contiguous()


def _exact_axes(b):
    """exactly orthogonal axes with exactly representable entries: the 24 proper signed permutations, and the same applied
    to the integer matrix [[2,-2,1],[2,1,-2],[1,2,2]] (orthogonal columns of length 3), each axis then scaled by 1, 2, 0.5, 3"""
    perms = []
    for p in itertools.permutations(range(3)):
        for sg in itertools.product((1.0, -1.0), repeat=3):
            m = torch.zeros(3, 3, dtype=torch.float64)
            for c in range(3):
                m[p[c], c] = sg[c]
            if torch.det(m) > 0:
                perms.append(m)
    q3 = torch.tensor([[2.0, -2.0, 1.0], [2.0, 1.0, -2.0], [1.0, 2.0, 2.0]], dtype=torch.float64)
    bases = perms + [m @ q3 for m in perms]
    scales = (1.0, 2.0, 0.5, 3.0)
    out = []
    for i in range(b):
        s = torch.tensor([scales[(i + k) % 4] for k in range(3)], dtype=torch.float64)
        out.append(bases[i % len(bases)] * s.view(1, 3))
    return torch.stack(out)


@functools.lru_cache(maxsize=None)
def inputs(cls, b=64):
    """(o9 (b, 9) fp32, G (b, 3, 3) fp32), CPU"""
    seed = 18 if cls == EXACT_CLASS else AUTOGRAD_CLASSES[cls][0]
    g = torch.Generator().manual_seed(1000 * seed + b)
    rn = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float64)          # noqa: E731
    if cls == "gaussian":
        axes = rn(b, 3, 3)
    elif cls == "gaussian_scaled":
        axes = rn(b, 3, 3) * torch.exp2(torch.rand(b, 1, 3, generator=g, dtype=torch.float64) * 40 - 20)
    elif cls in ("ortho_noise_1e-2", "ortho_noise_1e-4"):
        noise = float(cls.rsplit("_", 1)[1])
        scale = 0.5 + 2.5 * torch.rand(b, 1, 3, generator=g, dtype=torch.float64)
        axes = (_rotations(b, g) + noise * rn(b, 3, 3)) * scale
    elif cls == "ortho_noise_1e-6":
        axes = _rotations(b, g) + 1e-6 * rn(b, 3, 3)
    elif cls == "left_handed":
        axes = _rotations(b, g)
        axes[:, :, 2] = -axes[:, :, 2]
        axes = axes + 0.3 * rn(b, 3, 3)
    elif cls == "third_near_first":
        axes = rn(b, 3, 3)
        axes[:, :, 2] = 1.5 * axes[:, :, 0] + 1e-3 * rn(b, 3)
    elif cls == EXACT_CLASS:
        axes = _exact_axes(b)
    else:
        raise KeyError(cls)
    G = torch.randn(b, 3, 3, generator=g).contiguous()
    return _to_o9(axes), G


def forward64(o9):
    """the reference composition (models/DCL_Net.py:15-36 with utils/transform3D.py:6-30) in float64: (b, 9) -> (b, 3, 3)"""
    def nrm(v):
        return v / (torch.sqrt(v.pow(2).sum(1, keepdim=True)) + 1e-8)
    M = torch.stack((nrm(o9[:, :3]), nrm(o9[:, 3:6]), nrm(o9[:, 6:])), dim=2)
    U, S, V = torch.svd(M)
    ones = torch.ones(M.shape[0], dtype=M.dtype)
    sigma = torch.stack([ones, ones, torch.bmm(U, V.transpose(1, 2)).det()], dim=1)
    return U @ torch.diag_embed(sigma) @ V.transpose(1, 2)


@functools.lru_cache(maxsize=None)
def reference(cls, b=64):
    """float64 gradient of sum(G * R) with respect to the fp32 o9 of inputs(cls, b): (b, 9) float64"""
    o9, G = inputs(cls, b)
    if cls == EXACT_CLASS:
        return central_differences(o9, G)
    x = o9.double().requires_grad_(True)
    (forward64(x) * G.double()).sum().backward()
    return x.grad.detach()


def central_differences(o9, G, h=1e-6):
    x = o9.double()
    b = x.shape[0]
    eye = torch.eye(9, dtype=torch.float64) * h
    plus = (x.unsqueeze(1) + eye).reshape(b * 9, 9)
    minus = (x.unsqueeze(1) - eye).reshape(b * 9, 9)
    Gd = G.double().repeat_interleave(9, dim=0)
    lp = (forward64(plus) * Gd).sum(dim=(1, 2))
    lm = (forward64(minus) * Gd).sum(dim=(1, 2))
    return ((lp - lm) / (2 * h)).reshape(b, 9)


def bound(cls):
    return EXACT_BOUND if cls == EXACT_CLASS else AUTOGRAD_CLASSES[cls][1]


def worst_ratio(got, cls, b=64):
    """largest per-crop max|got - ref| / max|ref| over the batch (no crop left out); NaN if anything is not finite"""
    ref = reference(cls, b)
    assert torch.isfinite(ref).all(), "the float64 reference of class %s is not finite: pick another seed" % cls
    err = (got.double() - ref).abs().amax(dim=1) / ref.abs().amax(dim=1)
    return float(err.max()) if torch.isfinite(got).all() else float("nan")
