"""Shapes, operands and float64 twins of the train_heads="kernels" tests (tests/test_heads_abi.py, tests/test_gpu_train_heads.py):
the narrow per-point layer (csrc/linear_narrow.hip) and the two pose heads in training (csrc/pose_heads_grad.hip).  Operands are
built on the CPU, once (lru_cache), and are never modified.

Random cases serve the project's rule against float64 (tests/train_dense_cases.py::compare); EXACT cases hold small integers
chosen so that every partial sum of every chain is an integer below 2^24 -- fp32 in any order then equals float64, and a dropped
or doubled element shows as an inequality.  The builders assert that bound in float64 before a case is used.

The twins are the torch compositions (linear, ReLU) written as functions of a dtype: float64 is the reference, fp32 on the CPU
the module form whose error the rule measures against.  The pose heads' twin takes its ReLU masks from the forward under test
(h > 0 of the stored activations), as tests/train_dense_cases.py does."""
import functools

import torch
import torch.nn.functional as Fn

from train_dense_cases import compare, same_bits  # noqa: F401  (re-exported for the tests)

NARROW_MAX_N, NARROW_ROWS = 16, 64           # include/dclnet_hip.h: DCL_NARROW_MAX_N, DCL_NARROW_ROWS
LIMIT = float(1 << 24)

# (M, K, N): one element; the model's widths with a ragged last chunk; across chunk boundaries; K not a multiple of 4; the widest;
# and more chunks than the finish launch adds in one round (512), so that its second round and its batched adds run
NARROW_SHAPES = [(1, 1, 1), (257, 128, 1), (300, 128, 3), (2 * NARROW_ROWS + 1, 128, 3), (513, 130, 9), (64, 7, NARROW_MAX_N),
                 (512 * NARROW_ROWS + 1, 5, 2)]
NARROW_IDS = ["x".join(str(v) for v in s) for s in NARROW_SHAPES]
NARROW_OUT = ("y", "dx", "dW", "db")
NARROW_FORMS = ("dense", "strided", "misaligned")


def _ints(g, *shape, density=1.0):
    """integers in {-1, 0, 1}; density: the share of entries that may be non-zero"""
    v = torch.randint(-1, 2, shape, generator=g).float()
    if density < 1.0:
        v = v * (torch.rand(*shape, generator=g) < density).float()
    return v


@functools.lru_cache(maxsize=None)
def narrow_case(i, exact=False):
    M, K, N = NARROW_SHAPES[i]
    g = torch.Generator().manual_seed(900 + i + (50 if exact else 0))
    if exact:
        k = dict(x=_ints(g, M, K), W=_ints(g, N, K, 1), bias=_ints(g, N), g=_ints(g, M, N))
        # every partial sum of y, dx, dW, db is an integer bounded by the sum of absolute values: K + 1, N, M, M
        assert max(K + 1, N, M) < LIMIT
        x, W, gg = k["x"].double().abs(), k["W"][:, :, 0].double().abs(), k["g"].double().abs()
        assert float((x @ W.t()).max()) + 1 < LIMIT and float((gg @ W).max()) < LIMIT and float((gg.t() @ x).max()) < LIMIT
        return k
    r = lambda *s: torch.randn(*s, generator=g)                                              # noqa: E731
    return dict(x=r(M, K), W=r(N, K, 1) / K ** 0.5, bias=r(N) * 0.1, g=r(M, N) * 0.1)


def narrow_x(x, form):
    """the same values as a dense matrix, as a column block of a wider one whose pitch is no multiple of 4, or from an address
    off 16-byte alignment"""
    M, K = x.shape
    if form == "dense":
        return x.contiguous()
    if form == "strided":
        pad = 5 if (K + 5) % 4 else 6
        wide = torch.full((M, K + pad), 7.0, dtype=x.dtype, device=x.device)
        wide[:, 3:3 + K] = x
        v = wide[:, 3:3 + K]
        assert v.stride(0) % 4 != 0 and (M == 1 or not v.is_contiguous())
        return v
    buf = torch.full((M * K + 1,), 7.0, dtype=x.dtype, device=x.device)
    buf[1:] = x.reshape(-1)
    v = buf[1:].view(M, K)
    assert v.data_ptr() % 16 != 0
    return v


def narrow_form(k, dtype):
    """Conv1d(kernel 1) with autograd in `dtype`: y, dx, dW (N, K, 1), db"""
    x, W, b = (k[n].detach().to(dtype).clone().requires_grad_(True) for n in ("x", "W", "bias"))
    y = Fn.linear(x, W[:, :, 0], b)
    y.backward(k["g"].to(dtype))
    return dict(y=y.detach(), dx=x.grad, dW=W.grad, db=b.grad)


# ---------------------------------------------------------------------------------------------------- the pose heads
WIDTHS = (1024, 512, 128, 9, 3)              # d0, d1, d2, n_rot, n_trans: the model's
POSE_B = (1, 3, 33, 130)                     # below and above a wave's worth of rows, odd, above the eval path's POSE_HEADS_MAX
POSE_IDS = ["b%d" % b for b in POSE_B]
PARAMS = ("rW0", "rb0", "rW1", "rb1", "rW2", "rb2", "tW0", "tb0", "tW1", "tb1", "tW2", "tb2")
POSE_OUT = ("o9", "t3", "dx") + tuple("d_" + n for n in PARAMS)


def _pose_shapes():
    d0, d1, d2, nr, nt = WIDTHS
    out = {}
    for h, n in (("r", nr), ("t", nt)):
        for l, (o, i) in enumerate(((d1, d0), (d2, d1), (n, d2))):
            out["%sW%d" % (h, l)], out["%sb%d" % (h, l)] = (o, i, 1), (o,)
    return out


@functools.lru_cache(maxsize=None)
def pose_case(b, exact=False):
    d0, d1, d2, nr, nt = WIDTHS
    g = torch.Generator().manual_seed(700 + b + (50 if exact else 0))
    k = {}
    for name, shape in _pose_shapes().items():
        if exact:                                   # sparse rows: about 8 non-zero weights per output
            k[name] = _ints(g, *shape, density=12.0 / shape[1]) if len(shape) == 3 else _ints(g, *shape)
        else:
            k[name] = torch.randn(*shape, generator=g) * (1.0 / shape[1] ** 0.5 if len(shape) == 3 else 0.1)
    if exact:
        k.update(x=_ints(g, b, d0), g_o9=_ints(g, b, nr), g_t3=_ints(g, b, nt))
        _assert_exact(k)
    else:
        k.update(x=torch.randn(b, d0, generator=g), g_o9=torch.randn(b, nr, generator=g), g_t3=torch.randn(b, nt, generator=g))
    return k


def _assert_exact(k):
    """bounds every partial sum of the forward and the backward by the same sums over absolute values, in float64"""
    A = {n: v.double().abs().flatten(1) if v.dim() == 3 else v.double().abs() for n, v in k.items()}
    x = A["x"]
    dx = 0
    for h, g in (("r", A["g_o9"]), ("t", A["g_t3"])):
        h1 = x @ A[h + "W0"].t() + A[h + "b0"]
        h2 = h1 @ A[h + "W1"].t() + A[h + "b1"]
        out = h2 @ A[h + "W2"].t() + A[h + "b2"]
        dz2 = g @ A[h + "W2"]
        dz1 = dz2 @ A[h + "W1"]
        dx = dx + dz1 @ A[h + "W0"]
        sums = [h1, h2, out, dz2, dz1, dx, g.t() @ h2, dz2.t() @ h1, dz1.t() @ x, g.sum(0), dz2.sum(0), dz1.sum(0)]
        assert max(float(s.max()) for s in sums) < LIMIT, max(float(s.max()) for s in sums)


def pose_params(k):
    return [k[n] for n in PARAMS]


def pose_masks(h1, h2):
    """the ReLU masks of a forward under test from its stored activations h1 (2, b, d1), h2 (2, b, d2)"""
    return [(h1[0] > 0).cpu(), (h2[0] > 0).cpu(), (h1[1] > 0).cpu(), (h2[1] > 0).cpu()]


def pose_form(k, dtype, masks=None):
    """both heads as Conv1d -> ReLU -> Conv1d -> ReLU -> Conv1d with autograd in `dtype`; masks: [rot h1, rot h2, trans h1,
    trans h2] > 0 of the forward under test, or None (the form's own).  -> POSE_OUT and "masks" (its own)"""
    L = {n: k[n].detach().to(dtype).clone().requires_grad_(True) for n in PARAMS + ("x",)}
    own, outs = [], []
    for hi, h in enumerate("rt"):
        y = L["x"]
        for l in (0, 1):
            y = Fn.linear(y, L["%sW%d" % (h, l)][:, :, 0], L["%sb%d" % (h, l)])
            own.append((y > 0).detach())
            m = own[-1] if masks is None else masks[2 * hi + l]
            y = torch.where(m, y, torch.zeros_like(y))
        outs.append(Fn.linear(y, L[h + "W2"][:, :, 0], L[h + "b2"]))
    torch.autograd.backward(outs, [k["g_o9"].to(dtype), k["g_t3"].to(dtype)])
    res = {"o9": outs[0].detach(), "t3": outs[1].detach(), "dx": L["x"].grad, "masks": own}
    res.update({"d_" + n: L[n].grad for n in PARAMS})
    return res


def pose_crop(k, c):
    """crop c of a case alone"""
    one = dict(k)
    for n in ("x", "g_o9", "g_t3"):
        one[n] = k[n][c:c + 1].contiguous()
    return one
